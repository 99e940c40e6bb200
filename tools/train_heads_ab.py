"""Training step at a smaller width: the split-fp16 attention (default) against the fp32 attention (D3DP_TRAIN_ATTN=f32) in ONE process and
one library, the two settings alternating -- whole step (forward + backward, device events) and the attention profile classes.
usage: train_heads_ab.py [cs ...]   (default 256 128; B = 4, F = 243, dep = 8 as BASELINE configs[4])
The switch is read when a model's context is created (its first step), so each setting gets a model of its own.  Figures:
profiles/train_small_heads.md."""
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from d3dp_amd import D3DP  # noqa: E402
from d3dp_amd.weights import H36M_JOINTS_LEFT as KL, H36M_JOINTS_RIGHT as KR, make_state_dict  # noqa: E402

F, J, B, DEP = 243, 17, 4, 8
ROUNDS, STEPS, WARM = 4, 10, 3
ATTN = ("train_attn_fwd_spatial", "train_attn_fwd_temporal", "train_attn_bwd_q_spatial", "train_attn_bwd_q_temporal",
        "train_attn_bwd_kv_spatial", "train_attn_bwd_kv_temporal")


def main():
    widths = [int(a) for a in sys.argv[1:]] or [256, 128]
    for cs in widths:
        x2 = torch.rand(B, F, J, 2, device="cuda") * 2 - 1
        x3 = torch.randn(B, F, J, 3, device="cuda") * 0.3
        models = {}

        def step(m):
            m.zero_grad(set_to_none=True)
            pr = m(x2, x3)
            loss = torch.mean(torch.norm(pr - x3, dim=-1))
            loss.backward(loss.clone().detach())

        for name in ("x2", "f32"):
            if name == "f32":
                os.environ["D3DP_TRAIN_ATTN"] = "f32"
            else:
                os.environ.pop("D3DP_TRAIN_ATTN", None)
            args = SimpleNamespace(number_of_frames=F, test_time_augmentation=True, timestep=1000, scale=1.0, cs=cs, dep=DEP)
            m = D3DP(args, KL, KR, is_train=True)
            m.load_state_dict(make_state_dict(7, cs, DEP, F), strict=False)
            m = m.cuda().train()
            for _ in range(WARM):                      # (discarded: code objects load, the context and its workspace are made)
                step(m)
            torch.cuda.synchronize()
            models[name] = m
            print(f"cs={cs} {name}: {m.pose_estimator.train_arithmetic()}", flush=True)
        os.environ.pop("D3DP_TRAIN_ATTN", None)
        ms = {k: [] for k in models}
        for _ in range(ROUNDS):
            for name, m in models.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(STEPS):
                    step(m)
                b.record()
                torch.cuda.synchronize()
                ms[name].append(a.elapsed_time(b) / STEPS)
        for name in models:
            print(f"cs={cs} {name}: step (fwd + bwd, B={B} F={F} dep={DEP}) ms per round: " + " ".join(f"{v:.2f}" for v in ms[name]), flush=True)
        prof = {k: {} for k in models}
        for _ in range(2):
            for name, m in models.items():
                pe = m.pose_estimator
                pe.profile_enable(True)
                step(m)                                # (discarded: the first profiled step creates the event pool)
                torch.cuda.synchronize()
                pe.profile_read()
                for _ in range(STEPS):
                    step(m)
                torch.cuda.synchronize()
                for k, (cnt, t) in pe.profile_read().items():
                    c0, t0 = prof[name].get(k, (0, 0.0))
                    prof[name][k] = (c0 + cnt, t0 + t)
                pe.profile_enable(False)
        for name in models:
            n = 2 * STEPS
            tot = sum(prof[name][k][1] for k in ATTN) / n
            print(f"cs={cs} {name}: profiled classes, ms per step (launches per step): "
                  + "; ".join(f"{k} {prof[name][k][1] / n:.3f} ({prof[name][k][0] // n})" for k in ATTN + ("train_operand_pass",))
                  + f"; attention classes summed {tot:.3f}", flush=True)


if __name__ == "__main__":
    main()
