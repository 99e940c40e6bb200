"""Training step at `-cs` 192 / 320 / 384 / 448: the opt-in split-fp16 route (D3DP_TRAIN_IMPL=f16x2) against the fp32 path these widths
train on without it, in ONE process and one library, the two settings alternating -- whole step (forward + backward, device events)
and the per-class profile of the training step; clock and power sampled as bench.py samples them.
usage: train_widths_ab.py [cs ...]   (default 192 320 384 448; B = 4, F = 243, dep = 8 as BASELINE configs[4])
The switch is read when a model's context is created (its first step), so each setting gets a model of its own.  Figures:
profiles/train_widths.md."""
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (GpuTelemetry: shader clock and package power from the card's hwmon files)
from d3dp_amd import D3DP  # noqa: E402
from d3dp_amd.weights import H36M_JOINTS_LEFT as KL, H36M_JOINTS_RIGHT as KR, make_state_dict  # noqa: E402

F, J, B, DEP = 243, 17, 4, 8
ROUNDS, STEPS, WARM = 4, 10, 3


def main():
    widths = [int(a) for a in sys.argv[1:]] or [192, 320, 384, 448]
    for cs in widths:
        x2 = torch.rand(B, F, J, 2, device="cuda") * 2 - 1
        x3 = torch.randn(B, F, J, 3, device="cuda") * 0.3
        models = {}

        def step(m):
            m.zero_grad(set_to_none=True)
            pr = m(x2, x3)
            loss = torch.mean(torch.norm(pr - x3, dim=-1))
            loss.backward(loss.clone().detach())

        for name in ("f16x2", "fp32"):
            if name == "f16x2":
                os.environ["D3DP_TRAIN_IMPL"] = "f16x2"
            else:
                os.environ.pop("D3DP_TRAIN_IMPL", None)
            args = SimpleNamespace(number_of_frames=F, test_time_augmentation=True, timestep=1000, scale=1.0, cs=cs, dep=DEP)
            m = D3DP(args, KL, KR, is_train=True)
            m.load_state_dict(make_state_dict(7, cs, DEP, F), strict=False)
            m = m.cuda().train()
            for _ in range(WARM):                      # (discarded: code objects load, the context and its workspace are made)
                step(m)
            torch.cuda.synchronize()
            print(f"cs={cs} {name}: {m.pose_estimator.train_arithmetic()}", flush=True)
            models[name] = m
        os.environ.pop("D3DP_TRAIN_IMPL", None)
        ms = {k: [] for k in models}
        teles = {k: bench.GpuTelemetry(torch.cuda.current_device()) for k in models}
        for _ in range(ROUNDS):
            for name, m in models.items():
                teles[name].start()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(STEPS):
                    step(m)
                b.record()
                torch.cuda.synchronize()
                teles[name].stop()
                ms[name].append(a.elapsed_time(b) / STEPS)
        for name in models:
            tr = teles[name].report()
            print(f"cs={cs} {name}: step (fwd + bwd, B={B} F={F} dep={DEP}) ms per round: " + " ".join(f"{v:.2f}" for v in ms[name])
                  + f"; spread {(max(ms[name]) - min(ms[name])) / min(ms[name]) * 100:.1f} %; clock {tr['clock_mhz_mean']} MHz, power "
                  f"{tr['power_w_mean']} W (cap {tr['power_cap_w']} W) over its timed rounds", flush=True)
        lo, hi = min(ms["fp32"]) / max(ms["f16x2"]), max(ms["fp32"]) / min(ms["f16x2"])
        print(f"cs={cs}: fp32 / f16x2 step time between {lo:.2f} and {hi:.2f} over the rounds", flush=True)
        for name, m in models.items():
            pe = m.pose_estimator
            pe.profile_enable(True)
            step(m)                                    # (discarded: the first profiled step creates the event pool)
            torch.cuda.synchronize()
            pe.profile_read()
            for _ in range(STEPS):
                step(m)
            torch.cuda.synchronize()
            prof = pe.profile_read()
            pe.profile_enable(False)
            print(f"cs={cs} {name}: profiled classes, ms per step (launches per step): "
                  + "; ".join(f"{k} {t / STEPS:.3f} ({cnt // STEPS})" for k, (cnt, t) in prof.items() if cnt and k.startswith(("train_", "event_")))
                  + f"; all classes {sum(t for _, t in prof.values()) / STEPS:.3f}", flush=True)
        del models
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
