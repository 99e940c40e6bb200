"""Training step: the whole-sequence fp32 attention backward against its chunked form (D3DP_TRAIN_LONG_ATTN=chunked) in ONE process
and one library, the two routes alternating round by round -- whole step (forward + backward, device events), B = 4, dep = 8, J = 17 --
at shapes both take (cs 64 / F 243, cs 96 / F 243, cs 576 / F 150); then the absolute step time of the chunked route where the
whole-sequence kernels refuse (cs 96 / F 351, cs 64 / F 351, cs 1024 / F 243).
usage: train_long_ab.py [ab | beyond]   (default: both parts)
The switch is read when a model's context is created (its first step), so each route gets a model of its own.  The last line per
shape gives the per-round ratio chunked / whole-sequence and says whether it exceeds the run's own round-to-round spread.  Nothing is
gated on these times.  Figures: profiles/train_long_f32.md."""
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from d3dp_amd import D3DP  # noqa: E402
from d3dp_amd.weights import H36M_JOINTS_LEFT as KL, H36M_JOINTS_RIGHT as KR, make_state_dict  # noqa: E402

J, B, DEP = 17, 4, 8
ROUNDS, STEPS, WARM = 6, 5, 2
SWITCH = "D3DP_TRAIN_LONG_ATTN"
ROUTES = (("whole-sequence", None), ("chunked", "chunked"))
BOTH = ((64, 243), (96, 243), (576, 150))
BEYOND = ((96, 351), (64, 351), (1024, 243))


def model(cs, F, value):
    if value:
        os.environ[SWITCH] = value
    else:
        os.environ.pop(SWITCH, None)
    args = SimpleNamespace(number_of_frames=F, test_time_augmentation=True, timestep=1000, scale=1.0, cs=cs, dep=DEP)
    m = D3DP(args, KL, KR, is_train=True)
    m.load_state_dict(make_state_dict(7, cs, DEP, F), strict=False)
    return m.cuda().train()


def timed(cs, F, routes):
    """{route: [ms per step of each round]}, the routes alternating inside every round."""
    x2 = torch.rand(B, F, J, 2, device="cuda") * 2 - 1
    x3 = torch.randn(B, F, J, 3, device="cuda") * 0.3

    def step(m):
        m.zero_grad(set_to_none=True)
        pr = m(x2, x3)
        loss = torch.mean(torch.norm(pr - x3, dim=-1))
        loss.backward(loss.clone().detach())

    models = {}
    for name, value in routes:
        m = model(cs, F, value)
        for _ in range(WARM):                      # (discarded: code objects load, the context and its workspace are made)
            step(m)
        torch.cuda.synchronize()
        print(f"cs={cs} F={F} {name}: {m.pose_estimator.train_arithmetic()}", flush=True)
        models[name] = m
    os.environ.pop(SWITCH, None)
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
        print(f"cs={cs} F={F} {name}: step (fwd + bwd, B={B} dep={DEP}) ms per round: " + " ".join(f"{v:.3f}" for v in ms[name])
              + f"; spread {(max(ms[name]) - min(ms[name])) / min(ms[name]) * 100:.2f} %", flush=True)
    del models
    torch.cuda.empty_cache()
    return ms


def main():
    part = sys.argv[1] if len(sys.argv) > 1 else "all"
    if part in ("all", "ab"):
        for cs, F in BOTH:
            ms = timed(cs, F, ROUTES)
            ratios = [c / w for w, c in zip(ms["whole-sequence"], ms["chunked"])]
            noise = max((max(v) - min(v)) / min(v) for v in ms.values())
            med = sorted(ratios)[len(ratios) // 2]
            beyond = min(ratios) - 1 > noise or 1 - max(ratios) > noise
            print(f"cs={cs} F={F}: chunked / whole-sequence step time per round " + " ".join(f"{r:.4f}" for r in ratios)
                  + f", median {med:.4f}, round-to-round spread {noise * 100:.2f} %: the difference is "
                  + ("BEYOND the spread" if beyond else "NOT beyond the spread") + " (not gated)", flush=True)
    if part in ("all", "beyond"):
        for cs, F in BEYOND:
            timed(cs, F, ROUTES[1:])


if __name__ == "__main__":
    main()
