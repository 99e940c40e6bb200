"""Training step: the default three-pass split-fp16 Linears against the opt-in one-pass route (D3DP_TRAIN_PASSES=1) in ONE process and
one library, the two settings alternating -- whole step (forward + backward, device events), the per-class profile of the training
step (train_linear / train_wgrad are the classes the route touches); clock and power sampled as bench.py samples them.
usage: train_passes_ab.py [cs ...]   (default 512 256; B = 4, F = 243, dep = 8 as BASELINE configs[4]; 192 / 320 / 384 / 448 run
both settings under D3DP_TRAIN_IMPL=f16x2)
The switch is read when a model's context is created (its first step), so each setting gets a model of its own.  The last line per
width says whether the gain exceeds the run's own round-to-round spread.  Figures: profiles/train_one_pass.md."""
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (GpuTelemetry: shader clock and package power from the card's hwmon files)
from d3dp_amd import D3DP  # noqa: E402
from d3dp_amd.weights import H36M_JOINTS_LEFT as KL, H36M_JOINTS_RIGHT as KR, make_state_dict  # noqa: E402

F, J, B, DEP = 243, 17, 4, 8
ROUNDS, STEPS, WARM = 6, 10, 3
SWITCH = "D3DP_TRAIN_PASSES"
ROUTES = (("three-pass", None), ("one-pass", "1"))


def main():
    widths = [int(a) for a in sys.argv[1:]] or [512, 256]
    for cs in widths:
        x2 = torch.rand(B, F, J, 2, device="cuda") * 2 - 1
        x3 = torch.randn(B, F, J, 3, device="cuda") * 0.3
        models = {}
        if cs in (192, 320, 384, 448):
            os.environ["D3DP_TRAIN_IMPL"] = "f16x2"

        def step(m):
            m.zero_grad(set_to_none=True)
            pr = m(x2, x3)
            loss = torch.mean(torch.norm(pr - x3, dim=-1))
            loss.backward(loss.clone().detach())

        for name, value in ROUTES:
            if value:
                os.environ[SWITCH] = value
            else:
                os.environ.pop(SWITCH, None)
            args = SimpleNamespace(number_of_frames=F, test_time_augmentation=True, timestep=1000, scale=1.0, cs=cs, dep=DEP)
            m = D3DP(args, KL, KR, is_train=True)
            m.load_state_dict(make_state_dict(7, cs, DEP, F), strict=False)
            m = m.cuda().train()
            for _ in range(WARM):                      # (discarded: code objects load, the context and its workspace are made)
                step(m)
            torch.cuda.synchronize()
            print(f"cs={cs} {name}: {m.pose_estimator.train_arithmetic()}", flush=True)
            models[name] = m
        os.environ.pop(SWITCH, None)
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
        spread = {}
        for name in models:
            tr = teles[name].report()
            spread[name] = (max(ms[name]) - min(ms[name])) / min(ms[name])
            print(f"cs={cs} {name}: step (fwd + bwd, B={B} F={F} dep={DEP}) ms per round: " + " ".join(f"{v:.3f}" for v in ms[name])
                  + f"; spread {spread[name] * 100:.2f} %; clock {tr['clock_mhz_mean']} MHz, power "
                  f"{tr['power_w_mean']} W (cap {tr['power_cap_w']} W) over its timed rounds", flush=True)
        prof = {}
        for name, m in models.items():
            pe = m.pose_estimator
            pe.profile_enable(True)
            step(m)                                    # (discarded: the first profiled step creates the event pool)
            torch.cuda.synchronize()
            pe.profile_read()
            for _ in range(STEPS):
                step(m)
            torch.cuda.synchronize()
            prof[name] = pe.profile_read()
            pe.profile_enable(False)
            print(f"cs={cs} {name}: profiled classes, ms per step (launches per step): "
                  + "; ".join(f"{k} {t / STEPS:.3f} ({cnt // STEPS})" for k, (cnt, t) in prof[name].items()
                              if cnt and k.startswith(("train_", "event_")))
                  + f"; all classes {sum(t for _, t in prof[name].values()) / STEPS:.3f}", flush=True)
        # per round: the pair of neighbouring measurements; the gain counts only beyond the larger of the two routes' own spreads
        gains = [1.0 - o / t for t, o in zip(ms["three-pass"], ms["one-pass"])]
        med = sorted(gains)[len(gains) // 2]
        noise = max(spread.values())
        cls = "; ".join(f"{k} {prof['three-pass'][k][1] / STEPS:.3f} -> {prof['one-pass'][k][1] / STEPS:.3f} ms" for k in ("train_linear", "train_wgrad"))
        same = all(prof["three-pass"][k][0] == prof["one-pass"][k][0] for k in prof["three-pass"])
        print(f"cs={cs}: one-pass step-time gain per round " + " ".join(f"{g * 100:+.2f}%" for g in gains) + f", median {med * 100:+.2f} %, "
              f"round-to-round spread {noise * 100:.2f} %: " + ("BEYOND the spread" if min(gains) > noise else "NOT beyond the spread")
              + f"; {cls}; launch counts per class " + ("equal" if same else "DIFFER"), flush=True)
        del models
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
