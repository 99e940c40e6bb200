"""Training step: the opt-in one-pass attention (D3DP_TRAIN_ATTN_PASSES=1) against the default, alone and beside the one-pass Linears
(D3DP_TRAIN_PASSES=1), in ONE process and one library -- four routes alternating round by round: default, attention one-pass,
Linears one-pass, both.  Every round prints, per route, the whole step (forward + backward, device events) and the six attention
classes of the per-kernel profile (forward, pass Q and pass KV of both axes: the classes the route touches); clock and power are
sampled as bench.py samples them.
usage: train_attn_passes_ab.py [cs ...]   (default 512 256 128; B = 4, F = 243, dep = 8 as BASELINE configs[4])
The switches are read when a model's context is created (its first step), so each route gets a model of its own.  Every comparison
is against the SAME run's default route (or, for `both`, its Linears-one-pass route); the last lines per width say whether a gain
exceeds the run's own round-to-round spread.  Figures: profiles/train_attn_one_pass.md."""
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (GpuTelemetry: shader clock and package power from the card's hwmon files)
from d3dp_amd import D3DP  # noqa: E402
from d3dp_amd.weights import H36M_JOINTS_LEFT as KL, H36M_JOINTS_RIGHT as KR, make_state_dict  # noqa: E402

F, J, B, DEP = 243, 17, 4, 8
ROUNDS, STEPS, PSTEPS, WARM = 6, 10, 4, 3
ATTN, LIN = "D3DP_TRAIN_ATTN_PASSES", "D3DP_TRAIN_PASSES"
ROUTES = (("default", {}), ("attn-1p", {ATTN: "1"}), ("lin-1p", {LIN: "1"}), ("both-1p", {ATTN: "1", LIN: "1"}))
PAIRS = (("attn-1p", "default"), ("both-1p", "lin-1p"), ("both-1p", "default"))      # (route, the route of the same run it is compared with)
CLASSES = tuple(f"train_attn_{k}_{a}" for a in ("spatial", "temporal") for k in ("fwd", "bwd_q", "bwd_kv"))


def main():
    widths = [int(a) for a in sys.argv[1:]] or [512, 256, 128]
    for cs in widths:
        x2 = torch.rand(B, F, J, 2, device="cuda") * 2 - 1
        x3 = torch.randn(B, F, J, 3, device="cuda") * 0.3
        models = {}

        def step(m):
            m.zero_grad(set_to_none=True)
            pr = m(x2, x3)
            loss = torch.mean(torch.norm(pr - x3, dim=-1))
            loss.backward(loss.clone().detach())

        for name, env in ROUTES:
            for k in (ATTN, LIN):
                os.environ.pop(k, None)
            os.environ.update(env)
            args = SimpleNamespace(number_of_frames=F, test_time_augmentation=True, timestep=1000, scale=1.0, cs=cs, dep=DEP)
            m = D3DP(args, KL, KR, is_train=True)
            m.load_state_dict(make_state_dict(7, cs, DEP, F), strict=False)
            m = m.cuda().train()
            for _ in range(WARM):                      # (discarded: code objects load, the context and its workspace are made)
                step(m)
            pe = m.pose_estimator
            pe.profile_enable(True)
            step(m)                                    # (discarded: the first profiled step creates the event pool)
            torch.cuda.synchronize()
            pe.profile_read()
            pe.profile_enable(False)
            print(f"cs={cs} {name}: {pe.train_arithmetic()}", flush=True)
            models[name] = m
        for k in (ATTN, LIN):
            os.environ.pop(k, None)
        ms = {k: [] for k in models}
        attn = {k: [] for k in models}
        counts = {}
        teles = {k: bench.GpuTelemetry(torch.cuda.current_device()) for k in models}
        for rnd in range(ROUNDS):
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
                pe = m.pose_estimator
                pe.profile_enable(True)
                for _ in range(PSTEPS):
                    step(m)
                torch.cuda.synchronize()
                prof = pe.profile_read()
                pe.profile_enable(False)
                counts[name] = {k: cnt // PSTEPS for k, (cnt, _) in prof.items()}
                attn[name].append(sum(prof[k][1] for k in CLASSES) / PSTEPS)
                print(f"cs={cs} round {rnd} {name}: step {ms[name][-1]:.3f} ms; attention classes, ms per step: "
                      + " ".join(f"{k[len('train_attn_'):]} {prof[k][1] / PSTEPS:.3f}" for k in CLASSES)
                      + f"; their sum {attn[name][-1]:.3f}", flush=True)
        spread = {}
        for name in models:
            tr = teles[name].report()
            spread[name] = (max(ms[name]) - min(ms[name])) / min(ms[name])
            print(f"cs={cs} {name}: step (fwd + bwd, B={B} F={F} dep={DEP}) ms per round: " + " ".join(f"{v:.3f}" for v in ms[name])
                  + f"; spread {spread[name] * 100:.2f} %; clock {tr['clock_mhz_mean']} MHz, power "
                  f"{tr['power_w_mean']} W (cap {tr['power_cap_w']} W) over its timed rounds", flush=True)
        same = all(counts[n] == counts["default"] for n in models)
        # per round: the pair of neighbouring measurements; a gain counts only beyond the larger of the two routes' own spreads
        for new, old in PAIRS:
            gains = [1.0 - n / o for o, n in zip(ms[old], ms[new])]
            med = sorted(gains)[len(gains) // 2]
            noise = max(spread[new], spread[old])
            a_old, a_new = sorted(attn[old])[ROUNDS // 2], sorted(attn[new])[ROUNDS // 2]
            print(f"cs={cs}: {new} against {old}: step-time gain per round " + " ".join(f"{g * 100:+.2f}%" for g in gains)
                  + f", median {med * 100:+.2f} %, round-to-round spread {noise * 100:.2f} %: "
                  + ("BEYOND the spread" if min(gains) > noise else "NOT beyond the spread")
                  + f"; six attention classes (median round) {a_old:.3f} -> {a_new:.3f} ms", flush=True)
        print(f"cs={cs}: launch counts per class " + ("equal over the four routes" if same else "DIFFER"), flush=True)
        del models
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
