"""Training step: the opt-in one-pass Linears (D3DP_TRAIN_PASSES=1) against the same route on hi-only operand rows (D3DP_TRAIN_ROWS=hi),
alone and beside the one-pass attention (D3DP_TRAIN_ATTN_PASSES=1), in ONE process and one library, the four settings alternating --
whole step (forward + backward, device events), the per-class profile of the training step (train_linear / train_wgrad /
train_operand_pass are the classes the rows touch); clock and power sampled as bench.py samples them.
usage: train_rows_ab.py [cs ...]   (default 512 256: the widths of the route; B = 4, F = 243, dep = 8 as BASELINE configs[4])
The switches are read when a model's context is created (its first step), so each setting gets a model of its own.  The baseline of
every gain is the D3DP_TRAIN_PASSES=1 route (beside the one-pass attention: PASSES=1 + ATTN_PASSES=1) of the SAME run; the last lines
per width say whether each gain exceeds the run's own round-to-round spread.  Figures: profiles/train_hi_rows.md.  (The HBM-side
traffic of the two routes is a counter run of its own: this script's first argument `pmc-split` / `pmc-hi` runs ten steps of one
route at cs 512 and nothing else, for a profiler that collects counters alone.)"""
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
SWITCHES = ("D3DP_TRAIN_PASSES", "D3DP_TRAIN_ROWS", "D3DP_TRAIN_ATTN_PASSES")
# name: (values of SWITCHES, the route its gain is measured against)
ROUTES = {"one-pass": (("1", None, None), None), "one-pass + hi rows": (("1", "hi", None), "one-pass"),
          "one-pass + attn": (("1", None, "1"), None), "all three": (("1", "hi", "1"), "one-pass + attn")}
CLASSES = ("train_linear", "train_wgrad", "train_operand_pass")


def model_under(cs, values):
    for k, v in zip(SWITCHES, values):
        if v:
            os.environ[k] = v
        else:
            os.environ.pop(k, None)
    args = SimpleNamespace(number_of_frames=F, test_time_augmentation=True, timestep=1000, scale=1.0, cs=cs, dep=DEP)
    m = D3DP(args, KL, KR, is_train=True)
    m.load_state_dict(make_state_dict(7, cs, DEP, F), strict=False)
    return m.cuda().train()


def main():
    argv = sys.argv[1:]
    x2 = torch.rand(B, F, J, 2, device="cuda") * 2 - 1
    x3 = torch.randn(B, F, J, 3, device="cuda") * 0.3

    def step(m):
        m.zero_grad(set_to_none=True)
        pr = m(x2, x3)
        loss = torch.mean(torch.norm(pr - x3, dim=-1))
        loss.backward(loss.clone().detach())

    if argv and argv[0] in ("pmc-split", "pmc-hi"):
        m = model_under(512, ("1", "hi" if argv[0] == "pmc-hi" else None, None))
        for _ in range(STEPS):
            step(m)
        torch.cuda.synchronize()
        print(f"{argv[0]}: {STEPS} steps of cs=512 B={B} F={F} dep={DEP}: {m.pose_estimator.train_arithmetic()}")
        return
    for cs in [int(a) for a in argv] or [512, 256]:
        models = {}
        for name, (values, _) in ROUTES.items():
            m = model_under(cs, values)
            for _ in range(WARM):                      # (discarded: code objects load, the context and its workspace are made)
                step(m)
            torch.cuda.synchronize()
            print(f"cs={cs} {name}: {m.pose_estimator.train_arithmetic()}", flush=True)
            models[name] = m
        for k in SWITCHES:
            os.environ.pop(k, None)
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
        # per round: the pair of neighbouring measurements; a gain counts only beyond the larger of the two routes' own spreads
        for name, (_, base) in ROUTES.items():
            if base is None:
                continue
            gains = [1.0 - h / s for s, h in zip(ms[base], ms[name])]
            med = sorted(gains)[len(gains) // 2]
            noise = max(spread[name], spread[base])
            cls = "; ".join(f"{k} {prof[base][k][1] / STEPS:.3f} -> {prof[name][k][1] / STEPS:.3f} ms" for k in CLASSES)
            same = all(prof[base][k][0] == prof[name][k][0] for k in prof[base])
            print(f"cs={cs}: `{name}` against `{base}`: step-time gain per round " + " ".join(f"{g * 100:+.2f}%" for g in gains)
                  + f", median {med * 100:+.2f} %, round-to-round spread {noise * 100:.2f} %: "
                  + ("BEYOND the spread" if min(gains) > noise else "NOT beyond the spread")
                  + f"; {cls}; launch counts per class " + ("equal" if same else "DIFFER"), flush=True)
        del models
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
