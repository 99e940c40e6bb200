#!/usr/bin/env python3
"""The Python sampling loop against the native sampler (D3DP(sampler='native'): one d3dp_sample call), same model, same library,
one process: per shape and numerics the two hosts ALTERNATE for `--rounds` rounds, and each call is timed twice -- the wall time
until the device has finished it, and the host time until the call returned (the device still busy).  Neither injects noise: the
Python loop draws with torch.randn, the native call with the library's generator, as a user runs them.

    python tools/sampler_bench.py [--rounds 6] [--numerics exact fast16] [--out profiles/native_sampler_table.md]

Prints a markdown table: ms per call (median over the rounds), host ms until the call returns, the round spread ((max - min) /
median of the per-round figures, the larger of the two hosts'), and whether the difference between the hosts is beyond that spread.
"""
import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from d3dp_amd import D3DP  # noqa: E402
from d3dp_amd.weights import H36M_JOINTS_LEFT as KL, H36M_JOINTS_RIGHT as KR, flip_2d, make_state_dict, synthetic_inputs_2d  # noqa: E402

SHAPES = [(1, 1, 1), (4, 1, 1), (1, 20, 10), (4, 5, 5)]        # (B, H, K); the last is BASELINE configs[1]


def one_call(m, x2d, x2f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = m(x2d, None, input_2d_flip=x2f)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    assert out.shape[0] == x2d.shape[0]
    return (t2 - t0) * 1e3, (t1 - t0) * 1e3


def bench(numerics, B, H, K, rounds, frames, cs, dep):
    args = SimpleNamespace(number_of_frames=frames, test_time_augmentation=True, timestep=1000, scale=1.0, cs=cs, dep=dep)
    m = D3DP(args, KL, KR, is_train=False, num_proposals=H, sampling_timesteps=K, numerics=numerics)
    m.load_state_dict(make_state_dict(7, cs, dep, frames), strict=False)
    m = m.cuda().eval()
    x = synthetic_inputs_2d(3, B, frames)
    x2d, x2f = torch.from_numpy(x).cuda(), torch.from_numpy(flip_2d(x)).cuda()
    reps = max(1, min(10, 200 // (B * H * K)))                  # small calls: several per round, their median
    for sampler in ("python", "native"):                        # warm-up: contexts, workspaces, the allocator's pools
        m.sampler = sampler
        one_call(m, x2d, x2f)
        one_call(m, x2d, x2f)
    res = {"python": ([], []), "native": ([], [])}
    for _ in range(rounds):
        for sampler in ("python", "native"):
            m.sampler = sampler
            calls = [one_call(m, x2d, x2f) for _ in range(reps)]
            res[sampler][0].append(statistics.median(c[0] for c in calls))
            res[sampler][1].append(statistics.median(c[1] for c in calls))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--numerics", nargs="+", default=["exact", "fast16"])
    ap.add_argument("--frames", type=int, default=243)
    ap.add_argument("--cs", type=int, default=512)
    ap.add_argument("--dep", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sampler_bench needs an MI355X: libd3dp_hip has no CPU fallback")
    lines = [f"| numerics | B | H | K | python ms / call | native ms / call | python host ms | native host ms | round spread | native - python | beyond the spread |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for numerics in a.numerics:
        for B, H, K in SHAPES:
            r = bench(numerics, B, H, K, a.rounds, a.frames, a.cs, a.dep)
            med = {s: statistics.median(r[s][0]) for s in r}
            host = {s: statistics.median(r[s][1]) for s in r}
            spread = max((max(r[s][0]) - min(r[s][0])) / med[s] for s in r)
            diff = (med["native"] - med["python"]) / med["python"]
            lines.append(f"| {numerics} | {B} | {H} | {K} | {med['python']:.3f} | {med['native']:.3f} | {host['python']:.3f} | {host['native']:.3f} | "
                         f"{100 * spread:.2f} % | {100 * diff:+.2f} % | {'yes' if abs(diff) > spread else 'no'} |")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
