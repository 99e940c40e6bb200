#!/usr/bin/env python3
"""Interleaved same-process comparison of numerics modes on BASELINE configs[2] (ddim_sample_flip, F=243, J=17, B=16, H=20, K=10).

    python tools/mode_bench.py --numerics fast,fast16 [--steps 20] [--warmup 5] [--rounds 4] [--frames 243] [--cs 512]

`--frames N` runs the same sampler on clips of N frames (1 ... 1024), `--cs C` at a width of C channels (8 heads; 512, 256, 128
or 64, and for `exact` any width the library takes: 192, 320, 384 and 448 have two routes).  An `:f16x2` suffix (`exact:f16x2`)
creates that model's context with D3DP_EXACT_IMPL=f16x2: at `--cs` 192 / 320 / 384 / 448 the split-fp16 implementation with padded
heads instead of the fp32 implementation -- `--cs 384 --numerics exact,exact:f16x2` is the A/B of the two.  An `:mfma` suffix on a
FAST mode (`fast:mfma`, `fast16:mfma`) creates that model's context with D3DP_FAST_IMPL=mfma: the only way such a context exists at
`--cs` 192 / 320 / 384 / 448 -- `--cs 384 --numerics exact:f16x2,fast:mfma,fast16:mfma` compares the three opt-in routes there.  A `:rows` suffix on a mode name (`fast:rows`, `exact:rows`)
creates that model's library context with D3DP_LONG_ATTN=rows in the environment: the row attention kernel wherever the mode would
take a chunked-key or, in the FAST modes, a whole-sequence matrix-core kernel beyond 256 frames / 32 joints, and at head dims 32
and 16 (`--cs 256`, `--cs 128`) for every attention of a FAST mode -- the A/B of those kernels in one process:
`--cs 256 --numerics fast:rows,fast,fast16:rows,fast16`.  A `:scale` suffix on `fast16` creates that model's context with
D3DP_FAST16_RANGE=scale: blocks whose proven bound reaches 65504 store the tensors it covers at a power of two of their value instead
of moving the context to bf16.  It shows on weights that trip the proof, which `--edit NAME` makes of the seed weights, for every
model alike -- a tensor of one block multiplied by a factor (EDITS below; `norm1x32`: gain and bias of TTEblocks.1.norm1 x 32) --
`--edit norm1x32 --numerics fast,fast16:scale --batch 4 --hyps 5 --ksteps 5` is the A/B at BASELINE configs[1] size: without the
switch `fast16` runs `fast`'s kernels on such weights, so `fast` is the yardstick.  The variables are read when a context is
created, so every context is created before anything is timed.

Every mode gets its own model (and library context) on the same weights, inputs and generator seed.  After `--warmup` steps of each,
the timed steps are taken in `--rounds` rounds that visit the modes in turn (a b a b ...), steps / rounds steps per visit, a host
clock around a device synchronise per visit: drift of the box (clock, temperature, neighbours) lands on every mode alike, which two
back-to-back bench.py runs cannot offer.  Clock and power are sampled the way bench.py samples them (its GpuTelemetry), per mode,
over that mode's timed visits only.  Prints ONE JSON line: per mode hypothesis-clips/s, ms per step, the per-visit spread, mean
clock / power; the ratio of every mode to the first; the operand type and proven bound of the FAST modes; the library's sha256;
and, from one more untimed step per mode under d3dp_profile_read, launches and kernel ms of the two attention classes (EXACT
modes: of every class, with the implementation the context reports; `--classes`: of every class for every mode).
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


# --edit: (parameter names under pose_estimator., factor) -- the weight edits of tests/test_hip_fast16_scaled.py
EDITS = {"norm1x32": (("TTEblocks.1.norm1.weight", "TTEblocks.1.norm1.bias"), 32.0),
         "norm1x256": (("TTEblocks.1.norm1.weight", "TTEblocks.1.norm1.bias"), 256.0),
         "fc1x256": (("STEblocks.0.mlp.fc1.weight",), 256.0),
         "fc2x16": (("TTEblocks.0.mlp.fc2.weight",), 16.0),
         "projx32": (("STEblocks.1.attn.proj.weight",), 32.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--numerics", default="fast,fast16", help="comma-separated modes, e.g. fast,fast16,exact")
    ap.add_argument("--steps", type=int, default=20, help="timed steps per mode (>= rounds)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4, help="interleaving rounds the timed steps are split into")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--hyps", type=int, default=20)
    ap.add_argument("--ksteps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=None, help="clip length (default: bench.py's, 243)")
    ap.add_argument("--cs", type=int, default=None, help="channels, 8 heads (default: bench.py's, 512)")
    ap.add_argument("--classes", action="store_true", help="report launches and kernel ms of EVERY profile class for every mode")
    ap.add_argument("--edit", choices=sorted(EDITS), default=None, help="multiply one block's tensor(s) in every model (see the docstring)")
    a = ap.parse_args()
    modes = [m.strip() for m in a.numerics.split(",") if m.strip()]
    if not modes or a.steps < a.rounds or a.rounds < 1 or a.warmup < 0:
        ap.error("need at least one mode, --rounds >= 1 and --steps >= --rounds")
    import torch
    import bench
    from d3dp_amd.weights import flip_2d, synthetic_inputs_2d
    B, H, K = a.batch, a.hyps, a.ksteps
    frames = bench.F_ if a.frames is None else a.frames
    # the switch a suffix sets in the environment while that mode's context is created
    suffixes = {"rows": ("D3DP_LONG_ATTN", "rows"), "f16x2": ("D3DP_EXACT_IMPL", "f16x2"), "mfma": ("D3DP_FAST_IMPL", "mfma"),
                "scale": ("D3DP_FAST16_RANGE", "scale")}
    if not 1 <= frames <= 1024 or any(m.count(":") > 1 or (":" in m and m.split(":")[1] not in suffixes) for m in modes):
        ap.error("--frames must be in [1, 1024]; the mode suffixes are ':rows', ':f16x2', ':mfma' and ':scale'")
    x2d_np = synthetic_inputs_2d(1234, B, frames)
    x2d, x2f = torch.from_numpy(x2d_np).cuda(), torch.from_numpy(flip_2d(x2d_np)).cuda()
    cs = bench.C_ if a.cs is None else a.cs
    models = {m: bench.build_model(H, K, m.split(":")[0], 0, frames=frames, cs=cs) for m in modes}
    if a.edit:
        names, factor = EDITS[a.edit]
        with torch.no_grad():
            for model in models.values():
                params = dict(model.pose_estimator.named_parameters())
                for n in names:
                    params[n].mul_(factor)
    for m in modes:                                    # the contexts, now: a suffixed one with its switch set for its creation
        key, val = suffixes[m.split(":")[1]] if ":" in m else (None, None)
        saved = os.environ.get(key) if key else None
        if key:
            os.environ[key] = val
        try:
            models[m].pose_estimator._context(torch.device("cuda", torch.cuda.current_device()))
        finally:
            if key:
                os.environ.pop(key)
                if saved is not None:
                    os.environ[key] = saved
    gens = {m: torch.Generator(device="cuda").manual_seed(1) for m in modes}
    teles = {m: bench.GpuTelemetry(torch.cuda.current_device()) for m in modes}
    for m in modes:
        for _ in range(a.warmup):
            models[m](x2d, None, input_2d_flip=x2f, generator=gens[m])
    torch.cuda.synchronize()
    per_visit = [a.steps // a.rounds + (1 if r < a.steps % a.rounds else 0) for r in range(a.rounds)]
    visits = {m: [] for m in modes}
    out = None
    for n in per_visit:
        for m in modes:
            teles[m].start()
            t0 = time.perf_counter()
            for _ in range(n):
                out = models[m](x2d, None, input_2d_flip=x2f, generator=gens[m])
            torch.cuda.synchronize()
            visits[m].append((time.perf_counter() - t0) / n)
            teles[m].stop()
            assert bool(torch.isfinite(out).all())
    res = {"workload": f"{'BASELINE configs[2]: ' if (frames, cs) == (bench.F_, bench.C_) else ''}ddim_sample_flip F={frames} J=17 B={B} H={H} K={K} flip-TTA, cs={cs} dep=8",
           "weight_edit": a.edit, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "order": modes, "library_sha256": bench.lib_sha256(), "modes": {}}
    for m in modes:
        dt = sum(v * n for v, n in zip(visits[m], per_visit))
        tr = teles[m].report()
        fo = models[m].pose_estimator.fast_operands()
        prof = bench.profile_step(models[m], x2d, x2f, gens[m])       # (one more step, after everything timed)
        res["modes"][m] = {"value": B * H * a.steps / dt, "unit": "hypothesis-clips/s", "ms_per_step": dt / a.steps * 1e3,
                           "ms_per_step_by_visit": [round(v * 1e3, 2) for v in visits[m]],
                           "clock_mhz_mean": tr["clock_mhz_mean"], "power_w_mean": tr["power_w_mean"], "power_cap_w": tr["power_cap_w"],
                           "fast_operands": None if fo is None else {"type": fo[0], "proven_bound": fo[1]},
                           "attention_classes_one_step": {k: {"launches": c, "kernel_ms": round(ms, 3)} for k, (c, ms) in prof.items()
                                                          if k.startswith("attn")}}
        if m.split(":")[0] == "exact":
            res["modes"][m]["exact_implementation"] = models[m].pose_estimator.exact_scales()[2]
        if m.split(":")[0] == "exact" or a.classes:
            res["modes"][m]["classes_one_step"] = {k: {"launches": c, "kernel_ms": round(ms, 3)} for k, (c, ms) in prof.items() if c}
    base = res["modes"][modes[0]]["value"]
    res["ratio_to_first"] = {m: res["modes"][m]["value"] / base for m in modes}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
