#!/usr/bin/env python3
"""Micro-benchmark of the attention kernels through the C ABI (d3dp_op_attention) at the denoiser's shapes.

`--cs C`: rows of C channels (8 heads).  `--impls 0,1` times several implementations on the same rows in one run, visited in turn
within every iteration: on 2-byte rows impl 0 is the fp32 row kernel and impl 1 the matrix-core kernels of the FAST modes, so
`--cs 256 --impls 0,1` is the A/B of the two routes a FAST context can take at head dim 32.  `--fp16`: IEEE fp16 rows (act 4)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from d3dp_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=15)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--which", default="temporal,spatial")
    ap.add_argument("--joints", type=int, default=17, help="J (temporal sequences gather rows at a stride of J token rows)")
    ap.add_argument("--exact", action="store_true", help="the EXACT-mode (split-fp16) kernels on fp32 rows (impl 2) instead of the bf16 ones")
    ap.add_argument("--cs", type=int, default=512, help="channels (8 heads)")
    ap.add_argument("--frames", type=int, default=243)
    ap.add_argument("--impls", default=None, help="comma-separated impl codes to time on the same rows, e.g. 0,1 (default: 1; 2 with --exact)")
    ap.add_argument("--fp16", action="store_true", help="IEEE fp16 rows (act 4) instead of bf16")
    a = ap.parse_args()
    lib = _lib.load()
    F, J, C, heads = a.frames, a.joints, a.cs, 8
    T = a.seqs * F * J
    qkv = torch.randn(T, 3 * C, device="cuda")
    out = torch.empty(T, C, device="cuda")
    if not a.exact:
        dt = torch.float16 if a.fp16 else torch.bfloat16
        qkv, out = qkv.to(dt), out.to(dt)
    act = 0 if a.exact else (4 if a.fp16 else 1)
    impls = [int(i) for i in a.impls.split(",")] if a.impls else [2 if a.exact else 1]
    st = torch.cuda.current_stream().cuda_stream
    for name in a.which.split(","):
        axis = 1 if name == "temporal" else 0
        for impl in impls:
            for _ in range(2):
                _lib.check(lib.d3dp_op_attention(act, impl, axis, qkv.data_ptr(), out.data_ptr(), a.seqs, F, J, C, heads, st))
        evs = {impl: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)] for impl in impls}
        for i in range(a.iters):
            for impl in impls:
                e0, e1 = evs[impl][i]
                e0.record()
                _lib.check(lib.d3dp_op_attention(act, impl, axis, qkv.data_ptr(), out.data_ptr(), a.seqs, F, J, C, heads, st))
                e1.record()
        torch.cuda.synchronize()
        n = F if axis else J
        flops = 4.0 * n * C * T
        med = {}
        for impl in impls:
            ts = sorted(e0.elapsed_time(e1) for e0, e1 in evs[impl])
            med[impl] = ts[len(ts) // 2]
            print(f"{name:9s} cs={C} F={F} J={J} act={act} impl={impl} T={T}: median {med[impl]*1e3:7.1f} us  min {ts[0]*1e3:7.1f} us  "
                  f"{flops/med[impl]/1e9:7.1f} TFLOP/s  {T*4*C*2/med[impl]/1e9*1e-3:6.2f} TB/s")
        if len(impls) > 1:
            print(f"{name:9s} cs={C} F={F} J={J} act={act}: " + "  ".join(f"impl {i} / impl {impls[-1]} = {med[i]/med[impls[-1]]:.2f}x" for i in impls[:-1]))


if __name__ == "__main__":
    main()
