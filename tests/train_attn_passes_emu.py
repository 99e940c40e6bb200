"""CPU emulation of the one-pass training attention (D3DP_TRAIN_ATTN_PASSES=1) and the references the two test files of the route
share (tests/test_train_attn_passes_host.py, tests/test_hip_train_attn_passes.py).  Test infrastructure: nothing in d3dp_amd imports it.

The route (d3dp_amd/csrc/train_attn_1p.hip: the kernels of train_attn.hip with PASSES = 1) runs every product of the attention as ONE
fp16-MFMA pass with fp32 accumulation.  What is rounded to IEEE fp16, once each, and at which power of two:

    q, k, v      at the scale of the absmax of the whole qkv tensor (ta_scale = the Linears' dyn_scale)
    dO           at the scale of its own absmax
    P x 2^10     forward: p = exp(s - rowmax) against the row maximum; backward: p = exp(s - L), L the forward's log-sum-exp
    dS           at the power of two of the largest |dS| of its query (dQ = dS K) / of its key (dK = dS^T Q)

and what stays fp32: the logits s, the softmax denominator (the sum of the UNROUNDED p), L, D = dO . O (of the unrounded dO and O), the
output and every accumulator.  The kernels pass keys / queries in pairs of tiles with a RUNNING maximum and a RUNNING dS exponent; the
emulation uses the final ones -- the same roundings at, here and there, a coarser grid.

`one_pass_attention()` replaces oracle.d3dp_oracle.attention -- the module attribute its blocks look up -- by the same function with
an autograd Function between the qkv and the proj Linear, for fp32 runs at the head dims the kernels exist for (64, 32, 16); the two
Linears go through torch.nn.functional.linear at call time, so the block nests with train_passes_emu.one_pass_linears().  axes="t":
the temporal blocks alone (D3DP_TRAIN_ATTN=x2t: the spatial axis runs fp32 kernels).  order="halves": every product as two
half-contraction sums -- the second accumulation order of the admissibility check."""
from __future__ import annotations

import contextlib
from functools import lru_cache
from typing import Dict, NamedTuple, Tuple

import torch
import torch.nn.functional as F

import train_passes_emu as lin_emu
from oracle import d3dp_oracle as orc
from oracle import grad_check as gc
from test_hip_train_grads import Case, problem

SWITCH = "D3DP_TRAIN_ATTN_PASSES"
HEAD_DIMS = (64, 32, 16)

# The GPU cases of the training step (tests/test_hip_train_attn_passes.py): J = 17, dep = 2, recorded DropPath.  Together: each of the
# six sequence-length instantiations (9 and the 17 joints -> 32, 40 -> 64, 100 -> 128, 243 -> 256, 300 -> 512, 520 -> 1024), the
# one-kernel backward of the spatial axis, and a partial last tile everywhere.
STEP_CASES = [
    Case(512, 9, 2), Case(512, 100, 2), Case(512, 243, 2),
    Case(256, 40, 2), Case(256, 300, 2),
    Case(128, 9, 2), Case(128, 520, 1),
]
BOTH_CASE = Case(256, 40, 2)          # beside D3DP_TRAIN_PASSES=1
X2T_CASE = Case(256, 40, 2)           # under D3DP_TRAIN_ATTN=x2t
DROPPED_CASE = Case(128, 9, 2, masks="dropped")
UPSTREAM_CASE = Case(256, 40, 2)
UPSTREAM_K = (-40, 0, 30)


def r16_at(x: torch.Tensor, s) -> torch.Tensor:
    """fp16(x s) / s for a power of two s (a float or a tensor that broadcasts)."""
    return (x * s).to(torch.float16).to(torch.float32) / s


def pow2_scale(m: torch.Tensor) -> torch.Tensor:
    """ta_scale / ta_split_run elementwise on a tensor of absmax values: 2^(14 - e) for m = f 2^e, f in [0.5, 1); 1 for m = 0."""
    _, e = torch.frexp(m.to(torch.float32))
    s = torch.ldexp(torch.ones_like(m, dtype=torch.float32), 14 - e)
    return torch.where((m > 0) & torch.isfinite(m), s, torch.ones_like(s))


def _mm(a, b, halves):
    """a @ b over the last / second-to-last axis, optionally as two half-contraction sums."""
    k = a.shape[-1]
    if not halves or k < 8:
        return a @ b
    return a[..., :k // 2] @ b[..., :k // 2, :] + a[..., k // 2:] @ b[..., k // 2:, :]


def _heads(x, heads):
    """(S, N, heads hd) -> (S, heads, N, hd)"""
    S, N, C = x.shape
    return x.reshape(S, N, heads, C // heads).transpose(1, 2)


class _OnePassAttention(torch.autograd.Function):
    """qkv (S, N, 3 C) -> o (S, N, C)"""

    @staticmethod
    def forward(ctx, qkv, heads, halves):
        S, N, C3 = qkv.shape
        C = C3 // 3
        hd = C // heads
        qkv_r = r16_at(qkv, lin_emu.dyn_scale(qkv))
        q, k, v = (_heads(t, heads) for t in qkv_r.split(C, dim=-1))
        s = _mm(q, k.transpose(-1, -2), halves) * hd ** -0.5
        m = s.amax(dim=-1, keepdim=True)
        p = torch.exp(s - m)
        den = p.sum(dim=-1, keepdim=True)                        # of the unrounded p
        o = _mm(r16_at(p, 1024.0), v, halves) / den
        o = o.transpose(1, 2).reshape(S, N, C)
        ctx.save_for_backward(qkv_r, o, m + torch.log(den))
        ctx.heads, ctx.halves = heads, halves
        return o

    @staticmethod
    def backward(ctx, do):
        qkv_r, o, L = ctx.saved_tensors
        heads, halves = ctx.heads, ctx.halves
        S, N, C = o.shape
        hd = C // heads
        q, k, v = (_heads(t, heads) for t in qkv_r.split(C, dim=-1))
        D = _heads(do * o, heads).sum(dim=-1, keepdim=True)      # dO . O of the unrounded fp32 tensors
        g = _heads(r16_at(do, lin_emu.dyn_scale(do)), heads)
        p = torch.exp(_mm(q, k.transpose(-1, -2), halves) * hd ** -0.5 - L)
        ds = p * (_mm(g, v.transpose(-1, -2), halves) - D) * hd ** -0.5
        ds_q = r16_at(ds, pow2_scale(ds.abs().amax(dim=-1, keepdim=True)))      # per query: pass Q
        ds_k = r16_at(ds, pow2_scale(ds.abs().amax(dim=-2, keepdim=True)))      # per key: pass KV
        dq = _mm(ds_q, k, halves)
        dk = _mm(ds_k.transpose(-1, -2), q, halves)
        dv = _mm(r16_at(p, 1024.0).transpose(-1, -2), g, halves)
        back = lambda t: t.transpose(1, 2).reshape(S, N, C)
        return torch.cat([back(dq), back(dk), back(dv)], dim=-1), None, None


@contextlib.contextmanager
def one_pass_attention(order: str = "plain", axes: str = "both"):
    """oracle.d3dp_oracle.attention -> the emulation for fp32 activations at head dims 64 / 32 / 16 (axes="t": of the temporal blocks
    alone).  Yields the list of (block prefix, emulated) of every call inside the block."""
    assert order in ("plain", "halves") and axes in ("both", "t")
    plain, calls = orc.attention, []

    def attention(x, p, pre):
        C = x.shape[-1]
        emulated = (x.dtype == torch.float32 and p.get("__emulate_bf16__") is None and C // orc.NUM_HEADS in HEAD_DIMS
                    and (axes == "both" or pre.startswith("TTEblocks")))
        calls.append((pre, emulated))
        if not emulated:
            return plain(x, p, pre)
        qkv = F.linear(x, p[pre + "attn.qkv.weight"], p[pre + "attn.qkv.bias"])
        o = _OnePassAttention.apply(qkv, orc.NUM_HEADS, order == "halves")
        return F.linear(o, p[pre + "attn.proj.weight"], p[pre + "attn.proj.bias"])
    orc.attention = attention
    try:
        yield calls
    finally:
        orc.attention = plain


# ---- references, computed once per case and shared; never written to ----------------------------------------------------------------
class Base(NamedTuple):
    g64: Dict[str, torch.Tensor]          # fp64 autograd of the case; gc.PREDICTION holds the fp64 prediction
    e32: Tuple[float, float]              # the fp32 oracle against it (worst tensor, each figure)


def _worst(got, pred, want) -> Tuple[float, float]:
    n, m, _, _ = gc.worst_of({k: e for k, e in gc.grad_errors({**got, gc.PREDICTION: pred}, want).items() if not e.zero_ref})
    return n, m


@lru_cache(maxsize=None)
def base(case) -> Base:
    sd, x2d, gt, t, noise, dpd = problem(case)
    g64, p64 = gc.reference_grads(sd, x2d, gt, t, noise, case.dep, dpd, torch.float64)
    g32, p32 = gc.reference_grads(sd, x2d, gt, t, noise, case.dep, dpd, torch.float32)
    want = {**g64, gc.PREDICTION: p64}
    return Base(want, _worst(g32, p32, want))


@lru_cache(maxsize=None)
def emulated(case, axes: str = "both", linears: bool = False, order: str = "plain") -> Tuple[float, float]:
    """(norm, per-element) error against fp64 of the emulated step: the one-pass attention of `axes`, beside the one-pass Linears if
    `linears`, every emulated product in the accumulation order `order`."""
    sd, x2d, gt, t, noise, dpd = problem(case)
    with one_pass_attention(order, axes), (lin_emu.one_pass_linears(order) if linears else contextlib.nullcontext()):
        g, p = gc.reference_grads(sd, x2d, gt, t, noise, case.dep, dpd, torch.float32)
    return _worst(g, p, base(case).g64)


def spread(case, axes: str = "both", linears: bool = False) -> Tuple[float, float]:
    """the emulation under the second accumulation order, over the first"""
    e, h = emulated(case, axes, linears), emulated(case, axes, linears, "halves")
    return h[0] / e[0], h[1] / e[1]
