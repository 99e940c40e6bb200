"""Element-by-element check of FAST (bf16 operands) and FAST16 (fp16 operands) inference against the oracle's fp64 forward pass
(CPU only).

The gates the two 2x modes had at denoiser and sampler level are means over all B H F 17 joints (`mpjpe_mm <= 8`, `<= 1.5 x` the
2-byte emulation's own mean) and their single-op gates are `allclose` at about 5 x one correct 2-byte rounding: one wrong tile passes
both (profiles/fast_elementwise.md).  A TIGHT gate against the 2-byte emulation does not exist -- the pipeline is chaotic in its
roundings (test_sampler_fast_mode_vs_bf16_emulating_oracle) -- but a gate against fp64 IN THE EMULATION'S OWN ERROR CLASS does:

  e16     = (norm_rel, max_rms) of the oracle's 2-byte emulation of a case (orc.emulate_bf16, with orc._r16 the rounding of the
            type) against the oracle's fp64 run of it: how far a correct 2-byte pipeline lies from fp64 there;
  bound   = NORM16 x e16 in norm_rel, MAX16 x e16 in max_rms (the figures of grad_check.tensor_error), measured against fp64;
  spread  = the same two figures of the emulation under a second accumulation order (every Linear's K split in halves) over e16:
            how much of e16 is chance.  A case is admissible only if spread <= ADMIT_SPREAD.

NORM16 = 1.5 is the margin the project gives accumulation order everywhere (`e32 <= 1.5 emu32`).  MAX16 = 4 is three times the
largest reference-only spread of the per-element figure measured over eight cases (1.31), and below the smallest factor (7.1) by
which losing 32 k-columns in 16 rows of ONE Linear moves that figure.

The single-op models are the fp64 operation on operands already rounded to the type, with exactly the roundings the kernel's header
names; an op's e16 is the model's distance from the unrounded fp64 result of the same rounded operands."""
from __future__ import annotations

import contextlib
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from d3dp_amd.weights import H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, flip_2d

from . import d3dp_oracle as orc
from .grad_check import Err, tensor_error, violations  # noqa: F401
from .infer_check import _params, locate

NORM16, MAX16 = 1.5, 4.0
ADMIT_SPREAD = (1.15, 2.0)
FAST_PASS_SEQS = 15            # FAST / FAST16 contexts: sequences per pass unless chunk_seqs says otherwise (csrc/ctx.h: chunk())
EPI_BIAS, EPI_GELU = 0, 1


class Seen:
    """What went through the rounding of a `rounding` block: the largest finite magnitude and whether anything came out non-finite
    (an fp16 intermediate that overflowed)."""

    def __init__(self):
        self.max_abs, self.finite = 0.0, True

    def note(self, y):
        ok = torch.isfinite(y)
        if not bool(ok.all()):
            self.finite = False
        if bool(ok.any()):
            self.max_abs = max(self.max_abs, float(y[ok].abs().max()))


@contextlib.contextmanager
def rounding(dtype):
    """orc._r16 rounds to `dtype` (torch.bfloat16 or torch.float16) inside the block and is restored on exit.  Yields a Seen."""
    saved, seen = orc._r16, Seen()

    def r16(x):
        y = x.to(dtype).to(torch.float32)
        seen.note(y)
        return y
    orc._r16 = r16
    try:
        yield seen
    finally:
        orc._r16 = saved


@contextlib.contextmanager
def halves_order():
    """Every F.linear with K >= 64 computes the same products as two half-K sums (test_sampler_fast_mode_vs_bf16_emulating_oracle)."""
    plain = F.linear

    def halves(x, w, b=None):
        k = w.shape[1]
        if k < 64:
            return plain(x, w, b)
        y = plain(x[..., :k // 2], w[:, :k // 2]) + plain(x[..., k // 2:], w[:, k // 2:])
        return y if b is None else y + b
    F.linear = halves
    try:
        yield
    finally:
        F.linear = plain


def figures(got: torch.Tensor, ref64: torch.Tensor) -> Tuple[float, float]:
    e = tensor_error(got, ref64)
    return e.norm_rel, e.max_rms


def _spread(emu_h, emu, ref64) -> Tuple[float, float]:
    e, h = figures(emu, ref64), figures(emu_h, ref64)
    return h[0] / e[0], h[1] / e[1]


class Refs(NamedTuple):
    out64: torch.Tensor               # (B, H, F, J, 3) fp64
    emu: torch.Tensor                 # the 2-byte emulation in its plain accumulation order, as fp64
    emu_h: torch.Tensor               # ... with every Linear's K split in halves
    e16: Tuple[float, float]
    spread: Tuple[float, float]
    finite: bool                      # every value the emulations rounded to the type stayed finite
    max_abs: float                    # the largest of them


class SampleRefs(NamedTuple):
    out64: torch.Tensor               # (B, K, H, F, J, 3) fp64
    emu: torch.Tensor
    emu_h: torch.Tensor
    e16: List[Tuple[float, float]]    # one per step k, of out[:, k]
    spread: List[Tuple[float, float]]
    finite: bool
    max_abs: float


def denoise_fp64(sd, x2d, x3d, t, dep) -> torch.Tensor:
    with torch.no_grad():
        return orc.mixste_forward(_params(sd, torch.float64), x2d, x3d, t, dep).double()


def denoise_refs(sd, x2d, x3d, t, dep, dtype, out64: Optional[torch.Tensor] = None) -> Refs:
    """The fp64 `mixste_forward` (eval branch) of one case, its emulation in `dtype` under both accumulation orders, e16 and spread.
    x2d (B, F, J, 2), x3d (B, H, F, J, 3), t (B,) int64.  `out64`: the fp64 run where the caller has it already (it does not depend
    on the type)."""
    o64 = denoise_fp64(sd, x2d, x3d, t, dep) if out64 is None else out64
    p = orc.emulate_bf16(_params(sd, torch.float32))
    with torch.no_grad(), rounding(dtype) as seen:
        emu = orc.mixste_forward(p, x2d, x3d, t, dep).double()
        with halves_order():
            emu_h = orc.mixste_forward(p, x2d, x3d, t, dep).double()
    return Refs(o64, emu, emu_h, figures(emu, o64), _spread(emu_h, emu, o64), seen.finite, seen.max_abs)


def _sample(p, x2d, noises, H, K, dep, dtype):
    x2d = torch.as_tensor(x2d)
    with torch.no_grad():
        return orc.ddim_sample_flip(p, orc.cosine_schedule(1000), x2d.to(dtype), flip_2d(x2d).to(dtype), H, K, dep, H36M_JOINTS_LEFT,
                                    H36M_JOINTS_RIGHT, [n.to(dtype) for n in noises]).double()


def sample_fp64(sd, x2d, noises, H, K, dep) -> torch.Tensor:
    return _sample(_params(sd, torch.float64), x2d, noises, H, K, dep, torch.float64)


def sample_refs(sd, x2d, noises: Sequence[torch.Tensor], H, K, dep, dtype, out64: Optional[torch.Tensor] = None) -> SampleRefs:
    """The same for `ddim_sample_flip` (flip test-time augmentation, the recorded `noises`): out (B, K, H, F, J, 3), one e16 and one
    spread per step k."""
    o64 = sample_fp64(sd, x2d, noises, H, K, dep) if out64 is None else out64
    p = orc.emulate_bf16(_params(sd, torch.float32))
    with rounding(dtype) as seen:
        emu = _sample(p, x2d, noises, H, K, dep, torch.float32)
        with halves_order():
            emu_h = _sample(p, x2d, noises, H, K, dep, torch.float32)
    return SampleRefs(o64, emu, emu_h, [figures(emu[:, k], o64[:, k]) for k in range(K)],
                      [_spread(emu_h[:, k], emu[:, k], o64[:, k]) for k in range(K)], seen.finite, seen.max_abs)


def admissible(spread: Tuple[float, float]) -> bool:
    return spread[0] <= ADMIT_SPREAD[0] and spread[1] <= ADMIT_SPREAD[1]


def bounds(e16: Tuple[float, float]) -> Tuple[float, float]:
    return NORM16 * e16[0], MAX16 * e16[1]


def check(tag: str, got: torch.Tensor, ref64: torch.Tensor, e16: Tuple[float, float], pass_seqs: int = 0):
    """-> (one line with both figures, their ratios to e16 and the worst element; [violation lines]; Err) of one output against
    NORM16 x e16 in norm_rel and MAX16 x e16 in max_rms.  The worst element (for a non-finite output: the first non-finite one) is
    (b, h, f, j, c) with its pass row for a (B, H, F, J, 3) output, row and column for a single op's matrix."""
    e = tensor_error(got, ref64)
    label = "worst at " + (locate(e.worst, e.shape, pass_seqs or FAST_PASS_SEQS) if len(e.shape) == 5 else e.where())
    line = (f"{tag}: norm_rel {e.norm_rel:.2e} (e16 {e16[0]:.2e}, ratio {e.norm_rel / e16[0]:.2f}); max_rms {e.max_rms:.2e} "
            f"(e16 {e16[1]:.2e}, ratio {e.max_rms / e16[1]:.2f}), {label}")
    bad = violations({label: e}, bounds(e16), factor=1.0)       # (its "x e32" reads: x the bound)
    return line, [f"outside ({NORM16:g}, {MAX16:g}) x e16 -- " + b for b in bad], e


# ------------------------------------------------------------------------------------------------ the single-op models
def rnd(x: torch.Tensor, dtype) -> torch.Tensor:
    """One rounding to the 2-byte type (from the nearest fp32, as the kernels round their fp32 values), as fp64."""
    return x.to(torch.float32).to(dtype).double()


class OpRefs(NamedTuple):
    model: torch.Tensor               # the kernel's documented roundings on fp64 arithmetic
    exact: torch.Tensor               # the same operands, no rounding
    e16: Tuple[float, float]


def _op(model, exact) -> OpRefs:
    return OpRefs(model, exact, figures(model, exact))


def linear_model(A: torch.Tensor, W: torch.Tensor, bias: torch.Tensor, epi: int, dtype) -> OpRefs:
    """The streaming Linear (gemm.hip): A (M, K) and W (N, K) already rounded to `dtype`, fp32 bias.  EPI_BIAS: one rounding of
    acc + bias to the type -- the fp32-output form keeps finished tiles in the operand type too, so it has the same model.  EPI_GELU:
    the kernel parks acc + bias as FP16 in front of the nonlinearity in both types (gemm.hip, "the parked pre-activation is fp16, not
    bf16"; the scaled form of gemm_stream_scaled.hip parks the same value at its power of two), then rounds the kernels' polynomial
    GELU (orc.gelu_fast) of it to the type: two roundings, an eighth of the output's in front of it for bf16, one of the same size for
    fp16 (without it the fp16 kernel sits at 1.40 ... 1.48 x this model's norm figure: profiles/fast_elementwise.md)."""
    pre = A.double() @ W.double().t() + bias.double()
    if epi == EPI_BIAS:
        return _op(rnd(pre, dtype), pre)
    assert epi == EPI_GELU
    return _op(rnd(orc.gelu_fast(rnd(pre, torch.float16)), dtype), orc.gelu_fast(pre))


def _heads(qkv, n_bh, Fr, J, C, heads, axis):
    hd = C // heads
    x = qkv.double().reshape(n_bh, Fr, J, 3, heads, hd)
    perm = (0, 1, 3, 2, 4) if axis == 0 else (0, 2, 3, 1, 4)
    return tuple(x[:, :, :, i].permute(*perm) for i in range(3))


def attention_model(qkv: torch.Tensor, n_bh: int, Fr: int, J: int, C: int, heads: int, axis: int, dtype) -> OpRefs:
    """attention_fast.hip / orc.attention_bf16 on the (n_bh, F, J, 3 C) row layout, `qkv` already rounded to `dtype` (axis 0:
    sequences over joints, 1: over frames): p = exp(s - rowmax) with s = q k^T (C / heads)^-0.5, rounded to the type in front of
    P.V; the denominator is the sum of the unrounded p; the output is rounded once.  For padded heads pass the TRUE columns (C / heads
    = the true head dim); for scaled rows pass the values the rows stand for (2^s x the rows) and compare 2^s x the kernel's output."""
    q, k, v = _heads(qkv, n_bh, Fr, J, C, heads, axis)
    s = q @ k.transpose(-1, -2) * (C // heads) ** -0.5
    p = torch.exp(s - s.amax(dim=-1, keepdim=True))
    den = p.sum(dim=-1, keepdim=True)

    def rows(o):
        o = o.permute(0, 1, 3, 2, 4) if axis == 0 else o.permute(0, 3, 1, 2, 4)
        return o.reshape(n_bh * Fr * J, C)
    return _op(rows(rnd(rnd(p, dtype) @ v / den, dtype)), rows(p @ v / den))


def layernorm_model(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float, dtype) -> OpRefs:
    """The row kernels with 2-byte rows out: an fp32 LayerNorm of fp32 rows, rounded once."""
    exact = F.layer_norm(x.double(), (x.shape[-1],), w.double(), b.double(), eps)
    return _op(rnd(exact, dtype), exact)
