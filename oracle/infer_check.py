"""Element-by-element check of EXACT inference against the oracle's fp64 forward pass (CPU only).

Every gate EXACT mode has at denoiser and sampler level is `mpjpe_mm(...) <= 1e-3`, a MEAN over all B H F 17 joints of the output:
one wrong 16-row tile, one (sequence, head) problem of the persistent attention kernel, the rows of one pass or one lost split-fp16
pass in one tile class are averaged away.  Here the reference is the oracle in fp64, the comparator is grad_check's (the norm figure
and the per-element figure `max_rms = max|y - r| / rms(r)`), and the bound is the same: within FACTOR x e32 of fp64 in both, where
`e32` is how far the oracle's OWN fp32 evaluation of the same case lies from its fp64 one -- it comes from the reference alone (the
rationale for FACTOR = 8, 22 against 24 significant bits, is in grad_check.py).  A case is admissible only if e32 is within
grad_check's caps.

The worst element is named as (b, h, f, j, c) with its token row inside its pass: the denoiser lays a pass out as its sequences
(b, h) one after the other, F J rows each, row f J + j; that row / 16 is the row tile, / 256 the Linear's tile.  (Passes are taken
as uniform, `pass_seqs` sequences each; where the library's pass plan splits a batch otherwise, the row within the sequence --
the pass row modulo F J -- still holds.)"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Sequence, Tuple

import torch

from d3dp_amd.weights import H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, flip_2d

from . import d3dp_oracle as orc
from .grad_check import ADMIT_MAX_RMS, ADMIT_NORM_REL, FACTOR, Err, admissible, report, tensor_error, violations  # noqa: F401

DEFAULT_PASS_SEQS = 31          # EXACT contexts: sequences per pass unless chunk_seqs says otherwise (csrc/ctx.h: chunk())


class Pair(NamedTuple):
    out64: torch.Tensor               # (B, H, F, J, 3) fp64
    out32: torch.Tensor               # the same case through the oracle in fp32, as fp64
    e32: Tuple[float, float]


class SamplePair(NamedTuple):
    out64: torch.Tensor               # (B, K, H, F, J, 3) fp64
    out32: torch.Tensor
    e32: List[Tuple[float, float]]    # one per step k, of out[:, k]


def _params(sd, dtype):
    """The oracle's parameter dict in `dtype` from a state dict with or without the `pose_estimator.` prefix."""
    if any(k.startswith("pose_estimator.") or k.startswith("module.") for k in sd):
        return orc.strip_prefix(sd, dtype=dtype)
    return {k: v.to(dtype) for k, v in sd.items()}


def e32_of(out32: torch.Tensor, out64: torch.Tensor) -> Tuple[float, float]:
    e = tensor_error(out32, out64)
    return e.norm_rel, e.max_rms


def denoise_pair(sd, x2d, x3d, t, dep) -> Pair:
    """The fp64 and the fp32 `mixste_forward` (eval branch) of one case and the e32 they define.  x2d (B, F, J, 2), x3d
    (B, H, F, J, 3), t (B,) int64."""
    with torch.no_grad():
        o64 = orc.mixste_forward(_params(sd, torch.float64), x2d, x3d, t, dep).double()
        o32 = orc.mixste_forward(_params(sd, torch.float32), x2d, x3d, t, dep).double()
    return Pair(o64, o32, e32_of(o32, o64))


def sample_pair(sd, x2d, noises: Sequence[torch.Tensor], H, K, dep) -> SamplePair:
    """The same for `ddim_sample_flip` (flip test-time augmentation, the recorded `noises`): out (B, K, H, F, J, 3), one e32 per
    step k.  The fp64 run takes the noise draws as fp64 too (an exact conversion), so that nothing on its path is rounded to fp32."""
    x2d = torch.as_tensor(x2d)
    sched = orc.cosine_schedule(1000)

    def run(dtype):
        with torch.no_grad():
            return orc.ddim_sample_flip(_params(sd, dtype), sched, x2d.to(dtype), flip_2d(x2d).to(dtype), H, K, dep,
                                        H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, [n.to(dtype) for n in noises]).double()
    o64, o32 = run(torch.float64), run(torch.float32)
    return SamplePair(o64, o32, [e32_of(o32[:, k], o64[:, k]) for k in range(K)])


def locate(flat: int, shape: Tuple[int, ...], pass_seqs: int = 0) -> str:
    """The element `flat` of a (B, H, F, J, 3) output as (b, h, f, j, c), with the token row inside its pass (passes of `pass_seqs`
    sequences, 0: the default) and that row's 16-row tile."""
    B, H, F, J, Cc = shape
    c = flat % Cc
    j = flat // Cc % J
    f = flat // (Cc * J) % F
    h = flat // (Cc * J * F) % H
    b = flat // (Cc * J * F * H)
    seq = b * H + h
    n = pass_seqs or DEFAULT_PASS_SEQS
    row = (seq % n) * F * J + f * J + j
    return f"(b, h, f, j, c) = ({b}, {h}, {f}, {j}, {c}), row {row} of pass {seq // n} (16-row tile {row // 16})"


def output_errors(got: torch.Tensor, ref64: torch.Tensor, pass_seqs: int = 0) -> Dict[str, Err]:
    """{label: Err} of one output for grad_check's `violations` / `report`; the label is the worst element's position (for a
    non-finite output: the first non-finite element's) -- (b, h, f, j, c) and its pass row for a (B, H, F, J, 3) output, row and
    column for a single op's matrix."""
    e = tensor_error(got, ref64)
    return {"worst at " + (locate(e.worst, e.shape, pass_seqs) if len(e.shape) == 5 else e.where()): e}


def check(tag: str, got: torch.Tensor, ref64: torch.Tensor, e32: Tuple[float, float], pass_seqs: int = 0):
    """-> (one line with both figures, their ratios to e32 and the worst element; [violation lines]; Err) of one output against
    FACTOR x e32 in both figures."""
    errs = output_errors(got, ref64, pass_seqs)
    (label, e), = errs.items()
    line = (f"{tag}: norm_rel {e.norm_rel:.2e} (e32 {e32[0]:.2e}, ratio {e.norm_rel / e32[0]:.2f}); max_rms {e.max_rms:.2e} "
            f"(e32 {e32[1]:.2e}, ratio {e.max_rms / e32[1]:.2f}), {label}")
    return line, violations(errs, e32), e
