"""Element-by-element check of training gradients against the oracle's fp64 autograd (CPU only).

The bound is derived from the reference alone: for one case, `e32` is how far the oracle's own fp32 autograd lies from its fp64
autograd (the worst parameter, in each of the two figures below), and a gradient under test must lie within FACTOR x e32 of the
fp64 gradient in both.  FACTOR = 8 is three bits: a split-fp16 operand carries 22 significant bits against fp32's 24, and
test_linear_split_f16_is_fp32_class asserts 2^-21 for the split product against fp32's 2^-24 rounding.

  norm_rel = ||g - r|| / ||r||          the whole-tensor figure the older tests use (bound there: 2e-3 / 5e-3)
  max_rms  = max|g - r| / rms(r)        the per-element figure: one wrong 16-row tile moves it, not the norm

A case is admissible only if the reference itself is well-conditioned: e32(norm_rel) <= ADMIT_NORM_REL and e32(max_rms) <=
ADMIT_MAX_RMS (otherwise 8 x e32 says nothing about the kernels).  A parameter whose fp64 gradient is identically zero (a branch
DropPath dropped for every sample) must come back identically zero, which is checked by equality."""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

from . import d3dp_oracle as orc

FACTOR = 8.0
ADMIT_NORM_REL = 2e-6
ADMIT_MAX_RMS = 5e-5
PREDICTION = "<prediction>"


def reference_grads(sd, x2d, gt, t, noise, dep, droppath, dtype, upstream_scale=1.0):
    """One training step through the oracle in `dtype`: ({name: grad.double()}, prediction.double()).  `t` is (B, 1) as the model
    takes it; the upstream gradient of the MPJPE loss is the loss itself (as the trainer's) times `upstream_scale`."""
    p = {k: v.detach().clone().requires_grad_(True) for k, v in orc.strip_prefix(sd, dtype=dtype).items()}
    xp = orc.prepare_targets(orc.cosine_schedule(1000), gt, t[:, 0], noise)
    pred = orc.mixste_forward(p, x2d, xp, t[:, 0], dep, droppath=droppath)
    loss = torch.mean(torch.norm(pred - gt, dim=-1))
    loss.backward(loss.detach() * upstream_scale)
    return {k: v.grad.double() for k, v in p.items() if v.grad is not None}, pred.detach().double()


class Err(NamedTuple):
    norm_rel: float
    max_rms: float
    worst: int            # flat index of the element with the largest |g - r|
    shape: Tuple[int, ...]
    zero_ref: bool        # the fp64 gradient is identically zero: the figures are 0 (identically zero, finite) or inf

    def where(self) -> str:
        if len(self.shape) == 2:
            return f"row {self.worst // self.shape[1]} col {self.worst % self.shape[1]} of {self.shape[0]} x {self.shape[1]}"
        return f"element {self.worst} of {tuple(self.shape)}"


def tensor_error(g: torch.Tensor, r: torch.Tensor) -> Err:
    g, r = g.detach().double().cpu(), r.double()
    assert g.shape == r.shape, (g.shape, r.shape)
    shape = tuple(r.shape)
    if not bool(torch.isfinite(g).all()):
        bad = int((~torch.isfinite(g)).reshape(-1).nonzero()[0])
        return Err(float("inf"), float("inf"), bad, shape, not bool(r.any()))
    d = (g - r).reshape(-1)
    worst = int(d.abs().argmax())
    if not bool(r.any()):
        ok = not bool(g.any())
        return Err(0.0 if ok else float("inf"), 0.0 if ok else float("inf"), worst, shape, True)
    rms = r.pow(2).mean().sqrt().item()
    return Err(d.norm().item() / r.norm().item(), d.abs().max().item() / rms, worst, shape, False)


def grad_errors(got: Dict[str, torch.Tensor], ref64: Dict[str, torch.Tensor]) -> Dict[str, Err]:
    """Both figures and the worst element's flat index for every tensor of `got` (each must have its fp64 reference)."""
    return {k: tensor_error(g, ref64[k]) for k, g in got.items()}


def worst_of(errs: Dict[str, Err]) -> Tuple[float, float, str, str]:
    """(worst norm_rel, worst max_rms, the parameter of each)."""
    kn = max(errs, key=lambda k: errs[k].norm_rel)
    km = max(errs, key=lambda k: errs[k].max_rms)
    return errs[kn].norm_rel, errs[km].max_rms, kn, km


def e32_of(ref32: Dict[str, torch.Tensor], ref64: Dict[str, torch.Tensor]) -> Tuple[float, float]:
    """The oracle's own fp32 autograd against its fp64 autograd: the worst parameter in each figure."""
    n, m, _, _ = worst_of(grad_errors(ref32, ref64))
    return n, m


def admissible(e32: Tuple[float, float]) -> bool:
    return e32[0] <= ADMIT_NORM_REL and e32[1] <= ADMIT_MAX_RMS


def violations(errs: Dict[str, Err], e32: Tuple[float, float], factor: float = FACTOR) -> List[str]:
    """One line per tensor outside factor x e32 in either figure (NaN counts as outside), naming the worst element."""
    out = []
    for k, e in errs.items():
        if e.zero_ref:
            if e.norm_rel != 0.0:
                out.append(f"{k}: the fp64 gradient is identically zero, the gradient under test is not ({e.where()})")
            continue
        if not (e.norm_rel <= factor * e32[0]) or not (e.max_rms <= factor * e32[1]):
            out.append(f"{k}: norm_rel {e.norm_rel:.2e} ({e.norm_rel / e32[0]:.1f} x e32), max_rms {e.max_rms:.2e} "
                       f"({e.max_rms / e32[1]:.1f} x e32), worst at {e.where()}")
    return out


def report(tag: str, errs: Dict[str, Err], e32: Tuple[float, float]) -> str:
    n, m, kn, km = worst_of({k: e for k, e in errs.items() if not e.zero_ref} or errs)
    zeros = sum(e.zero_ref for e in errs.values())
    return (f"{tag}: norm_rel {n:.2e} (e32 {e32[0]:.2e}, ratio {n / e32[0]:.2f}, {kn}); max_rms {m:.2e} (e32 {e32[1]:.2e}, "
            f"ratio {m / e32[1]:.2f}, {km}, {errs[km].where()}); {zeros} exactly-zero references")


class Reference(NamedTuple):
    g64: Dict[str, torch.Tensor]
    g32: Dict[str, torch.Tensor]
    pred64: torch.Tensor
    pred32: torch.Tensor
    e32: Tuple[float, float]


def reference_pair(sd, x2d, gt, t, noise, dep, droppath, upstream_scale=1.0) -> Reference:
    """The fp64 and the fp32 oracle step of one case, and the e32 they define."""
    g64, p64 = reference_grads(sd, x2d, gt, t, noise, dep, droppath, torch.float64, upstream_scale)
    g32, p32 = reference_grads(sd, x2d, gt, t, noise, dep, droppath, torch.float32, upstream_scale)
    return Reference(g64, g32, p64, p32, e32_of(g32, g64))
