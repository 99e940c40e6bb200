"""CPU reference of the kernels AROUND the denoiser, one step at a time -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The sampler glue (csrc/sampler.hip: ddim_pre / ddim_post / q_sample) and JPMA (csrc/jpma.hip, jpma_combine in
csrc/caller.hip) carry no tolerance of their own: what they owe the reference is its arithmetic, operation by operation
(fp32 without contraction, fp64 where the schedule buffers promote, torch.clamp / torch.min semantics).  So they are
compared BIT FOR BIT (``bits_equal``) with the functions below, which are the expressions of oracle/d3dp_oracle.py
(``model_predictions_flip``, ``predict_noise_from_start``, the update at the end of ``ddim_sample_flip``) and of
d3dp_amd/jpma.py (``reproject``, ``jpma_metrics``, ``jpma_aggregate``) cut at the kernel boundaries, in plain torch on
the CPU and with no denoiser.  tests/test_glue_host.py ties them back to the whole-sampler oracle and to fixture g5;
tests/test_hip_glue.py runs the kernels against them.  ``q_sample`` needs nothing here: d3dp_oracle.prepare_targets is
its reference.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch

from d3dp_amd import jpma as _jpma
from oracle import d3dp_oracle as orc

Tensor = torch.Tensor


# --------------------------------------------------------------------------------------
# comparison
# --------------------------------------------------------------------------------------
def bit_mismatches(a: Tensor, b: Tensor) -> int:
    """Number of elements at which ``a`` and ``b`` differ as bit patterns, NaN payloads aside: where exactly one of
    them is NaN, or neither is and the integer views differ (so +0.0 != -0.0).  Shapes and dtypes must agree."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if not a.dtype.is_floating_point:
        return int((a != b).sum())
    iv = {torch.float32: torch.int32, torch.float64: torch.int64}[a.dtype]
    na, nb = torch.isnan(a), torch.isnan(b)
    return int(((na != nb) | (~na & ~nb & (a.view(iv) != b.view(iv)))).sum())


def bits_equal(a: Tensor, b: Tensor) -> bool:
    """The NaN masks are equal and everywhere else the integer views are: the sign of zero counts."""
    return bit_mismatches(a, b) == 0


# --------------------------------------------------------------------------------------
# the sampler, cut where the kernels cut it
# --------------------------------------------------------------------------------------
def ddim_pre_ref(img: Tensor, scale: float, joints_left: List[int], joints_right: List[int]) -> Tuple[Tensor, Tensor]:
    """First two lines of ``model_predictions_flip``: (x_t, x_t_flip)."""
    x_t = torch.clamp(img, min=-1.1 * scale, max=1.1 * scale) / scale
    return x_t, orc.flip_pose(x_t, joints_left, joints_right)


def ddim_post_ref(pred: Tensor, pred_flip: Tensor, img: Tensor, noise: Optional[Tensor], sched, time: int,
                  time_next: int, scale: float, eta: float, joints_left: List[int],
                  joints_right: List[int]) -> Tuple[Tensor, Optional[Tensor]]:
    """The rest of ``model_predictions_flip`` and the update of ``ddim_sample_flip``: (x_start, img_next).
    ``pred_flip`` is the denoiser's raw output for the flipped input (it is flipped back here); ``img_next`` is None
    on the last step (``time_next < 0``), where the reference keeps x_start."""
    pred = (pred + orc.flip_pose(pred_flip, joints_left, joints_right)) / 2
    x_start = torch.clamp(pred * scale, min=-1.1 * scale, max=1.1 * scale)
    if time_next < 0:
        return x_start, None
    t = torch.full((img.shape[0],), time, dtype=torch.long)
    pred_noise = orc.predict_noise_from_start(sched, img, t, x_start).to(img.dtype)
    ac = sched["alphas_cumprod"]
    alpha, alpha_next = ac[time], ac[time_next]
    sigma = eta * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
    c = (1 - alpha_next - sigma ** 2).sqrt()
    return x_start, x_start * alpha_next.sqrt() + c * pred_noise + sigma * noise


def ddim_loop_ref(denoiser, sched, x2d: Tensor, x2d_flip: Tensor, sampling_timesteps: int, joints_left, joints_right,
                  noises: Sequence[Tensor], scale: float = 1.0, eta: float = 1.0) -> Tensor:
    """``ddim_sample_flip`` as the composition ddim_pre_ref -> denoiser(x2d, x_t, t) twice -> ddim_post_ref."""
    img = noises[0].clone()
    preds, draw = [], 1
    for time, time_next in orc.time_pairs(sampling_timesteps):
        t = torch.full((img.shape[0],), time, dtype=torch.long)
        x_t, x_t_flip = ddim_pre_ref(img, scale, joints_left, joints_right)
        nz = None
        if time_next >= 0:
            nz = noises[draw]
            draw += 1
        x_start, img_next = ddim_post_ref(denoiser(x2d, x_t, t), denoiser(x2d_flip, x_t_flip, t), img, nz, sched, time,
                                          time_next, scale, eta, joints_left, joints_right)
        preds.append(x_start)
        img = x_start if img_next is None else img_next
    return torch.stack(preds, dim=1)


# A denoiser that is exactly reproducible on any device: three elementwise fp32 operations, each correctly rounded
# on its own when issued as separate eager torch ops.  The table is not symmetric under any left/right swap and, added
# to 0.5 x_t (|x_t| <= 1.1), drives part of the output past the +-1.1 clamp.
_TAB = [[1.4 * math.sin(1.7 * j + 2.3 * c + 0.5) for c in range(3)] for j in range(17)]
_TAB[3][0], _TAB[12][1] = 1.4, -1.4
STUB_TAB = torch.tensor(_TAB, dtype=torch.float32)


def stub_denoiser(x2d: Tensor, x_t: Tensor, t: Tensor) -> Tensor:
    """f(x2d (B,F,J,2), x_t (B,H,F,J,3), t) = (0.5 x_t + tab[j, c]) + 0.25 x2d[..., j, 0], broadcast over H and c."""
    a = 0.5 * x_t
    a = a + STUB_TAB.to(x_t.device)
    b = 0.25 * x2d[:, None, :, :, 0:1].to(torch.float32)
    return a + b


# --------------------------------------------------------------------------------------
# JPMA
# --------------------------------------------------------------------------------------
def project_linear(X: Tensor, cam: Tensor) -> Tensor:
    """f * clamp(X / Z, -1, 1) + c: the pinhole projection csrc/jpma.hip runs with ``linear``."""
    f, c = cam[:2], cam[2:4]
    XX = torch.clamp(X[..., :2] / X[..., 2:], min=-1, max=1)
    return f * XX + c


def _reproject(p: Tensor, traj: Tensor, cam: Tensor, linear: bool) -> Tensor:
    B, Fr = p.shape[0], p.shape[3]
    traj = traj.reshape(B, Fr, 1, 3)
    cam = cam.reshape(-1)[:9]
    return project_linear(p + traj[:, None, None], cam) if linear else _jpma.reproject(p, traj, cam)


def _zero_root(pred: Tensor, root_joint: int) -> Tensor:
    p = pred.clone().float()
    if root_joint >= 0:
        p[:, :, :, :, root_joint] = 0
    return p


def _take(x: Tensor, idx: Tensor) -> Tensor:
    """x (B,K,H,F,J,3) at idx (B,K,1,F,J) along H -> (B,K,F,J,3)."""
    return torch.gather(x, 2, idx[..., None].expand(-1, -1, -1, -1, -1, 3))[:, :, 0]


def jpma_ref(pred: Tensor, traj: Tensor, cam: Tensor, gt2d: Tensor, gt3d: Tensor, root_joint: int, linear: bool):
    """pred (B,K,H,F,J,3), traj (B,F,1,3) or (B,F,3), cam (9,), gt2d (B,F,J,2), gt3d (B,F,J,3), all fp32 ->
    agg (B,K,F,J,3), sel (B,K,F,J) int32, err_sel, err_min (B,K,F,J), jbest (B,K,F,J,3), mean64 (B,K,F,J,3) fp64.
    The selections are what jpma_metrics / jpma_aggregate state: torch.norm, torch.min over H, torch.gather."""
    p = _zero_root(pred, root_joint)
    err2d = torch.norm(_reproject(p, traj.float(), cam.float(), linear) - gt2d[:, None, None], dim=-1)
    err = torch.norm(p - gt3d[:, None, None], dim=-1)                          # (B,K,H,F,J)
    sel = err2d.min(dim=2, keepdim=True).indices
    agg = _take(p, sel)
    err_sel = torch.gather(err, 2, sel)[:, :, 0]
    emin, jsel = err.min(dim=2, keepdim=True)
    return agg, sel[:, :, 0].to(torch.int32), err_sel, emin[:, :, 0], _take(p, jsel), p.double().mean(dim=2)


def jpma_winners_ref(pred: Tensor, traj: Tensor, cam: Tensor, gt2d: Tensor, root_joint: int, linear: bool,
                     h_offset: int = 0) -> Tensor:
    """(B,K,F,J,5): the smallest 2D error, its pose and the int32 bits of ``h_offset`` + its hypothesis index."""
    p = _zero_root(pred, root_joint)
    err2d = torch.norm(_reproject(p, traj.float(), cam.float(), linear) - gt2d[:, None, None], dim=-1)
    e, sel = err2d.min(dim=2, keepdim=True)
    hbits = (sel[:, :, 0] + h_offset).to(torch.int32).view(torch.float32)
    return torch.cat((e[:, :, 0, ..., None], _take(p, sel), hbits[..., None]), dim=-1).contiguous()


def mean_bound(pred: Tensor, root_joint: int) -> Tensor:
    """Bound on |mean - mean64| for a sequential fp32 sum of the H hypotheses followed by one division: every one of
    the H roundings is at most 2^-24 relative to a partial result no larger than sum_h |x_h| = H mean_h |x_h|."""
    p = _zero_root(pred, root_joint).double()
    return 2.0 ** -24 * p.shape[2] * p.abs().mean(dim=2) * 1.001


def clamp_bound_table(scales: Sequence[float]) -> List[float]:
    """The scales at which the reference's bound fp32(1.1 * s), a Python double rounded once, is not the fp32 product
    fp32(1.1) * fp32(s)."""
    out = []
    for s in scales:
        ref = torch.tensor(1.1 * s, dtype=torch.float64).to(torch.float32)
        f32 = torch.tensor(1.1, dtype=torch.float32) * torch.tensor(s, dtype=torch.float32)
        if ref.item() != f32.item():
            out.append(s)
    return out
