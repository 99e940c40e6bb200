"""CPU emulation of the one-pass training Linears (D3DP_TRAIN_PASSES=1) and the references the two test files of the route share
(tests/test_train_passes_host.py, tests/test_hip_train_passes.py).  Test infrastructure: nothing in d3dp_amd imports it.

The route (d3dp_amd/csrc/gemm_x2_train.hip, PASSES = 1) keeps of every split operand the hi plane alone, which is the tensor rounded
to IEEE fp16 at the power of two its own absmax asks for (dyn_scale: the absmax lands in [2^13, 2^14)):

    r(x) = fp16(x s) / s,   s = 2^(14 - e)  with  absmax = f 2^e, f in [0.5, 1);   s = 1 for an all-zero tensor.

`one_pass_linears()` replaces torch.nn.functional.linear, the way oracle/lowp_check.halves_order does, by an autograd Function for
the Linears that go through X2Train in d3dp_amd/csrc/capi_train.hip -- qkv, proj, fc1 and fc2 of every block (x2_linears() reads
them from that file): forward r(X) r(W)^T + b, dgrad r(dY) r(W), wgrad r(dY)^T r(X), dY rounded once, the bias gradient from the
unrounded dY (the operand pass sums its fp32 input).  Everything else -- the embedding, the time MLP, the head, attention, LayerNorm,
GELU, the residual stream -- stays plain fp32.  The oracle feeds its blocks 3-d activations (sequences, tokens, C) and the time MLP
2-d ones (B, C): together with the shapes of the block weights, which x2_linears() names, that tells the Linears apart without a
guess about which weight tensor a call received.  order="halves": every product of the emulated Linears as two half-contraction
sums -- the second accumulation order of the admissibility check."""
from __future__ import annotations

import contextlib
import os
import re
from functools import lru_cache
from typing import Dict, NamedTuple, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from d3dp_amd.weights import make_state_dict, synthetic_inputs_2d, synthetic_noise
from oracle import caller_oracle as co
from oracle import d3dp_oracle as orc
from oracle import grad_check as gc
from oracle import lowp_check as lc
from test_hip_train_grads import Case, problem

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "D3DP_TRAIN_PASSES"

# The GPU cases of the training step (tests/test_hip_train_passes.py): J = 17, B = 2, dep = 2, recorded DropPath masks on the
# blocks behind the first -- each is shown admissible on a CPU by tests/test_train_passes_host.py.
STEP_CASES = [
    Case(512, 9, 2),      # T = 306 rows: 256-row tiles and the 16 x 64 remainder blocks
    Case(256, 27, 2),
    Case(128, 9, 2),      # TN weight gradients where N % 256 == 0 and K % 128 == 0, transposed operands elsewhere
    Case(64, 9, 2),       # head dim 8: fp32 attention under one-pass Linears
    Case(192, 9, 2),      # D3DP_TRAIN_IMPL=f16x2 beside the switch
    Case(128, 300, 2),
]
DROPPED_CASE = Case(128, 9, 2, masks="dropped")
ALL_CASES = STEP_CASES + [DROPPED_CASE]


def dyn_scale(x: torch.Tensor) -> float:
    """gemm_x2_train.hip dyn_scale on the tensor's absmax."""
    m = float(x.detach().abs().max()) if x.numel() else 0.0
    if not (m > 0.0) or not np.isfinite(m):
        return 1.0
    _, e = np.frexp(np.float32(m))
    return float(2.0 ** (14 - int(e)))


def r16(x: torch.Tensor) -> torch.Tensor:
    """r(x): one rounding to fp16 at the tensor's own power-of-two scale (x s is exact in fp32)."""
    s = dyn_scale(x)
    return ((x.to(torch.float32) * s).to(torch.float16).to(torch.float32) / s).to(x.dtype)


def x2_linears() -> Tuple[str, ...]:
    """The Linears d3dp_train_forward hands to X2Train::forward, read from capi_train.hip: the TrainLinearId `kName` its
    `lin(blk, kName, ...)` calls name.  (The embedding, the time MLP and the head have launchers of their own there.)"""
    src = open(os.path.join(REPO, "d3dp_amd", "csrc", "capi_train.hip")).read()
    fwd = src[src.index("int d3dp_train_forward("):src.index("int d3dp_train_backward(")]
    names = sorted(set(n.lower() for n in re.findall(r"\blin\(blk, k(\w+),", fwd)))
    for other in ("d3dp_train_time_mlp(", "d3dp_launch_embed_ln(", "d3dp_train_head_linear("):
        assert other in fwd, other
    return tuple(names)


def _block_shapes(C: int):
    """(N, K) of the four block Linears x2_linears() names, at the model's mlp_ratio 2."""
    by_name = {"qkv": (3 * C, C), "proj": (C, C), "fc1": (2 * C, C), "fc2": (C, 2 * C)}
    return {by_name[n] for n in x2_linears()}


def _mm(a, b, halves):
    """a @ b, optionally as two half-contraction sums."""
    k = a.shape[-1]
    if not halves or k < 64:
        return a @ b
    return a[..., :k // 2] @ b[:k // 2] + a[..., k // 2:] @ b[k // 2:]


class _OnePass(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, halves):
        xr, wr = r16(x), r16(w)
        ctx.save_for_backward(xr, wr)
        ctx.halves, ctx.has_bias = halves, b is not None
        y = _mm(xr, wr.t(), halves)
        return y if b is None else y + b

    @staticmethod
    def backward(ctx, dy):
        xr, wr = ctx.saved_tensors
        dyr = r16(dy)                                            # once: dgrad and wgrad read the same operand rows
        dx = _mm(dyr, wr, ctx.halves)
        dy2, x2 = dyr.reshape(-1, dyr.shape[-1]), xr.reshape(-1, xr.shape[-1])
        dw = _mm(dy2.t(), x2, ctx.halves)
        db = dy.reshape(-1, dy.shape[-1]).sum(0) if ctx.has_bias else None
        return dx, dw, db, None


@contextlib.contextmanager
def one_pass_linears(order: str = "plain"):
    """F.linear -> the emulation for the block Linears of X2Train (3-d fp32 activations, a block weight's shape).  Yields the list
    of (N, K, emulated) of every call inside the block."""
    assert order in ("plain", "halves")
    plain, calls, shapes = F.linear, [], {}

    def linear(x, w, b=None):
        C = min(w.shape)
        if C not in shapes:
            shapes[C] = _block_shapes(C)
        emulated = x.dim() == 3 and x.dtype == torch.float32 and tuple(w.shape) in shapes[C] and w.shape[0] % 32 == 0 and w.shape[1] % 32 == 0
        calls.append((w.shape[0], w.shape[1], emulated))
        return _OnePass.apply(x, w, b, order == "halves") if emulated else plain(x, w, b)
    F.linear = linear
    try:
        yield calls
    finally:
        F.linear = plain


class StepRefs(NamedTuple):
    g64: Dict[str, torch.Tensor]          # fp64 autograd of the case; gc.PREDICTION holds the fp64 prediction
    e32: Tuple[float, float]              # the fp32 oracle against it (worst tensor, each figure)
    e1p: Tuple[float, float]              # the one-pass emulation against it
    spread: Tuple[float, float]           # the emulation under the second accumulation order, over e1p


def _worst(got, pred, want) -> Tuple[float, float]:
    n, m, _, _ = gc.worst_of({k: e for k, e in gc.grad_errors({**got, gc.PREDICTION: pred}, want).items() if not e.zero_ref})
    return n, m


@lru_cache(maxsize=None)
def step_refs(case) -> StepRefs:
    """Computed once per case and shared; never written to."""
    sd, x2d, gt, t, noise, dpd = problem(case)
    g64, p64 = gc.reference_grads(sd, x2d, gt, t, noise, case.dep, dpd, torch.float64)
    g32, p32 = gc.reference_grads(sd, x2d, gt, t, noise, case.dep, dpd, torch.float32)
    want = {**g64, gc.PREDICTION: p64}
    with one_pass_linears():
        ge, pe = gc.reference_grads(sd, x2d, gt, t, noise, case.dep, dpd, torch.float32)
    with one_pass_linears("halves"):
        gh, ph = gc.reference_grads(sd, x2d, gt, t, noise, case.dep, dpd, torch.float32)
    e1p, eh = _worst(ge, pe, want), _worst(gh, ph, want)
    return StepRefs(want, _worst(g32, p32, want), e1p, (eh[0] / e1p[0], eh[1] / e1p[1]))


# ---- the short run: 20 AdamW steps at cs 128, F 9, dep 2 from one seed ------------------------------------------------------------
RUN_CS, RUN_F, RUN_DEP, RUN_B, RUN_STEPS, RUN_BATCHES, RUN_SEED, RUN_LR = 128, 9, 2, 2, 20, 4, 31, 2e-4


def run_problem():
    """(state dict, [(gt (B, F, 17, 3), x2d (B, F, 17, 2))] x RUN_BATCHES, [(t (B,), noise)] x RUN_BATCHES): step i uses batch and
    draw i mod RUN_BATCHES, so that a falling loss is a property of the run and not of the order of the batches."""
    sd = make_state_dict(RUN_SEED, RUN_CS, RUN_DEP, RUN_F)
    batches, draws = [], []
    for i in range(RUN_BATCHES):
        x2d = synthetic_inputs_2d(RUN_SEED + 10 * i, RUN_B, RUN_F)
        gt = synthetic_noise(RUN_SEED + 10 * i + 1, (RUN_B, RUN_F, 17, 3)) * 0.3
        gt[:, :, 0] = 0
        batches.append((gt.astype(np.float32), x2d.astype(np.float32)))
        draws.append((np.array([30 + 100 * i, 700 - 100 * i]), synthetic_noise(RUN_SEED + 10 * i + 2, (RUN_B, RUN_F, 17, 3))))
    return sd, batches, draws


def _oracle_run(emulated: bool):
    sd, batches, draws = run_problem()
    seq = [batches[i % RUN_BATCHES] for i in range(RUN_STEPS)]
    dr = [draws[i % RUN_BATCHES] for i in range(RUN_STEPS)]
    with (one_pass_linears() if emulated else contextlib.nullcontext()):
        losses, _, _ = co.train_loop(orc.strip_prefix(sd, dtype=torch.float32), RUN_DEP, 1.0, seq, dr, RUN_LR, 1.0, RUN_STEPS)
    return losses


@lru_cache(maxsize=None)
def oracle_runs():
    """(losses of caller_oracle.train_loop in plain fp32, losses under the emulation)."""
    return _oracle_run(False), _oracle_run(True)
