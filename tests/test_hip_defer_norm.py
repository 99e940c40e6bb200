"""The deferred shared norm of EXACT mode (ctx.h d3dp_ctx::defer_norm): at a block boundary without Temporal_pos the norm pair
leaves x un-normalised and stores (mean, rstd) per row; the next block's proj applies the norm in its residual epilogue
(gemm_x2.hip EPI_RESID_NORM).  Same expression on the same fp32 values: every comparison here is ``torch.equal`` against
``D3DP_DEFER_NORM=0``, the in-place form.

Seed weights with dep=2: the boundary after STE block 0 adds Temporal_pos and stays in place, the two behind it (TTE 0 -> STE 1,
STE 1 -> TTE 1) are deferred.  The switch is read at d3dp_create, which the first call of a model runs: the environment is set
around the whole life of each model.
"""
import contextlib
import ctypes as C
import os
from types import SimpleNamespace

import pytest
import torch

from d3dp_amd import D3DP, _lib
from d3dp_amd.weights import (H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, flip_2d, make_state_dict, synthetic_inputs_2d,
                              synthetic_noise)

pytestmark = pytest.mark.gpu
DEP, SEED = 2, 7


@contextlib.contextmanager
def defer_norm(on):
    old = os.environ.get("D3DP_DEFER_NORM")
    if on:
        os.environ.pop("D3DP_DEFER_NORM", None)
    else:
        os.environ["D3DP_DEFER_NORM"] = "0"
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("D3DP_DEFER_NORM", None)
        else:
            os.environ["D3DP_DEFER_NORM"] = old


def make_model(frames, cs, H, K, chunk_seqs=0):
    args = SimpleNamespace(number_of_frames=frames, test_time_augmentation=True, timestep=1000, scale=1.0, cs=cs, dep=DEP,
                           chunk_seqs=chunk_seqs)
    m = D3DP(args, H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, is_train=False, num_proposals=H, sampling_timesteps=K,
             numerics="exact")
    m.load_state_dict(make_state_dict(SEED, cs, DEP, frames), strict=False)
    return m.cuda().eval()


def sample(on, frames, cs, B, H, K, chunk_seqs=0):
    """(output of D3DP.forward, d3dp_status flag) of a fresh model in the deferred (on) or the in-place form."""
    x2d = synthetic_inputs_2d(11, B, frames)
    x2f = flip_2d(x2d)
    noises = [torch.from_numpy(synthetic_noise(20 + k, (B, H, frames, 17, 3))) for k in range(K)]
    with defer_norm(on):
        m = make_model(frames, cs, H, K, chunk_seqs)
        out = m(torch.from_numpy(x2d).cuda(), None, input_2d_flip=torch.from_numpy(x2f).cuda(), noise=noises)
        torch.cuda.synchronize()
        assert m.pose_estimator.exact_scales()[2] == "f16x2"    # the split-fp16 Linears: the path the deferral lives on
        return out.cpu(), m.pose_estimator.nonfinite_seen()


# case 1 of every form, computed once: cs=512, F=9, B=1, H=3, K=2.  The sampler denoises the clip and its flip together: 6 sequences
# of 153 rows, in uniform passes of 4 and 2 (chunk_seqs=-4) -- 612 and 306 rows, neither a multiple of the 256-row tile.
CASE1 = dict(frames=9, cs=512, B=1, H=3, K=2, chunk_seqs=-4)


@pytest.fixture(scope="module")
def case1():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return {on: sample(on, **CASE1) for on in (True, False)}


def test_partial_tiles_and_several_passes(case1):
    """The checked epilogue (a last row of tiles with 100 / 50 live rows) and the statistics area reused by the second pass."""
    (a, _), (b, _) = case1[True], case1[False]
    assert a.shape == (1, 2, 3, 9, 17, 3) and torch.isfinite(a).all()
    assert torch.equal(a, b)


def test_whole_tiles():
    """F=16, B=1, H=8, K=1: 16 sequences x 272 rows = 17 whole 256-row tiles in one pass -- the unchecked epilogue alone."""
    a, fa = sample(True, 16, 512, 1, 8, 1)
    b, fb = sample(False, 16, 512, 1, 8, 1)
    assert torch.isfinite(a).all() and not fa and not fb
    assert torch.equal(a, b)


def test_another_width():
    """cs=128: one column tile, the k-loop of four k-steps, other gamma / beta columns per lane."""
    a, fa = sample(True, 9, 128, 1, 2, 1)
    b, fb = sample(False, 9, 128, 1, 2, 1)
    assert torch.isfinite(a).all() and not fa and not fb
    assert torch.equal(a, b)


def test_poisoned_workspace():
    """d3dp_denoise on a workspace full of NaN, at the shape of case 1: finite, and equal to the run on a zeroed workspace --
    every statistic (and every other workspace value) a pass reads was written in that pass."""
    frames, cs, H = CASE1["frames"], CASE1["cs"], CASE1["H"]
    B = 2                                                       # the clip and its flip, as the sampler calls the denoiser
    lib = _lib.load()
    x2d = torch.from_numpy(synthetic_inputs_2d(11, B, frames)).cuda().contiguous()
    x3d = torch.from_numpy(synthetic_noise(20, (B, H, frames, 17, 3))).cuda().contiguous()
    t = torch.tensor([999, 499], dtype=torch.int64, device="cuda")
    with defer_norm(True):
        m = make_model(frames, cs, H, 1, CASE1["chunk_seqs"])
        net = m.pose_estimator
        ctx = net._context(x3d.device)
        n = C.c_size_t()
        _lib.check(lib.d3dp_workspace_bytes(ctx, B, H, C.byref(n)), "d3dp_workspace_bytes")
        ws = torch.empty((n.value + 3) // 4, dtype=torch.float32, device="cuda")
        outs = []
        for fill in (float("nan"), 0.0):
            ws.fill_(fill)
            out = torch.empty((B, H, frames, 17, 3), dtype=torch.float32, device="cuda")
            _lib.check(lib.d3dp_denoise(ctx, x2d.data_ptr(), x3d.data_ptr(), t.data_ptr(), out.data_ptr(), B, H, ws.data_ptr(),
                                        n.value, _lib.current_stream()), "d3dp_denoise")
            torch.cuda.synchronize()
            outs.append(out.cpu())
        assert not net.nonfinite_seen()
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])


def test_switch_selects_the_form():
    """The deferred form is the default and D3DP_DEFER_NORM=0 leaves it: only the deferred form has the statistics area --
    [rows of a pass + one tile of slack][2] floats -- in its workspace."""
    frames, cs, B, H = 9, 128, 2, 2
    size = {}
    for on in (True, False):
        with defer_norm(on):
            net = make_model(frames, cs, H, 1).pose_estimator
            n = C.c_size_t()
            _lib.check(_lib.load().d3dp_workspace_bytes(net._context(torch.device("cuda")), B, H, C.byref(n)), "d3dp_workspace_bytes")
            size[on] = n.value
    rows = B * H * frames * 17
    assert size[True] - size[False] == ((rows + 256) * 8 + 255) // 256 * 256


def test_status_flag_stays_clear(case1):
    """d3dp_status after case 1: no non-finite output and no operand outside the split range, in either form."""
    assert case1[True][1] is False and case1[False][1] is False
