"""Host side of the bit-for-bit glue checks (oracle/glue_check.py; the GPU side is tests/test_hip_glue.py).

Three things are pinned here, on the CPU: the step-wise reference IS the whole-sampler oracle (so a kernel equal to
the steps is equal to the reference's sampler), the JPMA reference IS what fixture g5 verifies, and the reference's
behaviour on the edge inputs the GPU tests plant (NaN, inf, ties, 0/0, the clamp bound) is recorded as observed, so
that what those tests expect of the kernels is torch's behaviour and not an assumption about it."""
import os

import numpy as np
import pytest
import torch

from d3dp_amd import jpma
from d3dp_amd.weights import H36M_JOINTS_LEFT as KL, H36M_JOINTS_RIGHT as KR, flip_2d, synthetic_inputs_2d, synthetic_noise
from oracle import d3dp_oracle as orc
from oracle import glue_check as gc

NAN, INF = float("nan"), float("inf")


# ---- the step-wise sampler reference is the oracle's sampler ------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 3.0])
@pytest.mark.parametrize("eta", [1.0, 0.0])
@pytest.mark.parametrize("K", [1, 3, 10])
def test_stepwise_reference_composes_to_the_oracle_sampler(monkeypatch, K, eta, scale):
    B, H, Fr = 2, 3, 27
    monkeypatch.setattr(orc, "mixste_forward", lambda p, x2d, x3, t, depth: gc.stub_denoiser(x2d, x3, t))
    x2d = synthetic_inputs_2d(11, B, Fr)
    x2, x2f = torch.from_numpy(x2d), torch.from_numpy(flip_2d(x2d))
    noises = [torch.from_numpy(synthetic_noise(40 + k, (B, H, Fr, 17, 3))) * scale for k in range(K)]
    sched = orc.cosine_schedule(1000)
    want = orc.ddim_sample_flip({}, sched, x2, x2f, H, K, 2, KL, KR, noises, scale=scale, eta=eta)
    got = gc.ddim_loop_ref(gc.stub_denoiser, sched, x2, x2f, K, KL, KR, noises, scale=scale, eta=eta)
    assert want.shape == (B, K, H, Fr, 17, 3)
    assert gc.bits_equal(got, want), gc.bit_mismatches(got, want)
    sat = (want.abs() == torch.tensor(1.1 * scale).float()).float().mean().item()
    assert 0.02 < sat < 0.9, sat                    # the stub drives part of x_start into the clamp, and not all of it


def test_stub_table_is_asymmetric_and_reaches_the_clamp():
    t = gc.STUB_TAB
    assert t.shape == (17, 3) and t.max().item() == np.float32(1.4) and t.min().item() == np.float32(-1.4)
    swapped = t.clone()
    swapped[KL + KR] = t[KR + KL]
    assert not torch.equal(swapped, t)


# ---- JPMA: the reference is what fixture g5 verifies --------------------------------------------------------------------
def _g5(golden_dir):
    g = np.load(os.path.join(golden_dir, "g5_caller.npz"))
    Fr = int(g["frames"])
    x2, x3 = jpma.eval_data_prepare(Fr, torch.from_numpy(g["seq2d"])[None], torch.from_numpy(g["seq3d"])[None])
    traj = x3[:, :, :1].clone()
    x3[:, :, 0] = 0
    return g, torch.from_numpy(g["pred"]), traj, torch.from_numpy(g["cam"]), x2, x3


def test_jpma_ref_reproduces_fixture_g5(golden_dir):
    g, pred, traj, cam, x2, x3 = _g5(golden_dir)
    agg, sel, es, em, jb, mean64 = gc.jpma_ref(pred, traj, cam, x2, x3, 0, False)
    pz = pred.clone()
    pz[:, :, :, :, 0] = 0
    assert torch.equal(agg, jpma.jpma_aggregate(pz, torch.from_numpy(g["reproj"]), x2))
    K = pred.shape[1]
    assert torch.allclose(es.permute(1, 0, 2, 3).reshape(K, -1).mean(-1), torch.from_numpy(g["e_jagg"]), atol=1e-6, rtol=1e-5)
    assert torch.allclose(em.permute(1, 0, 2, 3).reshape(K, -1).mean(-1), torch.from_numpy(g["e_jbest"]), atol=1e-6, rtol=1e-5)
    assert sel.dtype == torch.int32 and sel.shape == agg.shape[:-1] and jb.shape == agg.shape
    assert torch.allclose(mean64, pz.double().mean(2)) and mean64.dtype == torch.float64


def _edge_case():
    """A small problem with every edge of the GPU tests planted at a known (frame 0, joint) position."""
    torch.manual_seed(3)
    B, K, H, Fr, J = 1, 1, 4, 2, 17
    pred = torch.randn(B, K, H, Fr, J, 3) * 0.3
    traj = torch.randn(B, Fr, 1, 3) * 0.1 + torch.tensor([0.0, 0.0, 4.0])
    cam = torch.tensor([2.29, 2.287, 0.0254, 0.0289, -0.2070, 0.2477, -0.0030, -0.0009, -0.0014])
    gt2 = torch.rand(B, Fr, J, 2) * 2 - 1
    gt3 = torch.randn(B, Fr, J, 3) * 0.3
    pred[0, 0, 2, 0, 1, 1] = NAN                      # joint 1: NaN in one coordinate of hypothesis 2
    pred[0, 0, :, 0, 2, 0] = NAN                      # joint 2: NaN in every hypothesis
    pred[0, 0, 1, 0, 3, 2] = NAN                      # joint 3: NaN in hypotheses 1 and 3 -> the first one
    pred[0, 0, 3, 0, 3, 2] = NAN
    gt2[0, 0, 4, 0] = INF                             # joint 4: every 2D error +inf
    gt2[0, 0, 5, 1] = NAN                             # joint 5: every 2D error NaN
    gt3[0, 0, 6, 2] = NAN                             # joint 6: every 3D error NaN
    pred[0, 0, 1:, 0, 7] = pred[0, 0, 0, 0, 7]        # joint 7: all hypotheses equal
    pred[0, 0, 3, 0, 8] = pred[0, 0, 1, 0, 8]         # joint 8: hypotheses 1 and 3 equal
    return pred, traj, cam, gt2, gt3


def test_reference_semantics_on_edge_inputs_are_as_recorded():
    """torch.min: a NaN wins, the first NaN wins, an all-+inf row gives index 0, ties go to the lowest index;
    torch.clamp keeps NaN; 0/0 at a zeroed root under a zero trajectory is NaN."""
    v, i = torch.tensor([3.0, NAN, 1.0, NAN]).min(dim=0)
    assert torch.isnan(v) and int(i) == 1
    v, i = torch.tensor([INF, INF, INF]).min(dim=0)
    assert v.item() == INF and int(i) == 0
    v, i = torch.tensor([2.0, 1.0, 1.0]).min(dim=0)
    assert int(i) == 1
    c = torch.clamp(torch.tensor([NAN, -INF, INF, -0.0]), min=-1, max=1)
    assert torch.isnan(c[0]) and c[1:3].tolist() == [-1.0, 1.0] and gc.bits_equal(c[3:], torch.tensor([-0.0]))
    assert torch.isnan(torch.clamp(torch.tensor([NAN], dtype=torch.float64), min=-1.1, max=1.1)).all()

    pred, traj, cam, gt2, gt3 = _edge_case()
    for linear in (False, True):
        agg, sel, es, em, jb, _ = gc.jpma_ref(pred, traj, cam, gt2, gt3, 0, linear)
        p = pred.clone()
        p[:, :, :, :, 0] = 0
        s = sel[0, 0, 0]
        assert int(s[1]) == 2 and gc.bits_equal(agg[0, 0, 0, 1], p[0, 0, 2, 0, 1])         # the NaN hypothesis is SELECTED
        assert int(s[2]) == 0 and gc.bits_equal(agg[0, 0, 0, 2], p[0, 0, 0, 0, 2])         # all NaN: hypothesis 0's pose
        assert torch.isnan(es[0, 0, 0, 2]) and torch.isnan(em[0, 0, 0, 2])
        assert int(s[3]) == 1                                                              # the first NaN
        assert int(s[4]) == 0 and gc.bits_equal(agg[0, 0, 0, 4], p[0, 0, 0, 0, 4])         # all +inf: index 0, its pose
        assert int(s[5]) == 0 and gc.bits_equal(agg[0, 0, 0, 5], p[0, 0, 0, 0, 5])
        assert torch.isnan(em[0, 0, 0, 6]) and gc.bits_equal(jb[0, 0, 0, 6], p[0, 0, 0, 0, 6])
        assert int(s[7]) == 0
        assert int(s[8]) != 3
    z = torch.zeros(1, 1, 2, 1, 17, 3)
    absol = z + torch.zeros(1, 1, 1, 3)[:, None, None]
    assert torch.isnan(jpma.project_to_2d(absol, cam)[..., 0, :]).all()
    assert torch.isnan(gc.project_linear(absol, cam)[..., 0, :]).all()
    agg, sel, *_ = gc.jpma_ref(torch.randn(1, 1, 2, 1, 17, 3), torch.zeros(1, 1, 1, 3), cam, torch.zeros(1, 1, 17, 2),
                               torch.zeros(1, 1, 17, 3), 0, False)
    assert int(sel[0, 0, 0, 0]) == 0 and not agg[0, 0, 0, 0].any()


def test_host_branches_of_jpma_agree_with_the_reference_on_edge_inputs():
    """jpma_winners / jpma_combine on host tensors (the gloo path) state the selection with torch.min: they must pick
    what jpma_ref picks -- and what the kernels pick (tests/test_hip_glue.py) -- NaN, inf and ties included."""
    pred, traj, cam, gt2, gt3 = _edge_case()
    agg, sel, *_ = gc.jpma_ref(pred, traj, cam, gt2, gt3, 0, False)
    wins = torch.stack([jpma.jpma_winners(pred[:, :, r * 2:r * 2 + 2].contiguous(), traj, cam, gt2, h_offset=r * 2)
                        for r in range(2)])
    for r in range(2):
        want = gc.jpma_winners_ref(pred[:, :, r * 2:r * 2 + 2], traj, cam, gt2, 0, False, h_offset=r * 2)
        assert gc.bits_equal(wins[r], want)
    a2, s2 = jpma.jpma_combine(wins)
    assert gc.bits_equal(a2, agg) and torch.equal(s2, sel)


# ---- the clamp bound ----------------------------------------------------------------------------------------------------
def test_clamp_bound_table():
    """The reference clamps an fp32 tensor with the Python double 1.1 * scale: its bound is that double rounded once.
    Forming the bound as an fp32 product is one ulp off at some scales, which moves every saturated element."""
    scales = [0.5, 0.75, 1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 5.0, 6.0, 7.0, 10.0]
    off = gc.clamp_bound_table(scales)
    assert 3.0 in off and 0.75 in off and 1.0 not in off and 0.5 not in off
    assert off == [0.75, 1.5, 3.0, 6.0, 7.0], off
    big = torch.full((4,), 100.0)
    for s in scales:
        lim = torch.clamp(big, min=-1.1 * s, max=1.1 * s)[0]
        assert lim.item() == torch.tensor(1.1 * s, dtype=torch.float64).float().item()
    assert torch.clamp(big, max=1.1 * 3.0)[0].item() == np.float32(3.3)
    assert (torch.tensor(1.1) * torch.tensor(3.0)).item() == np.nextafter(np.float32(3.3), np.float32(4))
