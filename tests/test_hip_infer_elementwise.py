"""EXACT inference, element by element, against the oracle's fp64 forward pass (run with ``-m gpu`` on an MI355X).

Every other gate of EXACT mode at denoiser and sampler level is ``mpjpe_mm(...) <= 1e-3``: a mean over all B H F 17 joints, which
one wrong 16-row tile, one (sequence, head) problem of the persistent attention kernel or one lost split-fp16 pass in one tile
class passes.  Here the reference is fp64, there is a per-element figure next to the norm, and the bound comes from the reference
alone: 8 x e32, where e32 is how far the oracle's OWN fp32 forward lies from its fp64 forward in the same case
(oracle/infer_check.py over oracle/grad_check.py; tests/test_infer_elementwise_host.py checks on a CPU that every case below is
well-conditioned and that the comparator rejects a lost lo x hi pass in one row tile which the mm gate accepts).

  (a) SHAPES      the smallest shapes that reach each dispatch path of the inference route;
  (b) ROUTES      the cross-check routes (D3DP_EXACT_IMPL=f32 / bf16x3, D3DP_NO_FOLD=1, D3DP_DEFER_NORM=0, D3DP_LONG_ATTN=rows);
  (c) MAGNITUDES  one weight edit each: the six of test_hip_train_grads and two that reach the range proof with the softmax left
                  as it was (the v rows of one qkv matrix / one fc1 matrix scaled to twice the split-fp16 range);
  (d) SAMPLERS    the public sampler, every step against that step's own e32 (the DDIM pre / post kernels);
  (e) the single ops (d3dp_op_attention impl 2, d3dp_op_linear_x2 with EPI_BIAS / EPI_RESID) under the same comparator, with e32
      from torch's fp32 evaluation of the same op: what locates a failure of (a) - (d).

One model -- one context -- per case; every D3DP_* route switch is cleared unless the case sets it; each case asserts the
implementation it ran on.  The case tables are plain data (no GPU needed to import them): the host test walks them too."""
from functools import lru_cache
from types import SimpleNamespace
from typing import NamedTuple, Tuple

import numpy as np
import pytest
import torch

from d3dp_amd import D3DP, _lib
from d3dp_amd.model import MixSTE2
from d3dp_amd.weights import (H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, flip_2d, make_state_dict, synthetic_inputs_2d,
                              synthetic_noise)
from oracle import infer_check as ic
from test_hip_train_grads import EDITS as TRAIN_EDITS

pytestmark = pytest.mark.gpu
# every environment switch d3dp_create reads for an EXACT context (csrc/ctx_plan.h: CtxEnv)
_SWITCHES = ("D3DP_EXACT_IMPL", "D3DP_LONG_ATTN", "D3DP_NO_FOLD", "D3DP_DEFER_NORM", "D3DP_X2_SKEW", "D3DP_X2_PP", "D3DP_X2_WIDE",
             "D3DP_SEQ_PAD", "D3DP_FOLD_LN")
SD_SEED, X2D_SEED, X3D_SEED = 11, 911, 912
PRE = "pose_estimator."
SPLIT_RANGE = MixSTE2.SPLIT_RANGE
INSTANTIATED, PADDED = (64, 128, 256, 512), (192, 320, 384, 448)
HEADS = 8


class Case(NamedTuple):
    cs: int
    Fr: int
    B: int
    H: int
    dep: int = 2
    edit: str = ""                           # a key of EDITS: one change to the seed state dict
    env: Tuple[Tuple[str, str], ...] = ()    # route switches set for this case (every other one is cleared)
    chunk_seqs: int = 0                      # sequences per pass (0: the library's default)
    joints: int = 17

    @property
    def id(self):
        return (f"cs{self.cs}-F{self.Fr}-B{self.B}-H{self.H}" + (f"-dep{self.dep}" if self.dep != 2 else "")
                + (f"-J{self.joints}" if self.joints != 17 else "") + (f"-chunk{self.chunk_seqs}" if self.chunk_seqs else "")
                + (f"-{self.edit}" if self.edit else "") + "".join(f"-{k[5:]}={v}" for k, v in self.env))


class Sampler(NamedTuple):
    cs: int
    Fr: int
    B: int
    H: int
    K: int
    dep: int = 2

    @property
    def id(self):
        return f"cs{self.cs}-F{self.Fr}-B{self.B}-H{self.H}-K{self.K}"


F16X2 = (("D3DP_EXACT_IMPL", "f16x2"),)
# (a) the smallest shapes that reach each dispatch path; a pass holds B H sequences of F J token rows
SHAPES = [
    Case(512, 9, 1, 2),                  # one pass, 306 rows: one 256-row tile plus a remainder
    Case(512, 9, 2, 3, chunk_seqs=2),    # three passes, two different t across the batch
    Case(512, 27, 2, 2),
    Case(512, 49, 1, 1),                 # keys end inside a tile
    Case(512, 243, 1, 1),
    Case(512, 257, 1, 1),                # chunked keys, last chunk of one key
    Case(512, 300, 1, 1),
    Case(512, 9, 1, 2, dep=8),
    Case(512, 9, 1, 1, joints=33),       # the spatial axis on the whole-sequence kernel
    Case(256, 9, 2, 2), Case(256, 40, 1, 2), Case(256, 243, 1, 1), Case(256, 300, 1, 1),
    Case(128, 9, 2, 2), Case(128, 81, 1, 2), Case(128, 300, 1, 1), Case(128, 9, 1, 2, dep=8),
    Case(64, 27, 1, 2),                  # head dim 8: fp32 attention under split Linears, no deferred norm
    Case(96, 27, 1, 2),                  # the fp32 implementation
    Case(384, 27, 1, 2),                 # the fp32 implementation
    Case(384, 27, 1, 2, env=F16X2),      # head dim 48 padded to 64
    Case(192, 9, 1, 2, env=F16X2),       # head dim 24 padded to 32
]
# (b) the cross-check routes: each a product path somewhere, or the project's own A/B handle
ROUTES = ([Case(cs, 27, 2, 2, env=((k, v),)) for cs in (512, 128)
           for k, v in (("D3DP_EXACT_IMPL", "f32"), ("D3DP_EXACT_IMPL", "bf16x3"), ("D3DP_NO_FOLD", "1"), ("D3DP_DEFER_NORM", "0"))]
          + [Case(256, 40, 1, 2, env=(("D3DP_LONG_ATTN", "rows"),)), Case(512, 300, 1, 1, env=(("D3DP_LONG_ATTN", "rows"),))])


def _ln_bound(sd, blk, norm, cs):
    """|LN(x)_k| <= sqrt(C - 1) |gamma_k| + |beta_k| (fp64): what the range proof takes for the operand of qkv / fc1."""
    return (cs - 1) ** 0.5 * sd[PRE + blk + norm + ".weight"].double().abs() + sd[PRE + blk + norm + ".bias"].double().abs()


def _v_rows_to_2x_range(sd, cs):
    """The v rows of TTE block 0's qkv matrix times the factor that puts the bound the weights prove for q / k / v at twice what the
    scale 2^4 holds (the factor of test_out_of_range_qkv_lowers_the_scale_and_stays_on_f16x2, over the rows scaled): s_kv must
    drop, and the softmax -- q and k -- stays as it was, so the reference stays well-conditioned."""
    key = PRE + "TTEblocks.0.attn.qkv.weight"
    ln = _ln_bound(sd, "TTEblocks.0.", "norm1", cs)
    w = sd[key].clone()
    factor = 2.0 * SPLIT_RANGE / (w[2 * cs:].double().abs() @ ln).max().item()
    w[2 * cs:] *= factor
    sd[key] = w


def _fc1_to_2x_range(sd, cs):
    """TTE block 0's fc1 matrix times the factor that does the same for the bound of the MLP hidden operand: s_h must drop."""
    key = PRE + "TTEblocks.0.mlp.fc1.weight"
    ln = _ln_bound(sd, "TTEblocks.0.", "norm2", cs)
    sd[key] = sd[key] * (2.0 * SPLIT_RANGE / (sd[key].double().abs() @ ln).max().item())


RANGE_EDITS = {"tte0-v-rows-to-2x-range": _v_rows_to_2x_range, "tte0-fc1-to-2x-range": _fc1_to_2x_range}
EDITS = {**TRAIN_EDITS, **RANGE_EDITS}
# (c) one edit of the seed state dict each
MAGNITUDES = ([Case(cs, 27, 1, 2, edit=e) for cs in (512, 128) for e in EDITS]
              + [Case(256, 27, 1, 2, edit=e) for e in RANGE_EDITS] + [Case(384, 27, 1, 2, edit=e, env=F16X2) for e in RANGE_EDITS])
# (d) the public sampler: (cs, F, B, H, K)
SAMPLERS = [Sampler(512, 27, 1, 2, 3), Sampler(128, 9, 2, 2, 10), Sampler(512, 9, 2, 2, 5), Sampler(256, 40, 1, 2, 2),
            Sampler(512, 243, 1, 1, 2)]
ALL_CASES = list(dict.fromkeys(SHAPES + ROUTES + MAGNITUDES))


def state_dict_of(case):
    if case.joints != 17:
        assert not case.edit
        return make_state_dict(SD_SEED, case.cs, case.dep, case.Fr, prefix="", joints=case.joints)
    sd = make_state_dict(SD_SEED, case.cs, case.dep, case.Fr)
    if case.edit:
        EDITS[case.edit](sd, case.cs)
    return sd


def problem(case):
    """(state dict, x2d, x3d, t) of one denoiser case, all on the CPU."""
    sd = state_dict_of(case)
    B, H, Fr, J = case.B, case.H, case.Fr, case.joints
    if J == 17:
        x2d = torch.from_numpy(synthetic_inputs_2d(X2D_SEED, B, Fr))
    else:
        x2d = torch.rand(B, Fr, J, 2, generator=torch.Generator().manual_seed(X2D_SEED)) * 2 - 1
    x3d = torch.from_numpy(synthetic_noise(X3D_SEED, (B, H, Fr, J, 3)))
    return sd, x2d, x3d, torch.tensor([30, 700][:B], dtype=torch.long)


def sampler_problem(case):
    """(state dict, x2d (numpy), the K recorded noise draws) of one sampler case."""
    sd = make_state_dict(SD_SEED, case.cs, case.dep, case.Fr)
    x2d = synthetic_inputs_2d(X2D_SEED, case.B, case.Fr)
    return sd, x2d, [torch.from_numpy(synthetic_noise(X3D_SEED + k, (case.B, case.H, case.Fr, 17, 3))) for k in range(case.K)]


@lru_cache(maxsize=None)
def reference(case):
    """The oracle's fp64 and fp32 run of one case and the e32 they define: computed once, shared, never written to."""
    if isinstance(case, Sampler):
        sd, x2d, noises = sampler_problem(case)
        return ic.sample_pair(sd, x2d, noises, case.H, case.K, case.dep)
    sd, x2d, x3d, t = problem(case)
    return ic.denoise_pair(sd, x2d, x3d, t, case.dep)


def expected_implementation(case, sd):
    """What exact_scales()[2] must say (MixSTE2.exact_scales, include/d3dp_hip.h): the switch if it names a cross-check
    implementation; the fp32 implementation at a width outside the instantiated set unless D3DP_EXACT_IMPL=f16x2 opted a padded-head
    width in; otherwise split-fp16 -- unless a LayerNorm's own output bound leaves the split-fp16 range, where the context falls
    back by itself (split-bf16; a padded-head context: fp32)."""
    want = dict(case.env).get("D3DP_EXACT_IMPL", "")
    if want in ("f32", "bf16x3"):
        return want
    padded = want == "f16x2" and case.cs in PADDED
    if case.cs not in INSTANTIATED and not padded:
        return "f32"
    pre = PRE if case.joints == 17 else ""
    for k, v in sd.items():
        if k.startswith(pre) and (k.endswith("norm1.weight") or k.endswith("norm2.weight")) and "blocks." in k:
            bound = (case.cs - 1) ** 0.5 * v.double().abs() + sd[k[:-len("weight")] + "bias"].double().abs()
            if bound.max().item() >= SPLIT_RANGE:
                return "f32" if padded else "bf16x3"
    return "f16x2"


def clear_switches(monkeypatch, env=()):
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)


def denoiser_of(case, sd):
    """(the environment switches are read when the context is created, at the first call: one model per case)"""
    if case.joints != 17:
        m = MixSTE2(num_frame=case.Fr, num_joints=case.joints, embed_dim_ratio=case.cs, depth=case.dep, is_train=False,
                    numerics="exact", drop_path_rate=0.0, chunk_seqs=case.chunk_seqs)
        m.load_state_dict(sd, strict=True)
        return m.cuda().eval()
    args = SimpleNamespace(number_of_frames=case.Fr, test_time_augmentation=True, timestep=1000, scale=1.0, cs=case.cs, dep=case.dep,
                           chunk_seqs=case.chunk_seqs)
    m = D3DP(args, H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, is_train=False, num_proposals=case.H, sampling_timesteps=1, numerics="exact")
    m.load_state_dict(sd, strict=False)
    return m.cuda().eval().pose_estimator


def run_and_check(monkeypatch, case):
    """One pose_estimator(x2d, x3d, t) call of `case` on the GPU: the implementation it ran on, every output element finite and the
    whole (B, H, F, J, 3) output within 8 x e32 of the fp64 oracle in both figures.  -> the denoiser (for further assertions)."""
    clear_switches(monkeypatch, case.env)
    sd, x2d, x3d, t = problem(case)
    ref = reference(case)
    assert ic.admissible(ref.e32), (case.id, ref.e32)
    net = denoiser_of(case, sd)
    out = net(x2d.cuda(), x3d.cuda(), t.cuda())
    torch.cuda.synchronize()
    assert out.shape == ref.out64.shape and out.dtype == torch.float32
    impl = net.exact_scales()[2]
    assert impl == expected_implementation(case, sd), (case.id, impl)
    line, bad, _ = ic.check(f"EXACT inference vs fp64, {case.id} [{impl}]", out.cpu(), ref.out64, ref.e32, case.chunk_seqs)
    print(line)
    assert not bad, "\n".join([f"{case.id}: outside {ic.FACTOR:g} x e32 = ({ic.FACTOR * ref.e32[0]:.2e}, "
                               f"{ic.FACTOR * ref.e32[1]:.2e})"] + bad)
    return net


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: c.id)
def test_denoiser_elementwise_over_the_dispatch_shapes(monkeypatch, case):
    net = run_and_check(monkeypatch, case)
    assert not net.nonfinite_seen()


@pytest.mark.parametrize("case", ROUTES, ids=lambda c: c.id)
def test_denoiser_elementwise_on_the_cross_check_routes(monkeypatch, case):
    net = run_and_check(monkeypatch, case)
    assert not net.nonfinite_seen()


@pytest.mark.parametrize("case", MAGNITUDES, ids=lambda c: c.id)
def test_denoiser_elementwise_when_one_operand_leaves_its_usual_magnitude(monkeypatch, case):
    """The two range edits also say what the range proof did: the bound is beyond what 2^4 holds, the context stays on split-fp16
    and lowers the scale concerned of TTE block 0 (index dep + 0 of exact_scales) -- now held to the fp32-class bound."""
    net = run_and_check(monkeypatch, case)
    if case.edit in RANGE_EDITS:
        kv, hd, impl = net.exact_scales()
        bound, i = net.exact_range_bound(), case.dep + 0
        print(f"{case.id}: proven bound {bound:.4g} (2^4 holds {SPLIT_RANGE}), TTE block 0: s_kv {kv[i]:g}, s_h {hd[i]:g}")
        assert bound >= SPLIT_RANGE and impl == "f16x2"
        lowered = kv if case.edit == "tte0-v-rows-to-2x-range" else hd
        assert lowered[i] < 16.0 and lowered[i] * bound < 65504.0
    assert not net.nonfinite_seen()


@pytest.mark.parametrize("case", SAMPLERS, ids=lambda c: c.id)
def test_sampler_elementwise_every_step(monkeypatch, case):
    """The public m(x2d, None, input_2d_flip=..., noise=noises): out[:, k] of every step k within 8 x that step's e32 of the fp64
    sampler -- the flip permutation, the fp64 predict_noise_from_start and the clamp of the DDIM pre / post kernels included."""
    clear_switches(monkeypatch)
    sd, x2d, noises = sampler_problem(case)
    ref = reference(case)
    args = SimpleNamespace(number_of_frames=case.Fr, test_time_augmentation=True, timestep=1000, scale=1.0, cs=case.cs, dep=case.dep)
    m = D3DP(args, H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, is_train=False, num_proposals=case.H, sampling_timesteps=case.K,
             numerics="exact")
    m.load_state_dict(sd, strict=False)
    m = m.cuda().eval()
    out = m(torch.from_numpy(x2d).cuda(), None, input_2d_flip=torch.from_numpy(flip_2d(x2d)).cuda(), noise=noises)
    torch.cuda.synchronize()
    assert out.shape == ref.out64.shape and m.pose_estimator.exact_scales()[2] == "f16x2"
    out, bad = out.cpu(), []
    for k in range(case.K):
        assert ic.admissible(ref.e32[k]), (case.id, k, ref.e32[k])
        line, b, _ = ic.check(f"EXACT sampler vs fp64, {case.id} step {k}", out[:, k], ref.out64[:, k], ref.e32[k])
        print(line)
        bad += b
    assert not bad, "\n".join([f"{case.id}: outside {ic.FACTOR:g} x the step's e32"] + bad)
    assert not m.pose_estimator.nonfinite_seen()


# ------------------------------------------------------------------------------------------------ (e) the single ops
@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def check_op(tag, got, ref64, ref32):
    e32 = ic.e32_of(ref32, ref64)
    assert ic.admissible(e32), (tag, e32)
    line, bad, _ = ic.check(tag, got, ref64, e32)
    print(line)
    assert not bad, "\n".join([f"{tag}: outside {ic.FACTOR:g} x e32 = ({ic.FACTOR * e32[0]:.2e}, {ic.FACTOR * e32[1]:.2e})"] + bad)


def attention_reference(qkv, n_bh, F, J, C, axis, dtype):
    """softmax(q k^T hd^-0.5) v on the (n_bh, F, J, 3 C) row layout in `dtype` (axis 0: sequences over joints, 1: over frames)."""
    hd = C // HEADS
    x = qkv.to(dtype).reshape(n_bh, F, J, 3, HEADS, hd)
    perm = (0, 1, 3, 2, 4) if axis == 0 else (0, 2, 3, 1, 4)
    q, k, v = (x[:, :, :, i].permute(*perm) for i in range(3))
    a = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5, dim=-1) @ v
    a = a.permute(0, 1, 3, 2, 4) if axis == 0 else a.permute(0, 3, 1, 2, 4)
    return a.reshape(n_bh * F * J, C).double()


ATTN_SHAPES = [(1, F, 3) for F in (9, 49, 243, 257, 351)] + [(0, 9, 17)]       # (axis, F, J)


@pytest.mark.parametrize("axis,F,J", ATTN_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("C", [512, 256, 128])
def test_attention_op_elementwise(lib, C, axis, F, J):
    """d3dp_op_attention impl 2 (the split-fp16 kernels: spatial, whole-sequence, chunked keys) on fp32 rows."""
    n_bh = 2
    qkv = torch.randn(n_bh * F * J, 3 * C, generator=torch.Generator().manual_seed(F * 7 + C + J))
    qkv[:, :C] *= 2.0        # sharpen the softmax a little
    qd = qkv.cuda().contiguous()
    out = torch.full((n_bh * F * J, C), float("nan"), device="cuda")
    _lib.check(lib.d3dp_op_attention(0, 2, axis, qd.data_ptr(), out.data_ptr(), n_bh, F, J, C, HEADS, _lib.current_stream()))
    torch.cuda.synchronize()
    check_op(f"attention impl 2 C={C} axis={axis} F={F} J={J}", out.cpu(), attention_reference(qkv, n_bh, F, J, C, axis, torch.float64),
             attention_reference(qkv, n_bh, F, J, C, axis, torch.float32))


@pytest.mark.parametrize("N,K", [(1536, 512), (512, 1024), (384, 128)])
@pytest.mark.parametrize("M", [129, 306, 4131])
def test_linear_x2_op_elementwise(lib, M, N, K):
    """d3dp_op_linear_x2 with EPI_BIAS and EPI_RESID, the operands split as test_linear_split_f16_is_fp32_class splits them
    (activations at 2^4, weights at the power of two that puts max |w| in [2^13, 2^14))."""
    g = torch.Generator().manual_seed(M * 3 + N + K)
    A = torch.randn(M, K, generator=g) * 2
    W = torch.randn(N, K, generator=g) / K ** 0.5
    bias = torch.randn(N, generator=g)
    x = torch.randn(M, N, generator=g)
    Ad, Wd, bd = A.cuda(), W.cuda(), bias.cuda()
    A2 = torch.empty(2, M, K, dtype=torch.float16, device="cuda")
    W2 = torch.empty(2, N, K, dtype=torch.float16, device="cuda")
    st = _lib.current_stream()
    _lib.check(lib.d3dp_op_split2(Ad.data_ptr(), A2.data_ptr(), M * K, 16.0, st))
    w_scale = 2.0 ** (13 - int(np.floor(np.log2(W.abs().max().item()))))
    _lib.check(lib.d3dp_op_split2(Wd.data_ptr(), W2.data_ptr(), N * K, w_scale, st))
    lin64, lin32 = A.double() @ W.double().t() + bias.double(), A @ W.t() + bias
    out = torch.full((M, N), float("nan"), device="cuda")
    _lib.check(lib.d3dp_op_linear_x2(_lib.EPI_BIAS, A2.data_ptr(), W2.data_ptr(), bd.data_ptr(), w_scale, out.data_ptr(), M, N, K, st))
    acc = x.clone().cuda()
    _lib.check(lib.d3dp_op_linear_x2(_lib.EPI_RESID, A2.data_ptr(), W2.data_ptr(), bd.data_ptr(), w_scale, acc.data_ptr(), M, N, K, st))
    torch.cuda.synchronize()
    check_op(f"linear_x2 EPI_BIAS M={M} N={N} K={K}", out.cpu(), lin64, lin32.double())
    check_op(f"linear_x2 EPI_RESID M={M} N={N} K={K}", acc.cpu(), x.double() + lin64, (x + lin32).double())
