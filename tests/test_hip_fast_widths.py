"""GPU tests of D3DP_FAST_IMPL=mfma at channels 192 / 320 / 384 / 448 (head dims 24, 40, 48, 56 with the model's 8 heads): FAST and
FAST16 contexts at widths outside the instantiated set, opt-in.  The head dim is padded to 32 / 64 inside the packed 2-byte weights
(zero rows of the qkv matrix and bias, zero columns of proj), the streaming Linear runs at K / 64 in {3, 5, 6, 7, 10, 12, 14}
(gemm_stream_widths.hip), the attention kernels run their head dim 32 / 64 forms with the true head dim in the softmax exponent
(attention_fast_pad.hip) and the LayerNorms run run-time-width row kernels with 2-byte rows (pointwise_rows2.hip).  Without the
switch such a context is refused as before.

   1. the Linear alone at the (N, K) pairs of the four widths;
   2. the row kernels alone against an fp64 LayerNorm;
   3. the attention kernels alone through d3dp_op_attention's impl = 1 | (true head dim << 8);
   4. sampler parity in both modes against the fp32 oracle and its 2-byte emulation;
   5. without the switch: the refusal; with it at cs = 512: no bit moves;
   6. pad columns never leak;
   7. any pass split gives the same bits;
   8. the FAST16 fallback is a FAST context bit for bit;
   9. the call runs in exactly d3dp_workspace_bytes;
  10. the stream contract: side stream, capture and replay.
"""
import importlib.util
import os
import warnings

import pytest
import torch

from d3dp_amd import _lib
from d3dp_amd.model import MixSTE2
from d3dp_amd.weights import make_state_dict, synthetic_inputs_2d, synthetic_noise
from oracle import d3dp_oracle as orc
from test_hip_fast16 import FP16_MAX, f16_round, oracle_sample, proven_bound_fp64, sample, sampler_model
from test_hip_fast_heads import random_qkv
from test_hip_fast_long import TYPES
from test_hip_parity import FAST_TOL_MM, ref_attention

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("lib_ab_hash", os.path.join(REPO, "tools", "lib_ab_hash.py"))
ab = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ab)

pytestmark = pytest.mark.gpu
HEADS = 8
WIDTHS = [192, 320, 384, 448]
ACTS = [1, 4]                                      # the 2-byte types of the row launchers and d3dp_op_attention: bf16, fp16
OP_MODE = {1: _lib.MODE_FAST, 4: _lib.OP_FP16}     # ... and d3dp_op_linear's mode for them
NUMERICS = {"fast": "bf16", "fast16": "fp16"}


def padded(cs):
    """channels -> (head dim, padded head dim, heads x padded head dim)"""
    hd = cs // HEADS
    hdp = 32 if hd <= 32 else 64
    return hd, hdp, HEADS * hdp


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def switch(monkeypatch, on=True):
    """Read by d3dp_create, i.e. at the first call of a model made after this."""
    if on:
        monkeypatch.setenv("D3DP_FAST_IMPL", "mfma")
    else:
        monkeypatch.delenv("D3DP_FAST_IMPL", raising=False)


def denoiser(sd, frames, joints, cs, dep, numerics, chunk_seqs=0, heads=HEADS):
    m = MixSTE2(num_frame=frames, num_joints=joints, embed_dim_ratio=cs, depth=dep, num_heads=heads, is_train=False, numerics=numerics,
                drop_path_rate=0.0, chunk_seqs=chunk_seqs)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


def denoiser_case(seed, frames, joints, cs, dep, B, H):
    sd = make_state_dict(seed, cs, dep, frames, prefix="", joints=joints)
    g = torch.Generator().manual_seed(seed * 1000 + cs + frames)
    x2d = torch.rand(B, frames, joints, 2, generator=g) * 2 - 1
    x3d = torch.randn(B, H, frames, joints, 3, generator=g)
    t = torch.tensor([(999 - 379 * b) % 1000 for b in range(B)])
    return sd, x2d, x3d, t


# ------------------------------------------------------------------------------------------------ 1: the Linear alone
def linear_pairs(cs):
    """(name, epilogues, N, K) of the four Linears of a block: qkv and fc1 contract over C (K / 64 = 3, 5, 6, 7: both epilogues are
    instantiated there), fc2 over 2 C (6, 10, 12, 14), proj over Cp (4, 8)."""
    _, _, cp = padded(cs)
    return [("qkv", (_lib.EPI_BIAS, _lib.EPI_GELU), 3 * cp, cs), ("fc1", (_lib.EPI_GELU, _lib.EPI_BIAS), 2 * cs, cs),
            ("fc2", (_lib.EPI_BIAS,), cs, 2 * cs), ("proj", (_lib.EPI_BIAS,), cs, cp)]


def run_linear(lib, act, epi, A, W, bias, rows=None):
    """d3dp_op_linear on operands rounded to the type, into a NaN-filled output; against the fp64 product of the rounded operands on
    `rows` (all rows if None) at test_linear_all_epilogues' bf16 tolerances, an eighth of them for fp16."""
    dt, atol, rtol = TYPES[act][:3]
    M, K = A.shape
    N = W.shape[0]
    Ad, Wd, bd = A.to(dt).cuda().contiguous(), W.to(dt).cuda().contiguous(), bias.cuda()
    out = torch.full((M, N), float("nan"), dtype=dt, device="cuda")
    _lib.check(lib.d3dp_op_linear(OP_MODE[act], epi, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), out.data_ptr(), M, N, K,
                                  _lib.current_stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    sel = torch.arange(M) if rows is None else rows
    want = A[sel].to(dt).double() @ W.to(dt).double().t() + bias.double()
    if epi == _lib.EPI_GELU:
        want = torch.nn.functional.gelu(want)
    got = out.float().cpu().double()[sel]
    err = (got - want).abs().max().item()
    assert torch.allclose(got, want, atol=atol, rtol=rtol), (act, epi, M, N, K, err)
    return err


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("cs", WIDTHS)
def test_linear_alone(lib, cs, act):
    """M = 300: one full 256-row tile plus 44 rows; N = 192 / 320 / 448 end in half an N tile."""
    M = 300
    for name, epis, N, K in linear_pairs(cs):
        g = torch.Generator().manual_seed(M + N + K)
        A, W, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
        for epi in epis:
            err = run_linear(lib, act, epi, A, W, bias)
            print(f"linear cs={cs} act={act} {name} {M}x{N}x{K} epi {epi}: max |err| {err:.2e}")


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("cs", WIDTHS)
def test_linear_more_tiles_than_cus(lib, cs, act):
    """fc1 (EPI_GELU, N = 2 C, K = C) at M = 40000: 157 row tiles x 3 .. 7 column tiles on a persistent grid of one workgroup per CU,
    so every workgroup crosses tile boundaries with its ring running at a k-depth that is no multiple of the ring's 3 stages (or is:
    K / 64 = 3, 6).  Every output finite; every 13th row (13 and 256 are coprime: about 20 rows of every tile, at every position
    within a tile over the tiles) and the last 300 rows against the reference."""
    M, N, K = 40000, 2 * cs, cs
    g = torch.Generator().manual_seed(M + N + K)
    A, W, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    rows = torch.cat([torch.arange(0, M - 300, 13), torch.arange(M - 300, M)])
    err = run_linear(lib, act, _lib.EPI_GELU, A, W, bias, rows)
    print(f"linear cs={cs} act={act} fc1 {M}x{N}x{K}: max |err| {err:.2e} over {len(rows)} rows")


# ------------------------------------------------------------------------------------------------ 2: the row kernels alone
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("T", [5, 67])
@pytest.mark.parametrize("C_", WIDTHS)
def test_layernorm_with_two_byte_rows_out(lib, C_, T, act):
    """d3dp_op_layernorm codes 1 / 4 at a run-time width against an fp64 LayerNorm.  The kernel rounds an fp32 LayerNorm once to
    the type: with e0 the error of the library's fp32-output form (code 0) on the same inputs, every element lies within
    e0 + 2^-8 |want| (bf16: half an ulp of 8 significand bits) or e0 + 2^-11 |want| + 2^-24 (fp16: 11 bits, and its subnormal
    spacing).  T = 5: a partly filled workgroup of 4 rows.  A row of slack behind the output stays NaN."""
    dt = TYPES[act][0]
    g = torch.Generator().manual_seed(C_ + T)
    x = torch.randn(T, C_, generator=g) * 3 + 0.5
    w, b = torch.randn(C_, generator=g), torch.randn(C_, generator=g)
    want = torch.nn.functional.layer_norm(x.double(), (C_,), w.double(), b.double(), 1e-6)
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    out32 = torch.full((T, C_), float("nan"), device="cuda")
    _lib.check(lib.d3dp_op_layernorm(0, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), 1e-6, out32.data_ptr(), T, C_, _lib.current_stream()))
    out = torch.full((T + 1, C_), float("nan"), dtype=dt, device="cuda")
    _lib.check(lib.d3dp_op_layernorm(act, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), 1e-6, out.data_ptr(), T, C_, _lib.current_stream()))
    torch.cuda.synchronize()
    assert torch.isnan(out[T].float()).all()
    got = out[:T].float().cpu().double()
    assert torch.isfinite(got).all()
    e0 = (out32.cpu().double() - want).abs().max().item()
    bound = e0 + (2.0 ** -8 * want.abs() if act == 1 else 2.0 ** -11 * want.abs() + 2.0 ** -24)
    err = (got - want).abs()
    print(f"layernorm C={C_} T={T} act={act}: max |err| vs fp64 {err.max().item():.3e}, fp32 rows {e0:.3e}, "
          f"largest err / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------ 3: the attention kernels alone
def pad_heads(qkv, cs):
    """rows of 3 C columns -> rows of 3 Cp: zero columns behind every head's hd."""
    hd, hdp, cp = padded(cs)
    out = torch.zeros(qkv.shape[0], 3, HEADS, hdp, dtype=qkv.dtype)
    out[..., :hd] = qkv.reshape(qkv.shape[0], 3, HEADS, hd)
    return out.reshape(qkv.shape[0], 3 * cp)


def unpad_out(out, cs):
    """[rows, Cp] -> (the true columns [rows, C], the pad columns [rows, heads, hdp - hd])"""
    hd, hdp, _ = padded(cs)
    v = out.reshape(out.shape[0], HEADS, hdp)
    return v[..., :hd].reshape(out.shape[0], cs), v[..., hd:]


def padded_attention(lib, act, axis, qkv, n_bh, F, J, cs):
    """The hook on `qkv` (fp32, CPU, true width) rounded to the type and padded, into a NaN-filled output, twice: bit-equal run to
    run.  -> the 2-byte device result [rows, Cp] on the CPU."""
    hd, _, cp = padded(cs)
    qd = pad_heads(qkv.to(TYPES[act][0]), cs).cuda().contiguous()
    outs = []
    for _ in range(2):
        out = torch.full((n_bh * F * J, cp), float("nan"), dtype=qd.dtype, device="cuda")
        _lib.check(lib.d3dp_op_attention(act, 1 | (hd << 8), axis, qd.data_ptr(), out.data_ptr(), n_bh, F, J, cp, HEADS,
                                         _lib.current_stream()))
        torch.cuda.synchronize()
        outs.append(out)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    return outs[0].cpu()


def check_padded(tag, lib, act, axis, qkv, n_bh, F, J, cs, spike=False):
    _, atol, rtol, s_atol, s_rtol = TYPES[act]
    out = padded_attention(lib, act, axis, qkv, n_bh, F, J, cs)
    true, pads = unpad_out(out, cs)
    want = ref_attention(qkv.to(TYPES[act][0]).to(torch.float32), n_bh, F, J, cs, HEADS, axis)
    got = true.float().double()
    print(f"{tag}: max |err| vs fp64 {(got - want).abs().max().item():.2e}")
    assert torch.isfinite(got).all()
    assert (pads.float() == 0).all()                        # (exact zeros: V's pad columns are zeros)
    assert torch.allclose(got, want, atol=s_atol if spike else atol, rtol=s_rtol if spike else rtol), (got - want).abs().max().item()


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("cs,J", [(192, 1), (192, 17), (192, 32), (192, 40), (384, 1), (384, 17), (384, 32), (384, 40), (320, 17), (448, 17)])
def test_padded_attention_spatial(lib, cs, J, act):
    """One key, a partial second key tile, two full tiles on the one-wave spatial kernel; 40 joints on the whole-sequence kernel."""
    n_bh, F = 2, 3
    qkv = random_qkv(J * 7 + cs, n_bh * F * J, cs)
    check_padded(f"padded attention cs={cs} act={act} axis=0 J={J}", lib, act, 0, qkv, n_bh, F, J, cs)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("cs,F", [(192, 9), (192, 243), (192, 256), (192, 257), (192, 351), (384, 9), (384, 243), (384, 256), (384, 257),
                                  (384, 351), (320, 243), (448, 257)])
def test_padded_attention_temporal(lib, cs, F, act):
    """Whole-sequence: 2 and 16 key tiles, keys ending inside the last (243) or filling the image (256); chunked keys: the last chunk
    one key in (257) or ending inside a key tile (351)."""
    n_bh, J = (2, 3) if F <= 256 else (1, 3)
    qkv = random_qkv(F * 7 + cs + J, n_bh * F * J, cs)
    check_padded(f"padded attention cs={cs} act={act} axis=1 F={F}", lib, act, 1, qkv, n_bh, F, J, cs)


@pytest.mark.parametrize("act", ACTS)
def test_padded_attention_softmax_spike_in_the_last_chunk(lib, act):
    """test_chunked_key_kernel_softmax_spike_in_the_last_chunk's construction at C = 384: the maximum jumps in the last chunk under
    the 48^-0.5 scale of the true head dim (64^-0.5 would flatten the spike's row and miss the reference)."""
    n_bh, F, J, cs = 1, 351, 17, 384
    qkv = torch.randn(n_bh * F * J, 3 * cs, generator=torch.Generator().manual_seed(5))
    qkv[100 * J + 3, :cs] *= 30.0
    qkv[340 * J + 3, cs:2 * cs] = qkv[100 * J + 3, :cs] / 30.0 * 4.0
    check_padded(f"padded attention spike cs={cs} act={act}", lib, act, 1, qkv, n_bh, F, J, cs, spike=True)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("axis,F,J", [(1, 27, 3), (0, 3, 17)])
def test_padded_heads_do_not_see_each_other(lib, axis, F, J, act):
    """test_heads_do_not_see_each_other at C = 384: head 0's q, k and v columns are NaN in every row; heads 1 .. 7 stay finite, match
    the reference, and their pad columns stay exact zeros."""
    n_bh, cs = 2, 384
    hd = cs // HEADS
    qkv = random_qkv(F * 7 + cs + axis, n_bh * F * J, cs)
    for section in range(3):
        qkv[:, section * cs:section * cs + hd] = float("nan")
    true, pads = unpad_out(padded_attention(lib, act, axis, qkv, n_bh, F, J, cs), cs)
    got = true.float().double()
    want = ref_attention(qkv.to(TYPES[act][0]).to(torch.float32), n_bh, F, J, cs, HEADS, axis)
    _, atol, rtol, _, _ = TYPES[act]
    assert not torch.isfinite(got[:, :hd]).any() and not torch.isfinite(want[:, :hd]).any()
    assert torch.isfinite(got[:, hd:]).all() and (pads[:, 1:].float() == 0).all()
    assert torch.allclose(got[:, hd:], want[:, hd:], atol=atol, rtol=rtol)


def test_plain_impl_1_and_other_true_head_dims_are_still_refused(lib):
    qd = torch.zeros(45, 3 * 512, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(45, 512, dtype=torch.bfloat16, device="cuda")
    for impl, C_ in ((1 | (20 << 8), 256), (1 | (48 << 8), 256), (1 | (24 << 8), 512)):
        assert lib.d3dp_op_attention(1, impl, 1, qd.data_ptr(), out.data_ptr(), 1, 9, 5, C_, HEADS, _lib.current_stream()) == -2
        assert "true head dim" in lib.d3dp_last_error().decode()


# ------------------------------------------------------------------------------------------------ 4: sampler parity
@pytest.mark.parametrize("cs", WIDTHS)
def test_sampler_parity_in_both_modes(monkeypatch, cs):
    """F = 27, dep 2, B 2, H 2, K 2 under flip TTA.  e32 = kernels vs the fp32 oracle, emu32 = the oracle's own 2-byte emulation
    (orc.emulate_bf16; orc._r16 swapped to fp16 for fast16, as test_hip_fast16.py does) vs the fp32 oracle: e32 <= 1.5 emu32 (the
    project's margin for accumulation order), e32 <= FAST_TOL_MM, fast16 closer than fast.  The emulations alone, computed on a CPU:
    1.65 / 2.67 / 2.14 / 2.39 mm (bf16) and 0.199 / 0.195 / 0.177 / 0.204 mm (fp16) at the four widths."""
    switch(monkeypatch)
    frames, dep, B, H, K = 27, 2, 2, 2, 2
    sd = make_state_dict(43, cs, dep, frames)
    x2d = synthetic_inputs_2d(431, B, frames)
    noises = [torch.from_numpy(synthetic_noise(432 + k, (B, H, frames, 17, 3))) for k in range(K)]
    p = orc.strip_prefix(sd)
    want32 = oracle_sample(p, x2d, noises, H, K, dep)
    e32, emu32 = {}, {}
    for numerics, kind in NUMERICS.items():
        saved = orc._r16
        if numerics == "fast16":
            orc._r16 = f16_round
        try:
            emu = oracle_sample(orc.emulate_bf16(p), x2d, noises, H, K, dep)
        finally:
            orc._r16 = saved
        m = sampler_model(sd, frames, cs, dep, H, K, numerics)
        out = sample(m, x2d, noises)
        assert out.shape == (B, K, H, frames, 17, 3) and torch.isfinite(out).all()
        assert m.pose_estimator.fast_operands()[0] == kind and not m.pose_estimator.nonfinite_seen()
        e32[numerics], emu32[numerics] = orc.mpjpe_mm(out.cpu(), want32), orc.mpjpe_mm(emu, want32)
        print(f"cs={cs} {numerics} sampler under D3DP_FAST_IMPL=mfma: kernels vs the fp32 oracle {e32[numerics]:.4f} mm, "
              f"{kind} emulation vs the fp32 oracle {emu32[numerics]:.4f} mm, ratio {e32[numerics] / emu32[numerics]:.3f}")
    for numerics in NUMERICS:
        assert e32[numerics] <= 1.5 * emu32[numerics], (numerics, e32, emu32)
        assert e32[numerics] <= FAST_TOL_MM
    assert e32["fast16"] < e32["fast"]


@pytest.mark.parametrize("cs,heads", [(192, 6), (384, 6), (384, 16), (192, 4)])
def test_denoiser_with_other_head_counts(monkeypatch, cs, heads):
    """The head dims the switch takes beside those of 8 heads: 32 and 64 (no padding: the attention kernels of the instantiated
    widths between the new Linears and row kernels), and 24 / 48 at a width other than the one 8 heads give them (Cp = 512 / 256).
    One denoiser call (F = 27, dep 2, B 2, H 2) against the oracle run with that head count, in the form of test 4: kernels vs
    the fp32 oracle <= 1.5 x the oracle's own 2-byte emulation vs the fp32 oracle, fast16 closer than fast."""
    switch(monkeypatch)
    frames, dep, B, H = 27, 2, 2, 2
    sd, x2d, x3d, t = denoiser_case(47, frames, 17, cs, dep, B, H)
    monkeypatch.setattr(orc, "NUM_HEADS", heads)
    want32 = orc.mixste_forward(sd, x2d, x3d, t, dep)
    e32, emu32 = {}, {}
    for numerics, kind in NUMERICS.items():
        if numerics == "fast16":
            monkeypatch.setattr(orc, "_r16", f16_round)
        emu = orc.mixste_forward(orc.emulate_bf16(sd), x2d, x3d, t, dep)
        m = denoiser(sd, frames, 17, cs, dep, numerics, heads=heads)
        got = m(x2d.cuda(), x3d.cuda(), t.cuda())
        assert got.shape == (B, H, frames, 17, 3) and torch.isfinite(got).all()
        assert m.fast_operands()[0] == kind and not m.nonfinite_seen()
        e32[numerics], emu32[numerics] = orc.mpjpe_mm(got.cpu(), want32), orc.mpjpe_mm(emu, want32)
        print(f"cs={cs} heads={heads} {numerics} denoiser: kernels vs the fp32 oracle {e32[numerics]:.4f} mm, {kind} emulation "
              f"{emu32[numerics]:.4f} mm, ratio {e32[numerics] / emu32[numerics]:.3f}")
    for numerics in NUMERICS:
        assert e32[numerics] <= 1.5 * emu32[numerics], (numerics, e32, emu32)
    assert e32["fast16"] < e32["fast"]


# ------------------------------------------------------------------------------------------------ 5: without the switch
def _tiny_sampler(cs, numerics):
    frames, dep, B, H, K = 9, 1, 1, 2, 1
    sd = make_state_dict(45, cs, dep, frames)
    x2d = synthetic_inputs_2d(451, B, frames)
    noises = [torch.from_numpy(synthetic_noise(452, (B, H, frames, 17, 3)))]
    return sampler_model(sd, frames, cs, dep, H, K, numerics), x2d, noises


@pytest.mark.parametrize("numerics", list(NUMERICS))
def test_without_the_switch_the_width_is_refused_as_before(monkeypatch, numerics):
    switch(monkeypatch, False)
    with pytest.raises(Exception, match="contexts exist for"):
        m, x2d, noises = _tiny_sampler(384, numerics)
        sample(m, x2d, noises)


@pytest.mark.parametrize("numerics", list(NUMERICS))
def test_the_switch_moves_no_bit_at_an_instantiated_width(monkeypatch, numerics):
    outs = []
    for on in (False, True):
        switch(monkeypatch, on)
        m, x2d, noises = _tiny_sampler(512, numerics)
        outs.append(sample(m, x2d, noises).clone())
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ 6: pad columns
@pytest.mark.parametrize("numerics", list(NUMERICS))
def test_pad_columns_never_leak(monkeypatch, numerics):
    """The pad columns of the qkv rows and of the attention output are WRITTEN (exact zeros) by every call, never assumed: a
    workspace full of NaN bit patterns and a zeroed one give the same finite bits."""
    switch(monkeypatch)
    cs, frames, dep, B, H = 384, 27, 2, 1, 2
    sd, x2d, x3d, t = denoiser_case(37, frames, 17, cs, dep, B, H)
    m = denoiser(sd, frames, 17, cs, dep, numerics)
    args = (x2d.cuda(), x3d.cuda(), t.cuda())
    first = m(*args).clone()                                # allocates the workspace
    ws = m._state().ws
    outs = []
    for fill in (0xFF, 0x00):
        torch.cuda.synchronize()
        ws.fill_(fill)
        outs.append(m(*args).clone())
    assert m.fast_operands()[0] == NUMERICS[numerics]
    assert all(torch.isfinite(o).all() for o in outs)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], first)


# ------------------------------------------------------------------------------------------------ 7: pass split
@pytest.mark.parametrize("numerics", list(NUMERICS))
def test_pass_split_changes_no_bit(monkeypatch, numerics):
    """B H = 5 sequences in passes of 2, 2, 1 against one pass of 5."""
    switch(monkeypatch)
    cs, frames, dep, B, H = 384, 27, 2, 1, 5
    sd, x2d, x3d, t = denoiser_case(39, frames, 17, cs, dep, B, H)
    args = (x2d.cuda(), x3d.cuda(), t.cuda())
    m2, m5 = denoiser(sd, frames, 17, cs, dep, numerics, chunk_seqs=2), denoiser(sd, frames, 17, cs, dep, numerics, chunk_seqs=5)
    a, b = m2(*args).clone(), m5(*args).clone()
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert torch.equal(a, m2(*args)) and torch.equal(b, m5(*args))


# ------------------------------------------------------------------------------------------------ 8: the FAST16 fallback
def test_fast16_falls_back_to_a_fast_context_bit_for_bit(monkeypatch):
    """test_fast16_falls_back_to_bf16_when_the_weights_prove_no_range at cs = 384 (its seeds): TTE block 1's qkv matrix x 64 takes
    b_proj to 1.4e5 (fp64: proven_bound_fp64, on the caller's unpadded weights -- zero rows add nothing to any bound).  The fast16
    model reports bf16 operands and a bound >= 65504, warns once, and computes the bits of a `fast` model."""
    switch(monkeypatch)
    frames, cs, dep, B, H, K = 27, 384, 2, 2, 2, 2
    sd = make_state_dict(41, cs, dep, frames)
    key = "pose_estimator.TTEblocks.1.attn.qkv.weight"
    sd[key] = sd[key] * 64.0
    x2d = synthetic_inputs_2d(411, B, frames)
    noises = [torch.from_numpy(synthetic_noise(412 + k, (B, H, frames, 17, 3))) for k in range(K)]
    want_bound, parts = proven_bound_fp64(sd, cs, dep)
    assert want_bound >= FP16_MAX and parts["b_proj"] == want_bound
    m = sampler_model(sd, frames, cs, dep, H, K, "fast16")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = sample(m, x2d, noises)
        out_again = sample(m, x2d, noises)
    said = [w for w in caught if "fast16" in str(w.message)]
    assert len(said) == 1 and "bf16" in str(said[0].message), [str(w.message) for w in caught]
    kind, bound = m.pose_estimator.fast_operands()
    print(f"cs=384 qkv x 64: {kind}, device bound {bound:.4g} (fp64 {want_bound:.4g})")
    assert kind == "bf16" and bound >= FP16_MAX
    assert want_bound * (1 - 1e-6) <= bound <= want_bound * (1 + 1e-3)
    mf = sampler_model(sd, frames, cs, dep, H, K, "fast")
    out_fast = sample(mf, x2d, noises)
    assert mf.pose_estimator.fast_operands() == ("bf16", 0.0)
    assert torch.isfinite(out).all() and torch.isfinite(out_fast).all()
    assert torch.equal(out, out_fast) and torch.equal(out, out_again)


# ------------------------------------------------------------------------------------------------ 9: the workspace
class Guarded:
    """`n` workspace bytes between two guards of a fixed pattern (tests/test_hip_workspace.py)."""
    GUARD, PATTERN = 4096, 0xA5

    def __init__(self, n):
        self.n, self.buf = n, torch.full((n + 2 * self.GUARD,), self.PATTERN, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + self.GUARD
        assert self.ptr % 256 == 0

    def intact(self):
        torch.cuda.synchronize()
        return bool((self.buf[:self.GUARD] == self.PATTERN).all()) and bool((self.buf[self.GUARD + self.n:] == self.PATTERN).all())


@pytest.mark.parametrize("mode", list(NUMERICS))
@pytest.mark.parametrize("cs", [192, 384])
def test_denoise_workspace(monkeypatch, cs, mode):
    """The call runs in exactly d3dp_workspace_bytes (bufA: max(C, Cp) 2-byte columns, bufB: max(3 Cp, hidden)), writes nothing
    outside, computes the same in a roomier one and refuses a smaller one before it writes."""
    switch(monkeypatch)
    F, J, B, H, ESTATE = 9, 5, 1, 2, -4
    c = ab.RawCtx(mode, cs, F, J, 2, 0)
    kind, bound = ab.C.c_int32(), ab.C.c_float()
    _lib.check(c.lib.d3dp_fast_operands(c.ctx, ab.C.byref(kind), ab.C.byref(bound)), "d3dp_fast_operands")
    assert kind.value == (1 if mode == "fast16" else 0)
    n = c.infer_bytes(B, H)
    inputs = c.infer_inputs(B, H)
    tight, roomy = Guarded(n), Guarded(2 * n)
    out = torch.empty(B, H, F, J, 3, device="cuda")
    ref = torch.empty_like(out)
    assert c.denoise(inputs, out, B, H, tight.ptr, n) == 0, c.lib.d3dp_last_error()
    assert tight.intact()
    assert c.denoise(inputs, ref, B, H, roomy.ptr, 2 * n) == 0, c.lib.d3dp_last_error()
    assert roomy.intact()
    assert torch.isfinite(out).all() and torch.equal(out, ref)
    kept = torch.full_like(out, 7.0)
    assert c.denoise(inputs, kept, B, H, tight.ptr, n - 256) == ESTATE
    assert tight.intact() and bool((kept == 7.0).all())


# ------------------------------------------------------------------------------------------------ 10: the stream contract
def _stream_model(monkeypatch):
    switch(monkeypatch)
    cs, frames, dep = 384, 27, 2
    sd = make_state_dict(57, cs, dep, frames, prefix="")
    return denoiser(sd, frames, 17, cs, dep, "fast16")


def _stream_inputs(seed, B=2, H=3, Fr=27):
    return [torch.from_numpy(synthetic_inputs_2d(seed, B, Fr)).cuda(), torch.from_numpy(synthetic_noise(seed + 1, (B, H, Fr, 17, 3))).cuda(),
            torch.tensor([10 + seed, 800], dtype=torch.long).cuda()]


def test_denoiser_on_a_side_stream_equals_the_default_stream(monkeypatch):
    m = _stream_model(monkeypatch)
    args = _stream_inputs(58)
    ref = m.denoise(*args).clone()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = m.denoise(*args).clone()
    s.synchronize()
    assert m.fast_operands()[0] == "fp16"
    assert torch.isfinite(ref).all() and torch.equal(ref, got)


def test_denoise_is_capturable(monkeypatch):
    """One eager call, then the same call captured into a graph: the replay on new inputs computes the eager call's bits."""
    m = _stream_model(monkeypatch)
    x2d, x3d, t = _stream_inputs(58)
    out = torch.empty(tuple(x3d.shape), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.denoise(x2d, x3d, t, out=out)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        m.denoise(x2d, x3d, t, out=out)
    new = _stream_inputs(300)
    for buf, v in zip((x2d, x3d, t), new):
        buf.copy_(v)
    g.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    eager = m.denoise(*new)
    torch.cuda.synchronize()
    assert m.fast_operands()[0] == "fp16"
    assert torch.isfinite(eager).all() and torch.equal(eager, replayed)
