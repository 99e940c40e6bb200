"""GPU tests of numerics='fast16' (D3DP_MODE_FAST16): FAST mode's kernels instantiated for IEEE fp16 operands, behind the range
proof of d3dp_set_weights (include/d3dp_hip.h: d3dp_fast_operands).

  1. accuracy against the oracle, adaptively (the oracle's FAST emulation re-run with an fp16 rounding);
  2. the proven bound against the stated formula in fp64;
  3. the fallback to the bf16 kernels when the bound reaches 65504 -- bit for bit what numerics='fast' computes;
  4. non-finite weights;
  5. the routes around the MFMA attention kernels (more than 32 joints, clips beyond 256 frames, head dim 16);
  6. one operator each through the C ABI on fp16 operands;
  7. the stream contract: side stream, two contexts in one process, stream capture.
"""
import warnings
from types import SimpleNamespace

import pytest
import torch

from d3dp_amd import D3DP, _lib
from d3dp_amd.model import MixSTE2
from d3dp_amd.weights import (H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, flip_2d, make_state_dict, synthetic_inputs_2d,
                              synthetic_noise)
from oracle import d3dp_oracle as orc

pytestmark = pytest.mark.gpu
FP16_MAX = 65504.0


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def stream():
    return _lib.current_stream()


def f16_round(t):
    return t.to(torch.float16).to(torch.float32)


def sampler_model(sd, frames, cs, dep, H, K, numerics):
    args = SimpleNamespace(number_of_frames=frames, test_time_augmentation=True, timestep=1000, scale=1.0, cs=cs, dep=dep)
    m = D3DP(args, H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, is_train=False, num_proposals=H, sampling_timesteps=K, numerics=numerics)
    m.load_state_dict(sd, strict=False)
    return m.cuda().eval()


def sample(m, x2d, noises):
    return m(torch.from_numpy(x2d).cuda(), None, input_2d_flip=torch.from_numpy(flip_2d(x2d)).cuda(), noise=noises)


def oracle_sample(p, x2d, noises, H, K, dep):
    return orc.ddim_sample_flip(p, orc.cosine_schedule(1000), torch.from_numpy(x2d), torch.from_numpy(flip_2d(x2d)), H, K, dep,
                                H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, noises)


def proven_bound_fp64(sd, cs, dep, prefix="pose_estimator."):
    """The table of include/d3dp_hip.h (d3dp_fast_operands) in fp64: the largest, over all blocks, of L1, L2, b_qkv, b_proj, b_h,
    b_fc2 and max |w| of the four matrices; also returns the per-name maxima."""
    sq = (cs - 1) ** 0.5
    worst = {}

    def note(name, v):
        worst[name] = max(worst.get(name, 0.0), float(v))

    for kind in ("STEblocks", "TTEblocks"):
        for d in range(dep):
            g = lambda n: sd[f"{prefix}{kind}.{d}.{n}"].double()
            in1 = sq * g("norm1.weight").abs() + g("norm1.bias").abs()
            in2 = sq * g("norm2.weight").abs() + g("norm2.bias").abs()
            rows = g("attn.qkv.weight").abs() @ in1 + g("attn.qkv.bias").abs()
            b_v = rows[2 * cs:].max()
            b_h = (g("mlp.fc1.weight").abs() @ in2 + g("mlp.fc1.bias").abs()).max()
            note("L", max(in1.max(), in2.max()))
            note("b_qkv", rows.max())
            note("b_proj", (g("attn.proj.weight").abs().sum(dim=1) * b_v + g("attn.proj.bias").abs()).max())
            note("b_h", b_h)
            note("b_fc2", (g("mlp.fc2.weight").abs().sum(dim=1) * b_h + g("mlp.fc2.bias").abs()).max())
            note("w", max(g(n).abs().max() for n in ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight")))
    return max(worst.values()), worst


# ------------------------------------------------------------------------------------------------ 1, 2: accuracy and the proof
@pytest.mark.parametrize("frames,B,H,K", [(27, 2, 2, 2), (243, 1, 1, 1)])
def test_sampler_fast16_vs_fp16_emulating_oracle(frames, B, H, K):
    """The inputs of test_sampler_fast_mode_vs_bf16_emulating_oracle.  The oracle's FAST emulation rounds through the module-level
    orc._r16; here it rounds to fp16 instead (swapped for the run, restored after).  e32 = kernels vs the fp32 oracle, emu32 = the
    fp16 emulation vs the fp32 oracle: e32 <= 1.5 emu32 (the margin of the bf16 gate, for its reason: accumulation order) and
    e32 < 0.4 x the `fast` model's distance to the fp32 oracle on the same inputs (the ratio of the fp16-variants test; the
    emulations alone sit at 0.10 and 0.16, computed on a CPU: 0.316 mm against 3.32 mm and 0.342 mm against 2.11 mm)."""
    sd = make_state_dict(7, 512, 8, frames)
    x2d = synthetic_inputs_2d(81, B, frames)
    noises = [torch.from_numpy(synthetic_noise(90 + k, (B, H, frames, 17, 3))) for k in range(K)]
    p = orc.strip_prefix(sd)
    want32 = oracle_sample(p, x2d, noises, H, K, 8)
    saved = orc._r16
    orc._r16 = f16_round
    try:
        want16 = oracle_sample(orc.emulate_bf16(p), x2d, noises, H, K, 8)
    finally:
        orc._r16 = saved
    assert torch.isfinite(want32).all() and torch.isfinite(want16).all()
    m = sampler_model(sd, frames, 512, 8, H, K, "fast16")
    out = sample(m, x2d, noises).cpu()
    kind, bound = m.pose_estimator.fast_operands()
    mf = sampler_model(sd, frames, 512, 8, H, K, "fast")
    out_fast = sample(mf, x2d, noises).cpu()
    e32, emu32, fast32 = orc.mpjpe_mm(out, want32), orc.mpjpe_mm(want16, want32), orc.mpjpe_mm(out_fast, want32)
    print(f"fast16 F={frames}: kernels vs fp32 oracle {e32:.3f} mm (fp16 emulation vs fp32 oracle {emu32:.3f} mm; kernels vs "
          f"emulation {orc.mpjpe_mm(out, want16):.3f} mm); fast (bf16) vs fp32 oracle {fast32:.3f} mm; ratio {e32 / fast32:.3f}; "
          f"operands {kind}, proven bound {bound:.1f}")
    assert kind == "fp16" and mf.pose_estimator.fast_operands() == ("bf16", 0.0)
    assert torch.isfinite(out).all() and not m.pose_estimator.nonfinite_seen()
    assert e32 <= 1.5 * emu32
    assert e32 < 0.4 * fast32


def test_the_proven_bound_is_the_stated_formula():
    """d3dp_fast_operands' bound for make_state_dict(7, 512, 8, 243) against the table computed here in fp64: never below it
    (device >= fp64 (1 - 1e-6)) and not looser than stated (device <= fp64 (1 + 1e-3)).  The seed weights leave a factor 13.8."""
    frames, cs, dep = 243, 512, 8
    sd = make_state_dict(7, cs, dep, frames)
    want, parts = proven_bound_fp64(sd, cs, dep)
    m = sampler_model(sd, frames, cs, dep, 1, 1, "fast16")
    m.pose_estimator._context(torch.device("cuda", torch.cuda.current_device()))      # create + set_weights, no forward needed
    kind, bound = m.pose_estimator.fast_operands()
    print(f"proven bound: device {bound:.4f}, fp64 {want:.4f} ({', '.join('%s %.1f' % kv for kv in parts.items())}); "
          f"{FP16_MAX / bound:.1f}x below 65504")
    assert kind == "fp16"
    assert bound >= want * (1 - 1e-6)
    assert bound <= want * (1 + 1e-3)
    assert abs(want - 4762.0) < 1.0 and parts["b_fc2"] == want        # (the figure the documents quote)


# ------------------------------------------------------------------------------------------------ 3, 4: fallback
def _fallback_case(factor):
    frames, cs, dep, B, H, K = 27, 512, 2, 2, 2, 2
    sd = make_state_dict(41, cs, dep, frames)
    for n in ("weight", "bias"):
        key = f"pose_estimator.TTEblocks.1.norm1.{n}"
        sd[key] = sd[key] * float(factor)
    x2d = synthetic_inputs_2d(411, B, frames)
    noises = [torch.from_numpy(synthetic_noise(412 + k, (B, H, frames, 17, 3))) for k in range(K)]
    return sd, (frames, cs, dep, H, K), x2d, noises


@pytest.mark.parametrize("factor", [32, 256])
def test_fast16_falls_back_to_bf16_when_the_weights_prove_no_range(factor):
    """TTEblocks.1.norm1 gain and bias x 32: b_proj becomes 1.09e5 while b_qkv stays 8.9e3 (only the branch-output bound trips);
    x 256: b_qkv 7.1e4 trips as well.  The fast16 model reports bf16 operands and a bound >= 65504, warns once, and computes
    the bits of a `fast` model on the same weights, inputs and noises."""
    sd, (frames, cs, dep, H, K), x2d, noises = _fallback_case(factor)
    want_bound, parts = proven_bound_fp64(sd, cs, dep)
    m = sampler_model(sd, frames, cs, dep, H, K, "fast16")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = sample(m, x2d, noises)
        out_again = sample(m, x2d, noises)
    said = [w for w in caught if "fast16" in str(w.message)]
    assert len(said) == 1 and "bf16" in str(said[0].message), [str(w.message) for w in caught]
    kind, bound = m.pose_estimator.fast_operands()
    print(f"factor {factor}: {kind}, device bound {bound:.4g} (fp64 {want_bound:.4g}; b_qkv {parts['b_qkv']:.3g}, b_proj {parts['b_proj']:.3g})")
    assert kind == "bf16" and bound >= FP16_MAX
    assert (parts["b_qkv"] < FP16_MAX) == (factor == 32) and parts["b_proj"] >= FP16_MAX
    assert want_bound * (1 - 1e-6) <= bound <= want_bound * (1 + 1e-3)
    mf = sampler_model(sd, frames, cs, dep, H, K, "fast")
    out_fast = sample(mf, x2d, noises)
    assert torch.isfinite(out).all() and torch.isfinite(out_fast).all()
    assert torch.equal(out, out_fast) and torch.equal(out, out_again)
    assert not m.pose_estimator.nonfinite_seen()


def test_fast16_runs_fp16_on_the_unscaled_weights_of_the_fallback_case():
    sd, (frames, cs, dep, H, K), x2d, noises = _fallback_case(1)
    m = sampler_model(sd, frames, cs, dep, H, K, "fast16")
    with warnings.catch_warnings():
        warnings.simplefilter("error")                 # no fallback warning here
        out = sample(m, x2d, noises)
    kind, bound = m.pose_estimator.fast_operands()
    assert kind == "fp16" and 0.0 < bound < FP16_MAX
    out_fast = sample(sampler_model(sd, frames, cs, dep, H, K, "fast"), x2d, noises)
    assert torch.isfinite(out).all() and not torch.equal(out, out_fast)      # (other kernels did run)


def test_fast16_with_a_non_finite_weight_behaves_as_fast():
    sd, (frames, cs, dep, H, K), x2d, noises = _fallback_case(1)
    key = "pose_estimator.TTEblocks.0.attn.proj.weight"
    sd[key] = sd[key].clone()
    sd[key].view(-1)[3] = float("inf")
    m = sampler_model(sd, frames, cs, dep, H, K, "fast16")
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        out = sample(m, x2d, noises)                   # loads and runs: never an error
    kind, bound = m.pose_estimator.fast_operands()
    assert kind == "bf16" and bound == float("inf")
    mf = sampler_model(sd, frames, cs, dep, H, K, "fast")
    out_fast = sample(mf, x2d, noises)
    assert m.pose_estimator.nonfinite_seen() and mf.pose_estimator.nonfinite_seen()
    assert torch.equal(out.view(torch.int32), out_fast.view(torch.int32))    # bit-equal, nan payloads included


# ------------------------------------------------------------------------------------------------ 5: routes around the MFMA attention
def test_fast16_denoiser_with_more_than_32_joints():
    """(J, cs, F) = (40, 512, 27): the spatial axis runs the row kernel on fp16 rows (test_denoiser_with_more_than_32_joints)."""
    joints, cs, frames, B, H, dep = 40, 512, 27, 2, 2, 2
    sd = make_state_dict(37, cs, dep, frames, prefix="", joints=joints)
    g = torch.Generator().manual_seed(joints * 7 + cs)
    x2d = torch.rand(B, frames, joints, 2, generator=g) * 2 - 1
    x3d = torch.randn(B, H, frames, joints, 3, generator=g)
    t = torch.tensor([999, 120])
    want = orc.mixste_forward(sd, x2d, x3d, t, dep)
    errs = {}
    for numerics in ("fast16", "fast"):
        m = MixSTE2(num_frame=frames, num_joints=joints, embed_dim_ratio=cs, depth=dep, is_train=False, numerics=numerics,
                    drop_path_rate=0.0)
        m.load_state_dict(sd, strict=True)
        m = m.cuda().eval()
        got = m(x2d.cuda(), x3d.cuda(), t.cuda())
        assert got.shape == (B, H, frames, joints, 3) and torch.isfinite(got).all()
        assert m.fast_operands()[0] == ("fp16" if numerics == "fast16" else "bf16")
        errs[numerics] = orc.mpjpe_mm(got.cpu(), want)
    print(f"J=40: fast16 {errs['fast16']:.3f} mm, fast {errs['fast']:.3f} mm vs the fp32 oracle")
    assert errs["fast16"] < errs["fast"]


@pytest.mark.parametrize("frames,cs", [(351, 512), (27, 128)])
def test_fast16_sampler_on_the_row_attention_kernel(frames, cs):
    """F = 351 (temporal axis beyond the MFMA kernel's LDS images) and cs = 128 (head dim 16: both axes on the row kernel):
    the inputs of test_sampler_on_a_clip_longer_than_256_frames / test_sampler_at_the_reference_small_width."""
    dep, H, K = 2, 2, 2
    seed, B, s2d, sn = (13, 1, 131, 140) if frames == 351 else (29, 2, 291, 292)
    sd = make_state_dict(seed, cs, dep, frames)
    x2d = synthetic_inputs_2d(s2d, B, frames)
    noises = [torch.from_numpy(synthetic_noise(sn + k, (B, H, frames, 17, 3))) for k in range(K)]
    want = oracle_sample(orc.strip_prefix(sd), x2d, noises, H, K, dep)
    errs = {}
    for numerics in ("fast16", "fast"):
        m = sampler_model(sd, frames, cs, dep, H, K, numerics)
        out = sample(m, x2d, noises)
        assert out.shape == (B, K, H, frames, 17, 3) and torch.isfinite(out).all()
        assert m.pose_estimator.fast_operands()[0] == ("fp16" if numerics == "fast16" else "bf16")
        errs[numerics] = orc.mpjpe_mm(out.cpu(), want)
    print(f"F={frames} cs={cs}: fast16 {errs['fast16']:.3f} mm, fast {errs['fast']:.3f} mm vs the fp32 oracle")
    assert errs["fast16"] < errs["fast"]


# ------------------------------------------------------------------------------------------------ 6: single operators
@pytest.mark.parametrize("M,N,K", [(4131, 1536, 512), (300, 512, 1024), (17, 1024, 512)])
def test_linear_fp16_all_epilogues(lib, M, N, K):
    """test_linear_all_epilogues' FAST cases on fp16 operands (d3dp_op_linear mode 4) against fp64 torch on fp16-rounded inputs, at
    that test's bf16 tolerances divided by 8 (three more significand bits, O(1) values).  The streaming kernel parks finished
    tiles as packed fp16 even for fp32 output."""
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    bias = torch.randn(N, generator=g)
    lin = f16_round(A).double() @ f16_round(W).double().t() + bias.double()
    Ad, Wd, bd = A.half().cuda().contiguous(), W.half().cuda().contiguous(), bias.cuda()
    for epi, want in ((_lib.EPI_BIAS, lin), (_lib.EPI_GELU, torch.nn.functional.gelu(lin)), (_lib.EPI_BIAS | 16, lin)):
        out = torch.full((M, N), float("nan"), dtype=torch.float32 if epi & 16 else torch.float16, device="cuda")
        _lib.check(lib.d3dp_op_linear(_lib.OP_FP16, epi, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), out.data_ptr(), M, N, K, stream()))
        torch.cuda.synchronize()
        got = out.float().cpu().double()
        print(f"linear fp16 {M}x{N}x{K} epi {epi}: max |err| {(got - want).abs().max().item():.2e}")
        assert torch.allclose(got, want, atol=2.5e-3, rtol=1.25e-3), (epi, (got - want).abs().max().item())


@pytest.mark.parametrize("impl,axis,F", [(1, 0, 27), (1, 0, 243), (1, 1, 27), (1, 1, 243), (0, 1, 351), (0, 0, 27)])
def test_attention_fp16(lib, impl, axis, F):
    """test_attention's bf16 cases on fp16 rows (act code 4): the MFMA kernels on both axes, the row kernel at F = 351."""
    from test_hip_parity import ref_attention
    n_bh, J, heads, C_ = 2, 17, 8, 512
    g = torch.Generator().manual_seed(F * 7 + C_ + axis)
    qkv = torch.randn(n_bh * F * J, 3 * C_, generator=g)
    qkv[:, :C_] *= 2.0
    want = ref_attention(f16_round(qkv), n_bh, F, J, C_, heads, axis)
    qd = qkv.half().cuda().contiguous()
    out = torch.full((n_bh * F * J, C_), float("nan"), dtype=torch.float16, device="cuda")
    _lib.check(lib.d3dp_op_attention(_lib.OP_FP16, impl, axis, qd.data_ptr(), out.data_ptr(), n_bh, F, J, C_, heads, stream()))
    torch.cuda.synchronize()
    got = out.float().cpu().double()
    print(f"attention fp16 impl={impl} axis={axis} F={F}: max |err| {(got - want).abs().max().item():.2e}")
    assert torch.isfinite(got).all()
    assert torch.allclose(got, want, atol=2.5e-3, rtol=1.25e-3), (got - want).abs().max().item()


def test_attention_fp16_softmax_spike(lib):
    """test_attention_softmax_spike's bf16 case on fp16 rows (the raw score of the spiked pair is in the thousands: fp32 inside the
    kernel, and q, k themselves stay far below 65504)."""
    from test_hip_parity import ref_attention
    n_bh, F, J, C_, heads = 1, 243, 17, 512, 8
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(n_bh * F * J, 3 * C_, generator=g)
    qkv[100 * J + 3, :C_] *= 30.0
    qkv[7 * J + 3, C_:2 * C_] = qkv[100 * J + 3, :C_] / 30.0 * 4.0
    want = ref_attention(f16_round(qkv), n_bh, F, J, C_, heads, 1)
    qd = qkv.half().cuda().contiguous()
    out = torch.empty((n_bh * F * J, C_), dtype=torch.float16, device="cuda")
    _lib.check(lib.d3dp_op_attention(_lib.OP_FP16, 1, 1, qd.data_ptr(), out.data_ptr(), n_bh, F, J, C_, heads, stream()))
    got = out.float().cpu().double()
    print(f"attention fp16 spike: max |err| {(got - want).abs().max().item():.2e}")
    assert torch.isfinite(got).all()
    assert torch.allclose(got, want, atol=3.75e-3, rtol=2.5e-3)


@pytest.mark.parametrize("C_", [64, 128, 512])
def test_layernorm_fp16_output(lib, C_):
    T = 1001
    g = torch.Generator().manual_seed(C_)
    x = torch.randn(T, C_, generator=g) * 3 + 0.5
    w, b = torch.randn(C_, generator=g), torch.randn(C_, generator=g)
    want = torch.nn.functional.layer_norm(x.double(), (C_,), w.double(), b.double(), 1e-6)
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    out = torch.full((T, C_), float("nan"), dtype=torch.float16, device="cuda")
    _lib.check(lib.d3dp_op_layernorm(_lib.OP_FP16, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), 1e-6, out.data_ptr(), T, C_, stream()))
    got = out.float().cpu().double()
    print(f"layernorm fp16 C={C_}: max |err| {(got - want).abs().max().item():.2e}")
    assert torch.allclose(got, want, atol=3.75e-3, rtol=1.25e-3)
    # ... and it is the fp16 rounding of the fp32 kernel's result, bit for bit, at every width (the single-value store path of
    # C = 64 / 128 included: pointwise.hip keeps the compiler from merging the cast into v_fma_mixlo_f16, which rounds once)
    out32 = torch.empty((T, C_), device="cuda")
    _lib.check(lib.d3dp_op_layernorm(0, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), 1e-6, out32.data_ptr(), T, C_, stream()))
    print(f"layernorm fp16 C={C_}: {(out != out32.half()).sum().item()} of {out.numel()} elements differ from the cast of the fp32 kernel's")
    assert torch.equal(out, out32.half())


# ------------------------------------------------------------------------------------------------ 7: the stream contract
def _small_case(numerics, seed=57):
    frames, cs, dep, B, H, K = 27, 512, 2, 2, 2, 2
    sd = make_state_dict(seed, cs, dep, frames)
    m = sampler_model(sd, frames, cs, dep, H, K, numerics)
    x2d = synthetic_inputs_2d(seed + 1, B, frames)
    noises = [torch.from_numpy(synthetic_noise(seed + 2 + k, (B, H, frames, 17, 3))).cuda() for k in range(K)]
    return m, x2d, noises


def test_fast16_sampler_on_a_side_stream_equals_the_default_stream():
    m, x2d, noises = _small_case("fast16")
    ref = sample(m, x2d, noises)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = sample(m, x2d, noises)
    s.synchronize()
    assert m.pose_estimator.fast_operands()[0] == "fp16"
    assert torch.isfinite(ref).all() and torch.equal(ref, got)


def test_a_fast_and_a_fast16_context_in_one_process_do_not_disturb_each_other():
    m16, x2d, noises = _small_case("fast16")
    mf, _, _ = _small_case("fast")
    solo16, solof = sample(m16, x2d, noises).clone(), sample(mf, x2d, noises).clone()
    for _ in range(2):
        a = sample(m16, x2d, noises)
        b = sample(mf, x2d, noises)
        assert torch.equal(a, solo16) and torch.equal(b, solof)
    assert m16.pose_estimator.fast_operands()[0] == "fp16" and mf.pose_estimator.fast_operands()[0] == "bf16"
    assert not torch.equal(solo16, solof)


def test_fast16_denoise_is_capturable():
    """One eager call, then the same call captured into a graph: the replay on new inputs computes the eager call's bits."""
    B, H, Fr = 2, 3, 27
    m, _, _ = _small_case("fast16")
    pe = m.pose_estimator
    x2d = torch.from_numpy(synthetic_inputs_2d(58, B, Fr)).cuda()
    x3d = torch.from_numpy(synthetic_noise(59, (B, H, Fr, 17, 3))).cuda()
    t, out = torch.tensor([10, 800], dtype=torch.long).cuda(), torch.empty((B, H, Fr, 17, 3), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pe.denoise(x2d, x3d, t, out=out)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        pe.denoise(x2d, x3d, t, out=out)
    new = [torch.from_numpy(synthetic_inputs_2d(300, B, Fr)).cuda(), torch.from_numpy(synthetic_noise(310, (B, H, Fr, 17, 3))).cuda(),
           torch.tensor([500, 3], dtype=torch.long).cuda()]
    for buf, v in zip((x2d, x3d, t), new):
        buf.copy_(v)
    g.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    eager = pe.denoise(*new)
    torch.cuda.synchronize()
    assert pe.fast_operands()[0] == "fp16"
    assert torch.isfinite(eager).all() and torch.equal(eager, replayed)
