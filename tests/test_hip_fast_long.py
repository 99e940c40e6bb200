"""GPU tests of FAST / FAST16 attention on the matrix cores beyond the whole-sequence kernels' reach: more than 256 frames on the
chunked-key kernel (attention_fast.hip attn_long2_bf16_kernel: keys through LDS in chunks of 128 under an online softmax), more than
32 joints on the whole-sequence kernel with the spatial SeqMap.  cs = 512, 8 heads (head dim 64) throughout.

  1. the operator on the temporal axis, 257 ... 1024 frames, both 2-byte types;
  2. the online softmax rescaling in both directions (maximum set in the first chunk / raised in the last);
  3. more work units than resident workgroups (the grid is persistent);
  4. the operator on the spatial axis, 33 ... 256 joints;
  5. the contexts take the new kernels, and D3DP_LONG_ATTN=rows takes the row kernel back;
  6. the stream contract at a long shape: side stream, capture and replay;
  7. shapes the whole-sequence kernels already served do not move.

Operator references: fp64 softmax attention on operands rounded to the 2-byte type (test_hip_parity.ref_attention), at the
tolerances of test_attention (bf16) and test_attention_fp16; the spike cases at those of the two spike tests.  End-to-end
references: oracle.d3dp_oracle in fp32, at FAST_TOL_MM.
"""
import pytest
import torch

from d3dp_amd import _lib
from d3dp_amd.model import MixSTE2
from d3dp_amd.weights import make_state_dict, synthetic_inputs_2d, synthetic_noise
from oracle import d3dp_oracle as orc
from test_hip_fast16 import oracle_sample, sample, sampler_model
from test_hip_parity import FAST_TOL_MM, ref_attention

pytestmark = pytest.mark.gpu
C_, HEADS = 512, 8
# act code of d3dp_op_attention -> (torch type, atol, rtol, spike atol, spike rtol)
TYPES = {1: (torch.bfloat16, 2e-2, 1e-2, 3e-2, 2e-2), 4: (torch.float16, 2.5e-3, 1.25e-3, 3.75e-3, 2.5e-3)}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def op_attention(lib, act, impl, axis, qkv, n_bh, F, J):
    """d3dp_op_attention on `qkv` (fp32, CPU) rounded to the type of `act`, into a NaN-filled output: the 2-byte device result."""
    qd = qkv.to(TYPES[act][0]).cuda().contiguous()
    out = torch.full((n_bh * F * J, C_), float("nan"), dtype=qd.dtype, device="cuda")
    _lib.check(lib.d3dp_op_attention(act, impl, axis, qd.data_ptr(), out.data_ptr(), n_bh, F, J, C_, HEADS, _lib.current_stream()))
    torch.cuda.synchronize()
    return out


def check_against_reference(tag, out, qkv, act, n_bh, F, J, axis, spike=False):
    dt, atol, rtol, s_atol, s_rtol = TYPES[act]
    want = ref_attention(qkv.to(dt).to(torch.float32), n_bh, F, J, C_, HEADS, axis)
    got = out.float().cpu().double()
    print(f"{tag}: max |err| vs fp64 {(got - want).abs().max().item():.2e}")
    assert torch.isfinite(got).all()
    assert torch.allclose(got, want, atol=s_atol if spike else atol, rtol=s_rtol if spike else rtol), (got - want).abs().max().item()


def random_qkv(seed, rows):
    qkv = torch.randn(rows, 3 * C_, generator=torch.Generator().manual_seed(seed))
    qkv[:, :C_] *= 2.0        # sharpen the softmax a little
    return qkv


# ------------------------------------------------------------------------------------------------ 1: operator, temporal axis
@pytest.mark.parametrize("act", [1, 4])
@pytest.mark.parametrize("n_bh,J,F", [(2, 17, 257), (1, 17, 288), (1, 17, 351), (1, 5, 384), (1, 5, 512), (1, 5, 513), (1, 3, 1024)])
def test_attention_beyond_256_frames(lib, act, n_bh, J, F):
    """The last chunk ends one key in (257, 513), inside a key tile (351), on a tile-pair boundary (288) and on a chunk boundary
    for chunks of 128 (384) or of either size (512, 1024); the last query group holds one tile (257, 513), several (288, 351)
    or all eight (384, 512, 1024); 1024 is the library's maximum."""
    qkv = random_qkv(F * 7 + C_ + 1, n_bh * F * J)
    out = op_attention(lib, act, 1, 1, qkv, n_bh, F, J)
    check_against_reference(f"attention act={act} impl=1 axis=1 F={F}", out, qkv, act, n_bh, F, J, 1)


# ------------------------------------------------------------------------------------------------ 2: rescaling both ways
@pytest.mark.parametrize("act", [1, 4])
@pytest.mark.parametrize("key_frame", [3, 340])
def test_attention_softmax_spike_across_chunks(lib, act, key_frame):
    """test_attention_softmax_spike's construction at F = 351: query row (frame 100, joint 3) x 30, its matching key at frame 3
    (the row maximum is set in the first chunk and no later chunk rescales) or at frame 340 (the maximum jumps in the last chunk
    and everything accumulated before is rescaled, to nearly nothing)."""
    n_bh, F, J = 1, 351, 17
    qkv = torch.randn(n_bh * F * J, 3 * C_, generator=torch.Generator().manual_seed(5))
    qkv[100 * J + 3, :C_] *= 30.0
    qkv[key_frame * J + 3, C_:2 * C_] = qkv[100 * J + 3, :C_] / 30.0 * 4.0
    out = op_attention(lib, act, 1, 1, qkv, n_bh, F, J)
    check_against_reference(f"attention spike act={act} key at frame {key_frame}", out, qkv, act, n_bh, F, J, 1, spike=True)


# ------------------------------------------------------------------------------------------------ 3: persistent grid
@pytest.mark.parametrize("act", [1, 4])
def test_attention_beyond_256_frames_more_units_than_workgroups(lib, act):
    """816 (sequence, head) problems x 3 query groups = 2448 work units on a grid of two workgroups per CU: every workgroup walks
    several units, each starting in the LDS buffers the one before it was read from.  Against the reference, and run to run."""
    n_bh, J, F = 6, 17, 257
    qkv = random_qkv(257, n_bh * F * J)
    out = op_attention(lib, act, 1, 1, qkv, n_bh, F, J)
    check_against_reference(f"attention act={act} 2448 work units", out, qkv, act, n_bh, F, J, 1)
    assert torch.equal(out, op_attention(lib, act, 1, 1, qkv, n_bh, F, J))


# ------------------------------------------------------------------------------------------------ 4: operator, spatial axis
@pytest.mark.parametrize("act", [1, 4])
@pytest.mark.parametrize("J", [33, 40, 72, 256])
def test_attention_more_than_32_joints(lib, act, J):
    n_bh, F = 2, 3
    qkv = random_qkv(J * 7 + C_, n_bh * F * J)
    out = op_attention(lib, act, 1, 0, qkv, n_bh, F, J)
    check_against_reference(f"attention act={act} impl=1 axis=0 J={J}", out, qkv, act, n_bh, F, J, 0)


# ------------------------------------------------------------------------------------------------ 5: what the contexts launch
def _report_default_and_rows(tag, runs, want):
    """runs[(numerics, switch)] -> output.  Every run within FAST_TOL_MM of the fp32 oracle, fast16 closer than fast under either
    setting, and the two settings of a mode differ in some bit (different kernels ran)."""
    errs = {k: orc.mpjpe_mm(v.cpu(), want) for k, v in runs.items()}
    print(f"{tag} vs the fp32 oracle: " + ", ".join(f"{n}{'' if s == 'default' else ':rows'} {e:.4f} mm" for (n, s), e in errs.items()))
    for v in runs.values():
        assert torch.isfinite(v).all()
    assert all(e <= FAST_TOL_MM for e in errs.values()), errs
    for switch in ("default", "rows"):
        assert errs[("fast16", switch)] < errs[("fast", switch)], errs
    for numerics in ("fast", "fast16"):
        assert not torch.equal(runs[(numerics, "default")], runs[(numerics, "rows")]), numerics


def _set_switch(monkeypatch, switch):
    if switch == "rows":
        monkeypatch.setenv("D3DP_LONG_ATTN", "rows")       # (read when the model's first call creates its context)
    else:
        monkeypatch.delenv("D3DP_LONG_ATTN", raising=False)


def test_fast_contexts_run_the_chunked_key_kernel_beyond_256_frames(monkeypatch):
    """The inputs of test_sampler_on_a_clip_longer_than_256_frames (F = 351, dep 2, B 1, H 2, K 2)."""
    frames, cs, dep, B, H, K = 351, C_, 2, 1, 2, 2
    sd = make_state_dict(13, cs, dep, frames)
    x2d = synthetic_inputs_2d(131, B, frames)
    noises = [torch.from_numpy(synthetic_noise(140 + k, (B, H, frames, 17, 3))) for k in range(K)]
    want = oracle_sample(orc.strip_prefix(sd), x2d, noises, H, K, dep)
    runs = {}
    for switch in ("default", "rows"):
        _set_switch(monkeypatch, switch)
        for numerics in ("fast", "fast16"):
            m = sampler_model(sd, frames, cs, dep, H, K, numerics)
            runs[(numerics, switch)] = sample(m, x2d, noises)
            assert m.pose_estimator.fast_operands()[0] == ("fp16" if numerics == "fast16" else "bf16")
    _report_default_and_rows("F=351 sampler", runs, want)


def test_fast_contexts_run_the_whole_sequence_kernel_beyond_32_joints(monkeypatch):
    """The (J, F) = (40, 27) denoiser of test_denoiser_with_more_than_32_joints."""
    joints, cs, frames, B, H, dep = 40, C_, 27, 2, 2, 2
    sd = make_state_dict(37, cs, dep, frames, prefix="", joints=joints)
    g = torch.Generator().manual_seed(joints * 7 + cs)
    x2d = torch.rand(B, frames, joints, 2, generator=g) * 2 - 1
    x3d = torch.randn(B, H, frames, joints, 3, generator=g)
    t = torch.tensor([999, 120])
    want = orc.mixste_forward(sd, x2d, x3d, t, dep)
    runs = {}
    for switch in ("default", "rows"):
        _set_switch(monkeypatch, switch)
        for numerics in ("fast", "fast16"):
            m = MixSTE2(num_frame=frames, num_joints=joints, embed_dim_ratio=cs, depth=dep, is_train=False, numerics=numerics,
                        drop_path_rate=0.0)
            m.load_state_dict(sd, strict=True)
            runs[(numerics, switch)] = m.cuda().eval()(x2d.cuda(), x3d.cuda(), t.cuda())
            assert m.fast_operands()[0] == ("fp16" if numerics == "fast16" else "bf16")
    _report_default_and_rows("J=40 denoiser", runs, want)


# ------------------------------------------------------------------------------------------------ 6: the stream contract
def _long_denoiser_case(seed=61):
    frames, cs, dep, B, H = 257, C_, 2, 2, 2
    pe = sampler_model(make_state_dict(seed, cs, dep, frames), frames, cs, dep, H, 2, "fast16").pose_estimator
    make = lambda s: (torch.from_numpy(synthetic_inputs_2d(s, B, frames)).cuda(),
                      torch.from_numpy(synthetic_noise(s + 1, (B, H, frames, 17, 3))).cuda())
    return pe, make, (B, H, frames, 17, 3)


def test_fast16_long_clip_denoiser_on_a_side_stream_equals_the_default_stream():
    pe, make, _ = _long_denoiser_case()
    x2d, x3d = make(62)
    t = torch.tensor([10, 800], dtype=torch.long).cuda()
    ref = pe.denoise(x2d, x3d, t)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = pe.denoise(x2d, x3d, t)
    s.synchronize()
    assert pe.fast_operands()[0] == "fp16"
    assert torch.isfinite(ref).all() and torch.equal(ref, got)


def test_fast16_long_clip_denoise_is_capturable():
    """One eager call, then the same call captured into a graph: the replay on new inputs computes the eager call's bits."""
    pe, make, shape = _long_denoiser_case()
    x2d, x3d = make(64)
    t, out = torch.tensor([10, 800], dtype=torch.long).cuda(), torch.empty(shape, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pe.denoise(x2d, x3d, t, out=out)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        pe.denoise(x2d, x3d, t, out=out)
    new = [*make(300), torch.tensor([500, 3], dtype=torch.long).cuda()]
    for buf, v in zip((x2d, x3d, t), new):
        buf.copy_(v)
    g.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    eager = pe.denoise(*new)
    torch.cuda.synchronize()
    assert pe.fast_operands()[0] == "fp16"
    assert torch.isfinite(eager).all() and torch.equal(eager, replayed)


# ------------------------------------------------------------------------------------------------ 7: unchanged shapes
@pytest.mark.parametrize("act", [1, 4])
@pytest.mark.parametrize("axis,F,J", [(1, 243, 17), (0, 27, 17)])
def test_attention_on_served_shapes_ignores_the_switch(lib, monkeypatch, act, axis, F, J):
    n_bh = 2
    qkv = random_qkv(F * 7 + C_ + axis, n_bh * F * J)
    monkeypatch.delenv("D3DP_LONG_ATTN", raising=False)
    out = op_attention(lib, act, 1, axis, qkv, n_bh, F, J)
    monkeypatch.setenv("D3DP_LONG_ATTN", "rows")
    out_rows = op_attention(lib, act, 1, axis, qkv, n_bh, F, J)
    assert torch.isfinite(out.float()).all() and torch.equal(out, out_rows)


def test_fast_sampler_at_27_frames_ignores_the_switch(monkeypatch):
    frames, cs, dep, B, H, K = 27, C_, 2, 2, 2, 2
    sd = make_state_dict(57, cs, dep, frames)
    x2d = synthetic_inputs_2d(58, B, frames)
    noises = [torch.from_numpy(synthetic_noise(59 + k, (B, H, frames, 17, 3))).cuda() for k in range(K)]
    outs = []
    for switch in ("default", "rows"):
        _set_switch(monkeypatch, switch)
        outs.append(sample(sampler_model(sd, frames, cs, dep, H, K, "fast"), x2d, noises))
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
