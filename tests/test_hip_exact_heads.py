"""GPU tests of EXACT attention on the matrix cores at head dims 32 and 16 (cs = 256 and 128 with the model's 8 heads): the three
split-fp16 kernels of attention_x2.hip with their head dim a template parameter -- one 16x16x32 MFMA per pass and key tile for
S^T at head dim 32, one 16-deep MFMA at 16, HD / 16 output-channel tiles, K / V images of 64- and 32-byte rows per plane.

Operator level (d3dp_op_attention, act 0, impl 2, against the fp64 reference of test_hip_parity at test_attention's fp32-class
bounds: atol 2e-5, rtol 1e-4, mean |err| < 5e-7; the row kernel's -- impl 0 -- mean error on the same rows printed beside):
  1. the spatial kernel (<= 32 joints, one wave per problem);
  2. the whole-sequence kernel (<= 256 frames): every key-tile count, masked whole tiles, a key count ending inside the last
     tile, nothing masked, the workload's token stride;
  3. more problems than resident workgroups (the persistent loop);
  4. the chunked-key kernel (257 .. 1024 frames) and its rescaling on a sharp row;
  5. more than 32 joints: the whole-sequence launcher with the spatial map;
  6. no lane reads a neighbouring head's columns: a NaN head stays alone;
  7. a sequence's result does not depend on what else is in the batch, bit for bit;
  8. head dims 8 and 48 are refused by name before anything is launched.
Context level (D3DP(numerics="exact") against oracle.d3dp_oracle at EXACT_TOL_MM):
  9. the sampler at cs 256 / 128 takes the new kernels, D3DP_LONG_ATTN=rows takes the row kernel back; cs = 64 does not move;
 10. the plane-output form (act 3) of the 16-key-tile instantiation and of the chunked-key kernel;
 11. a q/k/v bound beyond the split-fp16 range lowers that block's scale and stays on f16x2 (bf16x3 under the switch);
 12. the stream contract at one new shape: side stream, capture and replay.
"""
import pytest
import torch

from d3dp_amd import _lib
from d3dp_amd.weights import make_state_dict, synthetic_inputs_2d, synthetic_noise
from oracle import d3dp_oracle as orc
from test_hip_fast16 import oracle_sample, sample, sampler_model
from test_hip_fast_long import _set_switch
from test_hip_parity import EXACT_TOL_MM, ref_attention

pytestmark = pytest.mark.gpu
HEADS = 8
WIDTHS = [256, 128]          # head dims 32 and 16
D3DP_ENOTSUP = -2
ATOL, RTOL, MEAN = 2e-5, 1e-4, 5e-7          # test_hip_parity.test_attention, fp32 rows
SPIKE_ATOL, SPIKE_RTOL = 5e-5, 1e-4          # test_hip_parity.test_attention_softmax_spike


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def launch_attention(lib, impl, axis, qd, out, n_bh, F, J, C):
    return lib.d3dp_op_attention(0, impl, axis, qd.data_ptr(), out.data_ptr(), n_bh, F, J, C, HEADS, _lib.current_stream())


def op_attention(lib, impl, axis, qkv, n_bh, F, J, C):
    """d3dp_op_attention on fp32 rows `qkv` (CPU) into a NaN-filled output."""
    qd = qkv.cuda().contiguous()
    out = torch.full((n_bh * F * J, C), float("nan"), device="cuda")
    _lib.check(launch_attention(lib, impl, axis, qd, out, n_bh, F, J, C))
    torch.cuda.synchronize()
    return out


def check_against_reference(lib, tag, qkv, n_bh, F, J, C, axis, atol=ATOL, rtol=RTOL):
    want = ref_attention(qkv, n_bh, F, J, C, HEADS, axis)
    got = op_attention(lib, 2, axis, qkv, n_bh, F, J, C).cpu().double()
    rows = op_attention(lib, 0, axis, qkv, n_bh, F, J, C).cpu().double()
    err, err0 = (got - want).abs().mean().item(), (rows - want).abs().mean().item()
    print(f"{tag}: impl 2 mean |err| vs fp64 {err:.2e}, max {(got - want).abs().max().item():.2e}; impl 0 (row kernel) mean {err0:.2e}")
    assert torch.isfinite(got).all()
    assert torch.allclose(got, want, atol=atol, rtol=rtol), (got - want).abs().max().item()
    assert err < MEAN, err


def random_qkv(seed, rows, C):
    qkv = torch.randn(rows, 3 * C, generator=torch.Generator().manual_seed(seed))
    qkv[:, :C] *= 2.0        # sharpen the softmax a little
    return qkv


# ------------------------------------------------------------------------------------------------ 1: spatial kernel
@pytest.mark.parametrize("J", [1, 16, 17, 32])
@pytest.mark.parametrize("C", WIDTHS)
def test_spatial_kernel(lib, C, J):
    """One key, exactly one key tile, a partial second tile, two full tiles."""
    n_bh, F = 2, 3
    qkv = random_qkv(J * 7 + C, n_bh * F * J, C)
    check_against_reference(lib, f"attention C={C} impl=2 axis=0 J={J}", qkv, n_bh, F, J, C, 0)


# ------------------------------------------------------------------------------------------------ 2: whole-sequence kernel
@pytest.mark.parametrize("F,J", [(9, 3), (33, 3), (49, 3), (100, 3), (130, 3), (243, 3), (256, 3), (27, 17)])
@pytest.mark.parametrize("C", WIDTHS)
def test_whole_sequence_kernel(lib, C, F, J):
    """2, 4, 8 and 16 key tiles; whole tiles masked (9, 33, 130), keys ending inside the last tile (49, 100, 243, 27), nothing
    masked (256); the workload's token stride (17 joints)."""
    n_bh = 2
    qkv = random_qkv(F * 7 + C + J, n_bh * F * J, C)
    check_against_reference(lib, f"attention C={C} impl=2 axis=1 F={F} J={J}", qkv, n_bh, F, J, C, 1)


# ------------------------------------------------------------------------------------------------ 3: persistence
@pytest.mark.parametrize("C", WIDTHS)
def test_many_problems_per_workgroup(lib, C):
    """test_attention_split_f16_many_problems_per_workgroup's shape: 3264 (sequence, head) problems, more than the resident
    workgroups at any occupancy (at most 4 per CU), so every workgroup loops with K(p+1) / V(p+1) streaming into the images."""
    n_bh, F, J = 24, 27, 17
    qkv = torch.randn(n_bh * F * J, 3 * C, generator=torch.Generator().manual_seed(99))
    check_against_reference(lib, f"attention C={C} impl=2 axis=1 n_bh=24", qkv, n_bh, F, J, C, 1)


# ------------------------------------------------------------------------------------------------ 4: chunked-key kernel
@pytest.mark.parametrize("F", [257, 288, 351, 384, 513])
@pytest.mark.parametrize("C", WIDTHS)
def test_chunked_key_kernel(lib, C, F):
    """The last chunk ends one key in (257), on a pair boundary (288), inside a key tile (351), on a chunk boundary (384); five
    chunks (513)."""
    n_bh, J = 1, 3
    qkv = random_qkv(F * 7 + C + 1, n_bh * F * J, C)
    check_against_reference(lib, f"attention C={C} impl=2 axis=1 F={F}", qkv, n_bh, F, J, C, 1)


def test_chunked_key_kernel_softmax_spike_in_the_last_chunk(lib):
    """test_hip_fast_heads' construction at C = 256: query row (frame 100, joint 3) x 30, its matching key at frame 340 -- the
    maximum jumps in the last chunk and everything accumulated before is rescaled, under the HD^-0.5 scale of head dim 32."""
    n_bh, F, J, C = 1, 351, 17, 256
    qkv = torch.randn(n_bh * F * J, 3 * C, generator=torch.Generator().manual_seed(5))
    qkv[100 * J + 3, :C] *= 30.0
    qkv[340 * J + 3, C:2 * C] = qkv[100 * J + 3, :C] / 30.0 * 4.0
    check_against_reference(lib, f"attention spike C={C} impl=2 key at frame 340", qkv, n_bh, F, J, C, 1, SPIKE_ATOL, SPIKE_RTOL)


# ------------------------------------------------------------------------------------------------ 5: more than 32 joints
@pytest.mark.parametrize("J", [33, 72])
@pytest.mark.parametrize("C", WIDTHS)
def test_more_than_32_joints(lib, C, J):
    n_bh, F = 2, 3
    qkv = random_qkv(J * 7 + C, n_bh * F * J, C)
    check_against_reference(lib, f"attention C={C} impl=2 axis=0 J={J}", qkv, n_bh, F, J, C, 0)


# ------------------------------------------------------------------------------------------------ 6: heads stay apart
@pytest.mark.parametrize("axis,F,J", [(1, 27, 3), (0, 3, 17)])
@pytest.mark.parametrize("C", WIDTHS)
def test_heads_do_not_see_each_other(lib, C, axis, F, J):
    """Head 0's q, k and v columns are NaN in every row.  Head 1's columns border head 0's own in every plane of the packed row, and
    at head dim 16 a 16-byte slot of a plane is half a head: a fragment load, a DMA piece or a k-depth that reached past its head
    would carry the NaN over."""
    n_bh, hd = 2, C // HEADS
    qkv = random_qkv(F * 7 + C + axis, n_bh * F * J, C)
    for section in range(3):
        qkv[:, section * C:section * C + hd] = float("nan")
    out = op_attention(lib, 2, axis, qkv, n_bh, F, J, C).cpu().double()
    want = ref_attention(qkv, n_bh, F, J, C, HEADS, axis)
    assert not torch.isfinite(out[:, :hd]).any() and not torch.isfinite(want[:, :hd]).any()
    assert torch.isfinite(out[:, hd:]).all()
    err = (out[:, hd:] - want[:, hd:]).abs()
    print(f"NaN head C={C} axis={axis}: heads 1..7 mean |err| vs fp64 {err.mean().item():.2e}, max {err.max().item():.2e}")
    assert torch.allclose(out[:, hd:], want[:, hd:], atol=ATOL, rtol=RTOL) and err.mean().item() < MEAN


# ------------------------------------------------------------------------------------------------ 7: batch composition
@pytest.mark.parametrize("axis,F,J", [(1, 100, 17), (0, 27, 17)])
@pytest.mark.parametrize("C", WIDTHS)
def test_bit_equal_alone_and_in_a_batch(lib, C, axis, F, J):
    """One problem is one (sequence, head): the rows of a batch element computed among three are the rows it gets alone."""
    n_bh = 3
    qkv = random_qkv(F + C + axis, n_bh * F * J, C)
    together = op_attention(lib, 2, axis, qkv, n_bh, F, J, C)
    assert torch.isfinite(together).all()
    assert torch.equal(together, op_attention(lib, 2, axis, qkv, n_bh, F, J, C))          # run to run
    for b in range(n_bh):
        rows = slice(b * F * J, (b + 1) * F * J)
        assert torch.equal(together[rows], op_attention(lib, 2, axis, qkv[rows], 1, F, J, C)), b


# ------------------------------------------------------------------------------------------------ 8: refusals
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("C,hd", [(64, 8), (384, 48)])
def test_other_head_dims_are_refused_by_name(lib, C, hd, axis):
    n_bh, F, J = 1, 9, 5
    qd = random_qkv(C, n_bh * F * J, C).cuda()
    out = torch.zeros(n_bh * F * J, C, device="cuda")
    assert launch_attention(lib, 2, axis, qd, out, n_bh, F, J, C) == D3DP_ENOTSUP
    msg = lib.d3dp_last_error().decode()
    assert f"head dim {hd}" in msg, msg
    torch.cuda.synchronize()
    assert not out.any()                                    # (nothing ran)


# ------------------------------------------------------------------------------------------------ 9: what the contexts launch
def _sampler_runs(monkeypatch, cs):
    """The sampler of test_sampler_at_the_reference_small_width (F = 27, dep 2, B 2, H 2, K 2, its seeds) with and without
    D3DP_LONG_ATTN=rows (read when the model's first call creates its context).  -> outputs, implementations, oracle."""
    frames, dep, B, H, K = 27, 2, 2, 2, 2
    sd = make_state_dict(29, cs, dep, frames)
    x2d = synthetic_inputs_2d(291, B, frames)
    noises = [torch.from_numpy(synthetic_noise(292 + k, (B, H, frames, 17, 3))) for k in range(K)]
    runs, impls = {}, {}
    for switch in ("default", "rows"):
        _set_switch(monkeypatch, switch)
        m = sampler_model(sd, frames, cs, dep, H, K, "exact")
        runs[switch] = sample(m, x2d, noises)
        impls[switch] = m.pose_estimator.exact_scales()[2]
    for v in runs.values():
        assert torch.isfinite(v).all()
    return runs, impls, oracle_sample(orc.strip_prefix(sd), x2d, noises, H, K, dep)


@pytest.mark.parametrize("cs", WIDTHS)
def test_exact_contexts_run_the_matrix_core_kernels_at_small_widths(monkeypatch, cs):
    """Both axes of a cs = 256 / 128 context are on the split-fp16 kernels (spatial kernel: 17 joints; whole-sequence kernel: 27
    frames); D3DP_LONG_ATTN=rows puts both back on the fp32 row kernel, so the two settings differ in some bit.  Both within
    EXACT_TOL_MM of the fp32 oracle, both on the split-fp16 Linears."""
    runs, impls, want = _sampler_runs(monkeypatch, cs)
    errs = {k: orc.mpjpe_mm(v.cpu(), want) for k, v in runs.items()}
    print(f"cs={cs} exact sampler vs the fp32 oracle: {errs['default']:.3e} mm, D3DP_LONG_ATTN=rows {errs['rows']:.3e} mm; "
          f"the two apart: {orc.mpjpe_mm(runs['default'].cpu(), runs['rows'].cpu()):.3e} mm")
    assert impls == {"default": "f16x2", "rows": "f16x2"}, impls
    assert all(e <= EXACT_TOL_MM for e in errs.values()), errs
    assert not torch.equal(runs["default"], runs["rows"])


def test_exact_contexts_at_head_dim_8_ignore_the_switch(monkeypatch):
    """cs = 64: the fp32 kernels either way -- that route did not move."""
    runs, impls, _ = _sampler_runs(monkeypatch, 64)
    assert impls == {"default": "f16x2", "rows": "f16x2"}, impls
    assert torch.equal(runs["default"], runs["rows"])


# ------------------------------------------------------------------------------------------------ 10: plane output, large shapes
@pytest.mark.parametrize("cs,frames", [(256, 243), (128, 300)])
def test_plane_output_of_the_large_instantiations(cs, frames):
    """Inside a context the kernels write the proj Linear's operand planes (act 3): the 16-key-tile instantiation at head dim 32
    (243 frames) and the chunked-key kernel at head dim 16 (300 frames), one block pair deep."""
    dep, B, H, K = 1, 1, 1, 1
    sd = make_state_dict(31, cs, dep, frames)
    x2d = synthetic_inputs_2d(311, B, frames)
    noises = [torch.from_numpy(synthetic_noise(312, (B, H, frames, 17, 3)))]
    m = sampler_model(sd, frames, cs, dep, H, K, "exact")
    out = sample(m, x2d, noises)
    err = orc.mpjpe_mm(out.cpu(), oracle_sample(orc.strip_prefix(sd), x2d, noises, H, K, dep))
    print(f"cs={cs} F={frames} exact: MPJPE vs the fp32 oracle {err:.3e} mm")
    assert torch.isfinite(out).all() and m.pose_estimator.exact_scales()[2] == "f16x2"
    assert err <= EXACT_TOL_MM


# ------------------------------------------------------------------------------------------------ 11: the range proof
def test_out_of_range_qkv_lowers_the_scale_and_stays_on_f16x2(monkeypatch):
    """test_exact_mode_operand_range's q/k/v case at cs = 256 (Fr 9, dep 2, B 2, H 2, K 1; its seeds): STE block 1's qkv matrix
    scaled so that the bound the weights prove for q, k, v is twice what 2^4 holds.  The context lowers that block's s_kv and
    keeps the split-fp16 implementation (0.05 mm: the project's bound for this case at cs = 512); where D3DP_LONG_ATTN=rows
    keeps the row kernel, whose plane outputs have no such scale, it moves to bf16x3 as before."""
    Fr, B, H, K, cs, dep = 9, 2, 2, 1, 256, 2
    sd = make_state_dict(7, cs, dep, Fr)
    blk = "pose_estimator.STEblocks.1."
    ln = (cs - 1) ** 0.5 * sd[blk + "norm1.weight"].double().abs() + sd[blk + "norm1.bias"].double().abs()
    w, b = sd[blk + "attn.qkv.weight"].double(), sd[blk + "attn.qkv.bias"].double().abs()
    x2d = synthetic_inputs_2d(5, B, Fr)
    noises = [torch.from_numpy(synthetic_noise(70, (B, H, Fr, 17, 3)))]
    probe = sampler_model(sd, Fr, cs, dep, H, K, "exact")
    split_range = probe.pose_estimator.SPLIT_RANGE
    # bound(f) = max_n f sum_k |W[n, k]| ln_k + |b_n| >= f max_n sum_k |W[n, k]| ln_k: f puts that at twice the range
    factor = 2.0 * split_range / (w.abs() @ ln).max().item()
    sd[blk + "attn.qkv.weight"] = sd[blk + "attn.qkv.weight"] * factor
    assert ((w.abs() * factor) @ ln + b).max().item() >= split_range
    want = oracle_sample(orc.strip_prefix(sd), x2d, noises, H, K, dep)
    _set_switch(monkeypatch, "default")
    m = sampler_model(sd, Fr, cs, dep, H, K, "exact")
    out = sample(m, x2d, noises)
    net = m.pose_estimator
    kv, hd, impl = net.exact_scales()
    bound, e = net.exact_range_bound(), orc.mpjpe_mm(out.cpu(), want)
    print(f"cs={cs} qkv x {factor:.1f}: bound {bound:.4g} (2^4 holds {split_range}), q/k/v scale of that block {kv[1]:g}, {impl}, error {e:.3e} mm")
    assert bound >= split_range and impl == "f16x2"
    assert kv[1] < 16.0 and kv[1] * bound < 65504.0
    assert torch.isfinite(out).all() and not net.nonfinite_seen() and e <= 0.05
    _set_switch(monkeypatch, "rows")
    m = sampler_model(sd, Fr, cs, dep, H, K, "exact")
    out = sample(m, x2d, noises)
    assert m.pose_estimator.exact_scales()[2] == "bf16x3" and torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------------ 12: the stream contract
def _stream_case(seed):
    n_bh, F, J, C = 2, 100, 3, 256
    return (2, 1), (n_bh, F, J, C), random_qkv(seed, n_bh * F * J, C).cuda()


def test_operator_on_a_side_stream_equals_the_default_stream(lib):
    how, shape, qd = _stream_case(91)
    ref, got = torch.empty(qd.shape[0], shape[3], device="cuda"), torch.empty(qd.shape[0], shape[3], device="cuda")
    _lib.check(launch_attention(lib, *how, qd, ref, *shape))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _lib.check(launch_attention(lib, *how, qd, got, *shape))
    s.synchronize()
    assert torch.isfinite(ref).all() and torch.equal(ref, got)


def test_operator_is_capturable(lib):
    """One eager call, then the same call captured into a graph: the replay on new inputs computes the eager call's bits."""
    how, shape, qd = _stream_case(92)
    out = torch.empty(qd.shape[0], shape[3], device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _lib.check(launch_attention(lib, *how, qd, out, *shape))
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        _lib.check(launch_attention(lib, *how, qd, out, *shape))
    qd.copy_(_stream_case(93)[2])
    g.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    eager = torch.empty_like(out)
    _lib.check(launch_attention(lib, *how, qd, eager, *shape))
    torch.cuda.synchronize()
    assert torch.isfinite(eager).all() and torch.equal(eager, replayed)
