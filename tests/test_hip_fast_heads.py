"""GPU tests of FAST / FAST16 attention on the matrix cores at head dims 32 and 16 (cs = 256 and 128 with the model's 8 heads):
the three kernels of attention_fast.hip with their head dim a template parameter -- one 16x16x32 MFMA per key tile for S^T at
head dim 32, one 16-deep MFMA at 16, HD / 16 output-channel tiles, K / V images of 64- and 32-byte rows.

  1. the spatial kernel (<= 32 joints, one wave per problem);
  2. the whole-sequence kernel (<= 256 frames), one shape per key-tile-count instantiation;
  3. the chunked-key kernel (257 .. 1024 frames) and its rescaling on a sharp row;
  4. more than 32 joints: the whole-sequence launcher with the spatial map;
  5. no lane reads a neighbouring head's columns: a NaN head stays alone;
  6. bit-equal run to run;
  7. head dims 8 and 48 are still refused, by name;
  8. the contexts take the new kernels, and D3DP_LONG_ATTN=rows takes the row kernel back; cs = 64 does not move;
  9. the stream contract at one new shape: side stream, capture and replay.

Operator references: fp64 softmax attention on operands rounded to the 2-byte type (test_hip_parity.ref_attention) at the
tolerances of test_hip_fast_long.TYPES; end to end: oracle.d3dp_oracle in fp32 at FAST_TOL_MM.  The helpers are those of
test_hip_fast_long.py with the width a parameter.
"""
import pytest
import torch

from d3dp_amd import _lib
from d3dp_amd.weights import make_state_dict, synthetic_inputs_2d, synthetic_noise
from oracle import d3dp_oracle as orc
from test_hip_fast16 import oracle_sample, sample, sampler_model
from test_hip_fast_long import TYPES, _set_switch
from test_hip_parity import FAST_TOL_MM, ref_attention

pytestmark = pytest.mark.gpu
HEADS = 8
WIDTHS = [256, 128]          # head dims 32 and 16
D3DP_ENOTSUP = -2


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def launch_attention(lib, act, impl, axis, qd, out, n_bh, F, J, C):
    return lib.d3dp_op_attention(act, impl, axis, qd.data_ptr(), out.data_ptr(), n_bh, F, J, C, HEADS, _lib.current_stream())


def op_attention(lib, act, impl, axis, qkv, n_bh, F, J, C):
    """d3dp_op_attention on `qkv` (fp32, CPU) rounded to the type of `act`, into a NaN-filled output: the 2-byte device result."""
    qd = qkv.to(TYPES[act][0]).cuda().contiguous()
    out = torch.full((n_bh * F * J, C), float("nan"), dtype=qd.dtype, device="cuda")
    _lib.check(launch_attention(lib, act, impl, axis, qd, out, n_bh, F, J, C))
    torch.cuda.synchronize()
    return out


def reference(qkv, act, n_bh, F, J, C, axis):
    return ref_attention(qkv.to(TYPES[act][0]).to(torch.float32), n_bh, F, J, C, HEADS, axis)


def check_against_reference(tag, out, qkv, act, n_bh, F, J, C, axis, spike=False):
    _, atol, rtol, s_atol, s_rtol = TYPES[act]
    want = reference(qkv, act, n_bh, F, J, C, axis)
    got = out.float().cpu().double()
    print(f"{tag}: max |err| vs fp64 {(got - want).abs().max().item():.2e}")
    assert torch.isfinite(got).all()
    assert torch.allclose(got, want, atol=s_atol if spike else atol, rtol=s_rtol if spike else rtol), (got - want).abs().max().item()


def random_qkv(seed, rows, C):
    qkv = torch.randn(rows, 3 * C, generator=torch.Generator().manual_seed(seed))
    qkv[:, :C] *= 2.0        # sharpen the softmax a little
    return qkv


# ------------------------------------------------------------------------------------------------ 1: spatial kernel
@pytest.mark.parametrize("act", [1, 4])
@pytest.mark.parametrize("J", [1, 16, 17, 32])
@pytest.mark.parametrize("C", WIDTHS)
def test_spatial_kernel(lib, C, J, act):
    """One key, exactly one key tile, a partial second tile, two full tiles."""
    n_bh, F = 2, 3
    qkv = random_qkv(J * 7 + C, n_bh * F * J, C)
    out = op_attention(lib, act, 1, 0, qkv, n_bh, F, J, C)
    check_against_reference(f"attention C={C} act={act} impl=1 axis=0 J={J}", out, qkv, act, n_bh, F, J, C, 0)


# ------------------------------------------------------------------------------------------------ 2: whole-sequence kernel
@pytest.mark.parametrize("act", [1, 4])
@pytest.mark.parametrize("F,J", [(9, 3), (33, 3), (100, 3), (243, 3), (256, 3), (27, 17)])
@pytest.mark.parametrize("C", WIDTHS)
def test_whole_sequence_kernel(lib, C, F, J, act):
    """2, 4, 8 and 16 key tiles (9, 33, 100, 243 frames), the full image (256), and the workload's token stride (17 joints)."""
    n_bh = 2
    qkv = random_qkv(F * 7 + C + J, n_bh * F * J, C)
    out = op_attention(lib, act, 1, 1, qkv, n_bh, F, J, C)
    check_against_reference(f"attention C={C} act={act} impl=1 axis=1 F={F} J={J}", out, qkv, act, n_bh, F, J, C, 1)


# ------------------------------------------------------------------------------------------------ 3: chunked-key kernel
@pytest.mark.parametrize("act", [1, 4])
@pytest.mark.parametrize("F", [257, 351, 513])
@pytest.mark.parametrize("C", WIDTHS)
def test_chunked_key_kernel(lib, C, F, act):
    """The last chunk ends one key in (257), inside a key tile (351); three chunks (513)."""
    n_bh, J = 1, 3
    qkv = random_qkv(F * 7 + C + 1, n_bh * F * J, C)
    out = op_attention(lib, act, 1, 1, qkv, n_bh, F, J, C)
    check_against_reference(f"attention C={C} act={act} impl=1 axis=1 F={F}", out, qkv, act, n_bh, F, J, C, 1)


@pytest.mark.parametrize("act", [1, 4])
def test_chunked_key_kernel_softmax_spike_in_the_last_chunk(lib, act):
    """test_attention_softmax_spike_across_chunks' construction at C = 256: query row (frame 100, joint 3) x 30, its matching key
    at frame 340 -- the maximum jumps in the last chunk and everything accumulated before is rescaled, under the HD^-0.5 scale of
    head dim 32."""
    n_bh, F, J, C = 1, 351, 17, 256
    qkv = torch.randn(n_bh * F * J, 3 * C, generator=torch.Generator().manual_seed(5))
    qkv[100 * J + 3, :C] *= 30.0
    qkv[340 * J + 3, C:2 * C] = qkv[100 * J + 3, :C] / 30.0 * 4.0
    out = op_attention(lib, act, 1, 1, qkv, n_bh, F, J, C)
    check_against_reference(f"attention spike C={C} act={act} key at frame 340", out, qkv, act, n_bh, F, J, C, 1, spike=True)


# ------------------------------------------------------------------------------------------------ 4: more than 32 joints
@pytest.mark.parametrize("act", [1, 4])
@pytest.mark.parametrize("J", [33, 72])
@pytest.mark.parametrize("C", WIDTHS)
def test_more_than_32_joints(lib, C, J, act):
    n_bh, F = 2, 3
    qkv = random_qkv(J * 7 + C, n_bh * F * J, C)
    out = op_attention(lib, act, 1, 0, qkv, n_bh, F, J, C)
    check_against_reference(f"attention C={C} act={act} impl=1 axis=0 J={J}", out, qkv, act, n_bh, F, J, C, 0)


# ------------------------------------------------------------------------------------------------ 5: heads stay apart
@pytest.mark.parametrize("act", [1, 4])
@pytest.mark.parametrize("axis,F,J", [(1, 27, 3), (0, 3, 17)])
@pytest.mark.parametrize("C", WIDTHS)
def test_heads_do_not_see_each_other(lib, C, axis, F, J, act):
    """Head 0's q, k and v columns are NaN in every row.  Head 7's q columns border head 0's k columns in the qkv row, head 1's
    border head 0's own: a fragment load or a k-depth that reached past its head would carry the NaN over."""
    n_bh, hd = 2, C // HEADS
    qkv = random_qkv(F * 7 + C + axis, n_bh * F * J, C)
    for section in range(3):
        qkv[:, section * C:section * C + hd] = float("nan")
    out = op_attention(lib, act, 1, axis, qkv, n_bh, F, J, C).float().cpu().double()
    want = reference(qkv, act, n_bh, F, J, C, axis)
    _, atol, rtol, _, _ = TYPES[act]
    assert not torch.isfinite(out[:, :hd]).any() and not torch.isfinite(want[:, :hd]).any()
    assert torch.isfinite(out[:, hd:]).all()
    print(f"NaN head C={C} act={act} axis={axis}: heads 1..7 max |err| vs fp64 {(out[:, hd:] - want[:, hd:]).abs().max().item():.2e}")
    assert torch.allclose(out[:, hd:], want[:, hd:], atol=atol, rtol=rtol)


# ------------------------------------------------------------------------------------------------ 6: run to run
@pytest.mark.parametrize("act", [1, 4])
@pytest.mark.parametrize("axis,F,J", [(1, 100, 17), (0, 27, 17)])
@pytest.mark.parametrize("C", WIDTHS)
def test_bit_equal_run_to_run(lib, C, axis, F, J, act):
    n_bh = 2
    qkv = random_qkv(F + C + axis, n_bh * F * J, C)
    first = op_attention(lib, act, 1, axis, qkv, n_bh, F, J, C)
    assert torch.isfinite(first.float()).all() and torch.equal(first, op_attention(lib, act, 1, axis, qkv, n_bh, F, J, C))


# ------------------------------------------------------------------------------------------------ 7: refusals kept
@pytest.mark.parametrize("act", [1, 4])
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("C,hd", [(64, 8), (384, 48)])
def test_other_head_dims_are_refused_by_name(lib, C, hd, axis, act):
    n_bh, F, J = 1, 9, 5
    qd = random_qkv(C, n_bh * F * J, C).to(TYPES[act][0]).cuda()
    out = torch.zeros(n_bh * F * J, C, dtype=qd.dtype, device="cuda")
    assert launch_attention(lib, act, 1, axis, qd, out, n_bh, F, J, C) == D3DP_ENOTSUP
    msg = lib.d3dp_last_error().decode()
    assert f"head dim {hd}" in msg, msg
    torch.cuda.synchronize()
    assert not out.any()                                    # (nothing ran)


# ------------------------------------------------------------------------------------------------ 8: what the contexts launch
def _sampler_runs(monkeypatch, cs):
    """The sampler of test_sampler_at_the_reference_small_width (F = 27, dep 2, B 2, H 2, K 2, its seeds) in both modes, with and
    without D3DP_LONG_ATTN=rows (read when the model's first call creates its context).  -> outputs, operand types, oracle."""
    frames, dep, B, H, K = 27, 2, 2, 2, 2
    sd = make_state_dict(29, cs, dep, frames)
    x2d = synthetic_inputs_2d(291, B, frames)
    noises = [torch.from_numpy(synthetic_noise(292 + k, (B, H, frames, 17, 3))) for k in range(K)]
    runs, operands = {}, {}
    for switch in ("default", "rows"):
        _set_switch(monkeypatch, switch)
        for numerics in ("fast", "fast16"):
            m = sampler_model(sd, frames, cs, dep, H, K, numerics)
            runs[(numerics, switch)] = sample(m, x2d, noises)
            operands[(numerics, switch)] = m.pose_estimator.fast_operands()[0]
    for v in runs.values():
        assert torch.isfinite(v).all()
    return runs, operands, oracle_sample(orc.strip_prefix(sd), x2d, noises, H, K, dep)


@pytest.mark.parametrize("cs", WIDTHS)
def test_fast_contexts_run_the_matrix_core_kernels_at_small_widths(monkeypatch, cs):
    """Both axes of a cs = 256 / 128 context are on the matrix cores (spatial kernel: 17 joints; whole-sequence kernel: 27 frames);
    D3DP_LONG_ATTN=rows puts both back on the fp32 row kernel, so the two settings of a mode differ in some bit.  Every run within
    FAST_TOL_MM of the fp32 oracle, fast16 (on fp16 operands) closer than fast under either setting."""
    runs, operands, want = _sampler_runs(monkeypatch, cs)
    errs = {k: orc.mpjpe_mm(v.cpu(), want) for k, v in runs.items()}
    print(f"cs={cs} sampler vs the fp32 oracle: " + ", ".join(f"{n}{'' if s == 'default' else ':rows'} {e:.4f} mm" for (n, s), e in errs.items()))
    assert all(operands[(n, s)] == ("fp16" if n == "fast16" else "bf16") for n, s in operands), operands
    assert all(e <= FAST_TOL_MM for e in errs.values()), errs
    for switch in ("default", "rows"):
        assert errs[("fast16", switch)] < errs[("fast", switch)], errs
    for numerics in ("fast", "fast16"):
        assert not torch.equal(runs[(numerics, "default")], runs[(numerics, "rows")]), numerics


def test_fast_contexts_at_head_dim_8_ignore_the_switch(monkeypatch):
    """cs = 64: the row kernel either way -- that route did not move."""
    runs, _, _ = _sampler_runs(monkeypatch, 64)
    for numerics in ("fast", "fast16"):
        assert torch.equal(runs[(numerics, "default")], runs[(numerics, "rows")]), numerics


# ------------------------------------------------------------------------------------------------ 9: the stream contract
def _stream_case(seed):
    n_bh, F, J, C, act = 2, 100, 3, 256, 4
    qd = random_qkv(seed, n_bh * F * J, C).to(TYPES[act][0]).cuda()
    return (act, 1, 1), (n_bh, F, J, C), qd


def test_operator_on_a_side_stream_equals_the_default_stream(lib):
    how, shape, qd = _stream_case(91)
    ref, got = torch.empty(qd.shape[0], shape[3], dtype=qd.dtype, device="cuda"), torch.empty(qd.shape[0], shape[3], dtype=qd.dtype, device="cuda")
    _lib.check(launch_attention(lib, *how, qd, ref, *shape))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _lib.check(launch_attention(lib, *how, qd, got, *shape))
    s.synchronize()
    assert torch.isfinite(ref.float()).all() and torch.equal(ref, got)


def test_operator_is_capturable(lib):
    """One eager call, then the same call captured into a graph: the replay on new inputs computes the eager call's bits."""
    how, shape, qd = _stream_case(92)
    out = torch.empty(qd.shape[0], shape[3], dtype=qd.dtype, device="cuda")
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
    assert torch.isfinite(eager.float()).all() and torch.equal(eager, replayed)
