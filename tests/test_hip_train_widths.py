"""The opt-in split-fp16 training route at `-cs` 192 / 320 / 384 / 448 (D3DP_TRAIN_IMPL=f16x2; run with ``-m gpu`` on an MI355X).

With the model's 8 heads these widths are head dims 24 / 40 / 48 / 56: the attention of both axes runs the padded forms of the
head dim 32 / 64 kernels of train_attn.hip (the head padded inside the LDS images), every Linear the split-fp16 products of
X2Train on operands whose absmax the run-time-width row kernels of train_g.hip leave behind.  Without the switch these widths
train on the fp32 path (tests/test_hip_widths.py, Case(96, ...) of tests/test_hip_train_grads.py pin it).

Gradients are checked as tests/test_hip_train_grads.py checks them: every parameter gradient and the prediction within 8 x e32 of
the oracle's fp64 autograd, in the norm and per element (oracle/grad_check.py; tests/test_train_widths_host.py shows on a CPU
that every case below is admissible).  J = 17, dep = 2 unless said otherwise, one model -- one context -- per case, the smallest
shapes that reach each dispatch case:
  F = 9              17 joints and 9 frames are <= 32 tokens: tattn_bwd_small_kernel on both axes, at each of the four head dims;
  F = 40 / 81 / 243  the whole-sequence kernels (4 / 8 / 16 key tiles; 243: two groups of eight waves, ragged last tiles; at the
                     head dims padded to 64, 33 .. 64 tokens run the 8-tile instantiation, so F = 40 is 4 tiles at cs = 192 only);
  F = 300            the chunked forms of all three kernels -- a clip length these widths refuse without the switch;
  cs = 384           fc1's weight gradient is a TN product (768 x 384), the other three run on transposed operands; at the other
                     widths all four do.
The case tables are plain data (no GPU needed to import them): the host test walks them too."""
import pytest
import torch

from d3dp_amd import _lib
from test_hip_train_grads import DROPPED_PARAMS, EDITS, UPSTREAM_K, Case, check, model_of, problem, step

pytestmark = pytest.mark.gpu
SWITCH = ("D3DP_TRAIN_IMPL", "f16x2")
_SWITCHES = ("D3DP_TRAIN_ATTN", "D3DP_TRAIN_ATTN_BWD", "D3DP_TRAIN_IMPL", "D3DP_TRAIN_WGRAD", "D3DP_EXACT_IMPL")
WIDTHS = (192, 320, 384, 448)

SHAPES = [
    Case(192, 9, 2), Case(192, 40, 2), Case(192, 243, 1), Case(192, 300, 1),
    Case(320, 9, 2), Case(320, 81, 2), Case(320, 300, 1),
    Case(384, 9, 1), Case(384, 9, 2), Case(384, 243, 1), Case(384, 300, 1),
    Case(384, 9, 2, dep=8),    # the reduce, zero and weight-prep tables fill with depth
    Case(448, 9, 2), Case(448, 40, 2), Case(448, 243, 1),
]
DROPPED = [Case(384, 27, 2, masks="dropped"), Case(192, 27, 2, masks="dropped")]
# (tte0-norm2-x300 at cs = 384 is 2.03e-6 in the norm by the reference alone, over the admissibility cap: it runs at 320 and 448)
MAGNITUDES = ([Case(192, 27, 2, edit=e) for e in EDITS] + [Case(384, 27, 2, edit=e) for e in EDITS if e != "tte0-norm2-x300"]
              + [Case(320, 27, 2, edit="tte0-norm2-x300"), Case(448, 27, 2, edit="tte0-norm2-x300")])
UPSTREAM = [Case(384, 9, 2), Case(192, 40, 2)]
ALL_CASES = list(dict.fromkeys(SHAPES + DROPPED + MAGNITUDES + UPSTREAM))


def route(monkeypatch, on=True, attn=None):
    """The environment of one context: every training switch cleared, then the opt-in route (and a cross-check switch beside it)."""
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if on:
        monkeypatch.setenv(*SWITCH)
    if attn:
        monkeypatch.setenv("D3DP_TRAIN_ATTN", attn)


def gpu_step(monkeypatch, case, ks=(0,), on=True, attn=None):
    route(monkeypatch, on, attn)
    sd, x2d, gt, t, noise, dpd = problem(case)
    m = model_of(case, sd)
    x2d, gt = x2d.cuda(), gt.cuda()
    return [step(m, x2d, gt, t, noise, dpd, k) for k in ks]


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: c.id)
def test_gradients_elementwise_over_the_dispatch_shapes(monkeypatch, case):
    (grads, pred), = gpu_step(monkeypatch, case)
    check(case, grads, pred)


@pytest.mark.parametrize("case", MAGNITUDES, ids=lambda c: c.id)
def test_gradients_elementwise_when_one_operand_leaves_its_usual_magnitude(monkeypatch, case):
    (grads, pred), = gpu_step(monkeypatch, case)
    check(case, grads, pred)


@pytest.mark.parametrize("case", DROPPED, ids=lambda c: c.id)
def test_a_branch_dropped_for_every_sample_has_exactly_zero_gradients(monkeypatch, case):
    (grads, pred), = gpu_step(monkeypatch, case)
    errs = check(case, grads, pred)
    assert sorted(n for n, e in errs.items() if e.zero_ref) == sorted(DROPPED_PARAMS)
    for n in DROPPED_PARAMS:
        assert torch.equal(grads[n], torch.zeros_like(grads[n])), n
    assert all(torch.isfinite(g).all() for g in grads.values())


@pytest.mark.parametrize("case", UPSTREAM, ids=lambda c: c.id)
def test_gradients_scale_with_the_upstream_gradient_bit_for_bit(monkeypatch, case):
    """loss.backward(loss * 2^k), k = -40, 0, +30: each run within the bound of the fp64 gradients x 2^k, the k != 0 gradients x 2^-k
    equal to the k = 0 ones bit for bit (every device-side scale is a power of two derived from an absmax -- the ones the row
    kernels of train_g.hip now leave included)."""
    runs = dict(zip(UPSTREAM_K, gpu_step(monkeypatch, case, UPSTREAM_K)))
    for k, (grads, pred) in runs.items():
        check(case, grads, pred, tag=f" upstream x 2^{k}", k=k)
    base = runs[0][0]
    for k in UPSTREAM_K:
        if k == 0:
            continue
        differ = [n for n, g in runs[k][0].items() if not torch.equal(g * 2.0 ** -k, base[n])]
        assert not differ, (k, differ)


@pytest.mark.parametrize("cs", WIDTHS)
def test_padded_attention_matches_the_fp32_attention_under_the_same_linears(monkeypatch, cs):
    """The switch alone against D3DP_TRAIN_ATTN=f32 beside it (split Linears around the fp32 attention with a run-time head dim, as
    cs = 64 runs): every gradient within 2e-5 relative, the prediction within 2e-5 absolute -- the figures of
    tests/test_hip_train_heads.py -- and some gradient bit differs (the switch selected other kernels)."""
    case = Case(cs, 40, 2)
    (g_x2, p_x2), = gpu_step(monkeypatch, case)
    (g_f32, p_f32), = gpu_step(monkeypatch, case, attn="f32")
    assert all(torch.isfinite(g).all() for g in g_x2.values()) and all(torch.isfinite(g).all() for g in g_f32.values())
    errs = {k: (g_f32[k].double() - g_x2[k].double()).norm().item() / max(g_f32[k].double().norm().item(), 1e-30) for k in g_f32}
    dp = (p_x2.double() - p_f32.double()).abs().max().item()
    worst = max(errs, key=errs.get)
    print(f"cs={cs} F=40: padded split-fp16 attention vs fp32 attention, worst relative gradient difference {errs[worst]:.2e} "
          f"({worst}), prediction max |diff| {dp:.2e}")
    for k, e in errs.items():
        assert e < 2e-5, (k, e)
    assert dp < 2e-5, dp
    assert any(not torch.equal(g_f32[k], g_x2[k]) for k in g_f32)


def profiled_step(monkeypatch, on):
    route(monkeypatch, on)
    case = Case(384, 40, 2)
    sd, x2d, gt, t, noise, _ = problem(case)
    m = model_of(case, sd)
    pe = m.pose_estimator
    pe._context(torch.device("cuda", torch.cuda.current_device()))
    pe.profile_enable(True)
    step(m, x2d.cuda(), gt.cuda(), t, noise, {})
    prof = pe.profile_read()
    pe.profile_enable(False)
    return prof, pe.train_arithmetic()


def test_the_route_is_observable_in_the_profile(monkeypatch):
    """Pass KV is a profile class of its own on the split-fp16 attention only (the fp32 path times both passes under pass Q)."""
    on, text_on = profiled_step(monkeypatch, True)
    off, text_off = profiled_step(monkeypatch, False)
    for axis in ("temporal", "spatial"):
        assert on[f"train_attn_bwd_kv_{axis}"][0] > 0 and on[f"train_attn_bwd_q_{axis}"][0] > 0, on
        assert off[f"train_attn_bwd_kv_{axis}"][0] == 0, off
    assert "D3DP_TRAIN_IMPL=f16x2" in text_on and "fp32 path" in text_off, (text_on, text_off)


def test_a_clip_longer_than_256_frames_trains_with_the_switch_and_is_refused_without(monkeypatch):
    case = Case(384, 300, 1)
    (grads, pred), = gpu_step(monkeypatch, case)
    assert torch.isfinite(pred).all() and all(torch.isfinite(g).all() for g in grads.values())
    assert any(g.abs().max() > 0 for g in grads.values())
    with pytest.raises(_lib.D3DPHipError) as e:
        gpu_step(monkeypatch, case, on=False)
    assert "holds a whole sequence in LDS" in str(e.value), str(e.value)
    with pytest.raises(_lib.D3DPHipError) as e:              # (the cross-check switch beside it keeps the fp32 attention's limit)
        gpu_step(monkeypatch, case, attn="f32")
    assert "frames=300 > 256" in str(e.value) and "D3DP_TRAIN_ATTN=f32" in str(e.value), str(e.value)


def test_the_step_is_bit_reproducible(monkeypatch):
    route(monkeypatch)
    case = Case(320, 81, 2)
    sd, x2d, gt, t, noise, dpd = problem(case)
    m = model_of(case, sd)
    x2d, gt = x2d.cuda(), gt.cuda()
    (g0, p0), (g1, p1) = step(m, x2d, gt, t, noise, dpd), step(m, x2d, gt, t, noise, dpd)
    assert torch.equal(p0, p1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    assert all(torch.isfinite(g).all() for g in g0.values()) and any(g.abs().max() > 0 for g in g0.values())


def test_the_step_on_a_side_stream(monkeypatch):
    """Stream contract: one step issued under torch.cuda.stream(s), after one eager step, gives the default-stream gradients bit for
    bit (the form of tests/test_hip_train_heads.py)."""
    route(monkeypatch)
    case = Case(448, 27, 2)
    sd, x2d, gt, t, noise, _ = problem(case)
    m = model_of(case, sd)
    x2d, gt = x2d.cuda(), gt.cuda()
    want, _ = step(m, x2d, gt, t, noise, {})
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got, _ = step(m, x2d, gt, t, noise, {})
    s.synchronize()
    for n in want:
        assert torch.equal(want[n], got[n]), n
    assert any(g.abs().max() > 0 for g in want.values())


def test_the_step_runs_in_exactly_the_workspace_its_size_query_returns(monkeypatch):
    """One forward + backward at cs = 384 between guard bytes, as tests/test_hip_workspace.py::test_train_workspace: the layout does
    not depend on the route, so the size query is the one of the fp32 path."""
    from test_hip_workspace import ESTATE, Guarded, ab
    B, F, J = 2, 9, 17
    route(monkeypatch, on=False)
    n_f32 = ab.RawCtx("train", 384, F, J, 1).train_bytes(B)
    route(monkeypatch)
    c = ab.RawCtx("train", 384, F, J, 1)
    n = c.train_bytes(B)
    assert n == n_f32
    inputs = c.train_inputs(B)
    res = []
    for ws in (Guarded(n), Guarded(2 * n)):
        out, grads = torch.empty(B, F, J, 3, device="cuda"), c.grad_buffers()
        assert c.train_forward(inputs, out, B, ws.ptr, ws.n) == 0, c.lib.d3dp_last_error()
        assert c.train_backward(inputs, grads, B, ws.ptr, ws.n) == 0, c.lib.d3dp_last_error()
        assert ws.intact()
        res.append((out, c.flat_grads(grads)))
    (out, grads), (ref, ref_grads) = res
    assert torch.isfinite(out).all() and torch.equal(out, ref)
    for i, (g, r) in enumerate(zip(grads, ref_grads)):
        assert torch.isfinite(g).all() and torch.equal(g, r), f"gradient {i}"
    tight = Guarded(n)
    kept = torch.full_like(out, 7.0)
    assert c.train_forward(inputs, kept, B, tight.ptr, n - 256) == ESTATE
    assert tight.intact() and bool((kept == 7.0).all())
