"""The opt-in one-pass fp16 training attention (D3DP_TRAIN_ATTN_PASSES=1; run with ``-m gpu`` on an MI355X).

With the switch every product of the attention kernels of the training step -- S = Q K^T and O = P V forward; S, dP = dO V^T,
dQ = dS K, dK = dS^T Q and dV = P^T dO backward, in pass Q, pass KV and the one-kernel spatial backward -- is ONE fp16-MFMA pass on
operands rounded once to fp16 at their device-side scale, from one-plane LDS images (train_attn_1p.hip: the kernels of
train_attn.hip with PASSES = 1).  Every case is a whole training step (J 17, dep 2, recorded DropPath) against the oracle's fp64
autograd, bounded by (lc.NORM16, lc.MAX16) x the error of the CPU emulation of the route in the same case
(tests/train_attn_passes_emu.py; tests/test_train_attn_passes_host.py shows every case admissible) -- and FARTHER than 8 x e32 from
fp64 in the norm, so it cannot be the three-pass route, whose twin in the same test still passes oracle/grad_check.py.

One deliberate defect was checked against this file (a library whose one-pass ta_tr_chunk leaves out the last channel tile):
profiles/train_attn_one_pass.md records how many of these tests fail on it."""
import ctypes as C

import pytest
import torch

import train_attn_passes_emu as emu
from create_host import D3DP_ENOTSUP, create
from d3dp_amd import _lib
from oracle import grad_check as gc
from oracle import lowp_check as lc
from test_hip_train_grads import DROPPED_PARAMS, model_of, problem, step

pytestmark = pytest.mark.gpu
_SWITCHES = ("D3DP_TRAIN_ATTN_PASSES", "D3DP_TRAIN_PASSES", "D3DP_TRAIN_ATTN", "D3DP_TRAIN_ATTN_BWD", "D3DP_TRAIN_IMPL", "D3DP_TRAIN_WGRAD",
             "D3DP_TRAIN_OVERLAP", "D3DP_TRAIN_TAIL", "D3DP_TRAIN_GELU", "D3DP_TRAIN_LN_OPERAND", "D3DP_TRAIN_LONG_ATTN", "D3DP_EXACT_IMPL")


def route(monkeypatch, **switches):
    """switches: without their D3DP_ prefix"""
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in switches.items():
        monkeypatch.setenv("D3DP_" + k, v)


def gpu_steps(monkeypatch, case, ks=(0,), **switches):
    """One step per k (upstream gradient x 2^k) of one model -- one context -- created under the switches: [({name: gradient},
    prediction)], and what the model says about its arithmetic."""
    route(monkeypatch, **switches)
    sd, x2d, gt, t, noise, dpd = problem(case)
    m = model_of(case, sd)
    x2d, gt = x2d.cuda(), gt.cuda()
    return [step(m, x2d, gt, t, noise, dpd, k) for k in ks], m.pose_estimator.train_arithmetic()


def errors(case, grads, pred, k=0):
    ref = emu.base(case)
    assert set(grads) | {gc.PREDICTION} == set(ref.g64), set(grads) ^ set(ref.g64)
    want = {n: (g if n == gc.PREDICTION else g * 2.0 ** k) for n, g in ref.g64.items()}
    return ref, gc.grad_errors({**grads, gc.PREDICTION: pred}, want)


def check_one_pass(case, grads, pred, axes="both", linears=False, k=0):
    """Every tensor within (lc.NORM16, lc.MAX16) x the emulation's own error of the fp64 oracle (each figure: the emulation's worst
    tensor, as e32 is the fp32 oracle's); exact zeros where the fp64 gradient is identically zero; the worst element named on
    failure.  -> (references, per-tensor errors, the worst norm error)."""
    ref, errs = errors(case, grads, pred, k)
    e1p = emu.emulated(case, axes, linears)
    bound = lc.bounds(e1p)
    n, m, kn, km = gc.worst_of({k_: e for k_, e in errs.items() if not e.zero_ref})
    print(f"one-pass attention step vs fp64, {case.id} axes={axes} linears={linears}: norm_rel {n:.2e} (emulation {e1p[0]:.2e}, ratio "
          f"{n / e1p[0]:.2f}, {kn}); max_rms {m:.2e} (emulation {e1p[1]:.2e}, ratio {m / e1p[1]:.2f}, {km}, {errs[km].where()}); "
          f"{n / ref.e32[0]:.0f} x e32 in the norm")
    bad = gc.violations(errs, bound, factor=1.0)            # (its "x e32" reads: x the bound)
    assert not bad, "\n".join([f"{case.id}: outside ({lc.NORM16:g}, {lc.MAX16:g}) x the emulation's error = ({bound[0]:.2e}, "
                               f"{bound[1]:.2e})"] + bad)
    return ref, errs, n


@pytest.mark.parametrize("case", emu.STEP_CASES, ids=lambda c: c.id)
def test_one_pass_step_is_in_the_emulations_error_class_and_its_twin_in_fp32_class(monkeypatch, case):
    ((g1, p1),), text1 = gpu_steps(monkeypatch, case, TRAIN_ATTN_PASSES="1")
    ((g3, p3),), text3 = gpu_steps(monkeypatch, case)
    assert emu.SWITCH + "=1" in text1 and "one fp16-MFMA pass" in text1 and emu.SWITCH not in text3, (text1, text3)
    ref, _, n1 = check_one_pass(case, g1, p1)
    # it IS another arithmetic: beyond the three-pass route's bound in the norm (a library that ignores the switch fails here)
    assert n1 > gc.FACTOR * ref.e32[0], (n1, ref.e32)
    # the default route beside it: untouched, fp32-class
    _, errs3 = errors(case, g3, p3)
    print(gc.report(f"default route in the same test, {case.id}", errs3, ref.e32))
    assert gc.violations(errs3, ref.e32) == []


def test_beside_the_one_pass_linears_it_is_bounded_by_the_emulation_of_both(monkeypatch):
    case = emu.BOTH_CASE
    ((gb, pb),), text = gpu_steps(monkeypatch, case, TRAIN_ATTN_PASSES="1", TRAIN_PASSES="1")
    ((gl, pl),), _ = gpu_steps(monkeypatch, case, TRAIN_PASSES="1")
    assert emu.SWITCH + "=1" in text and "D3DP_TRAIN_PASSES=1" in text, text
    check_one_pass(case, gb, pb, linears=True)
    assert not torch.equal(pb, pl)                                          # ... and it is not the Linears-only route
    differ = [n for n in gb if not torch.equal(gb[n], gl[n])]
    assert len(differ) > len(gb) // 2, differ


def test_under_x2t_the_temporal_axis_alone_takes_the_route(monkeypatch):
    case = emu.X2T_CASE
    ((g1, p1),), text = gpu_steps(monkeypatch, case, TRAIN_ATTN_PASSES="1", TRAIN_ATTN="x2t")
    ((g3, p3),), _ = gpu_steps(monkeypatch, case, TRAIN_ATTN="x2t")
    assert emu.SWITCH + "=1" in text and "temporal attention" in text.split(emu.SWITCH)[1], text
    ref, _, n1 = check_one_pass(case, g1, p1, axes="t")
    assert n1 > gc.FACTOR * ref.e32[0], (n1, ref.e32)
    _, errs3 = errors(case, g3, p3)
    assert gc.violations(errs3, ref.e32) == []


def test_branches_dropped_for_every_sample_have_exactly_zero_gradients(monkeypatch):
    case = emu.DROPPED_CASE
    ((grads, pred),), _ = gpu_steps(monkeypatch, case, TRAIN_ATTN_PASSES="1")
    _, errs, _ = check_one_pass(case, grads, pred)
    assert sorted(n for n, e in errs.items() if e.zero_ref) == sorted(DROPPED_PARAMS)
    for n in DROPPED_PARAMS:
        assert torch.equal(grads[n], torch.zeros_like(grads[n])), n
    assert all(torch.isfinite(g).all() for g in grads.values())


def test_gradients_scale_with_the_upstream_gradient_bit_for_bit(monkeypatch):
    """loss.backward(loss * 2^k), k = -40, 0, +30: dO is rounded at the power of two of its own absmax and dS at the running power of
    two of its row, so the k != 0 gradients x 2^-k equal the k = 0 gradients bit for bit."""
    case = emu.UPSTREAM_CASE
    steps, _ = gpu_steps(monkeypatch, case, ks=emu.UPSTREAM_K, TRAIN_ATTN_PASSES="1")
    runs = dict(zip(emu.UPSTREAM_K, steps))
    for k, (grads, pred) in runs.items():
        check_one_pass(case, grads, pred, k=k)
    base = runs[0][0]
    for k in emu.UPSTREAM_K:
        differ = [n for n, g in runs[k][0].items() if not torch.equal(g * 2.0 ** -k, base[n])]
        assert not differ, (k, differ)
        assert torch.equal(runs[k][1], runs[0][1])


def test_the_one_pass_step_is_bit_reproducible_on_one_and_two_streams(monkeypatch):
    """Two steps of one context give the same bits, under D3DP_TRAIN_OVERLAP=0, =1 and the default -- and the three agree: the
    stream schedule does not enter the arithmetic."""
    case = emu.STEP_CASES[3]
    runs = {}
    for overlap in ("0", "1", None):
        ((g0, p0), (g1, p1)), _ = gpu_steps(monkeypatch, case, ks=(0, 0), TRAIN_ATTN_PASSES="1",
                                            **({"TRAIN_OVERLAP": overlap} if overlap else {}))
        assert torch.equal(p0, p1), overlap
        for n in g0:
            assert torch.equal(g0[n], g1[n]), (overlap, n)
        runs[overlap] = (g0, p0)
    for overlap in ("0", "1"):
        assert torch.equal(runs[overlap][1], runs[None][1]), overlap
        for n, g in runs[None][0].items():
            assert torch.equal(runs[overlap][0][n], g), (overlap, n)
    assert any(g.abs().max() > 0 for g in runs[None][0].values())


def test_the_route_changes_neither_the_launches_nor_the_workspace(monkeypatch):
    case = emu.STEP_CASES[3]
    seen = {}
    for passes in (3, 1):
        route(monkeypatch, **({"TRAIN_ATTN_PASSES": "1"} if passes == 1 else {}))
        sd, x2d, gt, t, noise, dpd = problem(case)
        m = model_of(case, sd)
        pe = m.pose_estimator
        ctx = pe._context(torch.device("cuda", torch.cuda.current_device()))
        nbytes = C.c_size_t()
        _lib.check(_lib.load().d3dp_train_workspace_bytes(ctx, case.B, C.byref(nbytes)), "d3dp_train_workspace_bytes")
        pe.profile_enable(True)
        step(m, x2d.cuda(), gt.cuda(), t, noise, dpd)
        prof = pe.profile_read()
        pe.profile_enable(False)
        seen[passes] = (nbytes.value, {k: v[0] for k, v in prof.items()})
    assert seen[1] == seen[3], seen
    attn = [k for k, v in seen[1][1].items() if "attn" in k and v > 0]
    assert len(attn) >= 5, seen[1][1]                        # forward and pass Q of both axes, pass KV of the temporal one


def test_a_refusal_comes_back_through_the_real_library(monkeypatch):
    route(monkeypatch, TRAIN_ATTN_PASSES="2")
    rc, msg = create(512, _lib.MODE_TRAIN)
    assert rc == D3DP_ENOTSUP and emu.SWITCH + "=2" in msg, (rc, msg)
    sd, x2d, gt, t, noise, dpd = problem(emu.STEP_CASES[5])
    with pytest.raises(Exception, match=emu.SWITCH):
        step(model_of(emu.STEP_CASES[5], sd), x2d.cuda(), gt.cuda(), t, noise, dpd)
