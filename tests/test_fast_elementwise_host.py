"""The element-by-element FAST / FAST16 check of tests/test_hip_fast_elementwise.py, as far as a CPU can check it (no GPU needed):
every case of the GPU matrix is admissible by the reference's own measure (the 2-byte emulation under a second accumulation order
stays within (1.15, 2.0) x e16 of fp64, and passes the check itself); the comparator rejects the defect the mean gates let through
(ONE Linear of the emulated denoiser loses the first 32 k-columns in its first 16 rows); a single NaN is a violation that names its
element; the single-op models are in the class of one rounding."""
import pytest
import torch
import torch.nn.functional as F

from oracle import d3dp_oracle as orc
from oracle import lowp_check as lc
from test_hip_fast16 import FP16_MAX, proven_bound_fp64
from test_hip_fast16_scaled import block_bounds_fp64, shifts_fp64
from test_hip_fast_elementwise import BOTH_MODES, EDITS, MODES, SAMPLERS, SCALED, Case, problem, reference, state_dict_of
from test_hip_parity import FAST_TOL_MM

INJECT_CASES = [Case(128, 27, 2, 2), Case(512, 27, 2, 2), Case(256, 27, 2, 2), Case(128, 27, 2, 2, dep=8)]


def _admissible(case, mode, ref, e16, spread, tag=""):
    print(f"{case.id} {mode}{tag}: e16 norm_rel {e16[0]:.2e}, max_rms {e16[1]:.2e}; spread x{spread[0]:.3f}, x{spread[1]:.3f}")
    assert lc.admissible(spread), (case.id, mode, spread)
    assert e16[0] > 0 and e16[1] > 0


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", BOTH_MODES, ids=lambda c: c.id)
def test_every_gpu_case_is_admissible(case, mode):
    """spread <= (1.15, 2.0): what e16 says does not depend on the accumulation order, so (1.5, 4) x e16 separates 2-byte-class from
    almost; the fp64 output is finite and non-zero; both emulations pass the check; an unedited case's weights prove the fp16 range."""
    ref = reference(case, mode)
    assert torch.isfinite(ref.out64).all() and ref.out64.any() and ref.finite
    _admissible(case, mode, ref, ref.e16, ref.spread)
    for emu in (ref.emu, ref.emu_h):
        assert not lc.check(case.id, emu, ref.out64, ref.e16, case.chunk_seqs)[1]
    if mode == "fast16":
        prefix = "pose_estimator." if case.joints == 17 else ""
        assert proven_bound_fp64(problem(case)[0], case.cs, case.dep, prefix=prefix)[0] < FP16_MAX


@pytest.mark.parametrize("case", SCALED, ids=lambda c: c.id)
def test_every_scaled_case_is_admissible_and_its_emulation_stays_in_range(case):
    """The reference of a scaled case is the UNSCALED fp16 emulation on the edited weights: every value it rounds to fp16 stays
    finite (below 65504), so a power-of-two scale commutes with each of its roundings."""
    ref = reference(case, "fast16")
    print(f"{case.id}: largest fp16 intermediate of the emulation {ref.max_abs:.4g}")
    assert torch.isfinite(ref.out64).all() and ref.out64.any()
    assert ref.finite and ref.max_abs < FP16_MAX and torch.isfinite(ref.emu).all() and torch.isfinite(ref.emu_h).all()
    _admissible(case, "fast16", ref, ref.e16, ref.spread)


def test_the_scaled_edits_produce_their_exponents_and_the_v_row_edits_leave_the_softmax_alone():
    for case in SCALED:
        sd = state_dict_of(case)
        got = shifts_fp64(block_bounds_fp64(sd, case.cs, case.dep))
        assert got == EDITS[case.edit][1] and 0 < max(got) <= 8, (case.id, got)
        if EDITS[case.edit][0] is not None:
            base = state_dict_of(case._replace(edit=""))
            changed = [k for k in sd if not torch.equal(sd[k], base[k])]
            assert len(changed) == 1 and changed[0].endswith("attn.qkv.weight"), changed
            assert torch.equal(sd[changed[0]][:2 * case.cs], base[changed[0]][:2 * case.cs])
    assert all(any(EDITS[c.edit][1][i] > 0 for c in SCALED) for i in range(4))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", SAMPLERS, ids=lambda c: c.id)
def test_every_sampler_case_is_admissible_at_every_step(case, mode):
    ref = reference(case, mode)
    assert torch.isfinite(ref.out64).all() and ref.out64.any() and ref.finite
    for k in range(case.K):
        _admissible(case, mode, ref, ref.e16[k], ref.spread[k], f" step {k}")
        assert not lc.check(case.id, ref.emu_h[:, k], ref.out64[:, k], ref.e16[k])[1]


def _emulate_with_a_defect(case, mode, which):
    """The emulation of `case` with F.linear wrapped for ONE call (the `which`-th of the forward pass): its first 16 rows are computed
    without the first 32 k-columns.  Every other call goes straight through.  -> (output as fp64, the number of F.linear calls)."""
    sd, x2d, x3d, t = problem(case)
    plain, count = F.linear, [0]

    def linear(x, w, b=None):
        count[0] += 1
        y = plain(x, w, b)
        if count[0] == which:
            k = w.shape[1]
            lost = x.reshape(-1, k)[:16].clone()
            lost[:, :32] = 0
            y = y.clone()
            y.reshape(-1, w.shape[0])[:16] = plain(lost, w, b)
        return y
    F.linear = linear
    try:
        with torch.no_grad(), lc.rounding(MODES[mode][0]):
            out = orc.mixste_forward(orc.emulate_bf16(orc.strip_prefix(sd)), x2d, x3d, t, case.dep).double()
    finally:
        F.linear = plain
    return out, count[0]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", INJECT_CASES, ids=lambda c: c.id)
def test_comparator_rejects_lost_k_columns_in_one_tile_which_the_mean_gates_accept(case, mode):
    """One Linear in the middle of the stack and one near its end: the per-element figure leaves MAX16 x e16 by a factor 1.5 at
    least, while the same output passes the mean gate it passes today (bf16: <= 1.5 x the emulation's own mm; fp16: <= 8 mm)."""
    ref = reference(case, mode)
    clean, n = _emulate_with_a_defect(case, mode, 0)
    assert torch.equal(clean, ref.emu)
    want32 = ref.out64.float()
    emu_mm = orc.mpjpe_mm(ref.emu, want32)
    for which in (n // 2, n - 2):
        broken, _ = _emulate_with_a_defect(case, mode, which)
        assert not torch.equal(broken, ref.emu)
        line, bad, e = lc.check(f"{mode} emulation, Linear {which} of {n} lost 32 k-columns in 16 rows, {case.id}", broken, ref.out64,
                                ref.e16, case.chunk_seqs)
        mm = orc.mpjpe_mm(broken, want32)
        print(f"{line}; {mm:.3f} mm from the oracle (the emulation: {emu_mm:.3f} mm)")
        assert bad and e.max_rms >= 1.5 * lc.MAX16 * ref.e16[1], (case.id, mode, which, e, ref.e16)
        assert mm <= (1.5 * emu_mm if mode == "fast" else FAST_TOL_MM), (mm, emu_mm)


def test_a_single_nan_is_a_violation_that_names_its_element():
    case = Case(128, 27, 2, 2)
    ref = reference(case, "fast")
    got = ref.emu.clone()
    assert not lc.check("clean", got, ref.out64, ref.e16)[1]
    got[1, 0, 7, 16, 2] = float("nan")
    _, bad, e = lc.check("one NaN", got, ref.out64, ref.e16)
    assert len(bad) == 1 and "(b, h, f, j, c) = (1, 0, 7, 16, 2)" in bad[0], bad
    assert f"row {2 * 27 * 17 + 7 * 17 + 16} of pass 0" in bad[0], bad
    assert e.norm_rel == float("inf") and e.max_rms == float("inf")
    op = lc.linear_model(torch.randn(20, 64).bfloat16(), torch.randn(8, 64).bfloat16(), torch.randn(8), lc.EPI_BIAS, torch.bfloat16)
    got = op.model.clone()
    got[17, 5] = float("nan")
    _, bad, _ = lc.check("one NaN in an op", got, op.exact, op.e16)
    assert len(bad) == 1 and "row 17 col 5 of 20 x 8" in bad[0], bad


@pytest.mark.parametrize("dt,ulp", [(torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)], ids=["bf16", "fp16"])
def test_the_op_models_are_one_rounding_from_fp64_and_a_lost_tile_is_rejected(dt, ulp):
    """Each model passes its own check; its per-element distance from the unrounded result is at most an ulp of the largest output
    (the GELU form: its two roundings); and a Linear that lost 32 k-columns in 16 rows is outside the per-element bound."""
    g = torch.Generator().manual_seed(3)
    A, W, bias = torch.randn(300, 512, generator=g).to(dt), (torch.randn(192, 512, generator=g) / 512 ** 0.5).to(dt), torch.randn(192, generator=g)
    qkv = torch.randn(2 * 49 * 3, 3 * 128, generator=g).to(dt)
    x, w, b = torch.randn(67, 192, generator=g) * 3, torch.randn(192, generator=g), torch.randn(192, generator=g)
    ops = {"linear BIAS": lc.linear_model(A, W, bias, lc.EPI_BIAS, dt), "linear GELU": lc.linear_model(A, W, bias, lc.EPI_GELU, dt),
           "attention": lc.attention_model(qkv, 2, 49, 3, 128, 8, 1, dt), "layernorm": lc.layernorm_model(x, w, b, 1e-6, dt)}
    for name, op in ops.items():
        print(f"{name}: e16 norm_rel {op.e16[0]:.2e}, max_rms {op.e16[1]:.2e}")
        assert not lc.check(name, op.model, op.exact, op.e16)[1]
        rms = op.exact.pow(2).mean().sqrt().item()
        assert 0 < op.e16[1] * rms <= (2.5 if "GELU" in name else 1.0) * ulp * op.exact.abs().max().item()
    op = ops["linear BIAS"]
    lost = A.double().clone()
    lost[:16, :32] = 0
    line, bad, e = lc.check("32 k-columns lost in 16 rows", lc.rnd(lost @ W.double().t() + bias.double(), dt), op.exact, op.e16)
    print(line)
    assert bad and e.max_rms > 1.5 * lc.MAX16 * op.e16[1]
