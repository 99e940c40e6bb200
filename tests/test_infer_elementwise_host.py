"""The element-by-element inference check of tests/test_hip_infer_elementwise.py, as far as a CPU can check it (no GPU needed):
every case of the GPU matrix is well-conditioned by the reference's own measure and the fp32 oracle passes its own check; the
comparator rejects the defect the mm gate lets through (a split product that lost its lo x hi pass in one 16-row tile: a factor
1 + 2^-11 on 16 token rows of one MLP output); a single NaN is a violation that names its element."""
import pytest
import torch

from oracle import d3dp_oracle as orc
from oracle import infer_check as ic
from test_hip_infer_elementwise import ALL_CASES, RANGE_EDITS, SAMPLERS, SPLIT_RANGE, Case, expected_implementation, problem, reference

EXACT_TOL_MM = 1e-3            # tests/test_hip_parity.py: the gate of every denoiser- and sampler-level test of EXACT mode
LOST_PASS = 1 + 2.0 ** -11
INJECT_CASES = [Case(512, 243, 1, 1), Case(512, 27, 2, 2), Case(128, 27, 2, 2)]


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.id)
def test_every_gpu_case_is_admissible(case):
    """e32 -- the oracle's fp32 forward against its fp64 forward -- is at most 2e-6 (norm) and 5e-5 (per element): 8 x e32 then
    separates fp32-class from almost; and the fp32 oracle passes its own check."""
    ref = reference(case)
    print(f"{case.id}: e32 norm_rel {ref.e32[0]:.2e}, max_rms {ref.e32[1]:.2e}")
    assert ic.admissible(ref.e32), ref.e32
    line, bad, _ = ic.check(case.id, ref.out32, ref.out64, ref.e32, case.chunk_seqs)
    assert not bad, bad


@pytest.mark.parametrize("case", SAMPLERS, ids=lambda c: c.id)
def test_every_sampler_case_is_admissible_at_every_step(case):
    ref = reference(case)
    for k in range(case.K):
        print(f"{case.id} step {k}: e32 norm_rel {ref.e32[k][0]:.2e}, max_rms {ref.e32[k][1]:.2e}")
        assert ic.admissible(ref.e32[k]), (k, ref.e32[k])
        assert not ic.check(case.id, ref.out32[:, k], ref.out64[:, k], ref.e32[k])[1]
    on_clamp = (ref.out64.abs() == 1.1).double().mean().item()
    print(f"{case.id}: {100 * on_clamp:.2f} % of the fp64 outputs sit on the clamp")


def test_the_range_edits_reach_the_range_proof_and_nothing_else():
    """Both new edits put the bound the weights prove at twice what 2^4 holds (so a scale must drop) and leave every LayerNorm's own
    bound inside the range (so the context stays on split-fp16); the softmax operands q and k are untouched."""
    for case in ALL_CASES:
        if case.edit not in RANGE_EDITS:
            continue
        sd, base = problem(case)[0], problem(case._replace(edit=""))[0]
        assert expected_implementation(case, sd) == "f16x2"
        cs, blk = case.cs, "pose_estimator.TTEblocks.0."
        norm, key = ("norm1", "attn.qkv") if "v-rows" in case.edit else ("norm2", "mlp.fc1")
        ln = (cs - 1) ** 0.5 * sd[blk + norm + ".weight"].double().abs() + sd[blk + norm + ".bias"].double().abs()
        bound = (sd[blk + key + ".weight"].double().abs() @ ln + sd[blk + key + ".bias"].double().abs()).max().item()
        print(f"{case.id}: bound by the weights {bound:.1f}")
        assert 2.0 * SPLIT_RANGE <= bound < 2.0 * SPLIT_RANGE + 10.0
        changed = [k for k in sd if not torch.equal(sd[k], base[k])]
        assert changed == [blk + key + ".weight"]
        if "v-rows" in case.edit:
            assert torch.equal(sd[changed[0]][:2 * cs], base[changed[0]][:2 * cs])


def _lose_a_pass_in_one_tile(monkeypatch):
    """orc.mlp wrapped: token rows 16:32 of TTE block 0's MLP output come back x (1 + 2^-11).  Nothing else in the oracle's
    arithmetic changes (every other call goes straight through)."""
    plain = orc.mlp

    def mlp(x, p, pre):
        y = plain(x, p, pre)
        if pre == "TTEblocks.0.":
            y = y.clone()
            y.reshape(-1, y.shape[-1])[16:32] *= LOST_PASS
        return y
    monkeypatch.setattr(orc, "mlp", mlp)


def test_comparator_rejects_a_lost_pass_in_one_tile(monkeypatch):
    """The fp32 oracle with 16 consecutive token rows of one MLP output multiplied by 1 + 2^-11 -- what a lost lo x hi pass does to
    one row tile: 8 x e32 rejects its output in every case; the mm gate of EXACT mode accepts it at F = 243."""
    refs = {case: reference(case) for case in INJECT_CASES}         # (before the oracle is wrapped)
    _lose_a_pass_in_one_tile(monkeypatch)
    for case, ref in refs.items():
        sd, x2d, x3d, t = problem(case)
        with torch.no_grad():
            broken = orc.mixste_forward(orc.strip_prefix(sd), x2d, x3d, t, case.dep)
        assert not torch.equal(broken.double(), ref.out32)
        line, bad, e = ic.check(f"lost pass in rows 16:32 of TTEblocks.0's MLP, {case.id}", broken, ref.out64, ref.e32)
        mm = orc.mpjpe_mm(broken, ref.out32.float())
        print(f"{line}; {mm:.2e} mm from the fp32 oracle")
        assert bad and e.max_rms > ic.FACTOR * ref.e32[1], (case.id, e, ref.e32)
        if case.Fr == 243:
            assert mm <= EXACT_TOL_MM, mm


def test_a_single_nan_is_a_violation_that_names_its_element():
    ref = reference(Case(128, 9, 2, 2))
    got = ref.out32.clone()
    assert not ic.check("clean", got, ref.out64, ref.e32)[1]
    got[1, 0, 7, 16, 2] = float("nan")
    _, bad, e = ic.check("one NaN", got, ref.out64, ref.e32)
    assert len(bad) == 1 and "(b, h, f, j, c) = (1, 0, 7, 16, 2)" in bad[0], bad
    assert f"row {2 * 9 * 17 + 7 * 17 + 16} of pass 0" in bad[0], bad
    assert e.norm_rel == float("inf") and e.max_rms == float("inf")
