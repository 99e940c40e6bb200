"""The element-by-element gradient check of tests/test_hip_train_grads.py, as far as a CPU can check it (no GPU needed):
every case of the GPU matrix is well-conditioned by the reference's own measure, the comparator rejects the defect the older norm
bound lets through (a split product that lost its lo x hi pass: a factor 1 + 2^-11 on one tile), and the reference is exactly
equivariant under a power-of-two upstream gradient."""
import pytest
import torch

from oracle import grad_check as gc
from test_hip_train_grads import ALL_CASES, DROPPED, DROPPED_PARAMS, Case, problem, reference

OLD_NORM_BOUND = 2e-3          # tests/test_hip_parity.py, tests/test_hip_widths.py (5e-3 elsewhere)
INJECT_CASES = [Case(512, 27, 2), Case(128, 9, 2), Case(256, 40, 2)]
INJECT_PARAMS = [f"STEblocks.1.{n}" for n in ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.bias", "norm1.weight")]
DROPPED_PASS = 1 + 2.0 ** -11


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.id)
def test_every_gpu_case_is_admissible(case):
    """e32 -- the oracle's fp32 autograd against its fp64 autograd -- is at most 2e-6 (norm) and 5e-5 (per element): 8 x e32 then
    separates fp32-class from almost.  The dropped-branch cases have their 12 exactly-zero fp64 gradients."""
    ref = reference(case)
    print(f"{case.id}: e32 norm_rel {ref.e32[0]:.2e}, max_rms {ref.e32[1]:.2e}")
    assert ref.e32[0] <= gc.ADMIT_NORM_REL and ref.e32[1] <= gc.ADMIT_MAX_RMS, ref.e32
    zeros = sorted(n for n, g in ref.g64.items() if not g.any())
    assert zeros == (sorted(DROPPED_PARAMS) if case in DROPPED else []), zeros
    assert not gc.violations(gc.grad_errors(ref.g32, ref.g64), ref.e32)      # (the fp32 oracle passes its own check, zeros included)


def patterns(g):
    """The four perturbations of one gradient: (name, perturbed copy, must the comparator reject it)."""
    out = []

    def add(name, sel, must):
        p = g.clone()
        p[sel] *= DROPPED_PASS
        out.append((name, p, must))
    if g.dim() == 2:
        r0 = g.shape[0] // 2 // 16 * 16
        add("16 rows", slice(r0, r0 + 16), True)
        add("last 64 columns", (slice(None), slice(-64, None)), True)
        add("last row", slice(-1, None), False)
    else:
        add("first 16 entries", slice(0, 16), True)
        add("last entry", slice(-1, None), False)
    return out


def test_comparator_rejects_a_dropped_cross_pass_in_one_tile():
    """The fp32 oracle gradients with 16 rows / the last 64 columns / the first 16 entries of one parameter multiplied by 1 + 2^-11:
    the 8 x e32 bound rejects every one, the old 2e-3 norm bound accepts every one.  A single last row or entry is below what the
    bound resolves for some parameters (a trial: 3 misses in 15): that row is printed, not asserted."""
    last = []
    for case in INJECT_CASES:
        ref = reference(case)
        for name in INJECT_PARAMS:
            for pat, g, must in patterns(ref.g32[name]):
                e = gc.tensor_error(g, ref.g64[name])
                rejected = bool(gc.violations({name: e}, ref.e32))
                assert e.norm_rel < OLD_NORM_BOUND, (case.id, name, pat, e)
                if must:
                    assert rejected, (case.id, name, pat, e, ref.e32)
                else:
                    last.append((case.id, name, rejected, e.norm_rel / ref.e32[0], e.max_rms / ref.e32[1]))
    missed = [x for x in last if not x[2]]
    print(f"last row / entry x (1 + 2^-11): rejected in {len(last) - len(missed)} of {len(last)} tries; missed: "
          + "; ".join(f"{c} {n} (norm_rel {a:.1f} x e32, max_rms {b:.1f} x e32)" for c, n, _, a, b in missed))


def test_comparator_rejects_nonzero_or_nonfinite_where_the_reference_is_zero():
    r = {"w": torch.zeros(4, 4, dtype=torch.float64), "v": torch.ones(4, dtype=torch.float64)}
    e32 = (1e-7, 1e-6)
    ok = {"w": torch.zeros(4, 4), "v": torch.ones(4)}
    assert not gc.violations(gc.grad_errors(ok, r), e32)
    tiny = {"w": torch.zeros(4, 4), "v": torch.ones(4)}
    tiny["w"][3, 1] = 1e-30
    bad = gc.violations(gc.grad_errors(tiny, r), e32)
    assert len(bad) == 1 and "row 3 col 1" in bad[0], bad
    for poison in (float("nan"), float("inf")):
        for k in ("w", "v"):
            g = {n: t.clone() for n, t in ok.items()}
            g[k].view(-1)[2] = poison
            assert len(gc.violations(gc.grad_errors(g, r), e32)) == 1, (poison, k)


def test_reference_is_equivariant_under_a_power_of_two_upstream_gradient():
    """fp32 oracle gradients with the upstream gradient x 2^-40 and x 2^30 equal the unscaled ones x the same power bit for bit
    (nothing underflows), which is what the GPU test then demands of the kernels."""
    case = Case(128, 9, 2)
    sd, x2d, gt, t, noise, dpd = problem(case)
    base, _ = gc.reference_grads(sd, x2d, gt, t, noise, case.dep, dpd, torch.float32)
    for k in (-40, 30):
        g, _ = gc.reference_grads(sd, x2d, gt, t, noise, case.dep, dpd, torch.float32, upstream_scale=2.0 ** k)
        for n in base:
            assert torch.equal(g[n], base[n] * 2.0 ** k), (k, n)
