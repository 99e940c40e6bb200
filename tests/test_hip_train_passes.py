"""The opt-in one-pass fp16 training Linears (D3DP_TRAIN_PASSES=1; run with ``-m gpu`` on an MI355X).

With the switch every product of X2Train's Linears -- forward, dgrad, both weight-gradient forms -- is ONE fp16-MFMA pass on the hi
planes of its split operands: each operand rounded to IEEE fp16 at the power of two its own absmax asks for, fp32 accumulation, the
same scales, k order, partial sums and streams (gemm_x2_train.hip, PASSES = 1).  Three layers of checks:

  1. the Linear alone through the test hook (d3dp_debug_train_linear, tail | 16): bit-equal to the three-pass kernel on operands
     already rounded that way (their lo planes are zero), and within oracle/lowp_check.py's (1.5, 4) x of the one-rounding model's own
     distance from fp64;
  2. the training step: the prediction and every parameter gradient against the oracle's fp64 autograd, bounded by (1.5, 4) x the
     error of the CPU emulation of the route in the same case (tests/train_passes_emu.py; tests/test_train_passes_host.py shows every
     case admissible) -- and FARTHER than 8 x e32 from fp64 in the norm, so it cannot be the three-pass route, whose twin in the same
     test still passes oracle/grad_check.py;
  3. 20 AdamW steps of the trainer: the final loss of the two routes differs by at most 4 x what the emulation and plain fp32 differ
     by in oracle/caller_oracle.train_loop."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import train_passes_emu as emu
from d3dp_amd import D3DP, _lib
from d3dp_amd.trainer import fit
from d3dp_amd.weights import H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT
from oracle import grad_check as gc
from oracle import lowp_check as lc
from test_hip_train_grads import DROPPED_PARAMS, model_of, problem, step

pytestmark = pytest.mark.gpu
_SWITCHES = ("D3DP_TRAIN_PASSES", "D3DP_TRAIN_ATTN", "D3DP_TRAIN_ATTN_BWD", "D3DP_TRAIN_IMPL", "D3DP_TRAIN_WGRAD", "D3DP_TRAIN_OVERLAP",
             "D3DP_TRAIN_TAIL", "D3DP_TRAIN_GELU", "D3DP_TRAIN_LN_OPERAND", "D3DP_EXACT_IMPL")
ONE_PASS = 16                                         # d3dp_debug_train_linear: tail | 16


# ------------------------------------------------------------------------------------------------ 1. the Linear alone
def hook(A, W, b, tail, want_amax=False, amax_pos=0):
    M, K = A.shape
    N = W.shape[0]
    out = torch.full((M, N), float("nan"), device="cuda")
    amax = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = _lib.load().d3dp_debug_train_linear(A.data_ptr(), W.data_ptr(), _lib.ptr(b), out.data_ptr(), M, N, K, tail,
                                             amax.data_ptr() if want_amax else None, amax_pos, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "d3dp_debug_train_linear")
    return (out, amax.view(torch.float32).item()) if want_amax else out


def operands(M, N, K):
    """Both operands with an absmax of exactly 1.0 planted: rounding cannot move the scale (2^13)."""
    g = torch.Generator(device="cuda").manual_seed(M * 31 + N * 7 + K)
    A = (torch.randn(M, K, device="cuda", generator=g) * 0.25).clamp(-0.99, 0.99)
    W = (torch.randn(N, K, device="cuda", generator=g) * 0.25).clamp(-0.99, 0.99)
    A[M // 2, K // 3], W[N // 3, K // 2] = 1.0, -1.0
    b = torch.randn(N, device="cuda", generator=g)
    return A, W, b


def r16(x):
    """The emulation's rounding, on the device: fp16(x 2^13) / 2^13 for an absmax of 1.0."""
    s = emu.dyn_scale(x)
    assert s == 2.0 ** 13
    return (x * s).half().float() / s


LINEAR_SHAPES = [(300, 132, 64), (257, 64, 512), (256 + 140, 512, 512), (17, 1024, 512)]


@pytest.mark.parametrize("tail", [0, 1])
@pytest.mark.parametrize("M,N,K", LINEAR_SHAPES)
def test_one_pass_linear_is_the_three_pass_linear_on_rounded_operands(M, N, K, tail):
    """Operands already rounded to fp16 at their scale have lo = 0: both kernels then do the same arithmetic in the same order.  (A
    library without the route runs three passes on the UNROUNDED operands under tail | 16, or refuses the bit: either way this fails.)"""
    A, W, b = operands(M, N, K)
    Ar, Wr = r16(A), r16(W)
    assert not torch.equal(Ar, A) and not torch.equal(Wr, W)
    one = hook(A, W, b, tail | ONE_PASS)
    three_r = hook(Ar, Wr, b, tail)
    assert torch.isfinite(one).all()
    differ = (one != three_r).nonzero()
    assert differ.numel() == 0, f"{differ.shape[0]} elements differ, first at row {differ[0][0].item()} col {differ[0][1].item()}"
    assert torch.equal(hook(Ar, Wr, b, tail | ONE_PASS), one)              # rounding twice changes nothing
    assert not torch.equal(hook(A, W, b, tail), one)                       # ... and the three-pass product of A, W is another one


@pytest.mark.parametrize("tail", [0, 1])
@pytest.mark.parametrize("M,N,K", LINEAR_SHAPES)
def test_one_pass_linear_against_fp64(M, N, K, tail):
    """Within (1.5, 4) x the one-rounding model's own distance from fp64 (model: the fp64 product of the rounded operands)."""
    A, W, b = operands(M, N, K)
    exact = (A.double() @ W.double().t() + b.double()).cpu()
    model = (r16(A).double() @ r16(W).double().t() + b.double()).cpu()
    e16 = lc.figures(model, exact)
    line, bad, _ = lc.check(f"one-pass training Linear M={M} N={N} K={K} tail={tail}", hook(A, W, b, tail | ONE_PASS), exact, e16)
    print(line)
    assert not bad, "\n".join(bad)
    e3 = lc.figures(hook(A, W, b, tail), exact)
    assert e3[0] < e16[0] / 64, (e3, e16)                                   # (the three-pass kernel is another error class)


def test_one_pass_linear_leaves_the_absmax_of_its_output():
    A, W, b = operands(256 + 140, 512, 512)
    for tail in (0, 1):
        out, amax = hook(A, W, b, tail | ONE_PASS, want_amax=True)
        assert amax == out.abs().max().item()
        nobias, pmax = hook(A, W, None, tail | ONE_PASS, want_amax=True, amax_pos=1)
        assert pmax == max(nobias.max().item(), 0.0)
        assert torch.equal(hook(A, W, b, tail | ONE_PASS), out)


@pytest.mark.parametrize("tail", [2, 4, 8, 18, 32, 17 + 64, -1])
def test_the_hook_refuses_every_other_bit(tail):
    A, W, b = operands(17, 64, 64)
    out = torch.zeros(17, 64, device="cuda")
    rc = _lib.load().d3dp_debug_train_linear(A.data_ptr(), W.data_ptr(), b.data_ptr(), out.data_ptr(), 17, 64, 64, tail, None, 0,
                                             torch.cuda.current_stream().cuda_stream)
    assert rc == -1 and "tail" in _lib.load().d3dp_last_error().decode(), rc             # D3DP_EINVAL
    assert not out.any()


# ------------------------------------------------------------------------------------------------ 2. the training step
def route(monkeypatch, case, passes, overlap=None):
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if passes == 1:
        monkeypatch.setenv("D3DP_TRAIN_PASSES", "1")
    if case.cs in (192, 320, 384, 448):
        monkeypatch.setenv("D3DP_TRAIN_IMPL", "f16x2")
    if overlap is not None:
        monkeypatch.setenv("D3DP_TRAIN_OVERLAP", overlap)


def gpu_steps(monkeypatch, case, passes, n=1, overlap=None):
    """n steps of one model -- one context -- created under the route: [({name: gradient}, prediction)], and what the model says."""
    route(monkeypatch, case, passes, overlap)
    sd, x2d, gt, t, noise, dpd = problem(case)
    m = model_of(case, sd)
    x2d, gt = x2d.cuda(), gt.cuda()
    return [step(m, x2d, gt, t, noise, dpd) for _ in range(n)], m.pose_estimator.train_arithmetic()


def errors(case, grads, pred):
    ref = emu.step_refs(case)
    assert set(grads) | {gc.PREDICTION} == set(ref.g64), set(grads) ^ set(ref.g64)
    return ref, gc.grad_errors({**grads, gc.PREDICTION: pred}, ref.g64)


def check_one_pass(case, grads, pred):
    """Every tensor within (1.5, 4) x the emulation's own error of the fp64 oracle (each figure: the emulation's worst tensor, as
    e32 is the fp32 oracle's); exact zeros where the fp64 gradient is identically zero; the worst element named on failure."""
    ref, errs = errors(case, grads, pred)
    assert lc.admissible(ref.spread), ref.spread
    bound = lc.bounds(ref.e1p)
    n, m, kn, km = gc.worst_of({k: e for k, e in errs.items() if not e.zero_ref})
    print(f"one-pass step vs fp64, {case.id}: norm_rel {n:.2e} (emulation {ref.e1p[0]:.2e}, ratio {n / ref.e1p[0]:.2f}, {kn}); max_rms "
          f"{m:.2e} (emulation {ref.e1p[1]:.2e}, ratio {m / ref.e1p[1]:.2f}, {km}, {errs[km].where()}); {n / ref.e32[0]:.0f} x e32 in the norm")
    bad = gc.violations(errs, bound, factor=1.0)            # (its "x e32" reads: x the bound)
    assert not bad, "\n".join([f"{case.id}: outside ({lc.NORM16:g}, {lc.MAX16:g}) x the emulation's error = ({bound[0]:.2e}, "
                               f"{bound[1]:.2e})"] + bad)
    return ref, errs, n


@pytest.mark.parametrize("case", emu.STEP_CASES, ids=lambda c: c.id)
def test_one_pass_step_is_in_the_emulations_error_class_and_its_twin_in_fp32_class(monkeypatch, case):
    ((g1, p1),), text1 = gpu_steps(monkeypatch, case, 1)
    ((g3, p3),), text3 = gpu_steps(monkeypatch, case, 3)
    assert "D3DP_TRAIN_PASSES=1" in text1 and "one fp16-MFMA pass" in text1 and "D3DP_TRAIN_PASSES" not in text3, (text1, text3)
    ref, _, n1 = check_one_pass(case, g1, p1)
    # it IS another arithmetic: beyond the three-pass route's bound in the norm
    assert n1 > gc.FACTOR * ref.e32[0], (n1, ref.e32)
    # the default route beside it: untouched, fp32-class
    _, errs3 = errors(case, g3, p3)
    print(gc.report(f"default route in the same test, {case.id}", errs3, ref.e32))
    assert gc.violations(errs3, ref.e32) == []


def test_branches_dropped_for_every_sample_have_exactly_zero_gradients(monkeypatch):
    case = emu.DROPPED_CASE
    ((grads, pred),), _ = gpu_steps(monkeypatch, case, 1)
    _, errs, _ = check_one_pass(case, grads, pred)
    assert sorted(n for n, e in errs.items() if e.zero_ref) == sorted(DROPPED_PARAMS)
    for n in DROPPED_PARAMS:
        assert torch.equal(grads[n], torch.zeros_like(grads[n])), n
    assert all(torch.isfinite(g).all() for g in grads.values())


def test_the_one_pass_step_is_bit_reproducible_on_one_and_two_streams(monkeypatch):
    """Two steps of one context give the same bits, under D3DP_TRAIN_OVERLAP=0, =1 and the default -- and the three agree: the
    stream schedule does not enter the arithmetic."""
    case = emu.STEP_CASES[0]
    runs = {}
    for overlap in ("0", "1", None):
        ((g0, p0), (g1, p1)), _ = gpu_steps(monkeypatch, case, 1, n=2, overlap=overlap)
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
    case = emu.STEP_CASES[0]
    seen = {}
    for passes in (3, 1):
        route(monkeypatch, case, passes)
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
    assert seen[1][1]["train_linear"] > 0 and seen[1][1]["train_wgrad"] > 0


# ------------------------------------------------------------------------------------------------ 3. a short run
class _Batches:
    """The batcher interface trainer.fit uses, over the fixed batches of emu.run_problem()."""
    zero_root = True

    def __init__(self, batches):
        self.batches = [(torch.from_numpy(b3).cuda(), torch.from_numpy(b2).cuda()) for b3, b2 in batches]

    def batch_num(self):
        return emu.RUN_STEPS

    def next_epoch(self):
        for i in range(emu.RUN_STEPS):
            b3, b2 = self.batches[i % emu.RUN_BATCHES]
            yield None, b3, b2

    def random_state(self):
        return None


def trainer_run(monkeypatch, passes):
    case = SimpleNamespace(cs=emu.RUN_CS)
    route(monkeypatch, case, passes)
    sd, batches, draws = emu.run_problem()
    args = SimpleNamespace(number_of_frames=emu.RUN_F, test_time_augmentation=True, timestep=1000, scale=1.0, cs=emu.RUN_CS, dep=emu.RUN_DEP,
                           learning_rate=emu.RUN_LR, lr_decay=1.0, epochs=1, checkpoint="", checkpoint_frequency=1000, resume="",
                           debug=False, no_eval=True)
    m = D3DP(args, H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, is_train=True)
    m.load_state_dict(sd, strict=False)
    m = m.cuda()
    m.pose_estimator.drop_path_rate = 0.0               # (caller_oracle.train_loop has no DropPath)

    def kw(epoch, i):
        t, noise = draws[i % emu.RUN_BATCHES]
        return dict(t=torch.from_numpy(t)[:, None], noise=torch.from_numpy(noise))
    hist = fit(args, m, None, _Batches(batches), None, torch.device("cuda"), H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, log=lambda s: None,
               forward_kwargs=kw)
    return hist["iter_loss"]


def test_twenty_adamw_steps_end_where_the_emulation_says(monkeypatch):
    plain, emulated = emu.oracle_runs()
    budget = abs(emulated[-1] - plain[-1])
    one, three = trainer_run(monkeypatch, 1), trainer_run(monkeypatch, 3)
    diff = abs(one[-1] - three[-1])
    n = emu.RUN_BATCHES
    print(f"20 AdamW steps (cs {emu.RUN_CS}, F {emu.RUN_F}, dep {emu.RUN_DEP}): one-pass {one[0]:.5f} -> {one[-1]:.5f}, default {three[0]:.5f} -> "
          f"{three[-1]:.5f}; final-loss difference {diff:.3e}; oracle: emulation vs fp32 {budget:.3e} (ratio {diff / budget:.2f}); "
          f"default vs fp32 oracle {abs(three[-1] - plain[-1]):.3e}")
    assert len(one) == len(three) == emu.RUN_STEPS
    for losses in (one, three):
        assert sum(losses[-n:]) < sum(losses[:n]), losses
    assert diff <= 4 * budget, (diff, budget)
    assert one != three
