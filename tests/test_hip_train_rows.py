"""Opt-in hi-only operand rows of the one-pass training Linears (D3DP_TRAIN_ROWS=hi; run with ``-m gpu`` on an MI355X).

With the switch, beside D3DP_TRAIN_PASSES=1, every operand of X2Train's Linears -- activations, both forms of the weights, every dY --
is stored as plain fp16 rows (the hi value of the split alone, column c at offset c, half the row stride) and the products run the
whole-line forms of gemm_f16x2_dyn_kernel / gemm_f16x2_tn_kernel: the same hi values, the same k values in the same fragment positions
and order, the same partial sums.  So every check here is BIT equality with the D3DP_TRAIN_PASSES=1 route, whose arithmetic
tests/test_hip_train_passes.py holds against fp64:

  1. the Linear alone through the test hook (d3dp_debug_train_linear, tail | 48 against tail | 16);
  2. the training step: prediction and every parameter gradient, DropPath masks on, at the shapes that reach whole tiles, remainder
     blocks, no whole tile, no remainder and the chunked-key attention, beside every composing switch, and at depth 8 -- each test
     first asserts that the context's arithmetic text names the route (a library without it would ignore the variable and compare the
     baseline with itself);
  3. a first step at depth 8 in a NaN-filled workspace (the unused half regions and the zero rows must not leak);
  4. two steps of one context; 5. the step inside exactly the bytes of the unchanged size query, between guards; 6. per-class launch
  counts; 7. three AdamW steps of the trainer under the command line's flags."""
import ctypes as C
import importlib.util
import os
from types import SimpleNamespace

import pytest
import torch

from d3dp_amd import D3DP, _lib, cli
from d3dp_amd.trainer import fit
from d3dp_amd.weights import H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, make_state_dict, synthetic_inputs_2d, synthetic_noise
from test_hip_train_grads import Case, model_of, problem, step

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("lib_ab_hash", os.path.join(REPO, "tools", "lib_ab_hash.py"))
ab = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ab)

pytestmark = pytest.mark.gpu
SWITCH = "D3DP_TRAIN_ROWS"
_SWITCHES = (SWITCH, "D3DP_TRAIN_PASSES", "D3DP_TRAIN_ATTN_PASSES", "D3DP_TRAIN_ATTN", "D3DP_TRAIN_ATTN_BWD", "D3DP_TRAIN_IMPL",
             "D3DP_TRAIN_WGRAD", "D3DP_TRAIN_OVERLAP", "D3DP_TRAIN_TAIL", "D3DP_TRAIN_GELU", "D3DP_TRAIN_LN_OPERAND", "D3DP_TRAIN_LONG_ATTN",
             "D3DP_EXACT_IMPL")
ONE_PASS, HI_ROWS = 16, 32                             # d3dp_debug_train_linear: tail | 16, tail | 16 | 32
GUARD, PATTERN = 4096, 0xA5


# ------------------------------------------------------------------------------------------------ 1. the Linear alone
def hook_rc(A, W, b, tail, out, amax=None, amax_pos=0):
    M, K = A.shape
    return _lib.load().d3dp_debug_train_linear(A.data_ptr(), W.data_ptr(), _lib.ptr(b), out.data_ptr(), M, W.shape[0], K, tail,
                                               amax.data_ptr() if amax is not None else None, amax_pos,
                                               torch.cuda.current_stream().cuda_stream)


def hook(A, W, b, tail, want_amax=False, amax_pos=0):
    out = torch.full((A.shape[0], W.shape[0]), float("nan"), device="cuda")
    amax = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(hook_rc(A, W, b, tail, out, amax if want_amax else None, amax_pos), "d3dp_debug_train_linear")
    return (out, int(amax.item())) if want_amax else out


def operands(M, N, K):
    g = torch.Generator(device="cuda").manual_seed(M * 31 + N * 7 + K)
    A = torch.randn(M, K, device="cuda", generator=g) * 0.25
    W = torch.randn(N, K, device="cuda", generator=g) * 0.25
    return A, W, torch.randn(N, device="cuda", generator=g)


# (300: a tile and 44 remainder rows at one 64-k line; 257 / 396: remainder blocks at K = 512 (16 k-steps); 17: no whole tile;
#  256 x 128 x 128: exactly one tile, two lines)
LINEAR_SHAPES = [(300, 132, 64), (257, 64, 512), (396, 512, 512), (17, 1024, 512), (256, 128, 128)]


@pytest.mark.parametrize("tail", [0, 1])
@pytest.mark.parametrize("M,N,K", LINEAR_SHAPES)
def test_the_product_on_hi_rows_is_the_one_pass_product_bit_for_bit(M, N, K, tail):
    """(A library without the route refuses bit 5.)"""
    A, W, b = operands(M, N, K)
    one = hook(A, W, b, tail | ONE_PASS)
    hi = hook(A, W, b, tail | ONE_PASS | HI_ROWS)
    assert torch.isfinite(hi).all()
    differ = (hi != one).nonzero()
    assert differ.numel() == 0, f"{differ.shape[0]} elements differ, first at row {differ[0][0].item()} col {differ[0][1].item()}"
    assert torch.equal(hook(A, W, None, tail | ONE_PASS | HI_ROWS), hook(A, W, None, tail | ONE_PASS))      # without a bias
    for amax_pos in (0, 1):
        o1, a1 = hook(A, W, b, tail | ONE_PASS, want_amax=True, amax_pos=amax_pos)
        oh, ah = hook(A, W, b, tail | ONE_PASS | HI_ROWS, want_amax=True, amax_pos=amax_pos)
        assert torch.equal(oh, o1) and ah == a1 and ah != 0, (amax_pos, ah, a1)                              # the slot: the same bits


@pytest.mark.parametrize("tail", [32, 33, 48 | 64, 49 | 64, 48 | 2])
def test_the_hook_refuses_hi_rows_without_one_pass_and_every_other_bit(tail):
    A, W, b = operands(17, 64, 64)
    out = torch.zeros(17, 64, device="cuda")
    rc = hook_rc(A, W, b, tail, out)
    assert rc == -1 and "tail" in _lib.load().d3dp_last_error().decode(), rc             # D3DP_EINVAL
    assert not out.any()


def test_the_hook_refuses_a_contraction_that_is_no_whole_number_of_lines():
    A, W, b = operands(40, 64, 96)
    out = torch.zeros(40, 64, device="cuda")
    for tail in (48, 49):
        rc = hook_rc(A, W, b, tail, out)
        msg = _lib.load().d3dp_last_error().decode()
        assert rc == -1 and "K = 96" in msg and "64" in msg, (rc, msg)
    assert not out.any()
    assert torch.isfinite(hook(A, W, b, ONE_PASS)).all()                                  # (split rows take K = 96)


# ------------------------------------------------------------------------------------------------ 2. the training step
def route(monkeypatch, hi, **others):
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("D3DP_TRAIN_PASSES", "1")
    if hi:
        monkeypatch.setenv(SWITCH, "hi")
    for k, v in others.items():
        monkeypatch.setenv("D3DP_" + k, v)


def gpu_steps(monkeypatch, case, hi, n=1, **others):
    """n steps of one model -- one context -- created under the route: [({name: gradient}, prediction)], and what the model says."""
    route(monkeypatch, hi, **others)
    sd, x2d, gt, t, noise, dpd = problem(case)
    m = model_of(case, sd)
    x2d, gt = x2d.cuda(), gt.cuda()
    return [step(m, x2d, gt, t, noise, dpd) for _ in range(n)], m.pose_estimator.train_arithmetic()


_BASELINE = {}


def baseline(monkeypatch, case, **others):
    """The D3DP_TRAIN_PASSES=1 step of a case under the other switches: computed once, shared, never written to."""
    key = (case, tuple(sorted(others.items())))
    if key not in _BASELINE:
        ((g, p),), text = gpu_steps(monkeypatch, case, False, **others)
        assert "D3DP_TRAIN_PASSES=1" in text and SWITCH not in text, text
        _BASELINE[key] = (g, p)
    return _BASELINE[key]


def assert_same_step(got, want, tag):
    (g, p), (g0, p0) = got, want
    assert torch.isfinite(p).all() and torch.equal(p, p0), f"{tag}: the prediction differs in {(p != p0).sum().item()} elements"
    assert set(g) == set(g0)
    bad = [f"{n}: {(g[n] != g0[n]).sum().item()} of {g[n].numel()}" for n in g if not torch.equal(g[n], g0[n])]
    assert not bad, f"{tag}: gradients differ -- " + "; ".join(bad[:8])
    assert any(x.abs().max() > 0 for x in g.values())


def check_route(monkeypatch, case, **others):
    want = baseline(monkeypatch, case, **others)
    ((g, p),), text = gpu_steps(monkeypatch, case, True, **others)
    assert SWITCH + "=hi" in text and "D3DP_TRAIN_PASSES=1" in text, text           # else the variable was ignored: a vacuous comparison
    assert_same_step((g, p), want, case.id + "".join(f" {k}={v}" for k, v in others.items()))


STEP_CASES = [
    Case(512, 9, 2),           # T = 306: a row of tiles plus remainder blocks (K = 512, 1024)
    Case(256, 27, 2),          # T = 918: K = 256 has 8 k-steps -- whole tiles only; K = 512 remainder blocks
    Case(256, 9, 1),           # T = 153: no whole tile
    Case(256, 128, 2),         # T = 4352 = 17 x 256: no remainder
    Case(256, 300, 2),         # the chunked-key attention writes the proj operand
]
BESIDE = [("TRAIN_ATTN_PASSES", "1"), ("TRAIN_ATTN", "f32"), ("TRAIN_ATTN", "x2t"), ("TRAIN_OVERLAP", "0"), ("TRAIN_OVERLAP", "1")]


@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: c.id)
def test_the_step_on_hi_rows_is_the_one_pass_step_bit_for_bit(monkeypatch, case):
    check_route(monkeypatch, case)


@pytest.mark.parametrize("name,value", BESIDE)
def test_the_step_beside_every_composing_switch(monkeypatch, name, value):
    check_route(monkeypatch, Case(512, 9, 2) if name != "TRAIN_ATTN_PASSES" else Case(256, 27, 2), **{name: value})


DEEP = Case(256, 9, 2, dep=8)


def test_the_step_at_depth_eight(monkeypatch):
    check_route(monkeypatch, DEEP)


# ------------------------------------------------------------------------------------------------ 3. poisoned workspace
class Guarded:
    """`n` workspace bytes between two guards, the workspace itself filled with `fill` bytes."""

    def __init__(self, n, fill):
        self.n, self.buf = n, torch.full((n + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        self.buf[GUARD:GUARD + n] = fill
        self.ptr = self.buf.data_ptr() + GUARD
        assert self.ptr % 256 == 0

    def intact(self):
        torch.cuda.synchronize()
        return bool((self.buf[:GUARD] == PATTERN).all()) and bool((self.buf[GUARD + self.n:] == PATTERN).all())


def raw_step(c, inputs, B, ws):
    out, grads = torch.full((B, c.F, c.J, 3), float("nan"), device="cuda"), c.grad_buffers(fill=float("nan"))
    assert c.train_forward(inputs, out, B, ws.ptr, ws.n) == 0, c.lib.d3dp_last_error()
    assert c.train_backward(inputs, grads, B, ws.ptr, ws.n) == 0, c.lib.d3dp_last_error()
    torch.cuda.synchronize()
    return out, c.flat_grads(grads)


def test_the_first_step_at_depth_eight_in_a_nan_filled_workspace(monkeypatch):
    """0xFF bytes are NaN as fp32 and as fp16: a read of the unused half of a region, of an unwritten zero row or of a lo value that is
    no longer stored would reach the result."""
    route(monkeypatch, True)
    B = 2
    c = ab.RawCtx("train", 256, 9, 5, 8)
    n = c.train_bytes(B)
    inputs = c.train_inputs(B)
    poisoned, clean = Guarded(n, 0xFF), Guarded(n, 0)
    out, grads = raw_step(c, inputs, B, poisoned)          # the context's FIRST step
    ref, ref_grads = raw_step(c, inputs, B, clean)
    assert poisoned.intact() and clean.intact()
    assert torch.isfinite(out).all() and torch.equal(out, ref)
    for i, (g, r) in enumerate(zip(grads, ref_grads)):
        assert torch.isfinite(g).all() and torch.equal(g, r), f"gradient {i}"


# ------------------------------------------------------------------------------------------------ 4. reproducibility
def test_two_steps_of_one_context_give_the_same_bits(monkeypatch):
    ((g0, p0), (g1, p1)), text = gpu_steps(monkeypatch, Case(512, 9, 2), True, n=2)
    assert SWITCH + "=hi" in text
    assert_same_step((g1, p1), (g0, p0), "second step")


# ------------------------------------------------------------------------------------------------ 5. workspace bounds
@pytest.mark.parametrize("cs", [256, 512])
def test_the_step_runs_inside_the_bytes_of_the_unchanged_size_query(monkeypatch, cs):
    B = 2
    route(monkeypatch, False)
    n_split = ab.RawCtx("train", cs, 9, 5, 1).train_bytes(B)
    route(monkeypatch, True)
    c = ab.RawCtx("train", cs, 9, 5, 1)
    n = c.train_bytes(B)
    assert n == n_split
    inputs = c.train_inputs(B)
    res = []
    for ws in (Guarded(n, PATTERN), Guarded(2 * n, PATTERN)):
        res.append(raw_step(c, inputs, B, ws))
        assert ws.intact()
    (out, grads), (ref, ref_grads) = res
    assert torch.isfinite(out).all() and torch.equal(out, ref)
    for i, (g, r) in enumerate(zip(grads, ref_grads)):
        assert torch.isfinite(g).all() and torch.equal(g, r), f"gradient {i}"
    tight = Guarded(n, PATTERN)
    kept = torch.full_like(out, 7.0)
    assert c.train_forward(inputs, kept, B, tight.ptr, n - 256) == -4              # D3DP_ESTATE
    assert tight.intact() and bool((kept == 7.0).all())


# ------------------------------------------------------------------------------------------------ 6. launch counts
def test_the_route_changes_neither_the_launches_nor_the_workspace(monkeypatch):
    case = Case(512, 9, 2)
    seen = {}
    for hi in (False, True):
        route(monkeypatch, hi)
        sd, x2d, gt, t, noise, dpd = problem(case)
        m = model_of(case, sd)
        pe = m.pose_estimator
        ctx = pe._context(torch.device("cuda", torch.cuda.current_device()))
        assert (SWITCH + "=hi" in pe.train_arithmetic()) == hi
        nbytes = C.c_size_t()
        _lib.check(_lib.load().d3dp_train_workspace_bytes(ctx, case.B, C.byref(nbytes)), "d3dp_train_workspace_bytes")
        pe.profile_enable(True)
        step(m, x2d.cuda(), gt.cuda(), t, noise, dpd)
        prof = pe.profile_read()
        pe.profile_enable(False)
        seen[hi] = (nbytes.value, {k: v[0] for k, v in prof.items()})
    assert seen[True] == seen[False], seen
    counts = seen[True][1]
    assert counts["train_linear"] > 0 and counts["train_wgrad"] > 0 and counts["train_operand_pass"] > 0


# ------------------------------------------------------------------------------------------------ 7. the trainer
RUN_CS, RUN_F, RUN_DEP, RUN_B, RUN_STEPS, RUN_SEED = 256, 9, 2, 2, 3, 31


class _Batches:
    """The batcher interface trainer.fit uses, over RUN_STEPS fixed batches."""
    zero_root = True

    def __init__(self):
        self.batches = []
        for i in range(RUN_STEPS):
            gt = synthetic_noise(RUN_SEED + 10 * i + 1, (RUN_B, RUN_F, 17, 3)) * 0.3
            gt[:, :, 0] = 0
            x2d = synthetic_inputs_2d(RUN_SEED + 10 * i, RUN_B, RUN_F)
            self.batches.append((torch.from_numpy(gt).float().cuda(), torch.from_numpy(x2d).float().cuda()))

    def batch_num(self):
        return RUN_STEPS

    def next_epoch(self):
        for b3, b2 in self.batches:
            yield None, b3, b2

    def random_state(self):
        return None


def trainer_run(monkeypatch, flags):
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    a = cli.parse_args(flags)
    args = SimpleNamespace(number_of_frames=RUN_F, test_time_augmentation=True, timestep=1000, scale=1.0, cs=RUN_CS, dep=RUN_DEP,
                           learning_rate=2e-4, lr_decay=1.0, epochs=1, checkpoint="", checkpoint_frequency=1000, resume="", debug=False,
                           no_eval=True)
    m = D3DP(args, H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, is_train=True)
    m.load_state_dict(make_state_dict(RUN_SEED, RUN_CS, RUN_DEP, RUN_F), strict=False)
    m = m.cuda()
    m.pose_estimator.drop_path_rate = 0.0               # (as tests/test_hip_train_passes.py: the masks of a run are drawn, not recorded;
    torch.manual_seed(RUN_SEED)                          #  the steps of section 2 run with recorded masks on)
    start = {n: p.detach().cpu().clone() for n, p in m.pose_estimator.named_parameters()}
    with cli.train_passes_env(a.train_passes), cli.train_rows_env(a.train_rows):      # (as cli.run_train: the context is created inside)
        m.pose_estimator._context(torch.device("cuda", torch.cuda.current_device()))
        text = m.pose_estimator.train_arithmetic()
    assert os.environ.get(SWITCH) is None and os.environ.get("D3DP_TRAIN_PASSES") is None
    draws = [(torch.tensor([30 + 100 * i, 700 - 100 * i])[:, None], torch.from_numpy(synthetic_noise(RUN_SEED + 10 * i + 2, (RUN_B, RUN_F, 17, 3))))
             for i in range(RUN_STEPS)]
    hist = fit(args, m, None, _Batches(), None, torch.device("cuda"), H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, log=lambda s: None,
               forward_kwargs=lambda epoch, i: dict(t=draws[i][0], noise=draws[i][1]))
    torch.cuda.synchronize()
    end = {n: p.detach().cpu().clone() for n, p in m.pose_estimator.named_parameters()}
    assert sum(not torch.equal(end[n], start[n]) for n in end) > len(end) // 2        # the run did train
    return hist["iter_loss"], end, text


def test_three_adamw_steps_of_the_trainer_end_at_the_same_parameters(monkeypatch):
    loss1, par1, text1 = trainer_run(monkeypatch, ["--train-passes", "1"])
    lossh, parh, texth = trainer_run(monkeypatch, ["--train-rows", "hi", "--train-passes", "1"])
    assert SWITCH + "=hi" in texth and SWITCH not in text1 and "D3DP_TRAIN_PASSES=1" in text1
    assert len(loss1) == len(lossh) == RUN_STEPS and loss1 == lossh, (loss1, lossh)
    bad = [n for n in par1 if not torch.equal(par1[n], parh[n])]
    assert not bad, bad[:8]
