"""D3DP_TRAIN_ATTN_PASSES (the opt-in one-pass fp16 training attention) as far as a CPU can check it (no GPU needed): what
plan_context() of d3dp_amd/csrc/ctx_plan.h and plan_train_step() of train_plan.h decide under the switch -- through a stand-alone
driver, tests/train_attn_passes_driver.cpp, which prints the new members --, what d3dp_create of the real library answers before it
looks for a device, what MixSTE2.train_arithmetic() and the command line say about the route, that the CPU emulation of the route
(tests/train_attn_passes_emu.py) rounds what the kernels round, and that every case of tests/test_hip_train_attn_passes.py is
admissible: the emulation under a second accumulation order stays within oracle/lowp_check.py's window of the first, so
(lc.NORM16, lc.MAX16) x the emulation's own error is a bound on the kernels and not on chance, and the emulation lies at least
32 x the fp32 oracle's error from fp64 in the norm, so the GPU file's lower bound of 8 x tells the routes apart.

e32 is the error of the fp32 oracle as the CPU's BLAS computes it, so it moves with the CPU (not with the thread count from 4 up).
Measured, emulation over e32 in the norm, the seven step cases in their order: 140, 121, 138, 122, 96, 222, 141 x on the CPU this was
written on; 162, 59, 49, 131, 24, 168, 36 x on a CPU whose fp32 oracle is 3 - 4 x less accurate in the long cases (e32 1.51e-6
instead of 3.83e-7 at cs 256, F 300): there test_every_gpu_case_is_admissible[cs256-F300-B2] reads 24 x and misses the 32 x this file
asks for, while the GPU file's own bound (8 x the e32 of the machine it runs on) holds with the figures above."""
import os
import shutil
import subprocess

import pytest
import torch

import train_attn_passes_emu as emu
import train_passes_emu as lin_emu
from create_host import D3DP_ENOTSUP, create, reached_the_device_check
from d3dp_amd import _lib, cli
from oracle import d3dp_oracle as orc
from oracle import grad_check as gc
from oracle import lowp_check as lc
from test_hip_train_grads import DROPPED_PARAMS, problem
from test_train_widths_host import arithmetic

SWITCH = emu.SWITCH
EXACT, FAST, TRAIN, FAST16 = 0, 1, 2, 3
OK, ENOTSUP = 0, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ALL = ("D3DP_TRAIN_PASSES", "D3DP_TRAIN_IMPL", "D3DP_TRAIN_ATTN", "D3DP_TRAIN_ATTN_BWD", "D3DP_TRAIN_OVERLAP", "D3DP_TRAIN_WGRAD",
        "D3DP_TRAIN_TAIL", "D3DP_TRAIN_GELU", "D3DP_TRAIN_LN_OPERAND", "D3DP_TRAIN_LONG_ATTN", "D3DP_EXACT_IMPL", "D3DP_FAST_IMPL",
        "D3DP_LONG_ATTN", SWITCH)
COMPOSING = [("TRAIN_PASSES", "1"), ("TRAIN_OVERLAP", "0"), ("TRAIN_OVERLAP", "1"), ("TRAIN_LONG_ATTN", "chunked"), ("TRAIN_ATTN_BWD", "valu")]
SEPARATES = 32.0          # the emulation's norm error over the fp32 oracle's, at least (measured: 96 ... 260 x)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("train_attn_passes") / "driver")
    subprocess.run(["g++", "-std=c++17", os.path.join(ROOT, "tests", "train_attn_passes_driver.cpp"), "-o", exe], check=True)
    return exe


def case(mode, cs, frames=9, joints=17, heads=8, **env):
    """One line of the driver's input; env: the switches without their D3DP_ prefix."""
    fields = [mode, cs, heads, 2 * cs, frames, joints, 0]
    return "\t".join([str(f) for f in fields] + [f"D3DP_{k}={v}" for k, v in env.items()])


def plans(driver, *cases, step=False):
    """-> [(return code, message, {member: value})], one per case, from one run of the driver."""
    clean = {k: v for k, v in os.environ.items() if not k.startswith("D3DP_")}
    out = subprocess.run([driver] + (["step"] if step else []), input="".join(c + "\n" for c in cases), env=clean, capture_output=True,
                         text=True, check=True).stdout
    rows = [line.split("\t") for line in out.split("\n")[:-1]]
    assert len(rows) == len(cases), out
    return [(int(r[0]), r[1], {k: int(v) for k, v in (f.split("=") for f in r[2:])}) for r in rows]


def plan(driver, *a, **kw):
    (rc, msg, p), = plans(driver, case(*a, **kw))
    assert rc == OK and msg == "", (a, kw, rc, msg)
    return p


def refusal(driver, *a, **kw):
    (rc, msg, p), = plans(driver, case(*a, **kw))
    assert rc != OK and msg and p["train_attn_passes"] == 3, (a, kw, p)      # (a refusal leaves the caller's plan alone)
    return rc, msg


def env(monkeypatch, **kw):
    for k in _ALL:
        monkeypatch.delenv(k, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv("D3DP_" + k, v)


# ---------------------------------------------------------------------------------------------- accepted routes
@pytest.mark.parametrize("cs", [512, 256, 128])
def test_one_pass_plans_alone_and_beside_every_composing_switch(driver, cs):
    default = plan(driver, TRAIN, cs)
    assert default["train_attn_passes"] == 3
    p = plan(driver, TRAIN, cs, TRAIN_ATTN_PASSES="1")
    assert p == {**default, "train_attn_passes": 1}, p
    for name, value in COMPOSING:
        alone = plan(driver, TRAIN, cs, **{name: value})
        assert alone["train_attn_passes"] == 3
        assert plan(driver, TRAIN, cs, TRAIN_ATTN_PASSES="1", **{name: value}) == {**alone, "train_attn_passes": 1}, (name, value)
    x2t = plan(driver, TRAIN, cs, TRAIN_ATTN_PASSES="1", TRAIN_ATTN="x2t")
    assert x2t["train_attn_passes"] == 1 and x2t["train_attn_x2"] == 1, x2t
    assert plan(driver, TRAIN, cs, frames=520, TRAIN_ATTN_PASSES="1")["train_attn_passes"] == 1


def test_unset_or_three_is_the_default_plan_in_every_mode(driver):
    shapes = [(TRAIN, 512), (TRAIN, 64), (TRAIN, 96), (TRAIN, 384), (EXACT, 512), (EXACT, 96), (FAST, 512), (FAST16, 256)]
    for mode, cs in shapes:
        (rc0, msg0, p0), (rc3, msg3, p3) = plans(driver, case(mode, cs), case(mode, cs, TRAIN_ATTN_PASSES="3"))
        assert (rc0, msg0) == (OK, "") and (rc3, msg3, p3) == (rc0, msg0, p0) and p0["train_attn_passes"] == 3, (mode, cs, msg3)
    for impl in ("f32", "f16x2"):                                   # (the default's name is no request: nothing to refuse)
        cs = 512 if impl == "f32" else 384
        assert plan(driver, TRAIN, cs, TRAIN_ATTN_PASSES="3", TRAIN_IMPL=impl) == plan(driver, TRAIN, cs, TRAIN_IMPL=impl)


@pytest.mark.parametrize("value", ["1", "2", "junk"])
def test_contexts_of_other_modes_do_not_read_the_switch(driver, value):
    for mode, cs in ((EXACT, 512), (FAST, 512), (FAST16, 512), (EXACT, 96), (EXACT, 64)):
        (rc, msg, p), (rc0, msg0, p0) = plans(driver, case(mode, cs, TRAIN_ATTN_PASSES=value), case(mode, cs))
        assert (rc, msg, p) == (rc0, msg0, p0) and rc == OK and p["train_attn_passes"] == 3, (mode, cs, msg)
    (rc, msg, _), = plans(driver, case(FAST, 384, TRAIN_ATTN_PASSES=value))
    assert rc == ENOTSUP and SWITCH not in msg, msg


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("value", ["2", "0", "", "one", "11", "1 ", "3x"])
def test_any_other_value_is_refused_by_name(driver, value):
    for cs in (512, 64, 96):
        rc, msg = refusal(driver, TRAIN, cs, TRAIN_ATTN_PASSES=value)
        assert rc == ENOTSUP and f"{SWITCH}={value}" in msg, msg


@pytest.mark.parametrize("cs,impl", [(512, "f32"), (128, "f32"), (384, None), (96, None), (384, "f32")])
def test_one_pass_is_refused_on_the_fp32_path(driver, cs, impl):
    rc, msg = refusal(driver, TRAIN, cs, TRAIN_ATTN_PASSES="1", **({"TRAIN_IMPL": impl} if impl else {}))
    assert rc == ENOTSUP and SWITCH + "=1" in msg and "fp32 path" in msg and f"channels={cs}" in msg, msg
    assert ("D3DP_TRAIN_IMPL=f32" in msg) == (impl == "f32"), msg


def test_one_pass_is_refused_at_head_dim_8_and_beside_fp32_attention(driver):
    rc, msg = refusal(driver, TRAIN, 64, TRAIN_ATTN_PASSES="1")
    assert rc == ENOTSUP and SWITCH + "=1" in msg and "head dim 8" in msg, msg
    rc, msg = refusal(driver, TRAIN, 128, heads=16, TRAIN_ATTN_PASSES="1")
    assert rc == ENOTSUP and SWITCH + "=1" in msg and "head dim 8" in msg, msg
    for cs in (512, 256, 128):
        rc, msg = refusal(driver, TRAIN, cs, TRAIN_ATTN_PASSES="1", TRAIN_ATTN="f32")
        assert rc == ENOTSUP and SWITCH + "=1" in msg and "D3DP_TRAIN_ATTN=f32" in msg, msg


@pytest.mark.parametrize("cs,hd", [(192, 24), (320, 40), (384, 48), (448, 56)])
def test_one_pass_is_refused_at_the_padded_head_dims(driver, cs, hd):
    rc, msg = refusal(driver, TRAIN, cs, TRAIN_ATTN_PASSES="1", TRAIN_IMPL="f16x2")
    assert rc == ENOTSUP and SWITCH + "=1" in msg and f"head dim {hd}" in msg and "padded" in msg, msg
    assert plan(driver, TRAIN, cs, TRAIN_IMPL="f16x2")["train_attn_passes"] == 3


def test_the_earlier_refusals_keep_their_place_and_text(driver):
    """Steps 1 ... 7 of plan_context answer first, word for word as without the switch; steps 8 ... 10 answer behind it."""
    earlier = [dict(cs=512, frames=2000), dict(cs=500, heads=7), dict(cs=96, frames=351), dict(cs=200, TRAIN_IMPL="f16x2"),
               dict(cs=512, TRAIN_LONG_ATTN="rows"), dict(cs=512, TRAIN_PASSES="2"), dict(cs=512, TRAIN_PASSES="1", TRAIN_IMPL="f32"),
               dict(cs=512, TRAIN_PASSES="1", TRAIN_WGRAD="each")]
    for kw in earlier:
        kw = dict(kw)
        cs = kw.pop("cs")
        without = refusal(driver, TRAIN, cs, **kw)
        for value in ("1", "2"):
            assert refusal(driver, TRAIN, cs, TRAIN_ATTN_PASSES=value, **kw) == without, (kw, value)
        assert SWITCH not in without[1]
    for kw in (dict(cs=96, EXACT_IMPL="bf16x3"), dict(cs=512, TRAIN_WGRAD="each"), dict(cs=512, X2_SKEW="2")):
        kw = dict(kw)
        cs = kw.pop("cs")
        assert SWITCH not in refusal(driver, TRAIN, cs, **kw)[1]
        assert SWITCH + "=2" in refusal(driver, TRAIN, cs, TRAIN_ATTN_PASSES="2", **kw)[1]


def test_the_real_library_answers_the_same_before_it_looks_for_a_device(monkeypatch):
    for cs in (512, 256, 128):
        for value in (None, "3", "1"):
            env(monkeypatch, **({"TRAIN_ATTN_PASSES": value} if value else {}))
            assert reached_the_device_check(*create(cs, _lib.MODE_TRAIN))
        for name, value in COMPOSING + [("TRAIN_ATTN", "x2t")]:
            env(monkeypatch, TRAIN_ATTN_PASSES="1", **{name: value})
            assert reached_the_device_check(*create(cs, _lib.MODE_TRAIN)), (name, value)
    refused = [(512, dict(TRAIN_ATTN_PASSES="2"), "=2"), (512, dict(TRAIN_ATTN_PASSES="1", TRAIN_IMPL="f32"), "fp32 path"),
               (96, dict(TRAIN_ATTN_PASSES="1"), "fp32 path"), (64, dict(TRAIN_ATTN_PASSES="1"), "head dim 8"),
               (256, dict(TRAIN_ATTN_PASSES="1", TRAIN_ATTN="f32"), "D3DP_TRAIN_ATTN=f32"),
               (384, dict(TRAIN_ATTN_PASSES="1", TRAIN_IMPL="f16x2"), "head dim 48")]
    for cs, kw, words in refused:
        env(monkeypatch, **kw)
        rc, msg = create(cs, _lib.MODE_TRAIN)
        assert rc == D3DP_ENOTSUP and SWITCH in msg and words in msg, (cs, kw, rc, msg)
        for mode in (_lib.MODE_EXACT, _lib.MODE_FAST, _lib.MODE_FAST16):
            if cs in (512, 256, 64):
                assert reached_the_device_check(*create(cs, mode)), (cs, kw, mode)


# ---------------------------------------------------------------------------------------------- the step's plan
def test_the_training_step_plan_carries_the_pass_count(driver):
    rows = plans(driver, case(TRAIN, 512), case(TRAIN, 512, TRAIN_ATTN_PASSES="1"), case(TRAIN, 256, TRAIN_ATTN_PASSES="1", TRAIN_PASSES="1"),
                 case(TRAIN, 128, TRAIN_ATTN_PASSES="1", TRAIN_ATTN="x2t"), case(TRAIN, 512, TRAIN_PASSES="1"),
                 case(TRAIN, 512, TRAIN_ATTN_PASSES="3"), step=True)
    assert all(rc == OK for rc, _, _ in rows), rows
    (_, _, d), (_, _, one), (_, _, both), (_, _, x2t), (_, _, lin), (_, _, three) = rows
    assert d["attn_passes"] == 3 and d["passes"] == 3 and three == d
    assert one == {**d, "attn_passes": 1}                            # nothing else of the step moves
    assert both["attn_passes"] == 1 and both["passes"] == 1 and both["attn_x2_s"] == 1 and both["attn_x2_t"] == 1
    assert x2t["attn_passes"] == 1 and x2t["attn_x2_s"] == 0 and x2t["attn_x2_t"] == 1      # the temporal axis alone
    assert lin["attn_passes"] == 3 and lin["passes"] == 1


# ---------------------------------------------------------------------------------------------- Python and command line
def test_train_arithmetic_names_the_route_behind_its_unchanged_text(monkeypatch):
    env(monkeypatch)
    plain512, plain64, plain384 = arithmetic(512), arithmetic(64), arithmetic(384)
    assert SWITCH not in plain512
    env(monkeypatch, TRAIN_ATTN_PASSES="3")
    assert arithmetic(512) == plain512
    env(monkeypatch, TRAIN_ATTN_PASSES="1")
    text = arithmetic(512)
    assert text.startswith(plain512 + "; " + SWITCH + "=1: ") and "one fp16-MFMA pass" in text and "attention of both axes" in text[len(plain512):], text
    assert arithmetic(64) == plain64 and arithmetic(384) == plain384          # (refused there: no such route to name)
    env(monkeypatch, TRAIN_ATTN_PASSES="1", TRAIN_ATTN="x2t")
    tail = arithmetic(256).split(SWITCH + "=1: ")[1]
    assert "temporal attention" in tail and "both axes" not in tail, tail
    env(monkeypatch, TRAIN_ATTN_PASSES="1", TRAIN_PASSES="1")
    text = arithmetic(512)
    assert "D3DP_TRAIN_PASSES=1" in text and SWITCH + "=1" in text
    for kw in (dict(TRAIN_IMPL="f32"), dict(TRAIN_ATTN="f32")):
        env(monkeypatch, TRAIN_ATTN_PASSES="1", **kw)
        assert SWITCH not in arithmetic(512)
    env(monkeypatch, TRAIN_ATTN_PASSES="1", TRAIN_IMPL="f16x2")
    assert SWITCH not in arithmetic(384)


@pytest.mark.parametrize("before", [None, "3", "junk"])
def test_the_cli_flag_parses_and_leaves_the_environment_as_it_found_it(monkeypatch, before):
    env(monkeypatch, **({"TRAIN_ATTN_PASSES": before} if before is not None else {}))
    assert cli.parse_args([]).train_attn_passes is None
    assert cli.parse_args(["--train-attn-passes", "1"]).train_attn_passes == 1
    assert cli.parse_args(["--train-attn-passes", "3", "--train-passes", "1"]).train_attn_passes == 3
    with pytest.raises(SystemExit):
        cli.parse_args(["--train-attn-passes", "2"])
    for passes in (1, 3):
        with cli.train_attn_passes_env(passes):
            assert os.environ[SWITCH] == str(passes)
        assert os.environ.get(SWITCH) == before
    with pytest.raises(RuntimeError):
        with cli.train_attn_passes_env(1):
            raise RuntimeError("the creation of the context failed")
    assert os.environ.get(SWITCH) == before
    with cli.train_attn_passes_env(None):
        assert os.environ.get(SWITCH) == before


# ---------------------------------------------------------------------------------------------- the emulation checks itself
def test_the_emulation_replaces_the_attention_of_fp32_runs_at_the_kernels_head_dims():
    plain = orc.attention
    c = emu.STEP_CASES[5]
    sd, x2d, gt, t, noise, dpd = problem(c)
    with emu.one_pass_attention() as calls, lin_emu.one_pass_linears() as lins:
        gc.reference_grads(sd, x2d, gt, t, noise, c.dep, dpd, torch.float32)
    assert sorted(calls) == sorted([(f"{k}blocks.{i}.", True) for k in ("STE", "TTE") for i in range(c.dep)]), calls
    assert sum(e for _, _, e in lins) == 4 * 2 * c.dep                # nested: the qkv and proj Linears go through the Linear emulation
    with emu.one_pass_attention(axes="t") as calls:
        gc.reference_grads(sd, x2d, gt, t, noise, c.dep, dpd, torch.float32)
    assert all(e == pre.startswith("TTE") for pre, e in calls) and len(calls) == 2 * c.dep, calls
    with emu.one_pass_attention() as calls:                             # fp64 runs and head dim 8 are left alone
        gc.reference_grads(sd, x2d, gt, t, noise, c.dep, dpd, torch.float64)
        sd8, x8, g8, t8, n8, d8 = problem(emu.Case(64, 9, 2))
        gc.reference_grads(sd8, x8, g8, t8, n8, 2, d8, torch.float32)
    assert not any(e for _, e in calls), calls
    assert orc.attention is plain


def test_the_function_rounds_what_the_kernels_round():
    g = torch.Generator().manual_seed(7)
    S, N, heads, hd = 3, 21, 8, 16
    C = heads * hd
    qkv = torch.randn(S, N, 3 * C, generator=g).requires_grad_(True)
    up = torch.randn(S, N, C, generator=g) * 1e-3
    o = emu._OnePassAttention.apply(qkv, heads, False)
    o.backward(up)
    # the model in fp64 from the same rounded operands
    r = lambda x: emu.r16_at(x, lin_emu.dyn_scale(x)).double()
    q, k, v = (emu._heads(t, heads) for t in r(qkv.detach()).split(C, dim=-1))
    s = q @ k.transpose(-1, -2) * hd ** -0.5
    p = torch.softmax(s, dim=-1)
    pu = torch.exp(s - s.amax(-1, keepdim=True))
    want_o = (emu.r16_at(pu.float(), 1024.0).double() @ v / pu.sum(-1, keepdim=True)).transpose(1, 2).reshape(S, N, C)
    err_o = (o.detach().double() - want_o).abs().max() / want_o.abs().max()
    assert err_o < 2e-3, err_o                    # (an fp32 exponential one ulp away can move a rounding of P: half an fp16 ulp, 2^-11)
    go = emu._heads(r(up), heads)
    D = emu._heads(up.double() * o.detach().double(), heads).sum(-1, keepdim=True)
    ds = p * (go @ v.transpose(-1, -2) - D) * hd ** -0.5
    dsq = emu.r16_at(ds.float(), emu.pow2_scale(ds.float().abs().amax(-1, keepdim=True))).double()
    dsk = emu.r16_at(ds.float(), emu.pow2_scale(ds.float().abs().amax(-2, keepdim=True))).double()
    pr = emu.r16_at(p.float(), 1024.0).double()
    back = lambda t: t.transpose(1, 2).reshape(S, N, C)
    want = torch.cat([back(dsq @ k), back(dsk.transpose(-1, -2) @ q), back(pr.transpose(-1, -2) @ go)], dim=-1)
    err = (qkv.grad.double() - want).abs().max() / want.abs().max()
    assert err < 2e-3, err                        # (an fp32 logit one ulp away can move a rounding of P or dS: half an fp16 ulp, 2^-11)
    exact = torch.autograd.functional.vjp(lambda x: _plain(x, heads), qkv.detach().double(), up.double())[1]
    gap = (qkv.grad.double() - exact).abs().max() / exact.abs().max()
    assert 1e-5 < gap < 1e-2, gap                  # ... and it is not the fp32 attention
    # scales: the absmax lands in [2^13, 2^14); zero stays zero
    m = torch.tensor([0.0, 1.0, 0.75, 3e-20, 5e4])
    sc = emu.pow2_scale(m)
    assert sc[0] == 1.0 and all(2.0 ** 13 <= float(a * b) < 2.0 ** 14 for a, b in zip(m[1:], sc[1:]))
    assert float(sc[1]) == lin_emu.dyn_scale(torch.tensor([1.0])) and float(sc[4]) == lin_emu.dyn_scale(torch.tensor([5e4]))


def _plain(qkv, heads):
    S, N, C3 = qkv.shape
    C = C3 // 3
    q, k, v = (emu._heads(t, heads) for t in qkv.split(C, dim=-1))
    a = torch.softmax(q @ k.transpose(-1, -2) * (C // heads) ** -0.5, dim=-1)
    return (a @ v).transpose(1, 2).reshape(S, N, C)


# ---------------------------------------------------------------------------------------------- admissibility of the GPU cases
ROUTES = ([(c, "both", False) for c in emu.STEP_CASES] + [(emu.DROPPED_CASE, "both", False), (emu.BOTH_CASE, "both", True),
                                                          (emu.X2T_CASE, "t", False)])


@pytest.mark.parametrize("case_,axes,linears", ROUTES, ids=lambda v: v.id if hasattr(v, "id") else str(v))
def test_every_gpu_case_is_admissible(case_, axes, linears):
    b, e, s = emu.base(case_), emu.emulated(case_, axes, linears), emu.spread(case_, axes, linears)
    print(f"{case_.id} axes={axes} linears={linears}: e32 ({b.e32[0]:.2e}, {b.e32[1]:.2e}), emulation ({e[0]:.2e}, {e[1]:.2e}) = "
          f"({e[0] / b.e32[0]:.0f}, {e[1] / b.e32[1]:.0f}) x e32, second accumulation order ({s[0]:.3f}, {s[1]:.3f}) x")
    assert gc.admissible(b.e32), b.e32
    assert lc.admissible(s), s
    assert e[0] >= SEPARATES * b.e32[0], (e, b.e32)
    assert SEPARATES > 2 * gc.FACTOR
    zeros = sorted(n for n, g in b.g64.items() if not g.any())
    assert zeros == (sorted(DROPPED_PARAMS) if case_ is emu.DROPPED_CASE else []), zeros


def test_beside_the_one_pass_linears_the_attention_costs_no_measurable_accuracy():
    c = emu.BOTH_CASE
    both, lin = emu.emulated(c, "both", True), lin_emu.step_refs(c).e1p
    print(f"{c.id}: Linears alone ({lin[0]:.2e}, {lin[1]:.2e}), both ({both[0]:.2e}, {both[1]:.2e})")
    assert both[0] < lc.NORM16 * lin[0] and both[1] < lc.MAX16 * lin[1], (both, lin)
