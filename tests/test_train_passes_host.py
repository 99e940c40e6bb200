"""No GPU needed: what d3dp_create answers to D3DP_TRAIN_PASSES (the opt-in one-pass fp16 training Linears) is decided before the
device is looked for, so a machine without one sees every refusal -- the switch is never ignored -- and sees the contexts the switch
takes get as far as the device check; what MixSTE2.train_arithmetic() and the command line say about the route; that the CPU
emulation of the route (tests/train_passes_emu.py) rounds what the kernels round and nothing else; and that every case of
tests/test_hip_train_passes.py is admissible: the emulation under a second accumulation order stays within oracle/lowp_check.py's
(1.15, 2.0) x of the first, so (1.5, 4) x the emulation's own error is a bound on the kernels and not on chance."""
import os

import pytest
import torch
import torch.nn.functional as F

import train_passes_emu as emu
from create_host import D3DP_ENOTSUP, create, reached_the_device_check
from d3dp_amd import _lib, cli
from oracle import grad_check as gc
from oracle import lowp_check as lc
from test_hip_train_grads import DROPPED_PARAMS, problem
from test_train_widths_host import arithmetic

SWITCH = emu.SWITCH
_ALL = ("D3DP_TRAIN_PASSES", "D3DP_TRAIN_IMPL", "D3DP_TRAIN_ATTN", "D3DP_TRAIN_ATTN_BWD", "D3DP_TRAIN_OVERLAP", "D3DP_TRAIN_WGRAD",
        "D3DP_TRAIN_TAIL", "D3DP_TRAIN_GELU", "D3DP_TRAIN_LN_OPERAND", "D3DP_EXACT_IMPL", "D3DP_FAST_IMPL", "D3DP_LONG_ATTN")


def env(monkeypatch, **kw):
    for k in _ALL:
        monkeypatch.delenv(k, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv("D3DP_" + k, v)


# ---------------------------------------------------------------------------------------------- refusals and non-refusals
@pytest.mark.parametrize("cs", [64, 128, 256, 512])
@pytest.mark.parametrize("value", [None, "3", "1"])
def test_the_switch_passes_at_the_instantiated_widths(monkeypatch, cs, value):
    env(monkeypatch, **({"TRAIN_PASSES": value} if value else {}))
    assert reached_the_device_check(*create(cs, _lib.MODE_TRAIN))


@pytest.mark.parametrize("cs", [192, 320, 384, 448])
def test_the_switch_passes_at_the_opted_in_widths(monkeypatch, cs):
    env(monkeypatch, TRAIN_PASSES="1", TRAIN_IMPL="f16x2")
    assert reached_the_device_check(*create(cs, _lib.MODE_TRAIN))


@pytest.mark.parametrize("cs,impl", [(512, "f32"), (128, "f32"), (384, None), (96, None), (384, "f32")])
def test_one_pass_is_refused_on_the_fp32_path(monkeypatch, cs, impl):
    """(On the parent `=1` beside D3DP_TRAIN_IMPL=f32, or at a width that trains on the fp32 path, was accepted silently.)"""
    env(monkeypatch, TRAIN_PASSES="1", **({"TRAIN_IMPL": impl} if impl else {}))
    rc, msg = create(cs, _lib.MODE_TRAIN)
    assert rc == D3DP_ENOTSUP and SWITCH + "=1" in msg and "fp32 path" in msg and f"channels={cs}" in msg, (rc, msg)
    env(monkeypatch, TRAIN_PASSES="3", **({"TRAIN_IMPL": impl} if impl else {}))         # (the default's name is no request)
    assert reached_the_device_check(*create(cs, _lib.MODE_TRAIN))


@pytest.mark.parametrize("other", [("TRAIN_WGRAD", "each"), ("TRAIN_TAIL", "split"), ("TRAIN_GELU", "pass"), ("TRAIN_LN_OPERAND", "pass")])
def test_one_pass_is_refused_beside_the_superseded_launch_forms(monkeypatch, other):
    env(monkeypatch, TRAIN_PASSES="1", **{other[0]: other[1]})
    rc, msg = create(512, _lib.MODE_TRAIN)
    assert rc == D3DP_ENOTSUP and SWITCH + "=1" in msg and f"D3DP_{other[0]}={other[1]}" in msg, (rc, msg)


@pytest.mark.parametrize("value", ["2", "0", "", "one", "11", "1 ", "3x"])
def test_any_other_value_is_refused_by_name(monkeypatch, value):
    """(On the parent `=2` was accepted silently.)"""
    env(monkeypatch, TRAIN_PASSES=value)
    for cs in (512, 96):
        rc, msg = create(cs, _lib.MODE_TRAIN)
        assert rc == D3DP_ENOTSUP and f"{SWITCH}={value}" in msg, (rc, msg)


@pytest.mark.parametrize("value", ["1", "2"])
def test_contexts_of_other_modes_do_not_read_the_switch(monkeypatch, value):
    """The reference keeps a train model and two eval models in one process."""
    env(monkeypatch, TRAIN_PASSES=value)
    for mode in (_lib.MODE_EXACT, _lib.MODE_FAST, _lib.MODE_FAST16):
        assert reached_the_device_check(*create(512, mode))
    assert reached_the_device_check(*create(96, _lib.MODE_EXACT))
    rc, msg = create(384, _lib.MODE_FAST)
    assert rc == D3DP_ENOTSUP and SWITCH not in msg, (rc, msg)


@pytest.mark.parametrize("other", [("TRAIN_ATTN", "f32"), ("TRAIN_ATTN", "x2t"), ("TRAIN_ATTN_BWD", "valu"), ("TRAIN_OVERLAP", "0"),
                                   ("TRAIN_OVERLAP", "1")])
def test_the_attention_and_stream_switches_compose_with_it(monkeypatch, other):
    env(monkeypatch, TRAIN_PASSES="1", **{other[0]: other[1]})
    assert reached_the_device_check(*create(512, _lib.MODE_TRAIN))


# ---------------------------------------------------------------------------------------------- Python and command line
def test_train_arithmetic_names_the_route(monkeypatch):
    env(monkeypatch)
    plain512, plain384 = arithmetic(512), arithmetic(384)
    assert SWITCH not in plain512 and "three fp16-MFMA passes" in plain512
    env(monkeypatch, TRAIN_PASSES="3")
    assert arithmetic(512) == plain512
    env(monkeypatch, TRAIN_PASSES="1")
    text = arithmetic(512)
    assert SWITCH + "=1" in text and "one fp16-MFMA pass" in text and "three fp16-MFMA passes" not in text, text
    assert "attention of both axes, forward and backward, on split-fp16 operands" in text
    assert arithmetic(384) == plain384 and SWITCH not in plain384             # (the fp32 path: no such route there)
    env(monkeypatch, TRAIN_PASSES="1", TRAIN_IMPL="f16x2")
    text = arithmetic(384)
    assert SWITCH + "=1" in text and "one fp16-MFMA pass" in text and "D3DP_TRAIN_IMPL=f16x2" in text, text
    env(monkeypatch, TRAIN_PASSES="1", TRAIN_IMPL="f32")
    assert SWITCH not in arithmetic(512)


def test_the_text_without_the_switch_is_the_text_of_before(monkeypatch):
    env(monkeypatch)
    assert arithmetic(512).startswith("split-fp16 Linears (three fp16-MFMA passes, fp32 accumulate, device-side operand scales; forward "
                                      "and dgrad on 256 x 128 tiles")
    env(monkeypatch, TRAIN_IMPL="f16x2")
    assert "(cs = 384): split-fp16 Linears (three fp16-MFMA passes, fp32 accumulate, device-side operand scales; an operand pass in "\
           "front of every Linear" in arithmetic(384)


@pytest.mark.parametrize("before", [None, "3", "junk"])
def test_the_cli_flag_parses_and_leaves_the_environment_as_it_found_it(monkeypatch, before):
    env(monkeypatch, **({"TRAIN_PASSES": before} if before is not None else {}))
    assert cli.parse_args([]).train_passes is None
    assert cli.parse_args(["--train-passes", "1"]).train_passes == 1 and cli.parse_args(["--train-passes", "3"]).train_passes == 3
    with pytest.raises(SystemExit):
        cli.parse_args(["--train-passes", "2"])
    for passes in (1, 3):
        with cli.train_passes_env(passes):
            assert os.environ[SWITCH] == str(passes)
        assert os.environ.get(SWITCH) == before
    with pytest.raises(RuntimeError):
        with cli.train_passes_env(1):
            raise RuntimeError("the creation of the context failed")
    assert os.environ.get(SWITCH) == before
    with cli.train_passes_env(None):
        assert os.environ.get(SWITCH) == before


# ---------------------------------------------------------------------------------------------- the emulation checks itself
def test_the_emulated_linears_are_the_ones_the_step_sends_through_x2train():
    assert emu.x2_linears() == ("fc1", "fc2", "proj", "qkv")
    case = emu.STEP_CASES[2]
    sd, x2d, gt, t, noise, dpd = problem(case)
    with emu.one_pass_linears() as calls:
        gc.reference_grads(sd, x2d, gt, t, noise, case.dep, dpd, torch.float32)
    C = case.cs
    on, off = sorted((n, k) for n, k, e in calls if e), sorted((n, k) for n, k, e in calls if not e)
    assert on == sorted([(3 * C, C), (C, C), (2 * C, C), (C, 2 * C)] * 2 * case.dep), on
    assert off == sorted([(C, 5), (2 * C, C), (C, 2 * C), (3, C)]), off         # embedding, the two time-MLP Linears, head
    assert F.linear is torch.nn.functional.linear and F.linear.__name__ == "linear" and "one_pass" not in repr(F.linear)
    with emu.one_pass_linears():                                                # fp64 runs are left alone
        x, w = torch.randn(3, 4, 64, dtype=torch.float64), torch.randn(64, 64, dtype=torch.float64)
        assert torch.equal(F.linear(x, w), x @ w.t())


def test_the_rounding_is_fp16_at_the_scale_of_the_absmax():
    g = torch.Generator().manual_seed(3)
    for mag in (1e-30, 3e-5, 1.0, 0.75, 1000.0, 3e20):
        x = torch.randn(64, 96, generator=g) * mag
        s = emu.dyn_scale(x)
        top = float(x.abs().max()) * s
        assert 2.0 ** 13 <= top < 2.0 ** 14 and s == 2.0 ** round(torch.log2(torch.tensor(s)).item()), (mag, s, top)
        r = emu.r16(x)
        assert torch.equal(emu.r16(r), r)                                       # idempotent: the scale does not move
        rel = ((r - x).abs() / x.abs().clamp_min(1e-38))[x.abs() * s >= 2.0 ** -14]
        assert float(rel.max()) <= 2.0 ** -11                                   # half an ulp of an 11-bit significand
        assert torch.equal(r, ((x * s).half().float() / s))
    assert emu.dyn_scale(torch.zeros(4)) == 1.0 and torch.equal(emu.r16(torch.zeros(4, 4)), torch.zeros(4, 4))
    x = torch.tensor([1.0, 1.0 + 2.0 ** -11 + 2.0 ** -20, -(1.0 - 2.0 ** -12 - 2.0 ** -20), 2.0 ** -40])
    assert torch.equal(emu.r16(x), torch.tensor([1.0, 1.0 + 2.0 ** -10, -(1.0 - 2.0 ** -11), 0.0]))   # (2^-40 2^13: below half the smallest subnormal)


def test_the_function_rounds_both_operands_of_all_three_products_and_dy_once():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 40, 64, generator=g).requires_grad_(True)
    w = (torch.randn(192, 64, generator=g) / 8).requires_grad_(True)
    b = torch.randn(192, generator=g).requires_grad_(True)
    up = torch.randn(2, 40, 192, generator=g)
    with emu.one_pass_linears() as calls:
        y = F.linear(x, w, b)
    y.backward(up)
    assert calls == [(192, 64, True)]
    xr, wr, ur = emu.r16(x.detach()).double(), emu.r16(w.detach()).double(), emu.r16(up).double()
    tol = dict(rtol=0, atol=2e-5)
    assert torch.allclose(y.detach().double(), xr @ wr.t() + b.detach().double(), **tol)
    assert torch.allclose(x.grad.double(), ur @ wr, **tol)
    assert torch.allclose(w.grad.double(), ur.reshape(-1, 192).t() @ xr.reshape(-1, 64), rtol=0, atol=2e-4)
    assert torch.allclose(b.grad.double(), up.double().reshape(-1, 192).sum(0), rtol=0, atol=2e-4)          # the UNROUNDED dY
    assert not torch.allclose(y.detach(), F.linear(x.detach(), w.detach(), b.detach()), rtol=0, atol=1e-5)  # ... and it is not fp32


# ---------------------------------------------------------------------------------------------- admissibility of the GPU cases
@pytest.mark.parametrize("case", emu.ALL_CASES, ids=lambda c: c.id)
def test_every_gpu_case_is_admissible(case):
    r = emu.step_refs(case)
    print(f"{case.id}: e32 ({r.e32[0]:.2e}, {r.e32[1]:.2e}), one-pass emulation ({r.e1p[0]:.2e}, {r.e1p[1]:.2e}) = "
          f"({r.e1p[0] / r.e32[0]:.0f}, {r.e1p[1] / r.e32[1]:.0f}) x e32, second accumulation order ({r.spread[0]:.3f}, {r.spread[1]:.3f}) x")
    assert gc.admissible(r.e32), r.e32
    assert lc.admissible(r.spread), r.spread
    # the gate "the route exceeds 8 x e32 in the norm" can tell the routes apart only where a correct one-pass step does
    assert r.e1p[0] > 2 * gc.FACTOR * r.e32[0], (r.e1p, r.e32)
    zeros = sorted(n for n, g in r.g64.items() if not g.any())
    assert zeros == (sorted(DROPPED_PARAMS) if case is emu.DROPPED_CASE else []), zeros


def test_the_short_run_falls_in_both_arithmetics_on_the_cpu():
    plain, one = emu.oracle_runs()
    n = emu.RUN_BATCHES
    print(f"20 AdamW steps, oracle: fp32 {plain[0]:.5f} -> {plain[-1]:.5f}, one-pass emulation {one[0]:.5f} -> {one[-1]:.5f}, "
          f"final-loss difference {abs(one[-1] - plain[-1]):.3e}")
    for losses in (plain, one):
        assert len(losses) == emu.RUN_STEPS and sum(losses[-n:]) < sum(losses[:n])
    assert one[-1] != plain[-1]
