"""D3DP_TRAIN_LONG_ATTN=chunked as far as a CPU can check it (no GPU needed): what plan_context() of d3dp_amd/csrc/ctx_plan.h decides
under the switch -- through a stand-alone driver, tests/train_long_driver.cpp, which prints the new CtxPlan member --, what
MixSTE2.train_arithmetic() and the command line say about it, and that every case tests/test_hip_train_long.py compares with the
fp64 oracle is admissible in the sense of oracle/grad_check.py."""
import os
import shutil
import subprocess

import pytest

from d3dp_amd import cli
from oracle import grad_check as gc
from test_hip_train_long import DROPPED, DROPPED_PARAMS, FP64_CASES, SWITCH, reference
from test_train_widths_host import arithmetic

EXACT, FAST, TRAIN, FAST16 = 0, 1, 2, 3
OK, ENOTSUP = 0, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ALL = ("D3DP_TRAIN_PASSES", "D3DP_TRAIN_IMPL", "D3DP_TRAIN_ATTN", "D3DP_TRAIN_ATTN_BWD", "D3DP_TRAIN_OVERLAP", "D3DP_TRAIN_WGRAD",
        "D3DP_TRAIN_TAIL", "D3DP_TRAIN_GELU", "D3DP_TRAIN_LN_OPERAND", "D3DP_EXACT_IMPL", "D3DP_FAST_IMPL", "D3DP_LONG_ATTN", SWITCH)
# (cs, frames, joints) of TRAIN contexts that pass with the switch; without it step 6 of plan_context refuses all but (96, 9, 200) --
# 200 tokens of capacity 16 fit the whole-sequence kernels
BEYOND_SHAPES = [(1024, 243, 17), (576, 160, 17), (96, 351, 17), (96, 9, 200), (576, 9, 160)]
REFUSED_WITHOUT = [s for s in BEYOND_SHAPES if s != (96, 9, 200)]
OLD_REFUSAL = ("channels={cs} heads=8 frames={f} joints={j}: training at a width outside {{64,128,256,512}} runs the fp32 attention "
               "backward, which holds a whole sequence in LDS (<= 256 tokens; <= 153 at head dims above 64)")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("train_long") / "driver")
    subprocess.run(["g++", "-std=c++17", os.path.join(ROOT, "tests", "train_long_driver.cpp"), "-o", exe], check=True)
    return exe


def case(mode, cs, frames=9, joints=17, heads=8, **env):
    """One line of the driver's input; env: the switches without their D3DP_ prefix."""
    fields = [mode, cs, heads, 2 * cs, frames, joints, 0]
    return "\t".join([str(f) for f in fields] + [f"D3DP_{k}={v}" for k, v in env.items()])


def plans(driver, *cases):
    """-> [(return code, message, {member: value})], one per case, from one run of the driver."""
    clean = {k: v for k, v in os.environ.items() if not k.startswith("D3DP_")}
    out = subprocess.run([driver], input="".join(c + "\n" for c in cases), env=clean, capture_output=True, text=True, check=True).stdout
    rows = [line.split("\t") for line in out.split("\n")[:-1]]
    assert len(rows) == len(cases), out
    return [(int(r[0]), r[1], {k: int(v) for k, v in (f.split("=") for f in r[2:])}) for r in rows]


def plan(driver, *a, **kw):
    (rc, msg, p), = plans(driver, case(*a, **kw))
    assert rc == OK and msg == "", (a, kw, rc, msg)
    return p


def refusal(driver, *a, **kw):
    (rc, msg, p), = plans(driver, case(*a, **kw))
    assert rc != OK and msg and p["train_long_attn"] == 0, (a, kw, p)        # (a refusal leaves the caller's plan alone)
    return rc, msg


# ---------------------------------------------------------------------------------------------- what the switch lifts
@pytest.mark.parametrize("cs,frames,joints", BEYOND_SHAPES)
def test_train_contexts_beyond_the_token_limit_pass_with_the_switch(driver, cs, frames, joints):
    p = plan(driver, TRAIN, cs, frames, joints, TRAIN_LONG_ATTN="chunked")
    assert p["train_long_attn"] == 1 and p["train_x2"] == 0 and p["exact_impl_req"] == 2, p


@pytest.mark.parametrize("cs,frames,joints", REFUSED_WITHOUT)
def test_without_the_switch_the_refusal_reads_as_before(driver, cs, frames, joints):
    rc, msg = refusal(driver, TRAIN, cs, frames, joints)
    assert rc == ENOTSUP and msg == OLD_REFUSAL.format(cs=cs, f=frames, j=joints), msg


def test_without_the_switch_every_context_plans_as_before(driver):
    for cs, frames in ((512, 243), (64, 300), (96, 243), (384, 27)):
        assert plan(driver, TRAIN, cs, frames)["train_long_attn"] == 0
    # the limits of step 1 and of the fp32 implementation stay, with and without it
    for env in ({}, {"TRAIN_LONG_ATTN": "chunked"}):
        assert refusal(driver, TRAIN, 96, 1025, **env) == (ENOTSUP, "frames=1025 not in [1,1024]")
        assert refusal(driver, TRAIN, 96, 9, 257, **env) == (ENOTSUP, "joints=257 not in [1,256]")
        rc, msg = refusal(driver, TRAIN, 2048, 300, **env)
        assert rc == ENOTSUP and msg.startswith("channels=2048 heads=8 hidden=4096: the fp32 implementation takes channels <= 1024"), msg
    assert plan(driver, TRAIN, 96, 1024, TRAIN_LONG_ATTN="chunked")["train_long_attn"] == 1
    assert plan(driver, TRAIN, 1024, 9, 256, TRAIN_LONG_ATTN="chunked")["train_long_attn"] == 1


def test_the_switch_is_carried_at_every_width(driver):
    """(the instantiated widths: head dim 8 and the cross-check switches run the fp32 attention there; d3dp_train_forward reads it)"""
    for cs in (64, 128, 256, 512, 96, 384, 1024):
        assert plan(driver, TRAIN, cs, 300 if cs in (64, 128, 256, 512) else 27, TRAIN_LONG_ATTN="chunked")["train_long_attn"] == 1


@pytest.mark.parametrize("value", ["", "1", "rows", "Chunked", "chunked ", "chunk", "0"])
def test_any_other_value_is_refused_by_name_in_a_train_context(driver, value):
    for cs, frames in ((512, 27), (96, 27), (96, 351), (64, 300)):
        rc, msg = refusal(driver, TRAIN, cs, frames, TRAIN_LONG_ATTN=value)
        assert rc == ENOTSUP and msg.startswith(f"{SWITCH}={value}: the one value a TRAIN context takes is {SWITCH}=chunked"), msg


@pytest.mark.parametrize("value", ["chunked", "junk", ""])
def test_contexts_of_other_modes_do_not_read_the_switch(driver, value):
    """The reference keeps a train model and two eval models in one process."""
    for mode in (EXACT, FAST, FAST16):
        assert plan(driver, mode, 512, 300, TRAIN_LONG_ATTN=value)["train_long_attn"] == 0
    assert plan(driver, EXACT, 96, 351, TRAIN_LONG_ATTN=value)["train_long_attn"] == 0
    rc, msg = refusal(driver, FAST, 384, TRAIN_LONG_ATTN=value)
    assert rc == ENOTSUP and SWITCH not in msg and msg.startswith("channels=384 heads=8 hidden=768: FAST contexts exist"), msg


def test_the_earlier_refusals_keep_their_place(driver):
    """Steps 1 to 5 of plan_context win over a bad value of the switch; it wins over the steps behind it."""
    got = plans(driver,
                case(TRAIN, 96, 1025, TRAIN_LONG_ATTN="junk"),
                case(TRAIN, 96, EXACT_IMPL="f16x2", TRAIN_LONG_ATTN="junk"),
                case(TRAIN, 96, TRAIN_IMPL="f16x2", TRAIN_LONG_ATTN="junk"),
                case(TRAIN, 96, 351, TRAIN_LONG_ATTN="junk"),
                case(TRAIN, 512, TRAIN_PASSES="2", TRAIN_LONG_ATTN="junk"),
                case(TRAIN, 96, 351, TRAIN_PASSES="2", TRAIN_LONG_ATTN="chunked"))
    starts = ["frames=1025 not in", "D3DP_EXACT_IMPL=f16x2 outside", "D3DP_TRAIN_IMPL=f16x2 outside", f"{SWITCH}=junk: the one value",
              f"{SWITCH}=junk: the one value", "D3DP_TRAIN_PASSES=2: the values"]
    for (rc, msg, _), start in zip(got, starts):
        assert rc == ENOTSUP and msg.startswith(start), (start, msg)


@pytest.mark.parametrize("other", [("TRAIN_IMPL", "f32"), ("TRAIN_ATTN", "f32"), ("TRAIN_ATTN", "x2t"), ("TRAIN_ATTN_BWD", "valu"),
                                   ("TRAIN_PASSES", "1"), ("TRAIN_OVERLAP", "0"), ("TRAIN_OVERLAP", "1")])
def test_the_other_training_switches_compose_with_it(driver, other):
    base = plan(driver, TRAIN, 512, 300, **{other[0]: other[1]})
    both = plan(driver, TRAIN, 512, 300, TRAIN_LONG_ATTN="chunked", **{other[0]: other[1]})
    assert both == dict(base, train_long_attn=1), (base, both)


# ---------------------------------------------------------------------------------------------- Python and command line
def env(monkeypatch, **kw):
    for k in _ALL:
        monkeypatch.delenv(k, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv("D3DP_" + k, v)


def test_train_arithmetic_names_the_route(monkeypatch):
    env(monkeypatch)
    plain = {cs: arithmetic(cs) for cs in (512, 96, 64)}
    assert all(SWITCH not in text for text in plain.values())
    assert plain[512].startswith("split-fp16 Linears (three fp16-MFMA passes, fp32 accumulate, device-side operand scales; forward "
                                 "and dgrad on 256 x 128 tiles")
    assert plain[96].startswith("fp32 path of a width outside {64, 128, 256, 512} (cs = 96): fp32-MFMA Linears")
    assert plain[96].endswith("VALU attention backward with a run-time head dim, run-time-width row kernels")
    for value in ("junk", ""):                                                 # (the text without the switch is the text of before)
        env(monkeypatch, TRAIN_LONG_ATTN=value)
        assert {cs: arithmetic(cs) for cs in plain} == plain
    env(monkeypatch, TRAIN_LONG_ATTN="chunked")
    for cs, before in plain.items():
        text = arithmetic(cs)
        assert text.startswith(before + "; ") and SWITCH + "=chunked" in text[len(before):] and "chunks of rows" in text, text


@pytest.mark.parametrize("before", [None, "chunked", "junk"])
def test_the_cli_flag_parses_and_leaves_the_environment_as_it_found_it(monkeypatch, before):
    env(monkeypatch, **({"TRAIN_LONG_ATTN": before} if before is not None else {}))
    assert cli.parse_args([]).train_long_attn is False
    assert cli.parse_args(["--train-long-attn"]).train_long_attn is True
    assert cli.parse_args(["--train-long-attn", "--train-passes", "1"]).train_passes == 1
    with cli.train_long_attn_env(True):
        assert os.environ[SWITCH] == "chunked"
    assert os.environ.get(SWITCH) == before
    with pytest.raises(RuntimeError):
        with cli.train_long_attn_env(True):
            raise RuntimeError("the creation of the context failed")
    assert os.environ.get(SWITCH) == before
    with cli.train_long_attn_env(False):
        assert os.environ.get(SWITCH) == before
    with cli.train_passes_env(1), cli.train_long_attn_env(True):
        assert os.environ[SWITCH] == "chunked" and os.environ["D3DP_TRAIN_PASSES"] == "1"
    assert os.environ.get(SWITCH) == before and "D3DP_TRAIN_PASSES" not in os.environ


# ---------------------------------------------------------------------------------------------- the GPU cases' references
@pytest.mark.parametrize("prob", FP64_CASES, ids=lambda c: c.id)
def test_every_fp64_checked_gpu_case_is_admissible(prob):
    """e32 -- the oracle's fp32 autograd against its fp64 autograd -- is at most 2e-6 (norm) and 5e-5 (per element), so that 8 x e32
    separates fp32-class from almost; the dropped-branch case has its 12 exactly-zero fp64 gradients."""
    ref = reference(prob)
    print(f"{prob.id}: e32 norm_rel {ref.e32[0]:.2e}, max_rms {ref.e32[1]:.2e}")
    assert gc.admissible(ref.e32), ref.e32
    zeros = sorted(n for n, g in ref.g64.items() if not g.any())
    assert zeros == (sorted(DROPPED_PARAMS) if prob == DROPPED.problem else []), zeros
    assert not gc.violations(gc.grad_errors(ref.g32, ref.g64), ref.e32)
