"""No GPU and no library needed: the route d3dp_create decides for a context -- plan_context() of d3dp_amd/csrc/ctx_plan.h, pure
arithmetic on a d3dp_cfg and the environment switches -- checked through a stand-alone driver (tests/ctx_plan_driver.cpp): what an
ACCEPTED context is routed to, every parsing quirk of the switches, and the order of the ten refusal steps.  The *_host.py tests
beside this one see the refusals through the library; the routes they cannot see without a device are pinned here."""
import os
import shutil
import subprocess

import pytest

EXACT, FAST, TRAIN, FAST16 = 0, 1, 2, 3
OK, EINVAL, ENOTSUP = 0, -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXXFLAGS = ["-std=c++17"]
DEFAULTS = dict(hdp=0, fast16_scale=0, train_passes=3, exact_impl_req=0, long_rows=0, fold=1, defer=1, train_x2=1, train_overlap=1,
                train_overlap_sets=2, train_gelu_in_prep=1, train_wgrad_merged=1, train_ln_direct=1, train_tail_blocks=1,
                train_attn_x2=2, skew_d=0, pingpong=0, pad_override=-1, fold_ln_on=0)
OPTIN_WIDTHS = (192, 320, 384, 448)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("ctx_plan") / "driver")
    subprocess.run(["g++", *CXXFLAGS, os.path.join(ROOT, "tests", "ctx_plan_driver.cpp"), "-o", exe], check=True)
    return exe


def case(mode, cs, heads=8, hidden=None, frames=9, joints=5, variants=0, **env):
    """One line of the driver's input; env: the switches without their D3DP_ prefix."""
    fields = [mode, cs, heads, 2 * cs if hidden is None else hidden, frames, joints, variants]
    return "\t".join([str(f) for f in fields] + [f"D3DP_{k}={v}" for k, v in env.items()])


def plans(driver, *cases):
    """-> [(return code, message, {field: value})], one per case, from one run of the driver."""
    clean = {k: v for k, v in os.environ.items() if not k.startswith("D3DP_")}
    out = subprocess.run([driver], input="".join(c + "\n" for c in cases), env=clean, capture_output=True, text=True, check=True).stdout
    rows = [line.split("\t") for line in out.split("\n")[:-1]]
    assert len(rows) == len(cases), out
    return [(int(r[0]), r[1], {k: int(v) for k, v in (f.split("=") for f in r[2:])}) for r in rows]


def plan(driver, *a, **kw):
    """The plan of one ACCEPTED context."""
    (rc, msg, p), = plans(driver, case(*a, **kw))
    assert rc == OK and msg == "", (rc, msg)
    return p


def refusal(driver, *a, **kw):
    (rc, msg, p), = plans(driver, case(*a, **kw))
    assert rc != OK and msg, (a, kw, p)
    return rc, msg


def members(p):
    return {k: v for k, v in p.items() if k != "train_linears_split"}


# ---------------------------------------------------------------------------------------------- accepted contexts
@pytest.mark.parametrize("mode", [EXACT, FAST, FAST16, TRAIN])
def test_the_default_plan_at_512(driver, mode):
    assert members(plan(driver, mode, 512)) == DEFAULTS


@pytest.mark.parametrize("mode", [EXACT, TRAIN])
@pytest.mark.parametrize("cs", [96, 384])
def test_the_default_plan_outside_the_instantiated_widths_is_the_fp32_one(driver, cs, mode):
    assert members(plan(driver, mode, cs)) == dict(DEFAULTS, exact_impl_req=2, train_x2=0)


@pytest.mark.parametrize("mode,env", [(EXACT, {"EXACT_IMPL": "f16x2"}), (FAST, {"FAST_IMPL": "mfma"}), (FAST16, {"FAST_IMPL": "mfma"})])
def test_padded_heads(driver, mode, env):
    for cs, hdp in zip(OPTIN_WIDTHS, (32, 64, 64, 64)):                 # head dims 24, 40, 48, 56 with the model's 8 heads
        assert members(plan(driver, mode, cs, **env)) == dict(DEFAULTS, hdp=hdp), cs
    # head dims 32 and 64 need no padding but take the route: hdp is the head dim itself
    for cs, heads, hdp in ((384, 12, 32), (384, 6, 64), (192, 6, 32), (192, 3, 64), (448, 14, 32), (320, 5, 64)):
        assert members(plan(driver, mode, cs, heads=heads, **env)) == dict(DEFAULTS, hdp=hdp), (cs, heads)
    assert members(plan(driver, mode, 512, **env)) == DEFAULTS             # (an instantiated width: the value names the default)


def test_the_exact_switch_pads_head_dims_8_and_16_too(driver):
    """(D3DP_FAST_IMPL=mfma refuses them: tests/test_fast_widths_host.py)"""
    assert plan(driver, EXACT, 384, heads=24, EXACT_IMPL="f16x2")["hdp"] == 32
    assert plan(driver, EXACT, 384, heads=48, EXACT_IMPL="f16x2")["hdp"] == 32


@pytest.mark.parametrize("cs", OPTIN_WIDTHS)
def test_the_train_switch_opts_in_without_padding(driver, cs):
    assert members(plan(driver, TRAIN, cs, TRAIN_IMPL="f16x2")) == dict(DEFAULTS, exact_impl_req=2)       # train_x2 stays 1, hdp 0
    assert plan(driver, TRAIN, cs, frames=1024, TRAIN_IMPL="f16x2")["train_x2"] == 1
    assert members(plan(driver, EXACT, cs, TRAIN_IMPL="f16x2")) == dict(DEFAULTS, exact_impl_req=2, train_x2=0)   # (not read there)


def test_fast16_scale_is_set_for_fast16_at_an_instantiated_width_alone(driver):
    for cs in (128, 256, 512):
        assert members(plan(driver, FAST16, cs, FAST16_RANGE="scale")) == dict(DEFAULTS, fast16_scale=1)
        assert plan(driver, FAST16, cs)["fast16_scale"] == 0
        for mode in (FAST, EXACT, TRAIN):
            assert plan(driver, mode, cs, FAST16_RANGE="scale")["fast16_scale"] == 0
    assert plan(driver, FAST16, 384, FAST_IMPL="mfma")["fast16_scale"] == 0
    refusal(driver, FAST16, 384, FAST_IMPL="mfma", FAST16_RANGE="scale")
    refusal(driver, FAST16, 384, FAST16_RANGE="scale")


def test_train_passes_is_1_or_3(driver):
    assert plan(driver, TRAIN, 512)["train_passes"] == 3
    assert plan(driver, TRAIN, 512, TRAIN_PASSES="3")["train_passes"] == 3
    assert members(plan(driver, TRAIN, 512, TRAIN_PASSES="1")) == dict(DEFAULTS, train_passes=1)
    assert plan(driver, TRAIN, 384, TRAIN_IMPL="f16x2", TRAIN_PASSES="1")["train_passes"] == 1
    assert plan(driver, TRAIN, 384, TRAIN_PASSES="3")["train_passes"] == 3
    for mode in (EXACT, FAST, FAST16):
        for value in ("1", "2"):
            assert plan(driver, mode, 512, TRAIN_PASSES=value)["train_passes"] == 3


# ---------------------------------------------------------------------------------------------- parsing quirks
def field(driver, name, mode, cs, **kw):
    return plan(driver, mode, cs, **kw)[name]


def test_exact_impl_values(driver):
    for value, req in (("bf16x3", 1), ("f32", 2), ("f16x2", 0), ("F32", 0), ("bf16x3 ", 0), ("", 0)):
        assert field(driver, "exact_impl_req", EXACT, 512, EXACT_IMPL=value) == req, value
    for value in ("f32", "junk", ""):                                   # forced at a width neither instantiated nor padded
        assert field(driver, "exact_impl_req", EXACT, 96, EXACT_IMPL=value) == 2, value
    assert field(driver, "exact_impl_req", EXACT, 384, EXACT_IMPL="f16x2") == 0


def test_long_attn_is_exactly_rows(driver):
    assert [field(driver, "long_rows", EXACT, 512, LONG_ATTN=v) for v in ("rows", "Rows", "rows ", "row", "1", "")] == [1, 0, 0, 0, 0, 0]


def test_first_character_switches(driver):
    assert [field(driver, "fold", EXACT, 512, NO_FOLD=v) for v in ("1", "1x", "10", "0", "yes", " 1", "")] == [0, 0, 0, 1, 1, 1, 1]
    assert [field(driver, "defer", EXACT, 512, DEFER_NORM=v) for v in ("0", "0x", "01", "1", "off", " 0", "")] == [0, 0, 0, 1, 1, 1, 1]
    assert [field(driver, "fold_ln_on", EXACT, 512, variants=1, FOLD_LN=v) for v in ("1", "1x", "0", "on", "")] == [1, 1, 0, 0, 0]


def test_train_overlap(driver):
    got = [plan(driver, TRAIN, 512, TRAIN_OVERLAP=v) for v in ("0", "01", "1", "10", "2", "on", "")]
    assert [(p["train_overlap"], p["train_overlap_sets"]) for p in got] == [(0, 2), (0, 2), (1, 1), (1, 1), (1, 2), (1, 2), (1, 2)]


def test_train_attn(driver):
    assert [field(driver, "train_attn_x2", TRAIN, 512, TRAIN_ATTN=v) for v in ("f32", "x2t", "x2", "F32", "x2t ", "")] == [0, 1, 2, 2, 2, 2]


@pytest.mark.parametrize("name,value,member", [("TRAIN_GELU", "pass", "train_gelu_in_prep"), ("TRAIN_WGRAD", "each", "train_wgrad_merged"),
                                               ("TRAIN_LN_OPERAND", "pass", "train_ln_direct"), ("TRAIN_TAIL", "split", "train_tail_blocks")])
def test_the_superseded_launch_forms_take_exact_strings(driver, name, value, member):
    assert members(plan(driver, TRAIN, 512, variants=1, **{name: value})) == dict(DEFAULTS, **{member: 0})
    for other in (value.upper(), value + " ", value[:-1], "1", ""):
        assert members(plan(driver, TRAIN, 512, **{name: other})) == DEFAULTS, other           # (no request: the product library takes it)


def test_the_experiment_switches_take_exact_digits(driver):
    v1 = dict(variants=1)
    assert [field(driver, "skew_d", EXACT, 512, X2_SKEW=v, **v1) for v in ("0", "1", "2", "4", "3", "8", "12", "1 ", "")] == [0, 1, 2, 4, 0, 0, 0, 0, 0]
    assert [field(driver, "pingpong", EXACT, 512, X2_PP=v, **v1) for v in ("0", "1", "2", "11", "")] == [0, 1, 0, 0, 0]
    assert [field(driver, "pad_override", EXACT, 512, SEQ_PAD=v, **v1) for v in ("0", "1", "2", "01", "")] == [0, 1, -1, -1, -1]
    # D3DP_X2_WIDE=1 wins over whatever D3DP_X2_PP said; any other value leaves it
    assert [field(driver, "pingpong", EXACT, 512, X2_WIDE="1", X2_PP=v, **v1) for v in ("0", "1", "junk")] == [2, 2, 2]
    assert field(driver, "pingpong", EXACT, 512, X2_WIDE="1", **v1) == 2
    assert [field(driver, "pingpong", EXACT, 512, X2_WIDE=v, X2_PP="1", **v1) for v in ("11", "0", "")] == [1, 1, 1]


@pytest.mark.parametrize("mode,name,needle", [(FAST, "FAST_IMPL", "D3DP_FAST_IMPL=: the one value"), (FAST16, "FAST_IMPL", "D3DP_FAST_IMPL=: the one value"),
                                              (FAST16, "FAST16_RANGE", "D3DP_FAST16_RANGE=: the one value"),
                                              (TRAIN, "TRAIN_PASSES", "D3DP_TRAIN_PASSES=: the values")])
def test_a_set_but_empty_value_is_a_refused_value(driver, mode, name, needle):
    rc, msg = refusal(driver, mode, 512, **{name: ""})
    assert rc == ENOTSUP and msg.startswith(needle), msg


def test_the_mode_specific_switches_are_read_for_their_modes_only(driver):
    for mode in (EXACT, TRAIN):
        assert members(plan(driver, mode, 512, FAST_IMPL="rows", FAST16_RANGE="junk")) == DEFAULTS
    assert members(plan(driver, FAST, 512, FAST16_RANGE="junk", TRAIN_PASSES="2", TRAIN_IMPL="f16x2")) == DEFAULTS
    assert members(plan(driver, FAST16, 512, TRAIN_PASSES="2")) == DEFAULTS
    assert members(plan(driver, EXACT, 96, TRAIN_IMPL="f16x2", TRAIN_PASSES="1")) == dict(DEFAULTS, exact_impl_req=2, train_x2=0)
    assert field(driver, "train_x2", EXACT, 512, TRAIN_IMPL="f32") == 0        # (the cross-check value is parsed in every mode)


def test_the_variants_flag_turns_steps_9_and_10_from_refusal_into_acceptance(driver):
    rc, msg = refusal(driver, TRAIN, 512, TRAIN_WGRAD="each")
    assert rc == ENOTSUP and msg.startswith("D3DP_TRAIN_WGRAD=each / D3DP_TRAIN_TAIL=split / ") and "only the variants build honours" in msg
    assert members(plan(driver, TRAIN, 512, variants=1, TRAIN_WGRAD="each")) == dict(DEFAULTS, train_wgrad_merged=0)
    for env, want in (({"X2_SKEW": "1"}, {"skew_d": 1}), ({"X2_PP": "1"}, {"pingpong": 1}), ({"X2_WIDE": "1"}, {"pingpong": 2}),
                      ({"SEQ_PAD": "1"}, {"pad_override": 1}), ({"FOLD_LN": "1"}, {"fold_ln_on": 1})):
        rc, msg = refusal(driver, EXACT, 512, **env)
        assert rc == ENOTSUP and msg.startswith("D3DP_X2_SKEW / D3DP_X2_PP / D3DP_X2_WIDE / D3DP_SEQ_PAD / D3DP_FOLD_LN select experiment kernels")
        assert members(plan(driver, EXACT, 512, variants=1, **env)) == dict(DEFAULTS, **want)
    # the values that ask for nothing are no request
    assert members(plan(driver, EXACT, 512, X2_SKEW="0", X2_PP="0", SEQ_PAD="0", FOLD_LN="0")) == dict(DEFAULTS, pad_override=0)


# ---------------------------------------------------------------------------------------------- the order of the refusals
ORDER = [
    # (step, case that trips it and a later one, start of the message of the earlier)
    (1, case(EXACT, 96, frames=1025, EXACT_IMPL="f16x2"), ENOTSUP, "frames=1025 not in [1,1024]"),
    (1, case(EXACT, 96, joints=257, EXACT_IMPL="f16x2"), ENOTSUP, "joints=257 not in [1,256]"),
    (1, case(FAST, 384, heads=7), EINVAL, "heads=7 does not divide channels=384"),
    (1, case(7, 384), EINVAL, "mode=7"),
    (2, case(TRAIN, 96, EXACT_IMPL="f16x2", TRAIN_IMPL="f16x2"), ENOTSUP, "D3DP_EXACT_IMPL=f16x2 outside the instantiated widths exists for"),
    (2, case(EXACT, 96, EXACT_IMPL="f16x2", LONG_ATTN="rows"), ENOTSUP, "D3DP_EXACT_IMPL=f16x2 outside the instantiated widths exists for"),
    (2, case(EXACT, 384, frames=300, EXACT_IMPL="f16x2", LONG_ATTN="rows", X2_SKEW="1"), ENOTSUP, "D3DP_LONG_ATTN=rows with D3DP_EXACT_IMPL=f16x2 at channels=384"),
    (2, case(FAST16, 384, EXACT_IMPL="f16x2", FAST_IMPL="rows"), ENOTSUP, "D3DP_EXACT_IMPL=f16x2 outside"),
    (3, case(TRAIN, 96, TRAIN_IMPL="f16x2", TRAIN_PASSES="2"), ENOTSUP, "D3DP_TRAIN_IMPL=f16x2 outside the instantiated widths exists for"),
    (3, case(TRAIN, 2048, TRAIN_IMPL="f16x2"), ENOTSUP, "D3DP_TRAIN_IMPL=f16x2 outside"),                # (before step 6's width limit)
    (4, case(FAST16, 384, FAST_IMPL="rows", FAST16_RANGE="junk"), ENOTSUP, "D3DP_FAST_IMPL=rows: the one value"),
    (4, case(FAST, 96, FAST_IMPL="mfma", LONG_ATTN="rows"), ENOTSUP, "D3DP_FAST_IMPL=mfma outside the instantiated widths exists for"),
    (4, case(FAST16, 384, FAST_IMPL="mfma", LONG_ATTN="rows", FAST16_RANGE="scale"), ENOTSUP, "D3DP_LONG_ATTN=rows with D3DP_FAST_IMPL=mfma at channels=384"),
    (5, case(FAST16, 384, FAST16_RANGE="junk"), ENOTSUP, "D3DP_FAST16_RANGE=junk: the one value"),        # (before step 6's FAST16 refusal)
    (5, case(FAST16, 384, FAST_IMPL="mfma", FAST16_RANGE="junk"), ENOTSUP, "D3DP_FAST16_RANGE=junk: the one value"),
    (5, case(FAST16, 384, FAST_IMPL="mfma", FAST16_RANGE="scale", X2_PP="1"), ENOTSUP, "D3DP_FAST16_RANGE=scale with D3DP_FAST_IMPL=mfma at channels=384"),
    (5, case(FAST16, 64, hidden=832, FAST16_RANGE="scale", LONG_ATTN="rows"), ENOTSUP, "D3DP_FAST16_RANGE=scale at head dim 8 (channels=64 heads=8)"),
    (5, case(FAST16, 512, hidden=832, FAST16_RANGE="scale", LONG_ATTN="rows"), ENOTSUP, "D3DP_FAST16_RANGE=scale with D3DP_LONG_ATTN=rows"),
    (5, case(FAST16, 512, hidden=832, FAST16_RANGE="scale", FOLD_LN="1"), ENOTSUP, "D3DP_FAST16_RANGE=scale with hidden=832"),
    (6, case(FAST16, 384, FAST16_RANGE="scale", X2_SKEW="1"), ENOTSUP, "channels=384 heads=8 hidden=768: FAST16 contexts exist"),
    (6, case(FAST, 384, EXACT_IMPL="bf16x3"), ENOTSUP, "channels=384 heads=8 hidden=768: FAST contexts exist"),
    (6, case(TRAIN, 2048, frames=300, TRAIN_PASSES="2"), ENOTSUP, "channels=2048 heads=8 hidden=4096: the fp32 implementation takes"),
    (6, case(TRAIN, 384, frames=300, TRAIN_PASSES="2"), ENOTSUP, "channels=384 heads=8 frames=300 joints=5: training at a width outside"),
    (6, case(TRAIN, 1024, frames=154, EXACT_IMPL="bf16x3"), ENOTSUP, "channels=1024 heads=8 frames=154 joints=5: training at a width outside"),
    (7, case(TRAIN, 384, TRAIN_PASSES="2", EXACT_IMPL="bf16x3"), ENOTSUP, "D3DP_TRAIN_PASSES=2: the values a TRAIN context takes"),
    (7, case(TRAIN, 384, TRAIN_PASSES="1", EXACT_IMPL="bf16x3"), ENOTSUP, "D3DP_TRAIN_PASSES=1 exists for the split-fp16 training Linears; channels=384 trains"),
    (7, case(TRAIN, 512, TRAIN_PASSES="1", TRAIN_IMPL="f32", TRAIN_WGRAD="each"), ENOTSUP,
     "D3DP_TRAIN_PASSES=1 exists for the split-fp16 training Linears; channels=512 under D3DP_TRAIN_IMPL=f32 trains"),
    (7, case(TRAIN, 512, TRAIN_PASSES="1", TRAIN_TAIL="split"), ENOTSUP, "D3DP_TRAIN_PASSES=1 beside D3DP_TRAIN_WGRAD=each / "),
    (8, case(EXACT, 384, EXACT_IMPL="bf16x3", TRAIN_WGRAD="each"), ENOTSUP, "D3DP_EXACT_IMPL=bf16x3 exists for channels in {64,128,256,512}; channels=384 runs"),
    (8, case(TRAIN, 96, EXACT_IMPL="bf16x3", X2_SKEW="1"), ENOTSUP, "D3DP_EXACT_IMPL=bf16x3 exists for channels in {64,128,256,512}; channels=96 runs"),
    (9, case(TRAIN, 512, TRAIN_GELU="pass", X2_SKEW="1"), ENOTSUP, "D3DP_TRAIN_WGRAD=each / D3DP_TRAIN_TAIL=split / D3DP_TRAIN_GELU=pass / D3DP_TRAIN_LN_OPERAND=pass select"),
    (10, case(EXACT, 512, TRAIN_LN_OPERAND="pass", FOLD_LN="1"), ENOTSUP, "D3DP_TRAIN_WGRAD=each / "),   # (step 10 loses to step 9)
    (10, case(EXACT, 512, variants=0, SEQ_PAD="1"), ENOTSUP, "D3DP_X2_SKEW / D3DP_X2_PP / D3DP_X2_WIDE / D3DP_SEQ_PAD / D3DP_FOLD_LN select"),
]


def test_the_first_refusal_is_the_one_of_the_earliest_step(driver):
    assert sorted({step for step, *_ in ORDER}) == list(range(1, 11))
    got = plans(driver, *[c for _, c, _, _ in ORDER])
    for (step, c, code, start), (rc, msg, p) in zip(ORDER, got):
        assert rc == code and msg.startswith(start), (step, c, rc, msg)
        assert members(p) == DEFAULTS                                     # a refusal leaves the caller's plan alone


# ---------------------------------------------------------------------------------------------- the shared predicate
@pytest.mark.parametrize("cs,train_x2", [(64, (1, 0, 1)), (96, (0, 0, None)), (384, (0, 0, 1)), (512, (1, 0, 1))])
def test_train_linears_split_is_the_expression_trainpath_held(driver, cs, train_x2):
    """use_x2 = train_x2 && channels % 32 == 0 && hidden % 32 == 0 (TrainPath before it called the predicate); None: refused."""
    got = plans(driver, *[case(TRAIN, cs, **({"TRAIN_IMPL": v} if v else {})) for v in (None, "f32", "f16x2")])
    for (rc, msg, p), want in zip(got, train_x2):
        assert (rc == OK) == (want is not None), msg
        if rc == OK:
            assert p["train_x2"] == want
        assert p["train_linears_split"] == int(bool(p["train_x2"]) and cs % 32 == 0 and (2 * cs) % 32 == 0)
