"""No GPU needed: what d3dp_create answers to D3DP_TRAIN_ROWS (opt-in hi-only operand rows of the one-pass training Linears) is decided
before the device is looked for (ctx_plan.h plan_context, step 7b), so a machine without one sees every refusal -- the switch is never
ignored -- and sees the contexts the switch takes get as far as the device check; what MixSTE2.train_arithmetic() and the command
line say about the route; and, through a stand-alone driver of the two plan headers (tests/train_rows_driver.cpp), that
TrainPlan::rows_hi follows the context while train_layout's offsets and total do not move."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from create_host import D3DP_ENOTSUP, create, reached_the_device_check
from d3dp_amd import _lib, cli
from test_train_widths_host import arithmetic

SWITCH = "D3DP_TRAIN_ROWS"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ALL = (SWITCH, "D3DP_TRAIN_PASSES", "D3DP_TRAIN_ATTN_PASSES", "D3DP_TRAIN_IMPL", "D3DP_TRAIN_ATTN", "D3DP_TRAIN_ATTN_BWD",
        "D3DP_TRAIN_OVERLAP", "D3DP_TRAIN_LONG_ATTN", "D3DP_TRAIN_WGRAD", "D3DP_TRAIN_TAIL", "D3DP_TRAIN_GELU", "D3DP_TRAIN_LN_OPERAND",
        "D3DP_EXACT_IMPL", "D3DP_FAST_IMPL", "D3DP_LONG_ATTN")
ROUTE = [256, 512]                                    # the widths of the route (hidden = 2 C, depth <= 8)


def env(monkeypatch, **kw):
    for k in _ALL:
        monkeypatch.delenv(k, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv("D3DP_" + k, v)


def create_deep(cs, depth, mode=_lib.MODE_TRAIN, hidden=None, heads=8):
    """create_host.create with a depth: -> (return code, message)."""
    lib = _lib.load()
    cfg = _lib.Cfg(9, 5, cs, depth, heads, 2 * cs if hidden is None else hidden, 1e-6, 1e-5, mode, 0)
    h = C.c_void_p()
    rc = lib.d3dp_create(C.byref(cfg), C.byref(h))
    msg = lib.d3dp_last_error().decode() if rc != 0 else ""
    if rc == 0:
        lib.d3dp_destroy(h)
    return rc, msg


def refused(rc, msg, *needles):
    assert rc == D3DP_ENOTSUP and SWITCH in msg and all(n in msg for n in needles), (rc, msg)
    assert "no HIP device" not in msg


# ---------------------------------------------------------------------------------------------- refusals and non-refusals
@pytest.mark.parametrize("cs", ROUTE)
def test_the_switch_passes_exactly_where_the_route_exists(monkeypatch, cs):
    env(monkeypatch, TRAIN_ROWS="hi", TRAIN_PASSES="1")
    assert reached_the_device_check(*create(cs, _lib.MODE_TRAIN))
    assert reached_the_device_check(*create_deep(cs, 8))
    assert reached_the_device_check(*create(cs, _lib.MODE_TRAIN, hidden=4 * cs))
    assert reached_the_device_check(*create(cs, _lib.MODE_TRAIN, frames=300))


@pytest.mark.parametrize("cs", [64, 128, 256, 512, 96, 384])
@pytest.mark.parametrize("passes", [None, "1", "3"])
def test_split_names_the_default_everywhere(monkeypatch, cs, passes):
    kw = {"TRAIN_PASSES": passes} if passes else {}
    if passes == "1" and cs in (96, 384):
        return                                           # (D3DP_TRAIN_PASSES=1 itself is refused on the fp32 path)
    env(monkeypatch, TRAIN_ROWS="split", **kw)
    assert reached_the_device_check(*create(cs, _lib.MODE_TRAIN))


@pytest.mark.parametrize("value", ["lo", "1", "", "HI", "hi ", "hix", "h", "splits"])
def test_any_other_value_is_refused_by_name(monkeypatch, value):
    """(On the parent every value was accepted silently: the variable was not read.)"""
    for cs, passes in ((512, "1"), (512, None), (96, None)):        # (cs 96 beside D3DP_TRAIN_PASSES=1: step 7 refuses first)
        env(monkeypatch, TRAIN_ROWS=value, **({"TRAIN_PASSES": passes} if passes else {}))
        rc, msg = create(cs, _lib.MODE_TRAIN)
        refused(rc, msg, f"{SWITCH}={value}")


@pytest.mark.parametrize("passes", [None, "3"])
def test_hi_is_refused_without_one_pass_linears(monkeypatch, passes):
    env(monkeypatch, TRAIN_ROWS="hi", **({"TRAIN_PASSES": passes} if passes else {}))
    for cs in ROUTE:
        refused(*create(cs, _lib.MODE_TRAIN), SWITCH + "=hi", "D3DP_TRAIN_PASSES=1")


@pytest.mark.parametrize("cs,impl", [(512, "f32"), (256, "f32"), (96, None), (384, None)])
def test_hi_is_refused_on_the_fp32_path(monkeypatch, cs, impl):
    env(monkeypatch, TRAIN_ROWS="hi", **({"TRAIN_IMPL": impl} if impl else {}))
    refused(*create(cs, _lib.MODE_TRAIN), SWITCH + "=hi", "fp32 path", f"channels={cs}")


@pytest.mark.parametrize("cs", [64, 128])
def test_hi_is_refused_where_transposed_operands_are_used(monkeypatch, cs):
    env(monkeypatch, TRAIN_ROWS="hi", TRAIN_PASSES="1")
    refused(*create(cs, _lib.MODE_TRAIN), SWITCH + "=hi", f"channels={cs}", "transposed")


def test_hi_is_refused_at_a_hidden_width_without_tn_shapes(monkeypatch):
    env(monkeypatch, TRAIN_ROWS="hi", TRAIN_PASSES="1")
    refused(*create(256, _lib.MODE_TRAIN, hidden=320), SWITCH + "=hi", "hidden=320")


@pytest.mark.parametrize("cs", [192, 320, 384, 448])
def test_hi_is_refused_at_the_padded_widths(monkeypatch, cs):
    env(monkeypatch, TRAIN_ROWS="hi", TRAIN_PASSES="1", TRAIN_IMPL="f16x2")
    refused(*create(cs, _lib.MODE_TRAIN), SWITCH + "=hi", "D3DP_TRAIN_IMPL=f16x2", f"channels={cs}")


def test_hi_is_refused_beyond_the_batched_weight_preparation(monkeypatch):
    env(monkeypatch, TRAIN_ROWS="hi", TRAIN_PASSES="1")
    refused(*create_deep(256, 9), SWITCH + "=hi", "depth=9")
    assert reached_the_device_check(*create_deep(256, 8))


def test_hi_is_refused_at_head_dim_16_under_the_split_attention(monkeypatch):
    env(monkeypatch, TRAIN_ROWS="hi", TRAIN_PASSES="1")
    refused(*create(256, _lib.MODE_TRAIN, heads=16), SWITCH + "=hi", "head dim 16")
    env(monkeypatch, TRAIN_ROWS="hi", TRAIN_PASSES="1", TRAIN_ATTN="f32")             # (no attention kernel writes operand rows then)
    assert reached_the_device_check(*create(256, _lib.MODE_TRAIN, heads=16))


@pytest.mark.parametrize("other", [("TRAIN_WGRAD", "each"), ("TRAIN_TAIL", "split"), ("TRAIN_GELU", "pass"), ("TRAIN_LN_OPERAND", "pass")])
def test_hi_is_refused_beside_the_superseded_launch_forms(monkeypatch, other):
    env(monkeypatch, TRAIN_ROWS="hi", **{other[0]: other[1]})
    refused(*create(512, _lib.MODE_TRAIN), SWITCH + "=hi", f"D3DP_{other[0]}={other[1]}")


@pytest.mark.parametrize("value", ["hi", "junk"])
def test_contexts_of_other_modes_do_not_read_the_switch(monkeypatch, value):
    """The reference keeps a train model and two eval models in one process."""
    env(monkeypatch, TRAIN_ROWS=value)
    for mode in (_lib.MODE_EXACT, _lib.MODE_FAST, _lib.MODE_FAST16):
        assert reached_the_device_check(*create(512, mode))
    assert reached_the_device_check(*create(96, _lib.MODE_EXACT))
    rc, msg = create(384, _lib.MODE_FAST)
    assert rc == D3DP_ENOTSUP and SWITCH not in msg, (rc, msg)


@pytest.mark.parametrize("other", [("TRAIN_ATTN_PASSES", "1"), ("TRAIN_ATTN_PASSES", "3"), ("TRAIN_ATTN", "f32"), ("TRAIN_ATTN", "x2t"),
                                   ("TRAIN_ATTN_BWD", "valu"), ("TRAIN_OVERLAP", "0"), ("TRAIN_OVERLAP", "1"), ("TRAIN_LONG_ATTN", "chunked")])
def test_the_pass_attention_and_stream_switches_compose_with_it(monkeypatch, other):
    env(monkeypatch, TRAIN_ROWS="hi", TRAIN_PASSES="1", **{other[0]: other[1]})
    for cs in ROUTE:
        assert reached_the_device_check(*create(cs, _lib.MODE_TRAIN))


# ---------------------------------------------------------------------------------------------- Python and command line
def test_train_arithmetic_names_the_route(monkeypatch):
    env(monkeypatch, TRAIN_PASSES="1")
    one512, one256, one128 = arithmetic(512), arithmetic(256), arithmetic(128)
    assert SWITCH not in one512 and "D3DP_TRAIN_PASSES=1" in one512
    env(monkeypatch, TRAIN_PASSES="1", TRAIN_ROWS="split")
    assert arithmetic(512) == one512
    env(monkeypatch, TRAIN_PASSES="1", TRAIN_ROWS="hi")
    for cs, before in ((512, one512), (256, one256)):
        text = arithmetic(cs)
        assert text.startswith(before) and SWITCH + "=hi" in text[len(before):] and "plain fp16 rows" in text, text
    assert arithmetic(128) == one128                     # (refused there: no such route to name)
    env(monkeypatch, TRAIN_PASSES="1", TRAIN_ROWS="hi", TRAIN_ATTN_PASSES="1")
    text = arithmetic(512)
    assert SWITCH + "=hi" in text and "D3DP_TRAIN_ATTN_PASSES=1" in text and "D3DP_TRAIN_PASSES=1" in text
    env(monkeypatch, TRAIN_ROWS="hi")                   # (without the one-pass Linears: refused, nothing named)
    assert SWITCH not in arithmetic(512)
    env(monkeypatch, TRAIN_ROWS="hi", TRAIN_PASSES="1", TRAIN_IMPL="f32")
    assert SWITCH not in arithmetic(512)


def test_the_text_without_the_switch_is_the_text_of_before(monkeypatch):
    env(monkeypatch)
    assert arithmetic(512).startswith("split-fp16 Linears (three fp16-MFMA passes, fp32 accumulate, device-side operand scales; forward "
                                      "and dgrad on 256 x 128 tiles")
    assert SWITCH not in arithmetic(512) and SWITCH not in arithmetic(256)
    env(monkeypatch, TRAIN_PASSES="1")
    assert arithmetic(512).startswith("one-pass fp16 Linears of D3DP_TRAIN_PASSES=1 (one fp16-MFMA pass hi(A) x hi(W) per product")


@pytest.mark.parametrize("before", [None, "split", "junk"])
def test_the_cli_flag_parses_and_leaves_the_environment_as_it_found_it(monkeypatch, before):
    env(monkeypatch, **({"TRAIN_ROWS": before} if before is not None else {}))
    assert cli.parse_args([]).train_rows is None
    assert cli.parse_args(["--train-rows", "hi"]).train_rows == "hi" and cli.parse_args(["--train-rows", "split"]).train_rows == "split"
    with pytest.raises(SystemExit):
        cli.parse_args(["--train-rows", "lo"])
    for rows in ("hi", "split"):
        with cli.train_rows_env(rows):
            assert os.environ[SWITCH] == rows
        assert os.environ.get(SWITCH) == before
    with pytest.raises(RuntimeError):
        with cli.train_rows_env("hi"):
            raise RuntimeError("the creation of the context failed")
    assert os.environ.get(SWITCH) == before
    with cli.train_rows_env(None):
        assert os.environ.get(SWITCH) == before


# ---------------------------------------------------------------------------------------------- the host plan harness
TRAIN, EXACT = 2, 0


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("train_rows") / "driver")
    subprocess.run(["g++", "-std=c++17", os.path.join(ROOT, "tests", "train_rows_driver.cpp"), "-o", exe], check=True)
    return exe


def plans(driver, *cases):
    """cases: (mode, cs, frames, depth, B, {switch without D3DP_: value}) -> [(return code, message, {member: value})]."""
    lines = ["\t".join([str(x) for x in (mode, cs, 8, 2 * cs, frames, 17, depth, B)] + [f"D3DP_{k}={v}" for k, v in sw.items()])
             for mode, cs, frames, depth, B, sw in cases]
    clean = {k: v for k, v in os.environ.items() if not k.startswith("D3DP_")}
    out = subprocess.run([driver], input="".join(l + "\n" for l in lines), env=clean, capture_output=True, text=True, check=True).stdout
    rows = [line.split("\t") for line in out.split("\n")[:-1]]
    assert len(rows) == len(cases), out
    return [(int(r[0]), r[1], dict(x.split("=", 1) for x in r[2:])) for r in rows]


def test_the_modes_agree_with_the_library():
    assert (TRAIN, EXACT) == (_lib.MODE_TRAIN, _lib.MODE_EXACT)


@pytest.mark.parametrize("cs,frames,depth,B", [(512, 9, 2, 2), (256, 27, 2, 2), (256, 9, 2, 1), (256, 128, 2, 2), (256, 300, 2, 2),
                                               (512, 243, 8, 4), (256, 9, 8, 2)])
def test_rows_hi_follows_the_context_and_the_layout_does_not_move(driver, cs, frames, depth, B):
    one = {"TRAIN_PASSES": "1"}
    (rc1, m1, p1), (rch, mh, ph), (rcs, ms, psp) = plans(driver, (TRAIN, cs, frames, depth, B, one),
                                                         (TRAIN, cs, frames, depth, B, {**one, "TRAIN_ROWS": "hi"}),
                                                         (TRAIN, cs, frames, depth, B, {**one, "TRAIN_ROWS": "split"}))
    assert (rc1, m1, rch, mh, rcs, ms) == (0, "", 0, "", 0, ""), (m1, mh, ms)
    assert p1["train_rows_hi"] == "0" and p1["rows_hi"] == "0" and psp == p1
    assert ph == {**p1, "train_rows_hi": "1", "rows_hi": "1"}, ph                      # nothing else of either plan moves: layout included
    assert ph["layout"] == p1["layout"] and ph["layout"].count(",") > 30
    # what the route stands on: no transposed operand, the LayerNorm kernels write rows, one launch prepares every weight
    assert (ph["passes"], ph["all_tn"], ph["ln_direct"], ph["batched"]) == ("1", "1", "1", "1"), ph


def test_the_driver_refuses_what_the_library_refuses(driver):
    hi = {"TRAIN_ROWS": "hi", "TRAIN_PASSES": "1"}
    got = plans(driver, (TRAIN, 128, 9, 2, 2, hi), (TRAIN, 256, 9, 9, 2, hi), (TRAIN, 256, 9, 2, 2, {"TRAIN_ROWS": "hi"}),
                (TRAIN, 256, 9, 2, 2, {**hi, "TRAIN_ROWS": "lo"}), (EXACT, 256, 9, 2, 2, {"TRAIN_ROWS": "lo"}))
    for rc, msg, p in got[:4]:
        assert rc == D3DP_ENOTSUP and SWITCH in msg and p["train_rows_hi"] == "0", (rc, msg)      # (a refusal leaves the caller's plan alone)
    assert got[4][0] == 0 and got[4][2]["train_rows_hi"] == "0"
