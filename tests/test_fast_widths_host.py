"""No GPU needed: what d3dp_create answers to D3DP_FAST_IMPL=mfma (the opt-in FAST / FAST16 route with padded heads at channels
192 / 320 / 384 / 448) is decided before the device is looked for, so a machine without one sees every refusal -- the switch is
never ignored -- and sees the shapes the switch takes get as far as the device check.  The form of test_exact_widths_host.py."""
import pytest

from create_host import D3DP_ENOTSUP, create, reached_the_device_check
from d3dp_amd import _lib

SWITCH = "D3DP_FAST_IMPL=mfma"
FAST_MODES = [_lib.MODE_FAST, _lib.MODE_FAST16]
# the two refusals of a library without the switch (capi.hip), verbatim for channels = 384, heads = 8, hidden = 768
TODAY = {
    _lib.MODE_FAST: "channels=384 heads=8 hidden=768: FAST contexts exist for channels in {64,128,256,512} with head dim in "
                    "{8,16,32,64} and hidden a multiple of 64; other widths run in D3DP_MODE_EXACT / D3DP_MODE_TRAIN (fp32 implementation)",
    _lib.MODE_FAST16: "channels=384 heads=8 hidden=768: FAST16 contexts exist for the shapes FAST contexts exist for -- channels in "
                      "{64,128,256,512} with head dim in {8,16,32,64} and hidden a multiple of 64; other widths run in D3DP_MODE_EXACT / "
                      "D3DP_MODE_TRAIN (fp32 implementation)",
}


@pytest.mark.parametrize("mode", FAST_MODES)
@pytest.mark.parametrize("cs", [192, 320, 384, 448, 512])
def test_the_switch_passes_at_its_widths_and_at_an_instantiated_one(monkeypatch, cs, mode):
    """(512: the value names the default there)"""
    monkeypatch.setenv("D3DP_FAST_IMPL", "mfma")
    assert reached_the_device_check(*create(cs, mode))


@pytest.mark.parametrize("mode", FAST_MODES)
@pytest.mark.parametrize("cs", [96, 224, 576, 1024])
def test_the_switch_is_refused_at_widths_it_has_no_kernels_for(monkeypatch, cs, mode):
    """Head dims 12 and 28 are no multiple of 8; 72 and 128 exceed 64."""
    monkeypatch.setenv("D3DP_FAST_IMPL", "mfma")
    rc, msg = create(cs, mode)
    assert rc == D3DP_ENOTSUP and SWITCH in msg and f"channels={cs}" in msg, (rc, msg)


@pytest.mark.parametrize("mode", FAST_MODES)
@pytest.mark.parametrize("cs,heads", [(192, 12), (192, 24), (320, 20), (320, 40), (384, 24), (384, 48), (448, 28), (448, 56), (384, 32)])
def test_head_dims_without_a_kernel_are_refused_at_creation(monkeypatch, cs, heads, mode):
    """Other head counts than the model's 8: head dims 16 and 8 (and 12: 384 / 32) have no attention kernel behind the switch, and
    448 with 28 heads would pad its qkv rows beyond the Linear's bias area -- refused by name here, not at the first denoise."""
    monkeypatch.setenv("D3DP_FAST_IMPL", "mfma")
    rc, msg = create(cs, mode, heads=heads)
    assert rc == D3DP_ENOTSUP and SWITCH in msg and f"channels={cs}" in msg and f"heads={heads}" in msg, (rc, msg)


@pytest.mark.parametrize("mode", FAST_MODES)
@pytest.mark.parametrize("cs,heads", [(192, 6), (192, 3), (320, 10), (320, 5), (384, 12), (384, 6), (448, 14), (448, 7),   # head dims 32, 64
                                      (384, 16), (192, 4), (320, 8), (448, 8)])                                          # 24, 48, 40, 56
def test_the_head_dims_with_a_kernel_pass(monkeypatch, cs, heads, mode):
    monkeypatch.setenv("D3DP_FAST_IMPL", "mfma")
    assert reached_the_device_check(*create(cs, mode, heads=heads))


@pytest.mark.parametrize("mode", FAST_MODES)
@pytest.mark.parametrize("cs", [384, 512])
def test_another_value_of_the_variable_is_refused(monkeypatch, cs, mode):
    monkeypatch.setenv("D3DP_FAST_IMPL", "rows")
    rc, msg = create(cs, mode)
    assert rc == D3DP_ENOTSUP and SWITCH in msg and f"channels={cs}" in msg, (rc, msg)


@pytest.mark.parametrize("mode", FAST_MODES)
def test_the_row_attention_switch_is_refused_beside_it(monkeypatch, mode):
    monkeypatch.setenv("D3DP_FAST_IMPL", "mfma")
    monkeypatch.setenv("D3DP_LONG_ATTN", "rows")
    rc, msg = create(384, mode)
    assert rc == D3DP_ENOTSUP and "D3DP_LONG_ATTN=rows" in msg and SWITCH in msg and "channels=384" in msg, (rc, msg)
    assert reached_the_device_check(*create(512, mode))     # (an instantiated width: the cross-check as before)


@pytest.mark.parametrize("mode", FAST_MODES)
@pytest.mark.parametrize("hidden", [384, 1536, 832])
def test_a_hidden_that_is_not_twice_the_width_is_refused(monkeypatch, hidden, mode):
    monkeypatch.setenv("D3DP_FAST_IMPL", "mfma")
    rc, msg = create(384, mode, hidden=hidden)
    assert rc == D3DP_ENOTSUP and SWITCH in msg and "channels=384" in msg and f"hidden={hidden}" in msg, (rc, msg)


@pytest.mark.parametrize("value", ["mfma", "rows"])
@pytest.mark.parametrize("mode", [_lib.MODE_EXACT, _lib.MODE_TRAIN])
def test_exact_and_train_contexts_do_not_read_the_variable(monkeypatch, mode, value):
    monkeypatch.setenv("D3DP_FAST_IMPL", value)
    assert reached_the_device_check(*create(384, mode))
    assert reached_the_device_check(*create(512, mode))


@pytest.mark.parametrize("mode", FAST_MODES)
def test_the_exact_switch_keeps_its_own_refusal(monkeypatch, mode):
    monkeypatch.setenv("D3DP_EXACT_IMPL", "f16x2")
    monkeypatch.setenv("D3DP_FAST_IMPL", "mfma")
    rc, msg = create(384, mode)
    assert rc == D3DP_ENOTSUP and "D3DP_EXACT_IMPL=f16x2" in msg, (rc, msg)


@pytest.mark.parametrize("mode", FAST_MODES)
def test_without_the_switch_the_refusals_read_as_today(monkeypatch, mode):
    monkeypatch.delenv("D3DP_FAST_IMPL", raising=False)
    rc, msg = create(384, mode)
    assert rc == D3DP_ENOTSUP and msg == TODAY[mode], (rc, msg)
    assert reached_the_device_check(*create(512, mode))
