"""No GPU needed: what d3dp_create answers to D3DP_EXACT_IMPL=f16x2 (the opt-in split-fp16 implementation with padded heads at
channels 192 / 320 / 384 / 448) is decided before the device is looked for, so a machine without one sees every refusal -- a switch
is never ignored -- and sees the shapes the switch takes get as far as the device check."""
import pytest

from create_host import D3DP_ENOTSUP, create, reached_the_device_check
from d3dp_amd import _lib

SWITCH = "D3DP_EXACT_IMPL=f16x2"


@pytest.mark.parametrize("cs", [96, 224, 576, 1024])
def test_the_switch_is_refused_at_widths_it_has_no_kernels_for(monkeypatch, cs):
    """Head dims 12 and 28 are no multiple of 8; 72 and 128 exceed 64 (and fc1's columns the Linear's bias area)."""
    monkeypatch.setenv("D3DP_EXACT_IMPL", "f16x2")
    rc, msg = create(cs, _lib.MODE_EXACT)
    assert rc == D3DP_ENOTSUP and SWITCH in msg and f"channels={cs}" in msg, (rc, msg)


@pytest.mark.parametrize("mode", [_lib.MODE_TRAIN, _lib.MODE_FAST, _lib.MODE_FAST16])
def test_the_switch_is_refused_in_other_modes_at_its_widths(monkeypatch, mode):
    monkeypatch.setenv("D3DP_EXACT_IMPL", "f16x2")
    rc, msg = create(384, mode)
    assert rc == D3DP_ENOTSUP and SWITCH in msg, (rc, msg)


@pytest.mark.parametrize("cs", [192, 320, 384, 448, 512])
def test_the_switch_passes_at_its_widths_and_at_an_instantiated_one(monkeypatch, cs):
    monkeypatch.setenv("D3DP_EXACT_IMPL", "f16x2")
    assert reached_the_device_check(*create(cs, _lib.MODE_EXACT))
    if cs == 512:                                            # (there the value names the default: every mode as without it)
        assert reached_the_device_check(*create(cs, _lib.MODE_TRAIN))


def test_bf16x3_keeps_its_refusal(monkeypatch):
    """(decided before the device is looked for, like every refusal of d3dp_create: a machine without a GPU sees it too)"""
    monkeypatch.setenv("D3DP_EXACT_IMPL", "bf16x3")
    rc, msg = create(384, _lib.MODE_EXACT)
    assert rc == D3DP_ENOTSUP and "D3DP_EXACT_IMPL=bf16x3 exists for channels in {64,128,256,512}" in msg, (rc, msg)


def test_the_row_attention_switch_is_refused_beside_it(monkeypatch):
    monkeypatch.setenv("D3DP_EXACT_IMPL", "f16x2")
    monkeypatch.setenv("D3DP_LONG_ATTN", "rows")
    rc, msg = create(384, _lib.MODE_EXACT)
    assert rc == D3DP_ENOTSUP and "D3DP_LONG_ATTN=rows" in msg and SWITCH in msg, (rc, msg)
    assert reached_the_device_check(*create(512, _lib.MODE_EXACT))     # (an instantiated width: the cross-check as before)


def test_without_the_switch_nothing_moves(monkeypatch):
    monkeypatch.delenv("D3DP_EXACT_IMPL", raising=False)
    assert reached_the_device_check(*create(384, _lib.MODE_EXACT))
    assert reached_the_device_check(*create(96, _lib.MODE_EXACT))
    rc, msg = create(384, _lib.MODE_FAST)
    assert rc == D3DP_ENOTSUP and "FAST contexts exist" in msg, (rc, msg)
