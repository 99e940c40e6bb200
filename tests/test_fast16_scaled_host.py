"""No GPU needed: what d3dp_create answers to D3DP_FAST16_RANGE=scale (the opt-in FAST16 route that lowers a block's power-of-two
operand scales where the proven bound reaches 65504, instead of moving the context to bf16) is decided before the device is looked
for, so a machine without one sees every refusal -- the switch is never ignored -- and sees the shapes the switch takes get as far
as the device check.  The form of test_fast_widths_host.py."""
import pytest

from create_host import D3DP_ENOTSUP, create, reached_the_device_check
from d3dp_amd import _lib

SWITCH = "D3DP_FAST16_RANGE=scale"
OTHER_MODES = [_lib.MODE_FAST, _lib.MODE_EXACT, _lib.MODE_TRAIN]


@pytest.mark.parametrize("cs", [128, 256, 512])
def test_the_switch_passes_at_head_dims_16_32_and_64(monkeypatch, cs):
    monkeypatch.setenv("D3DP_FAST16_RANGE", "scale")
    assert reached_the_device_check(*create(cs, _lib.MODE_FAST16))
    assert reached_the_device_check(*create(cs, _lib.MODE_FAST16, frames=288))      # (the chunked-key attention kernel)
    assert reached_the_device_check(*create(cs, _lib.MODE_FAST16, joints=40))       # (the spatial axis on the whole-sequence kernel)


@pytest.mark.parametrize("value", ["", "1", "on", "Scale", "scale ", "bf16"])
@pytest.mark.parametrize("cs", [64, 512])
def test_another_value_of_the_variable_is_refused(monkeypatch, cs, value):
    monkeypatch.setenv("D3DP_FAST16_RANGE", value)
    rc, msg = create(cs, _lib.MODE_FAST16)
    assert rc == D3DP_ENOTSUP and SWITCH in msg, (rc, msg)


def test_head_dim_8_is_refused(monkeypatch):
    monkeypatch.setenv("D3DP_FAST16_RANGE", "scale")
    rc, msg = create(64, _lib.MODE_FAST16)
    assert rc == D3DP_ENOTSUP and SWITCH in msg and "head dim 8" in msg, (rc, msg)
    rc, msg = create(128, _lib.MODE_FAST16, heads=16)
    assert rc == D3DP_ENOTSUP and SWITCH in msg and "head dim 8" in msg, (rc, msg)
    assert reached_the_device_check(*create(64, _lib.MODE_FAST16, heads=4))         # (head dim 16 at the narrowest width)
    monkeypatch.delenv("D3DP_FAST16_RANGE")
    assert reached_the_device_check(*create(64, _lib.MODE_FAST16))                  # (without the switch: as before)


@pytest.mark.parametrize("cs", [128, 512])
def test_the_row_attention_switch_is_refused_beside_it(monkeypatch, cs):
    monkeypatch.setenv("D3DP_FAST16_RANGE", "scale")
    monkeypatch.setenv("D3DP_LONG_ATTN", "rows")
    rc, msg = create(cs, _lib.MODE_FAST16)
    assert rc == D3DP_ENOTSUP and SWITCH in msg and "D3DP_LONG_ATTN=rows" in msg, (rc, msg)
    monkeypatch.delenv("D3DP_FAST16_RANGE")
    assert reached_the_device_check(*create(cs, _lib.MODE_FAST16))                  # (the cross-check alone: as before)


@pytest.mark.parametrize("cs", [192, 320, 384, 448])
def test_the_padded_widths_are_refused_beside_it(monkeypatch, cs):
    monkeypatch.setenv("D3DP_FAST16_RANGE", "scale")
    monkeypatch.setenv("D3DP_FAST_IMPL", "mfma")
    rc, msg = create(cs, _lib.MODE_FAST16)
    assert rc == D3DP_ENOTSUP and SWITCH in msg and "D3DP_FAST_IMPL=mfma" in msg and f"channels={cs}" in msg, (rc, msg)
    assert reached_the_device_check(*create(512, _lib.MODE_FAST16))                 # (an instantiated width: mfma names the default)
    monkeypatch.delenv("D3DP_FAST16_RANGE")
    assert reached_the_device_check(*create(cs, _lib.MODE_FAST16))                  # (the padded route alone: as before)


def test_a_hidden_width_without_a_scaled_linear_is_refused(monkeypatch):
    """The scaled streaming Linear exists at the k-depths of the instantiated widths: K / 64 in {1, 2, 4, 8, 16}."""
    monkeypatch.setenv("D3DP_FAST16_RANGE", "scale")
    rc, msg = create(512, _lib.MODE_FAST16, hidden=768)
    assert rc == D3DP_ENOTSUP and SWITCH in msg and "hidden=768" in msg, (rc, msg)
    for hidden in (64, 128, 256, 512, 1024):
        assert reached_the_device_check(*create(512, _lib.MODE_FAST16, hidden=hidden))


@pytest.mark.parametrize("value", ["scale", "bf16", ""])
@pytest.mark.parametrize("mode", OTHER_MODES)
def test_fast_exact_and_train_contexts_do_not_read_the_variable(monkeypatch, mode, value):
    """Every answer with the variable set -- to its value or to one a FAST16 context refuses -- is the answer without it, beside
    the switches those modes do read."""
    def answers():
        out = [create(cs, mode) for cs in (64, 128, 512, 384)]
        out.append(create(512, mode, hidden=768))
        with monkeypatch.context() as mp:
            mp.setenv("D3DP_LONG_ATTN", "rows")
            out.append(create(512, mode))
            mp.setenv("D3DP_FAST_IMPL", "mfma")
            out.append(create(384, mode))
        return out

    monkeypatch.delenv("D3DP_FAST16_RANGE", raising=False)
    without = answers()
    monkeypatch.setenv("D3DP_FAST16_RANGE", value)
    assert answers() == without
    assert all(SWITCH not in msg for _, msg in without)
    assert reached_the_device_check(*without[2])
