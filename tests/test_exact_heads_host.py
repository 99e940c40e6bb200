"""No GPU needed: d3dp_op_attention with impl 2 (the EXACT split-fp16 kernels) checks the head dim before it touches the device --
before the stream-ordered temporary is allocated and the repack kernel launched -- so the refusal of a head dim other than 64, 32
or 16 is visible on a machine without one, by name."""
import ctypes

import pytest

from d3dp_amd import _lib

D3DP_ENOTSUP = -2


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("C,hd", [(64, 8), (384, 48), (1024, 128)])
def test_impl_2_refuses_other_head_dims_before_any_device_call(C, hd, axis):
    lib = _lib.load()
    rows = (ctypes.c_float * 16)()                       # never read: the refusal comes first
    p = ctypes.addressof(rows)
    assert lib.d3dp_op_attention(0, 2, axis, p, p, 1, 9, 5, C, 8, None) == D3DP_ENOTSUP
    msg = lib.d3dp_last_error().decode()
    assert f"head dim {hd}" in msg and "64, 32 and 16" in msg, msg
