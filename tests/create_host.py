"""What the host tests of d3dp_create share (tests/test_*_host.py; no GPU needed): create one context through the C ABI and say
whether the request got past every refusal that is decided before the device is looked for."""
import ctypes as C

from d3dp_amd import _lib

D3DP_OK, D3DP_ENOTSUP, D3DP_EHIP = 0, -2, -3


def create(cs, mode, frames=9, joints=5, heads=8, hidden=None):
    """-> (return code, message); a context that was created is destroyed again."""
    lib = _lib.load()
    cfg = _lib.Cfg(frames, joints, cs, 1, heads, 2 * cs if hidden is None else hidden, 1e-6, 1e-5, mode, 0)
    h = C.c_void_p()
    rc = lib.d3dp_create(C.byref(cfg), C.byref(h))
    msg = lib.d3dp_last_error().decode() if rc != D3DP_OK else ""
    if rc == D3DP_OK:
        lib.d3dp_destroy(h)
    return rc, msg


def reached_the_device_check(rc, msg):
    return rc == D3DP_OK or (rc == D3DP_EHIP and "no HIP device" in msg)
