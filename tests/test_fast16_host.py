"""numerics='fast16' (D3DP_MODE_FAST16, ABI v5) as far as a host without a GPU can see it: the mode's name reaches the C ABI from
the Python argument, the environment and the command line; d3dp_create takes it for exactly the shapes it takes FAST for and names
FAST16 where it refuses; d3dp_fast_operands is declared, exported and bound."""
import ctypes as C
import os
import re

import pytest

from d3dp_amd import _lib, cli
from d3dp_amd.model import MixSTE2, _resolve_mode

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    return _lib.load()


def test_fast16_is_a_numerics_name(monkeypatch):
    monkeypatch.delenv("D3DP_NUMERICS", raising=False)
    assert _lib.MODE_FAST16 == 3 and _lib.ABI_VERSION == 5
    assert _resolve_mode("fast16") == _lib.MODE_FAST16
    assert _resolve_mode("FAST16") == _lib.MODE_FAST16
    assert _resolve_mode("fast") == _lib.MODE_FAST and _resolve_mode(None) == _lib.MODE_EXACT     # (the others keep their meaning)
    monkeypatch.setenv("D3DP_NUMERICS", "fast16")
    assert _resolve_mode(None) == _lib.MODE_FAST16
    assert _resolve_mode("exact") == _lib.MODE_EXACT                 # (an argument beats the environment)
    for bad in ("fast32", "fp16", "fast16 "):
        with pytest.raises(ValueError):
            _resolve_mode(bad)


def test_model_reports_and_switches_to_fast16():
    m = MixSTE2(num_frame=9, num_joints=17, embed_dim_ratio=64, depth=1, is_train=False, numerics="fast16")
    assert m.numerics == "fast16"
    m.set_numerics("fast")
    assert m.numerics == "fast"
    m.set_numerics("fast16")
    assert m.numerics == "fast16" and m._mode == _lib.MODE_FAST16
    assert callable(m.fast_operands)


def test_create_takes_fast16_for_the_shapes_it_takes_fast_for(lib):
    """The form of tests/test_abi.py::test_create_validates_widths_and_joints_before_it_looks_for_a_device: an accepted shape gets as
    far as the device check (-3 on a host without a GPU; with one the context is made, and destroyed here), a refusal is
    D3DP_ENOTSUP (-2) with a reason that names FAST16."""
    def create(frames, joints, cs, heads, hidden, mode):
        cfg = _lib.Cfg(frames, joints, cs, 8, heads, hidden, 1e-6, 1e-5, mode, 0)
        h = C.c_void_p()
        rc, msg = lib.d3dp_create(C.byref(cfg), C.byref(h)), lib.d3dp_last_error().decode()
        if rc == 0:                          # (a GPU is visible: the shape was accepted and the context exists)
            lib.d3dp_destroy(h)
            rc = -3
        return rc, msg

    for cs in (64, 128, 256, 512):
        for joints in (17, 40, 256):
            assert create(27, joints, cs, 8, 2 * cs, _lib.MODE_FAST16)[0] == -3, (cs, joints)
    assert create(351, 17, 512, 8, 1024, _lib.MODE_FAST16)[0] == -3                # a clip beyond the MFMA attention kernels
    for cs in (96, 384, 1024):
        rc, msg = create(27, 17, cs, 8, 2 * cs, _lib.MODE_FAST16)
        assert rc == -2 and "FAST16" in msg, msg
        rc, msg = create(27, 17, cs, 8, 2 * cs, _lib.MODE_FAST)                    # (FAST's own message is unchanged)
        assert rc == -2 and "FAST contexts exist" in msg and "FAST16" not in msg, msg
    rc, msg = create(27, 17, 512, 8, 1024, 4)                                      # no such mode
    assert rc == -1 and "mode=4" in msg


def test_command_lines_take_fast16():
    assert cli.parse_args(["--numerics", "fast16"]).numerics == "fast16"
    assert cli.parse_args(["--numerics", "fast"]).numerics == "fast"
    with pytest.raises(SystemExit):
        cli.parse_args(["--numerics", "fast8"])


def test_fast_operands_is_declared_exported_and_bound(lib):
    hdr = open(os.path.join(REPO, "include", "d3dp_hip.h")).read()
    assert re.search(r"^D3DP_API int d3dp_fast_operands\(const d3dp_ctx\* ctx, int32_t\* type, float\* bound\);", hdr, flags=re.M)
    assert "D3DP_MODE_FAST16 = 3" in hdr and "#define D3DP_ABI_VERSION 5" in hdr
    assert hdr.index("d3dp_fast_operands(const") < hdr.index("---- test hooks")      # not a test hook
    assert "d3dp_fast_operands" in _lib.PROTOTYPES
    assert "stream" not in hdr[hdr.index("D3DP_API int d3dp_fast_operands"):].split(";")[0]
    assert hasattr(lib, "d3dp_fast_operands") and lib.d3dp_abi_version() == 5
    t, b = C.c_int32(), C.c_float()
    assert lib.d3dp_fast_operands(None, C.byref(t), C.byref(b)) == -1               # null context: D3DP_EINVAL, no crash
