"""No GPU needed: the step table of the native sampler -- plan_ddim_steps() of d3dp_amd/csrc/sampler_plan.h, what d3dp_ddim_steps
returns -- against D3DP.time_pairs() and the coefficient arithmetic of d3dp_amd/model.py, bit for bit, through a stand-alone driver
(tests/sampler_plan_driver.cpp).  Doubles are compared as the int64 of their bits, floats as the int32 of theirs."""
import ctypes as C
import math
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from d3dp_amd import D3DP, _lib
from d3dp_amd.weights import H36M_JOINTS_LEFT as KL, H36M_JOINTS_RIGHT as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
CASES = {1000: list(range(1, 65)), 50: [1, 7, 50]}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("sampler_plan") / "driver")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "sampler_plan_driver.cpp"), "-o", exe], check=True)
    return exe


def model(T):
    args = SimpleNamespace(number_of_frames=9, test_time_augmentation=True, timestep=T, scale=1.0, cs=64, dep=1)
    return D3DP(args, KL, KR, is_train=False, num_proposals=1, sampling_timesteps=1, numerics="exact")


def run(driver, tmp_path, ac, lines, buffers=()):
    paths = []
    for i, a in enumerate((ac,) + tuple(buffers)):
        paths.append(str(tmp_path / f"buf{i}.f64"))
        np.ascontiguousarray(a, dtype=np.float64).tofile(paths[-1])
    out = subprocess.run([driver, *paths], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True).stdout
    rows = [r.split("\t") for r in out.split("\n")[:-1]]
    assert len(rows) == len(lines), out
    return [(int(r[0]), r[1], [tuple(int(v) for v in f.split(":")) for f in r[2:]]) for r in rows]


def i64(x):
    return int(np.array(x, dtype=np.float64).view(np.int64))


def i32(x):
    return int(np.array(x, dtype=np.float64).astype(np.float32).view(np.int32))     # (one rounding to float, as ctypes.c_float)


def expected(m, K, eta, buffers=True):
    """Every field of every step as d3dp_amd/model.py forms it: ddim_sample_flip's Python doubles (math.sqrt, **), rounded to
    float where the C ABI takes a float, and the two buffers it reads.  buffers=False: the correctly rounded sqrt in their place
    (numpy's), what the table holds for a host without the buffers.  c_noise64 is ddim_sample's expression
    (1 - alpha_next - sigma ** 2).sqrt() in correctly rounded fp64 operations, which is what the DEVICE gives its fp64 tensors --
    torch's CPU sqrt is not correctly rounded, so a CPU tensor is no reference for it; tests/test_hip_sampler_native.py holds the
    table to the device's own values."""
    m.sampling_timesteps, m.ddim_sampling_eta = K, eta
    sch = m._sched()
    ac = sch["alphas_cumprod"]
    rows = []
    for time, time_next in m.time_pairs():
        last = time_next < 0
        if last:
            c_x, c_n, sg, c64 = 0.0, 0.0, 0.0, 0.0
        else:
            alpha, alpha_next = ac[time], ac[time_next]
            sg = eta * math.sqrt((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha))
            c_n = math.sqrt(1 - alpha_next - sg ** 2)
            c_x = math.sqrt(alpha_next)
            c64 = float(np.sqrt(np.float64(1) - np.float64(alpha_next) - np.float64(sg) * np.float64(sg)))
        if buffers:
            sr, srm1 = float(sch["sqrt_recip_alphas_cumprod"][time]), float(sch["sqrt_recipm1_alphas_cumprod"][time])
        else:
            sr, srm1 = float(np.sqrt(np.float64(1) / ac[time])), float(np.sqrt(np.float64(1) / ac[time] - np.float64(1)))
        rows.append((time, i64(sr), i64(srm1), i32(c_x), i32(c_n), i32(sg), int(last), i64(c64)))
    return rows


NAMES = ("t", "sqrt_recip", "sqrt_recipm1", "c_xstart", "c_noise", "sigma", "last", "c_noise64")


@pytest.mark.parametrize("T", list(CASES))
@pytest.mark.parametrize("eta", [1.0, 0.5])
@pytest.mark.parametrize("buffers", [True, False], ids=["module-buffers", "computed-sqrt"])
def test_step_table_equals_the_python_sampler_bit_for_bit(driver, tmp_path, T, eta, buffers):
    m = model(T)
    bufs = (m.sqrt_recip_alphas_cumprod.numpy(), m.sqrt_recipm1_alphas_cumprod.numpy()) if buffers else ()
    got = run(driver, tmp_path, m.alphas_cumprod.numpy(), [f"{K} {eta!r}" for K in CASES[T]], bufs)
    bad = []
    for K, (rc, msg, rows) in zip(CASES[T], got):
        assert rc == 0, (K, msg)
        want = expected(m, K, eta, buffers)
        assert len(rows) == K
        assert [r[6] for r in rows] == [0] * (K - 1) + [1], K                       # `last` exactly once, at the end
        bad += [f"T={T} K={K} step {k}: {n} {g} != {w}" for k, (gr, wr) in enumerate(zip(rows, want))
                for n, g, w in zip(NAMES, gr, wr) if g != w]
    assert not bad, "\n".join(bad[:20])


def test_why_the_table_takes_the_buffers():
    """torch's CPU sqrt of an fp64 tensor is not correctly rounded: the cosine schedule's own buffers differ from sqrt() in the
    last bit at a few timesteps, never by more."""
    m = model(1000)
    ac = m.alphas_cumprod.numpy()
    for buf, ref in ((m.sqrt_recip_alphas_cumprod, np.sqrt(1.0 / ac)), (m.sqrt_recipm1_alphas_cumprod, np.sqrt(1.0 / ac - 1))):
        d = np.abs(buf.numpy().view(np.int64) - ref.view(np.int64))
        print("entries of 1000 that differ from the correctly rounded sqrt:", int((d != 0).sum()))
        assert d.max() <= 1


def test_refusals(driver, tmp_path):
    m = model(50)
    got = run(driver, tmp_path, m.alphas_cumprod.numpy(), ["51 1.0", "0 1.0", "-3 1.0", "50 1.0",
                                                           "check 3 0 0 1", "check 3 0 1 1", "check 3 0 0 0", "check 3 1 0 1", "check 0",
                                                           "check 1 1", "check 1 0"])
    (rc, msg, _) = got[0]
    assert rc == EINVAL and "K = 51" in msg and "T = 50" in msg, msg
    for rc, msg, _ in got[1:3]:
        assert rc == EINVAL and "K = " in msg, msg
    assert got[3][0] == 0
    assert got[4][0] == 0 and got[9][0] == 0
    for i, needle in ((5, "steps[1].last"), (6, "steps[2].last"), (7, "steps[0].last"), (8, "K = 0"), (10, "steps[0].last")):
        assert got[i][0] == EINVAL and needle in got[i][1], got[i]


def test_the_library_exports_the_same_table():
    """d3dp_ddim_steps of the built library is that function (no device is touched)."""
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    lib = _lib.load()
    m = model(1000)
    ac = np.ascontiguousarray(m.alphas_cumprod.numpy(), dtype=np.float64)
    for K in (1, 5, 10):
        steps = (_lib.DdimStep * K)()
        assert lib.d3dp_ddim_steps(ac.ctypes.data_as(C.POINTER(C.c_double)), 1000, K, 1.0, steps) == 0
        fields = lambda table: [(s.t, i64(s.sqrt_recip), i64(s.sqrt_recipm1), i32(s.c_xstart), i32(s.c_noise), i32(s.sigma), s.last,
                                 i64(s.c_noise64)) for s in table]
        assert fields(steps) == expected(m, K, 1.0, buffers=False)
        m.sampling_timesteps = K
        assert fields(m._steps()) == expected(m, K, 1.0, buffers=True)               # (the module's table: its own buffers)
    assert lib.d3dp_ddim_steps(ac.ctypes.data_as(C.POINTER(C.c_double)), 1000, 1001, 1.0, steps) == EINVAL
    assert b"K = 1001" in lib.d3dp_last_error()
