"""No GPU needed: what d3dp_create answers to D3DP_TRAIN_IMPL=f16x2 (the opt-in split-fp16 training step at channels 192 / 320 /
384 / 448) is decided before the device is looked for, so a machine without one sees every refusal -- a switch is never ignored --
and sees the shapes the switch takes get as far as the device check; what MixSTE2.train_arithmetic() says about the route; and
that every case of tests/test_hip_train_widths.py is well-conditioned by the reference's own measure (oracle/grad_check.py)."""
from types import SimpleNamespace

import pytest

from create_host import D3DP_ENOTSUP, create, reached_the_device_check
from d3dp_amd import D3DP, _lib
from d3dp_amd.weights import H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT
from oracle import grad_check as gc
from test_hip_train_grads import DROPPED_PARAMS, reference
from test_hip_train_widths import ALL_CASES, DROPPED

SWITCH = "D3DP_TRAIN_IMPL=f16x2"
LDS_REFUSAL = "holds a whole sequence in LDS"


def switches(monkeypatch, train_impl=None):
    for k in ("D3DP_TRAIN_IMPL", "D3DP_TRAIN_ATTN", "D3DP_EXACT_IMPL", "D3DP_LONG_ATTN"):
        monkeypatch.delenv(k, raising=False)
    if train_impl:
        monkeypatch.setenv("D3DP_TRAIN_IMPL", train_impl)


@pytest.mark.parametrize("cs", [96, 224, 576, 1024])
def test_the_switch_is_refused_at_widths_it_has_no_kernels_for(monkeypatch, cs):
    """Head dims 12 and 28 are no multiple of 8; 72 and 128 exceed 64.  (Without the switch these widths train on the fp32 path.)"""
    switches(monkeypatch, "f16x2")
    rc, msg = create(cs, _lib.MODE_TRAIN)
    assert rc == D3DP_ENOTSUP and SWITCH in msg and f"channels={cs}" in msg, (rc, msg)
    switches(monkeypatch)
    assert reached_the_device_check(*create(cs, _lib.MODE_TRAIN))


@pytest.mark.parametrize("cs", [192, 320, 384, 448, 512])
def test_the_switch_passes_at_its_widths_and_at_an_instantiated_one(monkeypatch, cs):
    switches(monkeypatch, "f16x2")
    assert reached_the_device_check(*create(cs, _lib.MODE_TRAIN))


def test_the_switch_lifts_the_clip_length_limit_of_the_fp32_attention(monkeypatch):
    switches(monkeypatch, "f16x2")
    assert reached_the_device_check(*create(384, _lib.MODE_TRAIN, frames=300))
    assert reached_the_device_check(*create(192, _lib.MODE_TRAIN, frames=1024))
    rc, msg = create(384, _lib.MODE_TRAIN, frames=1025)
    assert rc == D3DP_ENOTSUP and "frames=1025" in msg, (rc, msg)
    switches(monkeypatch)
    rc, msg = create(384, _lib.MODE_TRAIN, frames=300)
    assert rc == D3DP_ENOTSUP and LDS_REFUSAL in msg and "channels=384" in msg, (rc, msg)


def test_contexts_of_other_modes_do_not_read_the_switch(monkeypatch):
    """The reference keeps a train and an eval model alive in one process: an EXACT context, or a FAST refusal, is what it is
    without the switch -- also at a width where a TRAIN context is refused."""
    switches(monkeypatch, "f16x2")
    assert reached_the_device_check(*create(384, _lib.MODE_EXACT))
    assert reached_the_device_check(*create(96, _lib.MODE_EXACT))
    rc, msg = create(384, _lib.MODE_FAST)
    assert rc == D3DP_ENOTSUP and "FAST contexts exist" in msg and SWITCH not in msg, (rc, msg)
    rc, msg = create(384, _lib.MODE_FAST16)
    assert rc == D3DP_ENOTSUP and "FAST16 contexts exist" in msg and SWITCH not in msg, (rc, msg)


def test_the_fp32_value_of_the_switch_behaves_as_before(monkeypatch):
    switches(monkeypatch, "f32")
    for cs in (384, 96, 512):
        assert reached_the_device_check(*create(cs, _lib.MODE_TRAIN))
    rc, msg = create(384, _lib.MODE_TRAIN, frames=300)
    assert rc == D3DP_ENOTSUP and LDS_REFUSAL in msg, (rc, msg)


def test_the_exact_switch_beside_it_keeps_refusing_a_train_context(monkeypatch):
    """(tests/test_exact_widths_host.py pins the refusal; the two switches are set around the creation of their own contexts)"""
    switches(monkeypatch, "f16x2")
    monkeypatch.setenv("D3DP_EXACT_IMPL", "f16x2")
    rc, msg = create(384, _lib.MODE_TRAIN)
    assert rc == D3DP_ENOTSUP and "D3DP_EXACT_IMPL=f16x2" in msg, (rc, msg)
    assert reached_the_device_check(*create(384, _lib.MODE_EXACT))


def arithmetic(cs, frames=27):
    args = SimpleNamespace(number_of_frames=frames, test_time_augmentation=True, timestep=1000, scale=1.0, cs=cs, dep=2)
    return D3DP(args, H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, is_train=True).pose_estimator.train_arithmetic()


def test_train_arithmetic_names_the_route(monkeypatch):
    both = "attention of both axes, forward and backward, on split-fp16 operands"
    switches(monkeypatch, "f16x2")
    text = arithmetic(384)
    assert SWITCH in text and "split-fp16 Linears" in text and both in text and "head dim 48 padded to 64" in text, text
    assert "head dim 24 padded to 32" in arithmetic(192)
    monkeypatch.setenv("D3DP_TRAIN_ATTN", "f32")
    text = arithmetic(384)
    assert SWITCH in text and "fp32 attention" in text and both not in text, text
    switches(monkeypatch, "f16x2")
    assert SWITCH not in arithmetic(512) and SWITCH not in arithmetic(96)      # (the default there / no such route there)
    switches(monkeypatch)
    text = arithmetic(384)
    assert "fp32 path of a width outside" in text and SWITCH not in text, text


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.id)
def test_every_gpu_case_is_admissible(case):
    """e32 -- the oracle's fp32 autograd against its fp64 autograd -- is at most 2e-6 (norm) and 5e-5 (per element); the dropped-branch
    cases have their 12 exactly-zero fp64 gradients; the fp32 oracle passes its own check."""
    ref = reference(case)
    print(f"{case.id}: e32 norm_rel {ref.e32[0]:.2e}, max_rms {ref.e32[1]:.2e}")
    assert ref.e32[0] <= gc.ADMIT_NORM_REL and ref.e32[1] <= gc.ADMIT_MAX_RMS, ref.e32
    zeros = sorted(n for n, g in ref.g64.items() if not g.any())
    assert zeros == (sorted(DROPPED_PARAMS) if case in DROPPED else []), zeros
    assert not gc.violations(gc.grad_errors(ref.g32, ref.g64), ref.e32)
