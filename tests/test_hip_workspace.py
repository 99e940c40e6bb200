"""The caller's workspaces (include/d3dp_hip.h d3dp_workspace_bytes / d3dp_train_workspace_bytes): a call runs in exactly the
byte count its size query returns, writes nothing outside it, computes what it computes in a roomier one, and refuses a
smaller one before it writes anything.  The size query and the carve come from one layout each (capi_denoise.hip InferLayout,
train_plan.h TrainLayout); the shapes are the smallest that reach each branch of the two.

Every workspace lies inside a larger torch byte buffer with a 4,096-byte guard of a fixed pattern on each side: an overrun
changes bytes of an allocation the test owns.
"""
import importlib.util
import os

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("lib_ab_hash", os.path.join(REPO, "tools", "lib_ab_hash.py"))
ab = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ab)

pytestmark = pytest.mark.gpu
GUARD, PATTERN, ESTATE = 4096, 0xA5, -4
F, J = 9, 5


class Guarded:
    """`n` workspace bytes between two guards."""

    def __init__(self, n):
        self.n, self.buf = n, torch.full((n + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD
        assert self.ptr % 256 == 0

    def intact(self):
        torch.cuda.synchronize()
        return bool((self.buf[:GUARD] == PATTERN).all()) and bool((self.buf[GUARD + self.n:] == PATTERN).all())


INFER_CASES = [
    pytest.param("exact", 512, 0, 2, id="exact-c512"),          # the deferred norm at d = 1: the nstat region
    pytest.param("exact", 128, 0, 2, id="exact-c128"),
    pytest.param("exact", 64, 0, 2, id="exact-c64"),            # C < 96: no deferred norm, no nstat
    pytest.param("exact", 96, 0, 2, id="exact-c96"),            # the run-time-width fp32 implementation
    pytest.param("fast", 512, 0, 2, id="fast-c512"),
    pytest.param("fast16", 256, 0, 2, id="fast16-c256"),
    pytest.param("exact", 512, 2, 5, id="exact-c512-passes"),   # sized for a pass of 2 sequences, not for the 5: passes 2, 2, 1
    pytest.param("exact", 512, 0, 2, id="exact-c512-fold-ln", marks=pytest.mark.variants),   # D3DP_FOLD_LN=1: the lnst regions
]


@pytest.mark.parametrize("mode,cs,chunk_seqs,H", INFER_CASES)
def test_denoise_workspace(mode, cs, chunk_seqs, H, request, monkeypatch):
    if "variants" in request.keywords:
        monkeypatch.setenv("D3DP_FOLD_LN", "1")
    B = 1
    c = ab.RawCtx(mode, cs, F, J, 2, chunk_seqs)
    n = c.infer_bytes(B, H)
    inputs = c.infer_inputs(B, H)
    tight, roomy = Guarded(n), Guarded(2 * n)
    out = torch.empty(B, H, F, J, 3, device="cuda")
    ref = torch.empty_like(out)
    assert c.denoise(inputs, out, B, H, tight.ptr, n) == 0, c.lib.d3dp_last_error()
    assert tight.intact()
    assert c.denoise(inputs, ref, B, H, roomy.ptr, 2 * n) == 0, c.lib.d3dp_last_error()
    assert roomy.intact()
    assert torch.isfinite(out).all() and torch.equal(out, ref)
    kept = torch.full_like(out, 7.0)
    assert c.denoise(inputs, kept, B, H, tight.ptr, n - 256) == ESTATE
    assert tight.intact() and bool((kept == 7.0).all())


@pytest.mark.parametrize("cs", [64, 256])                       # 256: the width at which the direct LayerNorm operands apply
def test_train_workspace(cs):
    B = 2
    c = ab.RawCtx("train", cs, F, J, 1)
    n = c.train_bytes(B)
    inputs = c.train_inputs(B)
    res = []
    for ws in (Guarded(n), Guarded(2 * n)):
        out, grads = torch.empty(B, F, J, 3, device="cuda"), c.grad_buffers()
        assert c.train_forward(inputs, out, B, ws.ptr, ws.n) == 0, c.lib.d3dp_last_error()
        assert c.train_backward(inputs, grads, B, ws.ptr, ws.n) == 0, c.lib.d3dp_last_error()
        assert ws.intact()
        res.append((out, c.flat_grads(grads)))
    (out, grads), (ref, ref_grads) = res
    assert torch.isfinite(out).all() and torch.equal(out, ref)
    for i, (g, r) in enumerate(zip(grads, ref_grads)):
        assert torch.isfinite(g).all() and torch.equal(g, r), f"gradient {i}"
    tight = Guarded(n)
    kept, kept_grads = torch.full_like(out, 7.0), c.grad_buffers(fill=7.0)
    assert c.train_forward(inputs, kept, B, tight.ptr, n - 256) == ESTATE
    assert c.train_backward(inputs, kept_grads, B, tight.ptr, n - 256) == ESTATE
    assert tight.intact() and bool((kept == 7.0).all())
    assert all(bool((g == 7.0).all()) for g in c.flat_grads(kept_grads))
