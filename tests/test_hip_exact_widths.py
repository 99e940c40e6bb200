"""GPU tests of D3DP_EXACT_IMPL=f16x2 at channels 192 / 320 / 384 / 448 (head dims 24, 40, 48, 56 with the model's 8 heads): EXACT
mode on the split-fp16 Linears and the matrix-core attention kernels at widths outside the instantiated set, opt-in.  The head dim
is padded to 32 / 64 inside the packed weights (zero rows of the qkv matrix and bias, zero columns of proj), the attention kernels
run their head dim 32 / 64 instantiations with the true head dim in the softmax exponent, and the LayerNorms run the run-time-width
row kernels with split-fp16 rows out (pointwise.hip *_h_kernel).  Without the switch such a context launches what it launched
before: the fp32 implementation.

  1. sampler parity at the four widths, with and without the switch, against the fp32 oracle at EXACT mode's 1e-3 mm;
  2. the three attention kernels behind padded heads;
  3. pad columns never leak: a workspace of NaN patterns against a zeroed one, bit for bit;
  4. any pass split and any two runs give the same bits;
  5. D3DP_NO_FOLD=1 changes no bit;
  6. the range proof: a lowered q/k/v scale stays on f16x2, a LayerNorm out of range lands on the fp32 implementation;
  7. the call runs in exactly d3dp_workspace_bytes;
  8. the row kernels alone against an fp64 LayerNorm.
"""
import importlib.util
import os
from types import SimpleNamespace

import pytest
import torch

from d3dp_amd import D3DP, _lib
from d3dp_amd.model import MixSTE2
from d3dp_amd.weights import (H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, flip_2d, make_state_dict, synthetic_inputs_2d,
                              synthetic_noise)
from oracle import d3dp_oracle as orc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("lib_ab_hash", os.path.join(REPO, "tools", "lib_ab_hash.py"))
ab = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ab)

pytestmark = pytest.mark.gpu
EXACT_TOL_MM = 1e-3          # the project's EXACT gate
WIDTHS = [192, 320, 384, 448]


def switch(monkeypatch, on):
    """Read by d3dp_create, i.e. at the first call of a model made after this."""
    if on:
        monkeypatch.setenv("D3DP_EXACT_IMPL", "f16x2")
    else:
        monkeypatch.delenv("D3DP_EXACT_IMPL", raising=False)


def sampler(sd, frames, cs, dep, H, K):
    args = SimpleNamespace(number_of_frames=frames, test_time_augmentation=True, timestep=1000, scale=1.0, cs=cs, dep=dep)
    m = D3DP(args, H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, is_train=False, num_proposals=H, sampling_timesteps=K, numerics="exact")
    m.load_state_dict(sd, strict=False)
    return m.cuda().eval()


def sample(m, x2d, noises):
    return m(torch.from_numpy(x2d).cuda(), None, input_2d_flip=torch.from_numpy(flip_2d(x2d)).cuda(), noise=noises)


def oracle_sample(sd, x2d, noises, H, K, dep):
    return orc.ddim_sample_flip(orc.strip_prefix(sd), orc.cosine_schedule(1000), torch.from_numpy(x2d), torch.from_numpy(flip_2d(x2d)),
                                H, K, dep, H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, noises)


def denoiser(sd, frames, joints, cs, dep, chunk_seqs=0):
    m = MixSTE2(num_frame=frames, num_joints=joints, embed_dim_ratio=cs, depth=dep, is_train=False, numerics="exact",
                drop_path_rate=0.0, chunk_seqs=chunk_seqs)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


def denoiser_case(seed, frames, joints, cs, dep, B, H):
    sd = make_state_dict(seed, cs, dep, frames, prefix="", joints=joints)
    g = torch.Generator().manual_seed(seed * 1000 + cs + frames)
    x2d = torch.rand(B, frames, joints, 2, generator=g) * 2 - 1
    x3d = torch.randn(B, H, frames, joints, 3, generator=g)
    t = torch.tensor([(999 - 379 * b) % 1000 for b in range(B)])
    return sd, x2d, x3d, t


# ------------------------------------------------------------------------------------------------ 1: sampler parity
@pytest.mark.parametrize("cs", WIDTHS)
def test_sampler_parity_with_and_without_the_switch(monkeypatch, cs):
    """F = 27, dep 2, B 2, H 2, K 2 under flip TTA: passes of 3672 token rows, 14 whole 256-row tiles of the Linears plus 88 rows.
    With the switch the context reports the split-fp16 implementation, without it the fp32 one; both within EXACT_TOL_MM."""
    frames, dep, B, H, K = 27, 2, 2, 2, 2
    sd = make_state_dict(33, cs, dep, frames)
    x2d = synthetic_inputs_2d(331, B, frames)
    noises = [torch.from_numpy(synthetic_noise(332 + k, (B, H, frames, 17, 3))) for k in range(K)]
    want = oracle_sample(sd, x2d, noises, H, K, dep)
    for on, impl in ((True, "f16x2"), (False, "f32")):
        switch(monkeypatch, on)
        m = sampler(sd, frames, cs, dep, H, K)
        out = sample(m, x2d, noises)
        err = orc.mpjpe_mm(out.cpu(), want)
        got = m.pose_estimator.exact_scales()[2]
        print(f"cs={cs} exact sampler, D3DP_EXACT_IMPL={'f16x2' if on else 'unset'}: {got}, MPJPE vs the fp32 oracle {err:.3e} mm")
        assert out.shape == (B, K, H, frames, 17, 3) and torch.isfinite(out).all()
        assert got == impl
        assert err <= EXACT_TOL_MM
        assert not m.pose_estimator.nonfinite_seen()


# ------------------------------------------------------------------------------------------------ 2: the attention kernels
@pytest.mark.parametrize("cs,frames,joints", [
    (384, 243, 17),      # hdp 64: the persistent whole-sequence kernel (16 key tiles, keys end inside the last) + the one-wave spatial kernel
    (192, 243, 17),      # hdp 32: the same two
    (448, 257, 5),       # the chunked-key kernel, its last chunk one key in
    (320, 9, 40),        # more than 32 joints: the spatial axis on the whole-sequence kernel
])
def test_attention_kernels_behind_padded_heads(monkeypatch, cs, frames, joints):
    switch(monkeypatch, True)
    dep, B, H = 1, 1, 1
    sd, x2d, x3d, t = denoiser_case(35, frames, joints, cs, dep, B, H)
    m = denoiser(sd, frames, joints, cs, dep)
    got = m(x2d.cuda(), x3d.cuda(), t.cuda())
    err = orc.mpjpe_mm(got.cpu(), orc.mixste_forward(sd, x2d, x3d, t, dep))
    print(f"cs={cs} F={frames} J={joints} f16x2 with padded heads: MPJPE vs the fp32 oracle {err:.3e} mm")
    assert got.shape == (B, H, frames, joints, 3) and torch.isfinite(got).all()
    assert m.exact_scales()[2] == "f16x2"
    assert err <= EXACT_TOL_MM


# ------------------------------------------------------------------------------------------------ 3: pad columns
def test_pad_columns_never_leak(monkeypatch):
    """The pad columns of the packed qkv rows and of the attention output are WRITTEN (exact zeros) by every call, never assumed:
    a workspace full of NaN bit patterns and a zeroed one give the same finite bits."""
    switch(monkeypatch, True)
    cs, frames, dep, B, H = 384, 27, 2, 1, 2
    sd, x2d, x3d, t = denoiser_case(37, frames, 17, cs, dep, B, H)
    m = denoiser(sd, frames, 17, cs, dep)
    args = (x2d.cuda(), x3d.cuda(), t.cuda())
    first = m(*args).clone()                                # allocates the workspace
    ws = m._state().ws
    outs = []
    for fill in (0xFF, 0x00):
        torch.cuda.synchronize()
        ws.fill_(fill)
        outs.append(m(*args).clone())
    assert m.exact_scales()[2] == "f16x2"
    assert all(torch.isfinite(o).all() for o in outs)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], first)


# ------------------------------------------------------------------------------------------------ 4: split invariance
def test_pass_split_and_reruns_change_no_bit(monkeypatch):
    """B H = 5 sequences in passes of 2, 2, 1 against one pass of 5."""
    switch(monkeypatch, True)
    cs, frames, dep, B, H = 384, 27, 2, 1, 5
    sd, x2d, x3d, t = denoiser_case(39, frames, 17, cs, dep, B, H)
    args = (x2d.cuda(), x3d.cuda(), t.cuda())
    m2, m5 = denoiser(sd, frames, 17, cs, dep, chunk_seqs=2), denoiser(sd, frames, 17, cs, dep, chunk_seqs=5)
    a, b = m2(*args).clone(), m5(*args).clone()
    assert m2.exact_scales()[2] == "f16x2" and torch.isfinite(a).all()
    assert torch.equal(a, b)
    assert torch.equal(a, m2(*args)) and torch.equal(b, m5(*args))


# ------------------------------------------------------------------------------------------------ 5: the residual fold
def test_residual_adds_inside_the_linears_change_no_bit(monkeypatch):
    """test_exact_residual_adds_inside_the_linears_change_no_bit's contract at cs = 384 under the switch: D3DP_NO_FOLD=1 (y1 / y
    buffers, added by the row kernels' yadd arguments) computes the folded run's bits."""
    switch(monkeypatch, True)
    cs, frames, dep, B, H = 384, 27, 2, 1, 2
    sd, x2d, x3d, t = denoiser_case(41, frames, 17, cs, dep, B, H)
    args = (x2d.cuda(), x3d.cuda(), t.cuda())
    folded = denoiser(sd, frames, 17, cs, dep)(*args).clone()
    monkeypatch.setenv("D3DP_NO_FOLD", "1")
    m = denoiser(sd, frames, 17, cs, dep)
    plain = m(*args)
    assert m.exact_scales()[2] == "f16x2" and torch.isfinite(folded).all()
    assert torch.equal(folded, plain)
    assert orc.mpjpe_mm(folded.cpu(), orc.mixste_forward(sd, x2d, x3d, t, dep)) <= EXACT_TOL_MM


# ------------------------------------------------------------------------------------------------ 6: the range proof
def _range_run(edit):
    """test_exact_mode_range_guard's run at cs = 384 (Fr 9, dep 2, B 2, H 2, K 1; its seeds)."""
    Fr, B, H, K, cs, dep = 9, 2, 2, 1, 384, 2
    x2d = synthetic_inputs_2d(5, B, Fr)
    noises = [torch.from_numpy(synthetic_noise(70, (B, H, Fr, 17, 3)))]
    sd = make_state_dict(7, cs, dep, Fr)
    key, factor = edit
    key = [k for k in sd if k.endswith(key)][0]
    sd[key] = sd[key] * factor
    m = sampler(sd, Fr, cs, dep, H, K)
    out = sample(m, x2d, noises)
    return m.pose_estimator, out, orc.mpjpe_mm(out.cpu(), oracle_sample(sd, x2d, noises, H, K, dep))


def test_out_of_range_qkv_lowers_the_scale_and_stays_on_f16x2(monkeypatch):
    """STE block 1's qkv matrix x 200: q, k, v of several hundred.  The block's s_kv drops, the context stays on the split-fp16
    implementation; 0.05 mm is the bound test_exact_mode_range_guard and test_hip_exact_heads apply to this edit."""
    switch(monkeypatch, True)
    net, out, e = _range_run(("STEblocks.1.attn.qkv.weight", 200.0))
    kv, hd, impl = net.exact_scales()
    print(f"cs=384 qkv x 200: bound {net.exact_range_bound():.4g}, q/k/v scale of that block {kv[1]:g}, {impl}, error {e:.3e} mm")
    assert impl == "f16x2" and kv[1] < 16.0 and kv[1] * net.exact_range_bound() < 65504.0 and set(hd) == {16.0}
    assert torch.isfinite(out).all() and not net.nonfinite_seen() and e <= 0.05


def test_out_of_range_layernorm_lands_on_the_fp32_implementation(monkeypatch):
    """A norm2 gain x 300 pushes LayerNorm's own output bound out of the split range: where an instantiated width moves to bf16x3
    this context moves to the fp32 implementation (bf16x3 does not exist at its width)."""
    switch(monkeypatch, True)
    net, out, e = _range_run(("TTEblocks.0.norm2.weight", 300.0))
    impl = net.exact_scales()[2]
    print(f"cs=384 norm2 gain x 300: implementation {impl}, error {e:.3e} mm")
    assert impl == "f32" and torch.isfinite(out).all() and not net.nonfinite_seen()
    assert e <= EXACT_TOL_MM


# ------------------------------------------------------------------------------------------------ 7: the workspace
class Guarded:
    """`n` workspace bytes between two guards of a fixed pattern (tests/test_hip_workspace.py)."""
    GUARD, PATTERN = 4096, 0xA5

    def __init__(self, n):
        self.n, self.buf = n, torch.full((n + 2 * self.GUARD,), self.PATTERN, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + self.GUARD
        assert self.ptr % 256 == 0

    def intact(self):
        torch.cuda.synchronize()
        return bool((self.buf[:self.GUARD] == self.PATTERN).all()) and bool((self.buf[self.GUARD + self.n:] == self.PATTERN).all())


@pytest.mark.parametrize("cs", [192, 384])
def test_denoise_workspace(monkeypatch, cs):
    """The call runs in exactly d3dp_workspace_bytes (bufA: max(C, Cp) columns, bufB: max(3 Cp, hidden)), writes nothing outside,
    computes the same in a roomier one and refuses a smaller one before it writes."""
    switch(monkeypatch, True)
    F, J, B, H, ESTATE = 9, 5, 1, 2, -4
    c = ab.RawCtx("exact", cs, F, J, 2, 0)
    impl = ab.C.c_int32()
    _lib.check(c.lib.d3dp_exact_scales(c.ctx, None, None, ab.C.byref(impl)), "d3dp_exact_scales")
    assert impl.value == 0
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


# ------------------------------------------------------------------------------------------------ 8: the row kernels alone
def h2i_planes(buf, T, C_):
    """h2i rows [T][C / 32][hi 32 | lo 32] -> (hi, lo), each [T, C] fp32."""
    v = buf.view(T, C_ // 32, 2, 32).float()
    return v[:, :, 0, :].reshape(T, C_), v[:, :, 1, :].reshape(T, C_)


@pytest.mark.parametrize("T", [5, 67])
@pytest.mark.parametrize("C_", WIDTHS)
def test_layernorm_with_split_fp16_rows_out(C_, T):
    """d3dp_op_layernorm(out 3) at a run-time width: (hi + lo) / 16 against an fp64 LayerNorm.  The kernel computes the fp32
    LayerNorm of the library's fp32-output form (code 0) and splits it into two fp16 (2 x 11 bits: <= 2^-22 |y|, common.h), so
    its largest error may exceed that form's on the same inputs by the split's own error and by what two fp32 roundings of the
    row statistics in another summation order differ by: 2^-21 max |y| in all.  T = 5: a partly filled workgroup of 4 rows."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(C_ + T)
    x = torch.randn(T, C_, generator=g) * 3 + 0.5
    w, b = torch.randn(C_, generator=g), torch.randn(C_, generator=g)
    want = torch.nn.functional.layer_norm(x.double(), (C_,), w.double(), b.double(), 1e-6)
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    out32 = torch.full((T, C_), float("nan"), device="cuda")
    _lib.check(lib.d3dp_op_layernorm(0, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), 1e-6, out32.data_ptr(), T, C_, _lib.current_stream()))
    out2 = torch.full((2 * (T + 1) * C_,), float("nan"), dtype=torch.float16, device="cuda")     # (a row of slack: must stay NaN)
    _lib.check(lib.d3dp_op_layernorm(3, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), 1e-6, out2.data_ptr(), T, C_, _lib.current_stream()))
    torch.cuda.synchronize()
    assert torch.isnan(out2[2 * T * C_:]).all()
    hi, lo = h2i_planes(out2[:2 * T * C_].cpu(), T, C_)
    assert torch.isfinite(hi).all() and torch.isfinite(lo).all()
    got = (hi.double() + lo.double()) / 16.0
    e3, e0 = (got - want).abs().max().item(), (out32.cpu().double() - want).abs().max().item()
    print(f"layernorm C={C_} T={T}: split-fp16 rows max |err| vs fp64 {e3:.3e}, fp32 rows {e0:.3e}, max |y| {want.abs().max().item():.3g}")
    assert e3 <= e0 + 2.0 ** -21 * want.abs().max().item()
