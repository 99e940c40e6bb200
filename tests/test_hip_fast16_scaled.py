"""GPU tests of D3DP_FAST16_RANGE=scale: a FAST16 context whose weights prove a bound of 65504 or more for a block's q/k/v, proj
output, MLP hidden or fc2 output stores that class of fp16 tensors at a power of two 2^-s (s <= 8) of its value instead of moving
the whole context to bf16 (include/d3dp_hip.h: d3dp_fast_operands; ctx.h BlockDev::r_*).

  1. one weight edit per scale, so that each producer / consumer pairing of scaled kernels runs alone, on the fixture of
     tests/test_hip_fast16.py::_fallback_case (cs 512, dep 2, F 27, B = H = K = 2, seed 41);
  2. the kernel forms those cases do not reach: head dims 32 and 16, the chunked-key attention kernel (F 288), the spatial axis on
     the whole-sequence kernel (J 40);
  3. the cap (s > 8 falls back), non-finite weights, the seed weights (every s is 0: the plain kernels, bit for bit);
  4. the stream contract on a scaled case.

Every accuracy gate is the existing FAST16 gate (test_sampler_fast16_vs_fp16_emulating_oracle): e32 <= 1.5 emu32 with emu32 the
oracle's UNSCALED fp16 emulation, and e32 < 0.4 x the `fast` model's distance on the same weights.  The emulations alone, on a CPU
(fp16 emulation / bf16 emulation, mm vs the fp32 oracle, and their ratio -- a case is kept only below 0.27, so that 1.5 x it stays
below 0.4):
    fc2 x 16       0.383 / 3.162  0.121        norm1 x 256, cs 256   6.349 / 37.21  0.171
    proj x 32      0.758 / 3.761  0.202        norm1 x 256, cs 128   4.385 / 28.18  0.156
    fc1 x 256      0.414 / 2.853  0.145        norm1 x 256, F 288    3.380 / 26.23  0.129
    norm1 x 32     3.379 / 26.34  0.128        norm1 x 256, J 40 F 9 1.890 / 17.69  0.107   (one denoiser call)
    norm1 x 256    6.630 / 34.82  0.190        norm1 x 512, cs 256   6.269 / 37.82  0.166
                                               norm1 x 1024, cs 128  5.413 / 28.23  0.192
"""
import functools
import warnings

import pytest
import torch

from d3dp_amd.model import MixSTE2
from d3dp_amd.weights import make_state_dict, synthetic_inputs_2d, synthetic_noise
from oracle import d3dp_oracle as orc
from test_hip_fast16 import FP16_MAX, f16_round, oracle_sample, sample, sampler_model

pytestmark = pytest.mark.gpu
CLASSES = ("b_qkv", "b_proj", "b_h", "b_fc2")
NORM1 = ("TTEblocks.1.norm1.weight", "TTEblocks.1.norm1.bias")
# name -> (cs, frames, B = H = K, [(state_dict keys, factor)], the exponents (s_qkv, s_proj, s_h, s_fc2) the edit must produce)
CASES = {
    "fc2x16": (512, 27, 2, [(("TTEblocks.0.mlp.fc2.weight",), 16)], (0, 0, 0, 1)),
    "projx32": (512, 27, 2, [(("STEblocks.1.attn.proj.weight",), 32)], (0, 1, 0, 0)),
    "fc1x256": (512, 27, 2, [(("STEblocks.0.mlp.fc1.weight",), 256)], (0, 0, 1, 5)),
    "norm1x32": (512, 27, 2, [(NORM1, 32)], (0, 1, 0, 0)),
    "norm1x256": (512, 27, 2, [(NORM1, 256)], (1, 4, 0, 0)),
    "norm1x256_cs256": (256, 27, 2, [(NORM1, 256)], (0, 3, 0, 0)),      # (at these widths x 256 leaves b_qkv in range: the row kernels
    "norm1x256_cs128": (128, 27, 2, [(NORM1, 256)], (0, 1, 0, 0)),      #  and proj alone run scaled; the next two reach the attention)
    "norm1x512_cs256": (256, 27, 2, [(NORM1, 512)], (1, 4, 0, 0)),
    "norm1x1024_cs128": (128, 27, 2, [(NORM1, 1024)], (1, 3, 0, 0)),
    "norm1x256_F288": (512, 288, 1, [(NORM1, 256)], (1, 4, 0, 0)),
    "seed": (512, 27, 2, [], (0, 0, 0, 0)),
    "fc2x4096": (512, 27, 2, [(("TTEblocks.0.mlp.fc2.weight",), 4096)], (0, 0, 0, 9)),
}


def block_bounds_fp64(sd, cs, dep, prefix="pose_estimator."):
    """The table of include/d3dp_hip.h (d3dp_fast_operands) in fp64, per block: L (both LayerNorm outputs), b_qkv, b_proj, b_h, b_fc2
    and w (max |w| of the four matrices)."""
    sq, out = (cs - 1) ** 0.5, []
    for kind in ("STEblocks", "TTEblocks"):
        for d in range(dep):
            g = lambda n: sd[f"{prefix}{kind}.{d}.{n}"].double()
            in1 = sq * g("norm1.weight").abs() + g("norm1.bias").abs()
            in2 = sq * g("norm2.weight").abs() + g("norm2.bias").abs()
            rows = g("attn.qkv.weight").abs() @ in1 + g("attn.qkv.bias").abs()
            b_h = (g("mlp.fc1.weight").abs() @ in2 + g("mlp.fc1.bias").abs()).max()
            out.append({"L": float(max(in1.max(), in2.max())), "b_qkv": float(rows.max()),
                        "b_proj": float((g("attn.proj.weight").abs().sum(dim=1) * rows[2 * cs:].max() + g("attn.proj.bias").abs()).max()),
                        "b_h": float(b_h),
                        "b_fc2": float((g("mlp.fc2.weight").abs().sum(dim=1) * b_h + g("mlp.fc2.bias").abs()).max()),
                        "w": float(max(g(n).abs().max() for n in ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight")))})
    return out


def shifts_fp64(blocks):
    """(s_qkv, s_proj, s_h, s_fc2), each the largest over the blocks of the smallest s >= 0 with bound x 2^-s < 65504."""
    def s(bound):
        n = 0
        while not bound * 2.0 ** -n < FP16_MAX:
            n += 1
        return n
    return tuple(max(s(b[c]) for b in blocks) for c in CLASSES)


def edited_state_dict(name, prefix="pose_estimator.", joints=17, frames=None):
    cs, fr, _, edits, _ = CASES[name]
    sd = make_state_dict(41, cs, 2, fr if frames is None else frames, prefix=prefix, joints=joints)
    for keys, factor in edits:
        for k in keys:
            sd[prefix + k] = sd[prefix + k] * float(factor)
    return sd


@functools.lru_cache(maxsize=None)
def case(name):
    """Weights, inputs and the two CPU references of a case, computed once: want32 (fp32 oracle) and emu32 = the distance of the
    oracle's fp16 emulation, unscaled, to it."""
    cs, frames, n, _, _ = CASES[name]
    sd = edited_state_dict(name)
    x2d = synthetic_inputs_2d(411, n, frames)
    noises = [torch.from_numpy(synthetic_noise(412 + k, (n, n, frames, 17, 3))) for k in range(n)]
    p = orc.strip_prefix(sd)
    want32 = oracle_sample(p, x2d, noises, n, n, 2)
    saved = orc._r16
    orc._r16 = f16_round
    try:
        want16 = oracle_sample(orc.emulate_bf16(p), x2d, noises, n, n, 2)
    finally:
        orc._r16 = saved
    assert torch.isfinite(want32).all() and torch.isfinite(want16).all()
    blocks = block_bounds_fp64(sd, cs, 2)
    return {"sd": sd, "x2d": x2d, "noises": noises, "want32": want32, "emu32": orc.mpjpe_mm(want16, want32), "blocks": blocks,
            "bound": max(max(b.values()) for b in blocks), "shape": (frames, cs, 2, n, n)}


def run(c, numerics):
    """-> (output on the CPU, fast_operands(), nonfinite_seen(), the fast16 warnings raised); a new model and context."""
    frames, cs, dep, H, K = c["shape"]
    m = sampler_model(c["sd"], frames, cs, dep, H, K, numerics)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = sample(m, c["x2d"], c["noises"])
    return out.cpu(), m.pose_estimator.fast_operands(), m.pose_estimator.nonfinite_seen(), [w for w in caught if "fast16" in str(w.message)]


def check_scaled(name, out, ops, nonfinite, said, out_fast, want32, emu32, bound_fp64):
    kind, bound = ops
    e32, fast32 = orc.mpjpe_mm(out, want32), orc.mpjpe_mm(out_fast, want32)
    print(f"{name}: {kind}, device bound {bound:.5g} (fp64 {bound_fp64:.5g}); e32 {e32:.3f} mm, emu32 {emu32:.3f} mm, fast32 {fast32:.3f} mm; "
          f"e32 / emu32 {e32 / emu32:.3f}, e32 / fast32 {e32 / fast32:.3f}")
    assert kind == "fp16" and bound >= FP16_MAX
    assert bound_fp64 * (1 - 1e-6) <= bound <= bound_fp64 * (1 + 1e-3)
    assert not said, [str(w.message) for w in said]
    assert torch.isfinite(out).all() and not nonfinite
    assert e32 <= 1.5 * emu32
    assert e32 < 0.4 * fast32
    assert not torch.equal(out, out_fast)


# ------------------------------------------------------------------------------------------------ 1, 2: one edit per scale; kernel forms
@pytest.mark.parametrize("name", ["fc2x16", "projx32", "fc1x256", "norm1x32", "norm1x256", "norm1x256_cs256", "norm1x256_cs128",
                                  "norm1x512_cs256", "norm1x1024_cs128", "norm1x256_F288"])
def test_scaled_fast16_on_an_edit_that_trips_the_plain_proof(monkeypatch, name):
    """The first five: one class of tensors each beyond 65504 (fc1 x 256: the hidden AND, by 2^5, fc2's output; norm1 x 256: q/k/v --
    the attention exponent -- and proj's output).  The rest: head dims 32 and 16 -- where norm1 x 256 scales proj's output alone and
    x 512 / x 1024 q/k/v as well, i.e. the attention kernels of those head dims -- and at F = 288 the chunked-key kernel on the
    temporal axis."""
    monkeypatch.setenv("D3DP_FAST16_RANGE", "scale")
    c = case(name)
    got = shifts_fp64(c["blocks"])
    want = CASES[name][4]
    print(f"{name}: exponents (s_qkv, s_proj, s_h, s_fc2) = {got}")
    assert got == want and max(got) <= 8
    assert all(b["L"] < FP16_MAX and b["w"] < FP16_MAX for b in c["blocks"])
    out, ops, nonfinite, said = run(c, "fast16")
    out_fast, ops_fast, _, _ = run(c, "fast")
    assert ops_fast == ("bf16", 0.0)
    check_scaled(name, out, ops, nonfinite, said, out_fast, c["want32"], c["emu32"], c["bound"])


def test_scaled_fast16_with_more_than_32_joints(monkeypatch):
    """(J, F) = (40, 9): the spatial axis runs the whole-sequence kernel, scaled; norm1 x 256.  One denoiser call, the inputs of
    test_fast16_denoiser_with_more_than_32_joints."""
    monkeypatch.setenv("D3DP_FAST16_RANGE", "scale")
    joints, cs, frames, B, H, dep = 40, 512, 9, 2, 2, 2
    sd = edited_state_dict("norm1x256", prefix="", joints=joints, frames=frames)
    blocks = block_bounds_fp64(sd, cs, dep, prefix="")
    got = shifts_fp64(blocks)
    assert got[0] >= 1 and max(got) <= 8, got
    g = torch.Generator().manual_seed(joints * 7 + cs)
    x2d = torch.rand(B, frames, joints, 2, generator=g) * 2 - 1
    x3d = torch.randn(B, H, frames, joints, 3, generator=g)
    t = torch.tensor([999, 120])
    want32 = orc.mixste_forward(sd, x2d, x3d, t, dep)
    saved = orc._r16
    orc._r16 = f16_round
    try:
        want16 = orc.mixste_forward(orc.emulate_bf16(sd), x2d, x3d, t, dep)
    finally:
        orc._r16 = saved
    res = {}
    for numerics in ("fast16", "fast"):
        m = MixSTE2(num_frame=frames, num_joints=joints, embed_dim_ratio=cs, depth=dep, is_train=False, numerics=numerics,
                    drop_path_rate=0.0)
        m.load_state_dict(sd, strict=True)
        m = m.cuda().eval()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            got_out = m(x2d.cuda(), x3d.cuda(), t.cuda()).cpu()
        res[numerics] = (got_out, m.fast_operands(), m.nonfinite_seen(), [w for w in caught if "fast16" in str(w.message)])
    out, ops, nonfinite, said = res["fast16"]
    assert out.shape == (B, H, frames, joints, 3)
    check_scaled("norm1x256 J=40 F=9", out, ops, nonfinite, said, res["fast"][0], want32, orc.mpjpe_mm(want16, want32),
                 max(max(b.values()) for b in blocks))


# ------------------------------------------------------------------------------------------------ 3: the cap, non-finite weights, s = 0
def test_a_bound_beyond_the_cap_falls_back_to_bf16(monkeypatch):
    """fc2 x 4096: b_fc2 = 1.92e7 > 65504 x 2^8.  'bf16', one warning, the bits of a `fast` model."""
    monkeypatch.setenv("D3DP_FAST16_RANGE", "scale")
    c = case("fc2x4096")
    assert shifts_fp64(c["blocks"]) == (0, 0, 0, 9) and abs(c["bound"] / 1.92e7 - 1) < 0.01
    m = sampler_model(c["sd"], *c["shape"], "fast16")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = sample(m, c["x2d"], c["noises"])
        out_again = sample(m, c["x2d"], c["noises"])
    said = [w for w in caught if "fast16" in str(w.message)]
    assert len(said) == 1 and "bf16" in str(said[0].message), [str(w.message) for w in caught]
    kind, bound = m.pose_estimator.fast_operands()
    assert kind == "bf16" and c["bound"] * (1 - 1e-6) <= bound <= c["bound"] * (1 + 1e-3)
    out_fast = run(c, "fast")[0]
    assert torch.isfinite(out).all() and torch.equal(out.cpu(), out_fast) and torch.equal(out, out_again)
    assert not m.pose_estimator.nonfinite_seen()


def test_a_non_finite_weight_behaves_as_without_the_switch(monkeypatch):
    monkeypatch.setenv("D3DP_FAST16_RANGE", "scale")
    c = dict(case("seed"))
    c["sd"] = dict(c["sd"])
    key = "pose_estimator.TTEblocks.0.attn.proj.weight"
    c["sd"][key] = c["sd"][key].clone()
    c["sd"][key].view(-1)[3] = float("inf")
    out, (kind, bound), nonfinite, said = run(c, "fast16")
    out_fast, _, nonfinite_fast, _ = run(c, "fast")
    assert kind == "bf16" and bound == float("inf") and len(said) == 1
    assert nonfinite and nonfinite_fast
    assert torch.equal(out.view(torch.int32), out_fast.view(torch.int32))    # bit-equal, nan payloads included


def test_the_seed_weights_run_the_plain_kernels_with_the_switch(monkeypatch):
    """Every s is 0: bit for bit the model without the switch, and its bound below 65504."""
    c = case("seed")
    monkeypatch.delenv("D3DP_FAST16_RANGE", raising=False)
    plain, ops_plain, _, _ = run(c, "fast16")
    monkeypatch.setenv("D3DP_FAST16_RANGE", "scale")
    out, ops, nonfinite, said = run(c, "fast16")
    assert ops == ops_plain and ops[0] == "fp16" and 0.0 < ops[1] < FP16_MAX
    assert not said and not nonfinite and torch.isfinite(out).all()
    assert torch.equal(out, plain)


# ------------------------------------------------------------------------------------------------ 4: the stream contract
def test_a_scaled_sampler_on_a_side_stream_equals_the_default_stream(monkeypatch):
    monkeypatch.setenv("D3DP_FAST16_RANGE", "scale")
    c = case("norm1x256")
    m = sampler_model(c["sd"], *c["shape"], "fast16")
    ref = sample(m, c["x2d"], c["noises"])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = sample(m, c["x2d"], c["noises"])
    s.synchronize()
    kind, bound = m.pose_estimator.fast_operands()
    assert kind == "fp16" and bound >= FP16_MAX
    assert torch.isfinite(ref).all() and torch.equal(ref, got)


def test_a_scaled_denoise_is_capturable(monkeypatch):
    """One eager call, then the same call captured into a graph: the replay on new inputs computes the eager call's bits (the
    multipliers are by-value kernel arguments fixed at d3dp_set_weights)."""
    monkeypatch.setenv("D3DP_FAST16_RANGE", "scale")
    c = case("norm1x256")
    B, H, Fr = 2, 3, 27
    pe = sampler_model(c["sd"], *c["shape"], "fast16").pose_estimator
    x2d = torch.from_numpy(synthetic_inputs_2d(58, B, Fr)).cuda()
    x3d = torch.from_numpy(synthetic_noise(59, (B, H, Fr, 17, 3))).cuda()
    t, out = torch.tensor([10, 800], dtype=torch.long).cuda(), torch.empty((B, H, Fr, 17, 3), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pe.denoise(x2d, x3d, t, out=out)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        pe.denoise(x2d, x3d, t, out=out)
    new = [torch.from_numpy(synthetic_inputs_2d(300, B, Fr)).cuda(), torch.from_numpy(synthetic_noise(310, (B, H, Fr, 17, 3))).cuda(),
           torch.tensor([500, 3], dtype=torch.long).cuda()]
    for buf, v in zip((x2d, x3d, t), new):
        buf.copy_(v)
    g.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    eager = pe.denoise(*new)
    torch.cuda.synchronize()
    kind, bound = pe.fast_operands()
    assert kind == "fp16" and bound >= FP16_MAX
    assert torch.isfinite(eager).all() and torch.equal(eager, replayed)
