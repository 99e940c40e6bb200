"""GPU tests (-m gpu) of the native sampler (include/d3dp_hip.h, "the whole sampler as one call"): d3dp_sample against the Python
loop it replaces, bit for bit wherever the noise is injected; its non-flip glue kernels alone against oracle/glue_check.py; the
counter-based generator against a Philox4x32-10 written here in numpy (integer stage) and fp64 Box-Muller on the same words
(normal stage); the generator inside the sampler; the workspace, stream, capture and refusal contract; the command line.

Every test here fails on a library without d3dp_sample / d3dp_op_randn (d3dp_amd._lib refuses to load it).  Shapes are the
smallest that reach each branch: F 9 / 27 (one / several blocks of 256 rows), F 300 (chunked-key attention), chunk_seqs 3 (several
denoiser passes), K 1 / 2 / 3 (only / first + last / a middle step)."""
import ctypes as C
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_hip_streams as ts
from d3dp_amd import D3DP, D3DP3DHP, _lib
from d3dp_amd import eval3dhp as e3
from d3dp_amd.model import cosine_beta_schedule
from d3dp_amd.weights import H36M_JOINTS_LEFT as KL, H36M_JOINTS_RIGHT as KR, flip_2d, make_state_dict, synthetic_inputs_2d, synthetic_noise
from oracle import d3dp_oracle as orc
from oracle import glue_check as gc
from test_hip_glue import Cmp, NAN, INF, SENTINEL, GUARD, SHAPES, SCALES, TIME_PAIRS, out_buffer, guard_intact, plant, rng
from test_hip_workspace import Guarded, ab

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -4


# ---- models and calls ---------------------------------------------------------------------------------------------------
def make_model(numerics, cs, dep, Fr, H, K, chunk=0, flip=True, cls=D3DP, seed=23, scale=1.0):
    jl, jr = (e3.KPS_LEFT_3DHP, e3.KPS_RIGHT_3DHP) if cls is D3DP3DHP else (KL, KR)
    args = SimpleNamespace(number_of_frames=Fr, test_time_augmentation=flip, timestep=1000, scale=scale, cs=cs, dep=dep, chunk_seqs=chunk)
    m = cls(args, jl, jr, is_train=False, num_proposals=H, sampling_timesteps=K, numerics=numerics)
    m.load_state_dict(make_state_dict(seed, cs, dep, Fr), strict=False)
    return m.cuda().eval()


def inputs(m, B, seed=31):
    x2d = synthetic_inputs_2d(seed, B, m.frames)
    shape = (B, m.num_proposals, m.frames, 17, 3)
    noises = [torch.from_numpy(synthetic_noise(seed + 1 + k, shape)).cuda() for k in range(m.sampling_timesteps)]
    return torch.from_numpy(x2d).cuda(), torch.from_numpy(flip_2d(x2d)).cuda(), noises


def sample(m, sampler, x2d, x2f, noise=None, generator=None):
    """D3DP.forward through `sampler`; the non-flip list stacked to the flip result's shape (B, K, H, F, J, 3)."""
    m.sampler = sampler
    kw = {} if noise is None else {"noise": noise}
    out = m(x2d, None, input_2d_flip=x2f, generator=generator, **kw) if m.flip else m(x2d, None, generator=generator, **kw)
    torch.cuda.synchronize()
    return out if m.flip else torch.stack(list(out), dim=1)


# ---- 1. injected noise: the bits of the Python loop ----------------------------------------------------------------------
INJECTED = [
    pytest.param("exact", 64, 1, 9, 2, 2, 3, 0, True, D3DP, id="exact-c64-K3"),                # first / middle / last step
    pytest.param("exact", 64, 1, 9, 2, 2, 3, 3, True, D3DP, id="exact-c64-K3-chunk3"),         # 8 sequences in passes of 3, 3, 2
    pytest.param("fast", 128, 2, 27, 1, 2, 2, 0, True, D3DP, id="fast-c128"),
    pytest.param("fast16", 128, 2, 27, 1, 2, 2, 0, True, D3DP, id="fast16-c128"),
    pytest.param("exact", 128, 1, 300, 1, 1, 2, 0, True, D3DP, id="exact-c128-F300"),          # chunked-key attention
    pytest.param("fast16", 128, 1, 300, 1, 1, 2, 0, True, D3DP, id="fast16-c128-F300"),
    pytest.param("exact", 64, 1, 9, 1, 2, 3, 0, False, D3DP, id="noflip-K3"),                  # against ddim_sample
    pytest.param("exact", 64, 1, 9, 2, 2, 1, 0, True, D3DP, id="K1"),
    pytest.param("exact", 64, 1, 9, 1, 1, 1, 0, False, D3DP, id="noflip-K1"),
    pytest.param("exact", 64, 1, 9, 2, 2, 3, 0, True, D3DP3DHP, id="3dhp"),
]


@pytest.mark.parametrize("numerics,cs,dep,Fr,B,H,K,chunk,flip,cls", INJECTED)
def test_injected_noise_gives_the_python_loops_bits(numerics, cs, dep, Fr, B, H, K, chunk, flip, cls):
    m = make_model(numerics, cs, dep, Fr, H, K, chunk, flip, cls)
    x2d, x2f, noises = inputs(m, B)
    want = sample(m, "python", x2d, x2f, noises)
    got = sample(m, "native", x2d, x2f, noises)
    assert got.shape == (B, K, H, Fr, 17, 3) and torch.isfinite(want).all()
    c = Cmp()
    c.eq("preds", got, want)
    c.done()
    if not flip:                                    # ddim_sample's return type: a list of K contiguous (B, H, F, J, 3) tensors
        m.sampler = "native"
        out = m(x2d, None, noise=noises)
        assert isinstance(out, list) and len(out) == K and all(o.shape == (B, H, Fr, 17, 3) and o.is_contiguous() for o in out)


def test_step_table_holds_the_devices_non_flip_coefficients():
    """c_noise64 and sigma of d3dp_ddim_steps against D3DP.ddim_sample's own expressions evaluated where ddim_sample evaluates
    them: on fp64 tensors on the device (division and sqrt correctly rounded there; torch's CPU sqrt is not)."""
    m = make_model("exact", 64, 1, 9, 1, 1)
    bad = []
    for K in list(range(1, 17)) + [50, 64]:
        m.sampling_timesteps = K
        for s, (time, time_next) in zip(m._steps(), m.time_pairs()):
            if time_next < 0:
                continue
            alpha, alpha_next = m.alphas_cumprod[time], m.alphas_cumprod[time_next]
            sigma = m.ddim_sampling_eta * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
            c = (1 - alpha_next - sigma ** 2).sqrt()
            one = torch.ones(1, device="cuda")
            for name, got, want in (("c_noise64", s.c_noise64, c.item()), ("sigma", s.sigma, (one * sigma).item()),
                                    ("c_xstart", s.c_xstart, (one * alpha_next.sqrt()).item())):
                if np.float64(got).view(np.int64) != np.float64(want).view(np.int64):
                    bad.append(f"K={K} t={time}->{time_next}: {name} {got!r} != {want!r}")
    assert not bad, "\n".join(bad[:10])


# ---- 2. the non-flip glue alone, against oracle/glue_check.py -------------------------------------------------------------
def clamp_edges64(scale):
    """The fp64 bound 1.1 s and its neighbours, the fp32 bound fp32(1.1 s) and its fp32 neighbours, and the specials."""
    lim = 1.1 * scale
    l32 = np.float32(lim)
    vals = [lim, -lim, np.nextafter(lim, np.inf), np.nextafter(lim, 0.0), -np.nextafter(lim, np.inf), -np.nextafter(lim, 0.0),
            float(l32), -float(l32), float(np.nextafter(l32, np.float32(np.inf))), float(np.nextafter(l32, np.float32(0)))]
    return [float(v) for v in vals] + [INF, -INF, NAN, -0.0, 1e-40, -1e-40, 1e-310]


@pytest.mark.parametrize("first", [1, 0], ids=["fp32-img", "fp64-img"])
@pytest.mark.parametrize("scale", SCALES + [9.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_ddim_pre_noflip_alone(shape, scale, first):
    B, H, Fr, J = shape
    g = rng(B * 100 + Fr + first)
    stride = 2 if shape == SHAPES[0] else 4          # (51 elements hold the 17 edges at every second one)
    if first:                                       # the initial noise: fp32 values, clamped as an fp32 tensor
        img = plant(torch.randn(B, H, Fr, J, 3, generator=g) * scale, [float(np.float32(v)) for v in clamp_edges64(scale)], stride=stride)
        want = gc.ddim_pre_ref(img, scale, KL, KR)[0]
    else:
        img = plant(torch.randn(B, H, Fr, J, 3, generator=g, dtype=torch.float64) * scale, clamp_edges64(scale), stride=stride)
        want = gc.ddim_pre_ref(img, scale, KL, KR)[0].float()          # (what MixSTE2.denoise's .to(float32) leaves)
    flat, xt = out_buffer((B, H, Fr, J, 3))
    d_img = img.double().cuda()
    _lib.check(_lib.load().d3dp_op_ddim_pre_noflip(d_img.data_ptr(), xt.data_ptr(), scale, first, B, H, Fr, J, _lib.current_stream()),
               "d3dp_op_ddim_pre_noflip")
    torch.cuda.synchronize()
    c = Cmp()
    c.eq("x_t", xt, want)
    c.eq("img (input)", d_img, img.double())
    c.done()
    assert guard_intact(flat)


@pytest.fixture(scope="module")
def sched():
    return orc.cosine_schedule(1000)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", SHAPES)
def test_ddim_post_noflip_alone(sched, shape, scale):
    """The reference is glue_check.ddim_post_ref on an fp64 img (pred_noise then stays fp64, as in ddim_sample) with the flipped
    prediction built so that the flip average is the identity: (p + unflip(flip(p))) / 2 = p exactly.  The kernel's scalars are the
    reference's own 0-dim tensors, so the comparison is of the kernel's arithmetic alone."""
    lib = _lib.load()
    B, H, Fr, J = shape
    g = rng(B * 1000 + Fr)
    full = (B, H, Fr, J, 3)
    per_b, K = H * Fr * J * 3, 3
    pred = plant(torch.randn(full, generator=g), [NAN, INF, -INF, -0.0], stride=5)
    img = plant(torch.randn(full, generator=g, dtype=torch.float64) * scale, [INF, NAN, -0.0], stride=11, both_ends=False)
    noise = plant(torch.randn(full, generator=g), [NAN, -INF, INF], stride=7, both_ends=False)
    d_pred, d_img, d_noise = pred.cuda(), img.cuda(), noise.cuda()
    ac = sched["alphas_cumprod"]
    c = Cmp()
    for time, time_next in TIME_PAIRS:
        for eta in (1.0, 0.0):
            last = time_next < 0
            x_start, img_next = gc.ddim_post_ref(pred, orc.flip_pose(pred, KL, KR), img, noise, sched, time, time_next, scale, eta, KL, KR)
            assert x_start.dtype == torch.float32 and (last or img_next.dtype == torch.float64)
            if shape != SHAPES[0]:
                sat = (x_start.abs() == float(np.float32(1.1 * scale))).float().mean().item()
                assert 0.05 < sat < 0.6, sat
            if last:
                c_x, c64, sigma = 0.0, 0.0, 0.0
            else:
                alpha, alpha_next = ac[time], ac[time_next]
                sg = eta * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
                c_x, c64, sigma = alpha_next.sqrt().item(), (1 - alpha_next - sg ** 2).sqrt().item(), float(sg)
            for aliased in (False, True):
                xs_flat, xs = out_buffer((B, K) + full[1:])
                if aliased:
                    nx_flat = torch.cat((d_img.reshape(-1), torch.full((GUARD,), SENTINEL, device="cuda", dtype=torch.float64)))
                    nx = src = nx_flat[:B * per_b].view(full)
                else:
                    (nx_flat, nx), src = out_buffer(full, torch.float64), d_img
                _lib.check(lib.d3dp_op_ddim_post_noflip(d_pred.data_ptr(), src.data_ptr(), 0 if last else d_noise.data_ptr(), 0, 0, scale,
                                                        float(sched["sqrt_recip_alphas_cumprod"][time]),
                                                        float(sched["sqrt_recipm1_alphas_cumprod"][time]), c_x, c64, sigma, int(last),
                                                        xs[:, 1].data_ptr(), K * per_b, nx.data_ptr(), B, H, Fr, J,
                                                        _lib.current_stream()), "d3dp_op_ddim_post_noflip")
                torch.cuda.synchronize()
                tag = f"t={time}->{time_next} eta={eta:g} aliased={aliased}"
                c.eq(f"x_start [{tag}]", xs[:, 1], x_start)
                c.eq(f"x_start's other k [{tag}]", xs[:, [0, 2]], torch.full((B, 2) + full[1:], SENTINEL))
                if last:
                    c.eq(f"img_next untouched [{tag}]", nx, img if aliased else torch.full(full, SENTINEL, dtype=torch.float64))
                else:
                    c.eq(f"img_next [{tag}]", nx, img_next)
                assert guard_intact(xs_flat) and guard_intact(nx_flat), tag
    c.eq("pred (input)", d_pred, pred)
    c.eq("noise (input)", d_noise, noise)
    c.done()


# ---- 3. the generator, integer stage -------------------------------------------------------------------------------------
def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11) on numpy uint32: ctr (n, 4), key (2,) -> (n, 4).  Per round: (hi0, lo0) = M0 x c0,
    (hi1, lo1) = M1 x c2, c = (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); the key grows by the Weyl constants between rounds."""
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85
    c = [ctr[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]), int(key[1])
    lo32, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> sh) ^ c[1] ^ np.uint64(k0), p1 & lo32, (p0 >> sh) ^ c[3] ^ np.uint64(k1), p0 & lo32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=1).astype(np.uint32)


def reference_bits(seed, draw, n):
    q = np.arange((n + 3) // 4, dtype=np.uint32)
    ctr = np.stack([q, np.full_like(q, draw), np.zeros_like(q), np.zeros_like(q)], axis=1)
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:n]


def randn(seed, draw, n, want_bits=True, guard=True):
    flat, out = out_buffer((n,))
    bflat, bits = out_buffer((n,), torch.int32)
    _lib.check(_lib.load().d3dp_op_randn(seed, draw, out.data_ptr(), bits.data_ptr() if want_bits else 0, n, _lib.current_stream()),
               "d3dp_op_randn")
    torch.cuda.synchronize()
    assert guard_intact(flat) and guard_intact(bflat)
    return out, bits.cpu().numpy().view(np.uint32)


def test_philox_known_answer():
    """The numpy reference itself against the Random123 known-answer vectors of philox4x32-10 (kat_vectors): counter and key all
    zero, all ones, and the digits of pi."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = philox4x32_10(np.array([ctr], dtype=np.uint32), key)[0]
        assert tuple(int(v) for v in got) == want, [hex(int(v)) for v in got]


@pytest.mark.parametrize("n", [1, 5, 4096 + 3])
@pytest.mark.parametrize("seed", [0x0000000112345678, 0x0000000212345678, 0], ids=["hi1", "hi2", "zero"])
@pytest.mark.parametrize("draw", [0, 7])
def test_generator_words_are_philox(n, seed, draw):
    _, bits = randn(seed, draw, n)
    assert np.array_equal(bits, reference_bits(seed, draw, n))


def test_generator_words_depend_on_the_high_seed_word_and_the_draw():
    a, b = reference_bits(0x0000000112345678, 0, 64), reference_bits(0x0000000212345678, 0, 64)
    assert not np.array_equal(a, b) and not np.array_equal(a, reference_bits(0x0000000112345678, 7, 64))
    out, _ = randn(5, 0, 4096 + 3, want_bits=False)                                # bits = NULL: the normals alone
    ref, _ = randn(5, 0, 4096 + 3)
    assert ts.bits_equal(out, ref)


# ---- 4. the generator, normal stage --------------------------------------------------------------------------------------
N_STAT = 1 << 22


def box_muller(bits, dtype):
    """The header's formula on the words `bits` (n a multiple of 4), evaluated in `dtype` throughout."""
    f = dtype
    u = ((bits >> 8).astype(f) + f(0.5)) * f(2.0 ** -24)
    u = u.reshape(-1, 2)
    r = np.sqrt(f(-2.0) * np.log(u[:, 0]))
    a = f(6.2831855 if dtype is np.float32 else 2.0 * math.pi) * u[:, 1]
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=1).reshape(-1)


@pytest.fixture(scope="module")
def stat_draws():
    return [randn(2024, d, N_STAT) for d in (0, 1)]


def test_normals_are_box_muller_of_the_words(stat_draws):
    """out against fp64 Box-Muller of the same words.  The bound is not a constant: numpy's float32 evaluation of the same formula
    is measured against the fp64 one on the same words, and the kernel is allowed 8 times that (the margin of
    oracle/grad_check.py).  Measured on an MI355X: profiles/native_sampler.md."""
    out, bits = stat_draws[0]
    ref = box_muller(bits, np.float64)
    err32 = np.abs(box_muller(bits, np.float32).astype(np.float64) - ref).max()
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref).max()
    print(f"[native sampler] normal stage over {N_STAT} values: numpy float32 max |err| {err32:.3e}, kernel {err:.3e}, bound {8 * err32:.3e}")
    assert np.isfinite(out.cpu().numpy()).all()
    assert err <= 8 * err32, (err, err32)


def test_normals_have_the_moments_of_a_normal_stream(stat_draws):
    """Analytic 5-sigma bounds over n = 2^22 values: a correct generator passes each with probability > 0.999998."""
    x = stat_draws[0][0].cpu().numpy().astype(np.float64)
    y = stat_draws[1][0].cpu().numpy().astype(np.float64)
    n = x.size
    mean, var = x.mean(), x.var()
    lag1 = np.mean((x[:-1] - mean) * (x[1:] - mean)) / var
    cross = np.mean((x - mean) * (y - y.mean())) / np.sqrt(var * y.var())
    print(f"[native sampler] n = {n}: mean {mean:+.3e} (bound {5 / math.sqrt(n):.3e}), var - 1 {var - 1:+.3e} (bound "
          f"{5 * math.sqrt(2 / n):.3e}), lag-1 correlation {lag1:+.3e}, draw 0 x draw 1 correlation {cross:+.3e} (bound {5 / math.sqrt(n):.3e})")
    assert abs(mean) <= 5 / math.sqrt(n)
    assert abs(var - 1) <= 5 * math.sqrt(2 / n)
    assert abs(lag1) <= 5 / math.sqrt(n)
    assert abs(cross) <= 5 / math.sqrt(n)


# ---- 5. the generator inside the sampler ---------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [True, False], ids=["flip", "noflip"])
def test_native_noise_in_the_sampler(flip):
    B, H, Fr, K = 2, 2, 9, 3
    m = make_model("exact", 64, 1, Fr, H, K, flip=flip)
    x2d, x2f, _ = inputs(m, B)
    torch.manual_seed(77)

    def native(model, calls=0):
        model._native_calls = calls                  # (the per-call counter: the same call again)
        return sample(model, "native", x2d, x2f)

    a, b = native(m), native(m)
    assert torch.isfinite(a).all() and ts.bits_equal(a, b), "the same seed gave other bits on the second call"
    m3 = make_model("exact", 64, 1, Fr, H, K, chunk=3, flip=flip)
    assert ts.bits_equal(native(m3), a), "the stream depends on the denoiser's passes"
    seed, n = torch.initial_seed(), B * H * Fr * 17 * 3
    noises = [randn(seed, d, n)[0].view(B, H, Fr, 17, 3).clone() for d in range(K)]
    c = Cmp()
    c.eq("preds vs the Python loop on d3dp_op_randn's draws", a, sample(m, "python", x2d, x2f, noises))
    c.done()
    assert not ts.bits_equal(native(m, calls=1), a), "the next call drew the same noise"
    assert not ts.bits_equal(randn(seed + 1, 0, n)[0], randn(seed, 0, n)[0]), "another seed gave the same initial img"
    gen = torch.Generator(device="cuda").manual_seed(5)
    g1 = sample(m, "native", x2d, x2f, generator=gen)
    g2 = sample(m, "native", x2d, x2f, generator=gen)
    assert torch.isfinite(g1).all() and not ts.bits_equal(g1, g2) and not ts.bits_equal(g1, a)


# ---- 6. contract ---------------------------------------------------------------------------------------------------------
class RawSampler:
    """d3dp_sample straight on the C ABI over tools/lib_ab_hash.py's RawCtx (seeded random weights at any (C, F, J))."""

    def __init__(self, mode, cs, Fr, J, depth, K, chunk=0):
        self.c, self.K, self.F, self.J = ab.RawCtx(mode, cs, Fr, J, depth, chunk), K, Fr, J
        self.lib = self.c.lib
        ac = np.ascontiguousarray(torch.cumprod(1.0 - cosine_beta_schedule(1000), dim=0).numpy())
        self.steps = (_lib.DdimStep * K)()
        _lib.check(self.lib.d3dp_ddim_steps(ac.ctypes.data_as(C.POINTER(C.c_double)), 1000, K, 1.0, self.steps), "d3dp_ddim_steps")
        self.perm = torch.tensor([0, 2, 1, 4, 3][:J] + list(range(5, J)), dtype=torch.int32, device="cuda")

    def bytes(self, B, H, flip, K=None):
        n = C.c_size_t()
        _lib.check(self.lib.d3dp_sample_workspace_bytes(self.c.ctx, B, H, self.K if K is None else K, flip, C.byref(n)),
                   "d3dp_sample_workspace_bytes")
        return n.value

    def inputs(self, B, H):
        return (self.c.rand(B, self.F, self.J, 2), self.c.rand(B, self.F, self.J, 2), self.c.rand(self.K, B, H, self.F, self.J, 3))

    def __call__(self, inp, preds, B, H, flip, ws_ptr, ws_bytes, noise=True, seed=0, steps=None, K=None, x2f="auto"):
        x2d, x2f_t, nz = inp
        x2f_ptr = (x2f_t.data_ptr() if flip else 0) if x2f == "auto" else x2f
        return self.lib.d3dp_sample(self.c.ctx, x2d.data_ptr(), x2f_ptr, self.perm.data_ptr(), 1.0, self.steps if steps is None else steps,
                                    self.K if K is None else K, nz.data_ptr() if noise else 0, seed, preds.data_ptr(), B, H, flip,
                                    ws_ptr, ws_bytes, _lib.current_stream())


def nan_fill(g):
    g.buf[4096:4096 + g.n] = 0xFF                    # (test_hip_workspace.GUARD bytes on each side keep their pattern)


@pytest.mark.parametrize("mode,cs,chunk,flip,noise", [("exact", 128, 0, 1, True), ("exact", 64, 2, 0, False), ("fast16", 256, 0, 1, False)],
                         ids=["exact-flip-injected", "exact-noflip-passes-generated", "fast16-flip-generated"])
def test_sample_runs_in_exactly_its_workspace(mode, cs, chunk, flip, noise):
    """The method of tests/test_hip_workspace.py: the call runs in exactly d3dp_sample_workspace_bytes between guard bytes, in a
    workspace that held NaN bit patterns, computes what it computes in a roomier one, and a smaller one is refused untouched."""
    B, H, K = 1, 3, 2
    s = RawSampler(mode, cs, 9, 5, 2, K, chunk)
    n = s.bytes(B, H, flip)
    assert n > s.c.infer_bytes(2 * B if flip else B, H)
    inp = s.inputs(B, H)
    tight, roomy = Guarded(n), Guarded(2 * n)
    nan_fill(tight), nan_fill(roomy)
    out, ref = torch.empty(B, K, H, 9, 5, 3, device="cuda"), torch.empty(B, K, H, 9, 5, 3, device="cuda")
    assert s(inp, out, B, H, flip, tight.ptr, n, noise, seed=9) == 0, s.lib.d3dp_last_error()
    assert tight.intact()
    assert s(inp, ref, B, H, flip, roomy.ptr, 2 * n, noise, seed=9) == 0, s.lib.d3dp_last_error()
    assert roomy.intact()
    assert torch.isfinite(out).all() and torch.equal(out, ref)
    kept = torch.full_like(out, 7.0)
    assert s(inp, kept, B, H, flip, tight.ptr, n - 256, noise, seed=9) == ESTATE and b"ws_bytes" in s.lib.d3dp_last_error()
    assert tight.intact() and bool((kept == 7.0).all())


def test_refusals_leave_preds_untouched():
    B, H, K = 1, 2, 3
    s = RawSampler("exact", 64, 9, 5, 1, K)
    n = s.bytes(B, H, 1)
    inp = s.inputs(B, H)
    ws = Guarded(n)
    kept = torch.full((B, K, H, 9, 5, 3), 7.0, device="cuda")

    def table(flags):
        t = (_lib.DdimStep * K)()
        for i in range(K):
            C.memmove(C.byref(t[i]), C.byref(s.steps[i]), C.sizeof(_lib.DdimStep))
            t[i].last = flags[i]
        return t

    cases = [("K = 0", dict(K=0), EINVAL, b"K = 0"), ("K < 0", dict(K=-2), EINVAL, b"K = -2"),
             ("last set at step 0", dict(steps=table([1, 0, 1])), EINVAL, b"steps[0].last"),
             ("last set in the middle", dict(steps=table([0, 1, 1])), EINVAL, b"steps[1].last"),
             ("last unset at the end", dict(steps=table([0, 0, 0])), EINVAL, b"steps[2].last"),
             ("x2d_flip null with flip", dict(x2f=0), EINVAL, b"x2d_flip"),
             ("x2d_flip given without flip", dict(flip=0, x2f=inp[1].data_ptr()), EINVAL, b"x2d_flip"),
             ("workspace too small", dict(ws_bytes=n - 256), ESTATE, b"ws_bytes")]
    for what, kw, code, needle in cases:
        flip, ws_bytes = kw.pop("flip", 1), kw.pop("ws_bytes", n)
        rc = s(inp, kept, B, H, flip, ws.ptr, ws_bytes, **kw)
        msg = s.lib.d3dp_last_error()
        assert rc == code and needle in msg, (what, rc, msg)
    t = RawSampler("train", 64, 9, 5, 1, K)
    rc = t(inp, kept, B, H, 1, ws.ptr, n)
    assert rc == EINVAL and b"D3DP_MODE_TRAIN" in t.lib.d3dp_last_error(), t.lib.d3dp_last_error()
    big = (1 << 34) + 4                              # the generator's counter word: refused before anything is launched
    assert s.lib.d3dp_op_randn(1, 0, kept.data_ptr(), 0, big, _lib.current_stream()) == EINVAL
    torch.cuda.synchronize()
    assert ws.intact() and bool((kept == 7.0).all())
    assert s(inp, kept, B, H, 1, ws.ptr, n) == 0 and ws.intact() and not bool((kept == 7.0).any())   # (the same arguments, unbroken, run)


@pytest.mark.parametrize("numerics", ["exact", "fast16"])
def test_native_sampler_on_a_side_stream(numerics):
    """The method of tests/test_hip_streams.py (check_case): on a side stream behind a delay, with inputs that arrive late, and
    beside a busy null stream, the call returns while the stream is still busy and computes the default-stream run's bits."""
    B, H, Fr, K = 2, 2, 27, 2
    m = make_model(numerics, 128, 2, Fr, H, K)
    x2d, x2f, noises = inputs(m, B)
    want = sample(m, "python", x2d, x2f, noises)
    m.sampler = "native"
    ref = ts.check_case(ts.sampler_case(m, x2d, x2f, noises), f"native sampler F={Fr} B={B} H={H} K={K} ({numerics})")
    assert ts.bits_equal(ref[0], want)


def test_single_operators_on_a_side_stream():
    """d3dp_op_randn and the two non-flip glue operators under the same two detectors."""
    lib = _lib.load()
    B, H, Fr, J = 2, 3, 5, 17
    n = B * H * Fr * J * 3
    g = rng(3)
    img = torch.randn(B, H, Fr, J, 3, generator=g, dtype=torch.float64).cuda()
    pred, noise = torch.randn(B, H, Fr, J, 3, generator=g).cuda(), torch.randn(B, H, Fr, J, 3, generator=g).cuda()

    def call():
        out, bits = torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        xt, xs, nx = torch.empty(B, H, Fr, J, 3, device="cuda"), torch.empty(B, H, Fr, J, 3, device="cuda"), torch.empty_like(img)
        st = _lib.current_stream()
        _lib.check(lib.d3dp_op_randn(11, 2, out.data_ptr(), bits.data_ptr(), n, st), "d3dp_op_randn")
        _lib.check(lib.d3dp_op_ddim_pre_noflip(img.data_ptr(), xt.data_ptr(), 1.0, 0, B, H, Fr, J, st), "d3dp_op_ddim_pre_noflip")
        _lib.check(lib.d3dp_op_ddim_post_noflip(pred.data_ptr(), img.data_ptr(), noise.data_ptr(), 0, 0, 1.0, 1.5, 1.1, 0.8, 0.5, 0.3, 0,
                                                xs.data_ptr(), H * Fr * J * 3, nx.data_ptr(), B, H, Fr, J, st), "d3dp_op_ddim_post_noflip")
        return [out, bits, xt, xs, nx]
    ref = ts.check_case(ts.Case(call, [img, pred, noise]), "d3dp_op_randn + d3dp_op_ddim_{pre,post}_noflip")
    assert np.array_equal(ref[1].cpu().numpy().view(np.uint32), reference_bits(11, 2, n)) and torch.isfinite(ref[4]).all()


def test_native_sampler_is_capturable():
    """One capture (after eager calls) and two replays per set of new inputs: the bits of the eager call -- no allocation, no
    synchronisation on the capturing thread, the step table's values inside the graph."""
    B, H, Fr, K = 2, 2, 27, 3
    m = make_model("exact", 128, 2, Fr, H, K)
    m.sampler = "native"
    x2d, x2f, noises = inputs(m, B)
    fresh = [list(inputs(m, B, seed=100 + 10 * i)[:2]) + inputs(m, B, seed=100 + 10 * i)[2] for i in range(2)]
    holder = {}

    def run():
        holder["out"] = m(x2d, None, input_2d_flip=x2f, noise=noises)
    got, g = ts._captured(run, [x2d, x2f] + noises, fresh, lambda: [holder["out"]], torch.cuda.Stream())
    for values, (replayed,) in zip(fresh, got):
        eager = sample(m, "python", values[0], values[1], values[2:])
        assert torch.isfinite(eager).all() and ts.bits_equal(eager, replayed)
    assert not ts.bits_equal(got[0][0], got[1][0])


def test_profile_counts_the_sampler_kernels_as_other():
    B, H, K = 1, 2, 3
    s = RawSampler("exact", 64, 9, 5, 1, K)
    n = s.bytes(B, H, 1)
    ws, preds = Guarded(n), torch.empty(B, K, H, 9, 5, 3, device="cuda")
    _lib.check(s.lib.d3dp_profile_enable(s.c.ctx, 1))
    assert s(s.inputs(B, H), preds, B, H, 1, ws.ptr, n) == 0
    cnt, ms = (C.c_int64 * _lib.PROFILE_CLASSES)(), (C.c_double * _lib.PROFILE_CLASSES)()
    _lib.check(s.lib.d3dp_profile_read(s.c.ctx, cnt, ms))
    _lib.check(s.lib.d3dp_profile_enable(s.c.ctx, 0))
    names = [s.lib.d3dp_profile_class_name(i).decode() for i in range(_lib.PROFILE_CLASSES)]
    assert cnt[names.index("other")] == 1 + 2 * K and cnt[names.index("time_mlp")] == K


# ---- 7. command line -----------------------------------------------------------------------------------------------------
def test_cli_evaluates_with_the_native_sampler(tmp_path, capsys):
    from d3dp_amd import cli
    ck = str(tmp_path)
    argv = ["--synthetic", "-c", ck, "-f", "27", "-cs", "64", "-dep", "1", "--synthetic-frames", "60", "--synthetic-sequences", "1",
            "--evaluate", "none.bin", "-num_proposals", "2", "-sampling_timesteps", "2", "-b", "2", "--sampler", "native"]
    assert cli.parse_args(argv).sampler == "native" and cli.parse_args(argv[:-2]).sampler is None
    assert cli.main(argv) == 0
    lines = open(os.path.join(ck, "h36m_test_log_H2_K2.txt")).read().splitlines()
    assert lines[0] == "----synthetic----" and lines[-1] == "----------"
    vals = []
    for ii in range(2):
        for name in ("J_Best", "P_Best", "P_Agg", "J_Agg"):
            row = [l for l in lines if l.startswith("step %d : Protocol #1 Error (MPJPE) %s: " % (ii, name))]
            assert len(row) == 1 and row[0].endswith(" mm"), (ii, name, lines)
            vals.append(float(row[0].rsplit(": ", 1)[1].split()[0]))
    assert len(lines) == 2 + 8 and all(math.isfinite(v) and v > 0 for v in vals), vals
    assert "Protocol #1 Error (MPJPE) J_Agg:" in capsys.readouterr().out
