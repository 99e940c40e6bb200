"""GPU tests (-m gpu) of the kernels around the denoiser, each alone and bit for bit against oracle/glue_check.py:
d3dp_ddim_pre, d3dp_ddim_post, the whole sampler loop with the denoiser replaced by three exactly reproducible
elementwise operations, d3dp_q_sample, and d3dp_jpma / _ex / _gathered / _winners / _combine.

Every comparison is ``bits_equal`` (equal NaN masks, equal bit patterns elsewhere, the sign of zero included) over the
whole output, which lies in a buffer prefilled with a sentinel so that an element never written shows as well.  The one
bounded comparison is JPMA's hypothesis mean, a sequential fp32 sum whose order torch.mean does not share; its bound is
glue_check.mean_bound.  What the reference does on the planted edges is recorded in tests/test_glue_host.py;
profiles/glue_bitwise.md says which of these tests found what."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from d3dp_amd import D3DP, D3DP3DHP, _lib, jpma
from d3dp_amd import eval3dhp as e3
from d3dp_amd.weights import H36M_JOINTS_LEFT as KL, H36M_JOINTS_RIGHT as KR, flip_2d, synthetic_inputs_2d
from oracle import d3dp_oracle as orc
from oracle import glue_check as gc

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
SENTINEL = 12345.0
GUARD = 64                                     # sentinel elements past the end of every output: must survive
SHAPES = [(1, 1, 1, 17), (2, 3, 5, 17), (3, 2, 43, 17)]                 # 17 rows (one partial block); 510; 4386
SCALES = [1.0, 0.5, 3.0, 0.75]                                           # exact in fp32: the ABI receives float
PERMS = {"h36m": (KL, KR), "identity": ([], []), "cycle17": ([0], list(range(1, 17)))}
TIME_PAIRS = [(999, 899), (499, 399), (99, -1), (1, 0), (0, -1)]


class Cmp:
    """Collects every bitwise comparison of a test and fails once, naming each output that differs and on how many
    of its elements."""

    def __init__(self):
        self.bad = []

    def eq(self, name, got, want):
        got, want = got.detach().cpu(), want.detach().cpu()
        if got.shape != want.shape or got.dtype != want.dtype:
            self.bad.append(f"{name}: {tuple(got.shape)} {got.dtype} vs {tuple(want.shape)} {want.dtype}")
            return
        n = gc.bit_mismatches(got, want)
        if n:
            self.bad.append(f"{name}: {n} of {got.numel()} elements differ")

    def done(self):
        if self.bad:
            pytest.fail("\n".join(self.bad), pytrace=False)


def perm_tensor(jl, jr):
    perm = list(range(17))
    for dst, src in zip(jl + jr, jr + jl):
        perm[dst] = src
    return torch.tensor(perm, dtype=torch.int32, device="cuda")


def out_buffer(shape, dtype=torch.float32):
    """A contiguous output of ``shape`` followed by GUARD more elements, all holding the sentinel."""
    n = int(np.prod(shape))
    flat = torch.full((n + GUARD,), SENTINEL if dtype.is_floating_point else 12345, dtype=dtype, device="cuda")
    return flat, flat[:n].view(shape)


def guard_intact(flat):
    return bool((flat[-GUARD:] == (SENTINEL if flat.dtype.is_floating_point else 12345)).all())


def plant(x, values, stride=4, both_ends=True):
    """Writes ``values`` into the flattened ``x`` every ``stride`` elements from element 1 and, for a tensor of more
    than one block, again backwards from its end (the last, partial block)."""
    flat = x.view(-1)
    assert 1 + stride * len(values) <= flat.numel()
    for k, v in enumerate(values):
        flat[1 + stride * k] = v
        if both_ends and flat.numel() > 1024:
            flat[flat.numel() - 2 - stride * k] = v
    return x


def rng(seed):
    return torch.Generator().manual_seed(seed)


# ---- d3dp_ddim_pre ----------------------------------------------------------------------------------------------------
def clamp_edges(scale):
    lim = np.float32(1.1 * scale)                                         # the reference's bound: the double, rounded once
    up, dn = np.nextafter(lim, np.float32(np.inf)), np.nextafter(lim, np.float32(0))
    return [float(v) for v in (lim, -lim, up, dn, -up, -dn)] + [INF, -INF, NAN, -0.0, 1e-40, -1e-40]


# 9.0 is one more exact scale, for this kernel only: its output is bound / scale, and at 3.0 and 0.75 the two candidate
# bounds fp32(1.1 * s) and 1.1f * s, one ulp apart, divide to the same fp32 value; at 9.0 they do not
@pytest.mark.parametrize("perm", list(PERMS))
@pytest.mark.parametrize("scale", SCALES + [9.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_ddim_pre_alone(shape, scale, perm):
    B, H, Fr, J = shape
    jl, jr = PERMS[perm]
    img = plant(torch.randn(B, H, Fr, J, 3, generator=rng(B * 100 + Fr)) * scale, clamp_edges(scale))
    sat = (img.abs() > 1.1 * scale).float().mean().item()
    assert shape == SHAPES[0] or 0.15 < sat < 0.4, sat
    x_t, x_t_flip = gc.ddim_pre_ref(img, scale, jl, jr)
    flat, xt2 = out_buffer((2 * B, H, Fr, J, 3))
    d_img = img.cuda()
    _lib.check(_lib.load().d3dp_ddim_pre(d_img.data_ptr(), xt2.data_ptr(), perm_tensor(jl, jr).data_ptr(), scale, B, H, Fr, J,
                                         _lib.current_stream()), "d3dp_ddim_pre")
    torch.cuda.synchronize()
    c = Cmp()
    c.eq("x_t", xt2[:B], x_t)
    c.eq("x_t_flip", xt2[B:], x_t_flip)
    c.eq("img (input)", d_img, img)
    c.done()
    assert guard_intact(flat)


# ---- d3dp_ddim_post ---------------------------------------------------------------------------------------------------
def host_coefficients(sched_np, time, time_next, eta):
    """The sampler's scalars as d3dp_amd/model.py forms them: Python doubles through math.sqrt."""
    ac = sched_np["alphas_cumprod"]
    if time_next < 0:
        return 0.0, 0.0, 0.0
    alpha, alpha_next = ac[time], ac[time_next]
    sg = eta * math.sqrt((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha))
    return math.sqrt(alpha_next), math.sqrt(1 - alpha_next - sg ** 2), sg


@pytest.fixture(scope="module")
def sched():
    s = orc.cosine_schedule(1000)
    return s, {k: v.numpy() for k, v in s.items()}


@pytest.mark.parametrize("perm", list(PERMS))
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", SHAPES)
def test_ddim_post_alone(sched, shape, scale, perm):
    sched_t, sched_np = sched
    lib = _lib.load()
    B, H, Fr, J = shape
    jl, jr = PERMS[perm]
    g = rng(B * 1000 + Fr + len(jl))
    full = (B, H, Fr, J, 3)
    per_b, K = H * Fr * J * 3, 3
    pred2 = plant(torch.randn((2 * B,) + full[1:], generator=g), [NAN, INF, -INF, -0.0], stride=5)
    img = plant(torch.randn(full, generator=g) * scale, [INF, NAN, -0.0], stride=11, both_ends=False)
    noise = plant(torch.randn(full, generator=g), [NAN, -INF, INF], stride=7, both_ends=False)
    d_pred2, d_img, d_noise, d_perm = pred2.cuda(), img.cuda(), noise.cuda(), perm_tensor(jl, jr)
    c = Cmp()
    for time, time_next in TIME_PAIRS:
        for eta in (1.0, 0.0):
            last = time_next < 0
            x_start, img_next = gc.ddim_post_ref(pred2[:B], pred2[B:], img, noise, sched_t, time, time_next, scale, eta, jl, jr)
            if shape != SHAPES[0]:
                sat = (x_start.abs() == float(np.float32(1.1 * scale))).float().mean().item()
                assert 0.05 < sat < 0.25, sat
            c_x, c_n, sigma = host_coefficients(sched_np, time, time_next, eta)
            for aliased in (False, True):
                xs_flat, xs = out_buffer((B, K) + full[1:])
                if aliased:
                    nx_flat = torch.cat((d_img.reshape(-1), torch.full((GUARD,), SENTINEL, device="cuda")))
                    nx = src = nx_flat[:B * per_b].view(full)
                else:
                    (nx_flat, nx), src = out_buffer(full), d_img
                _lib.check(lib.d3dp_ddim_post(d_pred2.data_ptr(), src.data_ptr(), 0 if last else d_noise.data_ptr(),
                                              d_perm.data_ptr(), scale, float(sched_np["sqrt_recip_alphas_cumprod"][time]),
                                              float(sched_np["sqrt_recipm1_alphas_cumprod"][time]), c_x, c_n, sigma, int(last),
                                              xs[:, 1].data_ptr(), K * per_b, nx.data_ptr(), B, H, Fr, J,
                                              _lib.current_stream()), "d3dp_ddim_post")
                torch.cuda.synchronize()
                tag = f"t={time}->{time_next} eta={eta:g} aliased={aliased}"
                c.eq(f"x_start [{tag}]", xs[:, 1], x_start)
                c.eq(f"x_start's other k [{tag}]", xs[:, [0, 2]], torch.full((B, 2) + full[1:], SENTINEL))
                if last:                               # img_next is not written: whatever it held survives
                    c.eq(f"img_next untouched [{tag}]", nx, img if aliased else torch.full(full, SENTINEL))
                else:
                    c.eq(f"img_next [{tag}]", nx, img_next)
                assert guard_intact(xs_flat) and guard_intact(nx_flat), tag
    c.eq("pred2 (input)", d_pred2, pred2)
    c.eq("noise (input)", d_noise, noise)
    c.done()


# ---- the whole loop, the denoiser taken out ---------------------------------------------------------------------------
LOOP_B, LOOP_H, LOOP_F = 2, 3, 27


@pytest.fixture(scope="module")
def loop_inputs():
    x2d = synthetic_inputs_2d(11, LOOP_B, LOOP_F)
    noises = torch.randn(1000, LOOP_B, LOOP_H, LOOP_F, 17, 3, generator=rng(77))
    return torch.from_numpy(x2d), torch.from_numpy(flip_2d(x2d)), noises


def stub(x2, xt2, t2, out):
    out.copy_(gc.stub_denoiser(x2, xt2, t2))
    return out


def run_loop(cls, jl, jr, loop_inputs, monkeypatch, K, eta, scale):
    x2, x2f, noises = loop_inputs
    noises = list(noises[:K])
    monkeypatch.setattr(orc, "mixste_forward", lambda p, x2d, x3, t, depth: gc.stub_denoiser(x2d, x3, t))
    want = orc.ddim_sample_flip({}, orc.cosine_schedule(1000), x2, x2f, LOOP_H, K, 2, jl, jr, noises, scale=scale, eta=eta)
    args = SimpleNamespace(number_of_frames=LOOP_F, test_time_augmentation=True, timestep=1000, scale=scale, cs=128, dep=2)
    m = cls(args, jl, jr, is_train=False, num_proposals=LOOP_H, sampling_timesteps=K, numerics="exact").cuda().eval()
    m.ddim_sampling_eta = eta
    m.pose_estimator.denoise = stub
    out = m(x2.cuda(), None, input_2d_flip=x2f.cuda(), noise=noises)
    torch.cuda.synchronize()
    return out, want


def test_stub_denoiser_is_bit_reproducible_on_the_gpu(loop_inputs):
    x2, x2f, noises = loop_inputs
    t = torch.zeros(LOOP_B, dtype=torch.long)
    c = Cmp()
    for scale in (1.0, 3.0):
        for x2d, x_t in zip((x2, x2f), gc.ddim_pre_ref(noises[0], scale, KL, KR)):
            c.eq(f"f at scale {scale:g}", gc.stub_denoiser(x2d.cuda(), x_t.cuda(), t.cuda()), gc.stub_denoiser(x2d, x_t, t))
    c.done()


@pytest.mark.parametrize("K,eta,scale", [(K, eta, s) for K in (1, 3, 10) for eta in (1.0, 0.0) for s in (1.0, 3.0)] +
                         [(1000, 1.0, 1.0)])
def test_sampler_loop_without_denoiser(loop_inputs, monkeypatch, K, eta, scale):
    """Time pairs, host coefficient arithmetic, noise order, the preds[:, k] stride and the in-place img."""
    out, want = run_loop(D3DP, KL, KR, loop_inputs, monkeypatch, K, eta, scale)
    c = Cmp()
    c.eq("preds", out, want)
    c.done()


def test_sampler_loop_without_denoiser_3dhp(loop_inputs, monkeypatch):
    out, want = run_loop(D3DP3DHP, e3.KPS_LEFT_3DHP, e3.KPS_RIGHT_3DHP, loop_inputs, monkeypatch, 3, 1.0, 1.0)
    c = Cmp()
    c.eq("preds (mm)", out, want * D3DP3DHP.MM)
    c.done()


# ---- prepare_targets / d3dp_q_sample ------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
def test_prepare_targets_alone(scale):
    B, Fr, T = 3, 27, [0, 1, 500, 998, 999]
    g = rng(int(scale * 100))
    args = SimpleNamespace(number_of_frames=Fr, test_time_augmentation=True, timestep=1000, scale=scale, cs=128, dep=2)
    m = D3DP(args, KL, KR, is_train=True).cuda()
    x0 = plant(torch.randn(B, Fr, 17, 3, generator=g) * 0.9, [NAN, INF, -INF, -0.0, 1e-40], stride=9)
    noise = plant(torch.randn(B, Fr, 17, 3, generator=g), [INF, NAN, -INF, NAN], stride=13)
    sched = orc.cosine_schedule(1000)
    c = Cmp()
    for i in range(len(T)):
        t = torch.tensor([T[i], T[(i + 1) % 5], T[(i + 2) % 5]], dtype=torch.long)
        want = orc.prepare_targets(sched, x0, t, noise, scale=scale)
        sat = (want.abs() == float(np.float32(np.float32(1.1 * scale) / np.float32(scale)))).float().mean().item()
        assert sat > 0.02, sat
        got, n_out, t_out = m.prepare_targets(x0.cuda(), t=t[:, None], noise=noise)
        torch.cuda.synchronize()
        c.eq(f"x_t at t={t.tolist()}", got, want)
        c.eq("noise passed through", n_out, noise)
        assert torch.equal(t_out.cpu(), t[:, None])
    c.done()


# ---- JPMA -------------------------------------------------------------------------------------------------------------
JPMA_SHAPES = [(1, 1, 1, 1, 17), (2, 2, 5, 3, 17), (3, 2, 6, 9, 17)]     # (B, K, H, F, J): 17, 204 and 918 threads
H36M_CAM = [2.29, 2.287, 0.0254, 0.0289, -0.2070, 0.2477, -0.0030, -0.0009, -0.0014]
PIXEL_CAM = [1497.7, 1501.2, 1021.3, 998.6, 0.0, 0.0, 0.0, 0.0, 0.0]
CAMERAS = {"h36m": (H36M_CAM, 0, 0, 1.0), "3dhp": (PIXEL_CAM, 14, 1, 1000.0), "noroot": (H36M_CAM, -1, 0, 1.0)}
VARIANTS = ["base", "two_equal", "all_equal", "zero_depth", "small_depth", "nan_one", "nan_every_h", "nan_gt2d", "inf_gt2d",
            "nan_gt3d", "zero_traj"]


def jpma_case(shape, camera, variant):
    """One base problem per (shape, camera) and one planted edge per variant.  The edges sit on frame 0 (every shape
    has it), on joints 3, 5, 9 and 16 (none is a root) and, for ``zero_traj``, on the root."""
    B, K, H, Fr, J = shape
    cam, root, linear, unit = CAMERAS[camera]
    g = rng(B * 37 + H + (5 if linear else 0))
    pred = torch.randn(B, K, H, Fr, J, 3, generator=g) * 0.3 * unit
    traj = (torch.randn(B, Fr, 1, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 4.0])) * unit
    gt3 = torch.randn(B, Fr, J, 3, generator=g) * 0.3 * unit
    gt2 = (torch.randn(B, Fr, J, 2, generator=g) * 150 + 1000) if linear else torch.rand(B, Fr, J, 2, generator=g) * 2 - 1
    h1, h2, b, k = 1 % H, (H - 1), B - 1, K - 1
    if variant == "two_equal":
        pred[:, :, h2] = pred[:, :, h1]
    elif variant == "all_equal":
        pred[:] = pred[:, :, :1].clone()
    elif variant == "zero_depth":                       # X / 0 = +-inf -> +-1; joint 9 of h1 also has X = 0: 0 / 0
        for j in (3, 5, 9):
            pred[b, :, h1, 0, j, 2] = -traj[b, 0, 0, 2]
            pred[0, k, :, 0, j, 2] = -traj[0, 0, 0, 2]
        pred[b, :, h1, 0, 9, 0] = -traj[b, 0, 0, 0]
    elif variant == "small_depth":                      # |X / Z| > 1 for most joints of these frames
        traj[:, 0, 0, 2] = 0.05 * unit
        traj[b, Fr - 1, 0, 2] = -0.02 * unit
    elif variant == "nan_one":
        pred[b, k, h1, 0, 3, 1] = NAN
        pred[0, 0, h2, 0, 5, 2] = NAN
        pred[0, 0, 0, 0, 16, 0] = NAN
    elif variant == "nan_every_h":
        pred[b, k, :, 0, 5, 0] = NAN
        pred[0, 0, :, 0, 16, 2] = NAN
    elif variant == "nan_gt2d":
        gt2[b, 0, 3, 0] = NAN
        gt2[0, 0, 16, 1] = NAN
    elif variant == "inf_gt2d":
        gt2[b, 0, 5, 1] = INF
        gt2[0, 0, 9, 0] = INF
    elif variant == "nan_gt3d":
        gt3[b, 0, 9, 2] = NAN
        gt3[0, 0, 3, 0] = NAN
    elif variant == "zero_traj":                        # the zeroed root projects 0 / 0 in every hypothesis
        traj[b, 0] = 0.0
    return pred, traj, torch.tensor(cam), gt2, gt3, root, linear


def check_mean(c, name, got, pred, mean64, root):
    """Finite means within the derived bound; a NaN or infinite mean must be the same NaN or infinity."""
    got = got.detach().cpu().double()
    fin = torch.isfinite(mean64)
    n = int(((got - mean64).abs() > gc.mean_bound(pred, root))[fin].sum())
    n += int(((got != mean64) & ~(torch.isnan(got) & torch.isnan(mean64)))[~fin].sum())
    if n:
        c.bad.append(f"{name}: {n} of {got.numel()} elements beyond the bound")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("camera", list(CAMERAS))
@pytest.mark.parametrize("shape", JPMA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_jpma_alone(shape, camera, variant):
    lib = _lib.load()
    B, K, H, Fr, J = shape
    pred, traj, cam, gt2, gt3, root, linear = jpma_case(shape, camera, variant)
    agg, sel, es, em, jb, mean64 = gc.jpma_ref(pred, traj, cam, gt2, gt3, root, bool(linear))
    d_pred, d_traj, d_cam, d_gt2, d_gt3 = (x.cuda().contiguous() for x in (pred, traj.reshape(B, Fr, 3), cam, gt2, gt3))
    st = _lib.current_stream()
    c = Cmp()
    flats = []

    def outs():
        o = [out_buffer((B, K, Fr, J, 3)), out_buffer((B, K, Fr, J), torch.int32), out_buffer((B, K, Fr, J)),
             out_buffer((B, K, Fr, J)), out_buffer((B, K, Fr, J, 3)), out_buffer((B, K, Fr, J, 3))]
        flats.extend(f for f, _ in o)
        return [v for _, v in o]

    def check4(tag, o):
        c.eq(f"{tag} agg", o[0], agg)
        c.eq(f"{tag} sel", o[1], sel)
        c.eq(f"{tag} err_sel", o[2], es)
        c.eq(f"{tag} err_min", o[3], em)

    o = outs()
    _lib.check(lib.d3dp_jpma_ex(d_pred.data_ptr(), d_traj.data_ptr(), d_cam.data_ptr(), d_gt2.data_ptr(), d_gt3.data_ptr(),
                                *(x.data_ptr() for x in o), B, K, H, Fr, J, root, linear, st), "d3dp_jpma_ex")
    check4("jpma_ex", o)
    c.eq("jpma_ex jbest", o[4], jb)
    check_mean(c, "jpma_ex mean", o[5], pred, mean64, root)

    if not linear:                                      # the other entry points: distortion model, root 0 or none
        zr = int(root == 0)
        o = outs()
        _lib.check(lib.d3dp_jpma(d_pred.data_ptr(), d_traj.data_ptr(), d_cam.data_ptr(), d_gt2.data_ptr(), d_gt3.data_ptr(),
                                 *(x.data_ptr() for x in o[:4]), B, K, H, Fr, J, zr, st), "d3dp_jpma")
        check4("jpma", o)
        parts = list(torch.split(pred, 2, dim=2))       # ranks of 2 hypotheses (the last may hold 1)
        if H % 2 == 0:                                  # the all-gather layout (R, B, K, H_local, F, J, 3), read in place
            gathered = torch.stack(parts).cuda().contiguous()
            o = outs()
            _lib.check(lib.d3dp_jpma_gathered(gathered.data_ptr(), d_traj.data_ptr(), d_cam.data_ptr(), d_gt2.data_ptr(),
                                              d_gt3.data_ptr(), *(x.data_ptr() for x in o[:4]), len(parts), B, K, 2, Fr, J,
                                              zr, st), "d3dp_jpma_gathered")
            check4(f"jpma_gathered R={len(parts)}", o)
        wins = []
        for r, part in enumerate(parts):
            wf, w = out_buffer((B, K, Fr, J, 5))
            flats.append(wf)
            _lib.check(lib.d3dp_jpma_winners(part.cuda().contiguous().data_ptr(), d_traj.data_ptr(), d_cam.data_ptr(),
                                             d_gt2.data_ptr(), w.data_ptr(), 2 * r, B, K, part.shape[2], Fr, J, zr, st),
                       "d3dp_jpma_winners")
            c.eq(f"winners of rank {r}", w, gc.jpma_winners_ref(part, traj, cam, gt2, root, False, h_offset=2 * r))
            wins.append(w)
        wins = torch.stack(wins).contiguous()
        (af, a2), (sf, s2) = out_buffer((B, K, Fr, J, 3)), out_buffer((B, K, Fr, J), torch.int32)
        flats += [af, sf]
        _lib.check(lib.d3dp_jpma_combine(wins.data_ptr(), len(parts), B * K * Fr * J, a2.data_ptr(), s2.data_ptr(), st),
                   "d3dp_jpma_combine")
        c.eq("combine agg", a2, agg)
        c.eq("combine sel", s2, sel)
        a3, s3 = jpma.jpma_combine(wins.cpu())          # the host statement of the same step
        c.eq("host combine agg", a3, agg)
        c.eq("host combine sel", s3, sel)
    torch.cuda.synchronize()
    c.done()
    assert all(guard_intact(f) for f in flats)


def test_jpma_variants_plant_what_they_say():
    """The edge variants reach the reference: each changes the selection or an error of its base case somewhere."""
    shape = JPMA_SHAPES[2]
    for camera in CAMERAS:
        base = gc.jpma_ref(*jpma_case(shape, camera, "base"))
        for variant in VARIANTS[1:]:
            got = gc.jpma_ref(*jpma_case(shape, camera, variant))
            assert any(gc.bit_mismatches(a, b) for a, b in zip(got, base)), (camera, variant)
    for camera in CAMERAS:                              # ties exist and resolve to the lowest h
        pred, traj, cam, gt2, gt3, root, linear = jpma_case(shape, camera, "all_equal")
        assert not gc.jpma_ref(pred, traj, cam, gt2, gt3, root, bool(linear))[1].any()
