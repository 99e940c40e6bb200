"""FAST (bf16 operands) and FAST16 (fp16 operands) inference, element by element, against the oracle's fp64 forward pass (run with
``-m gpu`` on an MI355X).

Every other gate of the two 2x modes at denoiser and sampler level is a mean over all B H F 17 joints (``mpjpe_mm <= 8``, ``<= 1.5 x``
the 2-byte emulation's own mean) and every single-op gate an ``allclose`` at about 5 x one correct 2-byte rounding: one wrong tile
passes both.  Here the reference is fp64, there is a per-element figure next to the norm, and the bound comes from the reference
alone: (1.5, 4) x e16 in (norm_rel, max_rms), where e16 is how far the oracle's OWN 2-byte emulation of the same case lies from its
fp64 run (oracle/lowp_check.py; tests/test_fast_elementwise_host.py checks on a CPU that every case below is admissible -- the
emulation's second accumulation order stays within (1.15, 2.0) x e16 -- and that the comparator rejects 32 lost k-columns in 16 rows
of one Linear, which the mean gates accept).

  (a) SHAPES    the smallest shapes that reach each dispatch path, D3DP_FAST_IMPL=mfma at the padded widths included;
  (b) ROUTES    D3DP_LONG_ATTN=rows;
  (c) SCALED    D3DP_FAST16_RANGE=scale on three weight edits (fast16 only) against the UNSCALED fp16 emulation on the edited
                weights;
  (d) SAMPLERS  the public sampler, every step against that step's own e16;
  (e) the single ops (d3dp_op_linear modes FAST and 4, d3dp_op_attention act 1 and 4, d3dp_op_layernorm), the scaled forms of the
      Linear and of the attention kernels included, under the same comparator against the models of oracle/lowp_check.py.

One model -- one context -- per case and mode; every D3DP_* route switch is cleared unless the case sets it; each case asserts the
operand type it ran on.  The case tables are plain data (no GPU needed to import them): the host test walks them too."""
from functools import lru_cache
from types import SimpleNamespace
from typing import NamedTuple, Tuple

import pytest
import torch

from d3dp_amd import D3DP, _lib
from d3dp_amd.model import MixSTE2
from d3dp_amd.weights import (H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, flip_2d, make_state_dict, synthetic_inputs_2d,
                              synthetic_noise)
from oracle import lowp_check as lc
from test_hip_fast16 import FP16_MAX
from test_hip_fast16_scaled import CASES as SCALED_EDITS
from test_hip_fast16_scaled import block_bounds_fp64, edited_state_dict, shifts_fp64

pytestmark = pytest.mark.gpu
# every environment switch d3dp_create reads for an inference context (csrc/capi.hip)
_SWITCHES = ("D3DP_EXACT_IMPL", "D3DP_LONG_ATTN", "D3DP_NO_FOLD", "D3DP_DEFER_NORM", "D3DP_X2_SKEW", "D3DP_X2_PP", "D3DP_X2_WIDE",
             "D3DP_SEQ_PAD", "D3DP_FOLD_LN", "D3DP_FAST_IMPL", "D3DP_FAST16_RANGE", "D3DP_NUMERICS")
SD_SEED, X2D_SEED, X3D_SEED = 11, 911, 912
MODES = {"fast": (torch.bfloat16, "bf16"), "fast16": (torch.float16, "fp16")}
HEADS = 8
MFMA = (("D3DP_FAST_IMPL", "mfma"),)
ROWS = (("D3DP_LONG_ATTN", "rows"),)
SCALE = (("D3DP_FAST16_RANGE", "scale"),)


class Case(NamedTuple):
    cs: int
    Fr: int
    B: int
    H: int
    dep: int = 2
    edit: str = ""                           # a key of EDITS: the weights of a scaled case
    env: Tuple[Tuple[str, str], ...] = ()    # route switches set for this case (every other one is cleared)
    chunk_seqs: int = 0                      # sequences per pass (0: the library's default)
    joints: int = 17

    @property
    def id(self):
        return (f"cs{self.cs}-F{self.Fr}-B{self.B}-H{self.H}" + (f"-dep{self.dep}" if self.dep != 2 else "")
                + (f"-J{self.joints}" if self.joints != 17 else "") + (f"-chunk{self.chunk_seqs}" if self.chunk_seqs else "")
                + (f"-{self.edit}" if self.edit else "") + "".join(f"-{k[5:]}={v}" for k, v in self.env))


class Sampler(NamedTuple):
    cs: int
    Fr: int
    B: int
    H: int
    K: int
    dep: int = 2
    env: Tuple[Tuple[str, str], ...] = ()

    @property
    def id(self):
        return f"cs{self.cs}-F{self.Fr}-B{self.B}-H{self.H}-K{self.K}" + "".join(f"-{k[5:]}={v}" for k, v in self.env)


# (a) the smallest shapes that reach each dispatch path; a pass holds B H sequences of F J token rows
SHAPES = [
    Case(512, 27, 2, 2), Case(256, 27, 2, 2), Case(128, 27, 2, 2),      # spatial and whole-sequence kernel at head dims 64 / 32 / 16
    Case(64, 9, 2, 2),                       # head dim 8: the row kernel
    Case(512, 9, 1, 2),                      # whole key tiles masked
    Case(512, 243, 1, 1),                    # every key tile live
    Case(512, 257, 1, 1),                    # chunked keys, one key in the last chunk
    Case(128, 288, 1, 1),                    # chunked keys at head dim 16, a tile-pair boundary
    Case(512, 3, 1, 2, joints=33), Case(512, 3, 1, 2, joints=40),      # the spatial axis on the whole-sequence kernel
    Case(128, 27, 2, 2, dep=8),              # a deep stack
    Case(512, 9, 2, 3, chunk_seqs=2),        # three passes, two different t across the batch
    # padded heads; the streaming Linear at K / 64 in {3, 5, 6, 7, 10, 12, 14}
    Case(192, 27, 1, 2, env=MFMA), Case(320, 27, 1, 2, env=MFMA), Case(384, 27, 1, 2, env=MFMA), Case(448, 27, 1, 2, env=MFMA),
    Case(192, 257, 1, 1, env=MFMA),          # the padded chunked-key kernel
]
# (b) the row attention kernel taken back: each case has its default twin in SHAPES
ROUTES = [Case(256, 27, 2, 2, env=ROWS), Case(512, 257, 1, 1, env=ROWS)]


def _v_rows_to_3x_range(block):
    """The v rows of one block's qkv matrix times the factor that puts the bound the weights prove for q / k / v at 3 x 65504: the
    block's q, k and v are stored at 2^-2 and, through b_proj, its proj output at 2^-5 -- while q and k, i.e. the softmax, stay as
    they were, so the reference stays well-conditioned (the norm1 edits of test_hip_fast16_scaled.py, the ones that reach a q/k/v
    exponent there, multiply q AND k by 256 ... 1024: their softmax is one-hot on near ties and the fp16 emulation's own distance
    from fp64 moves by 10 x with the accumulation order -- profiles/fast_elementwise.md)."""
    def edit(sd, cs):
        pre = "pose_estimator." + block
        ln = (cs - 1) ** 0.5 * sd[pre + "norm1.weight"].double().abs() + sd[pre + "norm1.bias"].double().abs()
        w = sd[pre + "attn.qkv.weight"].clone()
        bound = (w[2 * cs:].double().abs() @ ln + sd[pre + "attn.qkv.bias"][2 * cs:].double().abs()).max().item()
        w[2 * cs:] *= 3.0 * FP16_MAX / bound
        sd[pre + "attn.qkv.weight"] = w
    return edit


# name -> (None: the weights of test_hip_fast16_scaled.CASES[name] (seed 41) | an edit of the seed state dict,
#          the exponents (s_qkv, s_proj, s_h, s_fc2) it must produce)
EDITS = {"fc1x256": (None, SCALED_EDITS["fc1x256"][4]),
         "tte1-v-rows-to-3x-range": (_v_rows_to_3x_range("TTEblocks.1."), (2, 5, 0, 0)),     # the scaled whole-sequence kernel
         "ste0-v-rows-to-3x-range": (_v_rows_to_3x_range("STEblocks.0."), (2, 5, 0, 0))}     # the scaled spatial kernel
# (c) fast16 only: one edit at each width; together a non-zero exponent in each of q/k/v, proj output, hidden, fc2 output
SCALED = [Case(512, 27, 2, 2, edit="fc1x256", env=SCALE), Case(256, 27, 2, 2, edit="tte1-v-rows-to-3x-range", env=SCALE),
          Case(128, 27, 2, 2, edit="ste0-v-rows-to-3x-range", env=SCALE)]
# (d) the public sampler
SAMPLERS = [Sampler(128, 27, 2, 2, 2), Sampler(128, 27, 2, 2, 3), Sampler(512, 27, 1, 2, 2), Sampler(384, 27, 1, 2, 2, env=MFMA)]
BOTH_MODES = SHAPES + ROUTES


def state_dict_of(case):
    if case.edit:
        assert case.dep == 2 and case.joints == 17
        if EDITS[case.edit][0] is None:
            assert SCALED_EDITS[case.edit][:2] == (case.cs, case.Fr)
            return edited_state_dict(case.edit)
        sd = make_state_dict(SD_SEED, case.cs, case.dep, case.Fr)
        EDITS[case.edit][0](sd, case.cs)
        return sd
    if case.joints != 17:
        return make_state_dict(SD_SEED, case.cs, case.dep, case.Fr, prefix="", joints=case.joints)
    return make_state_dict(SD_SEED, case.cs, case.dep, case.Fr)


def problem(case):
    """(state dict, x2d, x3d, t) of one denoiser case, all on the CPU."""
    sd = state_dict_of(case)
    B, H, Fr, J = case.B, case.H, case.Fr, case.joints
    if J == 17:
        x2d = torch.from_numpy(synthetic_inputs_2d(X2D_SEED, B, Fr))
    else:
        x2d = torch.rand(B, Fr, J, 2, generator=torch.Generator().manual_seed(X2D_SEED)) * 2 - 1
    x3d = torch.from_numpy(synthetic_noise(X3D_SEED, (B, H, Fr, J, 3)))
    return sd, x2d, x3d, torch.tensor([30, 700][:B], dtype=torch.long)


def sampler_problem(case):
    """(state dict, x2d (numpy), the K recorded noise draws) of one sampler case."""
    sd = make_state_dict(SD_SEED, case.cs, case.dep, case.Fr)
    x2d = synthetic_inputs_2d(X2D_SEED, case.B, case.Fr)
    return sd, x2d, [torch.from_numpy(synthetic_noise(X3D_SEED + k, (case.B, case.H, case.Fr, 17, 3))) for k in range(case.K)]


def _shape_only(case):
    """The fp64 run does not depend on the switches: cases that differ in them alone share it."""
    return case._replace(env=())


@lru_cache(maxsize=None)
def _fp64(case):
    if isinstance(case, Sampler):
        sd, x2d, noises = sampler_problem(case)
        return lc.sample_fp64(sd, x2d, noises, case.H, case.K, case.dep)
    sd, x2d, x3d, t = problem(case)
    return lc.denoise_fp64(sd, x2d, x3d, t, case.dep)


@lru_cache(maxsize=None)
def _reference(case, mode):
    dtype = MODES[mode][0]
    if isinstance(case, Sampler):
        sd, x2d, noises = sampler_problem(case)
        return lc.sample_refs(sd, x2d, noises, case.H, case.K, case.dep, dtype, out64=_fp64(case))
    sd, x2d, x3d, t = problem(case)
    return lc.denoise_refs(sd, x2d, x3d, t, case.dep, dtype, out64=_fp64(case))


def reference(case, mode):
    """The oracle's fp64 run of one case (once per case), its emulation in the mode's type under both accumulation orders, e16 and
    spread (once per case and mode): shared, never written to."""
    return _reference(_shape_only(case), mode)


def clear_switches(monkeypatch, env=()):
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)


def denoiser_of(case, sd, mode):
    """(the environment switches are read when the context is created, at the first call: one model per case and mode)"""
    if case.joints != 17:
        m = MixSTE2(num_frame=case.Fr, num_joints=case.joints, embed_dim_ratio=case.cs, depth=case.dep, is_train=False,
                    numerics=mode, drop_path_rate=0.0, chunk_seqs=case.chunk_seqs)
        m.load_state_dict(sd, strict=True)
        return m.cuda().eval()
    args = SimpleNamespace(number_of_frames=case.Fr, test_time_augmentation=True, timestep=1000, scale=1.0, cs=case.cs, dep=case.dep,
                           chunk_seqs=case.chunk_seqs)
    m = D3DP(args, H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, is_train=False, num_proposals=case.H, sampling_timesteps=1, numerics=mode)
    m.load_state_dict(sd, strict=False)
    return m.cuda().eval().pose_estimator


def run_denoiser(monkeypatch, case, mode, env=None):
    clear_switches(monkeypatch, case.env if env is None else env)
    sd, x2d, x3d, t = problem(case)
    net = denoiser_of(case, sd, mode)
    out = net(x2d.cuda(), x3d.cuda(), t.cuda())
    torch.cuda.synchronize()
    return net, out.cpu()


def run_and_check(monkeypatch, case, mode):
    """One pose_estimator(x2d, x3d, t) call of `case` on the GPU: the operand type it ran on, every output element finite and the
    whole (B, H, F, J, 3) output within (1.5, 4) x e16 of the fp64 oracle.  -> (the denoiser, its output on the CPU)."""
    ref = reference(case, mode)
    assert lc.admissible(ref.spread) and ref.finite, (case.id, mode, ref.spread)
    net, out = run_denoiser(monkeypatch, case, mode)
    assert out.shape == ref.out64.shape and out.dtype == torch.float32
    kind, bound = net.fast_operands()
    line, bad, _ = lc.check(f"{mode} inference vs fp64, {case.id} [{kind}]", out, ref.out64, ref.e16, case.chunk_seqs)
    print(line)
    assert kind == MODES[mode][1], (case.id, mode, kind, bound)
    assert torch.isfinite(out).all() and not net.nonfinite_seen()
    b = lc.bounds(ref.e16)
    assert not bad, "\n".join([f"{case.id} {mode}: bounds ({b[0]:.2e}, {b[1]:.2e})"] + bad)
    return net, out


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", SHAPES, ids=lambda c: c.id)
def test_denoiser_elementwise_over_the_dispatch_shapes(monkeypatch, case, mode):
    run_and_check(monkeypatch, case, mode)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", ROUTES, ids=lambda c: c.id)
def test_denoiser_elementwise_on_the_row_attention_route(monkeypatch, case, mode):
    """... and the switch selected another kernel: some bit differs from the default's output (as _report_default_and_rows asserts)."""
    _, out = run_and_check(monkeypatch, case, mode)
    _, default = run_denoiser(monkeypatch, case, mode, env=())
    assert torch.isfinite(default).all() and not torch.equal(out, default)


@pytest.mark.parametrize("case", SCALED, ids=lambda c: c.id)
def test_scaled_fast16_denoiser_elementwise(monkeypatch, case):
    """D3DP_FAST16_RANGE=scale against the UNSCALED fp16 emulation on the edited weights (powers of two commute with the fp16
    rounding while nothing overflows: the host test asserts the emulation's intermediates stay finite).  'fp16' beside a bound of
    65504 or more says the scaled kernels ran (without the switch such weights move the context to bf16); the exponents are those
    the edit must produce."""
    sd = state_dict_of(case)
    blocks = block_bounds_fp64(sd, case.cs, case.dep)
    got = shifts_fp64(blocks)
    print(f"{case.id}: exponents (s_qkv, s_proj, s_h, s_fc2) = {got}")
    assert got == EDITS[case.edit][1] and 0 < max(got) <= 8
    net, out = run_and_check(monkeypatch, case, "fast16")
    kind, bound = net.fast_operands()
    want = max(max(b.values()) for b in blocks)
    assert kind == "fp16" and bound >= FP16_MAX and want * (1 - 1e-6) <= bound <= want * (1 + 1e-3)


def test_the_scaled_cases_cover_every_class_of_exponent():
    got = [EDITS[c.edit][1] for c in SCALED]
    assert all(any(g[i] > 0 for g in got) for i in range(4)), got
    assert sorted(c.cs for c in SCALED) == [128, 256, 512]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", SAMPLERS, ids=lambda c: c.id)
def test_sampler_elementwise_every_step(monkeypatch, case, mode):
    """The public m(x2d, None, input_2d_flip=..., noise=noises): out[:, k] of every step k within (1.5, 4) x that step's e16 of the
    fp64 sampler."""
    clear_switches(monkeypatch, case.env)
    sd, x2d, noises = sampler_problem(case)
    ref = reference(case, mode)
    args = SimpleNamespace(number_of_frames=case.Fr, test_time_augmentation=True, timestep=1000, scale=1.0, cs=case.cs, dep=case.dep)
    m = D3DP(args, H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, is_train=False, num_proposals=case.H, sampling_timesteps=case.K, numerics=mode)
    m.load_state_dict(sd, strict=False)
    m = m.cuda().eval()
    out = m(torch.from_numpy(x2d).cuda(), None, input_2d_flip=torch.from_numpy(flip_2d(x2d)).cuda(), noise=noises)
    torch.cuda.synchronize()
    kind = m.pose_estimator.fast_operands()[0]
    assert out.shape == ref.out64.shape and kind == MODES[mode][1]
    out, bad = out.cpu(), []
    assert torch.isfinite(out).all()
    for k in range(case.K):
        assert lc.admissible(ref.spread[k]), (case.id, mode, k, ref.spread[k])
        line, b, _ = lc.check(f"{mode} sampler vs fp64, {case.id} step {k} [{kind}]", out[:, k], ref.out64[:, k], ref.e16[k])
        print(line)
        bad += b
    assert not bad, "\n".join([f"{case.id} {mode}"] + bad)
    assert not m.pose_estimator.nonfinite_seen()


# ------------------------------------------------------------------------------------------------ (e) the single ops
TYPES = {1: torch.bfloat16, 4: torch.float16}       # act code of the hooks -> the 2-byte type
OP_MODE = {1: _lib.MODE_FAST, 4: _lib.OP_FP16}      # ... and d3dp_op_linear's mode for them
ACTS = [1, 4]
K64_INSTANTIATED, K64_BOTH_EPI, K64_BIAS_ONLY = (1, 2, 4, 8, 16), (3, 5, 6, 7), (10, 12, 14)
SCALED_FLAG = 32


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def check_op(tag, got, op):
    """`got` (CPU) against the unrounded fp64 result within (1.5, 4) x the model's own distance from it; every element finite."""
    line, bad, _ = lc.check(tag, got, op.exact, op.e16)
    print(line)
    assert torch.isfinite(got).all(), bad
    b = lc.bounds(op.e16)
    assert not bad, "\n".join([f"{tag}: bounds ({b[0]:.2e}, {b[1]:.2e})"] + bad)


def op_linear(lib, act, epi, A, W, bias, f32_out=False):
    """d3dp_op_linear on operands of the type (CPU tensors of that dtype) into a NaN-filled output -> the device result on the CPU."""
    (M, K), N = A.shape, W.shape[0]
    Ad, Wd, bd = A.cuda().contiguous(), W.cuda().contiguous(), bias.cuda()
    out = torch.full((M, N), float("nan"), dtype=torch.float32 if f32_out else A.dtype, device="cuda")
    _lib.check(lib.d3dp_op_linear(OP_MODE[act], epi, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), out.data_ptr(), M, N, K,
                                  _lib.current_stream()))
    torch.cuda.synchronize()
    return out.float().cpu()


def linear_operands(seed, M, N, K, dt):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(M, K, generator=g).to(dt), (torch.randn(N, K, generator=g) / K ** 0.5).to(dt), torch.randn(N, generator=g))


def linear_epilogues(k64):
    epis = [("BIAS", _lib.EPI_BIAS, False)]
    if k64 not in K64_BIAS_ONLY:
        epis.append(("GELU", _lib.EPI_GELU, False))
    if k64 in K64_INSTANTIATED:
        epis.append(("BIAS|16", _lib.EPI_BIAS | 16, True))       # the fp32-output form: gemm.hip's own k-depths alone
    return epis


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("M", [17, 300])
@pytest.mark.parametrize("k64", K64_INSTANTIATED + K64_BOTH_EPI + K64_BIAS_ONLY)
def test_linear_op_elementwise(lib, k64, M, act):
    """Every instantiated k-depth of the streaming Linear with every epilogue it has there; M = 17 is a partial tile, M = 300 one
    256-row tile and a remainder; N = 192 ends in half an N tile."""
    N, K, dt = 192, 64 * k64, TYPES[act]
    A, W, bias = linear_operands(M + N + K, M, N, K, dt)
    for name, epi, f32_out in linear_epilogues(k64):
        got = op_linear(lib, act, epi, A, W, bias, f32_out)
        check_op(f"linear act={act} {name} M={M} N={N} K={K}", got, lc.linear_model(A, W, bias, epi & 3, dt))


@pytest.mark.parametrize("act", ACTS)
def test_linear_op_elementwise_more_tiles_than_cus(lib, act):
    """N = 64, K = 64, M = 300 x 256 + 17: 301 tiles of 256 rows on a persistent grid of one workgroup per CU (256 of them): workgroups
    cross tile boundaries with their ring running, and the last tile is partial."""
    M, N, K, dt = 300 * 256 + 17, 64, 64, TYPES[act]
    A, W, bias = linear_operands(M + N + K, M, N, K, dt)
    for name, epi, f32_out in linear_epilogues(1):
        got = op_linear(lib, act, epi, A, W, bias, f32_out)
        check_op(f"linear act={act} {name} M={M} N={N} K={K}", got, lc.linear_model(A, W, bias, epi & 3, dt))


@pytest.mark.parametrize("M", [17, 300])
@pytest.mark.parametrize("k64", K64_INSTANTIATED)
def test_scaled_linear_op_elementwise(lib, k64, M):
    """d3dp_op_linear mode 4 with epi | 32 | (r_in << 8) | (r_out << 12) (gemm_stream_scaled.hip) against the UNSCALED model on the
    values the operands stand for: A holds 2^-r_in times its value, the rows come back at 2^-r_out.  EPI_BIAS with r_in != r_out in
    both orders; EPI_GELU (r_in = 0) with the park rounding of the pre-activation."""
    N, K, dt = 192, 64 * k64, torch.float16
    for name, epi, r_in, r_out in (("BIAS", _lib.EPI_BIAS, 3, 1), ("BIAS", _lib.EPI_BIAS, 0, 5), ("GELU", _lib.EPI_GELU, 0, 2),
                                   ("GELU", _lib.EPI_GELU, 0, 8)):
        A, W, bias = linear_operands(M + N + K + r_in + r_out, M, N, K, dt)
        stored = (A.double() * 2.0 ** -r_in).to(dt)                    # what the kernel reads ...
        value = (stored.double() * 2.0 ** r_in).to(dt)                 # ... and what it stands for (exact: a power of two)
        assert torch.equal(value.double() * 2.0 ** -r_in, stored.double())
        got = op_linear(lib, 4, epi | SCALED_FLAG | (r_in << 8) | (r_out << 12), stored, W, bias) * 2.0 ** r_out
        check_op(f"scaled linear {name} r_in={r_in} r_out={r_out} M={M} N={N} K={K}", got,
                 lc.linear_model(value, W, bias, epi, dt))


def test_scaled_linear_op_refuses_what_it_cannot_run(lib):
    """Bits outside the encoding, exponents beyond 8, EPI_GELU with r_in != 0, a k-depth without a scaled form, and the flag in bf16
    mode (refused there exactly as before) launch nothing."""
    A, W, bias = linear_operands(1, 17, 64, 192, torch.float16)
    Ad, Wd, bd = A.cuda(), W.cuda(), bias.cuda()
    out = torch.zeros(17, 64, dtype=torch.float16, device="cuda")
    call = lambda mode, epi, K: lib.d3dp_op_linear(mode, epi, Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), out.data_ptr(), 17, 64, K,
                                                   _lib.current_stream())
    for epi in (32 | 64, 32 | 2, 32 | 16, 32 | (9 << 8), 32 | (9 << 12), 32 | 1 | (1 << 8), 32 | (1 << 16)):
        assert call(4, epi, 64) == -1, epi
    assert call(4, 32 | (1 << 12), 192) == -1                           # K / 64 = 3: no scaled form
    assert call(_lib.MODE_FAST, 32, 64) == -1 and "epilogues 0, 1 and 0|16" in lib.d3dp_last_error().decode()
    torch.cuda.synchronize()
    assert not out.any()


def qkv_rows(seed, rows, C, dt):
    qkv = torch.randn(rows, 3 * C, generator=torch.Generator().manual_seed(seed))
    qkv[:, :C] *= 2.0        # sharpen the softmax a little
    return qkv.to(dt)


def padded(cs):
    """channels -> (head dim, padded head dim, heads x padded head dim)"""
    hd = cs // HEADS
    hdp = hd if hd in (16, 32, 64) else (32 if hd < 32 else 64)
    return hd, hdp, HEADS * hdp


def op_attention(lib, act, axis, qkv, n_bh, F, J, cs, s=0):
    """d3dp_op_attention impl 1 on `qkv` (CPU, of the type, cs true columns per third) into a NaN-filled output; at a padded width
    through impl 1 | (true head dim << 8) on rows whose heads were padded with zero columns, whose pad columns must come back as exact
    zeros; s: impl 1 | (s << 16).  -> the true columns of the device result on the CPU."""
    hd, hdp, cp = padded(cs)
    rows = qkv.shape[0]
    if hdp != hd:
        p = torch.zeros(rows, 3, HEADS, hdp, dtype=qkv.dtype)
        p[..., :hd] = qkv.reshape(rows, 3, HEADS, hd)
        qkv = p.reshape(rows, 3 * cp)
    impl = 1 | (hd << 8 if hdp != hd else 0) | (s << 16)
    qd = qkv.cuda().contiguous()
    out = torch.full((rows, cp), float("nan"), dtype=qd.dtype, device="cuda")
    _lib.check(lib.d3dp_op_attention(act, impl, axis, qd.data_ptr(), out.data_ptr(), n_bh, F, J, cp, HEADS, _lib.current_stream()))
    torch.cuda.synchronize()
    v = out.float().cpu().reshape(rows, HEADS, hdp)
    assert (v[..., hd:] == 0).all()
    return v[..., :hd].reshape(rows, cs)


WIDTHS = [512, 256, 128, 192, 320, 384, 448]                            # head dims 64 / 32 / 16 and the padded 24 / 40 / 48 / 56
# (axis, n_bh, F, J): the spatial kernel (a partial second key tile / two full ones); the whole-sequence kernel (whole key tiles
# masked ... every tile live; 33 joints on the spatial axis); the chunked-key kernel at test_hip_fast_long.py's edges
ATTN_SHAPES = ([(0, 2, 3, 17), (0, 2, 3, 32), (0, 2, 3, 33)] + [(1, 2, F, 3) for F in (9, 33, 49, 243, 256)]
               + [(1, 1, F, 3) for F in (257, 288, 351, 384, 513)])


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("axis,n_bh,F,J", ATTN_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("cs", WIDTHS)
def test_attention_op_elementwise(lib, cs, axis, n_bh, F, J, act):
    dt = TYPES[act]
    qkv = qkv_rows(F * 7 + cs + J, n_bh * F * J, cs, dt)
    got = op_attention(lib, act, axis, qkv, n_bh, F, J, cs)
    check_op(f"attention act={act} cs={cs} axis={axis} F={F} J={J}", got, lc.attention_model(qkv, n_bh, F, J, cs, HEADS, axis, dt))


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("key_frame", [3, 340])
@pytest.mark.parametrize("cs", [512, 384])
def test_attention_op_elementwise_softmax_spike_across_chunks(lib, cs, key_frame, act):
    """test_attention_softmax_spike_across_chunks' construction at F = 351: the row maximum is set in the first chunk (key at frame 3)
    or jumps in the last (frame 340), where everything accumulated before is rescaled to nearly nothing."""
    n_bh, F, J, dt = 1, 351, 17, TYPES[act]
    qkv = torch.randn(n_bh * F * J, 3 * cs, generator=torch.Generator().manual_seed(5))
    qkv[100 * J + 3, :cs] *= 30.0
    qkv[key_frame * J + 3, cs:2 * cs] = qkv[100 * J + 3, :cs] / 30.0 * 4.0
    qkv = qkv.to(dt)
    got = op_attention(lib, act, 1, qkv, n_bh, F, J, cs)
    check_op(f"attention spike act={act} cs={cs} key at frame {key_frame}", got, lc.attention_model(qkv, n_bh, F, J, cs, HEADS, 1, dt))


@pytest.mark.parametrize("s", [1, 8])
@pytest.mark.parametrize("axis,n_bh,F,J", [(0, 2, 3, 17), (0, 2, 3, 33), (1, 2, 49, 3), (1, 1, 288, 3)], ids=lambda v: str(v))
@pytest.mark.parametrize("cs", [512, 256, 128])
def test_scaled_attention_op_elementwise(lib, cs, axis, n_bh, F, J, s):
    """d3dp_op_attention act 4 with impl 1 | (s << 16) (attention_fast_scaled.hip) on rows that hold 2^-s times their value, against
    the UNSCALED model on the values the rows stand for; the output comes back at v's scale."""
    dt = torch.float16
    stored = (qkv_rows(F * 7 + cs + J + s, n_bh * F * J, cs, dt).double() * 2.0 ** -s).to(dt)
    value = (stored.double() * 2.0 ** s).to(dt)
    assert torch.equal(value.double() * 2.0 ** -s, stored.double())
    got = op_attention(lib, 4, axis, stored, n_bh, F, J, cs, s=s) * 2.0 ** s
    check_op(f"scaled attention s={s} cs={cs} axis={axis} F={F} J={J}", got, lc.attention_model(value, n_bh, F, J, cs, HEADS, axis, dt))


def test_scaled_attention_op_refuses_what_it_cannot_run(lib):
    """s beyond 8, bf16 rows, a padded head dim beside s, head dim 8: D3DP_ENOTSUP, nothing launched."""
    qd = torch.zeros(45, 3 * 512, dtype=torch.float16, device="cuda")
    out = torch.zeros(45, 512, dtype=torch.float16, device="cuda")
    call = lambda act, impl, C_: lib.d3dp_op_attention(act, impl, 1, qd.data_ptr(), out.data_ptr(), 1, 9, 5, C_, HEADS, _lib.current_stream())
    for act, impl, C_ in ((4, 1 | (9 << 16), 512), (1, 1 | (1 << 16), 512), (4, 1 | (48 << 8) | (1 << 16), 512), (4, 1 | (1 << 16), 64)):
        assert call(act, impl, C_) == -2, (act, impl, C_)
    torch.cuda.synchronize()
    assert not out.any()


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("C", [128, 192, 512])
def test_layernorm_op_elementwise(lib, C, act):
    """d3dp_op_layernorm with 2-byte rows out: the instantiated-width kernels (128, 512) and the run-time-width one (192); T = 67 ends
    in a partly filled workgroup."""
    T, dt = 67, TYPES[act]
    g = torch.Generator().manual_seed(C + T)
    x = torch.randn(T, C, generator=g) * 3 + 0.5
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    out = torch.full((T, C), float("nan"), dtype=dt, device="cuda")
    _lib.check(lib.d3dp_op_layernorm(act, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), 1e-6, out.data_ptr(), T, C, _lib.current_stream()))
    torch.cuda.synchronize()
    check_op(f"layernorm act={act} C={C} T={T}", out.float().cpu(), lc.layernorm_model(x, w, b, 1e-6, dt))
