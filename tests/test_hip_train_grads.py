"""Every training gradient, element by element, against the oracle's fp64 autograd (run with ``-m gpu`` on an MI355X).

The older comparisons with autograd bound the whole-tensor figure ||g - ref|| / ||ref|| by 2e-3 or 5e-3 against the fp32 oracle; a
split-fp16 product that loses one of its three passes is off by 2^-11 = 4.9e-4 and passes them, one wrong 16-row tile by a wider
margin still.  Here the reference is fp64, there is a per-element figure next to the norm, and the bound comes from the reference
alone: 8 x e32, where e32 is how far the oracle's OWN fp32 autograd lies from its fp64 autograd in the same case
(oracle/grad_check.py; tests/test_train_grads_host.py checks on a CPU that every case below is well-conditioned and that the
comparator rejects a dropped cross pass in one tile).

The public training step is driven as tests/test_hip_train_heads.py drives it: J = 17, dep = 2 unless said otherwise, the default
path (every D3DP_TRAIN_* switch cleared), one model -- one context -- per case.  The case tables are plain data (no GPU needed to
import them): the host test walks them too."""
from functools import lru_cache
from types import SimpleNamespace
from typing import NamedTuple

import pytest
import torch

from d3dp_amd import D3DP
from d3dp_amd.weights import H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, make_state_dict, synthetic_inputs_2d, synthetic_noise
from oracle import grad_check as gc

pytestmark = pytest.mark.gpu
_SWITCHES = ("D3DP_TRAIN_ATTN", "D3DP_TRAIN_ATTN_BWD", "D3DP_TRAIN_IMPL", "D3DP_TRAIN_WGRAD")
# (the seeds of test_hip_train_heads' cross-check test.  Those of its autograd tests, 7 / 901, put the cs = 512 outlier-row case at
#  e32(max_rms) = 5.16e-5, over the admissibility cap, by the reference alone: with these it is 2.3e-5)
SD_SEED, INPUT_SEED, MASK_SEED = 11, 911, 5
PRE = "pose_estimator."


class Case(NamedTuple):
    cs: int
    Fr: int
    B: int
    dep: int = 2
    edit: str = ""             # a key of EDITS: one change to the seed state dict
    masks: str = "recorded"    # "recorded": drawn at the model's rates; "dropped": two branches dropped for every sample

    @property
    def id(self):
        return (f"cs{self.cs}-F{self.Fr}-B{self.B}" + (f"-dep{self.dep}" if self.dep != 2 else "")
                + (f"-{self.edit}" if self.edit else "") + ("-dropped" if self.masks == "dropped" else ""))


# (a) the smallest shapes that reach each dispatch case; T = B F 17 tokens
SHAPES = [
    Case(512, 9, 1),           # T = 153: one 256-row tile with padded rows; n <= 32, the one-kernel attention backward
    Case(512, 9, 2),           # T = 306: M > 256 with a 50-row remainder
    Case(512, 40, 2),          # 4 key tiles
    Case(512, 81, 2),          # 8 key tiles
    Case(512, 243, 1),         # two wave groups, ragged last tiles
    Case(512, 300, 1),         # chunked keys and queries
    Case(256, 9, 2), Case(256, 40, 2), Case(256, 243, 1), Case(256, 300, 1),
    Case(128, 9, 2), Case(128, 81, 2), Case(128, 300, 1),     # qkv N = 384: the transposed-operand wgrad path
    Case(128, 9, 2, dep=8),    # the reduce, zero and weight-prep tables fill with depth
    Case(64, 27, 2),           # head dim 8: fp32 attention under split Linears
    Case(96, 27, 2),           # train_g.hip, run-time width
]


def _scale(name, f):
    def edit(sd, cs):
        sd[PRE + name] = sd[PRE + name] * f
    return edit


def _outlier_v_row(sd, cs):
    """One v channel 256 times larger in both axes' qkv: it alone sets the tensor's absmax, every other value's lo plane moves
    eight binades toward the fp16 subnormals -- the case a per-tensor scale is weakest at."""
    for blk in ("STEblocks.1", "TTEblocks.1"):
        w = sd[PRE + blk + ".attn.qkv.weight"].clone()
        w[2 * cs + 5] *= 256
        sd[PRE + blk + ".attn.qkv.weight"] = w


# (b) one edit of the seed state dict each: the device-side scales (dyn_scale, ta_scale, ta_split_run) leave their usual exponents
EDITS = {
    "ste1-qkv-x4": _scale("STEblocks.1.attn.qkv.weight", 4.0),
    "tte1-qkv-x4": _scale("TTEblocks.1.attn.qkv.weight", 4.0),
    "ste1-fc1-x50": _scale("STEblocks.1.mlp.fc1.weight", 50.0),
    "tte0-norm2-x300": _scale("TTEblocks.0.norm2.weight", 300.0),
    "tte1-fc2-x2^-10": _scale("TTEblocks.1.mlp.fc2.weight", 2.0 ** -10),
    "outlier-v-row-x256": _outlier_v_row,
}
MAGNITUDES = [Case(cs, 27, 2, edit=e) for cs in (512, 128) for e in EDITS]
# (c) STEblocks.1's attention branch and TTEblocks.1's MLP branch dropped for every sample
DROPPED = [Case(512, 27, 2, masks="dropped"), Case(128, 9, 2, masks="dropped")]
DROPPED_PARAMS = ([f"STEblocks.1.{n}" for n in ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight",
                                                "attn.proj.bias")]
                  + [f"TTEblocks.1.{n}" for n in ("norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight",
                                                  "mlp.fc2.bias")])
# (d) the upstream gradient times 2^k
UPSTREAM = [Case(256, 40, 2), Case(512, 9, 2)]
UPSTREAM_K = (-40, 0, 30)
ALL_CASES = list(dict.fromkeys(SHAPES + MAGNITUDES + DROPPED + UPSTREAM))


def problem(case):
    """(state dict, x2d, gt, t, noise, DropPath masks) of one case, all on the CPU."""
    sd = make_state_dict(SD_SEED, case.cs, case.dep, case.Fr)
    if case.edit:
        EDITS[case.edit](sd, case.cs)
    B, Fr = case.B, case.Fr
    x2d = torch.from_numpy(synthetic_inputs_2d(INPUT_SEED, B, Fr))
    gt = torch.from_numpy(synthetic_noise(INPUT_SEED + 1, (B, Fr, 17, 3))) * 0.3
    gt[:, :, 0] = 0
    noise = torch.from_numpy(synthetic_noise(INPUT_SEED + 2, (B, Fr, 17, 3)))
    t = torch.tensor([[30], [700]][:B], dtype=torch.long)
    dpd = {}
    if case.masks == "dropped":
        one, zero = (lambda S: torch.ones(S, 1, 1)), (lambda S: torch.zeros(S, 1, 1))
        dpd["STEblocks.1"] = (zero(B * Fr), one(B * Fr))
        dpd["TTEblocks.1"] = (one(B * 17), zero(B * 17))
    else:       # recorded masks of the blocks behind the first (timm semantics: 0 or 1 / keep), as test_hip_train_heads draws them
        rates = [x.item() for x in torch.linspace(0, 0.1, case.dep)]
        gen = torch.Generator().manual_seed(MASK_SEED)
        for i in range(1, case.dep):
            keep = 1 - rates[i]
            mk = lambda S: (torch.rand(S, 1, 1, generator=gen) < keep).float() / keep
            dpd[f"STEblocks.{i}"] = (mk(B * Fr), mk(B * Fr))
            dpd[f"TTEblocks.{i}"] = (mk(B * 17), mk(B * 17))
    return sd, x2d, gt, t, noise, dpd


@lru_cache(maxsize=2)
def reference(case):
    """The oracle's fp64 and fp32 step of one case and the e32 they define: computed once, shared, never written to."""
    sd, x2d, gt, t, noise, dpd = problem(case)
    return gc.reference_pair(sd, x2d, gt, t, noise, case.dep, dpd)


def model_of(case, sd):
    """(the environment switches are read when the context is created, at the first step: one model per case)"""
    args = SimpleNamespace(number_of_frames=case.Fr, test_time_augmentation=True, timestep=1000, scale=1.0, cs=case.cs, dep=case.dep)
    m = D3DP(args, H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, is_train=True)
    m.load_state_dict(sd, strict=False)
    return m.cuda().train()


def step(m, x2d, gt, t, noise, dpd, k=0):
    """One training step with the upstream gradient loss * 2^k: ({name: gradient}, prediction), on the CPU."""
    m.zero_grad(set_to_none=True)
    pred = m(x2d, gt, t=t, noise=noise, droppath=dpd)
    loss = torch.mean(torch.norm(pred - gt, dim=-1))
    loss.backward(loss.clone().detach() * 2.0 ** k)
    torch.cuda.synchronize()
    return {n: p.grad.detach().cpu().clone() for n, p in m.pose_estimator.named_parameters()}, pred.detach().cpu()


def gpu_step(monkeypatch, case, ks=(0,)):
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    sd, x2d, gt, t, noise, dpd = problem(case)
    m = model_of(case, sd)
    x2d, gt = x2d.cuda(), gt.cuda()
    return [step(m, x2d, gt, t, noise, dpd, k) for k in ks]


def check(case, grads, pred, tag="", k=0):
    """Every parameter gradient and the prediction within 8 x e32 of the fp64 oracle (x 2^k) in both figures; exact zeros where the
    fp64 gradient is identically zero.  Returns the per-tensor errors."""
    ref = reference(case)
    assert gc.admissible(ref.e32), (case.id, ref.e32)
    assert set(grads) == set(ref.g64), set(grads) ^ set(ref.g64)
    want = {n: g * 2.0 ** k for n, g in ref.g64.items()}
    want[gc.PREDICTION] = ref.pred64
    errs = gc.grad_errors({**grads, gc.PREDICTION: pred}, want)
    print(gc.report(f"training gradients vs fp64, {case.id}{tag}", errs, ref.e32))
    bad = gc.violations(errs, ref.e32)
    assert not bad, "\n".join([f"{case.id}{tag}: outside {gc.FACTOR:g} x e32 = ({gc.FACTOR * ref.e32[0]:.2e}, "
                               f"{gc.FACTOR * ref.e32[1]:.2e})"] + bad)
    return errs


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: c.id)
def test_gradients_elementwise_over_the_dispatch_shapes(monkeypatch, case):
    (grads, pred), = gpu_step(monkeypatch, case)
    check(case, grads, pred)


@pytest.mark.parametrize("case", MAGNITUDES, ids=lambda c: c.id)
def test_gradients_elementwise_when_one_operand_leaves_its_usual_magnitude(monkeypatch, case):
    (grads, pred), = gpu_step(monkeypatch, case)
    check(case, grads, pred)


@pytest.mark.parametrize("case", DROPPED, ids=lambda c: c.id)
def test_a_branch_dropped_for_every_sample_has_exactly_zero_gradients(monkeypatch, case):
    """The backward pass of a dropped branch runs on an all-zero tensor (the amax == 0 branch of dyn_scale / ta_scale): its 12
    parameters get exactly-zero gradients, everything is finite, every other parameter stays within the bound."""
    (grads, pred), = gpu_step(monkeypatch, case)
    errs = check(case, grads, pred)
    assert sorted(n for n, e in errs.items() if e.zero_ref) == sorted(DROPPED_PARAMS)
    for n in DROPPED_PARAMS:
        assert torch.equal(grads[n], torch.zeros_like(grads[n])), n
    assert all(torch.isfinite(g).all() for g in grads.values())


@pytest.mark.parametrize("case", UPSTREAM, ids=lambda c: c.id)
def test_gradients_scale_with_the_upstream_gradient_bit_for_bit(monkeypatch, case):
    """loss.backward(loss * 2^k), k = -40, 0, +30: each run within the bound of the fp64 gradients x 2^k, and -- every device-side
    scale being a power of two derived from an absmax, the backward pass linear in the upstream gradient -- the k != 0 gradients
    x 2^-k equal the k = 0 gradients bit for bit."""
    runs = dict(zip(UPSTREAM_K, gpu_step(monkeypatch, case, UPSTREAM_K)))
    for k, (grads, pred) in runs.items():
        check(case, grads, pred, tag=f" upstream x 2^{k}", k=k)
    base = runs[0][0]
    for k in UPSTREAM_K:
        if k == 0:
            continue
        differ = [n for n, g in runs[k][0].items() if not torch.equal(g * 2.0 ** -k, base[n])]
        assert not differ, (k, differ)
