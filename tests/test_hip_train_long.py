"""D3DP_TRAIN_LONG_ATTN=chunked: the fp32 attention backward of the training step on its chunked kernels (train.hip
attn_bwd_q_chunk_kernel / attn_bwd_kv_chunk_kernel), at any width and clip length (run with ``-m gpu`` on an MI355X).

1. Where the whole-sequence kernels run too, a step with the switch equals a step without it bit for bit: the chunked kernels keep
   the arithmetic and its order, so no tolerance is needed.
2. Beyond the old limits -- more than 256 tokens per sequence, more than 153 at head dims above 64 -- every gradient and the
   prediction lie within oracle/grad_check.py's bound (8 x the fp32 oracle's own error, in the norm and per element) of the oracle's
   fp64 autograd.  Without the switch d3dp_create or d3dp_train_forward refuses every one of these with D3DP_ENOTSUP.
3. The new route is the fp32 cross-check of the split-fp16 training attention at long clips: both within the bound of one reference.
4. Bit-reproducible on one and on two streams; exactly zero gradients for a branch dropped for every sample; gradients scale bit
   for bit with the upstream gradient x 2^-40 and x 2^30.
5. With dqkv and the statistics region of the workspace pre-filled with NaN or with zeros the gradients are the same bits: no row
   beyond a sequence is read as a gradient or written outside its sequence.

The model is MixSTE2 itself (D3DP builds 17 joints; the spatial-axis cases need 150 / 160), dep = 1, the model's 8 heads.  The case
tables are plain data: tests/test_train_long_host.py walks them on a CPU and shows every fp64-checked case admissible."""
import os
import shutil
import subprocess
from functools import lru_cache
from typing import NamedTuple, Tuple

import numpy as np
import pytest
import torch

from d3dp_amd.model import MixSTE2
from d3dp_amd.weights import make_state_dict, synthetic_noise
from oracle import d3dp_oracle as orc
from oracle import grad_check as gc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "D3DP_TRAIN_LONG_ATTN"
_SWITCHES = ("D3DP_TRAIN_ATTN", "D3DP_TRAIN_ATTN_BWD", "D3DP_TRAIN_IMPL", "D3DP_TRAIN_WGRAD", "D3DP_TRAIN_PASSES", "D3DP_TRAIN_OVERLAP",
             SWITCH)
SD_SEED, INPUT_SEED, MASK_SEED = 11, 911, 5
PRE = "pose_estimator."
ATTN_F32 = (("D3DP_TRAIN_ATTN", "f32"),)


class Case(NamedTuple):
    cs: int
    Fr: int
    J: int = 17
    B: int = 1
    dep: int = 1
    env: Tuple[Tuple[str, str], ...] = ()     # switches beside D3DP_TRAIN_LONG_ATTN
    masks: str = "none"                        # "recorded": drawn at the model's rates; "dropped": two branches dropped for every sample

    @property
    def id(self):
        return (f"cs{self.cs}-F{self.Fr}" + (f"-J{self.J}" if self.J != 17 else "") + f"-B{self.B}" + (f"-dep{self.dep}" if self.dep != 1 else "")
                + "".join(f"-{k[5:].lower()}={v}" for k, v in self.env) + (f"-{self.masks}" if self.masks != "none" else ""))

    @property
    def problem(self):
        """The part of a case that fixes its inputs and its reference (the switches do not)."""
        return self._replace(env=())


# 1. both forms run: head dim 8; the run-time head dim at capacities 16 and 128; head dim 64 on the VALU pair; row counts at the edges of
#    a workgroup's 256 rows and of its 512 threads (J = 5 keeps T small); the last spatial count the 153-token limit allows
BOTH = [
    Case(64, 27, B=2),
    Case(96, 40, B=2),
    Case(576, 30, B=2),
    Case(512, 27, B=2, env=ATTN_F32 + (("D3DP_TRAIN_ATTN_BWD", "valu"),)),
    Case(64, 128, J=5, B=2), Case(64, 129, J=5, B=2), Case(64, 255, J=5, B=2), Case(64, 256, J=5, B=2),
    Case(576, 9, J=150),
]
# 2. beyond the old limits, against fp64: one row past a row block and a chunk (257), ragged (300), a second block of 128 rows -- 512
#    threads' worth of pairs, half a chunk -- (384) and one row past it (385); run-time head dims 12, 72 and 128 (two chunks of 128 rows at
#    160 and 243); head dim 64; the spatial axis
BEYOND = [
    Case(64, 257), Case(64, 300), Case(64, 384), Case(64, 385),
    Case(96, 300),
    Case(576, 160),
    Case(1024, 160), Case(1024, 243),
    Case(512, 300, env=ATTN_F32),
    Case(576, 9, J=160),
    Case(96, 300, B=2, dep=2, masks="recorded"),
]
# 3. the product path at long clips (split-fp16 attention, no switch) and its fp32 cross-check (the switch) on one problem
CROSS = [Case(cs, 300) for cs in (512, 256, 128)]
# 4.
REPRO = Case(64, 300)
DROPPED = Case(96, 300, B=2, dep=2, masks="dropped")
DROPPED_PARAMS = ([f"STEblocks.1.{n}" for n in ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight",
                                                "attn.proj.bias")]
                  + [f"TTEblocks.1.{n}" for n in ("norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight",
                                                  "mlp.fc2.bias")])
UPSTREAM = Case(64, 300)
UPSTREAM_K = (-40, 0, 30)
# 5. several sequences share dqkv: B = 2, one row past a row block
PREFILL = Case(64, 257, B=2)
# every case compared with the fp64 oracle: tests/test_train_long_host.py shows each admissible
FP64_CASES = list(dict.fromkeys([c.problem for c in BEYOND + CROSS + [REPRO, DROPPED, UPSTREAM, PREFILL]]))


def problem(case):
    """(state dict, x2d, gt, noise, t, DropPath masks) of one case, all on the CPU."""
    B, Fr, J = case.B, case.Fr, case.J
    sd = make_state_dict(SD_SEED, case.cs, case.dep, Fr, joints=J)
    rng = np.random.Generator(np.random.PCG64(INPUT_SEED))
    x2d = torch.from_numpy(rng.uniform(-1.0, 1.0, size=(B, Fr, J, 2)).astype(np.float32))
    gt = torch.from_numpy(synthetic_noise(INPUT_SEED + 1, (B, Fr, J, 3))) * 0.3
    gt[:, :, 0] = 0
    noise = torch.from_numpy(synthetic_noise(INPUT_SEED + 2, (B, Fr, J, 3)))
    t = torch.tensor([[30], [700]][:B], dtype=torch.long)
    dpd = {}
    if case.masks == "dropped":
        one, zero = (lambda S: torch.ones(S, 1, 1)), (lambda S: torch.zeros(S, 1, 1))
        dpd["STEblocks.1"] = (zero(B * Fr), one(B * Fr))
        dpd["TTEblocks.1"] = (one(B * J), zero(B * J))
    elif case.masks == "recorded":         # the blocks behind the first (timm semantics: 0 or 1 / keep), as test_hip_train_grads draws them
        rates = [x.item() for x in torch.linspace(0, 0.1, case.dep)]
        gen = torch.Generator().manual_seed(MASK_SEED)
        for i in range(1, case.dep):
            keep = 1 - rates[i]
            mk = lambda S: (torch.rand(S, 1, 1, generator=gen) < keep).float() / keep
            dpd[f"STEblocks.{i}"] = (mk(B * Fr), mk(B * Fr))
            dpd[f"TTEblocks.{i}"] = (mk(B * J), mk(B * J))
    return sd, x2d, gt, noise, t, dpd


@lru_cache(maxsize=2)
def reference(prob):
    """The oracle's fp64 and fp32 step of one problem and the e32 they define: computed once, shared, never written to."""
    sd, x2d, gt, noise, t, dpd = problem(prob)
    return gc.reference_pair(sd, x2d, gt, t, noise, prob.dep, dpd or None)


def model_of(case, sd):
    m = MixSTE2(num_frame=case.Fr, num_joints=case.J, embed_dim_ratio=case.cs, depth=case.dep, is_train=True, numerics="train",
                drop_path_rate=0.0)
    m.load_state_dict(orc.strip_prefix(sd), strict=True)
    return m.cuda().train()


def step(m, x2d, x_t, gt, t, dpd, k=0):
    """One training step with the upstream gradient loss * 2^k: ({name: gradient}, prediction), on the CPU."""
    m.zero_grad(set_to_none=True)
    pred = m(x2d, x_t, t, droppath=dpd or None)
    loss = torch.mean(torch.norm(pred - gt, dim=-1))
    loss.backward(loss.clone().detach() * 2.0 ** k)
    torch.cuda.synchronize()
    return {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}, pred.detach().cpu()


class Run(NamedTuple):
    model: MixSTE2
    args: tuple

    def step(self, k=0):
        return step(self.model, *self.args, k)


def start(monkeypatch, case, switch, extra=()):
    """A fresh model for `case` under its switches (+ `extra`), with or without D3DP_TRAIN_LONG_ATTN=chunked.  The context reads them
    when it is created, at the first step -- D3DP_TRAIN_ATTN_BWD at every step -- so they stay set until the test ends."""
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in tuple(case.env) + tuple(extra):
        monkeypatch.setenv(k, v)
    if switch:
        monkeypatch.setenv(SWITCH, "chunked")
    sd, x2d, gt, noise, t, dpd = problem(case.problem)
    x_t = orc.prepare_targets(orc.cosine_schedule(1000), gt, t[:, 0], noise)
    return Run(model_of(case, sd), (x2d.cuda(), x_t.cuda(), gt.cuda(), t[:, 0].cuda(), dpd))


def check(case, grads, pred, tag="", k=0):
    """Every parameter gradient and the prediction within 8 x e32 of the fp64 oracle (x 2^k) in both figures; exact zeros where the
    fp64 gradient is identically zero.  Prints the figures, returns the per-tensor errors."""
    ref = reference(case.problem)
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


def differing(a, b):
    return [n for n in a if not torch.equal(a[n], b[n])]


# ------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("case", BOTH, ids=lambda c: c.id)
def test_chunked_and_whole_sequence_kernels_agree_bit_for_bit(monkeypatch, case):
    whole_g, whole_p = start(monkeypatch, case, False).step()
    run = start(monkeypatch, case, True)
    assert "D3DP_TRAIN_LONG_ATTN=chunked" in run.model.train_arithmetic()
    chunk_g, chunk_p = run.step()
    assert all(torch.isfinite(g).all() for g in chunk_g.values()) and any(g.any() for g in chunk_g.values())
    assert torch.equal(whole_p, chunk_p)
    assert not differing(whole_g, chunk_g), differing(whole_g, chunk_g)


# ------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("case", BEYOND, ids=lambda c: c.id)
def test_gradients_beyond_the_whole_sequence_limits_against_fp64(monkeypatch, case):
    grads, pred = start(monkeypatch, case, True).step()
    check(case, grads, pred)


# ------------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("case", CROSS, ids=lambda c: c.id)
def test_the_chunked_route_cross_checks_the_split_fp16_attention_at_long_clips(monkeypatch, case):
    run = start(monkeypatch, case, False)
    assert "split-fp16 operands" in run.model.train_arithmetic()
    grads, pred = run.step()
    check(case, grads, pred, tag=" split-fp16 attention")
    grads, pred = start(monkeypatch, case._replace(env=ATTN_F32), True).step()
    check(case, grads, pred, tag=" D3DP_TRAIN_ATTN=f32 chunked")


# ------------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("overlap", [None, "0"], ids=["two-streams", "one-stream"])
def test_a_step_beyond_the_limits_is_bit_reproducible(monkeypatch, overlap):
    run = start(monkeypatch, REPRO, True, extra=(("D3DP_TRAIN_OVERLAP", overlap),) if overlap else ())
    g1, p1 = run.step()
    g2, p2 = run.step()
    check(REPRO, g1, p1, tag=f" D3DP_TRAIN_OVERLAP={overlap}")
    assert torch.equal(p1, p2) and not differing(g1, g2), differing(g1, g2)


def test_a_dropped_branch_has_exactly_zero_gradients_beyond_the_limits(monkeypatch):
    grads, pred = start(monkeypatch, DROPPED, True).step()
    errs = check(DROPPED, grads, pred)
    assert sorted(n for n, e in errs.items() if e.zero_ref) == sorted(DROPPED_PARAMS)
    for n in DROPPED_PARAMS:
        assert torch.equal(grads[n], torch.zeros_like(grads[n])), n
    assert all(torch.isfinite(g).all() for g in grads.values())


def test_gradients_beyond_the_limits_scale_with_the_upstream_gradient_bit_for_bit(monkeypatch):
    run = start(monkeypatch, UPSTREAM, True)
    runs = {k: run.step(k) for k in UPSTREAM_K}
    for k, (grads, pred) in runs.items():
        check(UPSTREAM, grads, pred, tag=f" upstream x 2^{k}", k=k)
    base = runs[0][0]
    for k in UPSTREAM_K:
        differ = [n for n, g in runs[k][0].items() if not torch.equal(g * 2.0 ** -k, base[n])]
        assert not differ, (k, differ)


# ------------------------------------------------------------------------------------------------------------------- 5
def workspace_regions(case, tmp_path):
    """[(first float, floats)] of dqkv and of the attention statistics in the step's workspace: TrainLayout's own figures, through the
    stand-alone driver of train_plan.h (tests/train_plan_driver.cpp)."""
    assert shutil.which("g++") is not None, "g++ compiles tests/train_plan_driver.cpp"
    exe = str(tmp_path / "train_plan_driver")
    subprocess.run(["g++", "-std=c++17", os.path.join(ROOT, "tests", "train_plan_driver.cpp"), "-o", exe], check=True)
    line = "\t".join(str(v) for v in (case.cs, 8, 2 * case.cs, case.Fr, case.J, case.dep, case.B, 256, 0))
    out = subprocess.run([exe], input=line + "\n", capture_output=True, text=True, check=True).stdout.rstrip("\n").split("\t")
    assert out[0] == "0", out[:2]
    L = {k: int(v) for k, v in (f.split("=") for f in out[2:])}
    nmax = max(case.Fr, case.J)
    stats = case.B * nmax * 8 * nmax * 3 + 64            # d3dp_train_attn_stats_bytes(B max(F, J), max(F, J), heads) / 4 + 64
    assert L["L_stats"] + stats <= L["L_op_a"] and L["L_dqkv"] + 3 * L["L_unit"] <= L["L_dh"]
    return [(L["L_dqkv"], 3 * L["L_unit"]), (L["L_stats"], stats)], L["L_total_floats"]


def test_rows_beyond_a_sequence_are_neither_read_nor_stored(monkeypatch, tmp_path):
    regions, total = workspace_regions(PREFILL, tmp_path)
    run = start(monkeypatch, PREFILL, True)
    g0, p0 = run.step()                                   # (allocates the workspace)
    check(PREFILL, g0, p0)
    ws = run.model._state().train_ws.view(torch.float32)
    assert ws.numel() >= total
    got = {}
    for name, fill in (("nan", float("nan")), ("zero", 0.0)):
        for first, count in regions:
            ws[first:first + count] = fill
        torch.cuda.synchronize()
        got[name] = run.step()
    for name, (g, p) in got.items():
        assert all(torch.isfinite(v).all() for v in g.values()), name
        assert torch.equal(p, p0) and not differing(g, g0), (name, differing(g, g0))
