"""The training step's attention on the fp16 matrix cores at head dims 32 and 16 (`-cs 256` / `-cs 128` with the model's 8 heads): the
split-fp16 kernels of train_attn.hip with the head dim as a template parameter, driven through the public training step
(run with ``-m gpu`` on an MI355X).  All shapes: J = 17, dep = 2, and the smallest clip lengths that reach each dispatch case:
  n <= 32 tokens (17 joints, 9 frames)  the one-kernel backward (tattn_bwd_small_kernel);
  40 / 81 / 243 frames                  4 / 8 / 16 key tiles; 243 runs two groups of eight waves per problem and ragged last tiles;
  300 / 513 frames                      the chunked forms of all three kernels, pass KV's query chunks included.
The one-kernel backward and the two-kernel backward cannot both be reached for one shape through the public step (the dispatch
takes the one-kernel form at n <= 32 and nothing forces the other), so their bit equality is not asserted here: the one-kernel
form is covered through the cross-check and the autograd comparisons below only (9 frames, and the 17 joints of every case).

Bounds: those of the head-dim-64 tests of the same comparisons (tests/test_hip_parity.py
test_attention_backward_on_matrix_cores_matches_the_valu_kernels, test_training_step_config5_vs_oracle_autograd)."""
from types import SimpleNamespace

import pytest
import torch

from d3dp_amd import D3DP, _lib
from d3dp_amd.weights import H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, make_state_dict, synthetic_inputs_2d, synthetic_noise
from oracle import d3dp_oracle as orc

pytestmark = pytest.mark.gpu
EXACT_TOL_MM = 1e-3
DEP = 2
_SWITCHES = ("D3DP_TRAIN_ATTN", "D3DP_TRAIN_ATTN_BWD", "D3DP_TRAIN_IMPL")


def clear_switches(monkeypatch):
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)


def train_model(Fr, cs, seed, dep=DEP):
    """(the environment switches are read when the context is created, at the first step: one model per setting)"""
    args = SimpleNamespace(number_of_frames=Fr, test_time_augmentation=True, timestep=1000, scale=1.0, cs=cs, dep=dep)
    sd = make_state_dict(seed, cs, dep, Fr)
    m = D3DP(args, H36M_JOINTS_LEFT, H36M_JOINTS_RIGHT, is_train=True)
    m.load_state_dict(sd, strict=False)
    return m.cuda().train(), sd


def inputs(B, Fr, seed):
    x2d = torch.from_numpy(synthetic_inputs_2d(seed, B, Fr))
    gt = torch.from_numpy(synthetic_noise(seed + 1, (B, Fr, 17, 3))) * 0.3
    gt[:, :, 0] = 0
    noise = torch.from_numpy(synthetic_noise(seed + 2, (B, Fr, 17, 3)))
    t = torch.tensor([[30], [700]][:B], dtype=torch.long)
    return x2d, gt, t, noise


def droppath_masks(B, Fr, dep, seed):
    """Recorded DropPath masks of the blocks behind the first (timm semantics: 0 or 1 / keep), as the config-5 test draws them."""
    rates = [x.item() for x in torch.linspace(0, 0.1, dep)]
    gen = torch.Generator().manual_seed(seed)
    dpd = {}
    for i in range(1, dep):
        keep = 1 - rates[i]
        mk = lambda S: (torch.rand(S, 1, 1, generator=gen) < keep).float() / keep
        dpd[f"STEblocks.{i}"] = (mk(B * Fr), mk(B * Fr))
        dpd[f"TTEblocks.{i}"] = (mk(B * 17), mk(B * 17))
    return dpd


def step(m, x2d, gt, t, noise, dpd):
    m.zero_grad(set_to_none=True)
    pred = m(x2d, gt, t=t, noise=noise, droppath=dpd)
    loss = torch.mean(torch.norm(pred - gt, dim=-1))
    loss.backward(loss.clone().detach())
    return pred, loss


@pytest.mark.parametrize("Fr", [9, 40, 81, 243])
@pytest.mark.parametrize("cs", [256, 128])
def test_small_head_attention_matches_the_cross_check_kernels(monkeypatch, cs, Fr):
    """valu / mfma (D3DP_TRAIN_ATTN=f32: what this width ran before) / x2t / default: every parameter gradient within 2e-5 relative
    of the VALU run, the prediction within 2e-5 absolute, and some gradient bit differs (the switch selected another kernel)."""
    B = 2
    sd_seed = 11
    x2d, gt, t, noise = inputs(B, Fr, 911)
    x2d, gt = x2d.cuda(), gt.cuda()
    grads, preds = {}, {}
    for impl in ("valu", "mfma", "x2t", "x2"):
        clear_switches(monkeypatch)
        if impl == "x2t":
            monkeypatch.setenv("D3DP_TRAIN_ATTN", "x2t")
        elif impl != "x2":
            monkeypatch.setenv("D3DP_TRAIN_ATTN", "f32")
            monkeypatch.setenv("D3DP_TRAIN_ATTN_BWD", impl)
        m, _ = train_model(Fr, cs, sd_seed)
        pred, _ = step(m, x2d, gt, t, noise, {})
        torch.cuda.synchronize()
        preds[impl] = pred.detach().double().cpu()
        grads[impl] = {k: p.grad.double().cpu() for k, p in m.pose_estimator.named_parameters()}
        assert all(torch.isfinite(g).all() for g in grads[impl].values()), impl
    for impl in ("mfma", "x2t", "x2"):
        worst = max((grads["valu"][k] - grads[impl][k]).norm().item() / max(grads["valu"][k].norm().item(), 1e-30) for k in grads["valu"])
        dp = (preds[impl] - preds["valu"]).abs().max().item()
        print(f"training attention, cs={cs} F={Fr}: {impl} vs VALU kernels, worst relative gradient difference {worst:.2e}, "
              f"prediction max |diff| {dp:.2e}")
        for k in grads["valu"]:
            err = (grads["valu"][k] - grads[impl][k]).norm().item() / max(grads["valu"][k].norm().item(), 1e-30)
            assert err < 2e-5, (impl, k, err)
        assert dp < 2e-5, (impl, dp)
    assert any(not torch.equal(grads["valu"][k], grads["x2"][k]) for k in grads["valu"])   # (the default is another kernel)


def against_autograd(cs, Fr, B, tag):
    m, sd = train_model(Fr, cs, 7)
    x2d, gt, t, noise = inputs(B, Fr, 901)
    dpd = droppath_masks(B, Fr, DEP, 5)
    pred, loss = step(m, x2d.cuda(), gt.cuda(), t, noise, dpd)
    torch.cuda.synchronize()
    po = {k: v.clone().requires_grad_(True) for k, v in orc.strip_prefix(sd).items()}
    xp = orc.prepare_targets(orc.cosine_schedule(1000), gt, t[:, 0], noise)
    pred_o = orc.mixste_forward(po, x2d, xp, t[:, 0], DEP, droppath=dpd)
    loss_o = torch.mean(torch.norm(pred_o - gt, dim=-1))
    loss_o.backward(loss_o.clone().detach())
    errs = {}
    for name, p in m.pose_estimator.named_parameters():
        ref = po[name].grad.double()
        errs[name] = (p.grad.cpu().double() - ref).norm().item() / max(ref.norm().item(), 1e-12)
    worst = max(errs, key=errs.get)
    mm = orc.mpjpe_mm(pred.detach().cpu(), pred_o.detach())
    print(f"{tag} cs={cs} F={Fr}: prediction {mm:.2e} mm, |loss diff| {abs(loss.item() - loss_o.item()):.2e}, worst relative gradient "
          f"error over {len(errs)} parameters {errs[worst]:.2e} ({worst})")
    assert mm <= EXACT_TOL_MM
    assert abs(loss.item() - loss_o.item()) < 2e-6
    for name, err in errs.items():
        assert err < 5e-3, (name, err)


@pytest.mark.parametrize("Fr", [27, 243])
@pytest.mark.parametrize("cs", [256, 128])
def test_small_head_training_step_vs_oracle_autograd(monkeypatch, cs, Fr):
    """Prediction, loss and EVERY parameter gradient against torch autograd through the CPU oracle, recorded DropPath masks included
    (the head-dim-64 figure of the same comparison at full size: 2.1e-6)."""
    clear_switches(monkeypatch)
    against_autograd(cs, Fr, 2, "training step vs autograd,")


@pytest.mark.parametrize("Fr", [300, 513])
@pytest.mark.parametrize("cs", [256, 128])
def test_small_head_training_step_on_a_clip_longer_than_256_frames(monkeypatch, cs, Fr):
    """The chunked forms of all three kernels (keys through LDS in chunks of 128; pass KV's queries too): these contexts were refused
    with D3DP_ENOTSUP while the widths ran the fp32 attention."""
    clear_switches(monkeypatch)
    against_autograd(cs, Fr, 1, "long clip,")


@pytest.mark.parametrize("cs,switch", [(256, "D3DP_TRAIN_ATTN"), (128, "D3DP_TRAIN_ATTN"), (64, None)])
def test_fp32_attention_still_refuses_more_than_256_frames(monkeypatch, cs, switch):
    """The fp32 attention holds a whole sequence in LDS: under the cross-check switch, and at head dim 8, 300 frames are refused -- and
    the message names the switch."""
    clear_switches(monkeypatch)
    if switch:
        monkeypatch.setenv(switch, "f32")
    Fr, B = 300, 1
    m, _ = train_model(Fr, cs, 7)
    x2d, gt, t, noise = inputs(B, Fr, 901)
    with pytest.raises(_lib.D3DPHipError) as e:
        m(x2d.cuda(), gt.cuda(), t=t, noise=noise, droppath={})
    assert "frames=300 > 256" in str(e.value) and "D3DP_TRAIN_ATTN=f32" in str(e.value), str(e.value)


def profiled_step(monkeypatch, attn):
    clear_switches(monkeypatch)
    if attn:
        monkeypatch.setenv("D3DP_TRAIN_ATTN", attn)
    Fr, B = 40, 2
    m, _ = train_model(Fr, 256, 7)
    x2d, gt, t, noise = inputs(B, Fr, 901)
    pe = m.pose_estimator
    pe._context(torch.device("cuda", torch.cuda.current_device()))
    pe.profile_enable(True)
    step(m, x2d.cuda(), gt.cuda(), t, noise, {})
    torch.cuda.synchronize()
    prof = pe.profile_read()
    pe.profile_enable(False)
    return prof


def test_the_route_is_observable_in_the_profile(monkeypatch):
    """Pass KV is timed as a class of its own only on the split-fp16 route (the fp32 path times both passes under the pass-Q class), and
    the forward writes proj's operand rows there, so the step counts fewer operand passes than under D3DP_TRAIN_ATTN=f32."""
    x2 = profiled_step(monkeypatch, None)
    f32 = profiled_step(monkeypatch, "f32")
    assert x2["train_attn_bwd_kv_temporal"][0] > 0 and x2["train_attn_bwd_q_temporal"][0] > 0, x2
    assert f32["train_attn_bwd_kv_temporal"][0] == 0, f32
    assert x2["train_operand_pass"][0] < f32["train_operand_pass"][0], (x2["train_operand_pass"], f32["train_operand_pass"])


def test_small_head_training_step_is_bit_reproducible(monkeypatch):
    clear_switches(monkeypatch)
    Fr, B = 81, 2
    m, _ = train_model(Fr, 256, 3)
    x2d, gt, t, noise = inputs(B, Fr, 21)
    x2d, gt = x2d.cuda(), gt.cuda()
    dpd = droppath_masks(B, Fr, DEP, 1)
    runs = []
    for _ in range(2):
        pred, _ = step(m, x2d, gt, t, noise, dpd)
        torch.cuda.synchronize()
        runs.append((pred.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0])
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n
    assert all(torch.isfinite(g).all() for g in runs[0][1].values()) and any(g.abs().max() > 0 for g in runs[0][1].values())


def test_small_head_training_step_on_a_side_stream(monkeypatch):
    """Stream contract: one step issued under torch.cuda.stream(s), after one eager step, gives the default-stream gradients bit for
    bit (cs = 128: no proj operand rows from the forward, the absmax of the attention output through the block reduction)."""
    clear_switches(monkeypatch)
    Fr, B = 27, 2
    m, _ = train_model(Fr, 128, 3)
    x2d, gt, t, noise = inputs(B, Fr, 31)
    x2d, gt = x2d.cuda(), gt.cuda()
    step(m, x2d, gt, t, noise, {})
    torch.cuda.synchronize()
    want = {n: p.grad.clone() for n, p in m.named_parameters()}
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        step(m, x2d, gt, t, noise, {})
    s.synchronize()
    for n, p in m.named_parameters():
        assert torch.equal(want[n], p.grad), n
    assert any(g.abs().max() > 0 for g in want.values())
