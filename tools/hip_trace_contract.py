"""The program tests/test_hip_streams.py::test_traced_step_makes_no_forbidden_hip_call runs under `rocprofv3 --hip-trace`:
one warmed EXACT sampler step (d3dp_ddim_pre, d3dp_denoise, d3dp_ddim_post) and one warmed training step (d3dp_train_forward,
d3dp_train_backward) at small shapes on a side stream, every tensor pre-allocated or served from the warmed allocator, so that
between the brackets only the library's calls reach the HIP runtime.

A bracket opens with THREE torch.cuda.synchronize() in a row (no other place of a torch program does that) and closes with one:
the test reads the HIP API rows in between.  Nothing else belongs in the same profiler run (no counters, no other tracing mode).

usage: rocprofv3 --hip-trace --output-format csv -d OUT -- python tools/hip_trace_contract.py"""
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from d3dp_amd import D3DP, _lib  # noqa: E402
from d3dp_amd.weights import (H36M_JOINTS_LEFT as KL, H36M_JOINTS_RIGHT as KR, flip_2d, make_state_dict,  # noqa: E402
                              synthetic_inputs_2d, synthetic_noise)

Fr, B, H, cs, dep = 27, 2, 2, 512, 2
WARM = 3


def model(is_train):
    args = SimpleNamespace(number_of_frames=Fr, test_time_augmentation=True, timestep=1000, scale=1.0, cs=cs, dep=dep)
    m = D3DP(args, KL, KR, is_train=is_train, num_proposals=H, sampling_timesteps=1, numerics=None if is_train else "exact")
    m.load_state_dict(make_state_dict(7, cs, dep, Fr), strict=False)
    return (m.cuda().train() if is_train else m.cuda().eval())


def bracket(fn, s):
    for _ in range(3):
        torch.cuda.synchronize()
    with torch.cuda.stream(s):
        fn()
    torch.cuda.synchronize()


def main():
    lib = _lib.load()
    s = torch.cuda.Stream()
    x2d = synthetic_inputs_2d(11, B, Fr)
    x2 = torch.cat((torch.from_numpy(x2d), torch.from_numpy(flip_2d(x2d)))).cuda().contiguous()
    img = torch.from_numpy(synthetic_noise(12, (B, H, Fr, 17, 3))).cuda()
    nz = torch.from_numpy(synthetic_noise(13, (B, H, Fr, 17, 3))).cuda()
    xt2, pred2 = torch.empty((2 * B, H, Fr, 17, 3), device="cuda"), torch.empty((2 * B, H, Fr, 17, 3), device="cuda")
    xs, nxt = torch.empty_like(img), torch.empty_like(img)
    t2 = torch.full((2 * B,), 999, dtype=torch.long, device="cuda")
    ev = model(False)
    perm, pe = ev._perm(img.device), ev.pose_estimator

    def sampler_step():
        st = _lib.current_stream()
        _lib.check(lib.d3dp_ddim_pre(img.data_ptr(), xt2.data_ptr(), perm.data_ptr(), 1.0, B, H, Fr, 17, st), "d3dp_ddim_pre")
        pe.denoise(x2, xt2, t2, out=pred2)
        _lib.check(lib.d3dp_ddim_post(pred2.data_ptr(), img.data_ptr(), nz.data_ptr(), perm.data_ptr(), 1.0, 1.7, 1.3, 0.8, 0.5, 0.3, 0,
                                      xs.data_ptr(), xs[0].numel(), nxt.data_ptr(), B, H, Fr, 17, st), "d3dp_ddim_post")

    tr = model(True)
    tp = tr.pose_estimator
    x3 = (torch.from_numpy(synthetic_noise(14, (B, Fr, 17, 3))) * 0.3).cuda()
    tt = torch.tensor([40, 900], dtype=torch.long).cuda()
    gout = torch.from_numpy(synthetic_noise(15, (B, Fr, 17, 3))).cuda()
    x2t = x2[:B].contiguous()
    masks = tp._droppath_masks(B, img.device)          # (train mode: random DropPath scales, drawn once)
    keep = {}

    def train_step():
        keep["pred"] = tp._train_forward(x2t, x3, tt, masks)
        keep["grads"] = tp._train_backward(x2t, x3, tt, masks, gout)

    with torch.cuda.stream(s):
        for _ in range(WARM):
            sampler_step()
            train_step()
    torch.cuda.synchronize()
    bracket(sampler_step, s)
    bracket(train_step, s)
    assert torch.isfinite(xs).all() and torch.isfinite(keep["pred"]).all() and all(torch.isfinite(g).all() for g in keep["grads"])
    print(f"hip_trace_contract: sampler step and training step done on stream {s.cuda_stream:#x} (null stream 0x0)")


if __name__ == "__main__":
    main()
