#!/usr/bin/env python3
"""What one build of the library computes on a table of tiny contexts, as text: per entry the two workspace sizes, the sha256
of the d3dp_denoise output or of every gradient of one training step, and for a training step the launches per profile class of one
more, profiled, step (d3dp_profile_read).  The library is bit-deterministic, so two builds that
compute the same thing print the same lines: `D3DP_LIB=a.so python tools/lib_ab_hash.py > a.txt`, the same for b.so, `diff`.
An entry with environment switches runs in a fresh child process (`--only NAME`: that entry alone, in this process; the form
to put behind `rocprofv3 --kernel-trace --stats --`): d3dp_create reads the switches once.  `--match TEXT`: the entries whose
name contains TEXT.

RawCtx, a context over seeded random weights straight on the C ABI, at any (C, F, J), also serves tests/test_hip_workspace.py."""
import ctypes as C
import hashlib
import math
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from d3dp_amd import _lib  # noqa: E402

MODES = {"exact": _lib.MODE_EXACT, "fast": _lib.MODE_FAST, "fast16": _lib.MODE_FAST16, "train": _lib.MODE_TRAIN}


class RawCtx:
    """heads = 8, hidden = 2 C; weights and inputs from torch.Generator(seed) on the host, so every build sees the same bits."""

    def __init__(self, mode, cs, frames, joints, depth, chunk_seqs=0, seed=5):
        self.lib, self.mode, self.C, self.F, self.J, self.depth = _lib.load(), mode, cs, frames, joints, depth
        self.gen = torch.Generator().manual_seed(seed)
        Hd, half = 2 * cs, cs // 2
        mat = lambda n, k: self.rand(n, k, scale=k ** -0.5)
        gamma = lambda: 1.0 + self.rand(cs, scale=0.1)
        block = lambda: [gamma(), self.rand(cs, scale=0.1), mat(3 * cs, cs), self.rand(3 * cs, scale=0.1), mat(cs, cs),
                         self.rand(cs, scale=0.1), gamma(), self.rand(cs, scale=0.1), mat(Hd, cs), self.rand(Hd, scale=0.1),
                         mat(cs, Hd), self.rand(cs, scale=0.1)]
        freq = torch.exp(torch.arange(half) * -(math.log(10000) / (half - 1))).float().cuda()
        self.top = [self.rand(joints, cs, scale=0.02), self.rand(frames, cs, scale=0.02), mat(cs, 5), self.rand(cs, scale=0.1), freq,
                    mat(2 * cs, cs), self.rand(2 * cs, scale=0.1), mat(cs, 2 * cs), self.rand(cs, scale=0.1), gamma(),
                    self.rand(cs, scale=0.1), gamma(), self.rand(cs, scale=0.1), gamma(), self.rand(cs, scale=0.1), mat(3, cs),
                    self.rand(3, scale=0.1)]
        self.ste, self.tte = [block() for _ in range(depth)], [block() for _ in range(depth)]
        cfg = _lib.Cfg(frames, joints, cs, depth, 8, Hd, 1e-6, 1e-5, MODES[mode], chunk_seqs)
        self.ctx = C.c_void_p()
        _lib.check(self.lib.d3dp_create(C.byref(cfg), C.byref(self.ctx)), "d3dp_create")
        w = self.struct(self.top, self.ste, self.tte)
        if mode == "train":
            _lib.check(self.lib.d3dp_set_weights_borrowed(self.ctx, C.byref(w)), "d3dp_set_weights_borrowed")
        else:
            _lib.check(self.lib.d3dp_set_weights(self.ctx, C.byref(w), _lib.current_stream()), "d3dp_set_weights")

    def __del__(self):
        if getattr(self, "ctx", None):
            torch.cuda.synchronize()
            self.lib.d3dp_destroy(self.ctx)

    def rand(self, *shape, scale=1.0):
        return (torch.randn(*shape, generator=self.gen) * scale).cuda().contiguous()

    def struct(self, top, ste, tte):
        arr = lambda blocks: (_lib.BlockWeights * len(blocks))(*[_lib.BlockWeights(*[t.data_ptr() for t in b]) for b in blocks])
        self._keep = (arr(ste), arr(tte))
        return _lib.Weights(*[t.data_ptr() for t in top], *self._keep)

    def infer_bytes(self, B, H):
        n = C.c_size_t()
        _lib.check(self.lib.d3dp_workspace_bytes(self.ctx, B, H, C.byref(n)), "d3dp_workspace_bytes")
        return n.value

    def train_bytes(self, B):
        n = C.c_size_t()
        _lib.check(self.lib.d3dp_train_workspace_bytes(self.ctx, B, C.byref(n)), "d3dp_train_workspace_bytes")
        return n.value

    def infer_inputs(self, B, H):
        return (self.rand(B, self.F, self.J, 2), self.rand(B, H, self.F, self.J, 3),
                torch.tensor([(999 - 500 * b) % 1000 for b in range(B)], dtype=torch.int64, device="cuda"))

    def denoise(self, inputs, out, B, H, ws_ptr, ws_bytes):
        """The call's return code: `out` [B, H, F, J, 3] is written through the workspace at ws_ptr."""
        x2d, xt, t = inputs
        return self.lib.d3dp_denoise(self.ctx, x2d.data_ptr(), xt.data_ptr(), t.data_ptr(), out.data_ptr(), B, H, ws_ptr, ws_bytes,
                                     _lib.current_stream())

    def train_inputs(self, B):
        shape = (B, self.F, self.J)
        return (self.rand(*shape, 2), self.rand(*shape, 3), torch.tensor([(999 - 500 * b) % 1000 for b in range(B)],
                                                                         dtype=torch.int64, device="cuda"), self.rand(*shape, 3))

    def grad_buffers(self, fill=0.0):
        like = lambda ts: [torch.full_like(t, fill) for t in ts]
        return like(self.top), [like(b) for b in self.ste], [like(b) for b in self.tte]

    def train_forward(self, inputs, out, B, ws_ptr, ws_bytes):
        x2d, x3d, t, _ = inputs
        return self.lib.d3dp_train_forward(self.ctx, x2d.data_ptr(), x3d.data_ptr(), t.data_ptr(), None, out.data_ptr(), B, ws_ptr,
                                           ws_bytes, _lib.current_stream())

    def train_backward(self, inputs, grads, B, ws_ptr, ws_bytes):
        x2d, x3d, t, gout = inputs
        g = self.struct(*grads)
        return self.lib.d3dp_train_backward(self.ctx, x2d.data_ptr(), x3d.data_ptr(), t.data_ptr(), None, gout.data_ptr(),
                                            C.byref(g), B, ws_ptr, ws_bytes, _lib.current_stream())

    @staticmethod
    def flat_grads(grads):
        """Every gradient tensor but time_freq's (never written), in the order of the C structs."""
        top, ste, tte = grads
        return [t for i, t in enumerate(top) if i != 4] + [t for b in ste + tte for t in b]


# name: (mode, C, F, J, depth, B, H, chunk_seqs, environment)
INFER = dict(F=9, J=5, depth=2, B=1, H=2, chunk=0, env={})
TABLE = {}
for name, mode, cs, extra in [("exact_c512", "exact", 512, {}), ("exact_c128", "exact", 128, {}), ("exact_c64", "exact", 64, {}),
                              ("exact_c96", "exact", 96, {}), ("fast_c512", "fast", 512, {}), ("fast16_c256", "fast16", 256, {}),
                              ("exact_c512_chunk2", "exact", 512, dict(chunk=2, H=5)),
                              ("exact_c512_fold_ln", "exact", 512, dict(env={"D3DP_FOLD_LN": "1"}))]:
    TABLE[name] = dict(INFER, mode=mode, C=cs, **extra)
for cs in (64, 256, 512):
    TABLE[f"train_c{cs}"] = dict(mode="train", C=cs, F=9, J=5, depth=1, B=2, H=1, chunk=0, env={})
for mode in ("exact", "fast"):
    for cs in (512, 128):                                    # head dims 64 and 16: the long (F > 256) and wide (J > 32) routes
        TABLE[f"{mode}_c{cs}_long_wide"] = dict(mode=mode, C=cs, F=257, J=33, depth=1, B=1, H=1, chunk=0, env={})
        TABLE[f"{mode}_c{cs}_long_wide_rows"] = dict(TABLE[f"{mode}_c{cs}_long_wide"], env={"D3DP_LONG_ATTN": "rows"})
for key, val in [("D3DP_EXACT_IMPL", "bf16x3"), ("D3DP_EXACT_IMPL", "f32"), ("D3DP_NO_FOLD", "1"), ("D3DP_DEFER_NORM", "0")]:
    TABLE[f"exact_c512_{key[5:].lower()}_{val}"] = dict(TABLE["exact_c512"], env={key: val})
for key, val in [("D3DP_TRAIN_IMPL", "f32"), ("D3DP_TRAIN_ATTN", "f32"), ("D3DP_TRAIN_ATTN", "x2t"), ("D3DP_TRAIN_OVERLAP", "0")]:
    TABLE[f"train_c512_{key[5:].lower()}_{val}"] = dict(TABLE["train_c512"], env={key: val})
# the smallest training shapes that reach each branch of the step's plan (csrc/train_plan.h)
TABLE["train_c128"] = dict(TABLE["train_c64"], C=128)                    # transposed-operand weight gradients (fc1 alone is TN)
TABLE["train_c96"] = dict(TABLE["train_c64"], C=96)                      # the fp32 path at a run-time width
TABLE["train_c384_f16x2"] = dict(TABLE["train_c64"], C=384, env={"D3DP_TRAIN_IMPL": "f16x2"})   # the mixed case: fc1 alone is TN
TABLE["train_c256_dep9"] = dict(TABLE["train_c256"], depth=9)            # more than 64 Linears: every weight prepared where it is used
TABLE["train_c512_tail"] = dict(TABLE["train_c512"], F=159, J=17)        # T = 21 x 256 + 30: qkv's remainder rows as 16 x 64 blocks
for key, val in [("D3DP_TRAIN_TAIL", "split"), ("D3DP_TRAIN_WGRAD", "each"), ("D3DP_TRAIN_GELU", "pass"), ("D3DP_TRAIN_LN_OPERAND", "pass")]:
    TABLE[f"train_c512_tail_{key[11:].lower()}_{val}"] = dict(TABLE["train_c512_tail"], env={key: val}, variants=True)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def run(name):
    e = TABLE[name]
    if ("D3DP_FOLD_LN" in e["env"] or e.get("variants")) and _lib.load().d3dp_debug_x2_variants() != 1:
        print(f"{name}: needs the variants build")
        return
    c = RawCtx(e["mode"], e["C"], e["F"], e["J"], e["depth"], e["chunk"])
    B, H = e["B"], e["H"]
    line = f"{name}: workspace {c.infer_bytes(B, H)} train_workspace {c.train_bytes(B)}"
    if e["mode"] == "train":
        n = c.train_bytes(B)
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        out, grads = torch.empty(B, e["F"], e["J"], 3, device="cuda"), c.grad_buffers()
        inputs = c.train_inputs(B)
        rcs = c.train_forward(inputs, out, B, ws.data_ptr(), n), c.train_backward(inputs, grads, B, ws.data_ptr(), n)
        assert rcs == (0, 0), (rcs, c.lib.d3dp_last_error())
        torch.cuda.synchronize()
        line += f" out {sha(out)} grads " + " ".join(sha(g) for g in c.flat_grads(grads))
        counts, ms = (C.c_int64 * _lib.PROFILE_CLASSES)(), (C.c_double * _lib.PROFILE_CLASSES)()
        _lib.check(c.lib.d3dp_profile_enable(c.ctx, 1), "d3dp_profile_enable")
        rcs = c.train_forward(inputs, out, B, ws.data_ptr(), n), c.train_backward(inputs, grads, B, ws.data_ptr(), n)
        assert rcs == (0, 0), (rcs, c.lib.d3dp_last_error())
        _lib.check(c.lib.d3dp_profile_read(c.ctx, counts, ms), "d3dp_profile_read")
        _lib.check(c.lib.d3dp_profile_enable(c.ctx, 0), "d3dp_profile_enable")
        line += " launches " + ",".join(str(k) for k in counts)
    else:
        n = c.infer_bytes(B, H)
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        out = torch.empty(B, H, e["F"], e["J"], 3, device="cuda")
        rc = c.denoise(c.infer_inputs(B, H), out, B, H, ws.data_ptr(), n)
        assert rc == 0, (rc, c.lib.d3dp_last_error())
        torch.cuda.synchronize()
        line += f" out {sha(out)}"
    print(line, flush=True)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--only":
        return run(sys.argv[2])
    match = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--match" else ""
    for name, e in TABLE.items():
        if match not in name:
            continue
        if e["env"]:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--only", name], env=dict(os.environ, **e["env"]), check=True,
                           timeout=300)
        else:
            run(name)


if __name__ == "__main__":
    main()
