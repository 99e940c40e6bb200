"""No GPU and no library needed: what a training step decides before it launches anything -- train_layout() and plan_train_step() of
d3dp_amd/csrc/train_plan.h, pure arithmetic on a d3dp_cfg, the context's switches, the batch size and the CU count -- checked
through a stand-alone driver (tests/train_plan_driver.cpp).  The pins below were worked by hand from the rules d3dp_train_forward /
d3dp_train_backward held inline before the plan existed; the sweep checks what must hold at every shape."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXXFLAGS = ["-std=c++17", "-Wall", "-Werror"]
ROWS, ROWS_T, LN_INPUT, PRODUCER = 0, 1, 2, 3                          # TrainOperand
WHOLE, BLOCKS, SPLIT = 0, 1, 2                                         # TrainTailForm
LINEARS = ("qkv", "proj", "fc1", "fc2")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("train_plan") / "driver")
    subprocess.run(["g++", *CXXFLAGS, os.path.join(ROOT, "tests", "train_plan_driver.cpp"), "-o", exe], check=True)
    return exe


def case(cs, hidden=None, heads=8, frames=9, joints=5, depth=1, B=2, n_cu=256, variants=0, **env):
    fields = [cs, heads, 2 * cs if hidden is None else hidden, frames, joints, depth, B, n_cu, variants]
    return "\t".join([str(f) for f in fields] + [f"D3DP_{k}={v}" for k, v in env.items()])


def plans(driver, *cases):
    """-> [{field: value}] of the accepted cases (None for a refused one), from one run of the driver."""
    clean = {k: v for k, v in os.environ.items() if not k.startswith("D3DP_")}
    out = subprocess.run([driver], input="".join(c + "\n" for c in cases), env=clean, capture_output=True, text=True, check=True).stdout
    rows = [line.split("\t") for line in out.split("\n")[:-1]]
    assert len(rows) == len(cases), out
    return [{k: int(v) for k, v in (f.split("=") for f in r[2:])} if int(r[0]) == 0 else None for r in rows]


def plan(driver, *a, **kw):
    (p,) = plans(driver, case(*a, **kw))
    assert p is not None, (a, kw)
    assert p["path_agrees"] == 1                                        # plan_train_path() alone says what the plan's path part says
    return p


def per_linear(p, field):
    return tuple(p[f"{n}_{field}"] for n in LINEARS)


def flags(p):
    return {k: p[k] for k in ("ln_fused", "ln_direct", "att_direct_s", "att_direct_t", "gelu_operand", "gip", "mip1", "mip2", "merged")}


ALL_ON = dict(ln_fused=1, ln_direct=1, att_direct_s=1, att_direct_t=1, gelu_operand=1, gip=1, mip1=1, mip2=1, merged=1)
ALL_OFF = {k: 0 for k in ALL_ON}
CONFIGS4 = dict(hidden=1024, depth=8, B=4, frames=243, joints=17)      # T = 16,524 = 64 x 256 + 140


# ---------------------------------------------------------------------------------------------- pins worked by hand
def test_configs4(driver):
    p = plan(driver, 512, **CONFIGS4)
    assert (p["use_x2"], p["attn_x2_s"], p["attn_x2_t"], p["needs_aux"], p["passes"], p["overlap_sets"]) == (1, 1, 1, 1, 3, 2)
    assert p["T"] == 16524 and p["L_Tp_max"] == 18592
    assert per_linear(p, "N") == (1536, 512, 1024, 512) and per_linear(p, "K") == (512, 512, 512, 1024)
    assert per_linear(p, "tn") == (1, 1, 1, 1)
    assert (p["merged"], p["mZ"], p["mTp"]) == (1, 4, 16640)            # 64 tiles on 256 CUs; 517 k-steps -> 4 x 130
    assert list(zip(per_linear(p, "Z"), per_linear(p, "Tp"))) == [(10, 16640), (32, 17408), (16, 16896), (16, 16896)]
    assert per_linear(p, "pad_rows") == tuple(max(tp, 16640) for tp in per_linear(p, "Tp"))
    # q = 64, rem = 140: every product's last row of tiles crosses a round, every contraction is a multiple of 16 k-steps
    assert per_linear(p, "fwd_tail") == (BLOCKS,) * 4 and per_linear(p, "dgrad_tail") == (BLOCKS,) * 4
    assert flags(p) == ALL_ON
    assert p["batched"] == 1 and p["attn_t_f32_mfma"] == 0 and p["rows_fit"] == 1 and p["parts_fit"] == 1
    # block 0's qkv keeps the pass over norm1's input; from block 1 on every operand comes from its producer
    assert per_linear(p, "src0") == (LN_INPUT, PRODUCER, PRODUCER, PRODUCER)
    assert per_linear(p, "src1") == per_linear(p, "src2") == (PRODUCER,) * 4


def test_configs4_under_the_superseded_switches(driver):
    p = plan(driver, 512, variants=1, TRAIN_TAIL="split", **CONFIGS4)
    # 16 k-steps: the extra round; 32 and 48 k-steps: Z = 16 chunks, 16 x 140 x 512 floats of the 16 x 256 x 1536 there are
    assert per_linear(p, "fwd_tail") == (WHOLE, WHOLE, WHOLE, SPLIT) and p["fc2_fwd_tail_Z"] == 16
    assert per_linear(p, "dgrad_tail") == (SPLIT, WHOLE, SPLIT, WHOLE) and (p["qkv_dgrad_tail_Z"], p["fc1_dgrad_tail_Z"]) == (16, 16)
    assert p["L_part_rem_floats"] == 16 * 256 * 1536
    p = plan(driver, 512, variants=1, TRAIN_WGRAD="each", **CONFIGS4)
    assert p["merged"] == 0 and per_linear(p, "pad_rows") == per_linear(p, "Tp") == (16640, 17408, 16896, 16896)
    p = plan(driver, 512, variants=1, TRAIN_GELU="pass", **CONFIGS4)
    assert flags(p) == dict(ALL_ON, gip=0)
    p = plan(driver, 512, variants=1, TRAIN_LN_OPERAND="pass", **CONFIGS4)
    assert flags(p) == dict(ALL_ON, ln_direct=0, att_direct_s=0, att_direct_t=0)
    assert per_linear(p, "src0") == per_linear(p, "src1") == (LN_INPUT, ROWS, LN_INPUT, PRODUCER)


def test_configs4_on_other_cu_counts(driver):
    p = plan(driver, 512, n_cu=304, **CONFIGS4)
    assert (p["mZ"], p["mTp"]) == (4, 16640)                            # 304 / 64 tiles is still 4
    assert (p["qkv_Z"], p["qkv_Tp"]) == (12, 16896)                     # 304 / 24 tiles; 517 k-steps -> 12 x 44
    # 780 / 768 qkv tiles are 3 rounds of 304 either way, 260 / 256 proj tiles 1, 520 / 512 fc1 tiles 2: no remainder costs a round
    assert per_linear(p, "fwd_tail") == (WHOLE,) * 4
    p = plan(driver, 512, n_cu=128, **CONFIGS4)
    assert (p["merged"], p["mZ"], p["mTp"]) == (1, 2, 16576)            # 128 / 64 tiles; 517 k-steps -> 2 x 259
    assert per_linear(p, "fwd_tail") == (BLOCKS,) * 4                   # 780 / 768 -> 7 / 6, 260 / 256 -> 3 / 2, 520 / 512 -> 5 / 4


def test_attention_switches_move_the_proj_operand_alone(driver):
    p = plan(driver, 512, TRAIN_ATTN="x2t", **CONFIGS4)
    assert (p["attn_x2_s"], p["attn_x2_t"], p["att_direct_s"], p["att_direct_t"]) == (0, 1, 0, 1)
    assert (p["proj_src0"], p["proj_src1"], p["proj_src2"]) == (ROWS, PRODUCER, ROWS)      # blocks 0, 2: spatial; 1: temporal
    p = plan(driver, 512, TRAIN_ATTN="f32", **CONFIGS4)
    assert (p["attn_x2_s"], p["attn_x2_t"], p["att_direct_s"], p["att_direct_t"], p["attn_t_f32_mfma"]) == (0, 0, 0, 0, 1)
    assert (p["proj_src0"], p["proj_src1"]) == (ROWS, ROWS) and p["qkv_src1"] == PRODUCER
    assert plan(driver, 512, TRAIN_OVERLAP="0", **CONFIGS4)["needs_aux"] == 0
    assert plan(driver, 512, TRAIN_OVERLAP="1", **CONFIGS4)["overlap_sets"] == 1
    assert plan(driver, 512, TRAIN_PASSES="1", **CONFIGS4)["passes"] == 1


def test_width_256(driver):
    p = plan(driver, 256)
    assert per_linear(p, "tn") == (1, 1, 1, 1) and flags(p) == ALL_ON
    assert per_linear(p, "src1") == (PRODUCER,) * 4


def test_width_64_is_below_the_tn_tile(driver):
    p = plan(driver, 64)
    assert p["use_x2"] == 1 and per_linear(p, "tn") == (0, 0, 0, 0) and flags(p) == ALL_OFF
    assert per_linear(p, "src0") == per_linear(p, "src1") == (ROWS_T,) * 4
    assert per_linear(p, "pad_rows") == per_linear(p, "Tp")
    assert (p["attn_x2_t"], p["attn_x2_s"]) == (0, 0)                   # head dim 8


def test_width_128_has_one_tn_linear(driver):
    """fc1 is [256, 128] at the model's mlp_ratio 2 -- one whole 256 x 128 tile: d3dp_tn_applies held there before the plan existed
    too.  The other three are below the tile."""
    p = plan(driver, 128)
    assert p["use_x2"] == 1 and per_linear(p, "tn") == (0, 0, 1, 0)
    assert flags(p) == dict(ALL_OFF, gip=1)
    assert per_linear(p, "src0") == per_linear(p, "src1") == (ROWS_T, ROWS_T, ROWS, ROWS_T)
    assert per_linear(p, "pad_rows") == per_linear(p, "Tp")
    assert (p["attn_x2_t"], p["attn_x2_s"]) == (1, 1)                   # head dim 16
    p = plan(driver, 128, hidden=128)                                  # (fc1 [128, 128]: nothing TN)
    assert per_linear(p, "tn") == (0, 0, 0, 0) and flags(p) == ALL_OFF


def test_the_mixed_case_at_384(driver):
    p = plan(driver, 384, TRAIN_IMPL="f16x2")                          # (1152, 384), (384, 384), (768, 384), (384, 768)
    assert p["use_x2"] == 1 and per_linear(p, "tn") == (0, 0, 1, 0)
    assert flags(p) == dict(ALL_OFF, gip=1)
    assert per_linear(p, "src0") == per_linear(p, "src1") == (ROWS_T, ROWS_T, ROWS, ROWS_T)
    assert plan(driver, 384)["use_x2"] == 0                            # (without the switch: the fp32 path)


def test_the_fp32_path_routes_nothing(driver):
    for p in (plan(driver, 96), plan(driver, 512, TRAIN_IMPL="f32")):
        assert (p["use_x2"], p["attn_x2_s"], p["attn_x2_t"], p["needs_aux"], p["attn_t_f32_mfma"]) == (0, 0, 0, 0, 0)
        assert flags(p) == ALL_OFF
    assert per_linear(plan(driver, 96), "N") == (288, 96, 192, 96) and per_linear(plan(driver, 96), "K") == (96, 96, 96, 192)


def test_depth_9_prepares_each_weight_where_it_is_used(driver):
    assert plan(driver, 256, depth=8)["batched"] == 1                  # 64 Linears: d3dp_launch_wprep's table
    assert plan(driver, 256, depth=9)["batched"] == 0


def test_a_short_batch_takes_remainder_blocks_where_the_round_count_changes(driver):
    p = plan(driver, 512, B=2, frames=159, joints=17)                  # T = 5,406 = 21 x 256 + 30
    assert p["T"] == 5406
    # qkv: 22 x 12 = 264 tiles are two rounds of 256, 21 x 12 = 252 one; proj / fc2 (88 / 84) and fc1 (176 / 168): one either way
    assert per_linear(p, "fwd_tail") == (BLOCKS, WHOLE, WHOLE, WHOLE)
    assert per_linear(p, "dgrad_tail") == (WHOLE,) * 4                  # (512, 512, 512, 1024 output columns: at most 176 tiles)


def test_the_split_remainder_needs_32_k_steps(driver):
    # (hidden is a multiple of 64 at these widths: an even number of k-steps, so some Z in 2 .. 16 always divides it)
    kw = dict(variants=1, TRAIN_TAIL="split", B=4, frames=243, joints=17)
    p = plan(driver, 512, hidden=1152, **kw)                           # fc2: 36 k-steps, the largest divisor up to 16 is 12
    assert (p["fc2_fwd_tail"], p["fc2_fwd_tail_Z"]) == (SPLIT, 12)
    p = plan(driver, 512, hidden=960, **kw)                            # 30 k-steps: below 32
    assert (p["fc2_fwd_tail"], p["fc2_fwd_tail_Z"]) == (WHOLE, 1)


# ---------------------------------------------------------------------------------------------- invariants over a sweep
REGIONS = ("temb", "x_final", "saved0", "xn", "y", "hid", "dA", "dB", "dC", "dqkv", "dh", "z", "At", "Xt", "Wt", "dtemb", "stats", "op_a",
           "op_w", "op_at", "part", "op_a2", "op_at2", "part2", "part_rem", "slots", "x_cols", "w_rows", "w_cols", "stats_x2", "red")


def region_sizes(p, C, Hd, heads, F, J, depth, B):
    """Floats every region of the workspace holds, from what it is documented to hold."""
    T, Tpad, Tp_max = p["L_T"], p["L_Tpad"], p["L_Tp_max"]
    unit, wide, kmax, nmax = T * C, max(3 * C, Hd), max(C, Hd), max(F, J)
    return dict(temb=B * C, x_final=unit, saved0=p["L_saved_stride"] * 2 * depth, xn=unit, y=unit, hid=T * Hd, dA=unit, dB=unit, dC=unit,
                dqkv=3 * unit, dh=T * Hd, z=unit, At=wide * Tpad, Xt=wide * Tpad, Wt=wide * wide, dtemb=2 * B * C,
                stats=B * nmax * heads * nmax * 12 // 4 + 64, op_a=p["L_dy_set_floats"], op_w=wide * kmax, op_at=wide * Tp_max,
                part=p["L_part_floats"], op_a2=p["L_dy_set_floats"], op_at2=wide * Tp_max, part2=p["L_part_floats"],
                part_rem=p["L_part_rem_floats"], slots=2 * p["slots"], x_cols=p["L_x_block"] * 2 * depth, w_rows=p["L_w_block"] * 2 * depth,
                w_cols=p["L_w_block"] * 2 * depth, stats_x2=p["L_stats_x2_stride"] * 2 * depth, red=p["L_red_floats"])


def check_invariants(p, C, Hd, heads, F, J, depth, B):
    align = lambda n: (n + 63) // 64 * 64
    size = region_sizes(p, C, Hd, heads, F, J, depth, B)
    off = 0
    for name in REGIONS:                                                # ascending, nothing between or over two regions, the end is the total
        assert p[f"L_{name}"] == off, name
        off += align(size[name])
    assert off == p["L_total_floats"]
    T = p["L_T"]
    assert p["L_saved_stride"] >= 7 * T * C + T * Hd and p["L_dy_set_floats"] == p["L_Tp_max"] * (5 * C + Hd)
    assert p["L_x_block"] == (3 * C + Hd) * p["L_Tp_max"] and p["L_w_block"] == 4 * C * C + 2 * Hd * C
    assert p["L_stats_x2_stride"] * 4 >= B * J * heads * F * 8
    assert p["L_bias_rows"] == 512 and p["L_ln_rows"] == min((T + 3) // 4, 512)
    # the forward pass' three slot ranges and the backward pass' do not meet
    assert 2 * (8 * depth - 1) + 1 < p["slot_qkv0"] and p["slot_qkv0"] + 2 * depth <= p["slot_pmax0"]
    assert p["slot_pmax0"] + 2 * depth <= p["slot_bwd0"] < p["slots"]
    if not p["use_x2"]:
        return
    fits = all(p[f"{n}_pad_rows"] <= p["L_Tp_max"] and p[f"{n}_Tp"] <= p["L_Tp_max"] for n in LINEARS)
    assert fits or not (p["rows_fit"] and p["parts_fit"])
    assert all(p[f"{n}_Z"] * p[f"{n}_N"] * p[f"{n}_K"] <= p["L_part_floats"] for n in LINEARS) or not p["parts_fit"]
    for n in LINEARS:
        assert p[f"{n}_Tp"] >= T and p[f"{n}_Tp"] % (32 * p[f"{n}_Z"]) == 0 and p[f"{n}_pad_rows"] >= p[f"{n}_Tp"]
        assert p[f"{n}_tn"] == int(p[f"{n}_N"] % 256 == 0 and p[f"{n}_K"] % 128 == 0)
        for side, cols in (("fwd", p[f"{n}_N"]), ("dgrad", p[f"{n}_K"])):
            if p[f"{n}_{side}_tail"] == SPLIT:
                assert p[f"{n}_{side}_tail_Z"] * (T % 256) * cols <= p["L_part_rem_floats"]
            else:
                assert p[f"{n}_{side}_tail_Z"] == 1
    if p["merged"]:
        assert p["mTp"] <= p["L_Tp_max"] and p["mTp"] >= T and p["mTp"] % (32 * p["mZ"]) == 0
        assert p["mZ"] * sum(p[f"{n}_N"] * p[f"{n}_K"] for n in LINEARS) <= p["L_part_floats"]
        assert all(p[f"{n}_tn"] for n in LINEARS) and all(p[f"{n}_pad_rows"] >= p["mTp"] for n in LINEARS)
    # a flag that names a TN-only launch form implies the TN shape of the Linear it concerns
    assert p["ln_direct"] <= p["ln_fused"] <= min(p["qkv_tn"], p["fc1_tn"]) and p["gip"] <= p["fc1_tn"]
    assert p["gelu_operand"] == p["mip2"] == p["fc2_tn"] and p["mip1"] == p["proj_tn"]
    assert max(p["att_direct_s"], p["att_direct_t"]) <= min(p["ln_direct"], p["proj_tn"])


TOKENS = (1, 31, 33, 255, 256, 257, 4095, 4097, 5406, 8192, 16524, 19999)


def test_invariants_over_a_sweep(driver):
    shapes = []
    for cs in range(64, 1025, 32):
        for env in ({}, {"TRAIN_IMPL": "f16x2"}) if cs in (192, 320, 384, 448) else ({},):
            for depth in (1, 8, 9):
                for i, T in enumerate(TOKENS):
                    n_cu = 304 if i % 3 == 2 else 256
                    shapes.append((dict(heads=8, frames=1, joints=1, depth=depth, B=T, n_cu=n_cu, **env), cs))
    got = plans(driver, *[case(cs, **kw) for kw, cs in shapes])
    split = 0
    for (kw, cs), p in zip(shapes, got):
        assert p is not None, (cs, kw)
        check_invariants(p, cs, 2 * cs, 8, 1, 1, kw["depth"], kw["B"])
        split += p["use_x2"]
    assert split == 8 * 3 * len(TOKENS)                                 # 64, 128, 256, 512 and the four opted-in widths


def test_invariants_at_real_clip_shapes_and_the_superseded_forms(driver):
    kws = [dict(CONFIGS4), dict(CONFIGS4, n_cu=304), dict(hidden=1024, depth=2, B=3, frames=27, joints=17),
           dict(CONFIGS4, variants=1, TRAIN_TAIL="split"), dict(CONFIGS4, variants=1, TRAIN_WGRAD="each"),
           dict(hidden=1152, depth=1, B=4, frames=243, joints=17, variants=1, TRAIN_TAIL="split")]
    for kw, p in zip(kws, plans(driver, *[case(512, **kw) for kw in kws])):
        assert p is not None, kw
        check_invariants(p, 512, kw["hidden"], 8, kw["frames"], kw["joints"], kw["depth"], kw["B"])


def test_the_workspace_holds_no_region_nobody_reads(driver):
    """The sum of the documented regions IS the size query's answer (check_invariants): neither the transposed activation operand
    of the fp32 layout's early form (kmax x Tp_max floats) nor a bias of zeros (4 C floats) is part of it."""
    p = plan(driver, 512, **CONFIGS4)
    assert "L_op_xt" not in p and "L_zero_bias" not in p
    check_invariants(p, 512, 1024, 8, 243, 17, 8, 4)
