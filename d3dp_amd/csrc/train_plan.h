// What a training step decides before it launches anything: where every tensor of the step lies in the caller's workspace
// (TrainLayout, train_layout) and which launch forms the step's shape and the context's switches select (TrainPlan,
// plan_train_step).  Both passes of a step -- d3dp_train_forward and d3dp_train_backward, capi_train.hip -- begin by computing the
// two and only carry them out: the operand forms, row paddings and slots the backward pass reads are the ones the forward pass
// of the same step wrote because both read them here.  Pure integer arithmetic on a d3dp_cfg, a CtxPlan, the batch size and the
// CU count: no HIP, so that any machine can check it (tests/test_train_plan_host.py).  Recomputed per call: a few dozen operations.
#pragma once
#include <cstddef>

#include "ctx_plan.h"

// ---- what the layout and the plan need to know of the kernels (the file that owns the real thing asserts the value) ----------
constexpr int D3DP_DYPREP_ROWS = 96;        // partial rows of column sums d3dp_launch_dyprep leaves (gemm_x2_train.hip)
constexpr int D3DP_ROWPREP_ROWS = 512;      // ... at most, d3dp_launch_rowprep
constexpr int D3DP_LN_BWD_BLOCKS = 512;     // workgroups of a LayerNorm-backward call: one [dgamma | dbeta] partial row each (train.hip)
constexpr int D3DP_EMBED_BWD_ROWS = 64;     // partial tables of d3dp_train_embed_bwd
constexpr int D3DP_TN_MAX = 4;              // products of one d3dp_launch_linear_f16x2_tn_many launch
constexpr size_t D3DP_TRAIN_ATTN_STAT_BYTES = 12;           // per query: train.hip AttnStats
constexpr size_t D3DP_TRAIN_ATTN_X2_STAT_BYTES = 8;         // per query: train_attn.hip TAStat
// (D3DP_WPREP_MAX, D3DP_TN_TILE_N / _K and d3dp_tn_applies: ctx_plan.h -- plan_context's step 7b asks them too)
// partial rows one LayerNorm-backward call over T tokens leaves
inline int d3dp_train_ln_bwd_blocks(int T) { return (T + 3) / 4 < D3DP_LN_BWD_BLOCKS ? (T + 3) / 4 : D3DP_LN_BWD_BLOCKS; }
inline size_t d3dp_train_attn_stats_bytes(int n_seq, int n_tok, int heads) { return (size_t)n_seq * heads * n_tok * D3DP_TRAIN_ATTN_STAT_BYTES; }
inline size_t d3dp_train_attn_x2_stats_bytes(int n_seq, int n_tok, int heads) { return (size_t)n_seq * heads * n_tok * D3DP_TRAIN_ATTN_X2_STAT_BYTES; }

// absmax / unscale slots of a step's operands (X2Train, capi_train.hip): the forward pass owns [0, kTrainBwdSlot0) -- slots 2 l and
// 2 l + 1 of Linear l from 0, a block's qkv-output absmax from kTrainQkvSlot0, its largest positive fc1 output from kTrainPmaxSlot0 --,
// the backward pass allocates from kTrainBwdSlot0
constexpr int kTrainSlots = 8192, kTrainBwdSlot0 = 4096, kTrainQkvSlot0 = 2048, kTrainPmaxSlot0 = 3072;

// ---- the workspace of a step ------------------------------------------------------------------------------------------------
struct TrainLayout {
  size_t T, Tpad, C, Hd, unit;      // unit = T*C floats
  // offsets in floats
  size_t temb, x_final, saved0, saved_stride;
  // per-block saved tensors (offsets inside a block's slab)
  size_t o_xin, o_qkv, o_att, o_xmid, o_hpre, o_xout;
  // temporaries
  size_t xn, y, hid, dA, dB, dC, dqkv, dh, z, At, Xt, Wt, dtemb, stats;
  // split-fp16 operands of the training Linears (X2Train, capi_train.hip): row form [rows][2 K] and transposed form [features][2 Tp]
  size_t op_a, op_w, op_at, part, part_rem, slots;
  size_t dy_set_floats;             // capacity of `op_a` and of `op_a2`: the four dY of a block side by side
  size_t part_floats;               // capacity of `part` and of `part2`: split-K partial products, at most ~ (CUs + tiles) output tiles
  size_t part_rem_floats;           // capacity of `part_rem`
  size_t op_a2, op_at2, part2;      // a second set of the dY operand and partial-tile regions: two weight-gradient products in flight
  size_t x_cols, x_block;           // every Linear's activation operand kept from the forward pass for its wgrad: the ROW form [Tp][2 K]
                                    // where the TN kernel applies (it is then also the forward product's operand), else the transposed [K][2 Tp]
  size_t w_rows, w_cols, w_block;   // every weight's split operands (row form / transposed form), prepared once per step: w_block floats per block
  size_t Tp_max;                    // columns (tokens, padded) of a transposed operand row
  size_t stats_x2, stats_x2_stride; // per block: (log-sum-exp, dO . O) of every query of the split-fp16 temporal attention
  size_t red, red_floats;           // partial sums of the backward pass (LayerNorm gammas / betas, biases, embedding side),
                                    // summed in a fixed order by d3dp_train_reduce_many at its end
  // partial rows the producers of `red` leave, as its size counts them
  int ln_rows;                      // of one LayerNorm-backward call over T tokens (<= D3DP_LN_BWD_BLOCKS)
  int bias_rows;                    // of a dY's column sums (the bias gradient), whichever operand pass leaves them
  int head_rows, embed_bias_rows;   // of the head Linear's backward; of the embedding bias' column sums
  int group_slices;                 // slices of the grouped row sums (position / time embedding gradients)
  size_t total_floats;
};

inline TrainLayout train_layout(const d3dp_cfg& g, int B) {
  TrainLayout L{};
  L.T = (size_t)B * g.frames * g.joints;
  L.Tpad = (L.T + 15) / 16 * 16;
  L.C = g.channels; L.Hd = g.hidden; L.unit = L.T * L.C;
  L.ln_rows = d3dp_train_ln_bwd_blocks((int)L.T);
  L.bias_rows = std::max(D3DP_DYPREP_ROWS, D3DP_ROWPREP_ROWS);
  L.head_rows = 512; L.embed_bias_rows = 512; L.group_slices = 32;
  size_t off = 0;
  auto take = [&](size_t n) { size_t o = off; off += (n + 63) / 64 * 64; return o; };
  L.temb = take((size_t)B * L.C);
  L.x_final = take(L.unit);
  L.o_xin = 0; L.o_qkv = L.unit; L.o_att = 4 * L.unit; L.o_xmid = 5 * L.unit; L.o_hpre = 6 * L.unit;
  L.o_xout = 6 * L.unit + L.T * L.Hd;
  L.saved_stride = (7 * L.unit + L.T * L.Hd + 63) / 64 * 64;
  L.saved0 = take(L.saved_stride * 2 * g.depth);
  L.xn = take(L.unit); L.y = take(L.unit); L.hid = take(L.T * L.Hd);
  L.dA = take(L.unit); L.dB = take(L.unit); L.dC = take(L.unit);
  L.dqkv = take(3 * L.unit); L.dh = take(L.T * L.Hd); L.z = take(L.unit);
  const size_t wide = std::max<size_t>(3 * L.C, L.Hd);
  L.At = take(wide * L.Tpad); L.Xt = take(wide * L.Tpad); L.Wt = take(wide * wide);
  L.dtemb = take((size_t)B * 2 * L.C);              // (the training forward's time-MLP hidden layer borrows it: B x 2 C)
  L.stats = take(d3dp_train_attn_stats_bytes(B * std::max(g.frames, g.joints), std::max(g.frames, g.joints), g.heads) / 4 + 64);
  {
    const size_t fmax = std::max<size_t>(3 * L.C, L.Hd), kmax = std::max<size_t>(L.C, L.Hd);
    L.Tp_max = ((L.T + 31) / 32 + 64) * 32;          // (room for rounding the k-steps up to a multiple of the split count)
    const size_t dy_all = 5 * L.C + L.Hd;            // the four dY of a block side by side (their weight gradients go out as ONE launch)
    L.dy_set_floats = L.Tp_max * dy_all;
    L.op_a = take(L.dy_set_floats);                  // [Tp][2 N] fp16 = Tp N floats per dY (rows T .. Tp - 1: the TN wgrad's zero rows)
    L.op_w = take(fmax * kmax);                      // [N][2 K] or [K][2 N] fp16
    L.op_at = take(fmax * L.Tp_max);                 // dY^T: [N][2 Tp] fp16
    L.part_floats = (size_t)(1024 + 64) * 256 * 128;
    L.part = take(L.part_floats);
    L.op_a2 = take(L.dy_set_floats); L.op_at2 = take(fmax * L.Tp_max); L.part2 = take(L.part_floats);
    L.part_rem_floats = (size_t)16 * 256 * fmax;
    L.part_rem = take(L.part_rem_floats);            // ... of a forward / dgrad product's remainder rows (its own region: the
                                                     // weight-gradient product of the same dY runs concurrently on the second stream)
    L.slots = take(2 * kTrainSlots);                       // absmax words | 1 / scale per operand
    L.w_block = 4 * L.C * L.C + 2 * L.Hd * L.C;      // qkv | proj | fc1 | fc2 of one block ([N][2 K] fp16 = N K floats each)
    L.x_block = (3 * L.C + L.Hd) * L.Tp_max;         // qkv | proj | fc1 | fc2 inputs of one block
    L.x_cols = take(L.x_block * 2 * g.depth);
    L.w_rows = take(L.w_block * 2 * g.depth);
    L.w_cols = take(L.w_block * 2 * g.depth);
  }
  L.stats_x2_stride = (d3dp_train_attn_x2_stats_bytes(B * g.joints, g.frames, g.heads) / 4 + 63) / 64 * 64;   // (temporal axis: B J sequences of F tokens)
  L.stats_x2 = take(L.stats_x2_stride * 2 * g.depth);
  {
    const size_t lnb = (size_t)D3DP_LN_BWD_BLOCKS * 2 * L.C;         // one LayerNorm call's [dgamma | dbeta] rows
    L.red_floats = (size_t)(6 * g.depth + 2) * lnb                   // 3 LayerNorm backward calls per block + the head's
                   + (size_t)2 * g.depth * L.bias_rows * (5 * L.C + L.Hd + 256)   // bias gradients: the column sums of every dY
                   + (size_t)L.head_rows * (3 * L.C + 4) + (size_t)D3DP_EMBED_BWD_ROWS * 5 * L.C + (size_t)L.embed_bias_rows * L.C   // head, embedding
                   + (size_t)L.group_slices * (g.joints + (size_t)B) * L.C + 4096;                              // spos, time embedding
    L.red = take(L.red_floats);
  }
  L.total_floats = off;
  return L;
}

// ---- the route of a step ----------------------------------------------------------------------------------------------------
// The head dims the training step's attention kernels take (train_attn.hip): mfma_head_dim's, and 24 / 40 / 48 / 56 padded to 32 / 64
// inside its kernels -- the head dims of channels in {192, 320, 384, 448} with the model's 8 heads, reached under
// D3DP_TRAIN_IMPL=f16x2 only (plan_context)
inline bool train_attn_head_dim(int hd) { return mfma_head_dim(hd) || hd == 24 || hd == 40 || hd == 48 || hd == 56; }

// Which path a TRAIN context's step takes: the part of the plan that needs neither a batch size nor a device (d3dp_create asks it
// whether to make the second stream).
//   use_x2     the Linears on split-fp16 operands (train_linears_split); else the fp32 matrix cores.  CtxPlan::train_x2: the
//              instantiated widths unless D3DP_TRAIN_IMPL=f32, and channels in {192, 320, 384, 448} under D3DP_TRAIN_IMPL=f16x2
//   attn_x2(a) axis a's attention on the split-fp16 kernels of train_attn.hip: they need the split Linears' device-side scales
//              and a head dim those kernels take (train_attn_head_dim: 64, 32, 16 -- `-cs` 512 / 256 / 128 with the model's 8 heads --
//              and 56, 48, 40, 24 -- `-cs` 448 / 384 / 320 / 192 -- padded to 64 / 32 inside the kernels); clips of up to 1024 frames
//              (beyond 256 their keys / queries pass through LDS in chunks).  Head dim 8, the cross-check switches and every
//              context on the fp32 path stay on the fp32 kernels of train.hip (<= 256 frames; any length up to 1024 under
//              D3DP_TRAIN_LONG_ATTN=chunked: TrainPlan::attn_bwd_chunked)
//   needs_aux  the backward pass forks its weight-gradient products onto the context's second stream (made by d3dp_create)
struct TrainPath {
  bool use_x2, attn_x2_t, attn_x2_s, needs_aux;
  bool attn_x2(int axis) const { return axis == 1 ? attn_x2_t : attn_x2_s; }
};
inline TrainPath plan_train_path(const CtxPlan& c, const d3dp_cfg& g) {
  TrainPath p{};
  p.use_x2 = train_linears_split(c, g);
  p.attn_x2_t = p.use_x2 && c.train_attn_x2 > 0 && train_attn_head_dim(g.channels / g.heads) && g.frames <= 1024;
  p.attn_x2_s = p.attn_x2_t && c.train_attn_x2 > 1;      // the spatial axis too
  p.needs_aux = g.mode == D3DP_MODE_TRAIN && p.use_x2 && c.train_overlap;
  return p;
}

enum TrainLinearId { kQkv = 0, kProj = 1, kFc1 = 2, kFc2 = 3 };   // Linear l of the step = 4 block + one of these

// Where the activation operand of a forward product comes from (split-fp16 path)
enum class TrainOperand {
  ROWS,        // an operand pass over fp32 rows: the row form [Tp][2 K], kept for the TN weight gradient (d3dp_launch_rowprep)
  ROWS_T,      // ... the row form for this product and the transposed form [K][2 Tp] for the weight gradient (d3dp_launch_dyprep)
  LN_INPUT,    // an operand pass over the INPUT of the LayerNorm in front of the Linear, normalising on the fly (d3dp_launch_rowprep_ln)
  PRODUCER     // no pass: the kernel that produced the activation wrote its operand rows
};
// How a forward / dgrad product out[T, N] = A2 . W2^T handles its last T mod 256 rows (X2Train::gemm)
enum class TrainTailForm {
  WHOLE_TILES, // one launch over ceil(T / 256) rows of tiles
  REM_BLOCKS,  // one launch: the remainder rows as 16 x 64 blocks spread over all workgroups
  SPLIT_REM    // the whole tiles, then the remainder rows as a split-K product over Z chunks and the sum of its partial products
};
struct TrainTail { TrainTailForm form; int Z; };
inline TrainTail train_tail(int T, int N, int K, int n_cu, bool tail_blocks, size_t part_rem_floats) {
  const int tn = (N + 127) / 128, q = T / 256, rem = T - q * 256;
  const int rounds_all = ((q + (rem ? 1 : 0)) * tn + n_cu - 1) / n_cu, rounds_full = (q * tn + n_cu - 1) / n_cu;
  const int nk = K / 32;
  int Z = 1;
  for (int z = 2; z <= 16; ++z)
    if (nk % z == 0) Z = z;
  // (measured: a last round of a few tiles runs its k-steps at 0.75 us -- few CUs active, full clock -- against 1.4 us in a
  //  full round, so for 16 k-steps it costs 12 us, what the second launch and the sum cost too: split from 32 k-steps on)
  // the remainder rows as 16 x 64 blocks at the end of the same launch (gemm_f16x2_dyn_kernel): wherever they would cost a round
  if (tail_blocks && rem && q && rounds_all > rounds_full && nk % 16 == 0) return {TrainTailForm::REM_BLOCKS, 1};
  if (rem == 0 || q == 0 || rounds_all == rounds_full || Z == 1 || nk < 32 || (size_t)Z * rem * N > part_rem_floats)
    return {TrainTailForm::WHOLE_TILES, 1};
  return {TrainTailForm::SPLIT_REM, Z};
}

// One of a block's four Linears out[T, N] = A[T, K] W[N, K]^T + b, the same in every block
struct TrainLinear {
  int N, K;
  bool tn;                 // d3dp_tn_applies(N, K): the weight gradient reads both operands in their row forms
  int Z, Tp;               // split count / padded token count of its own weight-gradient product dW[N, K] = dY^T X
  int pad_rows;            // rows its operands -- the activation's, kept from the forward pass, and its dY's -- have (zero behind T)
  TrainOperand src;        // of its forward product.  (qkv in block 0: TrainPlan::qkv_src0; proj behind a split-fp16 attention that
                           // writes the operand: TrainPlan::source)
  TrainTail fwd_tail, dgrad_tail;
};

struct TrainPlan {
  TrainPath path;
  bool use_x2;                       // = path.use_x2; everything below but T, passes, attn_passes and overlap_sets is false / unused without it
  int T, passes, overlap_sets;
  // D3DP_TRAIN_ATTN_PASSES (CtxPlan::train_attn_passes): the fp16-MFMA passes per product of every attention that runs on
  // train_attn.hip (path.attn_x2); 1 = its one-pass kernels (train_attn_1p.hip).  The fp32 attention of an axis does not read it.
  int attn_passes;
  // D3DP_TRAIN_ROWS=hi (CtxPlan::train_rows_hi): every operand row of X2Train's Linears is K plain fp16 values (half the stride of the
  // split rows; train_layout's regions are unchanged and half used) and the products run the whole-line one-pass kernels
  bool rows_hi;
  // D3DP_TRAIN_LONG_ATTN=chunked (CtxPlan::train_long_attn): an axis on the fp32 attention runs the chunked VALU backward of train.hip
  // wherever the whole-sequence VALU pair ran or refused, so the forward pass takes clips beyond 256 frames there too
  bool attn_bwd_chunked;
  TrainLinear lin[4];                // by TrainLinearId
  // the qkv / fc1 operands straight from the INPUT of the LayerNorm in front of them (no fp32 normalised activation is written)
  bool ln_fused;
  // ... and (round 6) written BY the kernel that produces that input, at the scale the LayerNorm's own weights bound (train.hip
  // ln_operand_scale): the operand pass in front of qkv / fc1 disappears (block 0's qkv operand: the embedding kernel is shared
  // with inference and keeps the pass)
  bool ln_direct;
  TrainOperand qkv_src0;
  // the split-fp16 attention of an axis also writes the proj Linear's operand rows (scale: the qkv absmax bounds every output), round 6
  bool att_direct_s, att_direct_t;
  bool att_direct(int axis) const { return axis == 1 ? att_direct_t : att_direct_s; }
  // the temporal attention runs on the fp32 matrix cores (the kernel is shared with inference and leaves no absmax: proj's operand
  // pass takes it first)
  bool attn_t_f32_mfma;
  // fc2 takes its GELU'd input straight from its producer's output: the fc2 operand = split(GELU(fc1 output)) in one pass, its scale
  // from the largest positive fc1 output (the fc1 epilogue leaves it): no fp32 hidden tensor, no separate operand pass
  bool gelu_operand;
  bool gip;                          // d h_pre = d hidden x gelu'(h_pre) is formed by the operand pass of the fc1 gradients
  bool mip1, mip2;                   // the DropPath scales of the proj / fc2 dY are applied by its operand pass
  bool batched;                      // every weight's absmax, row form and transposed form in three launches at the start of the forward pass
  // The four weight gradients of a block as ONE launch; mZ / mTp: split count and padded token count of the merged list
  bool merged;
  int mZ, mTp;
  bool rows_fit;                     // every pad_rows <= TrainLayout::Tp_max; else both passes refuse
  bool parts_fit;                    // every weight gradient's Z N K partial products fit TrainLayout::part_floats; else the backward pass refuses

  TrainOperand source(int blk, int j) const {
    if (j == kQkv && blk == 0) return qkv_src0;
    if (j == kProj && att_direct(blk & 1)) return TrainOperand::PRODUCER;
    return lin[j].src;
  }
};

inline TrainPlan plan_train_step(const CtxPlan& c, const d3dp_cfg& g, int B, int n_cu) {
  TrainPlan P{};
  const TrainLayout L = train_layout(g, B);
  const int T = (int)L.T, C = g.channels, Hd = g.hidden;
  P.path = plan_train_path(c, g);
  P.use_x2 = P.path.use_x2;
  P.T = T; P.passes = c.train_passes; P.overlap_sets = c.train_overlap_sets;
  P.attn_passes = c.train_attn_passes;
  P.attn_bwd_chunked = c.train_long_attn;
  P.rows_hi = c.train_rows_hi && P.path.use_x2;
  const int shape[4][2] = {{3 * C, C}, {C, C}, {Hd, C}, {C, Hd}};       // [N, K] by TrainLinearId
  for (int j = 0; j < 4; ++j) { P.lin[j].N = shape[j][0]; P.lin[j].K = shape[j][1]; }
  if (!P.use_x2) return P;                                              // (the fp32 path: four plain products per block, nothing to route)
  const int nk = (T + 31) / 32;
  {
    // merged: on where every Linear of the block has a TN shape
    int tiles = 0;
    bool ok = c.train_wgrad_merged;
    size_t nk_sum = 0;
    for (int j = 3; j >= 0; --j) {
      const int N = shape[j][0], K = shape[j][1];
      ok = ok && d3dp_tn_applies(N, K); tiles += ((N + 255) / 256) * ((K + 127) / 128); nk_sum += (size_t)N * K;
    }
    P.mZ = std::max(1, std::min(std::min(n_cu / std::max(tiles, 1), 64), nk / 4));
    P.mTp = P.mZ * ((nk + P.mZ - 1) / P.mZ) * 32;
    P.merged = ok && (size_t)P.mTp <= L.Tp_max && (size_t)P.mZ * nk_sum <= L.part_floats;
  }
  auto ln_operand_applies = [](int N, int K) { return d3dp_tn_applies(N, K) && K <= 512; };   // (d3dp_launch_rowprep_ln: C <= 512)
  P.ln_fused = ln_operand_applies(3 * C, C) && ln_operand_applies(Hd, C);
  P.ln_direct = P.ln_fused && c.train_ln_direct && C % 256 == 0;
  P.gelu_operand = d3dp_tn_applies(C, Hd);                  // TN shapes only (the row form is then also the wgrad operand)
  P.att_direct_s = P.path.attn_x2(0) && P.ln_direct && d3dp_tn_applies(C, C);
  P.att_direct_t = P.path.attn_x2(1) && P.ln_direct && d3dp_tn_applies(C, C);
  P.attn_t_f32_mfma = !P.path.attn_x2(1) && C / g.heads == 64 && g.frames <= 256;
  P.gip = c.train_gelu_in_prep && d3dp_tn_applies(Hd, C) && Hd <= 1536;   // (TN shapes the row pass takes only)
  P.mip2 = d3dp_tn_applies(C, Hd); P.mip1 = d3dp_tn_applies(C, C);        // (TN shapes only)
  P.batched = 8 * g.depth <= D3DP_WPREP_MAX;                // (up to 64 Linears: depth <= 8; deeper models prepare each weight where it is used)
  P.rows_fit = P.parts_fit = true;
  for (int j = 0; j < 4; ++j) {
    TrainLinear& p = P.lin[j];
    p.tn = d3dp_tn_applies(p.N, p.K);
    {
      const int tiles = ((p.N + 255) / 256) * ((p.K + 127) / 128);
      p.Z = std::max(1, std::min(std::min(n_cu / tiles, 64), nk / 4));
      const int nkz = (nk + p.Z - 1) / p.Z;
      p.Tp = p.Z * nkz * 32;
    }
    p.pad_rows = P.merged ? std::max(p.Tp, P.mTp) : p.Tp;
    const TrainOperand pass = p.tn ? TrainOperand::ROWS : TrainOperand::ROWS_T;
    p.src = j == kFc2 ? (P.gelu_operand ? TrainOperand::PRODUCER : pass)
          : j == kProj ? pass
          : P.ln_direct ? TrainOperand::PRODUCER : P.ln_fused ? TrainOperand::LN_INPUT : pass;
    p.fwd_tail = train_tail(T, p.N, p.K, n_cu, c.train_tail_blocks, L.part_rem_floats);
    p.dgrad_tail = train_tail(T, p.K, p.N, n_cu, c.train_tail_blocks, L.part_rem_floats);   // dX[T, K] = dY[T, N] W[N, K]
    P.rows_fit = P.rows_fit && (size_t)p.pad_rows <= L.Tp_max;
    P.parts_fit = P.parts_fit && (size_t)p.Tp <= L.Tp_max && (size_t)p.Z * p.N * p.K <= L.part_floats;
  }
  P.qkv_src0 = P.ln_fused ? TrainOperand::LN_INPUT : P.lin[kQkv].src;
  return P;
}
