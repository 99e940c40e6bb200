// The training step (d3dp_train_forward / d3dp_train_backward): forward of the MixSTE2 train branch
// (mixste.py:215-225, H = 1) with saved activations, and the full backward, in a D3DP_MODE_TRAIN context (fp32 weights, borrowed).
// Every Linear -- forward, dgrad, wgrad -- runs on split-fp16 operands scaled on the device by their own absmax (X2Train), the
// weight gradients as TN products of two row-form operands (nothing is transposed), one merged launch per block on a second
// stream; attention on the split-fp16 kernels of train_attn.hip; the rest are row-wise fp32 kernels (train.hip) that leave the
// next Linear's operand or its absmax behind.  train_plan.h says which of these a step takes and where its tensors lie: both
// passes begin with its TrainLayout and TrainPlan and carry them out, neither decides a route here.  The fp32 matrix-core path
// (TrainPath::use_x2 false: D3DP_TRAIN_IMPL=f32, every width outside {64, 128, 256, 512} that D3DP_TRAIN_IMPL=f16x2 has not opted
// in) stays as the cross-check.  No float atomics (Reducer).
#include <optional>

#include "ctx.h"

namespace {

// one launch inside a profile scope of its class (pc: the context under d3dp_profile_enable, else null; st: the caller's stream)
#define TP(cls, call) { Scope ps_(pc, cls, st); LAUNCH_TRY(call); }

const float* mask_ptr(const float* masks, const d3dp_cfg& g, int B, int blk, int branch) {
  if (!masks) return nullptr;
  const size_t smax = (size_t)B * std::max(g.frames, g.joints);
  return masks + ((size_t)blk * 2 + branch) * smax;
}

// The backward pass' deferred, fixed-order sums: kernels leave partial rows in the workspace's `red` region (bump-allocated
// here), `add` only RECORDS where they go -- an item may be recorded long before its partial rows exist (the shared norms' rows are
// written by one LayerNorm-backward call per block) -- and `flush`, called once every producer has been launched, walks the list
// in launches of <= D3DP_REDUCE_MAX destinations (d3dp_train_reduce_many).  (Round 5 flushed from inside `add` when the table
// was full: at depth >= 6 that reduced the shared norms' rows before the remaining blocks had written theirs -- ADVICE r5.)
// Nothing in the backward pass adds floats atomically: its gradients are bit-reproducible.
struct Reducer {
  float* base;
  size_t cap, used = 0;
  hipStream_t st;
  std::vector<D3dpReduceItem> items{};
  int rc = 0;
  float* take(size_t n) {
    n = (n + 63) / 64 * 64;
    if (used + n > cap) { rc = -1; return nullptr; }
    float* p = base + used;
    used += n;
    return p;
  }
  void add(const float* part, float* dst, size_t n, size_t count, size_t stride, bool accumulate = false) {
    if (!part || !dst || rc) { rc = rc ? rc : -1; return; }
    items.push_back(D3dpReduceItem{part, dst, (unsigned)n, (unsigned)count, (unsigned)stride, accumulate ? 1u : 0u});
  }
  void flush() {
    for (size_t i = 0; i < items.size() && rc == 0; i += D3DP_REDUCE_MAX) {
      D3dpReduceTable tb{};
      tb.count = (int)std::min<size_t>(D3DP_REDUCE_MAX, items.size() - i);
      for (int j = 0; j < tb.count; ++j) tb.it[j] = items[i + j];
      rc = d3dp_train_reduce_many(tb, st);
    }
    items.clear();
  }
};

int lin32(const float* A, const float* W, const float* bias, float* out, int M, int N, int K, hipStream_t st) {
  return d3dp_launch_linear_f32(EPI_BIAS, A, W, bias, out, M, N, K, st);
}

// weight / bias of one of a block's four Linears (j: TrainLinearId)
const float* lin_w(const BlockDev& w, int j) { return (const float*)(j == kQkv ? w.qkv_w : j == kProj ? w.proj_w : j == kFc1 ? w.fc1_w : w.fc2_w); }
const float* lin_b(const BlockDev& w, int j) { return j == kQkv ? w.qkv_b : j == kProj ? w.proj_b : j == kFc1 ? w.fc1_b : w.fc2_b; }

// The training step's Linears on the split-fp16 scheme of EXACT inference (three fp16-MFMA passes, fp32-class; gemm_x2.hip
// gemm_f16x2_dyn_kernel) instead of the fp32 matrix cores (1/16 of the fp16 rate).  Every operand -- activations, weights,
// GRADIENTS -- is split at the power of two its own absmax asks for, computed and consumed on the device: no range is
// assumed and nothing synchronises.  forward: out = A W^T + b;  dgrad: dX = dY W (W^T split as the "weight" operand);
// wgrad: dW = dY^T X contracts over the batch's tokens into a handful of output tiles -> split-K over Z chunks of tokens,
// partial products summed in a fixed order (deterministic; the fp32 path's split-K used atomics).
// D3DP_TRAIN_PASSES=1 (TrainPlan::passes): the same launches on the one-pass instantiations of the two product kernels -- hi(A) x hi(W)
// alone, i.e. every operand rounded to fp16 at its own scale; operand passes, scales, k order, partial sums, streams: unchanged.
// D3DP_TRAIN_ROWS=hi (TrainPlan::rows_hi, beside passes = 1 alone): the same launches again with every operand -- activations, both weight
// forms, every dY -- as hi-only rows [.][K] at the START of its unchanged region, and the whole-line forms of the two product kernels.
// What a pass DECIDES is in the plan P (train_plan.h); this holds what a pass is in the middle of: the current operand set, the
// deferred TN products, the slot counter, the streams.
struct X2Train {
  hipStream_t st;
  float* ws;
  const TrainLayout& L;
  const TrainPlan& P;
  d3dp_ctx* pc;                                        // per-kernel profile (d3dp_profile_enable): classes T_LINEAR / T_WGRAD / T_OPERAND
  hipStream_t st_w = nullptr;                          // the weight-gradient products' stream (null: `st`)
  X2Train(d3dp_ctx* c, const TrainLayout& L_, const TrainPlan& P_, float* ws_, hipStream_t st_)
      : st(st_), ws(ws_), L(L_), P(P_), pc(c->prof ? c : nullptr) {
    use_set(0);
  }
  // the dY operand (row form / transposed form) and the weight-gradient product's partial tiles live in one of two sets of
  // regions: the backward pass alternates, so that the operand pass of the next dY need not wait for the product of this one
  size_t o_a = 0, o_at = 0, o_part = 0, set_base = 0, set_used = 0;
  void use_set(int s) {
    set_base = o_a = s ? L.op_a2 : L.op_a; set_used = 0; n_def = 0;
    o_at = s ? L.op_at2 : L.op_at; o_part = s ? L.part2 : L.part;
  }
  // The four weight gradients of a block as ONE launch (gemm_f16x2_tn_kernel's product table): each dY's operand pass takes the
  // next region of the set, wgrad() only records its product, flush_wgrads() launches them and the sum of their partial tiles.
  // On where every Linear of the block has a TN shape (TrainPlan::merged; mZ / mTp: split count and padded token count of the merged list).
  int n_def = 0;
  D3dpTnProduct def[D3DP_TN_MAX];
  float* def_dw[D3DP_TN_MAX];
  int flush_wgrads() {
    if (!n_def) return 0;
    hipStream_t sw = st_w ? st_w : st;
    Scope ps(pc, T_WGRAD, sw);
    int r = d3dp_launch_linear_f16x2_tn_many(def, n_def, P.mTp, P.mZ, sw, P.passes, P.rows_hi);
    if (r) return r;
    D3dpSumTable tb{};
    tb.n = n_def; tb.Z = P.mZ;
    for (int i = 0; i < n_def; ++i) { tb.part[i] = def[i].out; tb.out[i] = def_dw[i]; tb.n4[i] = (size_t)def[i].N * def[i].K / 4; }
    d3dp_launch_sum_partials_many(tb, sw);
    n_def = 0;
    return 0;
  }
  // absmax / unscale slots: the forward pass owns slots 2 l (activation operand) and 2 l + 1 (weight) of its Linear l = 4 block
  // + {qkv, proj, fc1, fc2} and leaves them -- with the operands themselves: the weights' two forms and every activation's
  // transposed form -- for the backward pass of the same step, whose wgrad / dgrad read the same tensors: 128 of the step's
  // 320 absmax launches are not repeated.  The backward pass allocates its own (the gradients) from kBwdSlot0.
  static constexpr int kBwdSlot0 = kTrainBwdSlot0;
  static constexpr int kQkvSlot0 = kTrainQkvSlot0;     // forward range: slot kQkvSlot0 + block = absmax of that block's qkv OUTPUT
  static constexpr int kPmaxSlot0 = kTrainPmaxSlot0;   // forward range: slot kPmaxSlot0 + block = largest positive fc1 output
  int next = 0;
  unsigned* amax() const { return reinterpret_cast<unsigned*>(ws + L.slots); }
  float* uns() const { return ws + L.slots + kTrainSlots; }
  // (null where the attention of that block's axis does not run on split-fp16 operands: nobody reads the slot)
  unsigned* qkv_amax(int blk) const { return P.path.attn_x2(blk & 1) ? amax() + kQkvSlot0 + blk : nullptr; }
  int begin(bool forward_pass) {
    next = forward_pass ? 0 : kBwdSlot0;
    return hipMemsetAsync(ws + L.slots + next, 0, (size_t)kBwdSlot0 * 4, st) == hipSuccess ? 0 : -3;
  }
  int take() { return (next < kBwdSlot0 || next >= kTrainSlots) ? -1 : next++; }   // a fresh slot of the backward range for a producer kernel to fill
  int slot_for(const float* src, size_t n) {           // absmax of a tensor into a fresh slot of the backward range
    if (next < kBwdSlot0 || next >= kTrainSlots) return -1;
    d3dp_launch_absmax(src, n, amax() + next, st);
    return next++;
  }
  void rows(const float* src, int R, int C, void* dst, int slot) {          // [R][C] -> [R][2 C]
    d3dp_launch_split2_dyn(src, dst, R, C, C, amax() + slot, uns() + slot, st);
  }
  void cols(const float* src, int R, int C, int Rpad, void* dst, int slot) {   // [R][C] -> [C][2 Rpad]
    d3dp_launch_split2_t_dyn(src, dst, R, C, Rpad, amax() + slot, uns() + slot, st);
  }
  // Every weight's absmax, row form and transposed form in three launches at the start of the forward pass (TrainPlan::batched: up
  // to 64 Linears, depth <= 8; deeper models prepare each weight where it is used).  woff(l): float offset of Linear l's operands
  // inside the w_rows / w_cols regions; xoff(l): of its activation operand inside x_cols.
  size_t xoff(int l) const { return (size_t)(l >> 2) * L.x_block + (size_t)(l & 3) * L.C * L.Tp_max; }
  size_t woff(int l) const {
    const size_t CC = L.C * L.C, j = (size_t)(l & 3);
    return (size_t)(l >> 2) * L.w_block + (j == 0 ? 0 : j == 1 ? 3 * CC : j == 2 ? 4 * CC : 4 * CC + L.Hd * L.C);
  }
  float* x_op(int l) const { return ws + L.x_cols + xoff(l); }   // Linear l's activation operand, kept for the backward pass of the step
  int prepare_weights(const d3dp_ctx* c) {
    if (!P.batched) return 0;
    const int nl = 8 * c->cfg.depth;
    D3dpWPrepTable tb{};
    tb.n = nl;
    for (int l = 0; l < nl; ++l) {
      const int blk = l >> 2, j = l & 3;
      const BlockDev& w = (blk & 1) ? c->tte[blk >> 1] : c->ste[blk >> 1];
      tb.it[l] = D3dpWPrepItem{lin_w(w, j), P.lin[j].N, P.lin[j].K, 2 * l + 1, 0, woff(l)};
    }
    return d3dp_launch_wprep(tb, ws + L.w_rows, ws + L.w_cols, amax(), uns(), st, P.rows_hi);
  }
  // out[T, N] = A2 . W2^T (+ bias) with T = 256 q + rem rows.  The persistent kernel works in rounds of n_cu tiles of 256 x 128;
  // the configs[4] batch has T = 16,524 = 64 x 256 + 140, so every forward / dgrad product had ONE row of tiles too many for
  // a whole number of rounds (fc2: 260 tiles on 256 CUs = two rounds for 1.02 rounds of work).  Where the remainder rows would cost
  // a round of their own the kernel takes them as 16 x 64 blocks spread over all workgroups (round 5; gemm_f16x2_dyn_kernel).
  // D3DP_TRAIN_TAIL=split, and contractions that are not a multiple of 16 k-steps, keep round 4's form: from 32 k-steps on a
  // second launch as a split-K product (Z chunks of the contraction: tn Z short work items instead of tn long ones) whose
  // partial sums are added in a fixed order, else the extra round.  (Which of the three: train_plan.h train_tail.)
  int gemm(TrainTail tail, const float* A2, const float* W2, const float* bias, const float* ua, const float* uw, float* out, int N,
           int K, unsigned* out_amax = nullptr, int amax_pos = 0) {
    Scope ps(pc, T_LINEAR, st);
    const int T = P.T, passes = P.passes;
    if (tail.form != TrainTailForm::SPLIT_REM)
      return d3dp_launch_linear_f16x2_dyn(A2, W2, bias, ua, uw, out, T, N, K, 1, st, out_amax, amax_pos,
                                          tail.form == TrainTailForm::REM_BLOCKS ? 1 : 0, passes, P.rows_hi);
    if (P.rows_hi) return -1;                            // (a superseded form: plan_context refuses it beside D3DP_TRAIN_ROWS=hi)
    const int q = T / 256, rem = T - q * 256;
    int r = d3dp_launch_linear_f16x2_dyn(A2, W2, bias, ua, uw, out, q * 256, N, K, 1, st, out_amax, amax_pos, 0, passes);
    if (r) return r;
    r = d3dp_launch_linear_f16x2_dyn(A2 + (size_t)q * 256 * K, W2, nullptr, ua, uw, ws + L.part_rem, rem, N, K, tail.Z, st, nullptr, 0, 0, passes);   // (a row = 2 K fp16 = K floats)
    if (r) return r;
    d3dp_launch_sum_partials_bias(ws + L.part_rem, bias, out + (size_t)q * 256 * N, (size_t)rem * N, N, tail.Z, st, out_amax, amax_pos);
    return 0;
  }
  // out[T, N] = A[T, K] W[N, K]^T + bias of Linear l = 4 blk + j (see the slots above).  Where its activation operand comes from
  // is the plan's TrainOperand:
  //   ROWS / ROWS_T  an operand pass over the fp32 rows A; the kernel that produced A already left its absmax in slot 2 l
  //                  (but the fp32-MFMA temporal attention in front of proj: TrainPlan::attn_t_f32_mfma)
  //   LN_INPUT       A is the INPUT of the LayerNorm whose output is this Linear's operand (norm1 in front of qkv, norm2 in front of
  //                  fc1), slot 2 l holds that output's absmax: the operand pass normalises on the fly, d3dp_launch_rowprep_ln
  //   PRODUCER       the operand -- planes at x_op(l), zero rows behind T, unscale slot 2 l -- was written by its producer; A is not read
  // The product's epilogue leaves the OUTPUT's absmax where a kernel behind it asks for one: qkv's in qkv_amax(blk), the largest
  // positive fc1 output in kPmaxSlot0 + blk where gelu_operand() follows.
  int forward(int blk, TrainLinearId j, const float* A, const BlockDev& w, float ln_eps, float* out) {
    const TrainLinear& p = P.lin[j];
    const int l = 4 * blk + j, sa = 2 * l, sw = 2 * l + 1, T = P.T, N = p.N, K = p.K;
    if (sw >= kBwdSlot0) return -1;
    const float* W = lin_w(w, j);
    const bool pmax = j == kFc1 && P.gelu_operand;
    unsigned* out_amax = j == kQkv ? qkv_amax(blk) : pmax ? amax() + kPmaxSlot0 + blk : nullptr;
    const TrainOperand src = P.source(blk, j);
    const float* a2 = x_op(l);
    if (P.rows_hi && (src == TrainOperand::ROWS_T || !P.batched)) return -1;   // (no hi-only form: plan_context lets no such shape through)
    if (src != TrainOperand::PRODUCER) {
      Scope ps(pc, T_OPERAND, st);
      if (j == kProj && (blk & 1) && P.attn_t_f32_mfma) d3dp_launch_absmax(A, (size_t)T * K, amax() + sa, st);
      // the operand of this product and, in the same pass, what the wgrad of this Linear will want of it: the backward pass
      // then neither recomputes this activation (LayerNorm / GELU outputs) nor reads it again.  Where the TN wgrad kernel applies
      // that is the SAME row form (kept, zero rows behind T), else a second, transposed form.
      const int Tp = p.pad_rows;
      int r;
      if (src == TrainOperand::LN_INPUT)
        r = d3dp_launch_rowprep_ln(A, j == kQkv ? w.n1w : w.n2w, j == kQkv ? w.n1b : w.n2b, ln_eps, x_op(l), T, Tp, K, amax() + sa, uns() + sa, st, P.rows_hi);
      else if (src == TrainOperand::ROWS)
        r = d3dp_launch_rowprep(A, x_op(l), nullptr, nullptr, T, Tp, K, amax() + sa, uns() + sa, st, nullptr, 0, 1, 1, nullptr, P.rows_hi);
      else {
        a2 = ws + o_a;
        r = d3dp_launch_dyprep(A, ws + o_a, x_op(l), nullptr, T, K, Tp, amax() + sa, uns() + sa, st);
      }
      if (r) return r;
    }
    const float* w2 = ws + L.op_w;
    if (P.batched) w2 = ws + L.w_rows + woff(l);
    else {
      Scope ps(pc, T_OPERAND, st);
      d3dp_launch_absmax(W, (size_t)N * K, amax() + sw, st);
      rows(W, N, K, ws + L.op_w, sw);
    }
    return gemm(p.fwd_tail, a2, w2, lin_b(w, j), uns() + sa, uns() + sw, out, N, K, out_amax, pmax ? 1 : 0);
  }
  // the fc2 operand of block blk from the fc1 output hpre (TrainPlan::gelu_operand)
  int gelu_operand(int blk, const float* hpre) {
    const int l = 4 * blk + kFc2;
    Scope ps(pc, T_OPERAND, st);
    return d3dp_launch_gelu_rowprep(hpre, x_op(l), P.T, P.lin[kFc2].pad_rows, P.lin[kFc2].K, amax() + kPmaxSlot0 + blk, amax() + 2 * l, uns() + 2 * l, st, P.rows_hi);
  }
  // dX[T, K] = dY[T, N] W[N, K] of Linear l = 4 blk + j   (sdy: the absmax slot of dY, shared with wgrad; always right behind the
  // wgrad of the same dY, whose prep_dy left the row form of dY in the current set)
  int dgrad(int blk, TrainLinearId j, int sdy, const float* W, float* dX, unsigned* out_amax = nullptr) {
    const TrainLinear& p = P.lin[j];
    const int l = 4 * blk + j, sw = 2 * l + 1;
    {
      Scope ps(pc, T_OPERAND, st);                     // (the profile counts this scope per dgrad, with or without a launch in it)
      if (!P.batched) cols(W, p.N, p.K, p.N, ws + L.op_w, sw);   // W^T: [K][2 N]  (N % 32 == 0: the model's widths)
    }
    const float* wt = ws + L.op_w;
    if (P.batched) wt = ws + L.w_cols + woff(l);       // (prepared by the forward pass of this step)
    return gemm(p.dgrad_tail, ws + o_a, wt, nullptr, uns() + sdy, uns() + sw, dX, p.K, p.N, out_amax);
  }
  // everything the backward pass of Linear j needs from its dY in one pass: row form -> op_a (dgrad), transposed form
  // -> op_at (wgrad, where the TN kernel does not apply), the bias gradient's partial column sums -> bias_part (*bias_rows rows of
  // N floats, at most TrainLayout::bias_rows).
  // (mask: the DropPath scales still to be applied to dY's rows -- TrainPlan::mip1 / mip2)
  // (gelu_pre: dY is d hidden and the Linear's dY is dY x gelu'(gelu_pre), formed by the operand pass; slot sdy then holds the
  //  absmax of d hidden -- TrainPlan::gip)
  int prep_dy(TrainLinearId j, const float* dY, int sdy, float* bias_part, int* bias_rows, const float* mask = nullptr, int axis = 0,
              int F = 1, int J = 1, const float* gelu_pre = nullptr) {
    const TrainLinear& p = P.lin[j];
    if (P.merged) {                  // the next region of the set: the block's four dY stay until flush_wgrads()
      if (set_used + L.Tp_max * (size_t)p.N > L.dy_set_floats) return -1;
      o_a = set_base + set_used;
      set_used += L.Tp_max * (size_t)p.N;
    }
    Scope ps(pc, T_OPERAND, st);
    if (p.tn)                        // the row form alone (zero rows behind T): dgrad's operand AND the TN wgrad's
      return d3dp_launch_rowprep(dY, ws + o_a, bias_part, bias_rows, P.T, p.pad_rows, p.N, amax() + sdy, uns() + sdy, st, mask, axis, F, J,
                                 gelu_pre, P.rows_hi);
    if (P.rows_hi) return -1;
    *bias_rows = D3DP_DYPREP_ROWS;
    return d3dp_launch_dyprep(dY, ws + o_a, ws + o_at, bias_part, P.T, p.N, p.pad_rows, amax() + sdy, uns() + sdy, st);
  }
  // dW[N, K] = dY[T, N]^T X[T, K] of Linear l = 4 blk + j   (dY: as prep_dy left it; X: the activation operand of forward Linear l,
  // left by the forward pass of this step)
  int wgrad(int blk, TrainLinearId j, int sdy, float* dW) {
    const TrainLinear& p = P.lin[j];
    const int l = 4 * blk + j, sx = 2 * l, N = p.N, K = p.K;
    if (P.merged) {                                    // recorded; launched with the block's other three by flush_wgrads()
      if (n_def >= D3DP_TN_MAX) return -1;
      size_t po = 0;
      for (int i = 0; i < n_def; ++i) po += (size_t)P.mZ * def[i].N * def[i].K;
      def[n_def] = D3dpTnProduct{ws + o_a, x_op(l), uns() + sdy, uns() + sx, ws + o_part + po, N, K, 0, 0};
      def_dw[n_def++] = dW;
      return 0;
    }
    int r;
    hipStream_t sw = st_w ? st_w : st;
    Scope ps(pc, T_WGRAD, sw);
    if (p.tn)                                          // both operands in their row forms [Tp][2 .]: nothing was transposed
      r = d3dp_launch_linear_f16x2_tn(ws + o_a, x_op(l), uns() + sdy, uns() + sx, ws + o_part, N, K, p.Tp, p.Z, sw, P.passes, P.rows_hi);
    else                                               // (the transposed form: left by prep_dy)
      r = d3dp_launch_linear_f16x2_dyn(ws + o_at, x_op(l), nullptr, uns() + sdy, uns() + sx, ws + o_part, N, K, p.Tp, p.Z, sw, nullptr, 0, 0, P.passes);
    if (r) return r;
    d3dp_launch_sum_partials(ws + o_part, dW, (size_t)N * K, p.Z, sw);
    return 0;
  }
};

}  // namespace

extern "C" {

int d3dp_train_workspace_bytes(const d3dp_ctx* c, int32_t B, size_t* bytes) {
  if (!c || !bytes || B < 1) return d3dp_fail(D3DP_EINVAL, "d3dp_train_workspace_bytes: bad argument");
  *bytes = train_layout(c->cfg, B).total_floats * 4;
  return D3DP_OK;
}

int d3dp_train_forward(d3dp_ctx* c, const float* x2d, const float* x3d, const int64_t* t, const float* masks, float* out,
                       int32_t B, void* workspace, size_t workspace_bytes, void* stream) {
  if (!c || !x2d || !x3d || !t || !out || !workspace || B < 1) return d3dp_fail(D3DP_EINVAL, "d3dp_train_forward: bad argument");
  if (!c->train()) return d3dp_fail(D3DP_ESTATE, "d3dp_train_forward needs a D3DP_MODE_TRAIN context");
  if (!c->weights_set) return d3dp_fail(D3DP_ESTATE, "weights not set");
  const d3dp_cfg& g = c->cfg;
  const TrainLayout L = train_layout(g, B);
  const TrainPlan P = plan_train_step(*c, g, B, c->n_cu);
  // clips longer than 256 frames (reference common/arguments.py:58, main.py:325 train at any `-f`): the split-fp16 attention kernels
  // pass their keys / queries through LDS in chunks (train_attn.hip: head dims 64, 32 and 16, and 24 / 40 / 48 / 56 at the widths
  // D3DP_TRAIN_IMPL=f16x2 opts in); the fp32 kernels hold whole sequences, and they are what head dim 8, a width on the fp32 path
  // and the cross-check switches run -- unless D3DP_TRAIN_LONG_ATTN=chunked (CtxPlan::train_long_attn) put their backward on the
  // chunked kernels (the forward side, d3dp_launch_attn_rows, passes K and V through LDS in chunks at every length)
  if (g.frames > 256 && !(P.path.attn_x2(0) && P.path.attn_x2(1)) && !P.attn_bwd_chunked)
    return d3dp_fail(D3DP_ENOTSUP, "frames=%d > 256: the training step runs such clips on its split-fp16 attention kernels only, which take "
                              "head dims 64, 32 and 16 -- 24, 40, 48 and 56 under D3DP_TRAIN_IMPL=f16x2 -- (channels=%d heads=%d is head dim %d) and are switched off by the cross-check "
                              "switches D3DP_TRAIN_IMPL=f32 and D3DP_TRAIN_ATTN=f32|x2t; the fp32 attention holds a whole sequence "
                              "in LDS (<= 256 frames)", g.frames, g.channels, g.heads, g.channels / g.heads);
  if (workspace_bytes < L.total_floats * 4) return d3dp_fail(D3DP_ESTATE, "train workspace too small");
  if (P.use_x2 && !P.rows_fit) return d3dp_fail(D3DP_EINVAL, "d3dp_train_forward: an operand's padded rows exceed the workspace's");
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const int T = P.T, C = g.channels, F = g.frames, J = g.joints, Hd = g.hidden;
  float *xn = ws + L.xn, *y = ws + L.y, *hid = ws + L.hid;
  d3dp_ctx* const pc = c->prof ? c : nullptr;
  std::optional<X2Train> x2s;
  if (P.use_x2) x2s.emplace(c, L, P, ws, st);
  X2Train* const x2 = P.use_x2 ? &*x2s : nullptr;
  if (x2) {
    Scope ps_(pc, T_OTHER, st);
    LAUNCH_TRY(x2->begin(true));
    LAUNCH_TRY(x2->prepare_weights(c));
  }
  // one of block blk's four Linears: src = the fp32 rows its operand pass reads -- its input, or where the plan says LN_INPUT the
  // input of the LayerNorm in front of it; not read where its producer wrote the operand -- and, on the fp32 path, its input
  auto lin = [&](int blk, TrainLinearId j, const float* src, float* out) -> int {
    const BlockDev& w = (blk & 1) ? c->tte[blk >> 1] : c->ste[blk >> 1];
    if (x2) return x2->forward(blk, j, src, w, g.eps_block, out);
    Scope ps_(pc, T_LINEAR, st);
    return lin32(src, lin_w(w, j), lin_b(w, j), out, T, P.lin[j].N, P.lin[j].K, st);
  };
  const bool ln_fused = P.ln_fused, ln_direct = P.ln_direct;
  TP(T_OTHER, d3dp_train_time_mlp(t, c->freq, c->t1w, c->t1b, c->t3w, c->t3b, ws + L.dtemb, ws + L.temb, B, C, st));   // (dtemb: free until the backward pass; needs B x 2 C)
  float* slab0 = ws + L.saved0;
  TP(T_LN_FWD, d3dp_launch_embed_ln(0, x2d, x3d, ws + L.temb, c->ew, c->eb, c->spos, c->ste[0].n1w, c->ste[0].n1b,
                                    g.eps_block, slab0 + L.o_xin, xn, 0, B, 1, F, J, C, st));
  // Every Linear's activation operand arrives with its absmax already in slot 2 l, left there by the kernel that produced it
  // (round 4 ran 64 absmax launches per step); the two exceptions are the first block's input, which the inference embedding
  // kernel writes, and the temporal attention's output (the fp32-MFMA kernel is shared with inference).
  auto slot = [&](int l) -> unsigned* { return x2 ? x2->amax() + 2 * l : nullptr; };
  if (x2) { Scope ps_(pc, T_OTHER, st); d3dp_launch_absmax(xn, (size_t)T * C, slot(0), st); }
  for (int blk = 0; blk < 2 * g.depth; ++blk) {
    const int kind = blk & 1, d = blk >> 1;
    const BlockDev& w = kind ? c->tte[d] : c->ste[d];
    float* S = ws + L.saved0 + (size_t)blk * L.saved_stride;
    const bool ax2 = P.path.attn_x2(kind);               // attention on split-fp16 operands (train_attn.hip)
    LAUNCH_TRY(lin(blk, kQkv, ln_fused ? S + L.o_xin : xn, S + L.o_qkv));
    const bool att_direct = P.att_direct(kind);
    void* att_op = att_direct ? x2->x_op(4 * blk + 1) : nullptr;
    const int att_tp = att_direct ? P.lin[kProj].pad_rows : 0;
    float* att_un = att_direct ? x2->uns() + 2 * (4 * blk + 1) : nullptr;
    const int n_seq = kind ? B * J : B * F;
    const SeqMap map = kind ? temporal_map(F, J) : spatial_map(F, J);
    auto attention = [&]() -> int {                      // (the launcher's own return code)
      if (ax2)
        return d3dp_train_attn_x2_fwd(S + L.o_qkv, S + L.o_att, ws + L.stats_x2 + (size_t)blk * L.stats_x2_stride, n_seq, map, C,
                                      g.heads, x2->qkv_amax(blk), slot(4 * blk + 1), st, att_op, T, att_tp, att_un, P.attn_passes, P.rows_hi);
      if (kind == 1 && P.attn_t_f32_mfma)                // temporal axis on the fp32 matrix cores (bitwise an fp32 fmaf chain per product)
        return d3dp_launch_attn_temporal_f32(0, S + L.o_qkv, S + L.o_att, n_seq, map, C, g.heads, st);
      return d3dp_launch_attn_rows(0, S + L.o_qkv, S + L.o_att, n_seq, map, C, g.heads, st, slot(4 * blk + 1));
    };
    TP(kind ? T_ATTN_FWD_T : T_ATTN_FWD_S, attention());
    LAUNCH_TRY(lin(blk, kProj, S + L.o_att, y));
    if (ln_direct)
      TP(T_LN_FWD, d3dp_train_add_mask_ln(S + L.o_xin, y, mask_ptr(masks, g, B, blk, 0), kind, F, J, w.n2w, w.n2b, g.eps_block,
                                          S + L.o_xmid, nullptr, slot(4 * blk + 2), T, C, st, x2->x_op(4 * blk + 2),
                                          P.lin[kFc1].pad_rows, x2->uns() + 2 * (4 * blk + 2), P.rows_hi))
    else
      TP(T_LN_FWD, d3dp_train_add_mask_ln(S + L.o_xin, y, mask_ptr(masks, g, B, blk, 0), kind, F, J, w.n2w, w.n2b, g.eps_block,
                                          S + L.o_xmid, ln_fused ? nullptr : xn, slot(4 * blk + 2), T, C, st));
    LAUNCH_TRY(lin(blk, kFc1, ln_fused ? S + L.o_xmid : xn, S + L.o_hpre));
    if (P.gelu_operand) {
      // the fc2 operand = split(GELU(fc1 output)) in one pass, its scale from the largest positive fc1 output (the fc1
      // epilogue leaves it): no fp32 hidden tensor, no separate operand pass
      LAUNCH_TRY(x2->gelu_operand(blk, S + L.o_hpre));
      LAUNCH_TRY(lin(blk, kFc2, nullptr, y));
    } else {
      TP(T_OPERAND, d3dp_train_gelu_fwd(S + L.o_hpre, hid, (size_t)T * Hd, slot(4 * blk + 3), st));
      LAUNCH_TRY(lin(blk, kFc2, hid, y));
    }
    // the block's end in one pass: residual add, the shared norm (+ Temporal_pos_embed after the first spatial block,
    // mixste.py:250) -> the next block's input, that block's norm1 -> its qkv operand (after the last block: the head's
    // LayerNorm -> z)
    const bool last = blk == 2 * g.depth - 1;
    float* x_next = last ? ws + L.x_final : S + L.saved_stride + L.o_xin;
    const float *nw = c->hnw, *nb = c->hnb;
    if (!last) { const BlockDev& wn = kind ? c->ste[d + 1] : c->tte[d]; nw = wn.n1w; nb = wn.n1b; }
    TP(T_LN_FWD, d3dp_train_add_mask_ln2(S + L.o_xmid, y, mask_ptr(masks, g, B, blk, 1), kind, F, J, kind ? c->tnw : c->snw,
                                         kind ? c->tnb : c->snb, g.eps_block, (kind == 0 && d == 0) ? c->tpos : nullptr, nw, nb,
                                         last ? g.eps_head : g.eps_block, S + L.o_xout, x_next,
                                         last ? ws + L.z : (ln_fused ? nullptr : xn), last ? nullptr : slot(4 * (blk + 1)), T, C, st,
                                         (ln_direct && !last) ? x2->x_op(4 * (blk + 1)) : nullptr,
                                         (ln_direct && !last) ? P.lin[kQkv].pad_rows : 0,
                                         (ln_direct && !last) ? x2->uns() + 2 * 4 * (blk + 1) : nullptr, P.rows_hi));
  }
  TP(T_OTHER, d3dp_train_head_linear(ws + L.z, c->hw, c->hb, out, T, C, st));
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

// grads: device fp32 buffers with the shapes of the corresponding weights (time_freq ignored); they are ZEROED here
// and then accumulated.  Must be called after d3dp_train_forward with the same inputs, masks and workspace.
int d3dp_train_backward(d3dp_ctx* c, const float* x2d, const float* x3d, const int64_t* t, const float* masks,
                        const float* grad_out, const d3dp_weights* grads, int32_t B, void* workspace,
                        size_t workspace_bytes, void* stream) {
  if (!c || !x2d || !x3d || !t || !grad_out || !grads || !grads->ste || !grads->tte || !workspace || B < 1)
    return d3dp_fail(D3DP_EINVAL, "d3dp_train_backward: bad argument");
  if (!c->train()) return d3dp_fail(D3DP_ESTATE, "d3dp_train_backward needs a D3DP_MODE_TRAIN context");
  const d3dp_cfg& g = c->cfg;
  const TrainLayout L = train_layout(g, B);
  const TrainPlan P = plan_train_step(*c, g, B, c->n_cu);   // (as the forward pass of this step: the operands it left are the plan's)
  if (workspace_bytes < L.total_floats * 4) return d3dp_fail(D3DP_ESTATE, "train workspace too small");
  if (P.use_x2 && !(P.rows_fit && P.parts_fit))
    return d3dp_fail(D3DP_EINVAL, "d3dp_train_backward: an operand's padded rows or a weight gradient's partial products exceed the workspace's");
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const int T = P.T, Tp = (int)L.Tpad, C = g.channels, F = g.frames, J = g.joints, Hd = g.hidden;
  auto G = [](const float* p) { return const_cast<float*>(p); };
  // (one launch for the few gradient buffers that are still ACCUMULATED into -- the time MLP's; everything else is written:
  //  weight matrices by their wgrad product, every other gradient by the fixed-order reduction at the end of this function)
  D3dpZeroTable ztab{};
  auto zero = [&](const float* p, size_t n) -> hipError_t {
    if (ztab.count < D3DP_ZERO_MAX && n < ((size_t)1 << 32)) {
      ztab.p[ztab.count] = G(p); ztab.n[ztab.count] = (unsigned)n; ++ztab.count;
      return hipSuccess;
    }
    return hipMemsetAsync(G(p), 0, n * 4, st);
  };
  const size_t CC = (size_t)C * C;
  HIP_TRY(zero(grads->time1_w, 2 * CC)); HIP_TRY(zero(grads->time1_b, 2 * C));
  HIP_TRY(zero(grads->time3_w, 2 * CC)); HIP_TRY(zero(grads->time3_b, C));
  d3dp_ctx* const pc = c->prof ? c : nullptr;
  if (ztab.count) TP(T_OTHER, d3dp_train_zero_many(ztab, st));
  float *xn = ws + L.xn, *hid = ws + L.hid, *dA = ws + L.dA, *dB = ws + L.dB, *dC = ws + L.dC, *dqkv = ws + L.dqkv,
        *dh = ws + L.dh, *At = ws + L.At, *Xt = ws + L.Xt, *Wt = ws + L.Wt;

  std::optional<X2Train> x2s;
  if (P.use_x2) x2s.emplace(c, L, P, ws, st);
  X2Train* const x2 = P.use_x2 ? &*x2s : nullptr;
  if (x2) TP(T_OTHER, x2->begin(false));
  // second stream for the weight-gradient products (see d3dp_ctx::aux)
  // (under the per-kernel profile everything runs on the caller's stream: a class's time must not contain a wait for CUs that a
  //  product on the second stream holds -- same arithmetic, test_training_step_stream_switches_change_no_bit)
  const bool overlap = P.path.needs_aux && !c->prof;
  if (overlap && !c->aux) return d3dp_fail(D3DP_ESTATE, "d3dp_train_backward: the second stream was not created (d3dp_create makes it)");
  // Up to two weight-gradient products are in flight on c->aux, each with its own operand / partial-tile set (X2Train::use_set):
  // product k takes set k & 1 and the caller's stream waits for product k - 2 before the operand pass overwrites that set -- not
  // for product k - 1, which goes on beside the dgrad product and the row kernels of this dY.  D3DP_TRAIN_OVERLAP=1: one set,
  // every operand pass waits for the product before it (the first form of this overlap).
  bool pending[2] = {false, false};
  int n_wgrad = 0, cur_set = 0;
  const int n_sets = P.overlap_sets;
  auto wait_set = [&](int s) -> int {                    // the caller's stream waits for the product that last used set s
    if (!pending[s]) return 0;
    pending[s] = false;
    return hipStreamWaitEvent(st, c->ev_done[s], 0) == hipSuccess ? 0 : -3;
  };
  auto join = [&]() -> int { int r = wait_set(0); return r ? r : wait_set(1); };
  Reducer red{ws + L.red, L.red_floats, 0, st};
  red.items.reserve(24 * (size_t)g.depth + 32);
  const int lnrows = L.ln_rows;                          // partial rows one LayerNorm-backward call leaves
  // [dgamma | dbeta] partial rows of a LayerNorm with `calls` backward calls per step (the shared norms: one per depth), and
  // their two destinations; call i writes rows [i lnrows, (i + 1) lnrows)
  auto ln_part = [&](const float* dgamma, const float* dbeta, int calls) -> float* {
    float* p = red.take((size_t)calls * lnrows * 2 * C);
    if (p) {
      red.add(p, G(dgamma), C, (size_t)calls * lnrows, 2 * (size_t)C);
      red.add(p + C, G(dbeta), C, (size_t)calls * lnrows, 2 * (size_t)C);
    }
    return p;
  };
  float* part_sn = ln_part(grads->spatial_norm_w, grads->spatial_norm_b, g.depth);
  float* part_tn = ln_part(grads->temporal_norm_w, grads->temporal_norm_b, g.depth);
  float* part_hn = ln_part(grads->head_norm_w, grads->head_norm_b, 1);
  if (red.rc) return d3dp_fail(D3DP_ESTATE, "d3dp_train_backward: partial-sum region too small");
  int sdy = -1;                                          // absmax slot of the dY the next wgrad / dgrad pair shares
  // wgrad of Linear l = 4 blk + j: dW[N, K] = dY[T, N]^T X[T, K]  (fp32 path: both operands transposed to [*, Tpad], zero padded;
  //  split-fp16 path: X's operand form was left by the forward pass of this step and X is not read)
  // (dbias: the Linear's bias gradient = column sums of dY, left as partial rows and summed at the end)
  // (pre_slot >= 0: the kernel that produced dY left its absmax there)
  // (mk / mk_axis: DropPath scales the operand pass still has to apply to dY's rows -- then dY is the UNSCALED gradient)
  // (gelu_pre: dY is d hidden, the Linear's dY is dY x gelu'(gelu_pre) and pre_slot holds the absmax of d hidden: split-fp16 path)
  auto wgrad = [&](int blk, TrainLinearId j, const float* dY, const float* X, float* dW, float* dbias, int pre_slot = -1,
                   const float* mk = nullptr, int mk_axis = 0, const float* gelu_pre = nullptr) -> int {
    const int N = P.lin[j].N, K = P.lin[j].K;
    int r;
    if (x2) {
      sdy = pre_slot >= 0 ? pre_slot : x2->slot_for(dY, (size_t)T * N);
      if (sdy < 0) return -1;
      float* bp = red.take((size_t)L.bias_rows * N);
      int brows = 0;
      if (!bp) return -1;
      // merged (one launch per block): fc2, fc1, proj, qkv arrive in this order, the set changes with the block and the
      // products are launched behind the last dY; else every weight gradient is a product, and takes a set, of its own
      const bool first = !P.merged || j == kFc2, last = !P.merged || j == kQkv;
      if (first) {
        cur_set = overlap ? (n_wgrad++ % n_sets) : 0;
        if ((r = wait_set(cur_set))) return r;           // the product that last used this set is done with its operands and partial tiles
        x2->use_set(cur_set);
      }
      if ((r = x2->prep_dy(j, dY, sdy, bp, &brows, mk, mk_axis, F, J, gelu_pre))) return r;
      red.add(bp, dbias, N, brows, N);
      if (last && overlap) {
        if (hipEventRecord(c->ev_fork, st) != hipSuccess || hipStreamWaitEvent(c->aux, c->ev_fork, 0) != hipSuccess) return -3;
        x2->st_w = c->aux;
      }
      if ((r = x2->wgrad(blk, j, sdy, dW))) return r;        // (merged: recorded)
      if (last && P.merged && (r = x2->flush_wgrads())) return r;
      if (last && overlap) {
        if (hipEventRecord(c->ev_done[cur_set], c->aux) != hipSuccess) return -3;
        pending[cur_set] = true;
      }
      return 0;
    }
    float* bp = red.take((size_t)D3DP_DYPREP_ROWS * N);
    int rows = 0;
    if (!bp || mk || gelu_pre) return -1;
    {
      Scope ps_(pc, T_OPERAND, st);
      if ((r = d3dp_train_colsum(dY, bp, &rows, D3DP_DYPREP_ROWS, T, N, st))) return r;
      red.add(bp, dbias, N, rows, N);
      if ((r = d3dp_train_transpose_pad(dY, At, T, N, Tp, st))) return r;
      if ((r = d3dp_train_transpose_pad(X, Xt, T, K, Tp, st))) return r;
    }
    Scope ps_(pc, T_WGRAD, st);
    // contraction over tokens: split-K, the chunks' partial products added in a fixed order (no float atomics: this path's gradients
    // are bit-reproducible too)
    return d3dp_launch_linear_f32_splitk(At, Xt, dW, N, K, Tp, st, ws + L.part, L.part_floats);
  };
  // dgrad of Linear l = 4 blk + j: dX[T, K] = dY[T, N] W[N, K]   (fp32 path: W transposed to [K, N]; no bias: a null one is zeros)
  auto dgrad = [&](int blk, TrainLinearId j, const float* dY, float* dX, unsigned* out_amax = nullptr) -> int {
    const BlockDev& w = (blk & 1) ? c->tte[blk >> 1] : c->ste[blk >> 1];
    const int N = P.lin[j].N, K = P.lin[j].K;
    if (x2) return sdy < 0 ? -1 : x2->dgrad(blk, j, sdy, lin_w(w, j), dX, out_amax);  // (always right behind the wgrad of the same dY)
    int r;
    { Scope ps_(pc, T_OPERAND, st); if ((r = d3dp_train_transpose_pad(lin_w(w, j), Wt, N, K, N, st))) return r; }
    Scope ps_(pc, T_LINEAR, st);
    return lin32(dY, Wt, nullptr, dX, T, K, N, st);
  };
  // a slot for the absmax the producer of the next dY leaves (split-fp16 path only)
  auto fresh = [&](int& slot) -> unsigned* {
    slot = x2 ? x2->take() : -1;
    return slot >= 0 ? x2->amax() + slot : nullptr;
  };
#define D3DP_FRESH(ps, pa)                                                                              \
  int ps = -1;                                                                                          \
  unsigned* pa = fresh(ps);                                                                             \
  if (x2 && ps < 0) return d3dp_fail(D3DP_ESTATE, "d3dp_train_backward: out of operand slots");

  // ---- head: Linear(C, 3) backward, then its LayerNorm and the last block's shared norm in one pass --------------
  const int nblk = 2 * g.depth;
  {
    float* hp = red.take((size_t)L.head_rows * (3 * C + 4));
    int rows = 0;
    if (!hp) return d3dp_fail(D3DP_ESTATE, "d3dp_train_backward: partial-sum region too small");
    TP(T_OTHER, d3dp_train_head_bwd(grad_out, ws + L.z, c->hw, dC, hp, &rows, T, C, st));   // (z: left by the forward pass)
    red.add(hp, G(grads->head_w), 3 * (size_t)C, rows, 3 * (size_t)C + 4);
    red.add(hp + 3 * C, G(grads->head_b), 3, rows, 3 * (size_t)C + 4);
  }
  // dB = d x_out of the last block; its DropPath-scaled form (the fc2 dY) in dC with its absmax in slot ps
  const float* dy = nullptr;                             // the dY of the branch about to be differentiated
  const float* dy_mask = nullptr;                        // ... and the DropPath scales its operand pass still has to apply
  int ps_next = -1;
  // (the DropPath-scaled gradient is not stored where the operand pass can apply the scales itself: only its absmax is)
  const bool mip2 = P.mip2, mip1 = P.mip1, gip = P.gip;
  {
    const int lb = nblk - 1, lk = lb & 1;
    const float* S = ws + L.saved0 + (size_t)lb * L.saved_stride;
    const float* mk = mask_ptr(masks, g, B, lb, 1);
    D3DP_FRESH(ps, pa)
    TP(T_LN_BWD, d3dp_train_ln_bwd(dC, ws + L.x_final, c->hnw, g.eps_head, nullptr, nullptr, S + L.o_xout, lk ? c->tnw : c->snw,
                                 g.eps_block, dB, mk, lk, F, J, (mk && !mip2) ? dC : nullptr, pa, part_hn,
                                 (lk ? part_tn : part_sn) + (size_t)(lb >> 1) * lnrows * 2 * C, T, C, st));
    dy = (mk && !mip2) ? dC : dB;
    dy_mask = mip2 ? mk : nullptr;
    ps_next = ps;
  }
  for (int blk = nblk - 1; blk >= 0; --blk) {
    const int kind = blk & 1, d = blk >> 1;
    const BlockDev& w = kind ? c->tte[d] : c->ste[d];
    const d3dp_block_weights& gw = (kind ? grads->tte : grads->ste)[d];
    float* S = ws + L.saved0 + (size_t)blk * L.saved_stride;
    // here: dB = d x_out(blk), dy = its DropPath-scaled form, absmax in slot ps_next
    // ---- MLP branch ----
    if (!x2) TP(T_OPERAND, d3dp_train_gelu_fwd(S + L.o_hpre, hid, (size_t)T * Hd, nullptr, st));   // (x2: wgrad reads the forward pass' operand)
    LAUNCH_TRY(wgrad(blk, kFc2, dy, hid, G(gw.fc2_w), G(gw.fc2_b), ps_next, dy_mask, kind));
    {
      // d hidden = dy W_fc2; d h_pre = d hidden x gelu'(h_pre).  Split-fp16 path (TrainPlan::gip): the product is formed by the operand
      // pass of the fc1 gradients (the only reader of d h_pre), from the absmax of d hidden the fc2 dgrad's epilogue leaves
      D3DP_FRESH(ps, pa)
      LAUNCH_TRY(dgrad(blk, kFc2, dy, dh, gip ? pa : nullptr));                                                         // d hidden
      if (!gip) TP(T_OPERAND, d3dp_train_gelu_bwd(dh, S + L.o_hpre, dh, (size_t)T * Hd, pa, st));             // d h_pre
      if (!x2) TP(T_LN_FWD, d3dp_train_ln_pos(S + L.o_xmid, w.n2w, w.n2b, g.eps_block, nullptr, F, J, xn, T, C, st));   // xn2
      LAUNCH_TRY(wgrad(blk, kFc1, dh, xn, G(gw.fc1_w), G(gw.fc1_b), ps, nullptr, 0, gip ? S + L.o_hpre : nullptr));
      LAUNCH_TRY(dgrad(blk, kFc1, dh, dC));                                                                             // d xn2
    }
    // norm2 backward + the residual: dA = d x_mid; its DropPath-scaled form (the proj dY) over dC
    {
      const float* mk = mask_ptr(masks, g, B, blk, 0);
      float* pn = ln_part(gw.norm2_w, gw.norm2_b, 1);
      D3DP_FRESH(ps, pa)
      if (!pn) return d3dp_fail(D3DP_ESTATE, "d3dp_train_backward: partial-sum region too small");
      TP(T_LN_BWD, d3dp_train_ln_bwd(dC, S + L.o_xmid, w.n2w, g.eps_block, dB, nullptr, nullptr, nullptr, 0.f, dA, mk, kind, F, J,
                                   (mk && !mip1) ? dC : nullptr, pa, pn, nullptr, T, C, st));
      dy = (mk && !mip1) ? dC : dA;
      // ---- attention branch ----
      LAUNCH_TRY(wgrad(blk, kProj, dy, S + L.o_att, G(gw.proj_w), G(gw.proj_b), ps, mip1 ? mk : nullptr, kind));
    }
    int ps_dqkv = -1;
    if (P.path.attn_x2(kind)) {
      // split-fp16 operands: the proj dgrad leaves d att's absmax, the attention backward that of dqkv
      D3DP_FRESH(pdo, pado)
      D3DP_FRESH(pq, paq)
      LAUNCH_TRY(dgrad(blk, kProj, dy, dB, pado));                                                                      // d att
      // (the per-kernel profile times the two passes apart; otherwise one call launches both)
      for (int part = pc ? 1 : 0; part <= (pc ? 2 : 0); ++part)
        TP(part == 2 ? (kind ? T_ATTN_BKV_T : T_ATTN_BKV_S) : (kind ? T_ATTN_BQ_T : T_ATTN_BQ_S),
           d3dp_train_attn_x2_bwd(S + L.o_qkv, S + L.o_att, dB, dqkv, ws + L.stats_x2 + (size_t)blk * L.stats_x2_stride,
                                  kind ? B * J : B * F, kind ? temporal_map(F, J) : spatial_map(F, J), C, g.heads,
                                  x2->qkv_amax(blk), pado, paq, st, part, P.attn_passes));
      ps_dqkv = pq;
    } else {
      LAUNCH_TRY(dgrad(blk, kProj, dy, dB));                                                                            // d att
      // (fp32 kernels: both passes behind one launcher -- timed together under the pass-Q class)
      TP(kind ? T_ATTN_BQ_T : T_ATTN_BQ_S, d3dp_train_attn_bwd(S + L.o_qkv, S + L.o_att, dB, dqkv, ws + L.stats, kind ? B * J : B * F,
                                                             kind ? temporal_map(F, J) : spatial_map(F, J), C, g.heads, st,
                                                             P.attn_bwd_chunked));
    }
    if (!x2) TP(T_LN_FWD, d3dp_train_ln_pos(S + L.o_xin, w.n1w, w.n1b, g.eps_block, nullptr, F, J, xn, T, C, st));    // xn1
    LAUNCH_TRY(wgrad(blk, kQkv, dqkv, xn, G(gw.qkv_w), G(gw.qkv_b), ps_dqkv));
    LAUNCH_TRY(dgrad(blk, kQkv, dqkv, dC));                                                                         // d xn1
    float* pn1 = ln_part(gw.norm1_w, gw.norm1_b, 1);
    if (!pn1) return d3dp_fail(D3DP_ESTATE, "d3dp_train_backward: partial-sum region too small");
    if (blk > 0) {
      // norm1 backward + the residual (= d x_in of this block = d of the previous block's shared-norm output), then that
      // shared norm's backward, in one pass: dB = d x_out(blk - 1) and its DropPath-scaled form over dC
      const int pb = blk - 1, pk = pb & 1;
      const float* Sp = ws + L.saved0 + (size_t)pb * L.saved_stride;
      const float* mk = mask_ptr(masks, g, B, pb, 1);
      float* g_out = pb == 0 ? ws + L.y : nullptr;       // d of Temporal_pos_embed's sum (added behind block 0's shared norm); y: a forward
                                                         // temporary -- NOT z, which a second backward over the same forward reads again
      D3DP_FRESH(ps, pa)
      TP(T_LN_BWD, d3dp_train_ln_bwd(dC, S + L.o_xin, w.n1w, g.eps_block, dA, g_out, Sp + L.o_xout, pk ? c->tnw : c->snw, g.eps_block,
                                   dB, mk, pk, F, J, (mk && !mip2) ? dC : nullptr, pa, pn1,
                                   (pk ? part_tn : part_sn) + (size_t)(pb >> 1) * lnrows * 2 * C, T, C, st));
      if (g_out) TP(T_OTHER, d3dp_train_groupsum(g_out, G(grads->temporal_pos), T, C, 1, F, J, 1, st));
      dy = (mk && !mip2) ? dC : dB;
      dy_mask = mip2 ? mk : nullptr;
      ps_next = ps;
    } else {
      TP(T_LN_BWD, d3dp_train_ln_bwd(dC, S + L.o_xin, w.n1w, g.eps_block, dA, nullptr, nullptr, nullptr, 0.f, dB, nullptr, 0, F, J,
                                   nullptr, nullptr, pn1, nullptr, T, C, st));
    }
  }
#undef D3DP_FRESH
  LAUNCH_TRY(join());                                    // every weight gradient is on the caller's stream's timeline again
  // ---- embedding, position and time embeddings (dB = d of the embedded tokens) ------------------------------------
  {
    Scope ps_(pc, T_OTHER, st);
    float* ep = red.take((size_t)D3DP_EMBED_BWD_ROWS * 5 * C);
    float* bp = red.take((size_t)L.embed_bias_rows * C);
    float* sp = red.take((size_t)L.group_slices * J * C);
    float* tp = red.take((size_t)L.group_slices * B * C);
    int rows = 0;
    if (!ep || !bp || !sp || !tp) return d3dp_fail(D3DP_ESTATE, "d3dp_train_backward: partial-sum region too small");
    LAUNCH_TRY(d3dp_train_embed_bwd(dB, x2d, x3d, ep, T, C, st));
    red.add(ep, G(grads->embed_w), 5 * (size_t)C, D3DP_EMBED_BWD_ROWS, 5 * (size_t)C);
    LAUNCH_TRY(d3dp_train_colsum(dB, bp, &rows, L.embed_bias_rows, T, C, st));
    red.add(bp, G(grads->embed_b), C, rows, C);
    LAUNCH_TRY(d3dp_train_groupsum(dB, sp, T, C, 0, F, J, L.group_slices, st));
    red.add(sp, G(grads->spatial_pos), (size_t)J * C, L.group_slices, (size_t)J * C);
    LAUNCH_TRY(d3dp_train_groupsum(dB, tp, T, C, 2, F, J, L.group_slices, st));
    red.add(tp, ws + L.dtemb, (size_t)B * C, L.group_slices, (size_t)B * C);
    red.flush();                                          // (dtemb feeds the time MLP's backward below)
  }
  if (red.rc) return d3dp_fail(D3DP_EHIP, "d3dp_train_backward: the gradient reduction failed");
  TP(T_OTHER, d3dp_train_time_mlp_bwd(t, c->freq, c->t1w, c->t1b, c->t3w, ws + L.dtemb, G(grads->time1_w),
                                      G(grads->time1_b), G(grads->time3_w), G(grads->time3_b), B, C, st));
  // (profile only) eight empty scopes on the still-busy stream: the time an event pair adds to every launch it brackets --
  // event-to-event durations of 15 - 80 us kernels are not kernel durations without it (bench.py subtracts the average)
  for (int i = 0; pc && i < 8; ++i) { Scope ps_(pc, P_EMPTY, st); }
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

}  // extern "C"
#undef TP
