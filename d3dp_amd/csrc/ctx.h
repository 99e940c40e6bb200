// Host-side types shared by the C-ABI translation units (capi.hip, capi_weights.hip, capi_denoise.hip, capi_ops.hip,
// capi_train.hip): the context -- the plan of its creation (ctx_plan.h), what d3dp_set_weights and the calls change later and the
// predicates derived from both --, a block's device weights, the profile scope and the token maps of the two attention axes.
// (The route and the workspace layout of a training step: train_plan.h, which kernels.h brings in.)
// Internal: nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "common.h"
#include "ctx_plan.h"
#include "kernels.h"

#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t e__ = (expr);                                                               \
    if (e__ != hipSuccess) return d3dp_fail(D3DP_EHIP, "%s: %s", #expr, hipGetErrorString(e__)); \
  } while (0)

#define LAUNCH_TRY(expr)                                                          \
  do {                                                                            \
    int r__ = (expr);                                                             \
    if (r__ != 0) return d3dp_fail(r__ == -1 ? D3DP_EINVAL : D3DP_ENOTSUP, "%s -> %d", #expr, r__); \
  } while (0)

enum ProfClass { P_QKV = 0, P_PROJ, P_FC1, P_FC2, P_ATTN_S, P_ATTN_T, P_LN, P_LN2, P_EMBED, P_HEAD, P_TIME, P_OTHER,
                 // the training step (d3dp_train_forward / d3dp_train_backward)
                 T_LINEAR, T_WGRAD, T_ATTN_FWD_S, T_ATTN_FWD_T, T_ATTN_BQ_S, T_ATTN_BQ_T, T_ATTN_BKV_S, T_ATTN_BKV_T, T_OPERAND,
                 T_LN_FWD, T_LN_BWD, T_OTHER,
                 P_EMPTY };                            // event pairs with nothing between them: what a scope adds to a launch's time
static_assert(P_EMPTY + 1 == D3DP_PROFILE_CLASSES, "include/d3dp_hip.h: D3DP_PROFILE_CLASSES");

struct BlockDev {
  const float *n1w, *n1b, *n2w, *n2b, *qkv_b, *proj_b, *fc1_b, *fc2_b;
  const void *qkv_w, *proj_w, *fc1_w, *fc2_w;   // bf16 (FAST) or fp16 (FAST16); EXACT: 2 fp16 planes (default), 3 bf16 planes or fp32
  float qkv_u = 1.f, proj_u = 1.f, fc1_u = 1.f, fc2_u = 1.f;   // EXACT f16x2: 2^-s of the per-matrix pre-scale 2^s
  const float* fc1_c12 = nullptr;   // fold_ln: [c2 | c1] of norm2 folded into fc1 (fc1_w then holds W diag(gamma)); see run_block
  // EXACT f16x2: the power-of-two scales of this block's DATA-dependent split-fp16 operands -- q / k / v and the attention
  // output (s_kv), the MLP hidden (s_h) -- chosen at d3dp_set_weights from the range the weights PROVE for them: 2^4 when
  // the bound is below 4094, the largest smaller power of two that keeps bound x scale below fp16's 65504 otherwise
  // (LayerNorm outputs always use 2^4: their bound is sqrt(C-1) |gamma| + |beta|).
  float s_kv = kActScale, s_h = kActScale;
  const float* proj_bgb = nullptr;  // defer_norm: [proj_b | gamma | beta] of the shared norm in FRONT of the block (EPI_RESID_NORM)
  // FAST16 under D3DP_FAST16_RANGE=scale (d3dp_ctx::fast16_scale): the exponents s of the power-of-two multipliers 2^-s at which this
  // block's four classes of fp16 tensors are stored -- q / k / v and the attention output (r_qkv, from b_qkv), the proj output
  // (r_proj, from b_proj), the MLP hidden and the pre-activation parked in front of the GELU (r_h, from b_h), the fc2 output (r_fc2,
  // from b_fc2) -- each the smallest s >= 0 with bound x 2^-s < 65504, chosen at d3dp_set_weights (at most kFast16MaxShift, or the
  // context falls back to bf16).  All 0 in every other context, and wherever the bound is below 65504: the plain kernels.
  int r_qkv = 0, r_proj = 0, r_h = 0, r_fc2 = 0;
};
// The largest exponent D3DP_FAST16_RANGE=scale takes.  An fp16 emulation on a CPU that stores all four classes of EVERY block at
// 2^-s stays within 1.17x of the unscaled emulation's distance to the fp32 oracle for every s <= 12 and is 2.2 - 2.6x away at s = 14
// (what 2^-s pushes into fp16's subnormal range is, up to there, far below the rounding of the large values it is added to); 8
// leaves 2^4 of that (profiles/fast16_scaled.md)
constexpr int kFast16MaxShift = 8;

constexpr size_t kAlign = 256;
inline size_t align_up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

// Which attention kernel family a context launches on an axis (0 = spatial, 1 = temporal): attn_route(), capi_denoise.hip
enum class AttnRoute { X2, FAST_SPATIAL, FAST_WHOLE_SEQ, F32_TEMPORAL, ROWS };
AttnRoute attn_route(int mode, int exact_impl, int hd, int frames, int joints, bool long_rows, int axis);

// The members d3dp_create decides are the base (CtxPlan); the ones below it change later: d3dp_set_weights (exact_impl, impl_fallback,
// fast_f16, fast_bound, the weights), the profile calls and the pass plan.
struct d3dp_ctx : CtxPlan {
  d3dp_cfg cfg{};
  int device = 0;
  bool weights_set = false;
  float range_bound = 0.f;       // d3dp_exact_range_bound (EXACT split-fp16 only)
  unsigned* d_flag = nullptr;    // device word: bit 0 = a d3dp_denoise output held inf / nan (d3dp_status)
  char* arena = nullptr;
  size_t arena_bytes = 0;
  const float *spos = nullptr, *tpos = nullptr, *ew = nullptr, *eb = nullptr, *freq = nullptr, *t1w = nullptr,
              *t1b = nullptr, *t3w = nullptr, *t3b = nullptr, *snw = nullptr, *snb = nullptr, *tnw = nullptr,
              *tnb = nullptr, *hnw = nullptr, *hnb = nullptr, *hw = nullptr, *hb = nullptr;
  std::vector<BlockDev> ste, tte;
  // profiling
  bool prof = false;
  struct Ev { hipEvent_t a, b; int cls; };
  std::vector<Ev> pool;
  size_t used = 0;
  int64_t counts[D3DP_PROFILE_CLASSES] = {0};
  double total_ms[D3DP_PROFILE_CLASSES] = {0};

  // FAST and FAST16 contexts are one dataflow (2-byte operands and branch outputs, fp32 residual stream, the streaming Linear
  // and the MFMA attention kernels) in two element types.  fast_f16: the type this context's kernels are instantiated for --
  // a FAST16 context has it set by d3dp_set_weights when the weights prove that no stored value can reach fp16's 65504
  // (fast_bound) and runs the bf16 kernels otherwise; a plain FAST context proves nothing and is bf16 (the `make fastf16`
  // library: fp16, D3DP_FAST_F16).
  bool fast16() const { return cfg.mode == D3DP_MODE_FAST16; }
  bool fast() const { return cfg.mode == D3DP_MODE_FAST || fast16(); }
  int fast_f16 = 0;
  float fast_bound = 0.f;
  // EXACT mode runs its Linears on split-fp16 operands (2 planes, 3 fp16-MFMA passes, gemm_x2.hip); activations that
  // feed a Linear are then two fp16 planes.  env D3DP_EXACT_IMPL=bf16x3 selects the round-1 six-pass split-bf16 kernels
  // and =f32 the plain fp32-MFMA kernels (bitwise an fp32 fmaf chain) -- both kept as cross-checks.
  int exact_impl = 0;            // 0 = f16x2, 1 = bf16x3, 2 = f32.  Starts as exact_impl_req; d3dp_set_weights moves an f16x2 context to
  bool impl_fallback = false;    // bf16x3 when LayerNorm's own output bound leaves the split-fp16 range (see there; with padded heads: to f32)
  bool train() const { return cfg.mode == D3DP_MODE_TRAIN; }
  bool exact() const { return !fast() && !train(); }
  bool x2() const { return exact() && exact_impl == 0; }
  // The split-fp16 attention kernels run (attn_route(): the same answer on both axes).  Everything that follows from the packed
  // qkv rows follows x2_attn(): EPI_QKV_PACK in linear(), the scale of the attention output planes in run_block, seq_pitch(), and
  // the range fallback of d3dp_set_weights, which lowers s_kv instead of leaving the split-fp16 implementation wherever these
  // kernels run.  cp(): the columns of a qkv third, padded heads (CtxPlan::hdp) included.
  int cp() const { return hdp ? cfg.heads * hdp : cfg.channels; }
  // (the columns of a packed qkv third / of the attention output while the split-fp16 implementation runs; the range fallback of
  //  a padded context is the fp32 implementation, which knows no padding)
  int attn_cols() const { return hdp && (fast() || exact_impl == 0) ? cp() : cfg.channels; }
  AttnRoute route(int axis) const {
    return attn_route(cfg.mode, exact_impl, attn_cols() / cfg.heads, cfg.frames, cfg.joints, long_rows, axis);
  }
  bool x2_attn() const { return route(0) == AttnRoute::X2; }
  // proj / fc2 add into the residual stream in their epilogue (x += ...), so the row kernels read x alone
  bool fold_resid() const { return x2() && fold; }
  // norm2 (mixste.py:115) has no kernel of its own: proj's epilogue leaves x + proj(...) a second time as fc1's split-fp16
  // operand, UN-normalised, with (mean, M2) of each 64-column slice of each row; fc1 runs on W diag(gamma) and applies
  // rstd (. - mean c1) + c2 in its epilogue (gemm_x2.hip EPI_RESID_LN / EPI_GELU_LN).  OFF by default (D3DP_FOLD_LN=1 turns it
  // on): measured on configs[2], same box, interleaved -- 50.06 / 49.86 hypothesis-clips/s folded against 49.83 / 49.70 with the
  // row kernel: the 284 ms/step of the LayerNorm kernel come back as +160 ms in proj (its tile epilogue now also splits, stores
  // the operand and reduces the statistics with the matrix pipes idle) and +90 ms in fc1 (profiles/r03_fold_ln_ab.md).
  bool fold_ln() const { return fold_resid() && fold_ln_on && 2 * cfg.hidden <= 2048; }
  // The shared norm at a block boundary (Spatial_norm in front of the TTE blocks, Temporal_norm in front of the STE blocks d >= 1)
  // is DEFERRED into the next block's proj: the norm pair stores the next qkv operand and 8 bytes of (mean, rstd) per row but does
  // not rewrite x (2 KB per row at C = 512, a third of its traffic); proj, the first kernel to touch x again and one that reads
  // and writes that row anyway, forms LN(x) in its epilogue (EPI_RESID_NORM) -- the same expression on the same values, so every
  // result bit stays.  The boundary that adds Temporal_pos (after STE block 0) keeps the in-place form.  D3DP_DEFER_NORM=0 keeps it
  // everywhere: the cross-check.  Plain-kernel dataflow only (proj's k-loop must cover the statistics' double buffer: C >= 96).
  bool defer_norm() const {
    // (ln2_defer_kernel is width-templated: a padded-head context keeps the in-place norm pair, as width 64 does)
    return fold_resid() && defer && !fold_ln() && skew_d == 0 && pingpong == 0 && cfg.channels >= 96 && 3 * cfg.channels <= 2048 && !hdp;
  }
  // The EXACT qkv / fc1 Linears run the SKEWED schedule of gemm_x2.hip (a tile's epilogue spread under the k-loop of the
  // next): the order in which a token row sums its k-steps then depends on (row within its pass) / 16 mod 4.  Every sequence
  // therefore starts at a multiple of 64 rows -- seq_pitch() rows per sequence, F J rounded up, the rest finite filler -- so
  // that order is a function of the token's index within its sequence alone and results stay bit-identical whatever the batch
  // composition, pass split or rank count (the H-sharding contract, tests/test_hip_parity.py::test_full_size_properties).
  bool skew() const { return x2_attn() && skew_d > 0 && cfg.channels >= 128 * skew_d; }   // (K = C >= 4 D k-steps of 32)
  int seq_pitch() const {
    const int fj = cfg.frames * cfg.joints;
    return (pad_override < 0 ? skew() : (pad_override > 0 && x2_attn())) ? (fj + 63) / 64 * 64 : fj;
  }
  // The backward pass runs the weight-gradient products (one merged TN launch per block, or one launch per Linear, and the sum of
  // their partial tiles) on a second stream beside the rest of the backward pass: a block's launch goes on while the next block's
  // dgrad products, attention and row kernels run (two operand / partial-tile sets, X2Train::use_set).  Forked and joined with events
  // on the caller's stream (nothing synchronises the host); D3DP_TRAIN_OVERLAP=0 keeps one stream.  Worth 0.2 ms of a 21 ms step
  // since the weight gradients are one launch per block: kept because it costs nothing.
  hipStream_t aux = nullptr;
  hipEvent_t ev_fork = nullptr, ev_done[2] = {nullptr, nullptr};
  bool x3() const { return exact() && exact_impl == 1; }
  int act() const { return fast() ? (fast_f16 ? 4 : 1) : (x3() ? 2 : (x2() ? 3 : 0)); }   // code understood by the row-wise launchers
  size_t act_size() const { return fast() ? 2 : (x3() ? 6 : 4); }    // bytes per element of a Linear-input activation
  size_t wide_size() const { return fast() ? 2 : 4; }                // bytes per element of bufB (qkv fp32 = 12C; hidden planes <= 12C)
  size_t y_size() const { return fast() ? 2 : 4; }
  // (clip, hypothesis) sequences per internal pass: 15 (61,965 tokens) measured best for FAST (working set near the
  // 256 MiB memory-side cache); EXACT is compute-bound in its Linears and gains 1.5 % from 30 (fewer, fuller tile rounds)
  int chunk() const { return cfg.chunk_seqs != 0 ? std::abs(cfg.chunk_seqs) : (exact() ? 31 : 15); }   // (< 0: uniform passes, for A/B)
  // EXACT split-fp16 Linears are persistent kernels over 256 x 128 tiles on n_cu workgroups: a pass over n sequences costs
  // sum over the four Linears of ceil(row_tiles(n) * column_tiles / n_cu) tile rounds x k-depth, and a partly filled last
  // round costs a full one (uniform chunks of 30 lose 4.4 % of the Linear time to it).  plan() splits `total` sequences
  // into passes of at most chunk() that minimise that sum (dynamic programme; any split gives bit-identical results).
  int n_cu = 0;
  std::vector<int> plan_cache;
  int plan_total = -1;
  const std::vector<int>& plan(int total) {
    if (total == plan_total) return plan_cache;
    const int cap = std::min(chunk(), total), SP = seq_pitch();
    plan_cache.clear();
    plan_total = total;
    if (!x2() || cfg.chunk_seqs < 0 || n_cu <= 0) {    // uniform passes (FAST, cross-check implementations)
      for (int s0 = 0; s0 < total; s0 += cap) plan_cache.push_back(std::min(cap, total - s0));
      return plan_cache;
    }
    // per Linear (qkv, proj, fc1, fc2): column strips, k-depth, and whether it runs the skewed schedule -- there a
    // workgroup owns the row tiles of one row group inside one strip (ceil(R / Q) tiles, Q = n_cu / strips row groups)
    // plus the flush of 3 D k-steps; in the plain schedule tiles are dealt round robin (ceil(R strips / n_cu) rounds)
    // (a padded-head context: qkv has 3 cp() columns and proj a k-depth of cp())
    const long tn[4] = {(3 * attn_cols() + 127) / 128, (cfg.channels + 127) / 128, (cfg.hidden + 127) / 128,
                        (cfg.channels + 127) / 128};
    const long kd[4] = {cfg.channels, attn_cols(), cfg.channels, cfg.hidden};
    const bool sk[4] = {skew(), false, skew(), false};
    std::vector<double> cost(cap + 1, 0.0);
    for (int n = 1; n <= cap; ++n) {
      const long R = ((long)n * SP + 255) / 256;
      for (int k = 0; k < 4; ++k) {
        const long Q = n_cu / tn[k];
        if (sk[k] && Q >= 1) cost[n] += ((double)((R + std::min(Q, R) - 1) / std::min(Q, R)) + 3.0 * skew_d * 32.0 / (double)kd[k]) * (double)kd[k];
        else cost[n] += (double)((R * tn[k] + n_cu - 1) / n_cu) * (double)kd[k];
      }
      cost[n] += 1e-3 * (double)kd[0];                   // (a pass has a fixed cost too: 7 launches per block)
    }
    std::vector<double> best(total + 1, 1e300);
    std::vector<int> pick(total + 1, 0);
    best[0] = 0.0;
    for (int b = 1; b <= total; ++b)
      for (int n = 1; n <= std::min(cap, b); ++n)
        if (best[b - n] + cost[n] < best[b]) { best[b] = best[b - n] + cost[n]; pick[b] = n; }
    for (int b = total; b > 0; b -= pick[b]) plan_cache.push_back(pick[b]);
    return plan_cache;
  }

  int flush_events() {
    for (size_t i = 0; i < used; ++i) {
      if (hipEventSynchronize(pool[i].b) != hipSuccess) return -1;
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, pool[i].a, pool[i].b) != hipSuccess) return -1;
      counts[pool[i].cls]++;
      total_ms[pool[i].cls] += ms;
    }
    used = 0;
    return 0;
  }
  // returns slot index or -1
  int begin(int cls, hipStream_t st) {
    if (!prof) return -1;
    if (used == pool.size()) {
      if (pool.size() >= 32768) { if (flush_events() != 0) return -1; }
      else {
        Ev e{};
        // (no system-scope fence at the event: the bracket must not add an L2 write-back of the kernel's output to the time it measures)
        if (hipEventCreateWithFlags(&e.a, hipEventDisableSystemFence) != hipSuccess || hipEventCreateWithFlags(&e.b, hipEventDisableSystemFence) != hipSuccess) return -1;
        pool.push_back(e);
      }
    }
    pool[used].cls = cls;
    (void)hipEventRecord(pool[used].a, st);
    return (int)used++;
  }
  void end(int slot, hipStream_t st) {
    if (slot >= 0) (void)hipEventRecord(pool[slot].b, st);
  }
};

struct Scope {
  d3dp_ctx* c; int slot; hipStream_t st;
  Scope(d3dp_ctx* c_, int cls, hipStream_t st_) : c(c_), slot(c_ ? c_->begin(cls, st_) : -1), st(st_) {}
  ~Scope() { if (c) c->end(slot, st); }
};

// (sp: rows per (clip, hypothesis) sequence in the token buffers, >= F J; d3dp_ctx::seq_pitch)
inline SeqMap spatial_map(int F, int J, int sp = 0) { return sp > F * J ? SeqMap{J, F, sp, J, 1} : SeqMap{J, 1, J, 0, 1}; }
inline SeqMap temporal_map(int F, int J, int sp = 0) { return SeqMap{F, J, sp > F * J ? sp : F * J, 1, J}; }
