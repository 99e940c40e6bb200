// What d3dp_create decides before it looks for a device: the environment switches of a context (CtxEnv), the route they and the
// shape select (CtxPlan) and the one function that derives the second from the first or refuses (plan_context).  Pure arithmetic
// on a d3dp_cfg and a dozen strings: no HIP here, so that any machine can check it (tests/test_ctx_plan_host.py).
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "../../include/d3dp_hip.h"

// The one error function: formats the message d3dp_last_error() returns for this thread and returns `code` (capi.hip)
int d3dp_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// The raw value of every switch a context reads at creation (null: unset), and the one place that reads them.
// (D3DP_TRAIN_ATTN_BWD alone is no part of a context: train.hip reads it per call, because tests flip it between two steps.)
struct CtxEnv {
  const char *exact_impl = nullptr, *long_attn = nullptr, *no_fold = nullptr, *defer_norm = nullptr, *train_impl = nullptr,
             *train_overlap = nullptr, *train_gelu = nullptr, *train_wgrad = nullptr, *train_ln_operand = nullptr, *train_tail = nullptr,
             *train_attn = nullptr, *train_passes = nullptr, *fast_impl = nullptr, *fast16_range = nullptr, *x2_skew = nullptr,
             *x2_pp = nullptr, *x2_wide = nullptr, *seq_pad = nullptr, *fold_ln = nullptr, *train_long_attn = nullptr,
             *train_attn_passes = nullptr, *train_rows = nullptr;
  static CtxEnv from_process() {
    CtxEnv e;
    e.exact_impl = getenv("D3DP_EXACT_IMPL");                 // bf16x3 | f32: cross-check implementations of EXACT mode; f16x2: opt-in at 192 ... 448
    e.long_attn = getenv("D3DP_LONG_ATTN");                   // rows: cross-check, clips > 256 frames on the fp32 row attention kernel
    e.no_fold = getenv("D3DP_NO_FOLD");                       // 1: cross-check, residual adds (and norm2) in the row kernels
    e.defer_norm = getenv("D3DP_DEFER_NORM");                 // 0: cross-check, keeps the shared norms in place in the norm pair
    e.train_impl = getenv("D3DP_TRAIN_IMPL");                 // f32: cross-check, training Linears on the fp32 matrix cores; f16x2: opt-in at 192 ... 448
    e.train_overlap = getenv("D3DP_TRAIN_OVERLAP");           // 0: profiling, one stream; 1: one operand set
    e.train_gelu = getenv("D3DP_TRAIN_GELU");                 // pass: d h_pre by a pass of its own (variants build only)
    e.train_wgrad = getenv("D3DP_TRAIN_WGRAD");               // each: a launch per weight gradient (variants build only)
    e.train_ln_operand = getenv("D3DP_TRAIN_LN_OPERAND");     // pass: round 5's operand pass behind every LayerNorm (variants build only)
    e.train_tail = getenv("D3DP_TRAIN_TAIL");                 // split: round 4's handling of a batch's last T mod 256 rows (variants build only)
    e.train_attn = getenv("D3DP_TRAIN_ATTN");                 // f32 | x2t: cross-check, the training attention of both / the spatial axis in fp32
    e.train_passes = getenv("D3DP_TRAIN_PASSES");             // 1: opt-in, one fp16-MFMA pass per product of the split-fp16 training Linears
    e.fast_impl = getenv("D3DP_FAST_IMPL");                   // mfma: opt-in, FAST / FAST16 contexts at 192 ... 448
    e.fast16_range = getenv("D3DP_FAST16_RANGE");             // scale: opt-in, per-block fp16 scales instead of FAST16's bf16 fallback
    e.x2_skew = getenv("D3DP_X2_SKEW");                       // 1 | 2 | 4: experiment, the row-class skewed schedule of the EXACT Linear
    e.x2_pp = getenv("D3DP_X2_PP");                           // 1: experiment, its ping-pong form
    e.x2_wide = getenv("D3DP_X2_WIDE");                       // 1: experiment, its 256 x 256 tile form
    e.seq_pad = getenv("D3DP_SEQ_PAD");                       // 0 | 1: experiment, the sequence padding of the skewed schedule without it / the reverse
    e.fold_ln = getenv("D3DP_FOLD_LN");                       // 1: experiment, norm2 folded into proj / fc1
    e.train_long_attn = getenv("D3DP_TRAIN_LONG_ATTN");       // chunked: opt-in, the fp32 training attention backward at any sequence length
    e.train_attn_passes = getenv("D3DP_TRAIN_ATTN_PASSES");   // 1: opt-in, one fp16-MFMA pass per product of the split-fp16 training attention
    e.train_rows = getenv("D3DP_TRAIN_ROWS");                 // hi: opt-in, the one-pass training Linears' operands as plain fp16 rows
    return e;
  }
};

// What creation decides; d3dp_ctx carries it as its base (ctx.h).
struct CtxPlan {
  // D3DP_EXACT_IMPL=f16x2 at channels in {192, 320, 384, 448}: the split-fp16 implementation at a width outside the instantiated
  // set.  The head dim is PADDED inside the packed weights to hdp = 32 or 64 (capi_weights.hip): the qkv Linear writes packed rows
  // of cp() = heads x hdp columns whose pad columns are exact zeros, the attention kernels run their head dim 32 / 64
  // instantiations on them (the softmax exponent takes the true head dim) and proj contracts over cp() columns against zero weight
  // columns.  The residual stream, the LayerNorms and the MLP keep the true width.  0: no padding (every other context).
  // D3DP_FAST_IMPL=mfma at the same widths (FAST / FAST16 contexts): the same padding inside 2-byte weights -- the streaming
  // Linear at the k-depths of these widths (gemm_stream_widths.hip), the FAST attention kernels' head dim 32 / 64 forms with the true head
  // dim in the exponent (attention_fast_pad.hip) and run-time-width row kernels with 2-byte rows (pointwise_rows2.hip).  Such a context
  // has no fallback implementation: FAST16's range fallback is the same route on bf16.
  int hdp = 0;
  // D3DP_FAST16_RANGE=scale: a per-block bound that reaches 65504 lowers that block's power-of-two scale for the tensor class it
  // bounds (BlockDev::r_*) instead of moving the whole context to bf16 -- what EXACT does with s_kv / s_h.  The context still falls
  // back when a weight is non-finite, when a LayerNorm output bound or a max |w| reaches 65504 (neither is scaled), or when a class
  // would need more than 2^-kFast16MaxShift.
  bool fast16_scale = false;
  int train_passes = 3;          // D3DP_TRAIN_PASSES=1 (TRAIN contexts with train_x2 alone): every product of X2Train's Linears --
                                 // forward, dgrad, both wgrad forms -- as ONE fp16-MFMA pass hi(A) x hi(W): the hi plane of a split operand
                                 // is that tensor rounded to fp16 at its own power-of-two scale, so nothing else in the step changes
  int train_attn_passes = 3;     // D3DP_TRAIN_ATTN_PASSES=1 (TRAIN contexts alone): every attention of the step that runs on the unpadded
                                 // kernels of train_attn.hip -- both axes, or the temporal one under D3DP_TRAIN_ATTN=x2t -- runs each of
                                 // its products (S, O; S, dP, dQ, dK, dV) as ONE fp16-MFMA pass on operands rounded once to fp16 at
                                 // their device-side scale, from one-plane LDS images (train_attn_1p.hip)
  bool train_rows_hi = false;    // D3DP_TRAIN_ROWS=hi (TRAIN contexts under D3DP_TRAIN_PASSES=1 alone): every operand of X2Train's Linears --
                                 // activations, both forms of the weights, every dY -- is stored as plain fp16 rows ("h1": column c at
                                 // offset c, half the row stride, the regions of the workspace half used) and the one-pass products
                                 // read whole 128-byte lines of 64 k.  Same hi values, same MFMAs in the same order: bit-equal
  int exact_impl_req = 0;        // what D3DP_EXACT_IMPL asked for (0 = f16x2, 1 = bf16x3, 2 = f32): d3dp_ctx::exact_impl starts from it
  bool long_rows = false;        // D3DP_LONG_ATTN=rows: the row-kernel cross-check
  bool fold = true;              // proj / fc2 add into the residual stream in their epilogue (d3dp_ctx::fold_resid)
  bool defer = true;             // the shared norm at a block boundary is deferred into the next proj (d3dp_ctx::defer_norm)
  bool train_x2 = true;          // D3DP_TRAIN_IMPL=f32: the training Linears on the fp32 matrix cores (round-1 path, cross-check).  Also
                                 // false at a width outside {64, 128, 256, 512} -- unless D3DP_TRAIN_IMPL=f16x2 opted a TRAIN context
                                 // at channels in {192, 320, 384, 448} into the split-fp16 step
  bool train_overlap = true;     // the weight-gradient products on the context's second stream (d3dp_ctx::aux)
  int train_overlap_sets = 2;    // D3DP_TRAIN_OVERLAP=1: one operand set (every operand pass waits for the product before it)
  bool train_gelu_in_prep = true;// D3DP_TRAIN_GELU=pass: d h_pre by a pass of its own (gelu_bwd_kernel) instead of inside the fc1 gradients' operand pass
  bool train_wgrad_merged = true;// D3DP_TRAIN_WGRAD=each: a launch (and 32 MB of partial tiles) per weight gradient instead of one per block
  bool train_ln_direct = true;   // D3DP_TRAIN_LN_OPERAND=pass: the qkv / fc1 operands by an operand pass behind the LayerNorm (round 5) instead of by its producer
  bool train_tail_blocks = true; // D3DP_TRAIN_TAIL=split: the round-4 handling of a batch's last T mod 256 rows (an extra round of tiles,
                                 // or a split-K launch of their own) instead of the 16 x 64 blocks at the end of the product's kernel
  int train_attn_x2 = 2;         // the training step's attention on the split-fp16 kernels of train_attn.hip: 2 = both axes (default),
                                 // 1 = D3DP_TRAIN_ATTN=x2t: the temporal axis only, 0 = D3DP_TRAIN_ATTN=f32: neither (the round-4
                                 // fp32 kernels -- fp32-MFMA temporal forward and backward, VALU spatial forward: the cross-check)
  bool train_long_attn = false;  // D3DP_TRAIN_LONG_ATTN=chunked (TRAIN contexts alone): every fp32 attention backward of the training step
                                 // that runs on the VALU kernels takes their chunked forms (train.hip attn_bwd_*_chunk_kernel: K / V,
                                 // then Q / dO / statistics pass through LDS in chunks of rows, a row block of 256 per workgroup), which
                                 // take any sequence length: no token limit in step 6, no frames <= 256 in d3dp_train_forward
  int skew_d = 0;                // D3DP_X2_SKEW=1|2|4: k-steps a parked row class takes to leave.  OFF by default: measured
                                 // 3 % slower on the whole step (gemm_x2.hip, DESIGN.md 7: the Linear is bound by its vector-memory
                                 // instruction rate, and an epilogue's stores cost the same wherever they issue)
  int pingpong = 0;              // D3DP_X2_PP=1: the ping-pong form of the EXACT Linear (gemm_x2.hip; bit-identical results;
                                 // measured 1.5-2 % SLOWER on the whole step, gpurun c8); 2 = D3DP_X2_WIDE=1: the 256 x 256
                                 // tile form (bit-identical; ties with the default, profiles/r04_gemm_probes.md section 4)
  int pad_override = -1;         // D3DP_SEQ_PAD=0|1: measurement switch (pad without the skewed schedule, or the reverse)
  bool fold_ln_on = false;       // D3DP_FOLD_LN=1 (d3dp_ctx::fold_ln)
};

inline bool env_is(const char* v, const char* s) { return v && !strcmp(v, s); }
// v is exactly one of the digits in `allowed`: that digit; anything else: dflt
inline int env_digit(const char* v, const char* allowed, int dflt) {
  return v && v[0] && !v[1] && strchr(allowed, v[0]) ? v[0] - '0' : dflt;
}
inline bool mfma_head_dim(int hd) { return hd == 64 || hd == 32 || hd == 16; }   // head dims the matrix-core attention kernels take

// The matrix-core kernels (split-fp16 / bf16 operands) and the row kernels around them are instantiated for the widths
// {64, 128, 256, 512} with head dims {8, 16, 32, 64}: every configuration the reference publishes (`-cs 512`, README.md:33-39)
// and its smaller powers of two.  The reference itself takes ANY `-cs` its 8 heads divide (common/arguments.py:49,
// mixste.py:46-62): such a width runs EXACT mode on the fp32 implementation -- fp32-MFMA Linears (gemm_f32_kernel), the fp32
// row attention with a run-time head dim, run-time-width row kernels (pointwise.hip *_g_kernel) -- i.e. the cross-check
// implementation D3DP_EXACT_IMPL=f32 selects by hand for the instantiated widths: same tolerance, roughly a fifth of the
// throughput.  A TRAIN context of such a width (the reference trains at any `-cs` too: main.py:325) takes the fp32 path of the
// training step -- what D3DP_TRAIN_IMPL=f32 selects for the instantiated widths -- through the run-time-width row kernels of
// train_g.hip and the VALU attention backward with a run-time head dim.  FAST / FAST16 contexts exist for the instantiated
// widths and, under D3DP_FAST_IMPL=mfma, for channels in {192, 320, 384, 448} (fast_optin_shape).
inline bool instantiated_width(const d3dp_cfg& g) {
  const int hd = g.channels / g.heads;
  return (g.channels == 64 || g.channels == 128 || g.channels == 256 || g.channels == 512) &&
         (hd == 8 || hd == 16 || hd == 32 || hd == 64) && g.hidden >= 64 && g.hidden % 64 == 0;
}
inline bool optin_width(int c) { return c == 192 || c == 320 || c == 384 || c == 448; }
inline int padded_head_dim(int hd) { return hd <= 32 ? 32 : 64; }
// The shape D3DP_EXACT_IMPL=f16x2 and D3DP_TRAIN_IMPL=f16x2 opt into the split-fp16 kernels, each for contexts of its own mode alone.
// An EXACT context there runs the split-fp16 implementation with its head dim padded to 32 / 64 inside the packed weights
// (CtxPlan::hdp).  A TRAIN context takes the split-fp16 training step -- X2Train's Linears take any N, K that are multiples of 32,
// the row kernels of train_g.hip leave the operand absmax behind, and the attention runs on train_attn.hip with the head padded to
// 32 / 64 inside its LDS images (no weight, workspace or Linear knows about the padding).  At an instantiated width either value
// names the default; anywhere else it cannot be honoured and is refused -- never ignored.
inline bool x2_optin_shape(const d3dp_cfg& g) {
  const int hd = g.channels / g.heads;
  return optin_width(g.channels) && hd % 8 == 0 && hd <= 64 && g.hidden >= 64 && g.hidden % 64 == 0;
}
// The shape D3DP_FAST_IMPL=mfma opts in (FAST / FAST16 contexts alone): such a context runs the mode's dataflow -- 2-byte weights and
// activations, fp32 residual stream, both attentions and all four Linears on the matrix cores -- with the head dim padded to 32 / 64
// inside the packed 2-byte weights (CtxPlan::hdp).  hidden = 2 x channels (what MixSTE2 builds): the k-depths the streaming Linear is
// instantiated for.  Head dims 24 / 40 / 48 / 56 (the model's 8 heads) are the ones the padded attention kernels carry the exponent
// of (attention_fast_pad.hip); 32 and 64 (6 or 3 heads at 192, ...) need no padding and run the kernels of the instantiated widths;
// 8 and 16 (12, 24, ... heads) have no kernel behind this route.  At an instantiated width the value names the default; any other
// value, width or shape is refused -- never ignored.
inline bool fast_optin_shape(const d3dp_cfg& g) {
  const int hd = g.channels / g.heads;
  return optin_width(g.channels) && (hd == 24 || hd == 32 || hd == 40 || hd == 48 || hd == 56 || hd == 64) && g.hidden == 2 * g.channels;
}
// The tile of the training step's product kernels (gemm_x2_tile.h XBM x XBN) and the weights d3dp_launch_wprep prepares in one call
constexpr int D3DP_TN_TILE_N = 256, D3DP_TN_TILE_K = 128;
constexpr int D3DP_WPREP_MAX = 64;
// the weight gradient dW[N, K] straight from the row forms of its two operands (gemm_f16x2_tn_kernel): whole tiles only
inline bool d3dp_tn_applies(int N, int K) { return N % D3DP_TN_TILE_N == 0 && K % D3DP_TN_TILE_K == 0; }
// The training Linears run on split-fp16 operands (X2Train, capi_train.hip); else on the fp32 matrix cores: TrainPath::use_x2 (train_plan.h)
inline bool train_linears_split(const CtxPlan& p, const d3dp_cfg& g) { return p.train_x2 && g.channels % 32 == 0 && g.hidden % 32 == 0; }

// The route of a context of shape g under the switches e, in a library with (variants_built) or without the experiment kernels of
// gemm_x2.hip: D3DP_OK and *out, or the first refusal in the order of the steps below, through d3dp_fail.  Every switch that
// cannot be honoured is refused by name -- never ignored -- and all of it before the device is looked for.
inline int plan_context(const d3dp_cfg& g, const CtxEnv& e, bool variants_built, CtxPlan* out) {
  // 1. Argument ranges.
  // (frames > 256: EXACT, FAST and FAST16 contexts take the chunked-key form of their attention kernels; at head dim 8 FAST / FAST16
  //  contexts stay on the row kernel -- fp32 arithmetic on their 2-byte rows -- and EXACT contexts on the fp32 kernels, at every clip
  //  length.  TRAIN contexts: the training step's split-fp16 attention (head dims 64, 32, 16: train_attn.hip) passes keys / queries
  //  through LDS in chunks and takes every length up to 1024; its fp32 attention -- head dim 8, the cross-check switches -- holds a
  //  whole sequence in LDS and d3dp_train_forward refuses more than 256 frames there; a TRAIN context of a width outside the
  //  instantiated set runs that fp32 attention with a run-time head dim and is refused in step 6 beyond 256 tokens, 153 at head dims
  //  above 64 -- unless D3DP_TRAIN_IMPL=f16x2 opted it into the split-fp16 step: head dims 24 / 40 / 48 / 56 then run padded forms
  //  of the split-fp16 attention and take every length up to 1024 too, and what the cross-check switches or head dim 8 leave on the
  //  fp32 attention there is refused by d3dp_train_forward like at every width.  D3DP_TRAIN_LONG_ATTN=chunked, step 5a, lifts both
  //  refusals: the fp32 attention backward then passes its rows through LDS in chunks, as the fp32 row attention forward does.)
  if (g.frames < 1 || g.frames > 1024) return d3dp_fail(D3DP_ENOTSUP, "frames=%d not in [1,1024]", g.frames);
  // (more than 32 joints: the spatial axis takes the whole-sequence attention kernels the temporal axis runs on, round 6)
  if (g.joints < 1 || g.joints > 256) return d3dp_fail(D3DP_ENOTSUP, "joints=%d not in [1,256]", g.joints);
  if (g.heads < 1 || g.channels < 1 || g.channels % g.heads) return d3dp_fail(D3DP_EINVAL, "heads=%d does not divide channels=%d", g.heads, g.channels);
  if (g.depth < 1) return d3dp_fail(D3DP_EINVAL, "depth=%d", g.depth);
  if (g.mode != D3DP_MODE_EXACT && g.mode != D3DP_MODE_FAST && g.mode != D3DP_MODE_TRAIN && g.mode != D3DP_MODE_FAST16)
    return d3dp_fail(D3DP_EINVAL, "mode=%d", g.mode);
  const int hd = g.channels / g.heads;
  const bool inst = instantiated_width(g), train = g.mode == D3DP_MODE_TRAIN, fast16 = g.mode == D3DP_MODE_FAST16;
  CtxPlan p;
  p.long_rows = env_is(e.long_attn, "rows");
  // 2. D3DP_EXACT_IMPL=f16x2 outside the instantiated widths (read in every mode).
  if (env_is(e.exact_impl, "f16x2") && !inst) {
    if (!x2_optin_shape(g) || g.mode != D3DP_MODE_EXACT)
      return d3dp_fail(D3DP_ENOTSUP, "D3DP_EXACT_IMPL=f16x2 outside the instantiated widths exists for D3DP_MODE_EXACT contexts with channels in "
                                "{192,320,384,448}, head dim a multiple of 8 up to 64 and hidden a multiple of 64; channels=%d heads=%d "
                                "hidden=%d mode=%d is not one (unset the switch: such a context runs the fp32 implementation)",
                  g.channels, g.heads, g.hidden, g.mode);
    if (p.long_rows)
      return d3dp_fail(D3DP_ENOTSUP, "D3DP_LONG_ATTN=rows with D3DP_EXACT_IMPL=f16x2 at channels=%d: the run-time-head-dim row attention has no "
                                "split-fp16 output form", g.channels);
    p.hdp = padded_head_dim(hd);
  }
  // 3. D3DP_TRAIN_IMPL=f16x2 outside the instantiated widths (TRAIN contexts alone).
  const bool train_widths = train && !inst && env_is(e.train_impl, "f16x2");
  if (train_widths && !x2_optin_shape(g))
    return d3dp_fail(D3DP_ENOTSUP, "D3DP_TRAIN_IMPL=f16x2 outside the instantiated widths exists for D3DP_MODE_TRAIN contexts with channels in "
                              "{192,320,384,448}, head dim a multiple of 8 up to 64 and hidden a multiple of 64; channels=%d heads=%d "
                              "hidden=%d is not one (unset the switch: such a context trains on the fp32 path)",
                g.channels, g.heads, g.hidden);
  // 4. D3DP_FAST_IMPL (FAST / FAST16 contexts alone).
  if ((g.mode == D3DP_MODE_FAST || fast16) && e.fast_impl) {
    if (strcmp(e.fast_impl, "mfma"))
      return d3dp_fail(D3DP_ENOTSUP, "D3DP_FAST_IMPL=%.32s: the one value a FAST / FAST16 context takes is D3DP_FAST_IMPL=mfma (channels=%d)",
                  e.fast_impl, g.channels);
    if (!inst) {
      if (!fast_optin_shape(g))
        return d3dp_fail(D3DP_ENOTSUP, "D3DP_FAST_IMPL=mfma outside the instantiated widths exists for FAST / FAST16 contexts with channels in "
                                  "{192,320,384,448}, head dim in {24,32,40,48,56,64} and hidden = 2 x channels; channels=%d heads=%d "
                                  "hidden=%d is not one (such a width runs in D3DP_MODE_EXACT / D3DP_MODE_TRAIN)",
                    g.channels, g.heads, g.hidden);
      if (p.long_rows)
        return d3dp_fail(D3DP_ENOTSUP, "D3DP_LONG_ATTN=rows with D3DP_FAST_IMPL=mfma at channels=%d: the row attention kernel would take the padded "
                                  "head dim for its exponent", g.channels);
      p.hdp = padded_head_dim(hd);
    }
  }
  // 5. D3DP_FAST16_RANGE=scale (FAST16 contexts alone): a block whose proven bound reaches 65504 stores the tensors that bound covers
  // at a power-of-two multiple of their value instead of moving the whole context to bf16 (CtxPlan::fast16_scale; chosen at
  // d3dp_set_weights).  The scaled kernels exist on the matrix-core route of the instantiated widths: the streaming Linear at K / 64
  // in {1, 2, 4, 8, 16}, the three attention kernels at head dims 64 / 32 / 16, the row kernels at widths 64 ... 512.  Any other value,
  // head dim 8 and the row attention kernel (no scaled form), and the padded widths of D3DP_FAST_IMPL=mfma are refused.
  if (fast16 && e.fast16_range) {
    if (strcmp(e.fast16_range, "scale"))
      return d3dp_fail(D3DP_ENOTSUP, "D3DP_FAST16_RANGE=%.32s: the one value a FAST16 context takes is D3DP_FAST16_RANGE=scale", e.fast16_range);
    if (p.hdp)
      return d3dp_fail(D3DP_ENOTSUP, "D3DP_FAST16_RANGE=scale with D3DP_FAST_IMPL=mfma at channels=%d: the padded-head kernels have no scaled "
                                "form", g.channels);
    if (inst && !mfma_head_dim(hd))
      return d3dp_fail(D3DP_ENOTSUP, "D3DP_FAST16_RANGE=scale at head dim %d (channels=%d heads=%d): the scaled attention kernels exist at head "
                                "dims 64, 32 and 16", hd, g.channels, g.heads);
    if (inst && p.long_rows)
      return d3dp_fail(D3DP_ENOTSUP, "D3DP_FAST16_RANGE=scale with D3DP_LONG_ATTN=rows: the row attention kernel has no scaled form");
    const int k = g.hidden;
    if (inst && !(k == 64 || k == 128 || k == 256 || k == 512 || k == 1024))
      return d3dp_fail(D3DP_ENOTSUP, "D3DP_FAST16_RANGE=scale with hidden=%d: the scaled streaming Linear exists at k-depths 64, 128, 256, 512 "
                                "and 1024", g.hidden);
    p.fast16_scale = inst;             // (any other width: refused in step 6 like every FAST16 context there)
  }
  // 5a. D3DP_TRAIN_LONG_ATTN (TRAIN contexts alone; in front of step 6 because it lifts that step's token limit): =chunked moves the
  // fp32 attention backward onto the chunked VALU kernels (CtxPlan::train_long_attn).  Any other value is refused -- never ignored.
  if (train && e.train_long_attn) {
    if (strcmp(e.train_long_attn, "chunked"))
      return d3dp_fail(D3DP_ENOTSUP, "D3DP_TRAIN_LONG_ATTN=%.32s: the one value a TRAIN context takes is D3DP_TRAIN_LONG_ATTN=chunked (the fp32 "
                                "attention backward passes its rows through LDS in chunks and takes any sequence length)", e.train_long_attn);
    p.train_long_attn = true;
  }
  // 6. A width neither instantiated nor padded: the fp32 implementation, EXACT and TRAIN contexts alone.
  const bool width_inst = inst || p.hdp != 0;
  if (!width_inst) {
    if (g.mode == D3DP_MODE_FAST)
      return d3dp_fail(D3DP_ENOTSUP, "channels=%d heads=%d hidden=%d: FAST contexts exist for channels in {64,128,256,512} with head dim in "
                                "{8,16,32,64} and hidden a multiple of 64; other widths run in D3DP_MODE_EXACT / D3DP_MODE_TRAIN (fp32 implementation)",
                  g.channels, g.heads, g.hidden);
    if (fast16)
      return d3dp_fail(D3DP_ENOTSUP, "channels=%d heads=%d hidden=%d: FAST16 contexts exist for the shapes FAST contexts exist for -- channels in "
                                "{64,128,256,512} with head dim in {8,16,32,64} and hidden a multiple of 64; other widths run in D3DP_MODE_EXACT / "
                                "D3DP_MODE_TRAIN (fp32 implementation)",
                  g.channels, g.heads, g.hidden);
    if (g.channels > 1024 || g.channels % 4 || hd % 4 || hd > 128 || g.hidden < 4 || g.hidden % 4)
      return d3dp_fail(D3DP_ENOTSUP, "channels=%d heads=%d hidden=%d: the fp32 implementation takes channels <= 1024, head dim a multiple of 4 up to 128 "
                                "and hidden a multiple of 4", g.channels, g.heads, g.hidden);
    // (the fp32 attention backward holds two whole-sequence images of its capacity head dim + the statistics in the CU's 160 KiB;
    //  its chunked form -- D3DP_TRAIN_LONG_ATTN=chunked -- holds a chunk of rows and takes every length step 1 lets through)
    const int nmax = std::max(g.frames, g.joints), cap = hd <= 16 ? 16 : hd <= 32 ? 32 : hd <= 64 ? 64 : 128;
    if (train && !train_widths && !p.train_long_attn && (nmax > 256 || (size_t)nmax * (8 * (cap + 4) + 12) > 160 * 1024))
      return d3dp_fail(D3DP_ENOTSUP, "channels=%d heads=%d frames=%d joints=%d: training at a width outside {64,128,256,512} runs the fp32 attention "
                                "backward, which holds a whole sequence in LDS (<= 256 tokens; <= 153 at head dims above 64)",
                  g.channels, g.heads, g.frames, g.joints);
  }
  // The switches that refuse nothing by themselves.  train_x2: the training step may run on split-fp16 operands at an instantiated
  // or padded width, or where D3DP_TRAIN_IMPL=f16x2 opted a TRAIN context in -- a decision of its own beside width_inst, so that
  // neither opt-in switch changes what a context of the other mode does.
  const bool train_f32 = env_is(e.train_impl, "f32");
  p.fold = !(e.no_fold && e.no_fold[0] == '1');
  p.defer = !(e.defer_norm && e.defer_norm[0] == '0');
  p.train_x2 = !train_f32 && (width_inst || train_widths);
  p.train_overlap = !(e.train_overlap && e.train_overlap[0] == '0');
  p.train_overlap_sets = (e.train_overlap && e.train_overlap[0] == '1') ? 1 : 2;
  p.train_gelu_in_prep = !env_is(e.train_gelu, "pass");
  p.train_wgrad_merged = !env_is(e.train_wgrad, "each");
  p.train_ln_direct = !env_is(e.train_ln_operand, "pass");
  p.train_tail_blocks = !env_is(e.train_tail, "split");
  p.train_attn_x2 = env_is(e.train_attn, "f32") ? 0 : env_is(e.train_attn, "x2t") ? 1 : 2;
  const bool superseded = !p.train_gelu_in_prep || !p.train_wgrad_merged || !p.train_tail_blocks || !p.train_ln_direct;
  // 7. D3DP_TRAIN_PASSES (TRAIN contexts alone): =1 runs every product of the split-fp16 training Linears as one fp16-MFMA pass
  // hi(A) x hi(W) (gemm_x2_train.hip, PASSES = 1); =3 names the default.  It exists where X2Train's Linears run in their default
  // launch forms: any other value, the fp32 path and the superseded launch forms of the variants build (no one-pass form) are
  // refused.  D3DP_TRAIN_ATTN, D3DP_TRAIN_ATTN_BWD and D3DP_TRAIN_OVERLAP compose with it: they select attention kernels and
  // streams, not Linear products.
  if (train && e.train_passes) {
    if (strcmp(e.train_passes, "1") && strcmp(e.train_passes, "3"))
      return d3dp_fail(D3DP_ENOTSUP, "D3DP_TRAIN_PASSES=%.32s: the values a TRAIN context takes are D3DP_TRAIN_PASSES=1 (one fp16-MFMA pass per "
                                "product of the split-fp16 training Linears) and 3 (the default)", e.train_passes);
    if (e.train_passes[0] == '1') {
      if (!train_linears_split(p, g))
        return d3dp_fail(D3DP_ENOTSUP, "D3DP_TRAIN_PASSES=1 exists for the split-fp16 training Linears; channels=%d%s trains on the fp32 path "
                                  "(fp32-MFMA Linears have no one-pass form)", g.channels, train_f32 ? " under D3DP_TRAIN_IMPL=f32" : "");
      if (superseded)
        return d3dp_fail(D3DP_ENOTSUP, "D3DP_TRAIN_PASSES=1 beside D3DP_TRAIN_WGRAD=each / D3DP_TRAIN_TAIL=split / D3DP_TRAIN_GELU=pass / "
                                  "D3DP_TRAIN_LN_OPERAND=pass: the superseded launch forms have no one-pass form");
      p.train_passes = 1;
    }
  }
  // 7a. D3DP_TRAIN_ATTN_PASSES (TRAIN contexts alone; behind step 7 so that every earlier refusal keeps its place): =1 runs every
  // product of the split-fp16 training attention as one fp16-MFMA pass (train_attn_1p.hip); =3 names the default.  It exists where at
  // least one axis runs train_attn.hip UNPADDED: the split-fp16 Linears (their epilogues leave the device-side scales), head dim 64,
  // 32 or 16, and not D3DP_TRAIN_ATTN=f32.  Under D3DP_TRAIN_ATTN=x2t it applies to the temporal axis alone.  D3DP_TRAIN_PASSES,
  // D3DP_TRAIN_OVERLAP, D3DP_TRAIN_LONG_ATTN and D3DP_TRAIN_ATTN_BWD compose with it.
  if (train && e.train_attn_passes) {
    if (strcmp(e.train_attn_passes, "1") && strcmp(e.train_attn_passes, "3"))
      return d3dp_fail(D3DP_ENOTSUP, "D3DP_TRAIN_ATTN_PASSES=%.32s: the values a TRAIN context takes are D3DP_TRAIN_ATTN_PASSES=1 (one fp16-MFMA "
                                "pass per product of the split-fp16 training attention) and 3 (the default)", e.train_attn_passes);
    if (e.train_attn_passes[0] == '1') {
      if (!train_linears_split(p, g))
        return d3dp_fail(D3DP_ENOTSUP, "D3DP_TRAIN_ATTN_PASSES=1 exists for the split-fp16 training attention; channels=%d%s trains on the fp32 "
                                  "path (its attention runs the fp32 kernels, which have no one-pass form)", g.channels,
                    train_f32 ? " under D3DP_TRAIN_IMPL=f32" : "");
      if (hd == 24 || hd == 40 || hd == 48 || hd == 56)
        return d3dp_fail(D3DP_ENOTSUP, "D3DP_TRAIN_ATTN_PASSES=1 at head dim %d (channels=%d heads=%d): the padded forms of the split-fp16 "
                                  "training attention have no one-pass form", hd, g.channels, g.heads);
      if (!mfma_head_dim(hd))
        return d3dp_fail(D3DP_ENOTSUP, "D3DP_TRAIN_ATTN_PASSES=1 at head dim %d (channels=%d heads=%d): the one-pass training attention exists at "
                                  "head dims 64, 32 and 16 (this head dim runs the fp32 attention kernels)", hd, g.channels, g.heads);
      if (p.train_attn_x2 == 0)
        return d3dp_fail(D3DP_ENOTSUP, "D3DP_TRAIN_ATTN_PASSES=1 beside D3DP_TRAIN_ATTN=f32: both axes then run the fp32 attention kernels, which "
                                  "have no one-pass form");
      p.train_attn_passes = 1;
    }
  }
  // 7b. D3DP_TRAIN_ROWS (TRAIN contexts alone; behind step 7a so that every earlier refusal keeps its place): =hi stores every operand
  // of the one-pass training Linears as plain fp16 rows and runs their products on the whole-line kernels (gemm_x2_train.hip, HI);
  // =split names the default.  The route exists where no operand of the step is transposed and every producer writes rows itself:
  // D3DP_TRAIN_PASSES=1 at an instantiated width, every Linear of a block a TN shape (the merged weight gradient reads row forms),
  // channels a multiple of 256 (the LayerNorm kernels write the qkv / fc1 operands), depth within the batched weight preparation --
  // `-cs` 256 and 512 with hidden = 2 x channels, depth <= 8.  Everything else is refused by name.  The attention and stream
  // switches compose with it: they select no Linear operand.
  if (train && e.train_rows) {
    if (strcmp(e.train_rows, "hi") && strcmp(e.train_rows, "split"))
      return d3dp_fail(D3DP_ENOTSUP, "D3DP_TRAIN_ROWS=%.32s: the values a TRAIN context takes are D3DP_TRAIN_ROWS=hi (the one-pass training "
                                "Linears' operands as plain fp16 rows) and split (the default)", e.train_rows);
    if (e.train_rows[0] == 'h') {
      if (!train_linears_split(p, g))
        return d3dp_fail(D3DP_ENOTSUP, "D3DP_TRAIN_ROWS=hi exists for the split-fp16 training Linears; channels=%d%s trains on the fp32 path "
                                  "(fp32-MFMA Linears read no operand rows)", g.channels, train_f32 ? " under D3DP_TRAIN_IMPL=f32" : "");
      if (!inst)
        return d3dp_fail(D3DP_ENOTSUP, "D3DP_TRAIN_ROWS=hi at channels=%d under D3DP_TRAIN_IMPL=f16x2: the padded widths run an operand pass in "
                                  "front of every Linear and transposed weight-gradient operands, which have no hi-only form", g.channels);
      if (superseded)
        return d3dp_fail(D3DP_ENOTSUP, "D3DP_TRAIN_ROWS=hi beside D3DP_TRAIN_WGRAD=each / D3DP_TRAIN_TAIL=split / D3DP_TRAIN_GELU=pass / "
                                  "D3DP_TRAIN_LN_OPERAND=pass: the superseded launch forms have no hi-only form");
      if (p.train_passes != 1)
        return d3dp_fail(D3DP_ENOTSUP, "D3DP_TRAIN_ROWS=hi without D3DP_TRAIN_PASSES=1: the three-pass products read the lo halves that hi-only "
                                  "rows do not store");
      const int C = g.channels, Hd = g.hidden;
      if (C % 256 != 0 || !d3dp_tn_applies(3 * C, C) || !d3dp_tn_applies(C, C) || !d3dp_tn_applies(Hd, C) || !d3dp_tn_applies(C, Hd))
        return d3dp_fail(D3DP_ENOTSUP, "D3DP_TRAIN_ROWS=hi at channels=%d hidden=%d: the hi-only route exists where no operand of the step is "
                                  "transposed and the LayerNorm kernels write the qkv / fc1 operand rows -- channels a multiple of 256 "
                                  "and hidden a multiple of 256 (`-cs` 256 and 512); narrower widths use transposed operands", C, Hd);
      if (hd == 16 && p.train_attn_x2 != 0)
        return d3dp_fail(D3DP_ENOTSUP, "D3DP_TRAIN_ROWS=hi at head dim 16 (channels=%d heads=%d): the split-fp16 training attention writes "
                                  "hi-only proj operand rows at head dims 64 and 32", g.channels, g.heads);
      if (8 * g.depth > D3DP_WPREP_MAX)
        return d3dp_fail(D3DP_ENOTSUP, "D3DP_TRAIN_ROWS=hi at depth=%d: the hi-only weight operands are written by the batched weight preparation "
                                  "(depth <= %d); the per-weight preparation of deeper models has no hi-only form", g.depth, D3DP_WPREP_MAX / 8);
      p.train_rows_hi = true;
    }
  }
  // 8. The EXACT cross-check implementations: bf16x3 exists at the instantiated widths; a width neither instantiated nor padded
  // runs f32 whatever the variable says.
  p.exact_impl_req = env_is(e.exact_impl, "bf16x3") ? 1 : env_is(e.exact_impl, "f32") ? 2 : 0;
  if (!width_inst) {
    if (p.exact_impl_req == 1)
      return d3dp_fail(D3DP_ENOTSUP, "D3DP_EXACT_IMPL=bf16x3 exists for channels in {64,128,256,512}; channels=%d runs the fp32 implementation", g.channels);
    p.exact_impl_req = 2;
  }
  // 9. D3DP_TRAIN_WGRAD=each / D3DP_TRAIN_TAIL=split / D3DP_TRAIN_GELU=pass / D3DP_TRAIN_LN_OPERAND=pass were round 5's same-box A/B
  // switches: they make the configs[4] shapes take the launch forms the library keeps for the shapes its merged / fused forms do not
  // cover (widths below 256, contractions that are not a multiple of 16 k-steps).  Measured and superseded:
  // like the experiment kernels of step 10 they are honoured by the `make variants` library only.  (What stays: the cross-check
  // implementations D3DP_TRAIN_IMPL=f32, D3DP_TRAIN_ATTN=f32|x2t, D3DP_TRAIN_ATTN_BWD=valu, D3DP_EXACT_IMPL, D3DP_NO_FOLD, and the
  // profiling switch D3DP_TRAIN_OVERLAP=0|1: one stream, so that no kernel's duration contains a wait for CUs.)
  if (superseded && !variants_built)
    return d3dp_fail(D3DP_ENOTSUP, "D3DP_TRAIN_WGRAD=each / D3DP_TRAIN_TAIL=split / D3DP_TRAIN_GELU=pass / D3DP_TRAIN_LN_OPERAND=pass select superseded launch forms of the "
                              "training step that only the variants build honours (make -C d3dp_amd/csrc variants; "
                              "D3DP_LIB=d3dp_amd/lib/variants/libd3dp_variants.so)");
  // 10. Measurement switches of experiments that were measured and not adopted.  Their kernels exist only in a
  // library built with -DD3DP_X2_VARIANTS=1 (`make variants`).
  p.skew_d = env_digit(e.x2_skew, "0124", 0);
  p.pingpong = env_is(e.x2_wide, "1") ? 2 : env_digit(e.x2_pp, "01", 0);
  p.pad_override = env_digit(e.seq_pad, "01", -1);
  p.fold_ln_on = e.fold_ln && e.fold_ln[0] == '1';
  if ((p.skew_d || p.pingpong || p.pad_override > 0 || p.fold_ln_on) && !variants_built)
    return d3dp_fail(D3DP_ENOTSUP, "D3DP_X2_SKEW / D3DP_X2_PP / D3DP_X2_WIDE / D3DP_SEQ_PAD / D3DP_FOLD_LN select experiment kernels that this "
                              "library was built without (make -C d3dp_amd/csrc variants; D3DP_LIB=d3dp_amd/lib/variants/libd3dp_variants.so)");
  *out = p;
  return D3DP_OK;
}
