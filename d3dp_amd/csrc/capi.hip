// C-ABI layer of libd3dp_hip.so (see include/d3dp_hip.h), part 1 of 5: the per-thread error state, the context's life
// (d3dp_create reads every environment switch once, d3dp_destroy), the profile and status calls and the thin wrappers of the
// sampler / JPMA kernels.  The rest of the layer, one concern per file over the shared types of ctx.h:
//   capi_weights.hip  d3dp_set_weights: range proofs and weight packing      capi_ops.hip    the single-op test hooks
//   capi_denoise.hip  the inference schedule, workspace layout, attention route   capi_train.hip  the training step
// D3DP_FAST_F16 (common.h; `make fastf16`) is read in this file alone.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "ctx.h"

namespace {
thread_local std::string g_err;
}  // namespace

int d3dp_fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int d3dp_set_error(int code, const char* msg) { return d3dp_fail(code, "%s", msg); }
int d3dp_check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return d3dp_fail(D3DP_EHIP, "%s: %s", what, hipGetErrorString(e));
  return D3DP_OK;
}

namespace {

const char* kClassNames[D3DP_PROFILE_CLASSES] = {"gemm_qkv", "gemm_proj", "gemm_fc1", "gemm_fc2", "attn_spatial",
                                                 "attn_temporal", "layernorm", "norm_pair", "embed_ln", "head",
                                                 "time_mlp", "other",
                                                 "train_linear", "train_wgrad", "train_attn_fwd_spatial", "train_attn_fwd_temporal",
                                                 "train_attn_bwd_q_spatial", "train_attn_bwd_q_temporal", "train_attn_bwd_kv_spatial",
                                                 "train_attn_bwd_kv_temporal", "train_operand_pass", "train_ln_fwd", "train_ln_bwd",
                                                 "train_other", "event_pair_overhead"};

// D3DP_TRAIN_PASSES (opt-in; read for TRAIN contexts alone, by d3dp_create BEFORE the device is looked for, like the width
// switches there): =1 runs every product of the split-fp16 training Linears as one fp16-MFMA pass hi(A) x hi(W) (gemm_x2_train.hip,
// PASSES = 1); =3 names the default.  It exists where X2Train's Linears run in their default launch forms: any other value, the
// fp32 path (`train_split`: as read_switches below) and the superseded launch forms of the variants build (no one-pass form)
// are refused -- never ignored.  D3DP_TRAIN_ATTN, D3DP_TRAIN_ATTN_BWD and D3DP_TRAIN_OVERLAP compose with it: they select attention
// kernels and streams, not Linear products.  D3DP_OK and *passes, or the refusal.
int read_train_passes(const d3dp_cfg& g, bool train_split, int* passes) {
  *passes = 3;
  const char* tp = g.mode == D3DP_MODE_TRAIN ? getenv("D3DP_TRAIN_PASSES") : nullptr;
  if (!tp) return D3DP_OK;
  if (strcmp(tp, "1") && strcmp(tp, "3"))
    return d3dp_fail(D3DP_ENOTSUP, "D3DP_TRAIN_PASSES=%.32s: the values a TRAIN context takes are D3DP_TRAIN_PASSES=1 (one fp16-MFMA pass per "
                              "product of the split-fp16 training Linears) and 3 (the default)", tp);
  if (tp[0] == '3') return D3DP_OK;
  const char* ti = getenv("D3DP_TRAIN_IMPL");
  const bool f32 = ti && !strcmp(ti, "f32");
  if (f32 || !train_split || g.channels % 32 || g.hidden % 32)      // (TrainPath::use_x2)
    return d3dp_fail(D3DP_ENOTSUP, "D3DP_TRAIN_PASSES=1 exists for the split-fp16 training Linears; channels=%d%s trains on the fp32 path "
                              "(fp32-MFMA Linears have no one-pass form)", g.channels, f32 ? " under D3DP_TRAIN_IMPL=f32" : "");
  auto is = [](const char* name, const char* v) { const char* e = getenv(name); return e && !strcmp(e, v); };
  if (is("D3DP_TRAIN_WGRAD", "each") || is("D3DP_TRAIN_TAIL", "split") || is("D3DP_TRAIN_GELU", "pass") || is("D3DP_TRAIN_LN_OPERAND", "pass"))
    return d3dp_fail(D3DP_ENOTSUP, "D3DP_TRAIN_PASSES=1 beside D3DP_TRAIN_WGRAD=each / D3DP_TRAIN_TAIL=split / D3DP_TRAIN_GELU=pass / "
                              "D3DP_TRAIN_LN_OPERAND=pass: the superseded launch forms have no one-pass form");
  *passes = 1;
  return D3DP_OK;
}

// The environment switches of a context, read once at d3dp_create: the cross-check implementations, the training step's
// scheduling switches and the measurement switches of the experiment kernels.  `width_inst`: the width is one the matrix-core
// kernels are instantiated for, or one the split-fp16 implementation takes with padded heads under D3DP_EXACT_IMPL=f16x2
// (d3dp_create).  `train_split`: the training step may run on split-fp16 operands -- an instantiated width, or a TRAIN context
// that D3DP_TRAIN_IMPL=f16x2 opted in (d3dp_create); a decision of its own, so that neither switch changes what a context of the
// other mode does.  D3DP_OK, or the refusal (the caller deletes the context).
// (D3DP_TRAIN_ATTN_BWD alone is read per call, in train.hip: tests flip it between steps.)
int read_switches(d3dp_ctx* c, bool width_inst, bool train_split) {
  const d3dp_cfg& g = c->cfg;
  const char* xf = getenv("D3DP_EXACT_IMPL");
  c->exact_impl = c->exact_impl_req = (xf && !strcmp(xf, "bf16x3")) ? 1 : (xf && !strcmp(xf, "f32")) ? 2 : 0;
  if (!width_inst) {
    if (c->exact_impl_req == 1)
      return d3dp_fail(D3DP_ENOTSUP, "D3DP_EXACT_IMPL=bf16x3 exists for channels in {64,128,256,512}; channels=%d runs the fp32 implementation", g.channels);
    c->exact_impl = c->exact_impl_req = 2;
  }
  const char* lr = getenv("D3DP_LONG_ATTN");             // cross-check: clips > 256 frames on the fp32 row attention kernel
  c->long_rows = lr && !strcmp(lr, "rows");
  const char* nf = getenv("D3DP_NO_FOLD");               // cross-check: residual adds (and norm2) in the row kernels
  c->fold = !(nf && nf[0] == '1');
  const char* dn = getenv("D3DP_DEFER_NORM");            // cross-check: =0 keeps the shared norms in place in the norm pair
  c->defer = !(dn && dn[0] == '0');
  const char* ti = getenv("D3DP_TRAIN_IMPL");
  c->train_x2 = !(ti && !strcmp(ti, "f32")) && train_split;    // (a width outside the instantiated set, not opted in: the fp32 path)
  const char* ov = getenv("D3DP_TRAIN_OVERLAP");
  c->train_overlap = !(ov && ov[0] == '0');
  c->train_overlap_sets = (ov && ov[0] == '1') ? 1 : 2;
  const char* tg = getenv("D3DP_TRAIN_GELU");
  c->train_gelu_in_prep = !(tg && !strcmp(tg, "pass"));
  const char* tw = getenv("D3DP_TRAIN_WGRAD");
  c->train_wgrad_merged = !(tw && !strcmp(tw, "each"));
  const char* tl = getenv("D3DP_TRAIN_LN_OPERAND");       // =pass: round 5's operand pass behind every LayerNorm (variants build only)
  c->train_ln_direct = !(tl && !strcmp(tl, "pass"));
  const char* tt = getenv("D3DP_TRAIN_TAIL");
  c->train_tail_blocks = !(tt && !strcmp(tt, "split"));
  const char* ta = getenv("D3DP_TRAIN_ATTN");
  c->train_attn_x2 = (ta && !strcmp(ta, "f32")) ? 0 : (ta && !strcmp(ta, "x2t")) ? 1 : 2;
  // D3DP_TRAIN_WGRAD=each / D3DP_TRAIN_TAIL=split / D3DP_TRAIN_GELU=pass were round 5's same-box A/B switches: they make the
  // configs[4] shapes take the launch forms the library keeps for the shapes its merged / fused forms do not cover (widths below
  // 256, contractions that are not a multiple of 16 k-steps).  Measured and superseded: like the experiment
  // kernels below they are honoured by the `make variants` library only and REFUSED here -- never ignored.  (What stays: the
  // cross-check implementations D3DP_TRAIN_IMPL=f32, D3DP_TRAIN_ATTN=f32|x2t, D3DP_TRAIN_ATTN_BWD=valu, D3DP_EXACT_IMPL, D3DP_NO_FOLD,
  // and the profiling switch D3DP_TRAIN_OVERLAP=0|1: one stream, so that no kernel's duration contains a wait for CUs.)
  if ((!c->train_gelu_in_prep || !c->train_wgrad_merged || !c->train_tail_blocks || !c->train_ln_direct) && !d3dp_x2_variants_built())
    return d3dp_fail(D3DP_ENOTSUP, "D3DP_TRAIN_WGRAD=each / D3DP_TRAIN_TAIL=split / D3DP_TRAIN_GELU=pass / D3DP_TRAIN_LN_OPERAND=pass select superseded launch forms of the "
                              "training step that only the variants build honours (make -C d3dp_amd/csrc variants; "
                              "D3DP_LIB=d3dp_amd/lib/variants/libd3dp_variants.so)");
  {
    // Measurement switches of experiments that were measured and not adopted: the row-class skewed schedule
    // (D3DP_X2_SKEW=1|2|4), the ping-pong (D3DP_X2_PP=1) and wide (D3DP_X2_WIDE=1) forms of the EXACT Linear, norm2 folded into
    // proj / fc1 (D3DP_FOLD_LN=1), the sequence padding the skewed schedule needs (D3DP_SEQ_PAD).  Their kernels exist only in a
    // library built with -DD3DP_X2_VARIANTS=1 (`make variants`): the product library refuses the request instead of ignoring it.
    const char* sk = getenv("D3DP_X2_SKEW");
    const char* pp = getenv("D3DP_X2_PP");
    const char* wide = getenv("D3DP_X2_WIDE");
    const char* pd = getenv("D3DP_SEQ_PAD");
    const char* nl = getenv("D3DP_FOLD_LN");
    int skew_d = 0, pingpong = 0, pad = -1;
    if (sk && (sk[0] == '0' || sk[0] == '1' || sk[0] == '2' || sk[0] == '4') && sk[1] == 0) skew_d = sk[0] - '0';
    if (pp && (pp[0] == '0' || pp[0] == '1') && pp[1] == 0) pingpong = pp[0] - '0';
    if (wide && wide[0] == '1' && wide[1] == 0) pingpong = 2;
    if (pd && (pd[0] == '0' || pd[0] == '1') && pd[1] == 0) pad = pd[0] - '0';
    const bool fold_ln = nl && nl[0] == '1';
    if ((skew_d || pingpong || pad > 0 || fold_ln) && !d3dp_x2_variants_built())
      return d3dp_fail(D3DP_ENOTSUP, "D3DP_X2_SKEW / D3DP_X2_PP / D3DP_X2_WIDE / D3DP_SEQ_PAD / D3DP_FOLD_LN select experiment kernels that this "
                                "library was built without (make -C d3dp_amd/csrc variants; D3DP_LIB=d3dp_amd/lib/variants/libd3dp_variants.so)");
    c->skew_d = skew_d; c->pingpong = pingpong; c->pad_override = pad; c->fold_ln_on = fold_ln;
  }
  return D3DP_OK;
}

}  // namespace

extern "C" {

int d3dp_abi_version(void) { return D3DP_ABI_VERSION; }
// test hook (include/d3dp_hip.h, "test hooks"): 1 if this library carries the experiment kernels of gemm_x2.hip
int d3dp_debug_x2_variants(void) { return d3dp_x2_variants_built() ? 1 : 0; }
const char* d3dp_last_error(void) { return g_err.c_str(); }
const char* d3dp_profile_class_name(int32_t cls) {
  return (cls >= 0 && cls < D3DP_PROFILE_CLASSES) ? kClassNames[cls] : "";
}

int d3dp_create(const d3dp_cfg* cfg, d3dp_ctx** out) {
  if (!cfg || !out) return d3dp_fail(D3DP_EINVAL, "d3dp_create: null argument");
  const d3dp_cfg& g = *cfg;
  // (frames > 256: EXACT, FAST and FAST16 contexts take the chunked-key form of their attention kernels; at head dim 8 FAST / FAST16
  //  contexts stay on the row kernel -- fp32 arithmetic on their 2-byte rows -- and EXACT contexts on the fp32 kernels, at every clip
  //  length.  TRAIN contexts: the training step's split-fp16 attention (head dims 64, 32, 16: train_attn.hip) passes keys / queries
  //  through LDS in chunks and takes every length up to 1024; its fp32 attention -- head dim 8, the cross-check switches -- holds a
  //  whole sequence in LDS and d3dp_train_forward refuses more than 256 frames there; a TRAIN context of a width outside the
  //  instantiated set runs that fp32 attention with a run-time head dim and is refused BELOW beyond 256 tokens, 153 at head dims
  //  above 64 -- unless D3DP_TRAIN_IMPL=f16x2 opted it into the split-fp16 step (channels in {192, 320, 384, 448}, below): head dims
  //  24 / 40 / 48 / 56 then run padded forms of the split-fp16 attention and take every length up to 1024 too, and what the
  //  cross-check switches or head dim 8 leave on the fp32 attention there is refused by d3dp_train_forward like at every width.)
  if (g.frames < 1 || g.frames > 1024) return d3dp_fail(D3DP_ENOTSUP, "frames=%d not in [1,1024]", g.frames);
  // (more than 32 joints: the spatial axis takes the whole-sequence attention kernels the temporal axis runs on, round 6)
  if (g.joints < 1 || g.joints > 256) return d3dp_fail(D3DP_ENOTSUP, "joints=%d not in [1,256]", g.joints);
  if (g.heads < 1 || g.channels < 1 || g.channels % g.heads) return d3dp_fail(D3DP_EINVAL, "heads=%d does not divide channels=%d", g.heads, g.channels);
  if (g.depth < 1) return d3dp_fail(D3DP_EINVAL, "depth=%d", g.depth);
  if (g.mode != D3DP_MODE_EXACT && g.mode != D3DP_MODE_FAST && g.mode != D3DP_MODE_TRAIN && g.mode != D3DP_MODE_FAST16)
    return d3dp_fail(D3DP_EINVAL, "mode=%d", g.mode);
  const int hd = g.channels / g.heads;
  // The matrix-core kernels (split-fp16 / bf16 operands) and the row kernels around them are instantiated for the widths
  // {64, 128, 256, 512} with head dims {8, 16, 32, 64}: every configuration the reference publishes (`-cs 512`, README.md:33-39)
  // and its smaller powers of two.  The reference itself takes ANY `-cs` its 8 heads divide (common/arguments.py:49,
  // mixste.py:46-62): such a width runs EXACT mode on the fp32 implementation -- fp32-MFMA Linears (gemm_f32_kernel), the fp32
  // row attention with a run-time head dim, run-time-width row kernels (pointwise.hip *_g_kernel) -- i.e. the cross-check
  // implementation D3DP_EXACT_IMPL=f32 selects by hand for the instantiated widths: same tolerance, roughly a fifth of the
  // throughput.  A TRAIN context of such a width (the reference trains at any `-cs` too: main.py:325) takes the fp32 path of the
  // training step -- what D3DP_TRAIN_IMPL=f32 selects for the instantiated widths -- through the run-time-width row kernels of
  // train_g.hip and the VALU attention backward with a run-time head dim.  FAST / FAST16 contexts exist for the instantiated
  // widths and, under D3DP_FAST_IMPL=mfma, for channels in {192, 320, 384, 448} (below).
  const bool width_inst = (g.channels == 64 || g.channels == 128 || g.channels == 256 || g.channels == 512) &&
                          (hd == 8 || hd == 16 || hd == 32 || hd == 64) && g.hidden >= 64 && g.hidden % 64 == 0;
  // D3DP_EXACT_IMPL=f16x2 (opt-in): an EXACT context at channels in {192, 320, 384, 448} runs the split-fp16 implementation with
  // its head dim padded to 32 / 64 inside the packed weights (ctx.h hdp).  At an instantiated width the switch names the default;
  // anywhere else it cannot be honoured and is refused HERE, before the device is looked for -- never ignored.
  int hdp = 0;
  {
    const char* xi = getenv("D3DP_EXACT_IMPL");
    if (xi && !strcmp(xi, "f16x2") && !width_inst) {
      const bool shape = (g.channels == 192 || g.channels == 320 || g.channels == 384 || g.channels == 448) && hd % 8 == 0 &&
                         hd <= 64 && g.hidden >= 64 && g.hidden % 64 == 0;
      if (!shape || g.mode != D3DP_MODE_EXACT)
        return d3dp_fail(D3DP_ENOTSUP, "D3DP_EXACT_IMPL=f16x2 outside the instantiated widths exists for D3DP_MODE_EXACT contexts with channels in "
                                  "{192,320,384,448}, head dim a multiple of 8 up to 64 and hidden a multiple of 64; channels=%d heads=%d "
                                  "hidden=%d mode=%d is not one (unset the switch: such a context runs the fp32 implementation)",
                    g.channels, g.heads, g.hidden, g.mode);
      const char* lr = getenv("D3DP_LONG_ATTN");
      if (lr && !strcmp(lr, "rows"))
        return d3dp_fail(D3DP_ENOTSUP, "D3DP_LONG_ATTN=rows with D3DP_EXACT_IMPL=f16x2 at channels=%d: the run-time-head-dim row attention has no "
                                  "split-fp16 output form", g.channels);
      hdp = hd <= 32 ? 32 : 64;
    }
  }
  // D3DP_TRAIN_IMPL=f16x2 (opt-in; read for TRAIN contexts alone): a TRAIN context at the same widths takes the split-fp16 training
  // step -- X2Train's Linears take any N, K that are multiples of 32, the row kernels of train_g.hip leave the operand absmax
  // behind, and the attention runs on train_attn.hip with the head padded to 32 / 64 inside its LDS images (no weight, workspace or
  // Linear knows about the padding).  At an instantiated width the value names the default; anywhere else it is refused here.
  bool train_widths = false;
  if (g.mode == D3DP_MODE_TRAIN && !width_inst) {
    const char* ti = getenv("D3DP_TRAIN_IMPL");
    if (ti && !strcmp(ti, "f16x2")) {
      const bool shape = (g.channels == 192 || g.channels == 320 || g.channels == 384 || g.channels == 448) && hd % 8 == 0 &&
                         hd <= 64 && g.hidden >= 64 && g.hidden % 64 == 0;
      if (!shape)
        return d3dp_fail(D3DP_ENOTSUP, "D3DP_TRAIN_IMPL=f16x2 outside the instantiated widths exists for D3DP_MODE_TRAIN contexts with channels in "
                                  "{192,320,384,448}, head dim a multiple of 8 up to 64 and hidden a multiple of 64; channels=%d heads=%d "
                                  "hidden=%d is not one (unset the switch: such a context trains on the fp32 path)",
                    g.channels, g.heads, g.hidden);
      train_widths = true;
    }
  }
  // D3DP_FAST_IMPL=mfma (opt-in; read for FAST / FAST16 contexts alone): such a context at the same widths runs the mode's dataflow -- 2-byte
  // weights and activations, fp32 residual stream, both attentions and all four Linears on the matrix cores -- with the head dim padded
  // to 32 / 64 inside the packed 2-byte weights (ctx.h hdp).  hidden = 2 x channels (what MixSTE2 builds): the k-depths the streaming
  // Linear is instantiated for.  Head dims 24 / 40 / 48 / 56 (the model's 8 heads) are the ones the padded attention kernels carry the
  // exponent of (attention_fast_pad.hip); 32 and 64 (6 or 3 heads at 192, ...) need no padding and run the kernels of the instantiated
  // widths; 8 and 16 (12, 24, ... heads) have no kernel behind this route and are refused here.  At an instantiated width the value names the default; any other value, width or shape is refused
  // here, before the device is looked for -- never ignored.
  if (g.mode == D3DP_MODE_FAST || g.mode == D3DP_MODE_FAST16) {
    if (const char* fi = getenv("D3DP_FAST_IMPL")) {
      if (strcmp(fi, "mfma"))
        return d3dp_fail(D3DP_ENOTSUP, "D3DP_FAST_IMPL=%.32s: the one value a FAST / FAST16 context takes is D3DP_FAST_IMPL=mfma (channels=%d)", fi,
                    g.channels);
      if (!width_inst) {
        const bool shape = (g.channels == 192 || g.channels == 320 || g.channels == 384 || g.channels == 448) &&
                           (hd == 24 || hd == 32 || hd == 40 || hd == 48 || hd == 56 || hd == 64) && g.hidden == 2 * g.channels;
        if (!shape)
          return d3dp_fail(D3DP_ENOTSUP, "D3DP_FAST_IMPL=mfma outside the instantiated widths exists for FAST / FAST16 contexts with channels in "
                                    "{192,320,384,448}, head dim in {24,32,40,48,56,64} and hidden = 2 x channels; channels=%d heads=%d "
                                    "hidden=%d is not one (such a width runs in D3DP_MODE_EXACT / D3DP_MODE_TRAIN)",
                      g.channels, g.heads, g.hidden);
        const char* lr = getenv("D3DP_LONG_ATTN");
        if (lr && !strcmp(lr, "rows"))
          return d3dp_fail(D3DP_ENOTSUP, "D3DP_LONG_ATTN=rows with D3DP_FAST_IMPL=mfma at channels=%d: the row attention kernel would take the padded "
                                    "head dim for its exponent", g.channels);
        hdp = hd <= 32 ? 32 : 64;
      }
    }
  }
  // D3DP_FAST16_RANGE=scale (opt-in; read for FAST16 contexts alone): a block whose proven bound reaches 65504 stores the tensors that
  // bound covers at a power-of-two multiple of their value instead of moving the whole context to bf16 (ctx.h fast16_scale; chosen at
  // d3dp_set_weights).  The scaled kernels exist on the matrix-core route of the instantiated widths: the streaming Linear at K / 64
  // in {1, 2, 4, 8, 16}, the three attention kernels at head dims 64 / 32 / 16, the row kernels at widths 64 ... 512.  Any other value,
  // head dim 8 and the row attention kernel (no scaled form), and the padded widths of D3DP_FAST_IMPL=mfma are refused here, before
  // the device is looked for -- never ignored.
  bool fast16_scale = false;
  if (g.mode == D3DP_MODE_FAST16) {
    if (const char* fr = getenv("D3DP_FAST16_RANGE")) {
      if (strcmp(fr, "scale"))
        return d3dp_fail(D3DP_ENOTSUP, "D3DP_FAST16_RANGE=%.32s: the one value a FAST16 context takes is D3DP_FAST16_RANGE=scale", fr);
      if (hdp)
        return d3dp_fail(D3DP_ENOTSUP, "D3DP_FAST16_RANGE=scale with D3DP_FAST_IMPL=mfma at channels=%d: the padded-head kernels have no scaled "
                                  "form", g.channels);
      if (width_inst && !mfma_head_dim(hd))
        return d3dp_fail(D3DP_ENOTSUP, "D3DP_FAST16_RANGE=scale at head dim %d (channels=%d heads=%d): the scaled attention kernels exist at head "
                                  "dims 64, 32 and 16", hd, g.channels, g.heads);
      const char* lr = getenv("D3DP_LONG_ATTN");
      if (width_inst && lr && !strcmp(lr, "rows"))
        return d3dp_fail(D3DP_ENOTSUP, "D3DP_FAST16_RANGE=scale with D3DP_LONG_ATTN=rows: the row attention kernel has no scaled form");
      auto depth = [](int k) { return k == 64 || k == 128 || k == 256 || k == 512 || k == 1024; };
      if (width_inst && !depth(g.hidden))
        return d3dp_fail(D3DP_ENOTSUP, "D3DP_FAST16_RANGE=scale with hidden=%d: the scaled streaming Linear exists at k-depths 64, 128, 256, 512 "
                                  "and 1024", g.hidden);
      fast16_scale = width_inst;         // (any other width: refused below like every FAST16 context there)
    }
  }
  if (!width_inst && !hdp) {
    if (g.mode == D3DP_MODE_FAST)
      return d3dp_fail(D3DP_ENOTSUP, "channels=%d heads=%d hidden=%d: FAST contexts exist for channels in {64,128,256,512} with head dim in "
                                "{8,16,32,64} and hidden a multiple of 64; other widths run in D3DP_MODE_EXACT / D3DP_MODE_TRAIN (fp32 implementation)",
                  g.channels, g.heads, g.hidden);
    if (g.mode == D3DP_MODE_FAST16)
      return d3dp_fail(D3DP_ENOTSUP, "channels=%d heads=%d hidden=%d: FAST16 contexts exist for the shapes FAST contexts exist for -- channels in "
                                "{64,128,256,512} with head dim in {8,16,32,64} and hidden a multiple of 64; other widths run in D3DP_MODE_EXACT / "
                                "D3DP_MODE_TRAIN (fp32 implementation)",
                  g.channels, g.heads, g.hidden);
    if (g.channels > 1024 || g.channels % 4 || hd % 4 || hd > 128 || g.hidden < 4 || g.hidden % 4)
      return d3dp_fail(D3DP_ENOTSUP, "channels=%d heads=%d hidden=%d: the fp32 implementation takes channels <= 1024, head dim a multiple of 4 up to 128 "
                                "and hidden a multiple of 4", g.channels, g.heads, g.hidden);
    // (the fp32 attention backward holds two whole-sequence images of its capacity head dim + the statistics in the CU's 160 KiB)
    const int nmax = std::max(g.frames, g.joints), cap = hd <= 16 ? 16 : hd <= 32 ? 32 : hd <= 64 ? 64 : 128;
    if (g.mode == D3DP_MODE_TRAIN && !train_widths && (nmax > 256 || (size_t)nmax * (8 * (cap + 4) + 12) > 160 * 1024))
      return d3dp_fail(D3DP_ENOTSUP, "channels=%d heads=%d frames=%d joints=%d: training at a width outside {64,128,256,512} runs the fp32 attention "
                                "backward, which holds a whole sequence in LDS (<= 256 tokens; <= 153 at head dims above 64)",
                  g.channels, g.heads, g.frames, g.joints);
  }
  int train_passes = 3;
  if (const int rc = read_train_passes(g, width_inst || hdp != 0 || train_widths, &train_passes); rc != D3DP_OK) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return d3dp_fail(D3DP_EHIP, "no HIP device visible: libd3dp_hip has no CPU fallback");
  d3dp_ctx* c = new d3dp_ctx();
  c->cfg = g;
  c->fast_f16 = c->fast16() ? 1 : (c->fast() ? D3DP_FAST_F16 : 0);   // (FAST16: until d3dp_set_weights has seen the weights)
  c->hdp = hdp;
  c->fast16_scale = fast16_scale;
  c->train_passes = train_passes;
  if (const int rc = read_switches(c, width_inst || hdp != 0, width_inst || hdp != 0 || train_widths); rc != D3DP_OK) {
    delete c;
    return rc;
  }
  HIP_TRY(hipGetDevice(&c->device));
  {
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, c->device));
    c->n_cu = prop.multiProcessorCount;
  }
  if (hipMalloc((void**)&c->d_flag, sizeof(unsigned)) != hipSuccess || hipMemset(c->d_flag, 0, sizeof(unsigned)) != hipSuccess) {
    delete c;
    return d3dp_fail(D3DP_EHIP, "d3dp_create: cannot allocate the status word");
  }
  // The second stream of d3dp_train_backward and its events are made HERE, not on the first step: d3dp_train_backward then creates
  // nothing, and even a context's first step keeps the header's "does not allocate" (tests/test_hip_streams.py).
  // (exactly the contexts whose backward pass forks: split-fp16 Linears and D3DP_TRAIN_OVERLAP not 0)
  if (TrainPath(*c).needs_aux) {
    bool ok = hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) == hipSuccess;
    for (hipEvent_t& e : c->ev_done) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
      (void)d3dp_destroy(c);
      return d3dp_fail(D3DP_EHIP, "d3dp_create: cannot create the training step's second stream and its events");
    }
  }
  *out = c;
  return D3DP_OK;
}

int d3dp_destroy(d3dp_ctx* c) {
  if (!c) return D3DP_OK;
  for (auto& e : c->pool) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  if (c->arena) (void)hipFree(c->arena);
  if (c->d_flag) (void)hipFree(c->d_flag);
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  for (hipEvent_t e : c->ev_done)
    if (e) (void)hipEventDestroy(e);
  if (c->aux) (void)hipStreamDestroy(c->aux);
  delete c;
  return D3DP_OK;
}

int d3dp_status(d3dp_ctx* c, int32_t* nonfinite) {
  if (!c || !nonfinite) return d3dp_fail(D3DP_EINVAL, "d3dp_status: null argument");
  unsigned v = 0;
  HIP_TRY(hipDeviceSynchronize());                     // every d3dp_denoise issued so far has written its verdict
  HIP_TRY(hipMemcpy(&v, c->d_flag, sizeof v, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(c->d_flag, 0, sizeof v));
  *nonfinite = (int32_t)(v != 0u);                     // bit 0: inf / nan in an output; bit 1: an operand left the split range
  return D3DP_OK;
}

int d3dp_ddim_pre(const float* img, float* xt2, const int32_t* perm, float scale, int32_t B, int32_t H, int32_t F,
                  int32_t J, void* stream) {
  if (!img || !xt2 || !perm || B < 1) return d3dp_fail(D3DP_EINVAL, "d3dp_ddim_pre: bad argument");
  LAUNCH_TRY(d3dp_launch_ddim_pre(img, xt2, perm, scale, B, H * F * J * 3, J, (hipStream_t)stream));
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

int d3dp_ddim_post(const float* pred2, const float* img, const float* noise, const int32_t* perm, float scale,
                   double sqrt_recip, double sqrt_recipm1, float c_xstart, float c_noise, float sigma, int32_t last,
                   float* x_start, size_t xs_bstride, float* img_next, int32_t B, int32_t H, int32_t F, int32_t J,
                   void* stream) {
  if (!pred2 || !perm || !x_start || B < 1) return d3dp_fail(D3DP_EINVAL, "d3dp_ddim_post: bad argument");
  if (!last && (!img || !noise || !img_next)) return d3dp_fail(D3DP_EINVAL, "d3dp_ddim_post: img/noise/img_next required");
  LAUNCH_TRY(d3dp_launch_ddim_post(pred2, img, noise, perm, scale, sqrt_recip, sqrt_recipm1, c_xstart, c_noise, sigma,
                                   last, x_start, xs_bstride, img_next, B, H * F * J * 3, J, (hipStream_t)stream));
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

int d3dp_q_sample(const float* x0, const float* noise, const double* a, const double* s, float scale, float* out,
                  int32_t B, int32_t per_b, void* stream) {
  if (!x0 || !noise || !a || !s || !out || B < 1 || per_b < 1) return d3dp_fail(D3DP_EINVAL, "d3dp_q_sample: bad argument");
  LAUNCH_TRY(d3dp_launch_q_sample(x0, noise, a, s, scale, out, B, per_b, (hipStream_t)stream));
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

int d3dp_jpma(const float* pred, const float* traj, const float* cam, const float* gt2d, const float* gt3d, float* agg,
              int32_t* sel, float* err_sel, float* err_min, int32_t B, int32_t K, int32_t H, int32_t F, int32_t J,
              int32_t zero_root, void* stream) {
  if (!pred || !traj || !cam || !gt2d || !agg || B < 1 || K < 1 || H < 1)
    return d3dp_fail(D3DP_EINVAL, "d3dp_jpma: bad argument");
  if ((err_sel || err_min) && !gt3d) return d3dp_fail(D3DP_EINVAL, "d3dp_jpma: error outputs need gt3d");
  LAUNCH_TRY(d3dp_launch_jpma(pred, traj, cam, gt2d, gt3d, agg, sel, err_sel, err_min, nullptr, nullptr, nullptr, 0, B,
                              K, H, F, J, zero_root ? 0 : -1, 0, (hipStream_t)stream));
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

int d3dp_jpma_gathered(const float* gathered, const float* traj, const float* cam, const float* gt2d, const float* gt3d,
                       float* agg, int32_t* sel, float* err_sel, float* err_min, int32_t R, int32_t B, int32_t K,
                       int32_t H_local, int32_t F, int32_t J, int32_t zero_root, void* stream) {
  if (!gathered || !traj || !cam || !gt2d || !agg || R < 1 || B < 1 || K < 1 || H_local < 1)
    return d3dp_fail(D3DP_EINVAL, "d3dp_jpma_gathered: bad argument");
  if ((err_sel || err_min) && !gt3d) return d3dp_fail(D3DP_EINVAL, "d3dp_jpma_gathered: error outputs need gt3d");
  LAUNCH_TRY(d3dp_launch_jpma(gathered, traj, cam, gt2d, gt3d, agg, sel, err_sel, err_min, nullptr, nullptr, nullptr, 0, B,
                              K, R * H_local, F, J, zero_root ? 0 : -1, 0, (hipStream_t)stream, H_local,
                              (size_t)B * K * H_local * F * J * 3));
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

int d3dp_jpma_ex(const float* pred, const float* traj, const float* cam, const float* gt2d, const float* gt3d, float* agg,
                 int32_t* sel, float* err_sel, float* err_min, float* jbest, float* mean, int32_t B, int32_t K, int32_t H,
                 int32_t F, int32_t J, int32_t root_joint, int32_t linear_projection, void* stream) {
  if (!pred || !traj || !cam || !gt2d || B < 1 || K < 1 || H < 1 || root_joint >= J)
    return d3dp_fail(D3DP_EINVAL, "d3dp_jpma_ex: bad argument");
  if ((err_sel || err_min || jbest) && !gt3d) return d3dp_fail(D3DP_EINVAL, "d3dp_jpma_ex: error / J-Best outputs need gt3d");
  LAUNCH_TRY(d3dp_launch_jpma(pred, traj, cam, gt2d, gt3d, agg, sel, err_sel, err_min, nullptr, jbest, mean, 0, B, K, H,
                              F, J, root_joint, linear_projection, (hipStream_t)stream));
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

int d3dp_jpma_winners(const float* pred, const float* traj, const float* cam, const float* gt2d, float* win,
                      int32_t h_offset, int32_t B, int32_t K, int32_t H, int32_t F, int32_t J, int32_t zero_root,
                      void* stream) {
  if (!pred || !traj || !cam || !gt2d || !win || B < 1 || K < 1 || H < 1 || h_offset < 0)
    return d3dp_fail(D3DP_EINVAL, "d3dp_jpma_winners: bad argument");
  LAUNCH_TRY(d3dp_launch_jpma(pred, traj, cam, gt2d, nullptr, nullptr, nullptr, nullptr, nullptr, win, nullptr, nullptr,
                              h_offset, B, K, H, F, J, zero_root ? 0 : -1, 0, (hipStream_t)stream));
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

int d3dp_profile_enable(d3dp_ctx* c, int32_t on) {
  if (!c) return d3dp_fail(D3DP_EINVAL, "null ctx");
  c->prof = on != 0;
  c->used = 0;
  memset(c->counts, 0, sizeof c->counts);
  for (auto& v : c->total_ms) v = 0.0;
  return D3DP_OK;
}

int d3dp_profile_read(d3dp_ctx* c, int64_t* counts, double* total_ms) {
  if (!c || !counts || !total_ms) return d3dp_fail(D3DP_EINVAL, "null argument");
  if (c->flush_events() != 0) return d3dp_fail(D3DP_EHIP, "event read failed");
  for (int i = 0; i < D3DP_PROFILE_CLASSES; ++i) { counts[i] = c->counts[i]; total_ms[i] = c->total_ms[i]; }
  memset(c->counts, 0, sizeof c->counts);
  for (auto& v : c->total_ms) v = 0.0;
  return D3DP_OK;
}

}  // extern "C"
