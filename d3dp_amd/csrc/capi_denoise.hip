// The inference schedule (d3dp_denoise): which kernels run in which order over which regions of the caller's workspace
// (InferLayout), and which attention kernel family a context launches (attn_route).
// Data layout in HBM, per internal pass over `n` (clip, hypothesis) sequences, Tc = n*F*J tokens in (sequence, frame, joint) order:
//   x    [Tc, C]   fp32  residual stream -- fp32 in every mode
//   bufA [Tc, C]   act   normalised input of the next Linear / attention output: bf16 FAST, fp16 FAST16; EXACT: split-fp16 h2i rows
//                        (two fp16 planes interleaved in 32-column blocks); fp32 / 3 bf16 planes in the f32 / bf16x3 cross-checks
//   bufB [Tc, 3C]  act   qkv (EXACT: the packed rows of the split-fp16 attention kernels); reused as the [Tc, hidden] MLP hidden
//   y1,y [Tc, C]   act   proj / fc2 outputs that the next row kernel adds to x: FAST modes and EXACT cross-checks.  EXACT split-fp16
//                        adds them in the proj / fc2 epilogues (x += ...) and leaves both regions unused
// A padded-head context (D3DP_EXACT_IMPL=f16x2 at channels 192 / 320 / 384 / 448, ctx.h hdp): qkv rows hold 3 Cp columns and the
// attention output Cp = heads x hdp, so bufA holds max(C, Cp) columns (LayerNorm rows at pitch 2 C, attention output rows at pitch
// 2 Cp fp16) and bufB max(3 Cp, hidden).  The same under D3DP_FAST_IMPL=mfma in the FAST modes: 2-byte rows of C, Cp and 3 Cp columns.
// The reference keeps two physical layouts and transposes between them 16 times per call (mixste.py:244,270,274); here spatial
// and temporal attention both index the single layout by stride.
#include "ctx.h"

// Which attention kernel family runs, from the facts of a context and the axis (0 = spatial, 1 = temporal).
//   X2              split-fp16 operands on the fp16 matrix cores, packed qkv rows (attention_x2.hip): EXACT f16x2 at head dims 64, 32, 16
//                   (`-cs` 512 / 256 / 128 with the model's 8 heads), both axes.  Up to 256 frames (every BASELINE configuration) the
//                   temporal kernel holds a whole sequence's K / V images in LDS; longer clips (`-f 351`, reference
//                   common/arguments.py:58, mixste.py:172) take the flash form of the same arithmetic (attn_temporal_x2_long_kernel:
//                   keys in chunks of 128 under an online softmax; round 5 ran both attentions of such clips on the chunked fp32
//                   VALU row kernel, ten times the cost per FLOP)
//   FAST_SPATIAL    FAST / FAST16, spatial axis, up to 32 joints (attention_fast.hip)
//   FAST_WHOLE_SEQ  FAST / FAST16 whole-sequence kernel: the temporal axis (chunked keys beyond 256 frames), and the spatial axis
//                   with more than 32 joints (it takes any SeqMap)
//   F32_TEMPORAL    fp32 matrix cores: the temporal axis of an EXACT context off the X2 route, head dim 64, up to 256 frames
//   ROWS            the fp32 VALU row kernel (fp32 arithmetic on whatever rows the context stores): everything else -- head dim 8
//                   and every head dim outside {64, 32, 16} in every mode
// D3DP_LONG_ATTN=rows (long_rows) keeps ROWS as a cross-check: at head dim 64 only for more than 256 frames and, in the FAST
// modes, for more than 32 joints; at head dims 32 and 16 for EVERY shape, in EXACT as in the FAST modes -- what such a context
// launched before these head dims had matrix-core kernels, i.e. the A/B handle.
AttnRoute attn_route(int mode, int exact_impl, int hd, int frames, int joints, bool long_rows, int axis) {
  const bool fast = mode == D3DP_MODE_FAST || mode == D3DP_MODE_FAST16, exact = mode == D3DP_MODE_EXACT;
  const bool mfma = hd == 64 || (mfma_head_dim(hd) && !long_rows);        // (hd 64: the switch acts per shape, below)
  if (exact && exact_impl == 0 && mfma && (hd != 64 || frames <= 256 || !long_rows)) return AttnRoute::X2;
  if (fast && mfma) {
    if (axis == 0 && joints <= 32) return AttnRoute::FAST_SPATIAL;
    if (axis == 0 ? !long_rows : (frames <= 256 || !long_rows)) return AttnRoute::FAST_WHOLE_SEQ;
  }
  if (axis == 1 && exact && hd == 64 && frames <= 256) return AttnRoute::F32_TEMPORAL;
  return AttnRoute::ROWS;
}

namespace {

// The caller's workspace of a d3dp_denoise call: byte offsets of its regions, for passes of up to min(chunk(), B H) sequences.
// One function serves the size query and the carve.  lnst / ln_rowstat (fold_ln: slice statistics [Tc][C / 64][2], then (mean,
// rstd) [Tc + 256][2]) and nstat (defer_norm: (mean, rstd) [Tc + 256][2], written by every deferring norm pair for the rows of
// its pass and read by the proj behind it for those rows alone; the tile of slack is fetched into LDS by proj's loaders, which
// fetch whole tiles, and never used) take no bytes in a context without them.
struct InferLayout {
  size_t temb, x, y1, y, bufA, bufB, lnst, ln_rowstat, nstat, total;
  InferLayout(const d3dp_ctx* c, int B, int H) {
    const d3dp_cfg& g = c->cfg;
    const size_t Tc = (size_t)std::min(c->chunk(), B * H) * c->seq_pitch(), C = g.channels, Cp = c->cp();   // (Cp = C without padded heads)
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes); return o; };
    temb = take((size_t)B * C * 4);
    x = take(Tc * C * 4);
    y1 = take(Tc * C * c->y_size());
    y = take(Tc * C * c->y_size());
    bufA = take(Tc * std::max(C, Cp) * c->act_size());
    bufB = take(Tc * std::max(3 * Cp, (size_t)g.hidden) * c->wide_size());   // (qkv fp32 = 12C; hidden planes <= 12C)
    lnst = take(c->fold_ln() ? Tc * ((C + 63) / 64) * 8 : 0);
    ln_rowstat = take(c->fold_ln() ? (Tc + 256) * 8 : 0);
    nstat = take(c->defer_norm() ? (Tc + 256) * 8 : 0);
    total = off;
  }
};

// out = epi(A W^T + bias).  out_f32: fp32 output even in FAST mode (the Linear outputs that feed a residual add).
// EXACT f16x2: `a_scale` = the scale the A operand was written at, `o_scale` = the scale of a plane output (BlockDev).
int linear(d3dp_ctx* c, int cls, int epi, int out_f32, const void* A, const void* W, float wu, const float* bias, void* out,
           int M, int N, int K, hipStream_t st, void* out2 = nullptr, float* aux = nullptr, float a_scale = kActScale,
           float o_scale = kActScale) {
  Scope s(c, cls, st);
  if (c->fast()) return d3dp_launch_linear_bf16_stream(epi, out_f32, A, W, bias, out, M, N, K, st, c->fast_f16);
  if (c->x2()) {
    // the qkv Linear writes the packed rows of the split-fp16 attention kernels (K and V already as fp16 planes)
    if (cls == P_QKV && c->x2_attn()) epi = EPI_QKV_PACK;
    // qkv and fc1 (epilogues without loads) run the skewed schedule when the context has it on (seq_pitch() pads for it)
    const int skew_d = c->skew() && (epi == EPI_QKV_PACK || epi == EPI_GELU) ? c->skew_d : 0;
    // proj walks its tiles from the LAST row of tiles to the first: the norm2 row kernel that follows starts at row 0, on the
    // rows of x this launch wrote last (its first 6 us run warm: -9.6 % cycles at -1 % L2 fetches).  Same tiles, same arithmetic.
    // Measured on two boxes: layernorm class 276 -> 254 / 279 -> 253 ms per step, proj -5, step -0.45 %; the same order on
    // fc2 (norm pair +28 ms), fc1, qkv or the row kernels themselves: neutral or worse (profiles/r06_tile_order_ab.md)
    const int rev = cls == P_PROJ ? X2_TILES_LAST_TO_FIRST : 0;
    return d3dp_launch_linear_f16x2(epi, A, W, bias, wu / a_scale, o_scale, (float*)out, out2 ? out2 : out, aux, c->d_flag, M, N,
                                    K, st, skew_d, c->pingpong | rev);
  }
  if (c->x3()) return d3dp_launch_linear_bf16x3(epi, A, W, bias, (float*)out, out, M, N, K, st);
  return d3dp_launch_linear_f32(epi, (const float*)A, (const float*)W, bias, (float*)out, M, N, K, st);
}

// A FAST16 Linear of a block under D3DP_FAST16_RANGE=scale: the A operand holds 2^-r_in times its value (0: a LayerNorm output, never
// scaled) and the fp16 rows leave at 2^-r_out.  Both 0: the plain kernel, as in every other context.
int linear_f16(d3dp_ctx* c, int cls, int epi, int r_in, int r_out, const void* A, const void* W, const float* bias, void* out, int M, int N,
               int K, hipStream_t st) {
  if (r_in == 0 && r_out == 0) return linear(c, cls, epi, 0, A, W, 1.f, bias, out, M, N, K, st);
  Scope s(c, cls, st);
  return d3dp_linear_stream_scaled(epi, A, W, bias, out, M, N, K, st, ldexpf(1.f, r_in - r_out), ldexpf(1.f, -r_out), ldexpf(1.f, r_out));
}

// (r_qkv: BlockDev's -- q, k and v at 2^-r_qkv in a FAST16 context under D3DP_FAST16_RANGE=scale; 0 everywhere else)
int attention(d3dp_ctx* c, int axis, const void* qkv, void* out, int n_bh, float s_kv, hipStream_t st, int r_qkv = 0) {
  const d3dp_cfg& g = c->cfg;
  Scope s(c, axis == 0 ? P_ATTN_S : P_ATTN_T, st);
  // (seq_pitch() exceeds F J on the X2 route alone: every other kernel sees the unpadded map)
  // (a padded-head context: rows of attn_cols() = heads x hdp columns, the true head dim in the softmax exponent)
  const int n = axis == 0 ? n_bh * g.frames : n_bh * g.joints, act = c->act(), C = c->attn_cols();
  const SeqMap map = axis == 0 ? spatial_map(g.frames, g.joints, c->seq_pitch()) : temporal_map(g.frames, g.joints, c->seq_pitch());
  if (r_qkv != 0) {          // (d3dp_create let the switch through for the matrix-core routes alone)
    const AttnRoute r = c->route(axis);
    if (r != AttnRoute::FAST_SPATIAL && r != AttnRoute::FAST_WHOLE_SEQ) return -2;
    return d3dp_attn_fast_scaled(r == AttnRoute::FAST_SPATIAL ? 0 : 1, qkv, out, n, map, C, g.heads, st, ldexpf(1.f, 2 * r_qkv));
  }
  switch (c->route(axis)) {
    case AttnRoute::X2: return d3dp_launch_attn_x2(3, axis, qkv, out, n, map, C, g.heads, s_kv, st, g.channels / g.heads);
    case AttnRoute::FAST_SPATIAL: return d3dp_launch_attn_spatial_bf16(qkv, out, n, map, C, g.heads, st, c->fast_f16, g.channels / g.heads);
    case AttnRoute::FAST_WHOLE_SEQ: return d3dp_launch_attn_temporal_bf16(qkv, out, n, map, C, g.heads, st, c->fast_f16, g.channels / g.heads);
    case AttnRoute::F32_TEMPORAL: return d3dp_launch_attn_temporal_f32(act, qkv, out, n, map, C, g.heads, st);
    case AttnRoute::ROWS: break;
  }
  return d3dp_launch_attn_rows(act, qkv, out, n, map, C, g.heads, st);
}

// x = x + proj(attn(qkv(xn)));  x = x + fc2(gelu(fc1(LN2(x))))        (mixste.py:113-115)
// The two residual adds are not done by the GEMMs: each residual-feeding Linear writes y = A W^T + b (fp32) and the
// (activation type: bf16 in FAST mode, fp16 in FAST16 -- one more 2-byte rounding on the branch output, none on the fp32 residual
// stream itself) and the next row-wise kernel (LN2 here; the norm pair / head in the caller) performs x += y while it has the row in
// registers anyway.  On return y1 / y hold the proj / fc2 outputs that the CALLER's next kernel must add to x.
// nstat: non-null if the norm pair in front of the block DEFERRED its shared norm (d3dp_ctx::defer_norm): x is still
// un-normalised, (mean, rstd) per row are there, and proj applies the norm as it adds (gamma / beta behind its bias: w.proj_bgb).
int run_block(d3dp_ctx* c, const BlockDev& w, int axis, float* x, void* y1, void* y, void* bufA, void* bufB, float* slices,
              float* rowstat, int n_bh, hipStream_t st, float* nstat = nullptr) {
  const d3dp_cfg& g = c->cfg;
  const int Tc = n_bh * c->seq_pitch(), C = g.channels, Ca = c->attn_cols();   // Ca: columns of q / k / v and of the attention output
  // (s_kv / s_h differ from kActScale only in EXACT f16x2 contexts whose weights asked for it, and s_kv only with the x2
  //  attention kernels: the other attention kernels write their output planes at kActScale)
  const float s_o = c->x2_attn() ? w.s_kv : kActScale;
  if (w.r_qkv | w.r_proj | w.r_h | w.r_fc2) {
    // FAST16 under D3DP_FAST16_RANGE=scale, a block with a bound beyond 65504: the FAST dataflow below with this block's four
    // multipliers (BlockDev::r_*).  proj takes the attention output's scale out as it applies its own, fc2 the hidden's; norm2 adds
    // y1 2^r_proj, and the caller's norm pair / head adds y1 2^r_proj and y 2^r_fc2.  A class whose exponent is 0 runs the plain kernel.
    LAUNCH_TRY(linear_f16(c, P_QKV, EPI_BIAS, 0, w.r_qkv, bufA, w.qkv_w, w.qkv_b, bufB, Tc, 3 * Ca, C, st));
    LAUNCH_TRY(attention(c, axis, bufB, bufA, n_bh, s_o, st, w.r_qkv));
    LAUNCH_TRY(linear_f16(c, P_PROJ, EPI_BIAS, w.r_qkv, w.r_proj, bufA, w.proj_w, w.proj_b, y1, Tc, C, Ca, st));
    {
      Scope s(c, P_LN, st);
      if (w.r_proj) LAUNCH_TRY(d3dp_launch_ln_scaled(x, y1, ldexpf(1.f, w.r_proj), w.n2w, w.n2b, g.eps_block, bufA, Tc, C, st));
      else LAUNCH_TRY(d3dp_launch_ln(c->act(), x, y1, 0, w.n2w, w.n2b, g.eps_block, bufA, Tc, C, st));
    }
    LAUNCH_TRY(linear_f16(c, P_FC1, EPI_GELU, 0, w.r_h, bufA, w.fc1_w, w.fc1_b, bufB, Tc, g.hidden, C, st));
    LAUNCH_TRY(linear_f16(c, P_FC2, EPI_BIAS, w.r_h, w.r_fc2, bufB, w.fc2_w, w.fc2_b, y, Tc, C, g.hidden, st));
    return 0;
  }
  LAUNCH_TRY(linear(c, P_QKV, EPI_BIAS, 0, bufA, w.qkv_w, w.qkv_u, w.qkv_b, bufB, Tc, 3 * Ca, C, st, nullptr, nullptr, kActScale, s_o));
  LAUNCH_TRY(attention(c, axis, bufB, bufA, n_bh, s_o, st));
  const bool fold = c->fold_resid();   // EXACT split-fp16 Linears: x += proj / fc2 inside their epilogues
  if (c->fold_ln()) {
    // norm2 folded into proj's epilogue (statistics, un-normalised operand -> y1) and fc1's (normalisation): no row kernel
    // (slices [Tc][C / 64][2], rowstat [Tc + 256][2]: InferLayout)
    LAUNCH_TRY(linear(c, P_PROJ, EPI_RESID_LN, 0, bufA, w.proj_w, w.proj_u, w.proj_b, x, Tc, C, Ca, st, y1, slices, s_o));
    {
      Scope s(c, P_LN, st);
      d3dp_launch_ln_combine(slices, rowstat, Tc, C, g.eps_block, st);
    }
    LAUNCH_TRY(linear(c, P_FC1, EPI_GELU_LN, 0, y1, w.fc1_w, w.fc1_u, w.fc1_c12, bufB, Tc, g.hidden, C, st, bufB, rowstat, kActScale, w.s_h));
  } else {
  if (nstat) LAUNCH_TRY(linear(c, P_PROJ, EPI_RESID_NORM, 0, bufA, w.proj_w, w.proj_u, w.proj_bgb, x, Tc, C, Ca, st, nullptr, nstat, s_o));
  else LAUNCH_TRY(linear(c, P_PROJ, fold ? EPI_RESID : EPI_BIAS, 0, bufA, w.proj_w, w.proj_u, w.proj_b, fold ? (void*)x : y1, Tc, C, Ca, st, nullptr, nullptr, s_o));
  {
    Scope s(c, P_LN, st);      // xn = LN2(x + y1); x itself stays untouched (the caller's norm pair adds y1 and y)
    LAUNCH_TRY(d3dp_launch_ln(c->act(), x, fold ? nullptr : y1, 0, w.n2w, w.n2b, g.eps_block, bufA, Tc, C, st));
  }
  LAUNCH_TRY(linear(c, P_FC1, EPI_GELU, 0, bufA, w.fc1_w, w.fc1_u, w.fc1_b, bufB, Tc, g.hidden, C, st, nullptr, nullptr, kActScale, w.s_h));
  }
  LAUNCH_TRY(linear(c, P_FC2, fold ? EPI_RESID : EPI_BIAS, 0, bufB, w.fc2_w, w.fc2_u, w.fc2_b, fold ? (void*)x : y, Tc, C, g.hidden, st, nullptr, nullptr, w.s_h));
  return 0;
}

}  // namespace

extern "C" {

int d3dp_workspace_bytes(const d3dp_ctx* c, int32_t B, int32_t H, size_t* bytes) {
  if (!c || !bytes || B < 1 || H < 1) return d3dp_fail(D3DP_EINVAL, "d3dp_workspace_bytes: bad argument");
  *bytes = InferLayout(c, B, H).total;
  return D3DP_OK;
}

int d3dp_denoise(d3dp_ctx* c, const float* x2d, const float* x_t, const int64_t* t, float* out, int32_t B, int32_t H,
                 void* workspace, size_t workspace_bytes, void* stream) {
  if (!c || !x2d || !x_t || !t || !out || !workspace || B < 1 || H < 1)
    return d3dp_fail(D3DP_EINVAL, "d3dp_denoise: bad argument");
  if (!c->weights_set) return d3dp_fail(D3DP_ESTATE, "d3dp_denoise: weights not set");
  const InferLayout L(c, B, H);
  if (workspace_bytes < L.total) return d3dp_fail(D3DP_ESTATE, "workspace %zu < required %zu bytes", workspace_bytes, L.total);
  hipStream_t st = (hipStream_t)stream;
  const d3dp_cfg& g = c->cfg;
  const int C = g.channels, F = g.frames, J = g.joints, FJ = F * J, SP = c->seq_pitch(), BH = B * H;
  char* const ws = (char*)workspace;
  float *temb = (float*)(ws + L.temb), *x = (float*)(ws + L.x), *slices = (float*)(ws + L.lnst), *rowstat = (float*)(ws + L.ln_rowstat);
  void *y1 = ws + L.y1, *y = ws + L.y, *bufA = ws + L.bufA, *bufB = ws + L.bufB;
  float* nstat = c->defer_norm() ? (float*)(ws + L.nstat) : nullptr;       // (null: no boundary defers its shared norm)

  {
    Scope s(c, P_TIME, st);
    LAUNCH_TRY(d3dp_launch_time_mlp(t, c->freq, c->t1w, c->t1b, c->t3w, c->t3b, temb, B, C, st));
  }
  int seq0 = 0;
  for (const int n : c->plan(BH)) {
    const int Tc = n * SP;
    {
      Scope s(c, P_EMBED, st);
      LAUNCH_TRY(d3dp_launch_embed_ln(c->act(), x2d, x_t, temb, c->ew, c->eb, c->spos, c->ste[0].n1w, c->ste[0].n1b,
                                      g.eps_block, x, bufA, seq0, n, H, F, J, C, st, SP));
    }
    const bool fold = c->fold_resid();
    for (int d = 0; d < g.depth; ++d) {
      // (the boundary in front of STE block d >= 1 deferred Temporal_norm; the one in front of TTE block d >= 1 Spatial_norm)
      const bool defer = nstat != nullptr && c->ste[d].proj_bgb && c->tte[d].proj_bgb;
      int r = run_block(c, c->ste[d], 0, x, y1, y, bufA, bufB, slices, rowstat, n, st, defer && d > 0 ? nstat : nullptr);
      if (r) return r;
      if (defer && d > 0) {
        Scope s(c, P_LN2, st);   // Spatial_norm deferred into TTE block d's proj; TTE block d's norm1
        LAUNCH_TRY(d3dp_launch_ln2_defer(c->act(), x, c->snw, c->snb, c->tte[d].n1w, c->tte[d].n1b, g.eps_block, bufA, nstat, Tc, C, st));
      } else {
        Scope s(c, P_LN2, st);   // x += fc2 out; Spatial_norm (+ Temporal_pos after block 0); TTE block d's norm1
        if (const BlockDev& p = c->ste[d]; p.r_proj | p.r_fc2)      // (FAST16, scaled branch outputs of the block in front)
          LAUNCH_TRY(d3dp_launch_ln2_scaled(x, y1, ldexpf(1.f, p.r_proj), y, ldexpf(1.f, p.r_fc2), c->snw, c->snb, d == 0 ? c->tpos : nullptr,
                                            c->tte[d].n1w, c->tte[d].n1b, g.eps_block, bufA, Tc, C, F, J, st, SP));
        else
          LAUNCH_TRY(d3dp_launch_ln2(c->act(), x, fold ? nullptr : y1, fold ? nullptr : y, c->snw, c->snb, d == 0 ? c->tpos : nullptr, c->tte[d].n1w,
                                     c->tte[d].n1b, g.eps_block, bufA, Tc, C, F, J, st, SP));
      }
      r = run_block(c, c->tte[d], 1, x, y1, y, bufA, bufB, slices, rowstat, n, st, defer && d > 0 ? nstat : nullptr);
      if (r) return r;
      if (d + 1 < g.depth && defer) {
        Scope s(c, P_LN2, st);   // Temporal_norm deferred into STE block d+1's proj; STE block d+1's norm1
        LAUNCH_TRY(d3dp_launch_ln2_defer(c->act(), x, c->tnw, c->tnb, c->ste[d + 1].n1w, c->ste[d + 1].n1b, g.eps_block, bufA, nstat, Tc, C, st));
      } else if (d + 1 < g.depth) {
        Scope s(c, P_LN2, st);   // x += fc2 out; Temporal_norm; STE block d+1's norm1
        if (const BlockDev& p = c->tte[d]; p.r_proj | p.r_fc2)
          LAUNCH_TRY(d3dp_launch_ln2_scaled(x, y1, ldexpf(1.f, p.r_proj), y, ldexpf(1.f, p.r_fc2), c->tnw, c->tnb, nullptr, c->ste[d + 1].n1w,
                                            c->ste[d + 1].n1b, g.eps_block, bufA, Tc, C, F, J, st, SP));
        else
          LAUNCH_TRY(d3dp_launch_ln2(c->act(), x, fold ? nullptr : y1, fold ? nullptr : y, c->tnw, c->tnb, nullptr, c->ste[d + 1].n1w, c->ste[d + 1].n1b,
                                     g.eps_block, bufA, Tc, C, F, J, st, SP));
      }
    }
    {
      Scope s(c, P_HEAD, st);    // x += fc2 out; Temporal_norm; head LayerNorm; Linear(C,3)
      if (const BlockDev& p = c->tte[g.depth - 1]; p.r_proj | p.r_fc2)
        LAUNCH_TRY(d3dp_launch_head_scaled(x, y1, ldexpf(1.f, p.r_proj), y, ldexpf(1.f, p.r_fc2), c->tnw, c->tnb, g.eps_block, c->hnw, c->hnb,
                                           g.eps_head, c->hw, c->hb, out + (size_t)seq0 * FJ * 3, Tc, C, st, FJ, SP));
      else
        LAUNCH_TRY(d3dp_launch_head(c->fast() ? c->act() : 0, x, fold ? nullptr : y1, fold ? nullptr : y, c->tnw, c->tnb, g.eps_block, c->hnw, c->hnb, g.eps_head, c->hw, c->hb,
                                    out + (size_t)seq0 * FJ * 3, Tc, C, st, FJ, SP));
    }
    seq0 += n;
  }
  d3dp_launch_nonfinite_flag(out, (size_t)BH * FJ * 3, c->d_flag, st);    // 15.9 MB at B = 32, H = 20: microseconds
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

}  // extern "C"
