// Internal launcher interface between the C-ABI layer (capi*.hip over ctx.h) and the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "train_plan.h"   // the training kernels' capacities (D3DP_DYPREP_ROWS ... D3DP_TN_MAX), d3dp_tn_applies, the statistics sizes

// "Once per DEVICE" cache of a launcher's set-up (the > 64 KiB dynamic-LDS opt-in of a kernel, which HIP records per device,
// or a number derived from the device's CU count): one process may drive several devices -- nn.DataParallel callers,
// one thread per device (reference main.py:242-248) -- so neither a process-wide `static bool` nor an unlocked one is right.
// get(fn): fn(dev) runs the first time the CURRENT device is seen and returns a value > 0 to cache (<= 0: error, not cached).
struct PerDeviceOnce {
  static constexpr int kMaxDev = 64;
  std::mutex mu;
  int val[kMaxDev] = {0};
  template <class F> int get(F&& fn) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return -3;
    std::lock_guard<std::mutex> lock(mu);
    if (val[dev] <= 0) {
      const int v = fn(dev);
      if (v <= 0) return v < 0 ? v : -3;
      val[dev] = v;
    }
    return val[dev];
  }
};
// multiProcessorCount of device `dev` (> 0) or -3
inline int d3dp_cu_count(int dev) {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess || prop.multiProcessorCount < 1) return -3;
  return prop.multiProcessorCount;
}
// opt one kernel in to `bytes` of dynamic LDS on the current device: 1 or -3
inline int d3dp_lds_opt_in(const void* kern, int bytes) {
  return hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess ? 1 : -3;
}

enum { EPI_BIAS = 0, EPI_GELU = 1, EPI_RESID = 2, EPI_PARTIAL = 3, EPI_QKV_PACK = 4, EPI_RESID_LN = 5, EPI_GELU_LN = 6,
       EPI_RESID_NORM = 7 };

// ---- gemm.hip ----------------------------------------------------------------------------------
// (f16: the 2-byte type of A, W and a 2-byte out -- 0 = bf16, 1 = IEEE fp16)
int d3dp_launch_linear_bf16_stream(int epi, int out_f32, const void* A, const void* W, const float* bias, void* out,
                                   int M, int N, int K, hipStream_t st, int f16 = 0);
// (K / 64 in {1, 2, 4, 8, 16}: gemm.hip itself; 2-byte rows out at K / 64 in {3, 5, 6, 7} and, EPI_BIAS, {10, 12, 14} -- the k-depths of
//  channels 192 / 320 / 384 / 448 -- through gemm_stream_widths.hip, the same kernel template at those NK; -1 for any other)
int d3dp_linear_stream_widths(int epi, const void* A, const void* W, const float* bias, void* out, int M, int N, int K,
                              hipStream_t st, int f16);
// (gemm_stream_scaled.hip: the same kernel template with the scaled epilogue of FAST16 contexts under D3DP_FAST16_RANGE=scale -- fp16
//  operands and fp16 rows out, K / 64 in {1, 2, 4, 8, 16}, epi EPI_BIAS or EPI_GELU.  out = fp16(fma(acc, m_acc, bias m_bias)); EPI_GELU
//  (m_acc == m_bias): that value parked as fp16, then fp16(gelu(. m_inv) m_acc) with m_inv = 1 / m_acc.  All three are powers of two;
//  -1 for any other shape)
int d3dp_linear_stream_scaled(int epi, const void* A, const void* W, const float* bias, void* out, int M, int N, int K, hipStream_t st,
                              float m_acc, float m_bias, float m_inv);
int d3dp_launch_linear_bf16x3(int epi, const void* A3, const void* W3, const float* bias, float* outf, void* out3, int M,
                              int N, int K, hipStream_t st);
void d3dp_launch_split3(const float* src, void* dst, size_t n, hipStream_t st);
// ---- gemm_x2.hip (EXACT mode: split-fp16 operands, three fp16-MFMA passes) ------------------------
// EPI_RESID_LN: outf += ... as EPI_RESID, plus out2 = the SUM's split-fp16 operand (h2i, un-normalised) and aux =
//   [M][ceil(N/64)][2] (mean, M2) of every 64-column slice of every row (the next LayerNorm's statistics, in pieces);
// EPI_GELU_LN: a LayerNorm FOLDED into the Linear: A2 = un-normalised rows, W2 = W . diag(gamma), bias = [c2 | c1] (2 N floats:
//   c2 = W beta + b, c1 = row sums of W diag(gamma)), aux = [M + 256][2] (mean, rstd) per row:
//   out2 = split(GELU(rstd (A W'^T - mean c1) + c2)).
// EPI_RESID_NORM (internal to d3dp_denoise like 5 / 6): outf = LN(outf) + A W^T + b -- EPI_RESID behind a DEFERRED LayerNorm of
//   the residual row: bias = [b | gamma | beta] (3 N floats), aux = [M + 256][2] (mean, rstd) per row as d3dp_launch_ln2_defer left
//   them; every residual value read becomes fmaf((x - mean) * rstd, gamma, beta), the expression of the row kernels, before
//   the Linear's value is added.  3 N <= 2048, K >= 96.
// `unscale` = 1 / (scale of the A operand x scale of the W operand); `oscale` = the power of two the plane outputs (EPI_GELU*,
// k / v of EPI_QKV_PACK, the operand copy of EPI_RESID_LN) are multiplied by before the hi / lo split (kActScale unless the
// proven range of that operand asks for less, capi_weights.hip)
int d3dp_launch_linear_f16x2(int epi, const void* A2, const void* W2, const float* bias, float unscale, float oscale,
                             float* outf, void* out2, float* aux, unsigned* flag, int M, int N, int K, hipStream_t st,
                             int skew_d = 0, int pingpong = 0);
// pingpong: the two-team form of the kernel (gemm_f16x2_pp_kernel: one wave of a SIMD reads its fragments while the other
// multiplies); same results bit for bit (the k order and the arithmetic are unchanged).  OR-ed with X2_TILES_LAST_TO_FIRST the
// plain kernel walks its tiles from the last row of tiles to the first (the rows a following row kernel reads first are then the
// ones written last); same tiles, same results bit for bit
constexpr int X2_TILES_LAST_TO_FIRST = 0x100;
// skew_d (1, 2, 4): the row-class skewed schedule of gemm_x2.hip for EPI_QKV_PACK / EPI_GELU -- a tile's epilogue leaves under the
// next tile's k-loop, D k-steps per 16-row class; d3dp_x2_skew_applies says whether the launcher will use it for a shape
bool d3dp_x2_skew_applies(int epi, int M, int N, int K, int skew_d, int n_cu);
// whether gemm_x2.hip was built with -DD3DP_X2_VARIANTS=1 (the ping-pong / wide / skewed kernels and the norm2-folding
// epilogues: measured-negative experiments, not part of the product library)
bool d3dp_x2_variants_built();
// out[0] = max over rows n of  sum_k |W[n,k]| in_k + |bias[n]|,  out[1] = max_k in_k,  in_k = sq |gamma_k| + |beta_k|: the
// magnitude bound of a Linear fed by a LayerNorm over K channels (sq = sqrt(K - 1): |LN(x)_k| <= sq |gamma_k| + |beta_k| for
// ANY x), as the bit patterns of non-negative floats (integer max == float max; `out` pre-zeroed)
void d3dp_launch_rowbound(const float* W, const float* gamma, const float* beta, const float* bias, int N, int K,
                          unsigned* out, hipStream_t st);
// rowstat[M][2] = (mean, 1 / sqrt(var + eps)) from the slice statistics EPI_RESID_LN wrote (S = ceil(C / 64) slices of 64)
void d3dp_launch_ln_combine(const float* slices, float* rowstat, int M, int C, float eps, hipStream_t st);
// Wp[n][k] = W[n][k] gamma[k];  c12[0..N) = sum_k W[n][k] beta[k] + bias[n],  c12[N..2N) = sum_k Wp[n][k]
void d3dp_launch_fold_ln(const float* W, const float* gamma, const float* beta, const float* bias, float* Wp, float* c12,
                         int N, int K, hipStream_t st);
void d3dp_launch_split2(const float* src, void* dst, size_t n, float scale, hipStream_t st);
// out[0] = max |src[i]| as the bit pattern of a non-negative float (`out` pre-zeroed)
void d3dp_launch_absmax(const float* src, size_t n, unsigned* out, hipStream_t st);
// flag[0] |= 1 if any of x[0..n) is inf / nan
void d3dp_launch_nonfinite_flag(const float* x, size_t n, unsigned* flag, hipStream_t st);
// ---- gemm_x2_train.hip (the training step's split-fp16 Linears, their operand passes and partial sums) ------------
// gemm_f16x2_dyn_kernel: operand scales live on the device.
// out_z[M, N] (z = 0 .. Z-1, M N floats apart) = A2[M][2 Kfull] . W2[N][2 Kfull]^T over k-chunk z, x dynA[0] x dynW[0], + bias
// (bias may be null).  Kfull % (32 Z) == 0, N % 4 == 0.
// amax_out (optional, Z == 1): absmax slot of the output (bit pattern of a non-negative float, pre-zeroed; one atomicMax per workgroup)
// (amax_pos: the largest POSITIVE output value instead of the largest magnitude)
// (rem_blocks: Z == 1, M > 256, Kfull % 512 == 0 -- the M mod 256 rows behind the last whole tile go to 16 x 64 blocks spread over
//  all workgroups instead of a last row of mostly empty 256 x 128 tiles; ignored where the conditions do not hold)
// (passes: 3 = the split scheme; 1 = the hi x hi pass alone -- D3DP_TRAIN_PASSES=1: fp16 operands at their own scale, fp32
//  accumulation; the same operand rows, of which the lo halves are not read.  Also of the two TN launchers below.)
// (rows_hi: D3DP_TRAIN_ROWS=hi -- the operand rows are hi-only, "h1": [.][K] plain fp16, column c at offset c; passes = 1 alone,
//  Kfull % (64 Z) == 0, else refused.  The operand launchers below take the same flag and then write such rows: the hi value of
//  split2h_scaled at the same scale, no lo value.  Also of the two TN launchers.)
int d3dp_launch_linear_f16x2_dyn(const void* A2, const void* W2, const float* bias, const float* dynA, const float* dynW,
                                 float* out, int M, int N, int Kfull, int Z, hipStream_t st, unsigned* amax_out = nullptr,
                                 int amax_pos = 0, int rem_blocks = 0, int passes = 3, int rows_hi = 0);
// drow [Rpad][2 C] = split(GELU(src [R][C])) (rows R .. Rpad - 1 zero) at the scale max(GELU(pmax), 0.17) asks for (pmax: the
// largest positive value of src, left by the Linear that produced it); writes that bound to amax_out[0] and 1 / scale to unscale[0]
int d3dp_launch_gelu_rowprep(const float* src, void* drow, int R, int Rpad, int C, const unsigned* pmax, unsigned* amax_out,
                             float* unscale, hipStream_t st, int rows_hi = 0);
// src [R][C] fp32 -> h2i [R][2 Cpad] (zero columns behind C) at the power of two the tensor's absmax (amax[0], bits of a
// float >= 0, d3dp_launch_absmax) asks for; unscale[0] = 1 / that scale
void d3dp_launch_split2_dyn(const float* src, void* dst, int R, int C, int Cpad, const unsigned* amax, float* unscale,
                            hipStream_t st, int rows_hi = 0);
// the TRANSPOSE as a split operand: src [R][C] -> h2i [C][2 Rpad] (zero behind R; Rpad % 32 == 0)
void d3dp_launch_split2_t_dyn(const float* src, void* dst, int R, int C, int Rpad, const unsigned* amax, float* unscale,
                              hipStream_t st);
// src [R][C] -> row form [R][2 C], transposed form [C][2 Rpad] and (colpart != null) its column sums as D3DP_DYPREP_ROWS
// partial rows of C floats (every row written; summed by d3dp_train_reduce_many) in one pass
int d3dp_launch_dyprep(const float* src, void* drow, void* dcol, float* colpart, int R, int C, int Rpad, const unsigned* amax,
                       float* unscale, hipStream_t st);
// the row form alone as a streaming pass: src [R][C] -> drow [Rpad][2 C] (rows R .. Rpad - 1 zero) + optional column sums as *rows
// (<= D3DP_ROWPREP_ROWS) partial rows of C floats; C % 32 == 0, C <= 1536
// (mask: optional per-sample scales applied to the rows first -- sample = r / J (axis 0) or (r / (F J)) J + r % J (axis 1))
// (gelu_pre: optional [R][C]; the operand is src x gelu'(gelu_pre) and amax[0] holds the absmax of SRC, see rowprep_kernel)
int d3dp_launch_rowprep(const float* src, void* drow, float* colpart, int* rows, int R, int Rpad, int C, const unsigned* amax,
                        float* unscale, hipStream_t st, const float* mask = nullptr, int axis = 0, int F = 1, int J = 1,
                        const float* gelu_pre = nullptr, int rows_hi = 0);
// drow = split(LayerNorm(src; w, b, eps)): the operand of a Linear fed by a LayerNorm, from the LayerNorm's INPUT (amax: the
// absmax of the LayerNorm's output, left by the kernel that produced src); C <= 512
int d3dp_launch_rowprep_ln(const float* src, const float* w, const float* b, float eps, void* drow, int R, int Rpad, int C,
                           const unsigned* amax, float* unscale, hipStream_t st, int rows_hi = 0);
// wgrad straight from the ROW forms (gemm_f16x2_tn_kernel): out_z[N, K] = sum_{t in chunk z} A2[t][n] W2[t][k] x dynA x dynW,
// Tp = Z NKz 32 rows per operand (rows beyond the real ones zero).  d3dp_tn_applies: N % 256 == 0 and K % 128 == 0.
int d3dp_launch_linear_f16x2_tn(const void* A2, const void* W2, const float* dynA, const float* dynW, float* out, int N, int K,
                                int Tp, int Z, hipStream_t st, int passes = 3, int rows_hi = 0);
// ... several such products over the same Tp rows in one launch (the weight gradients of a block): one merged tile list, one Z
struct D3dpTnProduct {
  const void* A2; const void* W2;                      // [Tp][2 N] and [Tp][2 K] row forms
  const float* dynA; const float* dynW;
  float* out;                                          // Z partial products, N K floats apart
  int N, K;
  int tiles_k, tile0;                                  // (filled by the launcher)
};
struct D3dpTnTable { D3dpTnProduct p[D3DP_TN_MAX]; int n; };
int d3dp_launch_linear_f16x2_tn_many(const D3dpTnProduct* prods, int n, int Tp, int Z, hipStream_t st, int passes = 3, int rows_hi = 0);
struct D3dpSumTable { const float* part[D3DP_TN_MAX]; float* out[D3DP_TN_MAX]; size_t n4[D3DP_TN_MAX]; int Z; int n; };
void d3dp_launch_sum_partials_many(const D3dpSumTable& tb, hipStream_t st);   // out_p[i] = sum_z part_p[z n_p + i], z ascending
// the training step's weight operands in three launches: absmax -> slot, rows form [N][2 K] at rows_base + 2 off
// halves, transposed form [K][2 N] at cols_base + 2 off halves, unscale[slot] = 1 / scale
struct D3dpWPrepItem { const float* w; int N, K, slot, pad; size_t off; };
struct D3dpWPrepTable { D3dpWPrepItem it[D3DP_WPREP_MAX]; int n; };
// (rows_hi: both forms hi-only, [N][K] and [K][N], at the same rows_base / cols_base + 2 off halves -- the first half of each weight's region)
int d3dp_launch_wprep(const D3dpWPrepTable& tb, void* rows_base, void* cols_base, unsigned* amax, float* unscale, hipStream_t st,
                      int rows_hi = 0);
// out[i] = sum over z of part[z n + i], z ascending
void d3dp_launch_sum_partials(const float* part, float* out, size_t n, int Z, hipStream_t st);
void d3dp_launch_sum_partials_bias(const float* part, const float* bias, float* out, size_t n, int N, int Z, hipStream_t st,
                                   unsigned* amax = nullptr, int amax_pos = 0);
// ---- gemm.hip again: the fp32-MFMA Linears of the fp32 implementations ---------------------------------------------
int d3dp_launch_linear_f32_splitk(const float* A, const float* W, float* out, int M, int N, int K, hipStream_t st, float* part,
                                  size_t part_floats);
int d3dp_launch_linear_f32(int epi, const float* A, const float* W, const float* bias, float* out, int M, int N,
                           int K, hipStream_t st);

// ---- attention: the sequence map every attention launcher takes ------------------------------------
// qkv: [T, 3C] (q | k | v, each head-major hd-minor), out: [T, C].  A "sequence" s of length n_tok has
// token index  tok(s, i) = (s / inner) * outer_stride + (s % inner) * inner_stride + i * tok_stride.
//   spatial : n_tok = J, inner = 1,  outer_stride = J,   inner_stride = 0, tok_stride = 1   (s = bh*F + f)
//   temporal: n_tok = F, inner = J,  outer_stride = F*J, inner_stride = 1, tok_stride = J   (s = bh*J + n)
struct SeqMap { int n_tok, inner, outer_stride, inner_stride, tok_stride; };
// ---- attention_f32.hip: fp32 arithmetic ---------------------------------------------------------
// (any sequence length; amax: optional absmax slot of an fp32 output, one atomicMax per workgroup)
int d3dp_launch_attn_rows(int act_bf16, const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads,
                          hipStream_t st, unsigned* amax = nullptr);
int d3dp_launch_attn_temporal_f32(int act, const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads,
                                  hipStream_t st);
// ---- attention_fast.hip: FAST / FAST16 on the 2-byte matrix cores -------------------------------
// (the MFMA kernels of the FAST modes -- f16: 0 = bf16 rows in and out, 1 = IEEE fp16; d3dp_launch_attn_rows: act 1 / act 4)
// hd_true: the head dim of the softmax exponent (hd_true^-0.5) where it is smaller than C / heads -- rows whose heads were padded with
// zero columns to head dim 32 (hd_true 24) or 64 (hd_true 40 / 48 / 56): attention_fast_pad.hip; 0 = C / heads itself
int d3dp_launch_attn_temporal_bf16(const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads,
                                   hipStream_t st, int f16 = 0, int hd_true = 0);
int d3dp_launch_attn_spatial_bf16(const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads, hipStream_t st,
                                  int f16 = 0, int hd_true = 0);
// (attention_fast_pad.hip: the padded forms behind the two launchers above; axis 0 = the spatial kernel, <= 32 tokens)
int d3dp_attn_fast_padded(int axis, const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads, hipStream_t st, int f16,
                          int hd_true);
// (attention_fast_scaled.hip: the same kernels on fp16 rows whose q, k and v hold 2^-s times their value -- FAST16 contexts under
//  D3DP_FAST16_RANGE=scale; the exponent scale is (C / heads)^-0.5 x emul, emul = 2^(2s); head dim 64, 32 or 16; axis as above)
int d3dp_attn_fast_scaled(int axis, const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads, hipStream_t st, float emul);
// ---- attention_x2.hip: EXACT on split-fp16 operands (head dim 64, 32 or 16; -2 for any other) ----
// split-fp16 attention: `qkv` = PACKED rows of 12 C bytes (q fp32 | k hi | k lo | v hi | v lo), written by the qkv Linear
// with EPI_QKV_PACK or from fp32 rows by d3dp_launch_qkv_pack_x2
// `act_scale`: the power of two the k / v planes were written at (q and, for plane output, o use the same)
// act 0: fp32 rows out, 3: the two fp16 planes of the proj Linear's operand.  Any SeqMap, up to 1024 tokens per sequence.
// hd_true: the head dim of the softmax exponent (hd_true^-0.5) where it is smaller than C / heads -- packed rows whose heads were
// padded with zero columns to a head dim the kernels are instantiated for (0: C / heads itself)
int d3dp_launch_attn_x2(int act, int axis, const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads,
                        float act_scale, hipStream_t st, int hd_true = 0);
void d3dp_launch_qkv_pack_x2(const float* src, void* dst, size_t T, int C, float act_scale, hipStream_t st);

// ---- pointwise.hip -----------------------------------------------------------------------------
int d3dp_launch_time_mlp(const int64_t* t, const float* freq, const float* w1, const float* b1, const float* w2,
                         const float* b2, float* temb, int B, int C, hipStream_t st);
// x[T,C] = embed(x2d, x3d) + spos + temb ;  xn = LN1(x)
int d3dp_launch_embed_ln(int act_bf16, const float* x2d, const float* x3d, const float* temb, const float* ew,
                         const float* eb, const float* spos, const float* lnw, const float* lnb, float eps, float* x,
                         void* xn, int seq0, int n_seq, int H, int F, int J, int C, hipStream_t st, int SP = 0);
// (SP: rows per sequence in x / xn, >= F J; 0 = F J.  Rows F J .. SP - 1 of every sequence are finite filler.)
// xn = LN(x)
// (residual adds: ln normalises x + yadd (writing the sum back only if write_x); ln2 / head form (x + yadd0) + yadd;
//  yadd has the activation type: bf16 in FAST mode, fp16 in FAST16 mode, fp32 in EXACT mode.
//  act_bf16 is the activation code of the row launchers: 0 fp32, 1 bf16, 2 split-bf16 planes, 3 split-fp16 planes, 4 IEEE fp16)
int d3dp_launch_ln(int act_bf16, float* x, const void* yadd, int write_x, const float* w, const float* b, float eps,
                   void* xn, int T, int C, hipStream_t st);
// x = LN_a(x) (+ pos[f]) in place ; xn = LN_b(x)   (shared Spatial/Temporal norm fused with the next block's norm1)
int d3dp_launch_ln2(int act_bf16, float* x, const void* yadd0, const void* yadd, const float* wa, const float* ba, const float* pos,
                    const float* wb, const float* bb, float eps, void* xn, int T, int C, int F, int J, hipStream_t st,
                    int SP = 0);
// the norm pair with its first norm DEFERRED: xn = LN_b(LN_a(x)), x untouched, stat[T][2] = (mean, rstd) of LN_a per row -- the
// next Linear that adds into x applies LN_a itself (EPI_RESID_NORM).  act_bf16 = 3 (split-fp16 planes) only.
int d3dp_launch_ln2_defer(int act_bf16, const float* x, const float* wa, const float* ba, const float* wb, const float* bb, float eps,
                          void* xn, float* stat, int T, int C, hipStream_t st);
// ---- pointwise_rows2.hip: the four row kernels at a run-time width with 2-byte rows (act 1 = bf16, 4 = IEEE fp16; C % 32 == 0,
// C <= 512; -2 otherwise) -- xn and the yadd rows have the type; reached through the four launchers around this block
int d3dp_rows2_embed_ln(int act, const float* x2d, const float* x3d, const float* temb, const float* ew, const float* eb,
                        const float* spos, const float* lnw, const float* lnb, float eps, float* x, void* xn, int seq0, int n_seq,
                        int H, int F, int J, int C, hipStream_t st, int SP);
int d3dp_rows2_ln(int act, float* x, const void* yadd, int write_x, const float* w, const float* b, float eps, void* xn, int T, int C,
                  hipStream_t st);
int d3dp_rows2_ln2(int act, float* x, const void* yadd0, const void* yadd, const float* wa, const float* ba, const float* pos,
                   const float* wb, const float* bb, float eps, void* xn, int T, int C, int F, int J, hipStream_t st, int SP);
int d3dp_rows2_head(int act, const float* x, const void* yadd0, const void* yadd, const float* wa, const float* ba, float eps_a,
                    const float* wh, const float* bh, float eps_h, const float* w, const float* b, float* out, int T, int C,
                    hipStream_t st, int FJ, int SP);
// ---- the ln / ln2 / head launchers around this block for FAST16 contexts under D3DP_FAST16_RANGE=scale: fp16 activations at the
// instantiated widths (-2 otherwise), every yadd operand there (-1 otherwise) with the power-of-two multiplier m that takes its
// fp16 rows back to their value -- x + yadd m (ln, never written back), (x + yadd0 m0) + yadd m (ln2, head)
int d3dp_launch_ln_scaled(const float* x, const void* yadd, float m, const float* w, const float* b, float eps, void* xn, int T, int C,
                          hipStream_t st);
int d3dp_launch_ln2_scaled(float* x, const void* yadd0, float m0, const void* yadd, float m, const float* wa, const float* ba,
                           const float* pos, const float* wb, const float* bb, float eps, void* xn, int T, int C, int F, int J,
                           hipStream_t st, int SP);
int d3dp_launch_head_scaled(const float* x, const void* yadd0, float m0, const void* yadd, float m, const float* wa, const float* ba,
                            float eps_a, const float* wh, const float* bh, float eps_h, const float* w, const float* b, float* out, int T,
                            int C, hipStream_t st, int FJ, int SP);
// out[T,3] = Linear(LN_head(LN_a(x)))
int d3dp_launch_head(int act_bf16, const float* x, const void* yadd0, const void* yadd, const float* wa, const float* ba, float eps_a, const float* wh,
                     const float* bh, float eps_h, const float* w, const float* b, float* out, int T, int C,
                     hipStream_t st, int FJ = 0, int SP = 0);   // (rows at pitch SP per sequence -> compact out rows; 0 = compact in)

// ---- sampler.hip -------------------------------------------------------------------------------
int d3dp_launch_ddim_pre(const float* img, float* xt2, const int* perm, float scale, int B, int per_b, int J,
                         hipStream_t st);
int d3dp_launch_ddim_post(const float* pred2, const float* img, const float* noise, const int* perm, float scale,
                          double sqrt_recip, double sqrt_recipm1, float c_xstart, float c_noise, float sigma,
                          int last, float* x_start, size_t xs_bstride, float* img_next, int B, int per_b, int J,
                          hipStream_t st);
int d3dp_launch_q_sample(const float* x0, const float* noise, const double* a, const double* b, float scale,
                         float* out, int B, int per_b, hipStream_t st);

// ---- sampler_native.hip (the kernels of d3dp_sample / d3dp_op_randn; the generator's definition: include/d3dp_hip.h) ----
// out[e] (and bits[e], optional) for e < n; -1 if (n - 1) >> 2 does not fit the 32-bit counter word
int d3dp_launch_randn(unsigned long long seed, unsigned draw, float* out, unsigned* bits, size_t n, hipStream_t st);
// the set-up of a d3dp_sample call: the initial img (n elements: noise0, or draw 0 of `seed`; into img64 if non-null, else img32),
// the timestep rows of steps k0 .. k0 + n_t - 1 (n_t <= 64 per launch; t: host array indexed by step) into trows[K][nb], and
// x2cat = x2d | x2f (nx2_half elements each; 0: none)
int d3dp_launch_sample_setup(const float* noise0, unsigned long long seed, float* img32, double* img64, size_t n, long long* trows,
                             const long long* t, int k0, int n_t, int nb, const float* x2d, const float* x2f, float* x2cat,
                             size_t nx2_half, hipStream_t st);
// d3dp_launch_ddim_post with the noise of (seed, draw) generated in registers
int d3dp_launch_ddim_post_gen(const float* pred2, const float* img, unsigned long long seed, unsigned draw, const int* perm, float scale,
                              double sqrt_recip, double sqrt_recipm1, float c_xstart, float c_noise, float sigma, int last,
                              float* x_start, size_t xs_bstride, float* img_next, int B, int per_b, int J, hipStream_t st);
// the non-flip forms (model.py ddim_sample's rounding points: img is fp64; first: it holds the fp32 initial noise)
int d3dp_launch_ddim_pre_noflip(const double* img, float* xt, float scale, int first, int B, int per_b, hipStream_t st);
int d3dp_launch_ddim_post_noflip(const float* pred, const double* img, const float* noise, unsigned long long seed, unsigned draw,
                                 float scale, double sqrt_recip, double sqrt_recipm1, float c_xstart, double c_noise64, float sigma,
                                 int last, float* x_start, size_t xs_bstride, double* img_next, int B, int per_b, hipStream_t st);

// ---- jpma.hip ----------------------------------------------------------------------------------
int d3dp_launch_jpma(const float* pred, const float* traj, const float* cam, const float* gt2d, const float* gt3d,
                     float* agg, int* sel, float* err_sel, float* err_min, float* win, float* jbest, float* mean,
                     int h_offset, int B, int K, int H, int F, int J, int root_joint, int linear, hipStream_t st,
                     int h_inner = 0, size_t outer_stride = 0);   // (h_inner, outer_stride): see jpma_kernel; 0 = contiguous H

// ---- capi_weights.hip ------------------------------------------------------------------------------------------
// fp32 -> bf16 (f16: IEEE fp16), a plain cast: the FAST / FAST16 weight matrices (d3dp_set_weights) and d3dp_op_to_bf16
void d3dp_launch_to_bf16(const float* s, void* d, size_t n, hipStream_t st, int f16 = 0);
// ... with padded heads (ctx.h hdp): dst [rows][cols] of the 2-byte type from src [.][src_cols]; pad_rows: the row axis is padded, in
// sections of heads x hdp rows (the qkv matrix), otherwise the column axis (the proj matrix); a pad element is an exact zero
void d3dp_launch_to_bf16_pad(const float* s, void* d, int rows, int cols, int src_cols, int pad_rows, int hd, int hdp, int heads,
                             hipStream_t st, int f16);

// ---- capi.hip helpers shared with caller.hip ---------------------------------------------------------------------
int d3dp_set_error(int code, const char* msg);        // records the message for d3dp_last_error(), returns code
int d3dp_check_launch(const char* what);              // hipGetLastError -> status
extern "C" int d3dp_clip_count(int32_t n, int32_t F);

// ---- train.hip (training step, fp32) -------------------------------------------------------------------------
// (amax: optional absmax slot of a kernel's result -- bit pattern of a non-negative float, pre-zeroed, one atomicMax per
//  workgroup -- so that the split-fp16 Linear that consumes the result needs no absmax pass of its own)
// x_out = x_in + mask[sample] y ; xn = LN(x_out)  (xn may be null: only amax, the absmax of LN(x_out), is produced)
int d3dp_train_add_mask_ln(const float* x_in, const float* y, const float* mask, int axis, int F, int J, const float* w,
                           const float* b, float eps, float* x_out, float* xn, unsigned* amax, int T, int C, hipStream_t st,
                           void* op = nullptr, int Tp = 0, float* op_unscale = nullptr, int op_hi = 0);
// (op_hi, also below: the operand rows are hi-only [Tp][C] -- D3DP_TRAIN_ROWS=hi)
// x_out = x_in + mask[sample] y ; x_next = LN_a(x_out) (+ pos[f]) ; xn = LN_b(x_next)  (wb null: no second norm; xn null with
// wb given: LN_b's output is not stored, only its absmax)
int d3dp_train_add_mask_ln2(const float* x_in, const float* y, const float* mask, int axis, int F, int J, const float* wa,
                            const float* ba, float eps_a, const float* pos, const float* wb, const float* bb, float eps_b,
                            float* x_out, float* x_next, float* xn, unsigned* amax, int T, int C, hipStream_t st, void* op = nullptr,
                            int Tp = 0, float* op_unscale = nullptr, int op_hi = 0);
int d3dp_train_ln_pos(const float* x, const float* w, const float* b, float eps, const float* pos, int F, int J, float* y,
                      int T, int C, hipStream_t st);
// LayerNorm backward, one (xa == null) or two chained LayerNorms (y = LN_b(xb), xb = LN_a(xa) (+ pos)) in one pass:
//   g = LN_b-backward(dy) + dres (g_out: optional copy, two-norm form only);  dx = two ? LN_a-backward(g) : g;
//   dxm (optional) = mask[sample] dx, amax (optional) its absmax -- dy and dxm may alias.
// part_b / part_a: d3dp_train_ln_bwd_blocks(T) rows of [dgamma | dbeta] (2 C floats) per LayerNorm, to be summed in order by
// d3dp_train_reduce_many (no float atomics anywhere in the backward pass: bit-reproducible gradients).
int d3dp_train_ln_bwd(const float* dy, const float* xb, const float* wb, float eps_b, const float* dres, float* g_out,
                      const float* xa, const float* wa, float eps_a, float* dx, const float* mask, int axis, int F, int J,
                      float* dxm, unsigned* amax, float* part_b, float* part_a, int T, int C, hipStream_t st);
// dst[i] (+)= sum_{p < count} part[p stride + i] in a fixed order, up to D3DP_REDUCE_MAX destinations per launch
constexpr int D3DP_REDUCE_MAX = 80;
struct D3dpReduceItem { const float* part; float* dst; unsigned n, count, stride, accumulate; };
struct D3dpReduceTable { D3dpReduceItem it[D3DP_REDUCE_MAX]; int count; };
int d3dp_train_reduce_many(const D3dpReduceTable& tb, hipStream_t st);
// (amax: optional absmax slot of the result, see train.hip block_amax_commit)
int d3dp_train_gelu_fwd(const float* x, float* y, size_t n, unsigned* amax, hipStream_t st);
int d3dp_train_gelu_bwd(const float* dh, const float* x, float* dpre, size_t n, unsigned* amax, hipStream_t st);
// column sums as *rows (<= max_rows <= 512) partial rows of C floats (summed by d3dp_train_reduce_many)
int d3dp_train_colsum(const float* in, float* part, int* rows, int max_rows, int T, int C, hipStream_t st);
// zero up to D3DP_ZERO_MAX fp32 buffers in one launch (the small gradient buffers of a backward pass)
constexpr int D3DP_ZERO_MAX = 192;
struct D3dpZeroTable { float* p[D3DP_ZERO_MAX]; unsigned n[D3DP_ZERO_MAX]; int count; };
int d3dp_train_zero_many(const D3dpZeroTable& tb, hipStream_t st);
// grouped row sums (mode 0: per joint, 1: per frame, 2: per batch element) as `slices` partial tables of groups x C floats
int d3dp_train_groupsum(const float* in, float* out, int T, int C, int mode, int F, int J, int slices, hipStream_t st);
int d3dp_train_transpose_pad(const float* in, float* out, int R, int C, int Rpad, hipStream_t st);
// chunked (CtxPlan::train_long_attn): every launch that goes to the whole-sequence VALU pair, or that they refuse with -2 (more than
// 256 tokens, or two images beyond 160 KiB), goes to the chunked pair instead -- any n, bit-equal gradients where both run
int d3dp_train_attn_bwd(const float* qkv, const float* o, const float* dout, float* dqkv, void* stats, int n_seq,
                        SeqMap map, int C, int heads, hipStream_t st, bool chunked = false);
// ---- train_attn.hip: the training step's attention on split-fp16 operands (head dim 64, 32 or 16, and 24 / 40 / 48 / 56 padded to 32 / 64
// inside the kernels: -2 for any other; <= 1024 tokens per sequence) ----
// stats: d3dp_train_attn_x2_stats_bytes per attention (the forward leaves the log-sum-exp of every query for the backward pass);
// amax_qkv / amax_do: absmax slots of the whole qkv tensor / of dout (left by the Linears that produced them); amax_out
// (optional): absmax slot of the result.
int d3dp_train_attn_x2_fwd(const float* qkv, float* out, void* stats, int n_seq, SeqMap map, int C, int heads,
                           const unsigned* amax_qkv, unsigned* amax_out, hipStream_t st, void* op = nullptr, int T = 0, int Tp = 0,
                           float* op_unscale = nullptr, int passes = 3, int op_hi = 0);
int d3dp_train_attn_x2_bwd(const float* qkv, const float* o, const float* dout, float* dqkv, void* stats, int n_seq, SeqMap map,
                           int C, int heads, const unsigned* amax_qkv, const unsigned* amax_do, unsigned* amax_out,
                           hipStream_t st, int part = 0, int passes = 3);
// train_attn_pad.hip: the padded-head instantiations behind the two launchers above (which: 0 = forward, 1 = both backward passes,
// 2 = pass Q alone, 3 = pass KV alone); called by train_attn.hip only
int d3dp_train_attn_x2_padded(int which, const float* qkv, const float* o, const float* dout, float* out, float* dqkv, void* stats,
                              int n_seq, SeqMap map, int C, int heads, const unsigned* amax_qkv, const unsigned* amax_do,
                              unsigned* amax_out, hipStream_t st);
// train_attn_1p.hip: the one-pass instantiations (passes = 1: every product as ONE fp16-MFMA pass on the hi planes, one-plane LDS
// images; head dims 64 / 32 / 16) behind the same two launchers; called by train_attn.hip only
int d3dp_train_attn_x2_1p(int which, const float* qkv, const float* o, const float* dout, float* out, float* dqkv, void* stats,
                          int n_seq, SeqMap map, int C, int heads, const unsigned* amax_qkv, const unsigned* amax_do,
                          unsigned* amax_out, hipStream_t st, void* op, int T, int Tp, float* op_unscale);
// train_attn_hi.hip: the forward with the proj operand as hi-only rows [Tp][C] (D3DP_TRAIN_ROWS=hi; passes 1 | 3, head dims 64 / 32);
// called by train_attn.hip only
int d3dp_train_attn_x2_fwd_hi(int passes, const float* qkv, float* out, void* stats, int n_seq, SeqMap map, int C, int heads,
                              const unsigned* amax_qkv, unsigned* amax_out, hipStream_t st, void* op, int T, int Tp, float* op_unscale);
int d3dp_train_embed_bwd(const float* dx, const float* x2d, const float* x3d, float* part, int T, int C, hipStream_t st);
int d3dp_train_head_linear(const float* z, const float* w, const float* b, float* out, int T, int C, hipStream_t st);
int d3dp_train_head_bwd(const float* g, const float* z, const float* w, float* dz, float* part, int* rows, int T, int C,
                        hipStream_t st);
// the time-embedding MLP of the training step (one wave per output unit, two launches); hidden: scratch of B x 2 C floats
int d3dp_train_time_mlp(const int64_t* t, const float* freq, const float* w1, const float* b1, const float* w2, const float* b2,
                        float* hidden, float* temb, int B, int C, hipStream_t st);
int d3dp_train_time_mlp_bwd(const int64_t* t, const float* freq, const float* w1, const float* b1, const float* w2,
                            const float* dtemb, float* dw1, float* db1, float* dw2, float* db2, int B, int C,
                            hipStream_t st);

// train_g.hip: the training step's row kernels at a run-time width (any C <= 1024; the fp32 path of capi_train.hip for the widths
// train.hip does not instantiate).  The d3dp_train_* launchers above forward to these when d3dp_width_instantiated(C) is false.
// amax (optional, as above): the three kernels that feed a split-fp16 Linear leave the absmax of what its operand pass will split
// (D3DP_TRAIN_IMPL=f16x2 at -cs 192 / 320 / 384 / 448); null on the fp32 path, whose results it does not touch.  No operand rows.
inline bool d3dp_width_instantiated(int C) { return C == 64 || C == 128 || C == 256 || C == 512; }
int d3dp_train_g_add_mask_ln(const float* x_in, const float* y, const float* mask, int axis, int F, int J, const float* w,
                             const float* b, float eps, float* x_out, float* xn, unsigned* amax, int T, int C, hipStream_t st);
int d3dp_train_g_add_mask_ln2(const float* x_in, const float* y, const float* mask, int axis, int F, int J, const float* wa,
                              const float* ba, float eps_a, const float* pos, const float* wb, const float* bb, float eps_b,
                              float* x_out, float* x_next, float* xn, unsigned* amax, int T, int C, hipStream_t st);
int d3dp_train_g_ln_pos(const float* x, const float* w, const float* b, float eps, const float* pos, int F, int J, float* y, int T,
                        int C, hipStream_t st);
int d3dp_train_g_ln_bwd(const float* dy, const float* xb, const float* wb, float eps_b, const float* dres, float* g_out,
                        const float* xa, const float* wa, float eps_a, float* dx, const float* mask, int axis, int F, int J,
                        float* dxm, unsigned* amax, float* part_b, float* part_a, int T, int C, int blocks, hipStream_t st);
int d3dp_train_g_head_linear(const float* z, const float* w, const float* b, float* out, int T, int C, hipStream_t st);
int d3dp_train_g_time_mlp_bwd(const int64_t* t, const float* freq, const float* w1, const float* b1, const float* w2,
                              const float* dtemb, float* dw1, float* db1, float* dw2, float* db2, int B, int C, hipStream_t st);
