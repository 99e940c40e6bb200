// Weights of libd3dp_hip.so (include/d3dp_hip.h d3dp_set_weights, d3dp_set_weights_borrowed): the range proofs of the EXACT
// split-fp16 and FAST16 contexts, which choose a context's implementation and operand scales from its weights, and the packing
// of the weights into the context's arena in the operand form of its Linears (2-byte elements, split-fp16 h2i rows, three bf16
// planes or fp32).
#include <cmath>

#include "ctx.h"

namespace {

template <typename E>   // E: bf16 or f16 -- a plain cast, round to nearest even
__global__ void to_bf16_kernel(const float* __restrict__ s, E* __restrict__ d, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) d[i] = (E)s[i];
}

// ---- padded heads (ctx.h hdp: D3DP_EXACT_IMPL=f16x2 at channels 192 / 320 / 384 / 448) -------------------------------------------
// A head of hd columns becomes hdp = 32 or 64 columns, the new ones zero, INSIDE the packed weights: index h hdp + d of the
// padded axis holds index h hd + d of the source for d < hd.  pad_rows: the padded axis is the ROW axis, in sections of
// heads x hdp rows (the qkv matrix, 3 sections: row s Cp + h hdp + d <- source row s C + h hd + d); otherwise the column axis (the
// proj matrix).  The split is d3dp_launch_split2's: src x scale -> hi / lo (split2h_scaled) in the h2i layout of a [rows][cols]
// matrix (cols % 32 == 0); a pad element is the split of 0, two exact zeros.  One thread per destination element.
__device__ __forceinline__ int unpad_index(int i, int hd, int hdp, int heads) {   // padded index -> source index, or -1
  const int per = heads * hdp, s = i / per, r = i - s * per, h = r / hdp, d = r - h * hdp;
  return d < hd ? s * heads * hd + h * hd + d : -1;
}
__global__ void split2h_pad_kernel(const float* __restrict__ src, f16* __restrict__ dst, int rows, int cols, int src_cols,
                                   int pad_rows, int hd, int hdp, int heads, float scale) {
  const size_t n = (size_t)rows * cols, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int r = (int)(i / cols), c = (int)(i - (size_t)r * cols);
    const int sr = pad_rows ? unpad_index(r, hd, hdp, heads) : r, sc = pad_rows ? c : unpad_index(c, hd, hdp, heads);
    const float v = sr >= 0 && sc >= 0 ? src[(size_t)sr * src_cols + sc] : 0.f;
    f16 a, b;
    split2h_scaled(v * scale, a, b);
    f16* d = dst + (size_t)r * 2 * cols + h2i_col(c);
    d[0] = a; d[kH2iLo] = b;
  }
}
// the qkv bias with the same row map: dst[i] = src[unpad(i)] or 0
__global__ void pad_bias_kernel(const float* __restrict__ src, float* __restrict__ dst, int n, int hd, int hdp, int heads) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int si = unpad_index(i, hd, hdp, heads);
  dst[i] = si >= 0 ? src[si] : 0.f;
}

// the plain cast of to_bf16_kernel with the same head map (a FAST / FAST16 context with padded heads): dst [rows][cols] of E, a pad
// element an exact zero.  One thread per destination element.
template <typename E>
__global__ void to_bf16_pad_kernel(const float* __restrict__ src, E* __restrict__ dst, int rows, int cols, int src_cols, int pad_rows,
                                   int hd, int hdp, int heads) {
  const size_t n = (size_t)rows * cols, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int r = (int)(i / cols), c = (int)(i - (size_t)r * cols);
    const int sr = pad_rows ? unpad_index(r, hd, hdp, heads) : r, sc = pad_rows ? c : unpad_index(c, hd, hdp, heads);
    dst[i] = (E)(sr >= 0 && sc >= 0 ? src[(size_t)sr * src_cols + sc] : 0.f);
  }
}

}  // namespace

void d3dp_launch_to_bf16_pad(const float* s, void* d, int rows, int cols, int src_cols, int pad_rows, int hd, int hdp, int heads,
                             hipStream_t st, int f16) {
  const size_t n = (size_t)rows * cols;
  const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
  if (f16) hipLaunchKernelGGL(to_bf16_pad_kernel<_Float16>, dim3(blocks ? blocks : 1), dim3(256), 0, st, s, (_Float16*)d, rows, cols, src_cols, pad_rows, hd, hdp, heads);
  else hipLaunchKernelGGL(to_bf16_pad_kernel<__bf16>, dim3(blocks ? blocks : 1), dim3(256), 0, st, s, (__bf16*)d, rows, cols, src_cols, pad_rows, hd, hdp, heads);
}

void d3dp_launch_to_bf16(const float* s, void* d, size_t n, hipStream_t st, int f16) {
  const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
  if (f16) hipLaunchKernelGGL(to_bf16_kernel<_Float16>, dim3(blocks ? blocks : 1), dim3(256), 0, st, s, (_Float16*)d, n);
  else hipLaunchKernelGGL(to_bf16_kernel<__bf16>, dim3(blocks ? blocks : 1), dim3(256), 0, st, s, (__bf16*)d, n);
}

namespace {

// ---- the range proof of D3DP_MODE_FAST16 (d3dp_set_weights; include/d3dp_hip.h d3dp_fast_operands) ----------------------------
// One wave per row n of W [N][K]:  s_n = sum_k |W[n,k]| in_k + |bias_n|  with  in_k = sq |gamma_k| + |beta_k|  (gamma given: the
// Linear reads a LayerNorm over K channels, sq = sqrt(K - 1)) or the constant cin[0] (the Linear reads a tensor bounded by a
// number an earlier launch of this kernel left on the device).  Products and sums run in fp64 -- the fp32 inputs' products are
// exact there and the accumulated rounding of <= 2048 terms stays below 2^-40 -- and every result is rounded UP to fp32, so a
// bound never under-states the formula and over-states it by less than 2^-22.  Results leave as the bit patterns of
// non-negative floats under an integer max (`out` pre-zeroed); a nan weight gives a nan bound, whose pattern is above inf's.
//   o_sum  = max_n s_n;   o_tail (optional) = max over rows n >= n_tail;   o_in (optional) = max_k in_k;   o_w = max |W|
__device__ __forceinline__ unsigned f32_bits_up(double v) {
  float f = (float)v;
  if ((double)f < v) f = __uint_as_float(__float_as_uint(f) + 1u);        // (v >= 0: the next float up; FLT_MAX -> inf)
  return __float_as_uint(f) & 0x7fffffffu;                                // (a nan may carry a sign bit)
}
__device__ __forceinline__ unsigned wave_max_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned t = (unsigned)__shfl_xor((int)v, o, 64); v = t > v ? t : v; }
  return v;
}
__global__ __launch_bounds__(256) void fast16_bound_kernel(const float* __restrict__ W, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const unsigned* __restrict__ cin,
                                                           const float* __restrict__ bias, int N, int K, double sq, int n_tail,
                                                           unsigned* o_sum, unsigned* o_tail, unsigned* o_in, unsigned* o_w) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const double c = cin ? (double)__uint_as_float(cin[0]) : 0.0;
  double a = 0.0;
  unsigned inmax = 0u, wmax = 0u;
  for (int k = lane; k < K; k += 64) {
    const float w = fabsf(W[(size_t)n * K + k]);
    const double in = gamma ? sq * (double)fabsf(gamma[k]) + (double)fabsf(beta[k]) : c;
    const unsigned ib = f32_bits_up(in), wb = __float_as_uint(w);
    inmax = ib > inmax ? ib : inmax;
    wmax = wb > wmax ? wb : wmax;
    a += (double)w * in;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  inmax = wave_max_u(inmax);
  wmax = wave_max_u(wmax);
  if (lane == 0) {
    const unsigned sb = f32_bits_up((a + (double)fabsf(bias[n])) * (1.0 + 0x1p-40));
    atomicMax(o_sum, sb);
    if (o_tail && n >= n_tail) atomicMax(o_tail, sb);
    if (o_in) atomicMax(o_in, inmax);
    atomicMax(o_w, wmax);
  }
}
constexpr int kF16Slots = 11;   // per block: L1, b_qkv, b_v, b_proj, L2, b_h, b_fc2, max |w| of qkv / proj / fc1 / fc2

// every pointer of a block's weights / of the top-level weights and of all 2 x depth blocks is there
bool block_weights_complete(const d3dp_block_weights& b) {
  return b.norm1_w && b.norm1_b && b.qkv_w && b.qkv_b && b.proj_w && b.proj_b && b.norm2_w && b.norm2_b && b.fc1_w && b.fc1_b &&
         b.fc2_w && b.fc2_b;
}
bool weights_complete(const d3dp_weights& w, int depth) {
  const float* top[] = {w.spatial_pos, w.temporal_pos, w.embed_w, w.embed_b, w.time_freq, w.time1_w, w.time1_b, w.time3_w, w.time3_b,
                        w.spatial_norm_w, w.spatial_norm_b, w.temporal_norm_w, w.temporal_norm_b, w.head_norm_w, w.head_norm_b,
                        w.head_w, w.head_b};
  for (const float* p : top)
    if (!p) return false;
  for (int d = 0; d < depth; ++d)
    if (!block_weights_complete(w.ste[d]) || !block_weights_complete(w.tte[d])) return false;
  return true;
}

}  // namespace

extern "C" {

int d3dp_set_weights(d3dp_ctx* c, const d3dp_weights* w, void* stream) {
  if (!c || !w || !w->ste || !w->tte) return d3dp_fail(D3DP_EINVAL, "d3dp_set_weights: null argument");
  if (!weights_complete(*w, c->cfg.depth)) return d3dp_fail(D3DP_EINVAL, "d3dp_set_weights: a weight pointer is null");
  hipStream_t st = (hipStream_t)stream;
  const d3dp_cfg& g = c->cfg;
  const size_t C = g.channels, Hd = g.hidden, J = g.joints, F = g.frames;
  // ---- EXACT f16x2: the range the weights PROVE for every data-dependent split-fp16 operand (d3dp_exact_range_bound), on
  // the device (one wave per weight row; 4 floats per block come back), and from it the operand scales of every block.
  //   LayerNorm output  |LN(x)_k| <= sqrt(C-1) |gamma_k| + |beta_k|                         (operand of qkv / fc1: fixed 2^4)
  //   q, k, v           |.| <= max_n sum_k |Wqkv[n,k]| in_k + |b_n|  -- and the attention output <= max |v|      (s_kv)
  //   MLP hidden        |GELU(y)| <= |y| <= the same form with Wfc1                                               (s_h)
  // A bound below 4094 keeps 2^4 (full 22 bits down to 2^-7); above it the scale drops to the largest power of two with
  // bound x scale < 65504: nothing can overflow to inf (the fp32 reference is finite there, so must this be -- VERDICT r3
  // item 5) and the representation error stays <= max(2^-22 |x|, 2^-25 / scale) <= 2^-40 x bound in absolute terms, far below
  // the fp32 rounding of the sums these operands enter.  A LayerNorm whose own output bound reaches 4094 (|gamma| ~ 180),
  // or an out-of-range q/k/v bound where the split-fp16 attention kernels do not apply, switches the whole context to the
  // six-pass split-bf16 implementation, which has fp32's exponent range (a padded-head context: to the fp32 implementation).
  c->range_bound = 0.f;
  c->impl_fallback = false;
  c->plan_total = -1;            // the pass plan depends on the implementation chosen below (x2-tuned or uniform passes)
  std::vector<float> blk_scale(4 * (size_t)g.depth, kActScale);      // [kind][d][s_kv, s_h]
  if (c->exact() && c->exact_impl_req == 0) {
    c->exact_impl = 0;
    const size_t nb = 2 * (size_t)g.depth;
    unsigned* dbound = nullptr;
    HIP_TRY(hipMalloc((void**)&dbound, nb * 6 * sizeof(unsigned)));
    struct Free { unsigned* p; ~Free() { (void)hipFree(p); } } free_dbound{dbound};
    HIP_TRY(hipMemsetAsync(dbound, 0, nb * 6 * sizeof(unsigned), st));
    for (int kind = 0; kind < 2; ++kind)
      for (int d = 0; d < g.depth; ++d) {
        const d3dp_block_weights& b = (kind == 0 ? w->ste : w->tte)[d];
        unsigned* o = dbound + ((size_t)kind * g.depth + d) * 6;
        d3dp_launch_rowbound(b.qkv_w, b.norm1_w, b.norm1_b, b.qkv_b, 3 * (int)C, (int)C, o, st);       // o[0] q/k/v, o[1] LN1 out
        d3dp_launch_rowbound(b.fc1_w, b.norm2_w, b.norm2_b, b.fc1_b, (int)Hd, (int)C, o + 2, st);      // o[2] hidden, o[3] LN2 out
        d3dp_launch_absmax(b.proj_w, C * C, o + 4, st);                                                // o[4], o[5]: the two matrices
        d3dp_launch_absmax(b.fc2_w, C * Hd, o + 5, st);                                                // no bound reads (inf check)
      }
    std::vector<float> hb(nb * 6);
    HIP_TRY(hipMemcpyAsync(hb.data(), dbound, nb * 6 * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const float kSafe = 65504.0f / kActScale;           // 4094: what 2^4 holds
    auto pick = [&](float bound) {                       // largest power of two <= 2^4 with bound x scale < 65504
      float sc = kActScale;
      while (!(bound * sc < 65504.0f) && sc > 1e-30f) sc *= 0.5f;
      return sc;
    };
    float worst = 0.f;
    bool fallback = false;
    for (size_t i = 0; i < nb; ++i) {
      const float bq = hb[6 * i], bl1 = hb[6 * i + 1], bh = hb[6 * i + 2], bl2 = hb[6 * i + 3];
      // Non-finite weights (a diverged checkpoint): ONE behaviour whichever tensor holds them -- the context moves
      // to the split-bf16 implementation, which has fp32's range and carries inf / nan through like the reference's fp32
      // kernels do; the output is then non-finite where the reference's is and d3dp_status reports it.  Never an error here.
      if (!(bq < INFINITY) || !(bh < INFINITY) || !(bl1 < INFINITY) || !(bl2 < INFINITY) || !(hb[6 * i + 4] < INFINITY) ||
          !(hb[6 * i + 5] < INFINITY)) {
        fallback = true;
        worst = INFINITY;
        continue;
      }
      worst = std::max(worst, std::max(std::max(bq, bh), std::max(bl1, bl2)));
      if (!(bl1 < kSafe) || !(bl2 < kSafe)) fallback = true;
      if (!(bq < kSafe) && !c->x2_attn()) fallback = true;   // (x2_attn(): head dims 64, 32 and 16 lower s_kv instead)
      blk_scale[2 * i] = pick(bq);
      blk_scale[2 * i + 1] = pick(bh);
    }
    c->range_bound = std::min(worst, 3.0e38f);
    if (fallback) {
      // split-bf16, six passes: no range limit.  A padded-head context (a width bf16x3 does not exist at) moves to the fp32
      // implementation instead: what it would run without its switch.
      c->exact_impl = c->hdp ? 2 : 1;
      c->impl_fallback = true;
      std::fill(blk_scale.begin(), blk_scale.end(), kActScale);
    }
  }
  // ---- FAST16: the range the weights PROVE for every tensor the context stores in 2 bytes, per block (header: d3dp_fast_operands)
  //   LayerNorm outputs      L1, L2  = max_k sqrt(C-1) |gamma_k| + |beta_k|
  //   q, k, v                b_qkv   = max_n sum_k |Wqkv[n,k]| (sqrt(C-1) |gamma1_k| + |beta1_k|) + |bqkv_n|;  b_v: rows n >= 2C alone
  //   attention output       <= b_v  (a convex combination of v rows; the probabilities themselves are <= 1)
  //   proj output            b_proj  = max_n sum_k |Wproj[n,k]| b_v + |bproj_n|
  //   MLP hidden             b_h     = the b_qkv form with Wfc1 / norm2  (|GELU(x)| <= |x|; it also bounds the pre-activation the
  //                                    streaming Linear parks as fp16 in front of the GELU)
  //   fc2 output             b_fc2   = max_n sum_k |Wfc2[n,k]| b_h + |bfc2_n|
  //   the four matrices      max |w|
  // The context's bound is the largest of these over all blocks.  Below 65504 and finite: fp16 operands, unscaled.  Otherwise
  // (or with a non-finite weight): the bf16 kernels, i.e. exactly what a D3DP_MODE_FAST context launches on these weights --
  // never an error, never an inf that FAST would not give.  Both types are 2 bytes, so nothing below depends on the outcome
  // but the conversion kernel's and the launchers' type argument.
  // D3DP_FAST16_RANGE=scale (c->fast16_scale): the four bounds a weight edit can push out of range -- b_qkv, b_proj, b_h, b_fc2 -- lower
  // their block's power-of-two multiplier for the tensors they cover instead (shift(): the smallest s >= 0 with bound x 2^-s < 65504;
  // ctx.h BlockDev::r_*), as pick() above does for EXACT.  LayerNorm outputs and the weight matrices are never scaled: L1, L2 and the
  // four max |w| must stay below 65504, every weight finite and every s <= kFast16MaxShift -- otherwise the bf16 kernels, as without
  // the switch.  fast_bound keeps its meaning: the proven maximum of the VALUES, so 'fp16' beside a bound >= 65504 means scaled.
  std::vector<int> blk_shift(8 * (size_t)g.depth, 0);                // [kind][d][r_qkv, r_proj, r_h, r_fc2]
  if (c->fast16()) {
    const size_t nb = 2 * (size_t)g.depth;
    unsigned* dbound = nullptr;
    HIP_TRY(hipMalloc((void**)&dbound, nb * kF16Slots * sizeof(unsigned)));
    struct Free { unsigned* p; ~Free() { (void)hipFree(p); } } free_dbound{dbound};
    HIP_TRY(hipMemsetAsync(dbound, 0, nb * kF16Slots * sizeof(unsigned), st));
    const double sq = std::sqrt((double)C - 1.0);
    for (int kind = 0; kind < 2; ++kind)
      for (int d = 0; d < g.depth; ++d) {
        const d3dp_block_weights& b = (kind == 0 ? w->ste : w->tte)[d];
        unsigned* o = dbound + ((size_t)kind * g.depth + d) * kF16Slots;
        const dim3 blk(256);
        hipLaunchKernelGGL(fast16_bound_kernel, dim3((3 * (unsigned)C + 3) / 4), blk, 0, st, b.qkv_w, b.norm1_w, b.norm1_b,
                           (const unsigned*)nullptr, b.qkv_b, 3 * (int)C, (int)C, sq, 2 * (int)C, o + 1, o + 2, o + 0, o + 7);
        hipLaunchKernelGGL(fast16_bound_kernel, dim3(((unsigned)C + 3) / 4), blk, 0, st, b.proj_w, (const float*)nullptr,
                           (const float*)nullptr, (const unsigned*)(o + 2), b.proj_b, (int)C, (int)C, 0.0, 0, o + 3,
                           (unsigned*)nullptr, (unsigned*)nullptr, o + 8);
        hipLaunchKernelGGL(fast16_bound_kernel, dim3(((unsigned)Hd + 3) / 4), blk, 0, st, b.fc1_w, b.norm2_w, b.norm2_b,
                           (const unsigned*)nullptr, b.fc1_b, (int)Hd, (int)C, sq, 0, o + 5, (unsigned*)nullptr, o + 4, o + 9);
        hipLaunchKernelGGL(fast16_bound_kernel, dim3(((unsigned)C + 3) / 4), blk, 0, st, b.fc2_w, (const float*)nullptr,
                           (const float*)nullptr, (const unsigned*)(o + 5), b.fc2_b, (int)C, (int)Hd, 0.0, 0, o + 6,
                           (unsigned*)nullptr, (unsigned*)nullptr, o + 10);
      }
    HIP_TRY(hipGetLastError());
    std::vector<float> hb(nb * kF16Slots);
    HIP_TRY(hipMemcpyAsync(hb.data(), dbound, hb.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    float worst = 0.f;
    bool finite = true;
    for (const float v : hb) {
      if (!(v < INFINITY)) finite = false;               // (inf, or the nan a nan weight leaves)
      else worst = std::max(worst, v);
    }
    c->fast_bound = finite ? worst : INFINITY;
    c->fast_f16 = (finite && worst < 65504.0f) ? 1 : 0;
    if (c->fast16_scale && finite && !c->fast_f16) {
      auto shift = [](float bound) {                     // (finite bounds only: at most 128 halvings)
        int sh = 0;
        while (!(ldexpf(bound, -sh) < 65504.0f)) ++sh;
        return sh;
      };
      bool ok = true;
      for (size_t i = 0; i < nb && ok; ++i) {
        const float* o = hb.data() + i * kF16Slots;     // (slots: fast16_bound_kernel's launches above)
        const int unscaled[] = {0, 4, 7, 8, 9, 10}, scaled[] = {1, 3, 5, 6};
        for (const int k : unscaled) ok = ok && o[k] < 65504.0f;
        for (int k = 0; k < 4; ++k) {
          blk_shift[4 * i + k] = shift(o[scaled[k]]);
          ok = ok && blk_shift[4 * i + k] <= kFast16MaxShift;
        }
      }
      if (ok) c->fast_f16 = 1;
      else std::fill(blk_shift.begin(), blk_shift.end(), 0);
    }
  }
  const size_t ws = c->fast() ? 2 : (c->x3() ? 6 : 4);   // bytes per weight-matrix element (bf16 or fp16 / 3 bf16 planes / fp32)
  // ---- arena layout ----
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += align_up(bytes); return o; };
  // (pad: 0 = a flat copy / split of n elements; a padded-head context running the split-fp16 implementation or a FAST mode packs 1 = the qkv
  //  matrix as [3 Cp][C], 2 = the proj matrix as [C][Cp], 3 = the qkv bias as [3 Cp] -- n_dst elements from the n of the source)
  struct Item { const void* src; size_t n; bool mat; size_t off; int pad; size_t n_dst; };
  std::vector<Item> items;
  const bool padded = (c->x2() || c->fast()) && c->hdp != 0;
  const size_t Cp = padded ? (size_t)c->cp() : C;
  auto add = [&](const void* src, size_t n, bool mat, int pad = 0, size_t n_dst = 0) {
    if (!padded) pad = 0;
    if (!pad) n_dst = n;
    items.push_back({src, n, mat, take(n_dst * (mat ? ws : 4)), pad, n_dst});
    return items.size() - 1;
  };
  const size_t i_spos = add(w->spatial_pos, J * C, false), i_tpos = add(w->temporal_pos, F * C, false);
  const size_t i_ew = add(w->embed_w, C * 5, false), i_eb = add(w->embed_b, C, false);
  const size_t i_fr = add(w->time_freq, C / 2, false);
  const size_t i_t1w = add(w->time1_w, 2 * C * C, false), i_t1b = add(w->time1_b, 2 * C, false);
  const size_t i_t3w = add(w->time3_w, 2 * C * C, false), i_t3b = add(w->time3_b, C, false);
  const size_t i_snw = add(w->spatial_norm_w, C, false), i_snb = add(w->spatial_norm_b, C, false);
  const size_t i_tnw = add(w->temporal_norm_w, C, false), i_tnb = add(w->temporal_norm_b, C, false);
  const size_t i_hnw = add(w->head_norm_w, C, false), i_hnb = add(w->head_norm_b, C, false);
  const size_t i_hw = add(w->head_w, 3 * C, false), i_hb = add(w->head_b, 3, false);
  struct BI { size_t v[13]; bool bgb; };
  std::vector<BI> bis;
  // fold_ln: fc1 runs on W diag(gamma2) with [c2 | c1] in place of its bias (computed into temporaries that live until the
  // synchronisation below)
  std::vector<float*> temps;
  struct TempFree { std::vector<float*>& t; ~TempFree() { for (float* p : t) (void)hipFree(p); } } temp_free{temps};
  for (int kind = 0; kind < 2; ++kind)
    for (int d = 0; d < g.depth; ++d) {
      const d3dp_block_weights& b = (kind == 0 ? w->ste : w->tte)[d];
      BI bi;
      bi.v[0] = add(b.norm1_w, C, false); bi.v[1] = add(b.norm1_b, C, false);
      bi.v[2] = add(b.qkv_w, 3 * C * C, true, 1, 3 * Cp * C); bi.v[3] = add(b.qkv_b, 3 * C, false, 3, 3 * Cp);
      bi.v[4] = add(b.proj_w, C * C, true, 2, C * Cp); bi.v[5] = add(b.proj_b, C, false);
      // defer_norm: gamma / beta of the shared norm in front of the block right behind proj's bias -- one array [b | gamma | beta]
      // (C floats are whole 256-byte units at the widths of the split-fp16 kernels, so the three items lie back to back)
      bi.bgb = c->defer_norm() && (C * 4) % kAlign == 0;
      if (bi.bgb) {
        add(kind == 0 ? w->temporal_norm_w : w->spatial_norm_w, C, false);
        add(kind == 0 ? w->temporal_norm_b : w->spatial_norm_b, C, false);
      }
      bi.v[6] = add(b.norm2_w, C, false); bi.v[7] = add(b.norm2_b, C, false);
      if (c->fold_ln()) {
        float *wp = nullptr, *c12 = nullptr;
        HIP_TRY(hipMalloc((void**)&wp, Hd * C * 4)); temps.push_back(wp);
        HIP_TRY(hipMalloc((void**)&c12, 2 * Hd * 4)); temps.push_back(c12);
        d3dp_launch_fold_ln(b.fc1_w, b.norm2_w, b.norm2_b, b.fc1_b, wp, c12, (int)Hd, (int)C, st);
        bi.v[8] = add(wp, Hd * C, true); bi.v[9] = add(b.fc1_b, Hd, false); bi.v[12] = add(c12, 2 * Hd, false);
      } else {
        bi.v[8] = add(b.fc1_w, Hd * C, true); bi.v[9] = add(b.fc1_b, Hd, false); bi.v[12] = bi.v[9];
      }
      bi.v[10] = add(b.fc2_w, C * Hd, true); bi.v[11] = add(b.fc2_b, C, false);
      bis.push_back(bi);
    }
  if (!c->arena || c->arena_bytes < off) {
    if (c->arena) HIP_TRY(hipFree(c->arena));
    c->arena = nullptr;
    HIP_TRY(hipMalloc((void**)&c->arena, off));
    c->arena_bytes = off;
  }
  // EXACT f16x2: every weight matrix is multiplied by 2^s, s = 14 - exponent(max |w|), before the hi/lo split (max |w| 2^s
  // in [2^13, 2^14): far from fp16 overflow, and the bulk of the matrix far above the subnormal range); the GEMM
  // multiplies its result by 2^-s.
  std::vector<float> unscale(items.size(), 1.f);
  if (c->x2()) {
    size_t n_mat = 0;
    for (auto& it : items) n_mat += it.mat;
    unsigned* dmax = nullptr;
    HIP_TRY(hipMalloc((void**)&dmax, n_mat * sizeof(unsigned)));
    HIP_TRY(hipMemsetAsync(dmax, 0, n_mat * sizeof(unsigned), st));
    size_t k = 0;
    for (auto& it : items)
      if (it.mat) d3dp_launch_absmax((const float*)it.src, it.n, dmax + k++, st);
    std::vector<float> hmax(n_mat);
    HIP_TRY(hipMemcpyAsync(hmax.data(), dmax, n_mat * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipFree(dmax));
    k = 0;
    for (size_t i = 0; i < items.size(); ++i) {
      if (!items[i].mat) continue;
      const float mx = hmax[k++];
      if (!(mx < INFINITY)) return d3dp_fail(D3DP_EINVAL, "d3dp_set_weights: a weight matrix holds inf/nan");
      int e = 0;
      if (mx > 0.f) frexpf(mx, &e);                  // mx = f 2^e, f in [0.5, 1)
      unscale[i] = ldexpf(1.f, e - 14);
    }
  }
  const int hd = g.channels / g.heads;
  for (size_t i = 0; i < items.size(); ++i) {
    auto& it = items[i];
    if (it.pad == 3)
      hipLaunchKernelGGL(pad_bias_kernel, dim3(((unsigned)it.n_dst + 255) / 256), dim3(256), 0, st, (const float*)it.src,
                         (float*)(c->arena + it.off), (int)it.n_dst, hd, c->hdp, g.heads);
    else if (it.pad && c->fast())   // (the plain cast of every FAST weight, to the type the range proof above chose)
      d3dp_launch_to_bf16_pad((const float*)it.src, c->arena + it.off, it.pad == 1 ? 3 * (int)Cp : (int)C, it.pad == 1 ? (int)C : (int)Cp,
                              (int)C, it.pad == 1 ? 1 : 0, hd, c->hdp, g.heads, st, c->fast_f16);
    else if (it.pad)     // (the same split arithmetic and the same per-matrix scale, from the absmax of the caller's unpadded matrix)
      hipLaunchKernelGGL(split2h_pad_kernel, dim3((unsigned)std::min<size_t>((it.n_dst + 255) / 256, 4096)), dim3(256), 0, st,
                         (const float*)it.src, (f16*)(c->arena + it.off), it.pad == 1 ? 3 * (int)Cp : (int)C,
                         it.pad == 1 ? (int)C : (int)Cp, (int)C, it.pad == 1 ? 1 : 0, hd, c->hdp, g.heads, 1.0f / unscale[i]);
    else if (it.mat && c->fast()) d3dp_launch_to_bf16((const float*)it.src, c->arena + it.off, it.n, st, c->fast_f16);
    else if (it.mat && c->x3()) d3dp_launch_split3((const float*)it.src, c->arena + it.off, it.n, st);
    else if (it.mat && c->x2()) d3dp_launch_split2((const float*)it.src, c->arena + it.off, it.n, 1.0f / unscale[i], st);
    else HIP_TRY(hipMemcpyAsync(c->arena + it.off, it.src, it.n * 4, hipMemcpyDeviceToDevice, st));
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  auto F32 = [&](size_t i) { return (const float*)(c->arena + items[i].off); };
  auto ANY = [&](size_t i) { return (const void*)(c->arena + items[i].off); };
  c->spos = F32(i_spos); c->tpos = F32(i_tpos); c->ew = F32(i_ew); c->eb = F32(i_eb); c->freq = F32(i_fr);
  c->t1w = F32(i_t1w); c->t1b = F32(i_t1b); c->t3w = F32(i_t3w); c->t3b = F32(i_t3b);
  c->snw = F32(i_snw); c->snb = F32(i_snb); c->tnw = F32(i_tnw); c->tnb = F32(i_tnb);
  c->hnw = F32(i_hnw); c->hnb = F32(i_hnb); c->hw = F32(i_hw); c->hb = F32(i_hb);
  c->ste.clear(); c->tte.clear();
  for (size_t k = 0; k < bis.size(); ++k) {
    const BI& bi = bis[k];
    BlockDev b{F32(bi.v[0]), F32(bi.v[1]), F32(bi.v[6]), F32(bi.v[7]), F32(bi.v[3]), F32(bi.v[5]), F32(bi.v[9]),
               F32(bi.v[11]), ANY(bi.v[2]), ANY(bi.v[4]), ANY(bi.v[8]), ANY(bi.v[10]),
               unscale[bi.v[2]], unscale[bi.v[4]], unscale[bi.v[8]], unscale[bi.v[10]], F32(bi.v[12]),
               blk_scale[2 * k], blk_scale[2 * k + 1]};
    if (bi.bgb) b.proj_bgb = F32(bi.v[5]);
    b.r_qkv = blk_shift[4 * k]; b.r_proj = blk_shift[4 * k + 1]; b.r_h = blk_shift[4 * k + 2]; b.r_fc2 = blk_shift[4 * k + 3];
    (k < (size_t)g.depth ? c->ste : c->tte).push_back(b);
  }
  c->weights_set = true;
  return D3DP_OK;
}

int d3dp_set_weights_borrowed(d3dp_ctx* c, const d3dp_weights* w) {
  if (!c || !w || !w->ste || !w->tte) return d3dp_fail(D3DP_EINVAL, "d3dp_set_weights_borrowed: null argument");
  if (!c->train()) return d3dp_fail(D3DP_ESTATE, "d3dp_set_weights_borrowed needs a D3DP_MODE_TRAIN context (fp32 weights)");
  if (!weights_complete(*w, c->cfg.depth)) return d3dp_fail(D3DP_EINVAL, "d3dp_set_weights_borrowed: a weight pointer is null");
  c->spos = w->spatial_pos; c->tpos = w->temporal_pos; c->ew = w->embed_w; c->eb = w->embed_b; c->freq = w->time_freq;
  c->t1w = w->time1_w; c->t1b = w->time1_b; c->t3w = w->time3_w; c->t3b = w->time3_b;
  c->snw = w->spatial_norm_w; c->snb = w->spatial_norm_b; c->tnw = w->temporal_norm_w; c->tnb = w->temporal_norm_b;
  c->hnw = w->head_norm_w; c->hnb = w->head_norm_b; c->hw = w->head_w; c->hb = w->head_b;
  c->ste.clear(); c->tte.clear();
  for (int kind = 0; kind < 2; ++kind)
    for (int d = 0; d < c->cfg.depth; ++d) {
      const d3dp_block_weights& b = (kind == 0 ? w->ste : w->tte)[d];
      BlockDev bd{b.norm1_w, b.norm1_b, b.norm2_w, b.norm2_b, b.qkv_b, b.proj_b, b.fc1_b, b.fc2_b, b.qkv_w, b.proj_w,
                  b.fc1_w, b.fc2_w};
      (kind == 0 ? c->ste : c->tte).push_back(bd);
    }
  c->weights_set = true;
  return D3DP_OK;
}

int d3dp_exact_range_bound(const d3dp_ctx* c, float* bound) {
  if (!c || !bound) return d3dp_fail(D3DP_EINVAL, "d3dp_exact_range_bound: null argument");
  if (!c->weights_set) return d3dp_fail(D3DP_ESTATE, "d3dp_exact_range_bound: weights not set");
  *bound = c->range_bound;
  return D3DP_OK;
}

int d3dp_exact_scales(const d3dp_ctx* c, float* s_kv, float* s_hidden, int32_t* implementation) {
  if (!c) return d3dp_fail(D3DP_EINVAL, "d3dp_exact_scales: null argument");
  if (!c->weights_set) return d3dp_fail(D3DP_ESTATE, "d3dp_exact_scales: weights not set");
  const int dep = c->cfg.depth;
  for (int i = 0; i < 2 * dep; ++i) {
    const BlockDev& b = i < dep ? c->ste[i] : c->tte[i - dep];
    if (s_kv) s_kv[i] = b.s_kv;
    if (s_hidden) s_hidden[i] = b.s_h;
  }
  if (implementation) *implementation = c->exact() ? c->exact_impl : -1;
  return D3DP_OK;
}

int d3dp_fast_operands(const d3dp_ctx* c, int32_t* type, float* bound) {
  if (!c || !type || !bound) return d3dp_fail(D3DP_EINVAL, "d3dp_fast_operands: null argument");
  if (!c->weights_set) return d3dp_fail(D3DP_ESTATE, "d3dp_fast_operands: weights not set");
  *type = c->fast() ? c->fast_f16 : -1;
  *bound = c->fast16() ? c->fast_bound : 0.f;
  return D3DP_OK;
}

}  // extern "C"
