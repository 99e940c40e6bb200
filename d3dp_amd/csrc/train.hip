// Row-wise / elementwise kernels of the TRAINING step (reference main.py:387-401 around
// common/diffusionpose.py:279-287 and the MixSTE2 train branch, common/mixste.py:215-225).  fp32 throughout.
// Linears (forward, dgrad, wgrad) reuse gemm_f32_kernel; attention forward reuses attn_rows_kernel<float>.
//
//   forward helpers : masked residual add (+LayerNorm), GELU
//   backward        : LayerNorm backward (dx, d-gamma, d-beta), GELU backward, column sums (bias grads), transposes
//                     (operands of the dgrad / wgrad GEMMs), attention backward (dQ | dK,dV), grouped row sums
//                     (position-embedding and time-embedding grads), embedding / head / time-MLP backward.
// DropPath (timm semantics: per-sample mask in {0, 1/keep}) enters as an optional per-sample scale of the branch
// output: sample = token / J for spatial blocks ((b f) n c), = (b, n) for temporal blocks ((b n) f c).
#include <cstdlib>

#include "common.h"
#include "kernels.h"

namespace {

__device__ __forceinline__ int sample_of(int tok, int axis, int F, int J) {
  return axis == 0 ? tok / J : (tok / (F * J)) * J + tok % J;
}

constexpr float kInvSqrt2 = 0.70710678118654752440f;
constexpr float kInvSqrt2Pi = 0.39894228040143267794f;

// A lane's slice of a C-channel row: NV = C / 64 values -- float4 groups at element (g 64 + lane) 4 when NV % 4 == 0 (16-byte
// accesses), scalars at i 64 + lane otherwise.
template <int C> struct TRow {
  static constexpr int NV = C / 64;
  static constexpr bool V4 = NV % 4 == 0;
  static __device__ __forceinline__ int col(int i, int lane) {
    if constexpr (V4) return ((i >> 2) * 64 + lane) * 4 + (i & 3);
    else return i * 64 + lane;
  }
  static __device__ __forceinline__ void load(const float* p, int lane, float (&v)[NV]) {
    if constexpr (V4) {
#pragma unroll
      for (int g = 0; g < NV / 4; ++g) {
        const float4 a = *reinterpret_cast<const float4*>(p + (g * 64 + lane) * 4);
        v[g * 4] = a.x; v[g * 4 + 1] = a.y; v[g * 4 + 2] = a.z; v[g * 4 + 3] = a.w;
      }
    } else {
#pragma unroll
      for (int i = 0; i < NV; ++i) v[i] = p[i * 64 + lane];
    }
  }
  static __device__ __forceinline__ void store(float* p, int lane, const float (&v)[NV]) {
    if constexpr (V4) {
#pragma unroll
      for (int g = 0; g < NV / 4; ++g)
        *reinterpret_cast<float4*>(p + (g * 64 + lane) * 4) = make_float4(v[g * 4], v[g * 4 + 1], v[g * 4 + 2], v[g * 4 + 3]);
    } else {
#pragma unroll
      for (int i = 0; i < NV; ++i) p[i * 64 + lane] = v[i];
    }
  }
  // (mean, 1 / sqrt(var + eps)) of the row a wave holds: two passes in registers
  static __device__ __forceinline__ void stats(const float (&v)[NV], float eps, float& mean, float& rstd) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) s += v[i];
    mean = wave_sum(s) * (1.0f / C);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) { const float d = v[i] - mean; q = fmaf(d, d, q); }
    rstd = 1.0f / sqrtf(wave_sum(q) * (1.0f / C) + eps);
  }
};

// One atomic per WORKGROUP for a kernel's result absmax (bit pattern of a non-negative float; amax may be null): the row
// kernels below walk the tokens grid-stride on at most kRowBlocks workgroups so that a launch ends with at most that many
// same-address atomics (one per wave of a 4,131-workgroup launch cost 56 us, profiles/r04_train_step_kernel_stats.md).
constexpr int kRowBlocks = 1024;
__device__ __forceinline__ void block_amax_commit(float m, unsigned* amax) {
  __shared__ float part_amax[4];
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) part_amax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0 && amax)
    atomicMax(amax, __float_as_uint(fmaxf(fmaxf(part_amax[0], part_amax[1]), fmaxf(part_amax[2], part_amax[3]))));
}

// A LayerNorm's output straight into the split-fp16 operand rows of the Linear behind it (round 6): no fp32 normalised tensor, no
// operand pass (round 5: the producer left the output's ABSMAX, rowprep_ln_kernel read the LayerNorm's input again and wrote the
// rows).  The operand scale must be known before the first element is written, and here it is, from the weights alone:
// sum x^2 <= C and sum x^ = 0 give |x^_i| <= sqrt(C - 1), so |LN(x)_i| <= sqrt(C - 1) max|gamma| + max|beta|.  The bound is a few binades
// above the true absmax (seed weights: 2^2 .. 2^3); a split operand keeps 22 bits of every element within 2^8 of its scale's range
// and an absolute error of 2^-40 of that range below, so nothing measurable is lost (test_training_step_* tolerances unchanged).
// ln_operand_scale: every wave of the launch derives the same power of two from the gamma / beta values its lanes hold.
template <int NV>
__device__ __forceinline__ float ln_operand_scale(const float (&wl)[NV], const float (&bl)[NV], int C, float& bound) {
  float gw = 0.f, gb = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) { gw = fmaxf(gw, fabsf(wl[i])); gb = fmaxf(gb, fabsf(bl[i])); }
  gw = wave_max(gw); gb = wave_max(gb);
  bound = fmaf(sqrtf((float)(C - 1)), gw, gb);
  if (!(bound > 0.f) || !(bound < INFINITY)) return 1.0f;
  int e;
  frexpf(bound, &e);                                   // (as gemm_x2.hip dyn_scale: the largest magnitude lands below 2^14)
  return ldexpf(1.0f, 14 - e);
}
// a lane's NV values of row `op_row` (TRow<C>::V4 layout: float4 groups at columns (g 64 + lane) 4) -> h2i split rows [.][2 C]
// (HI, D3DP_TRAIN_ROWS=hi: hi-only rows [.][C] -- the same hi value at column c, no lo value; kOpRow<C, HI> = fp16 elements per row)
template <int C, bool HI>
constexpr int kOpRow = HI ? C : 2 * C;
template <int C, int NV, bool HI = false>
__device__ __forceinline__ void store_operand_row(f16* op_row, int lane, const float (&v)[NV], float sc) {
#pragma unroll
  for (int g = 0; g < NV / 4; ++g) {
    f16x4 hi, lo;
#pragma unroll
    for (int e = 0; e < 4; ++e) { f16 h, l; split2h_scaled(v[g * 4 + e] * sc, h, l); hi[e] = h; lo[e] = l; }
    if constexpr (HI) {
      *reinterpret_cast<f16x4*>(op_row + (g * 64 + lane) * 4) = hi;
    } else {
      f16* d = op_row + h2i_col((g * 64 + lane) * 4);
      *reinterpret_cast<f16x4*>(d) = hi;
      *reinterpret_cast<f16x4*>(d + kH2iLo) = lo;
    }
  }
}

// ---- x_out = x_in + m[sample] * y ; xn = LN(x_out)  (+ absmax of xn: the fc1 operand) ------------------------------
// (op != null, C % 256 == 0: LN(x_out) as split operand rows [Tp][2 C] at the scale of ln_operand_scale, rows T .. Tp - 1 zero;
//  op_unscale[0] = 1 / scale, amax[0] = the bound)
template <int C, bool HI = false>
__global__ __launch_bounds__(256) void add_mask_ln_kernel(const float* __restrict__ x_in, const float* __restrict__ y,
                                                          const float* __restrict__ mask, int axis, int F, int J,
                                                          const float* __restrict__ w, const float* __restrict__ b,
                                                          float eps, float* __restrict__ x_out, float* __restrict__ xn,
                                                          unsigned* __restrict__ amax, int T, f16* __restrict__ op, int Tp,
                                                          float* __restrict__ op_unscale) {
  using R = TRow<C>;
  constexpr int NV = R::NV;
  const int lane = threadIdx.x & 63;
  float wl[NV], bl[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) { wl[i] = w[R::col(i, lane)]; bl[i] = b[R::col(i, lane)]; }
  float am = 0.f, sc = 1.f;
  if constexpr (R::V4) {
    if (op) {
      float bound;
      sc = ln_operand_scale<NV>(wl, bl, C, bound);
      if (blockIdx.x == 0 && threadIdx.x == 0) { op_unscale[0] = 1.0f / sc; if (amax) amax[0] = __float_as_uint(bound); }
    }
  }
  const int rows = (R::V4 && op) ? max(T, Tp) : T;
  for (int tok = blockIdx.x * 4 + (threadIdx.x >> 6); tok < rows; tok += gridDim.x * 4) {
    float v[NV];
    if (tok < T) {
      const float m = mask ? mask[sample_of(tok, axis, F, J)] : 1.0f;
      float yy[NV];
      R::load(x_in + (size_t)tok * C, lane, v);
      R::load(y + (size_t)tok * C, lane, yy);
#pragma unroll
      for (int i = 0; i < NV; ++i) v[i] = v[i] + m * yy[i];
      R::store(x_out + (size_t)tok * C, lane, v);
      float mean, rstd;
      R::stats(v, eps, mean, rstd);
#pragma unroll
      for (int i = 0; i < NV; ++i) { v[i] = fmaf((v[i] - mean) * rstd, wl[i], bl[i]); am = fmaxf(am, fabsf(v[i])); }
      if (xn) R::store(xn + (size_t)tok * C, lane, v);   // (null: only its absmax / its operand rows are wanted)
    } else {
#pragma unroll
      for (int i = 0; i < NV; ++i) v[i] = 0.f;           // (the TN weight-gradient product wants zero rows behind T)
    }
    if constexpr (R::V4) {
      if (op) store_operand_row<C, NV, HI>(op + (size_t)tok * kOpRow<C, HI>, lane, v, sc);
    }
  }
  if (!(R::V4 && op)) block_amax_commit(am, amax);
}

// ---- the end of a block in ONE pass over its rows (mixste.py:113-115 second line, then :243/:250 or :257/:273):
//   x_out = x_in + m[sample] * y ;  x_next = LN_a(x_out) (+ pos[f]) ;  xn = LN_b(x_next)  (+ absmax of xn)
// LN_a = the shared Spatial / Temporal norm, LN_b = the next block's norm1 (the head's LayerNorm after the last block;
// wb == nullptr: no second norm; xn == nullptr: LN_b's output is not stored, only its absmax).  As three kernels (add_mask_ln, ln_pos, ln_pos) the row was written and read back twice.
template <int C, bool HI = false>
__global__ __launch_bounds__(256) void add_mask_ln2_kernel(const float* __restrict__ x_in, const float* __restrict__ y,
                                                           const float* __restrict__ mask, int axis, int F, int J,
                                                           const float* __restrict__ wa, const float* __restrict__ ba, float eps_a,
                                                           const float* __restrict__ pos, const float* __restrict__ wb,
                                                           const float* __restrict__ bb, float eps_b, float* __restrict__ x_out,
                                                           float* __restrict__ x_next, float* __restrict__ xn,
                                                           unsigned* __restrict__ amax, int T, f16* __restrict__ op, int Tp,
                                                           float* __restrict__ op_unscale) {
  using R = TRow<C>;
  constexpr int NV = R::NV;
  const int lane = threadIdx.x & 63;
  float wal[NV], bal[NV], wbl[NV], bbl[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = R::col(i, lane);
    wal[i] = wa[c]; bal[i] = ba[c];
    wbl[i] = wb ? wb[c] : 0.f; bbl[i] = wb ? bb[c] : 0.f;
  }
  float am = 0.f, sc = 1.f;
  const bool to_op = R::V4 && op && wb;                  // (LN_b's output as the next Linear's operand rows: see add_mask_ln_kernel)
  if constexpr (R::V4) {
    if (to_op) {
      float bound;
      sc = ln_operand_scale<NV>(wbl, bbl, C, bound);
      if (blockIdx.x == 0 && threadIdx.x == 0) { op_unscale[0] = 1.0f / sc; if (amax) amax[0] = __float_as_uint(bound); }
    }
  }
  if constexpr (R::V4) {
    if (to_op)                                           // zero rows behind T (few: one workgroup pass)
      for (int tok = T + blockIdx.x * 4 + (threadIdx.x >> 6); tok < Tp; tok += gridDim.x * 4) {
        float z[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) z[i] = 0.f;
        store_operand_row<C, NV, HI>(op + (size_t)tok * kOpRow<C, HI>, lane, z, 1.0f);
      }
  }
  for (int tok = blockIdx.x * 4 + (threadIdx.x >> 6); tok < T; tok += gridDim.x * 4) {
    const float m = mask ? mask[sample_of(tok, axis, F, J)] : 1.0f;
    float v[NV], yy[NV];
    R::load(x_in + (size_t)tok * C, lane, v);
    R::load(y + (size_t)tok * C, lane, yy);
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = v[i] + m * yy[i];
    R::store(x_out + (size_t)tok * C, lane, v);
    float mean, rstd;
    R::stats(v, eps_a, mean, rstd);
    if (pos) {
      float pp[NV];
      R::load(pos + (size_t)((tok / J) % F) * C, lane, pp);
#pragma unroll
      for (int i = 0; i < NV; ++i) { float r = fmaf((v[i] - mean) * rstd, wal[i], bal[i]); r += pp[i]; v[i] = r; }
    } else {
#pragma unroll
      for (int i = 0; i < NV; ++i) v[i] = fmaf((v[i] - mean) * rstd, wal[i], bal[i]);
    }
    R::store(x_next + (size_t)tok * C, lane, v);
    if (wb) {                                            // (xn null: only the absmax of LN_b's output is wanted)
      R::stats(v, eps_b, mean, rstd);
#pragma unroll
      for (int i = 0; i < NV; ++i) { v[i] = fmaf((v[i] - mean) * rstd, wbl[i], bbl[i]); am = fmaxf(am, fabsf(v[i])); }
      if (xn) R::store(xn + (size_t)tok * C, lane, v);
      if constexpr (R::V4) {
        if (to_op) store_operand_row<C, NV, HI>(op + (size_t)tok * kOpRow<C, HI>, lane, v, sc);
      }
    }
  }
  if (!to_op) block_amax_commit(am, amax);
}

// ---- y = LN(x) (+ pos[f]) -- the fp32 cross-check path's recomputation of a Linear input in the backward pass -----------
template <int C>
__global__ __launch_bounds__(256) void ln_pos_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ b, float eps, const float* __restrict__ pos,
                                                     int F, int J, float* __restrict__ y, int T) {
  using R = TRow<C>;
  constexpr int NV = R::NV;
  const int lane = threadIdx.x & 63;
  float wl[NV], bl[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) { wl[i] = w[R::col(i, lane)]; bl[i] = b[R::col(i, lane)]; }
  for (int tok = blockIdx.x * 4 + (threadIdx.x >> 6); tok < T; tok += gridDim.x * 4) {
    float v[NV];
    R::load(x + (size_t)tok * C, lane, v);
    float mean, rstd;
    R::stats(v, eps, mean, rstd);
    const int f = (tok / J) % F;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      float r = fmaf((v[i] - mean) * rstd, wl[i], bl[i]);
      if (pos) r += pos[(size_t)f * C + R::col(i, lane)];
      v[i] = r;
    }
    R::store(y + (size_t)tok * C, lane, v);
  }
}

// ---- LayerNorm backward, one LayerNorm or two chained ones per pass over the rows ------------------------------------------
//   LN_b:  y = LN_b(xb), grad dy:   xhat = (xb - mean) rstd ; gg = dy gamma_b ;  g = rstd (gg - mean(gg) - xhat mean(gg xhat)) + dres
//   LN_a (TWO):  xb = LN_a(xa) (+ pos):  dx = the same formula on (g, xa, gamma_a);  ONE: dx = g
//   dxm = mask[sample] dx  (the DropPath-scaled dY of the branch below, with its absmax: the fused scale_mask pass)
// TWO covers the pairs the forward pass chains -- the head's LayerNorm over the last shared norm, a block's norm1 over the
// shared norm of the block before it: as two ln_bwd launches plus scale_mask the row went to memory and back twice more.
// dgamma / dbeta: every workgroup leaves ITS sums as one row [dgamma | dbeta] of `part_b` / `part_a` (gridDim.x rows of 2 C
// floats); d3dp_train_reduce_many adds the rows in a fixed order at the end of the backward pass -- no float atomics, so the
// step's gradients are bit-reproducible run to run.
// dy and dxm may alias (a wave reads its row of dy before it writes the row of dxm), hence no __restrict__ on them.
template <int C, bool TWO>
__global__ __launch_bounds__(256) void ln_bwd2_kernel(const float* dy, const float* __restrict__ xb, const float* __restrict__ wb,
                                                      float eps_b, const float* __restrict__ dres, float* __restrict__ g_out,
                                                      const float* __restrict__ xa, const float* __restrict__ wa, float eps_a,
                                                      float* __restrict__ dx, const float* __restrict__ mask, int axis, int F, int J,
                                                      float* dxm, unsigned* __restrict__ amax, float* __restrict__ part_b,
                                                      float* __restrict__ part_a, int T) {
  using R = TRow<C>;
  constexpr int NV = R::NV;
  __shared__ float sg[4][C], sb[4][C];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float agb[NV], abb[NV], wbl[NV];
  [[maybe_unused]] float aga[NV], aba[NV], wal[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    agb[i] = 0.f; abb[i] = 0.f; wbl[i] = wb[R::col(i, lane)];
    if constexpr (TWO) { aga[i] = 0.f; aba[i] = 0.f; wal[i] = wa[R::col(i, lane)]; }
  }
  const bool want_m = dxm != nullptr || amax != nullptr;
  float am = 0.f;
  // Every input row of a token -- xb, dy, the residual gradient, the second LayerNorm's input -- is requested up front, and the NEXT
  // token's rows while this one's are reduced (round 6): as loads issued where the formula first needs them (round 5) a row cost
  // three exposed memory latencies between its wave reductions, 41 - 43 us per launch against 24 - 30 us of HBM time.
  const int stride = gridDim.x * 4;
  auto load_row = [&](int tok, float (&vb)[NV], float (&dd)[NV], float (&dr)[NV], float (&va)[NV]) {
    R::load(xb + (size_t)tok * C, lane, vb);
    R::load(dy + (size_t)tok * C, lane, dd);
    if (dres) R::load(dres + (size_t)tok * C, lane, dr);
    if constexpr (TWO) R::load(xa + (size_t)tok * C, lane, va);
  };
  float v[NV], d[NV], dr[NV], va[NV], nv[NV], nd[NV], ndr[NV], nva[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) { dr[i] = 0.f; va[i] = 0.f; ndr[i] = 0.f; nva[i] = 0.f; }
  int tok = blockIdx.x * 4 + wv;
  if (tok < T) load_row(tok, v, d, dr, va);
  for (; tok < T; tok += stride) {
    const bool more = tok + stride < T;
    if (more) load_row(tok + stride, nv, nd, ndr, nva);
    float mean, rstd;
    R::stats(v, eps_b, mean, rstd);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      v[i] = (v[i] - mean) * rstd;                       // xhat
      agb[i] = fmaf(d[i], v[i], agb[i]);
      abb[i] += d[i];
      d[i] *= wbl[i];                                    // gg
      s1 += d[i];
      s2 = fmaf(d[i], v[i], s2);
    }
    s1 = wave_sum(s1) * (1.0f / C);
    s2 = wave_sum(s2) * (1.0f / C);
#pragma unroll
    for (int i = 0; i < NV; ++i) d[i] = rstd * (d[i] - s1 - v[i] * s2);
    if (dres) {
#pragma unroll
      for (int i = 0; i < NV; ++i) d[i] += dr[i];
    }
    if constexpr (TWO) {
      if (g_out) R::store(g_out + (size_t)tok * C, lane, d);
      R::stats(va, eps_a, mean, rstd);
      s1 = 0.f; s2 = 0.f;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        va[i] = (va[i] - mean) * rstd;
        aga[i] = fmaf(d[i], va[i], aga[i]);
        aba[i] += d[i];
        d[i] *= wal[i];
        s1 += d[i];
        s2 = fmaf(d[i], va[i], s2);
      }
      s1 = wave_sum(s1) * (1.0f / C);
      s2 = wave_sum(s2) * (1.0f / C);
#pragma unroll
      for (int i = 0; i < NV; ++i) d[i] = rstd * (d[i] - s1 - va[i] * s2);
    }
    R::store(dx + (size_t)tok * C, lane, d);
    if (want_m) {
      const float k = mask ? mask[sample_of(tok, axis, F, J)] : 1.0f;
#pragma unroll
      for (int i = 0; i < NV; ++i) { d[i] *= k; am = fmaxf(am, fabsf(d[i])); }
      if (dxm) R::store(dxm + (size_t)tok * C, lane, d);
    }
    if (more) {
#pragma unroll
      for (int i = 0; i < NV; ++i) { v[i] = nv[i]; d[i] = nd[i]; dr[i] = ndr[i]; va[i] = nva[i]; }
    }
  }
  // this workgroup's [dgamma | dbeta] rows: the four waves' sums in the order 0, 1, 2, 3
  auto flush = [&](const float (&ag)[NV], const float (&ab)[NV], float* part) {
#pragma unroll
    for (int i = 0; i < NV; ++i) { sg[wv][R::col(i, lane)] = ag[i]; sb[wv][R::col(i, lane)] = ab[i]; }
    __syncthreads();
    float* row = part + (size_t)blockIdx.x * 2 * C;
    for (int c = threadIdx.x; c < C; c += 256) {
      row[c] = ((sg[0][c] + sg[1][c]) + sg[2][c]) + sg[3][c];
      row[C + c] = ((sb[0][c] + sb[1][c]) + sb[2][c]) + sb[3][c];
    }
    __syncthreads();
  };
  flush(agb, abb, part_b);
  if constexpr (TWO) flush(aga, aba, part_a);
  if (want_m) block_amax_commit(am, amax);
}

// dst[i] (+)= sum over p < count of part[p stride + i] in a FIXED order (sixteen row groups, each summing its rows as eight
// interleaved chains, the groups added in order): the end of every partial sum of the backward pass (LayerNorm gammas / betas,
// biases, the small embedding-side gradients).  blockIdx.y = item; 64 columns x 16 row groups per workgroup; eight loads in
// flight per thread (the first version walked its rows one dependent load at a time: 228 us per launch for 100 MB).
__global__ __launch_bounds__(1024) void reduce_many_kernel(D3dpReduceTable tb) {
  __shared__ float acc[16][64];
  const D3dpReduceItem it = tb.it[blockIdx.y];
  if (blockIdx.x * 64 >= (int)it.n) return;
  const int l = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + l;
  const unsigned chunk = (it.count + 15) / 16;
  const unsigned p0 = rg * chunk, p1 = min(p0 + chunk, it.count);
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c < (int)it.n) {
    const float* src = it.part + c;
    unsigned p = p0;
    for (; p + 8 <= p1; p += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] += src[(size_t)(p + u) * it.stride];
    }
    for (int u = 0; p < p1; ++p, ++u) a[u] += src[(size_t)p * it.stride];
  }
  acc[rg][l] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  __syncthreads();
  if (rg == 0 && c < (int)it.n) {
    float t = acc[0][l];
#pragma unroll
    for (int g = 1; g < 16; ++g) t += acc[g][l];
    it.dst[c] = it.accumulate ? it.dst[c] + t : t;
  }
}

__device__ __forceinline__ float amax4f(const float4 v) { return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))); }

// (four elements per thread; n % 4 == 0: the hidden width is a multiple of 32)
__global__ __launch_bounds__(256) void gelu_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n4,
                                                       unsigned* __restrict__ amax) {
  float m = 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    // (the rational erf of the inference epilogue: fp32-class, half the instructions of libm's erff -- these two kernels
    //  are VALU-bound)
    const float4 r = make_float4(gelu_erf_rational(v.x), gelu_erf_rational(v.y), gelu_erf_rational(v.z), gelu_erf_rational(v.w));
    reinterpret_cast<float4*>(y)[i] = r;
    m = fmaxf(m, amax4f(r));
  }
  block_amax_commit(m, amax);
}

// dpre = dh * (Phi(x) + x phi(x))
__device__ __forceinline__ float gelu_grad(float v) { return gelu_grad_rational(v); }
__global__ __launch_bounds__(256) void gelu_bwd_kernel(const float* dh, const float* __restrict__ x, float* dpre, size_t n4,
                                                       unsigned* __restrict__ amax) {   // dpre may alias dh
  float m = 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float4 v = reinterpret_cast<const float4*>(x)[i], d = reinterpret_cast<const float4*>(dh)[i];
    const float4 r = make_float4(d.x * gelu_grad(v.x), d.y * gelu_grad(v.y), d.z * gelu_grad(v.z), d.w * gelu_grad(v.w));
    reinterpret_cast<float4*>(dpre)[i] = r;
    m = fmaxf(m, amax4f(r));
  }
  block_amax_commit(m, amax);
}

__global__ __launch_bounds__(256) void zero_many_kernel(D3dpZeroTable tb) {
  float* p = tb.p[blockIdx.y];
  const unsigned n = tb.n[blockIdx.y];
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) p[i] = 0.f;
}

// part[blockIdx.y][c] = sum over this workgroup row's tokens of in[t, c]  (gridDim.y partial rows of C floats, summed in a fixed
// order by reduce_many_kernel).  A thread owns four columns (one 16-byte load per row) of one row in four; the four row lanes
// of a workgroup meet in LDS.
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ in, float* __restrict__ part, int T, int C) {
  __shared__ float4 sh[4][64];
  const int cg = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = (blockIdx.x * 64 + cg) * 4;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c < C) {
    const int step = gridDim.y * 4;
    int t = blockIdx.y * 4 + rl;
    for (; t + 3 * step < T; t += 4 * step) {            // four independent loads in flight
      const float4 v0 = *reinterpret_cast<const float4*>(in + (size_t)t * C + c);
      const float4 v1 = *reinterpret_cast<const float4*>(in + (size_t)(t + step) * C + c);
      const float4 v2 = *reinterpret_cast<const float4*>(in + (size_t)(t + 2 * step) * C + c);
      const float4 v3 = *reinterpret_cast<const float4*>(in + (size_t)(t + 3 * step) * C + c);
      s.x += (v0.x + v1.x) + (v2.x + v3.x); s.y += (v0.y + v1.y) + (v2.y + v3.y);
      s.z += (v0.z + v1.z) + (v2.z + v3.z); s.w += (v0.w + v1.w) + (v2.w + v3.w);
    }
    for (; t < T; t += step) {
      const float4 v = *reinterpret_cast<const float4*>(in + (size_t)t * C + c);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  sh[rl][cg] = s;
  __syncthreads();
  if (rl == 0 && c < C) {
    const float4 a = sh[0][cg], b = sh[1][cg], d = sh[2][cg], e = sh[3][cg];
    *reinterpret_cast<float4*>(part + (size_t)blockIdx.y * C + c) =
        make_float4((a.x + b.x) + (d.x + e.x), (a.y + b.y) + (d.y + e.y), (a.z + b.z) + (d.z + e.z), (a.w + b.w) + (d.w + e.w));
  }
}

// out[z][g, c] = sum over the tokens of group g that slice z of gridDim.z owns of in[t, c]; group: 0 -> n = t % J, 1 -> f = (t / J) % F,
// 2 -> b = t / (F J).  gridDim.z partial tables of groups x C floats (gridDim.z == 1: the result itself); written, never added
// to: the slices meet in reduce_many_kernel, in order.
__global__ __launch_bounds__(256) void groupsum_kernel(const float* __restrict__ in, float* __restrict__ out, int T, int C,
                                                       int mode, int F, int J) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int g = blockIdx.y;
  if (c >= C) return;
  float s = 0.f;
  if (mode == 0) { for (int t = g + blockIdx.z * J; t < T; t += J * gridDim.z) s += in[(size_t)t * C + c]; }
  else if (mode == 1) {
    for (int b = blockIdx.z; b < T / (F * J); b += gridDim.z)
      for (int n = 0; n < J; ++n) s += in[((size_t)b * F * J + (size_t)g * J + n) * C + c];
  } else {
    for (int t = blockIdx.z; t < F * J; t += gridDim.z) s += in[((size_t)g * F * J + t) * C + c];
  }
  out[((size_t)blockIdx.z * gridDim.y + g) * C + c] = s;
}

// out[c, r] = in[r, c] for r < R, 0 for R <= r < Rpad     (in [R, C] -> out [C, Rpad])
__global__ __launch_bounds__(256) void transpose_pad_kernel(const float* __restrict__ in, float* __restrict__ out, int R,
                                                            int C, int Rpad) {
  __shared__ float tile[32][33];
  const int r0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = ty; k < 32; k += 8) {
    const int r = r0 + k, c = c0 + tx;
    tile[k][tx] = (r < R && c < C) ? in[(size_t)r * C + c] : 0.f;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int c = c0 + k, r = r0 + tx;
    if (c < C && r < Rpad) out[(size_t)c * Rpad + r] = tile[tx][k];
  }
}

// ---- attention backward --------------------------------------------------------------------------------------------
// Per (sequence, head): P = softmax(Q K^T s), O = P V.  Given dO:
//   D_i = dO_i . O_i ;  dS_ij = P_ij (dO_i . V_j - D_i) ;  dQ_i = s sum_j dS_ij K_j ; dK_j = s sum_i dS_ij Q_i ;
//   dV_j = sum_i P_ij dO_i.
// Pass 1 (thread per query row; K, V in LDS): row max m_i, denominator l_i, D_i, and dQ_i.
// Pass 2 (thread per key row; Q, dO in LDS, m/l/D from pass 1): dK_j, dV_j.
struct AttnStats { float m, l, D; };

// GEN (round 6: a head dim outside {8, 16, 32, 64}, i.e. a width train.hip does not instantiate): HD is the register / LDS
// capacity, the head dim itself the run-time hd_rt (a multiple of 4, <= HD); everything behind it is zero in q, k, v, dO and is
// not stored.
template <int HD, bool GEN = false>
__global__ __launch_bounds__(512) void attn_bwd_q_kernel(const float* __restrict__ qkv, const float* __restrict__ o,
                                                         const float* __restrict__ dout, float* __restrict__ dqkv,
                                                         AttnStats* __restrict__ stats, SeqMap map, int C, int heads, int hd_rt) {
  const int hd = GEN ? hd_rt : HD;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* Ks = reinterpret_cast<float*>(smem_raw);
  const int n = map.n_tok;
  constexpr int LDR = HD + 4;
  float* Vs = Ks + (size_t)n * LDR;
  const int seq = blockIdx.x / heads, head = blockIdx.x % heads;
  const int base = (seq / map.inner) * map.outer_stride + (seq % map.inner) * map.inner_stride;
  for (int u = threadIdx.x; u < n * (HD / 4); u += blockDim.x) {
    const int j = u / (HD / 4), c = u % (HD / 4);
    const float* src = qkv + (size_t)(base + j * map.tok_stride) * 3 * C + C + head * hd + c * 4;
    const bool in = !GEN || c * 4 < hd;
    *reinterpret_cast<float4*>(Ks + j * LDR + c * 4) = in ? *reinterpret_cast<const float4*>(src) : make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(Vs + j * LDR + c * 4) = in ? *reinterpret_cast<const float4*>(src + C) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  // two threads (adjacent lanes) per query row, each owning half of the head dimension: q, dO, dQ halves stay in
  // registers (96 instead of 192), partial dot products are combined with one lane exchange per key group
  const int i = threadIdx.x >> 1, half = threadIdx.x & 1;
  const bool live = i < n;
  const int ii = live ? i : n - 1;
  constexpr int HH = HD / 2;
  const size_t tok = (size_t)(base + ii * map.tok_stride);
  const float scale = 1.0f / sqrtf((float)hd);
  float q[HH], dO[HH], dq[HH];
  float D = 0.f;
#pragma unroll
  for (int d = 0; d < HH; ++d) {
    const bool in = !GEN || half * HH + d < hd;
    q[d] = in ? qkv[tok * 3 * C + head * hd + half * HH + d] : 0.f;
    dO[d] = in ? dout[tok * C + head * hd + half * HH + d] : 0.f;
    D = fmaf(dO[d], in ? o[tok * C + head * hd + half * HH + d] : 0.f, D);
    dq[d] = 0.f;
  }
  D += __shfl_xor(D, 1, 64);
  const float* Kh = Ks + half * HH;
  const float* Vh = Vs + half * HH;
  // KB keys at a time: independent dot-product chains.  Pass A: row max and denominator (online recurrence).
  constexpr int KB = 4;
  float m = -INFINITY, l = 0.f;
  for (int j0 = 0; j0 < n; j0 += KB) {
    float sc[KB];
#pragma unroll
    for (int u = 0; u < KB; ++u) sc[u] = 0.f;
#pragma unroll
    for (int c = 0; c < HH / 4; ++c) {
#pragma unroll
      for (int u = 0; u < KB; ++u) {
        const float4 kv = *reinterpret_cast<const float4*>(Kh + min(j0 + u, n - 1) * LDR + c * 4);
        sc[u] = fmaf(q[c * 4], kv.x, sc[u]); sc[u] = fmaf(q[c * 4 + 1], kv.y, sc[u]);
        sc[u] = fmaf(q[c * 4 + 2], kv.z, sc[u]); sc[u] = fmaf(q[c * 4 + 3], kv.w, sc[u]);
      }
    }
    float gm = m;
#pragma unroll
    for (int u = 0; u < KB; ++u) {
      sc[u] += __shfl_xor(sc[u], 1, 64);
      sc[u] = (j0 + u < n) ? sc[u] * scale : -INFINITY;
      gm = fmaxf(gm, sc[u]);
    }
    l *= expf(m - gm);
#pragma unroll
    for (int u = 0; u < KB; ++u) l += expf(sc[u] - gm);
    m = gm;
  }
  const float inv = 1.0f / l;
  // Pass B: dS_ij = P_ij (dO_i . V_j - D_i) s ;  dQ_i += dS_ij K_j
  for (int j0 = 0; j0 < n; j0 += KB) {
    float sc[KB], dp[KB];
#pragma unroll
    for (int u = 0; u < KB; ++u) { sc[u] = 0.f; dp[u] = 0.f; }
#pragma unroll
    for (int c = 0; c < HH / 4; ++c) {
#pragma unroll
      for (int u = 0; u < KB; ++u) {
        const int j = min(j0 + u, n - 1);
        const float4 kv = *reinterpret_cast<const float4*>(Kh + j * LDR + c * 4);
        const float4 vv = *reinterpret_cast<const float4*>(Vh + j * LDR + c * 4);
        sc[u] = fmaf(q[c * 4], kv.x, sc[u]); sc[u] = fmaf(q[c * 4 + 1], kv.y, sc[u]);
        sc[u] = fmaf(q[c * 4 + 2], kv.z, sc[u]); sc[u] = fmaf(q[c * 4 + 3], kv.w, sc[u]);
        dp[u] = fmaf(dO[c * 4], vv.x, dp[u]); dp[u] = fmaf(dO[c * 4 + 1], vv.y, dp[u]);
        dp[u] = fmaf(dO[c * 4 + 2], vv.z, dp[u]); dp[u] = fmaf(dO[c * 4 + 3], vv.w, dp[u]);
      }
    }
    float ds[KB];
#pragma unroll
    for (int u = 0; u < KB; ++u) {
      sc[u] += __shfl_xor(sc[u], 1, 64);
      dp[u] += __shfl_xor(dp[u], 1, 64);
      ds[u] = (j0 + u < n) ? expf(sc[u] * scale - m) * inv * (dp[u] - D) * scale : 0.f;
    }
#pragma unroll
    for (int c = 0; c < HH / 4; ++c) {
#pragma unroll
      for (int u = 0; u < KB; ++u) {
        const float4 kv = *reinterpret_cast<const float4*>(Kh + min(j0 + u, n - 1) * LDR + c * 4);
        dq[c * 4] = fmaf(ds[u], kv.x, dq[c * 4]); dq[c * 4 + 1] = fmaf(ds[u], kv.y, dq[c * 4 + 1]);
        dq[c * 4 + 2] = fmaf(ds[u], kv.z, dq[c * 4 + 2]); dq[c * 4 + 3] = fmaf(ds[u], kv.w, dq[c * 4 + 3]);
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int d = 0; d < HH; ++d)
    if (!GEN || half * HH + d < hd) dqkv[tok * 3 * C + head * hd + half * HH + d] = dq[d];
  if (half == 0) stats[(size_t)blockIdx.x * n + i] = AttnStats{m, l, D};
}

template <int HD, bool GEN = false>
__global__ __launch_bounds__(512) void attn_bwd_kv_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                          float* __restrict__ dqkv, const AttnStats* __restrict__ stats,
                                                          SeqMap map, int C, int heads, int hd_rt) {
  const int hd = GEN ? hd_rt : HD;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* Qs = reinterpret_cast<float*>(smem_raw);
  const int n = map.n_tok;
  constexpr int LDR = HD + 4;
  float* Os = Qs + (size_t)n * LDR;
  AttnStats* st = reinterpret_cast<AttnStats*>(Os + (size_t)n * LDR);
  const int seq = blockIdx.x / heads, head = blockIdx.x % heads;
  const int base = (seq / map.inner) * map.outer_stride + (seq % map.inner) * map.inner_stride;
  for (int u = threadIdx.x; u < n * (HD / 4); u += blockDim.x) {
    const int i = u / (HD / 4), c = u % (HD / 4);
    const size_t tok = (size_t)(base + i * map.tok_stride);
    const bool in = !GEN || c * 4 < hd;
    *reinterpret_cast<float4*>(Qs + i * LDR + c * 4) =
        in ? *reinterpret_cast<const float4*>(qkv + tok * 3 * C + head * hd + c * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(Os + i * LDR + c * 4) =
        in ? *reinterpret_cast<const float4*>(dout + tok * C + head * hd + c * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (int i = threadIdx.x; i < n; i += blockDim.x) st[i] = stats[(size_t)blockIdx.x * n + i];
  __syncthreads();
  // two threads (adjacent lanes) per key, each owning half of the head dimension of k, v, dK_j, dV_j; partial dot
  // products are combined with one lane exchange; KB queries at a time give independent FMA chains
  const int j = threadIdx.x >> 1, half = threadIdx.x & 1;
  const bool live = j < n;
  const int jj = live ? j : n - 1;
  constexpr int HH = HD / 2;
  const size_t tok = (size_t)(base + jj * map.tok_stride);
  const float scale = 1.0f / sqrtf((float)hd);
  float k[HH], v[HH], dk[HH], dv[HH];
#pragma unroll
  for (int d = 0; d < HH; ++d) {
    const bool in = !GEN || half * HH + d < hd;
    k[d] = in ? qkv[tok * 3 * C + C + head * hd + half * HH + d] : 0.f;
    v[d] = in ? qkv[tok * 3 * C + 2 * C + head * hd + half * HH + d] : 0.f;
    dk[d] = 0.f; dv[d] = 0.f;
  }
  const float* Qh = Qs + half * HH;
  const float* Oh = Os + half * HH;
  constexpr int KB = 2;
  for (int i0 = 0; i0 < n; i0 += KB) {
    float sc[KB], dp[KB];
#pragma unroll
    for (int u = 0; u < KB; ++u) { sc[u] = 0.f; dp[u] = 0.f; }
#pragma unroll
    for (int c = 0; c < HH / 4; ++c) {
#pragma unroll
      for (int u = 0; u < KB; ++u) {
        const int i = min(i0 + u, n - 1);
        const float4 qv = *reinterpret_cast<const float4*>(Qh + i * LDR + c * 4);
        const float4 ov = *reinterpret_cast<const float4*>(Oh + i * LDR + c * 4);
        sc[u] = fmaf(qv.x, k[c * 4], sc[u]); sc[u] = fmaf(qv.y, k[c * 4 + 1], sc[u]);
        sc[u] = fmaf(qv.z, k[c * 4 + 2], sc[u]); sc[u] = fmaf(qv.w, k[c * 4 + 3], sc[u]);
        dp[u] = fmaf(ov.x, v[c * 4], dp[u]); dp[u] = fmaf(ov.y, v[c * 4 + 1], dp[u]);
        dp[u] = fmaf(ov.z, v[c * 4 + 2], dp[u]); dp[u] = fmaf(ov.w, v[c * 4 + 3], dp[u]);
      }
    }
    float pr[KB], ds[KB];
#pragma unroll
    for (int u = 0; u < KB; ++u) {
      sc[u] += __shfl_xor(sc[u], 1, 64);
      dp[u] += __shfl_xor(dp[u], 1, 64);
      const AttnStats a = st[min(i0 + u, n - 1)];
      pr[u] = (i0 + u < n) ? expf(sc[u] * scale - a.m) / a.l : 0.f;
      ds[u] = pr[u] * (dp[u] - a.D) * scale;
    }
#pragma unroll
    for (int c = 0; c < HH / 4; ++c) {
#pragma unroll
      for (int u = 0; u < KB; ++u) {
        const int i = min(i0 + u, n - 1);
        const float4 qv = *reinterpret_cast<const float4*>(Qh + i * LDR + c * 4);
        const float4 ov = *reinterpret_cast<const float4*>(Oh + i * LDR + c * 4);
        dk[c * 4] = fmaf(ds[u], qv.x, dk[c * 4]); dk[c * 4 + 1] = fmaf(ds[u], qv.y, dk[c * 4 + 1]);
        dk[c * 4 + 2] = fmaf(ds[u], qv.z, dk[c * 4 + 2]); dk[c * 4 + 3] = fmaf(ds[u], qv.w, dk[c * 4 + 3]);
        dv[c * 4] = fmaf(pr[u], ov.x, dv[c * 4]); dv[c * 4 + 1] = fmaf(pr[u], ov.y, dv[c * 4 + 1]);
        dv[c * 4 + 2] = fmaf(pr[u], ov.z, dv[c * 4 + 2]); dv[c * 4 + 3] = fmaf(pr[u], ov.w, dv[c * 4 + 3]);
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int d = 0; d < HH; ++d) {
    if (GEN && half * HH + d >= hd) continue;
    dqkv[tok * 3 * C + C + head * hd + half * HH + d] = dk[d];
    dqkv[tok * 3 * C + 2 * C + head * hd + half * HH + d] = dv[d];
  }
}

// ---- the chunked forms of the two kernels above (D3DP_TRAIN_LONG_ATTN=chunked): any sequence length -------------------------------
// Grid (sequence x head, row blocks of 256): a thread pair still owns one query row (pass 1) / one key row (pass 2), and what the
// whole-sequence kernels hold in LDS for the whole sequence -- K, V; Q, dO, the statistics -- passes through it in chunks of CH rows
// (attn_bwd_chunk_rows: two images of pitch HD + 4 and the statistics within the CU's 160 KiB).  CH is a multiple of both kernels' KB, so
// that the groups of KB rows start where they start in the whole-sequence kernels and a clamped row min(j0 + u, n - 1) lies in the chunk
// being read.  Pass 1 walks the chunks twice: the online (m, l) recurrence, then dS and dQ -- what the whole-sequence kernel does over
// its one image.  The arithmetic and its order are those kernels': the same fmaf chains over keys / queries in ascending order, the
// same KB grouping, expf(m - gm) once per group, inv = 1 / l, / a.l in pass 2 -- so the gradients are bit-equal wherever both forms
// run (tests/test_hip_train_long.py).  Every thread of a block takes part in every barrier: a thread whose row lies beyond n stages,
// computes on row n - 1 and returns behind the last chunk without storing.  Two barriers per chunk, each in front of ~CH x HD
// fmaf per thread: their cost is noise.  LDS reads are one row address per half of a lane pair (a broadcast; the two halves lie
// HD / 2 dwords apart), the staging writes are 16-byte slots of consecutive lanes along rows of pitch HD + 4.  Pass 2 keeps a chunk
// row's Q and dO rows side by side (one per-lane LDS address and a constant offset serve both images: at capacity 128, where k, v,
// dK and dV alone fill the register file, that keeps its scratch below the whole-sequence kernel's; profiles/train_long_f32.md).
template <int HD> constexpr int attn_bwd_chunk_rows() { return HD <= 64 ? 256 : 128; }
constexpr int ATTN_BWD_BLOCK_ROWS = 256;

template <int HD, bool GEN = false>
__global__ __launch_bounds__(512) void attn_bwd_q_chunk_kernel(const float* __restrict__ qkv, const float* __restrict__ o,
                                                               const float* __restrict__ dout, float* __restrict__ dqkv,
                                                               AttnStats* __restrict__ stats, SeqMap map, int C, int heads, int hd_rt) {
  const int hd = GEN ? hd_rt : HD;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* Ks = reinterpret_cast<float*>(smem_raw);
  const int n = map.n_tok;
  constexpr int LDR = HD + 4, CH = attn_bwd_chunk_rows<HD>();
  float* Vs = Ks + (size_t)min(n, CH) * LDR;
  const int seq = blockIdx.x / heads, head = blockIdx.x % heads;
  const int base = (seq / map.inner) * map.outer_stride + (seq % map.inner) * map.inner_stride;
  // rows [c0, c0 + rows) of K (and of V) -> LDS; the barrier in front keeps the chunk before it until every thread has read it
  auto stage = [&](int c0, int rows, bool with_v) {
    __syncthreads();
    for (int u = threadIdx.x; u < rows * (HD / 4); u += blockDim.x) {
      const int j = u / (HD / 4), c = u % (HD / 4);
      const float* src = qkv + (size_t)(base + (c0 + j) * map.tok_stride) * 3 * C + C + head * hd + c * 4;
      const bool in = !GEN || c * 4 < hd;
      *reinterpret_cast<float4*>(Ks + j * LDR + c * 4) = in ? *reinterpret_cast<const float4*>(src) : make_float4(0.f, 0.f, 0.f, 0.f);
      if (with_v)
        *reinterpret_cast<float4*>(Vs + j * LDR + c * 4) = in ? *reinterpret_cast<const float4*>(src + C) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
  };
  const bool one = n <= CH;                              // one chunk: staged once, K and V, for both walks
  const int i = blockIdx.y * ATTN_BWD_BLOCK_ROWS + (threadIdx.x >> 1), half = threadIdx.x & 1;
  const bool live = i < n;
  const int ii = live ? i : n - 1;
  constexpr int HH = HD / 2;
  const size_t tok = (size_t)(base + ii * map.tok_stride);
  const float scale = 1.0f / sqrtf((float)hd);
  float q[HH], dO[HH], dq[HH];
  float D = 0.f;
#pragma unroll
  for (int d = 0; d < HH; ++d) {
    const bool in = !GEN || half * HH + d < hd;
    q[d] = in ? qkv[tok * 3 * C + head * hd + half * HH + d] : 0.f;
    dO[d] = in ? dout[tok * C + head * hd + half * HH + d] : 0.f;
    D = fmaf(dO[d], in ? o[tok * C + head * hd + half * HH + d] : 0.f, D);
    dq[d] = 0.f;
  }
  D += __shfl_xor(D, 1, 64);
  const float* Kh = Ks + half * HH;
  const float* Vh = Vs + half * HH;
  constexpr int KB = 4;
  static_assert(CH % KB == 0, "a group of KB keys lies in one chunk");
  // Walk A: row max and denominator (online recurrence)
  float m = -INFINITY, l = 0.f;
  for (int c0 = 0; c0 < n; c0 += CH) {
    const int c1 = min(c0 + CH, n);
    stage(c0, c1 - c0, one);
    for (int j0 = c0; j0 < c1; j0 += KB) {
      float sc[KB];
#pragma unroll
      for (int u = 0; u < KB; ++u) sc[u] = 0.f;
#pragma unroll
      for (int c = 0; c < HH / 4; ++c) {
#pragma unroll
        for (int u = 0; u < KB; ++u) {
          const float4 kv = *reinterpret_cast<const float4*>(Kh + (min(j0 + u, n - 1) - c0) * LDR + c * 4);
          sc[u] = fmaf(q[c * 4], kv.x, sc[u]); sc[u] = fmaf(q[c * 4 + 1], kv.y, sc[u]);
          sc[u] = fmaf(q[c * 4 + 2], kv.z, sc[u]); sc[u] = fmaf(q[c * 4 + 3], kv.w, sc[u]);
        }
      }
      float gm = m;
#pragma unroll
      for (int u = 0; u < KB; ++u) {
        sc[u] += __shfl_xor(sc[u], 1, 64);
        sc[u] = (j0 + u < n) ? sc[u] * scale : -INFINITY;
        gm = fmaxf(gm, sc[u]);
      }
      l *= expf(m - gm);
#pragma unroll
      for (int u = 0; u < KB; ++u) l += expf(sc[u] - gm);
      m = gm;
    }
  }
  const float inv = 1.0f / l;
  // Walk B: dS_ij = P_ij (dO_i . V_j - D_i) s ;  dQ_i += dS_ij K_j
  for (int c0 = 0; c0 < n; c0 += CH) {
    const int c1 = min(c0 + CH, n);
    if (!one) stage(c0, c1 - c0, true);
    for (int j0 = c0; j0 < c1; j0 += KB) {
      float sc[KB], dp[KB];
#pragma unroll
      for (int u = 0; u < KB; ++u) { sc[u] = 0.f; dp[u] = 0.f; }
#pragma unroll
      for (int c = 0; c < HH / 4; ++c) {
#pragma unroll
        for (int u = 0; u < KB; ++u) {
          const int j = min(j0 + u, n - 1) - c0;
          const float4 kv = *reinterpret_cast<const float4*>(Kh + j * LDR + c * 4);
          const float4 vv = *reinterpret_cast<const float4*>(Vh + j * LDR + c * 4);
          sc[u] = fmaf(q[c * 4], kv.x, sc[u]); sc[u] = fmaf(q[c * 4 + 1], kv.y, sc[u]);
          sc[u] = fmaf(q[c * 4 + 2], kv.z, sc[u]); sc[u] = fmaf(q[c * 4 + 3], kv.w, sc[u]);
          dp[u] = fmaf(dO[c * 4], vv.x, dp[u]); dp[u] = fmaf(dO[c * 4 + 1], vv.y, dp[u]);
          dp[u] = fmaf(dO[c * 4 + 2], vv.z, dp[u]); dp[u] = fmaf(dO[c * 4 + 3], vv.w, dp[u]);
        }
      }
      float ds[KB];
#pragma unroll
      for (int u = 0; u < KB; ++u) {
        sc[u] += __shfl_xor(sc[u], 1, 64);
        dp[u] += __shfl_xor(dp[u], 1, 64);
        ds[u] = (j0 + u < n) ? expf(sc[u] * scale - m) * inv * (dp[u] - D) * scale : 0.f;
      }
#pragma unroll
      for (int c = 0; c < HH / 4; ++c) {
#pragma unroll
        for (int u = 0; u < KB; ++u) {
          const float4 kv = *reinterpret_cast<const float4*>(Kh + (min(j0 + u, n - 1) - c0) * LDR + c * 4);
          dq[c * 4] = fmaf(ds[u], kv.x, dq[c * 4]); dq[c * 4 + 1] = fmaf(ds[u], kv.y, dq[c * 4 + 1]);
          dq[c * 4 + 2] = fmaf(ds[u], kv.z, dq[c * 4 + 2]); dq[c * 4 + 3] = fmaf(ds[u], kv.w, dq[c * 4 + 3]);
        }
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int d = 0; d < HH; ++d)
    if (!GEN || half * HH + d < hd) dqkv[tok * 3 * C + head * hd + half * HH + d] = dq[d];
  if (half == 0) stats[(size_t)blockIdx.x * n + i] = AttnStats{m, l, D};
}

template <int HD, bool GEN = false>
__global__ __launch_bounds__(512) void attn_bwd_kv_chunk_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                                float* __restrict__ dqkv, const AttnStats* __restrict__ stats,
                                                                SeqMap map, int C, int heads, int hd_rt) {
  const int hd = GEN ? hd_rt : HD;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* Qs = reinterpret_cast<float*>(smem_raw);
  const int n = map.n_tok;
  // (row i of the chunk: its Q row, then its dO row, each of pitch HD + 4 -- one per-lane LDS address serves both images)
  constexpr int LDR = HD + 4, LD2 = 2 * LDR, CH = attn_bwd_chunk_rows<HD>();
  float* Os = Qs + LDR;
  AttnStats* st = reinterpret_cast<AttnStats*>(Qs + (size_t)min(n, CH) * LD2);
  const int seq = blockIdx.x / heads, head = blockIdx.x % heads;
  const int base = (seq / map.inner) * map.outer_stride + (seq % map.inner) * map.inner_stride;
  const int j = blockIdx.y * ATTN_BWD_BLOCK_ROWS + (threadIdx.x >> 1), half = threadIdx.x & 1;
  const bool live = j < n;
  const int jj = live ? j : n - 1;
  constexpr int HH = HD / 2;
  const size_t tok = (size_t)(base + jj * map.tok_stride);
  const float scale = 1.0f / sqrtf((float)hd);
  float k[HH], v[HH], dk[HH], dv[HH];
#pragma unroll
  for (int d = 0; d < HH; ++d) {
    const bool in = !GEN || half * HH + d < hd;
    k[d] = in ? qkv[tok * 3 * C + C + head * hd + half * HH + d] : 0.f;
    v[d] = in ? qkv[tok * 3 * C + 2 * C + head * hd + half * HH + d] : 0.f;
    dk[d] = 0.f; dv[d] = 0.f;
  }
  const float* Qh = Qs + half * HH;
  const float* Oh = Os + half * HH;
  constexpr int KB = 2;
  static_assert(CH % KB == 0, "a group of KB queries lies in one chunk");
  for (int c0 = 0; c0 < n; c0 += CH) {
    const int c1 = min(c0 + CH, n);
    __syncthreads();                                     // (every thread has read the chunk before this one)
    for (int u = threadIdx.x; u < (c1 - c0) * (HD / 4); u += blockDim.x) {
      const int i = u / (HD / 4), c = u % (HD / 4);
      const size_t tk = (size_t)(base + (c0 + i) * map.tok_stride);
      const bool in = !GEN || c * 4 < hd;
      *reinterpret_cast<float4*>(Qs + i * LD2 + c * 4) =
          in ? *reinterpret_cast<const float4*>(qkv + tk * 3 * C + head * hd + c * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(Os + i * LD2 + c * 4) =
          in ? *reinterpret_cast<const float4*>(dout + tk * C + head * hd + c * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int i = threadIdx.x; i < c1 - c0; i += blockDim.x) st[i] = stats[(size_t)blockIdx.x * n + c0 + i];
    __syncthreads();
    for (int i0 = c0; i0 < c1; i0 += KB) {
      float sc[KB], dp[KB];
#pragma unroll
      for (int u = 0; u < KB; ++u) { sc[u] = 0.f; dp[u] = 0.f; }
#pragma unroll
      for (int c = 0; c < HH / 4; ++c) {
#pragma unroll
        for (int u = 0; u < KB; ++u) {
          const int i = min(i0 + u, n - 1) - c0;
          const float4 qv = *reinterpret_cast<const float4*>(Qh + i * LD2 + c * 4);
          const float4 ov = *reinterpret_cast<const float4*>(Oh + i * LD2 + c * 4);
          sc[u] = fmaf(qv.x, k[c * 4], sc[u]); sc[u] = fmaf(qv.y, k[c * 4 + 1], sc[u]);
          sc[u] = fmaf(qv.z, k[c * 4 + 2], sc[u]); sc[u] = fmaf(qv.w, k[c * 4 + 3], sc[u]);
          dp[u] = fmaf(ov.x, v[c * 4], dp[u]); dp[u] = fmaf(ov.y, v[c * 4 + 1], dp[u]);
          dp[u] = fmaf(ov.z, v[c * 4 + 2], dp[u]); dp[u] = fmaf(ov.w, v[c * 4 + 3], dp[u]);
        }
      }
      float pr[KB], ds[KB];
#pragma unroll
      for (int u = 0; u < KB; ++u) {
        sc[u] += __shfl_xor(sc[u], 1, 64);
        dp[u] += __shfl_xor(dp[u], 1, 64);
        const AttnStats a = st[min(i0 + u, n - 1) - c0];
        pr[u] = (i0 + u < n) ? expf(sc[u] * scale - a.m) / a.l : 0.f;
        ds[u] = pr[u] * (dp[u] - a.D) * scale;
      }
#pragma unroll
      for (int c = 0; c < HH / 4; ++c) {
#pragma unroll
        for (int u = 0; u < KB; ++u) {
          const int i = min(i0 + u, n - 1) - c0;
          const float4 qv = *reinterpret_cast<const float4*>(Qh + i * LD2 + c * 4);
          const float4 ov = *reinterpret_cast<const float4*>(Oh + i * LD2 + c * 4);
          dk[c * 4] = fmaf(ds[u], qv.x, dk[c * 4]); dk[c * 4 + 1] = fmaf(ds[u], qv.y, dk[c * 4 + 1]);
          dk[c * 4 + 2] = fmaf(ds[u], qv.z, dk[c * 4 + 2]); dk[c * 4 + 3] = fmaf(ds[u], qv.w, dk[c * 4 + 3]);
          dv[c * 4] = fmaf(pr[u], ov.x, dv[c * 4]); dv[c * 4 + 1] = fmaf(pr[u], ov.y, dv[c * 4 + 1]);
          dv[c * 4 + 2] = fmaf(pr[u], ov.z, dv[c * 4 + 2]); dv[c * 4 + 3] = fmaf(pr[u], ov.w, dv[c * 4 + 3]);
        }
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int d = 0; d < HH; ++d) {
    if (GEN && half * HH + d >= hd) continue;
    dqkv[tok * 3 * C + C + head * hd + half * HH + d] = dk[d];
    dqkv[tok * 3 * C + 2 * C + head * hd + half * HH + d] = dv[d];
  }
}

// ---- embedding backward: dW[c, i] = sum_t dx[t, c] in5[t, i] ; in5 = (u, v, x, y, z); gridDim.y partial tables of 5 C floats ----
__global__ __launch_bounds__(256) void embed_bwd_kernel(const float* __restrict__ dx, const float* __restrict__ x2d,
                                                        const float* __restrict__ x3d, float* __restrict__ part, int T, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float a[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  // eight rows' loads in flight per thread (one dependent load at a time this pass over 34 MB took 96 us); a fixed order all the same
  for (int t0 = blockIdx.y; t0 < T; t0 += 8 * gridDim.y) {
    float d[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int t = t0 + u * gridDim.y;
      d[u] = t < T ? dx[(size_t)t * C + c] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int t = min(t0 + u * (int)gridDim.y, T - 1);     // (rows behind T: d = 0)
      a[0] = fmaf(d[u], x2d[(size_t)t * 2], a[0]);
      a[1] = fmaf(d[u], x2d[(size_t)t * 2 + 1], a[1]);
      a[2] = fmaf(d[u], x3d[(size_t)t * 3], a[2]);
      a[3] = fmaf(d[u], x3d[(size_t)t * 3 + 1], a[3]);
      a[4] = fmaf(d[u], x3d[(size_t)t * 3 + 2], a[4]);
    }
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) part[(size_t)blockIdx.y * 5 * C + c * 5 + i] = a[i];
}

// ---- head: pred[t, o] = sum_c z[t, c] W[o, c] + b[o]  (o < 3) -------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void head_linear_kernel(const float* __restrict__ z, const float* __restrict__ w,
                                                          const float* __restrict__ b, float* __restrict__ out, int T) {
  constexpr int NV = C / 64;
  const int lane = threadIdx.x & 63;
  const int tok = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tok >= T) return;
  float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = i * 64 + lane;
    const float v = z[(size_t)tok * C + c];
#pragma unroll
    for (int o = 0; o < 3; ++o) acc[o] = fmaf(v, w[o * C + c], acc[o]);
  }
#pragma unroll
  for (int o = 0; o < 3; ++o) acc[o] = wave_sum(acc[o]) + b[o];
  if (lane < 3) out[(size_t)tok * 3 + lane] = lane == 0 ? acc[0] : (lane == 1 ? acc[1] : acc[2]);
}

// dz[t, c] = sum_o g[t, o] W[o, c] ; dW[o, c] = sum_t g[t, o] z[t, c] ; db[o] = sum_t g[t, o]: gridDim.y partial rows of
// 3 C + 4 floats ([dW | db, -]), summed in a fixed order by reduce_many_kernel
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ g, const float* __restrict__ z,
                                                       const float* __restrict__ w, float* __restrict__ dz,
                                                       float* __restrict__ part, int T, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float a[3] = {0.f, 0.f, 0.f}, sb[3] = {0.f, 0.f, 0.f};
  const float w0 = w[c], w1 = w[C + c], w2 = w[2 * C + c];
  for (int t = blockIdx.y; t < T; t += gridDim.y) {
    const float g0 = g[(size_t)t * 3], g1 = g[(size_t)t * 3 + 1], g2 = g[(size_t)t * 3 + 2];
    const float zz = z[(size_t)t * C + c];
    dz[(size_t)t * C + c] = g0 * w0 + g1 * w1 + g2 * w2;
    a[0] = fmaf(g0, zz, a[0]); a[1] = fmaf(g1, zz, a[1]); a[2] = fmaf(g2, zz, a[2]);
    if (c == 0) { sb[0] += g0; sb[1] += g1; sb[2] += g2; }
  }
  float* row = part + (size_t)blockIdx.y * (3 * C + 4);
#pragma unroll
  for (int o = 0; o < 3; ++o) row[o * C + c] = a[o];
  if (c == 0) { row[3 * C] = sb[0]; row[3 * C + 1] = sb[1]; row[3 * C + 2] = sb[2]; }
}

// ---- time MLP forward for the training step: one WAVE per output unit, coalesced weight rows ----------------------------
// (mixste.py:127-139, 179-184.  The inference kernel -- one workgroup per batch element, one serial dot product per thread with
//  strided weight reads -- is invisible beside a 6-second sampler call but was 175 us = 0.8 % of the configs[4] step.)
// layer 1: h[b][o] = GELU(sum_k e_b[k] w1[o][k] + b1[o]),  e_b = [sin(t_b freq) | cos(t_b freq)],  o < 2 C
__global__ __launch_bounds__(256) void time_mlp1_kernel(const int64_t* __restrict__ t, const float* __restrict__ freq,
                                                        const float* __restrict__ w1, const float* __restrict__ b1,
                                                        float* __restrict__ h, int B, int C) {
  const int lane = threadIdx.x & 63;
  const int unit = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit >= B * 2 * C) return;
  const int b = unit / (2 * C), o = unit - b * 2 * C, half = C / 2;
  const float tv = (float)t[b];
  const float* wr = w1 + (size_t)o * C;
  float a = 0.f;
  for (int k = lane; k < C; k += 64) {
    const float e = k < half ? sinf(tv * freq[k]) : cosf(tv * freq[k - half]);
    a = fmaf(e, wr[k], a);
  }
  a = wave_sum(a);
  if (lane == 0) h[unit] = gelu_erf(a + b1[o]);
}
// layer 2: temb[b][o] = sum_k h[b][k] w2[o][k] + b2[o],  o < C
__global__ __launch_bounds__(256) void time_mlp2_kernel(const float* __restrict__ h, const float* __restrict__ w2,
                                                        const float* __restrict__ b2, float* __restrict__ temb, int B, int C) {
  const int lane = threadIdx.x & 63;
  const int unit = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit >= B * C) return;
  const int b = unit / C, o = unit - b * C;
  const float* wr = w2 + (size_t)o * 2 * C;
  const float* hb = h + (size_t)b * 2 * C;
  float a = 0.f;
  for (int k = lane; k < 2 * C; k += 64) a = fmaf(hb[k], wr[k], a);
  a = wave_sum(a);
  if (lane == 0) temb[unit] = a + b2[o];
}

// ---- time MLP backward: one WAVE per hidden unit k of the 2C ---------------------------------------------------------
// (mixste.py:127-139: sinusoid -> Linear(C, 2C) -> GELU -> Linear(2C, C)).  The wave keeps row k of w1 and column k of w2
// in registers, walks the batch in order (deterministic sums, no atomics) and owns row k of dw1, column k of dw2 and
// db1[k]; the first C / 64 waves also write db2.  (The first version ran one workgroup per batch element with strided
// weight reads and atomics into the shared gradients: 1.0 ms of the configs[4] step for 4 MFLOP.)
template <int C>
__global__ __launch_bounds__(256) void time_mlp_bwd_kernel(const int64_t* __restrict__ t, const float* __restrict__ freq,
                                                           const float* __restrict__ w1, const float* __restrict__ b1,
                                                           const float* __restrict__ w2, const float* __restrict__ dtemb,
                                                           float* __restrict__ dw1, float* __restrict__ db1,
                                                           float* __restrict__ dw2, float* __restrict__ db2, int B) {
  constexpr int NV = C / 64, HALF = C / 2;
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);     // hidden unit
  if (k >= 2 * C) return;
  float w1r[NV], w2c[NV], fr[NV], g1[NV], g2[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int j = i * 64 + lane;                         // input channel j of the sinusoid / output channel j of the MLP
    w1r[i] = w1[(size_t)k * C + j];
    w2c[i] = w2[(size_t)j * 2 * C + k];
    fr[i] = freq[j < HALF ? j : j - HALF];
    g1[i] = 0.f; g2[i] = 0.f;
  }
  const float bias = b1[k];
  float gb1 = 0.f;
  for (int b = 0; b < B; ++b) {
    const float tv = (float)t[b];
    float e[NV], dy[NV];
    float pre = 0.f, dg = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int j = i * 64 + lane;
      const float a = tv * fr[i];
      e[i] = j < HALF ? sinf(a) : cosf(a);
      dy[i] = dtemb[(size_t)b * C + j];
      pre = fmaf(e[i], w1r[i], pre);
      dg = fmaf(dy[i], w2c[i], dg);
    }
    pre = wave_sum(pre) + bias;
    dg = wave_sum(dg);
    const float act = gelu_erf(pre);
    const float cdf = 0.5f * (1.0f + erff(pre * kInvSqrt2));
    const float pdf = kInvSqrt2Pi * expf(-0.5f * pre * pre);
    const float dpre = dg * (cdf + pre * pdf);
    gb1 += dpre;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      g1[i] = fmaf(dpre, e[i], g1[i]);
      g2[i] = fmaf(dy[i], act, g2[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int j = i * 64 + lane;
    dw1[(size_t)k * C + j] += g1[i];
    dw2[(size_t)j * 2 * C + k] += g2[i];
  }
  if (lane == 0) db1[k] += gb1;
  if (k < NV) {                                          // db2[j] for j = k * 64 + lane
    float a = 0.f;
    for (int b = 0; b < B; ++b) a += dtemb[(size_t)b * C + k * 64 + lane];
    db2[k * 64 + lane] += a;
  }
}

}  // namespace

#define TRAIN_DISPATCH_C(C, ...)                    \
  switch (C) {                                      \
    case 512: { constexpr int CC = 512; __VA_ARGS__; break; } \
    case 256: { constexpr int CC = 256; __VA_ARGS__; break; } \
    case 128: { constexpr int CC = 128; __VA_ARGS__; break; } \
    case 64:  { constexpr int CC = 64;  __VA_ARGS__; break; } \
    default: return -2;                             \
  }

#define TRAIN_DISPATCH_C256(C, ...)                 \
  switch (C) {                                      \
    case 512: { constexpr int CC = 512; __VA_ARGS__; break; } \
    case 256: { constexpr int CC = 256; __VA_ARGS__; break; } \
    default: return -2;                             \
  }

static int row_blocks(int T) { return (T + 3) / 4 < kRowBlocks ? (T + 3) / 4 : kRowBlocks; }
int d3dp_train_add_mask_ln(const float* x_in, const float* y, const float* mask, int axis, int F, int J, const float* w,
                           const float* b, float eps, float* x_out, float* xn, unsigned* amax, int T, int C, hipStream_t st,
                           void* op, int Tp, float* op_unscale, int op_hi) {
  if (!d3dp_width_instantiated(C))                     // (a run-time width: no operand rows)
    return op ? -2 : d3dp_train_g_add_mask_ln(x_in, y, mask, axis, F, J, w, b, eps, x_out, xn, amax, T, C, st);
  if (!w || !b || (!xn && !amax && !op) || (op && (C % 256 != 0 || Tp < T || !op_unscale))) return -1;
  if (op && op_hi) {                                   // (operand rows exist at C % 256 == 0: the two widths below)
    TRAIN_DISPATCH_C256(C, hipLaunchKernelGGL((add_mask_ln_kernel<CC, true>), dim3(row_blocks(T)), dim3(256), 0, st, x_in, y, mask, axis,
                                              F, J, w, b, eps, x_out, xn, amax, T, (f16*)op, Tp, op_unscale))
    return 0;
  }
  TRAIN_DISPATCH_C(C, hipLaunchKernelGGL((add_mask_ln_kernel<CC>), dim3(row_blocks(T)), dim3(256), 0, st, x_in, y, mask, axis,
                                         F, J, w, b, eps, x_out, xn, amax, T, (f16*)op, Tp, op_unscale))
  return 0;
}
int d3dp_train_add_mask_ln2(const float* x_in, const float* y, const float* mask, int axis, int F, int J, const float* wa,
                            const float* ba, float eps_a, const float* pos, const float* wb, const float* bb, float eps_b,
                            float* x_out, float* x_next, float* xn, unsigned* amax, int T, int C, hipStream_t st, void* op, int Tp,
                            float* op_unscale, int op_hi) {
  if (!d3dp_width_instantiated(C))
    return op ? -2 : d3dp_train_g_add_mask_ln2(x_in, y, mask, axis, F, J, wa, ba, eps_a, pos, wb, bb, eps_b, x_out, x_next, xn, amax, T, C, st);
  if (!wa || !ba || !x_out || !x_next || (xn && !wb) || (wb && !bb) || (op && (C % 256 != 0 || Tp < T || !op_unscale || !wb))) return -1;
  if (op && op_hi) {
    TRAIN_DISPATCH_C256(C, hipLaunchKernelGGL((add_mask_ln2_kernel<CC, true>), dim3(row_blocks(T)), dim3(256), 0, st, x_in, y, mask, axis,
                                              F, J, wa, ba, eps_a, pos, wb, bb, eps_b, x_out, x_next, xn, amax, T, (f16*)op, Tp, op_unscale))
    return 0;
  }
  TRAIN_DISPATCH_C(C, hipLaunchKernelGGL((add_mask_ln2_kernel<CC>), dim3(row_blocks(T)), dim3(256), 0, st, x_in, y, mask, axis,
                                         F, J, wa, ba, eps_a, pos, wb, bb, eps_b, x_out, x_next, xn, amax, T, (f16*)op, Tp, op_unscale))
  return 0;
}
int d3dp_train_ln_pos(const float* x, const float* w, const float* b, float eps, const float* pos, int F, int J, float* y,
                      int T, int C, hipStream_t st) {
  if (!d3dp_width_instantiated(C)) return d3dp_train_g_ln_pos(x, w, b, eps, pos, F, J, y, T, C, st);
  TRAIN_DISPATCH_C(C, hipLaunchKernelGGL((ln_pos_kernel<CC>), dim3(row_blocks(T)), dim3(256), 0, st, x, w, b, eps, pos, F, J,
                                         y, T))
  return 0;
}
// (D3DP_LN_BWD_BLOCKS workgroups: two per CU; every workgroup ends with one partial row per LayerNorm)
// (d3dp_train_ln_bwd_blocks(T), train_plan.h: the workgroups of a call over T tokens)
int d3dp_train_ln_bwd(const float* dy, const float* xb, const float* wb, float eps_b, const float* dres, float* g_out,
                      const float* xa, const float* wa, float eps_a, float* dx, const float* mask, int axis, int F, int J,
                      float* dxm, unsigned* amax, float* part_b, float* part_a, int T, int C, hipStream_t st) {
  if (!dy || !xb || !wb || !dx || !part_b || (xa && (!wa || !part_a))) return -1;
  const int blocks = d3dp_train_ln_bwd_blocks(T);
  if (!d3dp_width_instantiated(C))
    return d3dp_train_g_ln_bwd(dy, xb, wb, eps_b, dres, g_out, xa, wa, eps_a, dx, mask, axis, F, J, dxm, amax, part_b, part_a, T, C, blocks, st);
  if (xa) {
    TRAIN_DISPATCH_C(C, hipLaunchKernelGGL((ln_bwd2_kernel<CC, true>), dim3(blocks), dim3(256), 0, st, dy, xb, wb, eps_b, dres,
                                           g_out, xa, wa, eps_a, dx, mask, axis, F, J, dxm, amax, part_b, part_a, T))
  } else {
    TRAIN_DISPATCH_C(C, hipLaunchKernelGGL((ln_bwd2_kernel<CC, false>), dim3(blocks), dim3(256), 0, st, dy, xb, wb, eps_b, dres,
                                           nullptr, nullptr, nullptr, 0.f, dx, mask, axis, F, J, dxm, amax, part_b, nullptr, T))
  }
  return 0;
}
int d3dp_train_reduce_many(const D3dpReduceTable& tb, hipStream_t st) {
  if (tb.count < 1 || tb.count > D3DP_REDUCE_MAX) return -1;
  unsigned nmax = 1;
  for (int i = 0; i < tb.count; ++i) {
    if (!tb.it[i].part || !tb.it[i].dst || tb.it[i].n == 0) return -1;
    nmax = tb.it[i].n > nmax ? tb.it[i].n : nmax;
  }
  hipLaunchKernelGGL(reduce_many_kernel, dim3((nmax + 63) / 64, tb.count), dim3(1024), 0, st, tb);
  return 0;
}
static unsigned ew_blocks(size_t n4) { return (unsigned)((n4 + 255) / 256 < 512 ? (n4 + 255) / 256 : 512); }
int d3dp_train_gelu_fwd(const float* x, float* y, size_t n, unsigned* amax, hipStream_t st) {
  if (n % 4 != 0 || n == 0) return -2;
  hipLaunchKernelGGL(gelu_fwd_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, st, x, y, n / 4, amax);
  return 0;
}
int d3dp_train_gelu_bwd(const float* dh, const float* x, float* dpre, size_t n, unsigned* amax, hipStream_t st) {
  if (n % 4 != 0 || n == 0) return -2;
  hipLaunchKernelGGL(gelu_bwd_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, st, dh, x, dpre, n / 4, amax);
  return 0;
}
int d3dp_train_zero_many(const D3dpZeroTable& tb, hipStream_t st) {
  if (tb.count < 1 || tb.count > D3DP_ZERO_MAX) return -1;
  hipLaunchKernelGGL(zero_many_kernel, dim3(4, tb.count), dim3(256), 0, st, tb);
  return 0;
}
// partial rows of C floats; *rows = how many (<= max_rows <= 512)
int d3dp_train_colsum(const float* in, float* part, int* rows, int max_rows, int T, int C, hipStream_t st) {
  if (C % 4 != 0 || !rows || max_rows < 1) return -2;
  const int gx = (C + 255) / 256;
  int gy = 512 / gx;                                     // ~512 workgroups: two per CU
  if (gy > max_rows) gy = max_rows;
  if (gy > (T + 3) / 4) gy = (T + 3) / 4;
  if (gy < 1) gy = 1;
  *rows = gy;
  hipLaunchKernelGGL(colsum_kernel, dim3(gx, gy), dim3(256), 0, st, in, part, T, C);
  return 0;
}
// out: slices x groups x C floats (slices = 1: the sums themselves)
int d3dp_train_groupsum(const float* in, float* out, int T, int C, int mode, int F, int J, int slices, hipStream_t st) {
  const int groups = mode == 0 ? J : (mode == 1 ? F : T / (F * J));
  if (slices < 1 || groups < 1) return -1;
  hipLaunchKernelGGL(groupsum_kernel, dim3((C + 255) / 256, groups, slices), dim3(256), 0, st, in, out, T, C, mode, F, J);
  return 0;
}
int d3dp_train_transpose_pad(const float* in, float* out, int R, int C, int Rpad, hipStream_t st) {
  hipLaunchKernelGGL(transpose_pad_kernel, dim3((Rpad + 31) / 32, (C + 31) / 32), dim3(256), 0, st, in, out, R, C, Rpad);
  return 0;
}
static_assert(sizeof(AttnStats) == D3DP_TRAIN_ATTN_STAT_BYTES, "train_plan.h: d3dp_train_attn_stats_bytes");

// ------------------------------------------------------------------------------------------------
// Attention backward on the fp32 matrix cores (v_mfma_f32_16x16x4_f32: exact fp32 fma chains), head dim 64, sequences of
// up to 256 tokens (the temporal axis: 243 frames).  The two kernels above spend 13 ms of the configs[4] step on the VALU;
// the same five products per (sequence, head) cost the fp32 matrix pipe 37.8 MFLOP = 148 k cycles of one CU.
//   pass Q : K, V in LDS; one 16-query tile per wave.  S^T = K Q^T and dP^T = V dO^T as MFMA tiles [key][query] (the layout
//            of attention_fast.hip's forward kernel), two-pass softmax in registers, dS^T = P^T (dP^T - D) / 8 per key tile and
//            dQ^T += K^T dS^T straight from the registers that hold it.  Writes (row max, denominator, D) per query.
//   pass KV: Q, dO and the statistics in LDS; one 16-key tile per wave with its K / V fragments in registers.  S = Q K^T and
//            dP = dO V^T as tiles [query][key], P from the stored statistics, dV^T += dO^T P and dK^T += Q^T dS.
// A workgroup = eight waves = eight consecutive tiles of one problem (grid = problems x ceil(tiles / 8)): with one
// 139-KiB workgroup per CU, 544 problems of 16 tiles each would quantise to three rounds of 256; 1,088 half problems
// to 4.25 half rounds (four tiles per workgroup: the same rounds, but the K / V staging -- as long as a tile's MFMAs --
// twice as often and by half as many threads: measured 300 + 325 us per temporal block instead of the 130 + 160 of
// the MFMAs).  LDS rows: 68 floats (row-pattern fragments = four ds_read_b128 per 16 contraction steps;
// column-pattern fragments conflict-free ds_read_b32).
// ------------------------------------------------------------------------------------------------
constexpr int LDB = 68;
using f32x4m = float __attribute__((ext_vector_type(4)));

// NW = tiles (waves) per workgroup: 8 for the long sequences (two per SIMD cover each other's LDS waits), 2 for <= 32 tokens
__device__ __forceinline__ void bwd_stage_rows(float* dst, const float* src0, size_t row_stride, int n, int NK, int tid, int nthr) {
  for (int idx = tid; idx < NK * 16; idx += nthr) {
    const int row = idx >> 4, c4 = (idx & 15) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < n) v = *reinterpret_cast<const float4*>(src0 + (size_t)row * row_stride + c4);
    *reinterpret_cast<float4*>(dst + row * LDB + c4) = v;
  }
}
// 16 contraction steps of two independent tiles: acc_a += A_a[fi][16 fg + kk] b_a[kk], the same for b
__device__ __forceinline__ void bwd_chain2(const float* ra, const float* rb, const float (&ba)[16], const float (&bb)[16],
                                           f32x4m& a, f32x4m& b) {
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) {
    a = __builtin_amdgcn_mfma_f32_16x16x4f32(ra[kk], ba[kk], a, 0, 0, 0);
    b = __builtin_amdgcn_mfma_f32_16x16x4f32(rb[kk], bb[kk], b, 0, 0, 0);
  }
}

template <int NKT, int NW>
__global__ __launch_bounds__(NW * 64) void attn_bwd_q_mfma_kernel(const float* __restrict__ qkv, const float* __restrict__ o,
                                                                 const float* __restrict__ dout, float* __restrict__ dqkv,
                                                                 AttnStats* __restrict__ stats, SeqMap map, int C, int heads,
                                                                 int groups) {
  constexpr int NK = 16 * NKT;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* KS = reinterpret_cast<float*>(smem_raw);
  float* VS = KS + NK * LDB;
  const int n = map.n_tok;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int prob = blockIdx.x / groups, group = blockIdx.x % groups;
  const int seq = prob / heads, head = prob % heads;
  const int base = (seq / map.inner) * map.outer_stride + (seq % map.inner) * map.inner_stride;
  const int ts = map.tok_stride;
  const size_t ld = (size_t)3 * C;
  const float* qbase = qkv + (size_t)base * ld + (size_t)head * 64;
  bwd_stage_rows(KS, qbase + C, (size_t)ts * ld, n, NK, tid, NW * 64);
  bwd_stage_rows(VS, qbase + 2 * C, (size_t)ts * ld, n, NK, tid, NW * 64);
  __syncthreads();
  const int qt = group * NW + wave;
  if (qt * 16 >= n) return;
  const int fi = lane & 15, fg = lane >> 4;
  const int q = qt * 16 + fi;
  const size_t tok = (size_t)(base + min(q, n - 1) * ts);
  float qv[16], gv[16];
  float D = 0.f;
  {
    const float* qs = qkv + tok * ld + head * 64 + fg * 16;
    const float* gs = dout + tok * C + head * 64 + fg * 16;
    const float* os = o + tok * C + head * 64 + fg * 16;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float4 a = *reinterpret_cast<const float4*>(qs + c * 4);
      const float4 g = *reinterpret_cast<const float4*>(gs + c * 4);
      const float4 ov = *reinterpret_cast<const float4*>(os + c * 4);
      qv[c * 4] = a.x; qv[c * 4 + 1] = a.y; qv[c * 4 + 2] = a.z; qv[c * 4 + 3] = a.w;
      gv[c * 4] = g.x; gv[c * 4 + 1] = g.y; gv[c * 4 + 2] = g.z; gv[c * 4 + 3] = g.w;
      D = fmaf(g.x, ov.x, D); D = fmaf(g.y, ov.y, D); D = fmaf(g.z, ov.z, D); D = fmaf(g.w, ov.w, D);
    }
  }
  D += __shfl_xor(D, 16, 64);
  D += __shfl_xor(D, 32, 64);
  // S^T[key = 16 t + 4 fg + r][query fi], two key tiles (two accumulator chains) at a time
  f32x4m s[NKT];
#pragma unroll
  for (int t = 0; t < NKT; t += 2) {
    f32x4m a = {0.f, 0.f, 0.f, 0.f}, b = a;
    bwd_chain2(KS + (t * 16 + fi) * LDB + fg * 16, KS + ((t + 1) * 16 + fi) * LDB + fg * 16, qv, qv, a, b);
    s[t] = a; s[t + 1] = b;
    __builtin_amdgcn_sched_barrier(0);
  }
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    if (16 * (t + 1) > n) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (16 * t + 4 * fg + r >= n) s[t][r] = -INFINITY;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[t][r]);
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float cexp = 0.125f * 1.44269504088896340736f;
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s[t][r] = exp2f((s[t][r] - mx) * cexp);
      sum += s[t][r];
    }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  const float pscale = 0.125f / sum;                   // P / 8: dS = P (dP - D) / sqrt(64)
  f32x4m dq[4];
#pragma unroll
  for (int dn = 0; dn < 4; ++dn) dq[dn] = (f32x4m){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < NKT; t += 2) {
    f32x4m da = {0.f, 0.f, 0.f, 0.f}, db = da;          // dP^T of key tiles t, t + 1
    bwd_chain2(VS + (t * 16 + fi) * LDB + fg * 16, VS + ((t + 1) * 16 + fi) * LDB + fg * 16, gv, gv, da, db);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const f32x4m dp = u ? db : da;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float ds = s[t + u][r] * pscale * (dp[r] - D);
        const float* kr = KS + ((t + u) * 16 + 4 * fg + r) * LDB + fi;      // K[key][dn * 16 + fi]
#pragma unroll
        for (int dn = 0; dn < 4; ++dn) dq[dn] = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[dn * 16], ds, dq[dn], 0, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  if (q < n) {
    float* dst = dqkv + tok * ld + head * 64 + fg * 4;                      // dQ^T[d = dn * 16 + 4 fg + i][query fi]
#pragma unroll
    for (int dn = 0; dn < 4; ++dn)
      *reinterpret_cast<float4*>(dst + dn * 16) = make_float4(dq[dn][0], dq[dn][1], dq[dn][2], dq[dn][3]);
    if (fg == 0) stats[(size_t)prob * n + q] = AttnStats{mx, sum, D};       // (raw row max, denominator: private to pass KV)
  }
}

template <int NKT, int NW>
__global__ __launch_bounds__(NW * 64) void attn_bwd_kv_mfma_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                                  float* __restrict__ dqkv, const AttnStats* __restrict__ stats,
                                                                  SeqMap map, int C, int heads, int groups) {
  constexpr int NK = 16 * NKT;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* QS = reinterpret_cast<float*>(smem_raw);
  float* GS = QS + NK * LDB;
  float* ST = GS + NK * LDB;                           // [NK][4]: row max, 1 / (8 denominator), D, -
  const int n = map.n_tok;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int prob = blockIdx.x / groups, group = blockIdx.x % groups;
  const int seq = prob / heads, head = prob % heads;
  const int base = (seq / map.inner) * map.outer_stride + (seq % map.inner) * map.inner_stride;
  const int ts = map.tok_stride;
  const size_t ld = (size_t)3 * C;
  bwd_stage_rows(QS, qkv + (size_t)base * ld + (size_t)head * 64, (size_t)ts * ld, n, NK, tid, NW * 64);
  bwd_stage_rows(GS, dout + (size_t)base * C + (size_t)head * 64, (size_t)ts * C, n, NK, tid, NW * 64);
  for (int i = tid; i < NK; i += NW * 64) {
    // rows >= n: Q and dO rows are zero, so whatever finite P and dS they get contributes nothing
    float4 v = make_float4(0.f, 0.125f, 0.f, 0.f);
    if (i < n) {
      const AttnStats a = stats[(size_t)prob * n + i];
      v = make_float4(a.m, 0.125f / a.l, a.D, 0.f);
    }
    *reinterpret_cast<float4*>(ST + i * 4) = v;
  }
  __syncthreads();
  const int kt = group * NW + wave;
  if (kt * 16 >= n) return;
  const int fi = lane & 15, fg = lane >> 4;
  const int key = kt * 16 + fi;
  const size_t tok = (size_t)(base + min(key, n - 1) * ts);
  float kv[16], vv[16];
  {
    const float* ks = qkv + tok * ld + C + head * 64 + fg * 16;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float4 a = *reinterpret_cast<const float4*>(ks + c * 4);
      float4 b = *reinterpret_cast<const float4*>(ks + C + c * 4);
      if (key >= n) { a = make_float4(0.f, 0.f, 0.f, 0.f); b = a; }
      kv[c * 4] = a.x; kv[c * 4 + 1] = a.y; kv[c * 4 + 2] = a.z; kv[c * 4 + 3] = a.w;
      vv[c * 4] = b.x; vv[c * 4 + 1] = b.y; vv[c * 4 + 2] = b.z; vv[c * 4 + 3] = b.w;
    }
  }
  const float cexp = 0.125f * 1.44269504088896340736f;
  f32x4m dk[4], dv[4];
#pragma unroll
  for (int dn = 0; dn < 4; ++dn) { dk[dn] = (f32x4m){0.f, 0.f, 0.f, 0.f}; dv[dn] = dk[dn]; }
#pragma unroll 2
  for (int t = 0; t < NKT; ++t) {
    // S[query = 16 t + 4 fg + i][key fi] and dP of the same tile: two accumulator chains
    f32x4m sa = {0.f, 0.f, 0.f, 0.f}, da = sa;
    bwd_chain2(QS + (t * 16 + fi) * LDB + fg * 16, GS + (t * 16 + fi) * LDB + fg * 16, kv, vv, sa, da);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = t * 16 + 4 * fg + i;
      const float4 a = *reinterpret_cast<const float4*>(ST + row * 4);
      const float p8 = exp2f((sa[i] - a.x) * cexp) * a.y;               // P / 8
      const float ds = p8 * (da[i] - a.z);
      const float p = p8 * 8.0f;
      const float* gr = GS + row * LDB + fi;                             // dO[query][dn * 16 + fi]
      const float* qr = QS + row * LDB + fi;
#pragma unroll
      for (int dn = 0; dn < 4; ++dn) {
        dv[dn] = __builtin_amdgcn_mfma_f32_16x16x4f32(gr[dn * 16], p, dv[dn], 0, 0, 0);
        dk[dn] = __builtin_amdgcn_mfma_f32_16x16x4f32(qr[dn * 16], ds, dk[dn], 0, 0, 0);
      }
    }
  }
  if (key < n) {
    float* dst = dqkv + tok * ld + C + head * 64 + fg * 4;                // d{K,V}^T[d = dn * 16 + 4 fg + i][key fi]
#pragma unroll
    for (int dn = 0; dn < 4; ++dn) {
      *reinterpret_cast<float4*>(dst + dn * 16) = make_float4(dk[dn][0], dk[dn][1], dk[dn][2], dk[dn][3]);
      *reinterpret_cast<float4*>(dst + C + dn * 16) = make_float4(dv[dn][0], dv[dn][1], dv[dn][2], dv[dn][3]);
    }
  }
}

template <int NKT>
static int launch_attn_bwd_mfma(const float* qkv, const float* o, const float* dout, float* dqkv, void* stats, int n_seq,
                                SeqMap map, int C, int heads, hipStream_t st) {
  constexpr int NK = 16 * NKT, NW = NKT <= 2 ? 2 : 8;
  const size_t lds_q = (size_t)2 * NK * LDB * 4, lds_kv = lds_q + (size_t)NK * 16;
  static PerDeviceOnce once;
  if (once.get([&](int) {
        return d3dp_lds_opt_in(reinterpret_cast<const void*>(attn_bwd_q_mfma_kernel<NKT, NW>), 160 * 1024) < 0 ? -3
               : d3dp_lds_opt_in(reinterpret_cast<const void*>(attn_bwd_kv_mfma_kernel<NKT, NW>), 160 * 1024);
      }) < 0) return -3;
  const int tiles = (map.n_tok + 15) / 16, groups = (tiles + NW - 1) / NW;
  hipLaunchKernelGGL((attn_bwd_q_mfma_kernel<NKT, NW>), dim3(n_seq * heads * groups), dim3(NW * 64), lds_q, st, qkv, o, dout, dqkv,
                     (AttnStats*)stats, map, C, heads, groups);
  hipLaunchKernelGGL((attn_bwd_kv_mfma_kernel<NKT, NW>), dim3(n_seq * heads * groups), dim3(NW * 64), lds_kv, st, qkv, dout, dqkv,
                     (const AttnStats*)stats, map, C, heads, groups);
  return 0;
}

// the chunked VALU pair: any n >= 1
template <int HD, bool GEN>
static int launch_attn_bwd_chunked(const float* qkv, const float* o, const float* dout, float* dqkv, void* stats, int n_seq,
                                   SeqMap map, int C, int heads, hipStream_t st) {
  const int n = map.n_tok;
  if (n < 1) return -1;
  const int rows = n < attn_bwd_chunk_rows<HD>() ? n : attn_bwd_chunk_rows<HD>();            // rows of a chunk's LDS images
  const size_t lds_q = (size_t)2 * rows * (HD + 4) * 4;
  const size_t lds_kv = lds_q + (size_t)rows * sizeof(AttnStats);
  static_assert((size_t)2 * attn_bwd_chunk_rows<HD>() * (HD + 4) * 4 + attn_bwd_chunk_rows<HD>() * sizeof(AttnStats) <= 160 * 1024,
                "a chunk's two images and its statistics fit the CU's LDS");
  static PerDeviceOnce once;
  if (once.get([&](int) {
        return d3dp_lds_opt_in(reinterpret_cast<const void*>(attn_bwd_q_chunk_kernel<HD, GEN>), 160 * 1024) < 0 ? -3
               : d3dp_lds_opt_in(reinterpret_cast<const void*>(attn_bwd_kv_chunk_kernel<HD, GEN>), 160 * 1024);
      }) < 0) return -3;
  // two threads per row in both passes; a row block of ATTN_BWD_BLOCK_ROWS rows per workgroup
  const int threads = 2 * n <= 64 ? 64 : (2 * n <= 256 ? 256 : 512);
  const dim3 grid(n_seq * heads, (n + ATTN_BWD_BLOCK_ROWS - 1) / ATTN_BWD_BLOCK_ROWS);
  hipLaunchKernelGGL((attn_bwd_q_chunk_kernel<HD, GEN>), grid, dim3(threads), lds_q, st, qkv, o, dout, dqkv, (AttnStats*)stats, map, C,
                     heads, C / heads);
  hipLaunchKernelGGL((attn_bwd_kv_chunk_kernel<HD, GEN>), grid, dim3(threads), lds_kv, st, qkv, dout, dqkv, (const AttnStats*)stats, map,
                     C, heads, C / heads);
  return 0;
}

template <int HD, bool GEN = false>
static int launch_attn_bwd(const float* qkv, const float* o, const float* dout, float* dqkv, void* stats, int n_seq,
                           SeqMap map, int C, int heads, hipStream_t st, bool chunked) {
  const int n = map.n_tok;
  if constexpr (HD == 64 && !GEN) {
    // head dim 64 on the fp32 matrix cores; D3DP_TRAIN_ATTN_BWD=valu keeps the kernels below (cross-check)
    const char* e = getenv("D3DP_TRAIN_ATTN_BWD");     // (read per call: the tests switch it between two steps)
    const bool valu = e && e[0] == 'v';
    if (!valu && n <= 256 && C % 4 == 0) {
      if (n <= 32) return launch_attn_bwd_mfma<2>(qkv, o, dout, dqkv, stats, n_seq, map, C, heads, st);
      if (n <= 64) return launch_attn_bwd_mfma<4>(qkv, o, dout, dqkv, stats, n_seq, map, C, heads, st);
      if (n <= 128) return launch_attn_bwd_mfma<8>(qkv, o, dout, dqkv, stats, n_seq, map, C, heads, st);
      return launch_attn_bwd_mfma<16>(qkv, o, dout, dqkv, stats, n_seq, map, C, heads, st);
    }
  }
  if (chunked) return launch_attn_bwd_chunked<HD, GEN>(qkv, o, dout, dqkv, stats, n_seq, map, C, heads, st);
  const size_t lds_q = (size_t)2 * n * (HD + 4) * 4;
  const size_t lds_kv = lds_q + (size_t)n * sizeof(AttnStats);
  if (lds_kv > 160 * 1024 || n > 256) return -2;
  static PerDeviceOnce once;
  if (once.get([&](int) {
        return d3dp_lds_opt_in(reinterpret_cast<const void*>(attn_bwd_q_kernel<HD, GEN>), 160 * 1024) < 0 ? -3
               : d3dp_lds_opt_in(reinterpret_cast<const void*>(attn_bwd_kv_kernel<HD, GEN>), 160 * 1024);
      }) < 0) return -3;
  const int tkv = 2 * n <= 64 ? 64 : (2 * n <= 256 ? 256 : 512), tq = tkv;       // two threads per row in both passes
  hipLaunchKernelGGL((attn_bwd_q_kernel<HD, GEN>), dim3(n_seq * heads), dim3(tq), lds_q, st, qkv, o, dout, dqkv,
                     (AttnStats*)stats, map, C, heads, C / heads);
  hipLaunchKernelGGL((attn_bwd_kv_kernel<HD, GEN>), dim3(n_seq * heads), dim3(tkv), lds_kv, st, qkv, dout, dqkv,
                     (const AttnStats*)stats, map, C, heads, C / heads);
  return 0;
}

int d3dp_train_attn_bwd(const float* qkv, const float* o, const float* dout, float* dqkv, void* stats, int n_seq,
                        SeqMap map, int C, int heads, hipStream_t st, bool chunked) {
  switch (C / heads) {
    case 64: return launch_attn_bwd<64>(qkv, o, dout, dqkv, stats, n_seq, map, C, heads, st, chunked);
    case 32: return launch_attn_bwd<32>(qkv, o, dout, dqkv, stats, n_seq, map, C, heads, st, chunked);
    case 16: return launch_attn_bwd<16>(qkv, o, dout, dqkv, stats, n_seq, map, C, heads, st, chunked);
    case 8: return launch_attn_bwd<8>(qkv, o, dout, dqkv, stats, n_seq, map, C, heads, st, chunked);
    default: break;
  }
  // any other head dim (a multiple of 4 up to 128): the run-time form on the next capacity
  const int hd = C / heads;
  if (hd < 4 || hd % 4 || hd > 128 || hd * heads != C) return -2;
  if (hd <= 16) return launch_attn_bwd<16, true>(qkv, o, dout, dqkv, stats, n_seq, map, C, heads, st, chunked);
  if (hd <= 32) return launch_attn_bwd<32, true>(qkv, o, dout, dqkv, stats, n_seq, map, C, heads, st, chunked);
  if (hd <= 64) return launch_attn_bwd<64, true>(qkv, o, dout, dqkv, stats, n_seq, map, C, heads, st, chunked);
  return launch_attn_bwd<128, true>(qkv, o, dout, dqkv, stats, n_seq, map, C, heads, st, chunked);
}
// part: D3DP_EMBED_BWD_ROWS partial tables of 5 C floats
int d3dp_train_embed_bwd(const float* dx, const float* x2d, const float* x3d, float* part, int T, int C, hipStream_t st) {
  hipLaunchKernelGGL(embed_bwd_kernel, dim3((C + 255) / 256, D3DP_EMBED_BWD_ROWS), dim3(256), 0, st, dx, x2d, x3d, part, T, C);
  return 0;
}
int d3dp_train_head_linear(const float* z, const float* w, const float* b, float* out, int T, int C, hipStream_t st) {
  if (!d3dp_width_instantiated(C)) return d3dp_train_g_head_linear(z, w, b, out, T, C, st);
  TRAIN_DISPATCH_C(C, hipLaunchKernelGGL((head_linear_kernel<CC>), dim3((T + 3) / 4), dim3(256), 0, st, z, w, b, out, T))
  return 0;
}
// part: *rows (<= 512) partial rows of 3 C + 4 floats ([dW | db, -])
int d3dp_train_head_bwd(const float* g, const float* z, const float* w, float* dz, float* part, int* rows, int T, int C,
                        hipStream_t st) {
  if (!rows) return -1;
  *rows = T < 512 ? T : 512;
  hipLaunchKernelGGL(head_bwd_kernel, dim3((C + 255) / 256, *rows), dim3(256), 0, st, g, z, w, dz, part, T, C);
  return 0;
}
// hidden: scratch of B x 2 C floats
int d3dp_train_time_mlp(const int64_t* t, const float* freq, const float* w1, const float* b1, const float* w2, const float* b2,
                        float* hidden, float* temb, int B, int C, hipStream_t st) {
  if (B < 1 || C % 2 != 0) return -1;
  hipLaunchKernelGGL(time_mlp1_kernel, dim3((B * 2 * C + 3) / 4), dim3(256), 0, st, t, freq, w1, b1, hidden, B, C);
  hipLaunchKernelGGL(time_mlp2_kernel, dim3((B * C + 3) / 4), dim3(256), 0, st, hidden, w2, b2, temb, B, C);
  return 0;
}
int d3dp_train_time_mlp_bwd(const int64_t* t, const float* freq, const float* w1, const float* b1, const float* w2,
                            const float* dtemb, float* dw1, float* db1, float* dw2, float* db2, int B, int C,
                            hipStream_t st) {
  if (!d3dp_width_instantiated(C)) return d3dp_train_g_time_mlp_bwd(t, freq, w1, b1, w2, dtemb, dw1, db1, dw2, db2, B, C, st);
  TRAIN_DISPATCH_C(C, hipLaunchKernelGGL((time_mlp_bwd_kernel<CC>), dim3((2 * C + 3) / 4), dim3(256), 0, st, t, freq, w1, b1,
                                         w2, dtemb, dw1, db1, dw2, db2, B))
  return 0;
}
