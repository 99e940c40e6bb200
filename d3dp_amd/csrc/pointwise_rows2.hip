// Run-time width with 2-byte rows: the row kernels of a FAST / FAST16 context at a width outside the instantiated set
// (D3DP_FAST_IMPL=mfma at channels 192 / 320 / 384 / 448, ctx.h hdp), E = bf16 or IEEE fp16.  The activation xn leaves as rows of C
// elements of E, and the branch outputs yadd / yadd0 that a row adds to the fp32 residual stream arrive as such rows (the proj / fc2
// Linears of the FAST modes write 2-byte rows).  Row ownership is that of the *_h_kernel family of pointwise.hip: C % 32 == 0, C <= 512,
// a lane owns the 8 CONSECUTIVE columns 8 lane .. 8 lane + 7 (lanes >= C / 8 idle) -- two 16-byte fp32 loads, ONE 16-byte load per 2-byte
// input row and ONE 16-byte store of its eight outputs.  The arithmetic per row is that of the instantiated kernels: two-pass fp32
// statistics, 1 / C as a multiplied reciprocal, fma with gamma / beta, one plain cast (round to nearest even) to E.
// RowE repeats RowH's loads, store and norm (and kRowTokens) instead of sharing them through a header ON PURPOSE: pointwise.hip's
// translation unit stays as it was, so that its 92 kernels keep their device code beside these (profiles/fast_widths.md).
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int kRowTokens = 8;   // tokens per wave of the embedding and head kernels (pointwise.hip: the weights stay in registers)

struct RowE {
  static constexpr int NV = 8;
  template <typename T>
  static __device__ __forceinline__ void load(const T* p, int C, int lane, float* v) {
    if (8 * lane < C) load8(p + 8 * lane, v);
    else {
#pragma unroll
      for (int i = 0; i < NV; ++i) v[i] = 0.f;
    }
  }
  // (the fp32 residual stream: read or written once here and not touched again until kernels later)
  static __device__ __forceinline__ void load_nt(const float* p, int C, int lane, float* v) {
    if (8 * lane < C) {
      const f32x4 a = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p + 8 * lane));
      const f32x4 b = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p + 8 * lane + 4));
      v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
    } else {
#pragma unroll
      for (int i = 0; i < NV; ++i) v[i] = 0.f;
    }
  }
  template <typename T>
  static __device__ __forceinline__ void store(T* p, int C, int lane, const float* v) {
    if (8 * lane < C) store8(p + 8 * lane, v);
  }
  // the activation row: fp16 keeps the fp32 value a value of its own, so that the cast stays the round-to-nearest-even convert of the
  // fp32 result that every other store of this type is (Row<C>::store in pointwise.hip: left alone, the compiler merges the cast with
  // norm()'s fma into v_fma_mixlo_f16, which rounds the exact fma once)
  template <typename E>
  static __device__ __forceinline__ void store_act(E* p, int C, int lane, const float* v) {
    float t[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      t[i] = v[i];
      if constexpr (std::is_same<E, f16>::value) asm volatile("" : "+v"(t[i]));
    }
    if (8 * lane < C) store8(p + 8 * lane, t);
  }
  static __device__ __forceinline__ void norm(const float* v, const float* wv, const float* bv, float eps, int C, int lane, float* y) {
    const float rc = 1.0f / (float)C;
    const bool live = 8 * lane < C;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) s += v[i];                        // (idle lanes hold 0)
    const float mean = wave_sum(s) * rc;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) { const float d = live ? v[i] - mean : 0.f; q = fmaf(d, d, q); }
    const float rstd = 1.0f / sqrtf(wave_sum(q) * rc + eps);
#pragma unroll
    for (int i = 0; i < NV; ++i) y[i] = live ? fmaf((v[i] - mean) * rstd, wv[i], bv[i]) : 0.f;
  }
};

template <typename E>
__global__ __launch_bounds__(256) void ln_e_kernel(float* __restrict__ x, const E* __restrict__ yadd, const float* __restrict__ w,
                                                   const float* __restrict__ b, float eps, E* __restrict__ xn, int T, int C,
                                                   int write_x) {
  using R = RowE;
  const int lane = threadIdx.x & 63;
  const int tok = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tok >= T) return;
  float v[R::NV], y[R::NV], wv[R::NV], bv[R::NV];
  R::load_nt(x + (size_t)tok * C, C, lane, v);
  if (yadd != nullptr) {
    R::load(yadd + (size_t)tok * C, C, lane, y);
#pragma unroll
    for (int i = 0; i < R::NV; ++i) v[i] += y[i];
    if (write_x) R::store(x + (size_t)tok * C, C, lane, v);
  }
  R::load(w, C, lane, wv);
  R::load(b, C, lane, bv);
  R::norm(v, wv, bv, eps, C, lane, y);
  R::store_act(xn + (size_t)tok * C, C, lane, y);
}

template <typename E>
__global__ __launch_bounds__(256) void ln2_e_kernel(float* __restrict__ x, const E* __restrict__ yadd0, const E* __restrict__ yadd,
                                                    const float* __restrict__ wa, const float* __restrict__ ba,
                                                    const float* __restrict__ pos, const float* __restrict__ wb,
                                                    const float* __restrict__ bb, float eps, E* __restrict__ xn, int T, int C,
                                                    int F, int J, int SP) {
  using R = RowE;
  const int lane = threadIdx.x & 63;
  const int tok = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tok >= T) return;
  float v[R::NV], y[R::NV], z[R::NV], wv[R::NV], bv[R::NV];
  R::load_nt(x + (size_t)tok * C, C, lane, v);
  if (yadd0 != nullptr) {
    R::load(yadd0 + (size_t)tok * C, C, lane, y);
#pragma unroll
    for (int i = 0; i < R::NV; ++i) v[i] += y[i];
  }
  if (yadd != nullptr) {
    R::load(yadd + (size_t)tok * C, C, lane, y);
#pragma unroll
    for (int i = 0; i < R::NV; ++i) v[i] += y[i];
  }
  R::load(wa, C, lane, wv);
  R::load(ba, C, lane, bv);
  R::norm(v, wv, bv, eps, C, lane, y);
  if (pos != nullptr) {
    const int f = min((tok % SP) / J, F - 1);
    float pv[R::NV];
    R::load(pos + (size_t)f * C, C, lane, pv);
#pragma unroll
    for (int i = 0; i < R::NV; ++i) y[i] += pv[i];
  }
  R::store(x + (size_t)tok * C, C, lane, y);
  R::load(wb, C, lane, wv);
  R::load(bb, C, lane, bv);
  R::norm(y, wv, bv, eps, C, lane, z);
  R::store_act(xn + (size_t)tok * C, C, lane, z);
}

// kRowTokens tokens per wave, the weights of a lane's 8 columns held in registers across them
template <typename E>
__global__ __launch_bounds__(256) void embed_ln_e_kernel(const float* __restrict__ x2d, const float* __restrict__ x3d,
                                                         const float* __restrict__ temb, const float* __restrict__ ew,
                                                         const float* __restrict__ eb, const float* __restrict__ spos,
                                                         const float* __restrict__ lnw, const float* __restrict__ lnb, float eps,
                                                         float* __restrict__ x, E* __restrict__ xn, int seq0, int n_seq, int H,
                                                         int F, int J, int SP, int C) {
  using R = RowE;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int FJ = F * J, T = n_seq * SP;
  const bool live = 8 * lane < C;
  float w5[R::NV][5], ebv[R::NV], lw[R::NV], lb[R::NV];
#pragma unroll
  for (int i = 0; i < R::NV; ++i) {
#pragma unroll
    for (int k = 0; k < 5; ++k) w5[i][k] = live ? ew[(8 * lane + i) * 5 + k] : 0.f;
  }
  R::load(eb, C, lane, ebv);
  R::load(lnw, C, lane, lw);
  R::load(lnb, C, lane, lb);
  for (int it = 0; it < kRowTokens; ++it) {
    const int tl = (blockIdx.x * kRowTokens + it) * 4 + wave;    // chunk-local row: sequence tl / SP, token tl % SP
    if (tl >= T) break;
    const bool pad = (tl % SP) >= FJ;                            // (pad rows: finite filler, see embed_ln_kernel)
    const int seq = seq0 + tl / SP, fj = pad ? 0 : tl % SP, nj = fj % J;
    const int b = seq / H;
    const float* p2 = x2d + ((size_t)b * FJ + fj) * 2;
    const float* p3 = x3d + ((size_t)seq * FJ + fj) * 3;
    float in5[5] = {p2[0], p2[1], p3[0], p3[1], p3[2]};          // channel order [u, v, x, y, z]
    if (pad) { in5[0] = in5[1] = in5[2] = in5[3] = in5[4] = 0.f; }
    float v[R::NV], y[R::NV], sp[R::NV], tb[R::NV];
    R::load(spos + (size_t)nj * C, C, lane, sp);
    R::load(temb + (size_t)b * C, C, lane, tb);
#pragma unroll
    for (int i = 0; i < R::NV; ++i) {
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < 5; ++k) a = fmaf(in5[k], w5[i][k], a);
      a += ebv[i];
      a += sp[i];
      a += tb[i];
      v[i] = a;                                                  // (idle lanes: every term is 0)
    }
    R::store(x + (size_t)tl * C, C, lane, v);
    R::norm(v, lw, lb, eps, C, lane, y);
    R::store_act(xn + (size_t)tl * C, C, lane, y);
  }
}

// out[T,3] = Linear(LN_head(LN_a((x + yadd0) + yadd))): kRowTokens tokens per wave, the two norms' weights and the head's three rows
// of a lane's 8 columns held in registers across them (as head_kernel)
template <typename E>
__global__ __launch_bounds__(256) void head_e_kernel(const float* __restrict__ x, const E* __restrict__ yadd0,
                                                     const E* __restrict__ yadd, const float* __restrict__ wa,
                                                     const float* __restrict__ ba, float eps_a, const float* __restrict__ wh,
                                                     const float* __restrict__ bh, float eps_h, const float* __restrict__ w,
                                                     const float* __restrict__ b, float* __restrict__ out, int T, int C, int FJ,
                                                     int SP) {
  using R = RowE;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float wav[R::NV], bav[R::NV], whv[R::NV], bhv[R::NV], wv[3][R::NV];
  R::load(wa, C, lane, wav);
  R::load(ba, C, lane, bav);
  R::load(wh, C, lane, whv);
  R::load(bh, C, lane, bhv);
#pragma unroll
  for (int o = 0; o < 3; ++o) R::load(w + o * C, C, lane, wv[o]);       // (idle lanes: 0, so they add nothing below)
  const float b0 = b[0], b1 = b[1], b2 = b[2];
  for (int it = 0; it < kRowTokens; ++it) {
    const int tok = (blockIdx.x * kRowTokens + it) * 4 + wave;
    if (tok >= T) break;
    float v[R::NV], y[R::NV], z[R::NV];
    R::load_nt(x + (size_t)tok * C, C, lane, v);
    if (yadd0 != nullptr) {
      R::load(yadd0 + (size_t)tok * C, C, lane, y);
#pragma unroll
      for (int i = 0; i < R::NV; ++i) v[i] += y[i];
    }
    if (yadd != nullptr) {
      R::load(yadd + (size_t)tok * C, C, lane, y);
#pragma unroll
      for (int i = 0; i < R::NV; ++i) v[i] += y[i];
    }
    R::norm(v, wav, bav, eps_a, C, lane, y);
    R::norm(y, whv, bhv, eps_h, C, lane, z);
    float acc[3];
#pragma unroll
    for (int o = 0; o < 3; ++o) {
      float a = 0.f;
#pragma unroll
      for (int i = 0; i < R::NV; ++i) a = fmaf(z[i], wv[o][i], a);
      acc[o] = wave_sum(a) + (o == 0 ? b0 : o == 1 ? b1 : b2);
    }
    // rows are (sequence, token) at pitch SP >= FJ; the output is compact
    const int fj = tok % SP;
    if (lane < 3 && fj < FJ) out[((size_t)(tok / SP) * FJ + fj) * 3 + lane] = lane == 0 ? acc[0] : (lane == 1 ? acc[1] : acc[2]);
  }
}

inline bool shape_ok(int act, int C) { return (act == 1 || act == 4) && C >= 32 && C <= 512 && C % 32 == 0; }

}  // namespace

int d3dp_rows2_embed_ln(int act, const float* x2d, const float* x3d, const float* temb, const float* ew, const float* eb,
                        const float* spos, const float* lnw, const float* lnb, float eps, float* x, void* xn, int seq0, int n_seq,
                        int H, int F, int J, int C, hipStream_t st, int SP) {
  if (!shape_ok(act, C)) return -2;
  const int T = n_seq * SP;
  const dim3 g((T + 4 * kRowTokens - 1) / (4 * kRowTokens)), blk(256);
  if (act == 4) hipLaunchKernelGGL(embed_ln_e_kernel<f16>, g, blk, 0, st, x2d, x3d, temb, ew, eb, spos, lnw, lnb, eps, x, (f16*)xn, seq0, n_seq, H, F, J, SP, C);
  else hipLaunchKernelGGL(embed_ln_e_kernel<bf16>, g, blk, 0, st, x2d, x3d, temb, ew, eb, spos, lnw, lnb, eps, x, (bf16*)xn, seq0, n_seq, H, F, J, SP, C);
  return 0;
}

int d3dp_rows2_ln(int act, float* x, const void* yadd, int write_x, const float* w, const float* b, float eps, void* xn, int T, int C,
                  hipStream_t st) {
  if (!shape_ok(act, C)) return -2;
  const dim3 g((T + 3) / 4), blk(256);
  if (act == 4) hipLaunchKernelGGL(ln_e_kernel<f16>, g, blk, 0, st, x, (const f16*)yadd, w, b, eps, (f16*)xn, T, C, write_x);
  else hipLaunchKernelGGL(ln_e_kernel<bf16>, g, blk, 0, st, x, (const bf16*)yadd, w, b, eps, (bf16*)xn, T, C, write_x);
  return 0;
}

int d3dp_rows2_ln2(int act, float* x, const void* yadd0, const void* yadd, const float* wa, const float* ba, const float* pos,
                   const float* wb, const float* bb, float eps, void* xn, int T, int C, int F, int J, hipStream_t st, int SP) {
  if (!shape_ok(act, C)) return -2;
  const dim3 g((T + 3) / 4), blk(256);
  if (act == 4) hipLaunchKernelGGL(ln2_e_kernel<f16>, g, blk, 0, st, x, (const f16*)yadd0, (const f16*)yadd, wa, ba, pos, wb, bb, eps, (f16*)xn, T, C, F, J, SP);
  else hipLaunchKernelGGL(ln2_e_kernel<bf16>, g, blk, 0, st, x, (const bf16*)yadd0, (const bf16*)yadd, wa, ba, pos, wb, bb, eps, (bf16*)xn, T, C, F, J, SP);
  return 0;
}

int d3dp_rows2_head(int act, const float* x, const void* yadd0, const void* yadd, const float* wa, const float* ba, float eps_a,
                    const float* wh, const float* bh, float eps_h, const float* w, const float* b, float* out, int T, int C,
                    hipStream_t st, int FJ, int SP) {
  if (!shape_ok(act, C)) return -2;
  const dim3 g((T + 4 * kRowTokens - 1) / (4 * kRowTokens)), blk(256);
  if (act == 4) hipLaunchKernelGGL(head_e_kernel<f16>, g, blk, 0, st, x, (const f16*)yadd0, (const f16*)yadd, wa, ba, eps_a, wh, bh, eps_h, w, b, out, T, C, FJ, SP);
  else hipLaunchKernelGGL(head_e_kernel<bf16>, g, blk, 0, st, x, (const bf16*)yadd0, (const bf16*)yadd, wa, ba, eps_a, wh, bh, eps_h, w, b, out, T, C, FJ, SP);
  return 0;
}
