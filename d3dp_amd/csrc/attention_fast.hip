// Attention of the FAST and FAST16 modes on the 2-byte matrix cores (v_mfma_f32_16x16x32_bf16 / _f16 through Op2<E>, common.h):
// rows of E = bf16 or IEEE fp16 in and out, fp32 accumulation and softmax, probabilities rounded to E before P.V.  K and V rows
// live in LDS in the swizzled row-major images of attn_frag.h; S^T = K Q^T is computed transposed, so the probabilities land
// directly in the B fragment layout of O^T = V^T P^T.
//
//   attn_spatial_bf16_kernel   : <= 32 tokens per sequence, one wave per (sequence, head) with a private 8 KiB image.
//   attn_temporal2_bf16_kernel : <= 256 tokens, one workgroup per problem, the whole score row-block of a 16-query tile in
//                                registers: a plain two-pass softmax, no online rescaling.
//   attn_long2_bf16_kernel     : 257 .. 1024 tokens, the keys in chunks of 16 D3DP_FAST_LONG_NKT under an online softmax.
//
// attention() in capi.hip sends a FAST / FAST16 context here when its head dim is 64: the spatial axis up to 32 joints to the
// spatial kernel, with more joints to the temporal launcher (it takes any SeqMap), the temporal axis to the temporal launcher --
// except where D3DP_LONG_ATTN=rows keeps the fp32 row kernel (attention_f32.hip) beyond 32 joints / 256 frames.
// d3dp_op_attention reaches the same launchers with impl 1 on 2-byte rows.  The launchers refuse (-2) any other head dim, the
// spatial one more than 32 tokens, the temporal one more than 1024.
#include "common.h"
#include "kernels.h"
#include "ta_common.h"
#include "attn_frag.h"

namespace {

template <typename E, int NKT, int C0>
__device__ __forceinline__ void pv_chunks(const FragBases& fb, const typename Op2<E>::x8 (&pf)[NKT / 2], f32x4 (&o)[4]) {
  if constexpr (C0 < NKT / 2) {
#pragma unroll
    for (int dn = 0; dn < 4; ++dn)
      o[dn] = Op2<E>::mfma(load_vt_frag<C0, E>(fb.v[dn]), pf[C0], o[dn]);
    if (C0 & 1) __builtin_amdgcn_sched_barrier(0);
    pv_chunks<E, NKT, C0 + 1>(fb, pf, o);
  }
}

// One 16-query tile against NKT 16-key tiles resident in LDS.  q0/q1: the tile's Q fragments (d 0..31 / 32..63).
// Returns O^T accumulators (4 channel tiles) and the softmax denominator of query (lane & 15).
// ONLINE (the chunked-key kernel below): the resident keys are one chunk of a longer row.  `mrun` is the running row maximum
// in base-2 logit units (-inf before the first chunk); the probabilities are formed against the larger of it and this chunk's
// maximum, and `o` / `denom` -- the sums over the earlier chunks -- are rescaled to that maximum and added to.
template <typename E, int NKT, bool ONLINE>
__device__ __forceinline__ void attn_tile(const FragBases& fb, typename Op2<E>::x8 q0, typename Op2<E>::x8 q1, int n, int lane,
                                          f32x4 (&o)[4], float& denom, float& mrun) {
  using e8 = typename Op2<E>::x8;
  const int fg = lane >> 4;
  const float cexp = 0.125f * 1.44269504088896340736f;   // hd^-0.5 * log2(e), hd = 64
  f32x4 s[NKT];
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    const e8 k0 = *reinterpret_cast<const e8*>(fb.k0 + t * 2048);
    const e8 k1 = *reinterpret_cast<const e8*>(fb.k1 + t * 2048);
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    a = Op2<E>::mfma(k0, q0, a);
    a = Op2<E>::mfma(k1, q1, a);
    s[t] = a;
    if ((t & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // bound the ds_read hoisting window (VGPR pressure)
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
  float mc = mx * cexp, alpha = 0.f;
  if constexpr (ONLINE) {
    mc = fmaxf(mc, mrun);                                  // (finite: the chunk holds at least one key)
    alpha = __builtin_amdgcn_exp2f(mrun - mc);             // (first chunk: 0)
    mrun = mc;
  }
  float sum = 0.f;
  e8 pf[NKT / 2];
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = __builtin_amdgcn_exp2f(fmaf(s[t][r], cexp, -mc));
      sum += p;
      pf[t >> 1][(t & 1) * 4 + r] = (E)p;
    }
  }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  if constexpr (ONLINE) {
    denom = fmaf(denom, alpha, sum);
#pragma unroll
    for (int dn = 0; dn < 4; ++dn) o[dn] *= alpha;
  } else {
    denom = sum;
#pragma unroll
    for (int dn = 0; dn < 4; ++dn) o[dn] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  pv_chunks<E, NKT, 0>(fb, pf, o);
}
template <typename E, int NKT>
__device__ __forceinline__ void attn_tile(const FragBases& fb, typename Op2<E>::x8 q0, typename Op2<E>::x8 q1, int n, int lane,
                                          f32x4 (&o)[4], float& denom) {
  float m = 0.f;
  attn_tile<E, NKT, false>(fb, q0, q1, n, lane, o, denom, m);
}

// rows [0, n) of K and V (128 B per row for this head) -> swizzled LDS images; rows [n, NK) of V zeroed.
template <int NK, int NTHREADS, typename E>
__device__ __forceinline__ void stage_kv(const E* __restrict__ kbase, size_t row_stride, int n, char* KS, char* VS,
                                         int tid, int C) {
  for (int idx = tid; idx < NK * 8; idx += NTHREADS) {
    const int row = idx >> 3, slot = idx & 7;
    float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
    if (row < n) {
      const E* src = kbase + (size_t)row * row_stride + slot * 8;
      kv = *reinterpret_cast<const float4*>(src);
      vv = *reinterpret_cast<const float4*>(src + C);
    }
    *reinterpret_cast<float4*>(KS + row * 128 + ((slot ^ ((row >> 1) & 7)) << 4)) = kv;
    *reinterpret_cast<float4*>(VS + row * 128 + ((slot ^ (((row >> 1) & 3) << 1)) << 4)) = vv;
  }
}

template <typename E, int NKT>   // temporal axis: one workgroup per (sequence, head), 8 waves share the K/V images
__global__ __launch_bounds__(512, 4) void attn_temporal2_bf16_kernel(const E* __restrict__ qkv, E* __restrict__ out,
                                                                     SeqMap map, int C, int heads) {
  using e4 = typename Op2<E>::x4;
  using e8 = typename Op2<E>::x8;
  constexpr int NK = 16 * NKT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* KS = smem;
  char* VS = smem + NK * 128;
  const int n = map.n_tok;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int seq = blockIdx.x / heads, head = blockIdx.x % heads;
  const int base = ta_seq_base(map, seq);
  const int ts = map.tok_stride;
  const size_t ld = (size_t)3 * C;
  const E* qbase = qkv + (size_t)base * ld + (size_t)head * 64;
  // This wave's Q fragments for ALL of its query tiles are requested before K/V staging, so their HBM latency
  // overlaps the staging loads instead of being paid once per tile in the compute loop.
  const int fi = lane & 15, fg = lane >> 4;
  const int n_qt = (n + 15) >> 4;
  constexpr int QPW = (NKT + 7) / 8;                 // query tiles per wave
  e8 qf[QPW][2];
#pragma unroll
  for (int i = 0; i < QPW; ++i) {
    const int q = min((wave + 8 * i) * 16 + fi, n - 1);
    const E* qsrc = qbase + (size_t)q * ts * ld + fg * 8;
    qf[i][0] = *reinterpret_cast<const e8*>(qsrc);
    qf[i][1] = *reinterpret_cast<const e8*>(qsrc + 32);
  }
  stage_kv<NK, 512>(qbase + C, (size_t)ts * ld, n, KS, VS, tid, C);
  const FragBases fb = make_frag_bases(KS, VS, lane);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < QPW; ++i) {
    const int qt = wave + 8 * i;
    if (qt >= n_qt) break;
    const int q = qt * 16 + fi;
    f32x4 o[4];
    float denom;
    attn_tile<E, NKT>(fb, qf[i][0], qf[i][1], n, lane, o, denom);
    if (q < n) {
      const float inv = 1.0f / denom;
      E* dst = out + (size_t)(base + q * ts) * C + head * 64 + fg * 4;
#pragma unroll
      for (int dn = 0; dn < 4; ++dn) {
        e4 r = {(E)(o[dn][0] * inv), (E)(o[dn][1] * inv), (E)(o[dn][2] * inv), (E)(o[dn][3] * inv)};
        *reinterpret_cast<e4*>(dst + dn * 16) = r;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Sequences LONGER than 256 tokens (up to the library's 1024) on the same operands: the flash form, as
// attn_temporal_x2_long_kernel (attention_x2.hip) is for EXACT.  A work unit = one (sequence, head) problem x one group of eight 16-query tiles,
// one tile per wave; a persistent grid walks the units.  The keys pass through LDS in chunks of 16 NKT (K and V images in
// stage_kv's layouts, two buffers); attn_tile's ONLINE form runs its two-pass softmax over each chunk against the larger of
// the chunk's and the running row maximum -- probabilities rounded to E before P.V, the mode's definition -- and rescales the
// running denominator and O^T, which stay in registers, in base-2 units whenever a chunk raises the maximum (-inf before the
// first chunk: the empty sums are scaled by 0, never by inf - inf).  Chunk c + 1's global loads are issued
// into registers before chunk c's MFMAs and written to the other buffer after them, so one barrier per chunk serves both
// "buffer c is complete" and "buffer c - 1 is free".  Keys >= n: zero K / V rows, scores masked by attn_tile; queries >= n are
// computed on row n - 1 and not stored.  Correct for any n >= 1; launched for n > 256.
// -DD3DP_FAST_LONG_NKT=16 (measurement build): chunks of 256 keys, 128 KiB of LDS, one workgroup per CU
// (profiles/fast_long_attn.md has the comparison).
#ifndef D3DP_FAST_LONG_NKT
#define D3DP_FAST_LONG_NKT 8
#endif
template <typename E, int NKT>
__global__ __launch_bounds__(512, NKT == 8 ? 4 : 2) void attn_long2_bf16_kernel(const E* __restrict__ qkv, E* __restrict__ out,
                                                                                  SeqMap map, int C, int heads, int groups,
                                                                                  int n_work) {
  using e4 = typename Op2<E>::x4;
  using e8 = typename Op2<E>::x8;
  constexpr int NK = 16 * NKT, IMG = NK * 128, BUF = 2 * IMG, NLD = NK * 8 / 512;
  extern __shared__ __attribute__((aligned(16))) char smem[];       // two buffers of [K image | V image]
  const int n = map.n_tok;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fi = lane & 15, fg = lane >> 4;
  const int ts = map.tok_stride;
  const size_t ld = (size_t)3 * C, rs = (size_t)ts * ld;
  const int n_chunks = (n + NK - 1) / NK;
  float4 kr[NLD], vr[NLD];
  // Staging: thread `tid` moves 16-byte slot (tid & 7) of rows (tid >> 3) + 64 u of a chunk, so everything that depends on the
  // thread is one 32-bit element offset into the rows (63 tok_stride 3 C + 56 < 2^31 for every shape the library takes) and one
  // byte offset into each image (the swizzles have period 16 rows); the rest is wave-uniform.
  const int r0 = tid >> 3, slot = tid & 7;
  const unsigned goff = (unsigned)r0 * (unsigned)rs + slot * 8;
  const int koff = r0 * 128 + ((slot ^ ((r0 >> 1) & 7)) << 4);
  const int voff = IMG + r0 * 128 + ((slot ^ (((r0 >> 1) & 3) << 1)) << 4);
  // rows k0 .. k0 + NK - 1 of K and V -> registers (rows >= n: zeros) ...
  auto fetch = [&](const E* kbase, int k0) {
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      kr[u] = make_float4(0.f, 0.f, 0.f, 0.f); vr[u] = kr[u];
      if (k0 + 64 * u + r0 < n) {
        const E* src = kbase + (size_t)(k0 + 64 * u) * rs + goff;
        kr[u] = *reinterpret_cast<const float4*>(src);
        vr[u] = *reinterpret_cast<const float4*>(src + C);
      }
    }
  };
  // ... and from there into one buffer's swizzled images (stage_kv's layouts)
  auto commit = [&](char* buf) {
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      *reinterpret_cast<float4*>(buf + koff + u * 8192) = kr[u];
      *reinterpret_cast<float4*>(buf + voff + u * 8192) = vr[u];
    }
  };
  for (int unit = blockIdx.x; unit < n_work; unit += gridDim.x) {
    const int prob = unit / groups, group = unit - prob * groups;
    const int seq = prob / heads, head = prob - seq * heads;
    const int base = ta_seq_base(map, seq);
    const E* qbase = qkv + (size_t)base * ld + (size_t)head * 64;
    const int qt = group * 8 + wave;
    const bool active = qt * 16 < n;                     // (wave-uniform)
    const int q = qt * 16 + fi;
    e8 q0 = {}, q1 = {};
    if (active) {
      const E* qsrc = qbase + (size_t)min(q, n - 1) * rs + fg * 8;
      q0 = *reinterpret_cast<const e8*>(qsrc);
      q1 = *reinterpret_cast<const e8*>(qsrc + 32);
    }
    fetch(qbase + C, 0);
    __syncthreads();                                     // every wave is done with the previous unit's images
    commit(smem);
    float mrun = -INFINITY, lrun = 0.f;                  // running row maximum (base-2 logit units) and denominator
    f32x4 o[4];
#pragma unroll
    for (int dn = 0; dn < 4; ++dn) o[dn] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < n_chunks; ++c) {
      __syncthreads();                                   // buffer c & 1 is complete; every wave has left buffer (c + 1) & 1
      if (c + 1 < n_chunks) fetch(qbase + C, (c + 1) * NK);          // in flight under this chunk's MFMAs
      if (active) {
        const int off = (c & 1) * BUF, rem = n - c * NK; // (rem >= 1: the chunk holds a key, its maximum is finite)
        const FragBases fb = make_frag_bases(smem + off, smem + off + IMG, lane);
        attn_tile<E, NKT, true>(fb, q0, q1, rem, lane, o, lrun, mrun);
      }
      if (c + 1 < n_chunks) commit(smem + ((c + 1) & 1) * BUF);
    }
    if (active && q < n) {
      const float inv = 1.0f / lrun;
      E* dst = out + (size_t)(base + q * ts) * C + head * 64 + fg * 4;
#pragma unroll
      for (int dn = 0; dn < 4; ++dn) {
        e4 r = {(E)(o[dn][0] * inv), (E)(o[dn][1] * inv), (E)(o[dn][2] * inv), (E)(o[dn][3] * inv)};
        *reinterpret_cast<e4*>(dst + dn * 16) = r;
      }
    }
  }
}

// spatial axis (<= 32 tokens per sequence): one WAVE per (sequence, head) with a private 8 KiB K/V image;
// a 256-thread workgroup covers 4 heads of one sequence.
template <typename E>
__global__ __launch_bounds__(256) void attn_spatial_bf16_kernel(const E* __restrict__ qkv, E* __restrict__ out,
                                                                int n_prob, SeqMap map, int C, int heads) {
  using e4 = typename Op2<E>::x4;
  using e8 = typename Op2<E>::x8;
  __shared__ __attribute__((aligned(16))) char smem[4 * 8192];
  const int n = map.n_tok;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pid = blockIdx.x * 4 + wave;
  if (pid >= n_prob) return;
  const int seq = pid / heads, head = pid % heads;
  const int base = ta_seq_base(map, seq);
  const int ts = map.tok_stride;
  const size_t ld = (size_t)3 * C;
  const E* qbase = qkv + (size_t)base * ld + (size_t)head * 64;
  char* KS = smem + wave * 8192;
  char* VS = KS + 4096;
  // the query fragments of both 16-row tiles are requested BEFORE the K/V staging so that their HBM latency overlaps
  // it (the kernel is latency/HBM-bound: one small problem per wave)
  const int fi = lane & 15, fg = lane >> 4;
  const int n_qt = (n + 15) >> 4;
  e8 qf[2][2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const E* qsrc = qbase + (size_t)min(qt * 16 + fi, n - 1) * ts * ld + fg * 8;
    qf[qt][0] = *reinterpret_cast<const e8*>(qsrc);
    qf[qt][1] = *reinterpret_cast<const e8*>(qsrc + 32);
  }
  stage_kv<32, 64>(qbase + C, (size_t)ts * ld, n, KS, VS, lane, C);
  const FragBases fb = make_frag_bases(KS, VS, lane);
  // (wave-private LDS image: the LDS pipe executes one wave's accesses in order, no barrier needed)
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    if (qt >= n_qt) break;
    const int q = qt * 16 + fi;
    const e8 q0 = qf[qt][0], q1 = qf[qt][1];
    f32x4 o[4];
    float denom;
    attn_tile<E, 2>(fb, q0, q1, n, lane, o, denom);
    if (q < n) {
      const float inv = 1.0f / denom;
      E* dst = out + (size_t)(base + q * ts) * C + head * 64 + fg * 4;
#pragma unroll
      for (int dn = 0; dn < 4; ++dn) {
        e4 r = {(E)(o[dn][0] * inv), (E)(o[dn][1] * inv), (E)(o[dn][2] * inv), (E)(o[dn][3] * inv)};
        *reinterpret_cast<e4*>(dst + dn * 16) = r;
      }
    }
  }
}

template <typename E, int NKT>
int launch_temporal2(const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads, hipStream_t st) {
  constexpr int NK = 16 * NKT;
  const size_t lds = (size_t)NK * 256;
  auto kern = attn_temporal2_bf16_kernel<E, NKT>;
  static PerDeviceOnce once;                          // (one per template instantiation = per kernel)
  if (once.get([&](int) { return d3dp_lds_opt_in(reinterpret_cast<const void*>(kern), 160 * 1024); }) < 0) return -3;
  hipLaunchKernelGGL(kern, dim3(n_seq * heads), dim3(512), lds, st, (const E*)qkv, (E*)out, map, C, heads);
  return 0;
}

// n_tok > 256: the chunked-key kernel; a persistent grid of two workgroups per CU (64 KiB of LDS each)
template <typename E>
int launch_long2(const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads, hipStream_t st) {
  constexpr int NKT = D3DP_FAST_LONG_NKT;
  static_assert(NKT == 8 || NKT == 16, "chunks of 128 or 256 keys");
  const int groups = ((map.n_tok + 15) / 16 + 7) / 8, n_work = n_seq * heads * groups;
  auto kern = attn_long2_bf16_kernel<E, NKT>;
  static PerDeviceOnce once;                          // (one per template instantiation = per kernel)
  const int cus = once.get([&](int dev) {
    const int r = d3dp_lds_opt_in(reinterpret_cast<const void*>(kern), 160 * 1024);
    return r < 0 ? r : d3dp_cu_count(dev);
  });
  if (cus < 0) return -3;
  const int wgs = (NKT == 8 ? 2 : 1) * cus;
  hipLaunchKernelGGL(kern, dim3(n_work < wgs ? n_work : wgs), dim3(512), (size_t)NKT * 16 * 512, st, (const E*)qkv, (E*)out, map,
                     C, heads, groups, n_work);
  return 0;
}

}  // namespace

template <typename E>
static int attn_temporal2(const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads, hipStream_t st) {
  const int n = map.n_tok;
  if (n > 256) return launch_long2<E>(qkv, out, n_seq, map, C, heads, st);
  if (n <= 32) return launch_temporal2<E, 2>(qkv, out, n_seq, map, C, heads, st);
  if (n <= 64) return launch_temporal2<E, 4>(qkv, out, n_seq, map, C, heads, st);
  if (n <= 128) return launch_temporal2<E, 8>(qkv, out, n_seq, map, C, heads, st);
  return launch_temporal2<E, 16>(qkv, out, n_seq, map, C, heads, st);
}
// (f16: 0 = bf16 rows in and out, 1 = IEEE fp16.  Any SeqMap: <= 256 tokens the whole-sequence kernel, up to 1024 the
//  chunked-key one)
int d3dp_launch_attn_temporal_bf16(const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads,
                                   hipStream_t st, int f16) {
  if (C / heads != 64 || map.n_tok > 1024 || map.n_tok < 1) return -2;
  return f16 ? attn_temporal2<_Float16>(qkv, out, n_seq, map, C, heads, st) : attn_temporal2<__bf16>(qkv, out, n_seq, map, C, heads, st);
}

// spatial axis on MFMA (bf16 or, f16 == 1, IEEE fp16 rows; head dim 64, <= 32 tokens per sequence)
int d3dp_launch_attn_spatial_bf16(const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads, hipStream_t st, int f16) {
  if (C / heads != 64 || map.n_tok > 32 || map.n_tok < 1) return -2;
  const int n_prob = n_seq * heads;
  if (f16)
    hipLaunchKernelGGL(attn_spatial_bf16_kernel<_Float16>, dim3((n_prob + 3) / 4), dim3(256), 0, st, (const _Float16*)qkv,
                       (_Float16*)out, n_prob, map, C, heads);
  else
    hipLaunchKernelGGL(attn_spatial_bf16_kernel<__bf16>, dim3((n_prob + 3) / 4), dim3(256), 0, st, (const __bf16*)qkv, (__bf16*)out,
                       n_prob, map, C, heads);
  return 0;
}
