// Attention of the FAST and FAST16 modes on the 2-byte matrix cores (v_mfma_f32_16x16x32_bf16 / _f16 through Op2<E>, common.h):
// rows of E = bf16 or IEEE fp16 in and out, fp32 accumulation and softmax, probabilities rounded to E before P.V.  K and V rows
// live in LDS in the swizzled row-major images of attn_frag.h; S^T = K Q^T is computed transposed, so the probabilities land
// directly in the B fragment layout of O^T = V^T P^T.
//
// The head dim HD is a template parameter of every kernel: 64, 32 or 16 (`-cs` 512 / 256 / 128 with the model's 8 heads).  It is
// the k-depth of S^T -- two 16x16x32 MFMAs per key tile at 64, one at 32, and at 16 ONE 16-DEEP MFMA of the same family
// (v_mfma_f32_16x16x16_bf16 / _f16: lane (i, g) holds d = 4 g .. 4 g + 3 of row i, 8 bytes, so no lane ever addresses a column
// outside its head and nothing is padded) -- and the number HD / 16 of output-channel tiles of O^T, whose k-depth is keys.  A K or
// V row is 2 HD bytes in global memory and in LDS; attn_frag.h derives the three pairs of images.  Scale: HD^-0.5 log2(e).
//
//   attn_spatial_bf16_kernel   : <= 32 tokens per sequence, one wave per (sequence, head) with a private 8 KiB image.
//   attn_temporal2_bf16_kernel : <= 256 tokens, one workgroup per problem, the whole score row-block of a 16-query tile in
//                                registers: a plain two-pass softmax, no online rescaling.
//   attn_long2_bf16_kernel     : 257 .. 1024 tokens, the keys in chunks of 16 D3DP_FAST_LONG_NKT under an online softmax.
//
// attention() in capi_denoise.hip sends a FAST / FAST16 context here when its head dim is 64, 32 or 16: the spatial axis up to 32 joints
// to the spatial kernel, with more joints to the temporal launcher (it takes any SeqMap), the temporal axis to the temporal
// launcher -- except where D3DP_LONG_ATTN=rows keeps the fp32 row kernel (attention_f32.hip): beyond 32 joints / 256 frames at
// head dim 64, for every shape at head dims 32 and 16.  Head dim 8 (a quarter of the narrowest k-depth) stays on the row kernel.
// d3dp_op_attention reaches the same launchers with impl 1 on 2-byte rows.  The launchers refuse (-2) any other head dim, the
// spatial one more than 32 tokens, the temporal one more than 1024.
#include "common.h"
#include "kernels.h"
#include "ta_common.h"
#include "attn_frag.h"

// The padded forms (attention_fast_pad.hip includes this file with D3DP_FAST_PAD_TU defined): the same three kernels on rows whose heads
// were padded with zero columns from a TRUE head dim HDT = 24 to HD = 32, or from 40 / 48 / 56 to 64 -- channels 192 / 320 / 384 / 448
// with the model's 8 heads in a FAST / FAST16 context under D3DP_FAST_IMPL=mfma (ctx.h hdp).  The zero columns add nothing to S^T and
// come back as exact zeros of O^T; HDT enters the exponent alone.  There every kernel and launcher template below carries HDT as one
// more parameter; here the AF_ macros expand to nothing, the instantiations are the ones this file always had and keep their device
// code (profiles/fast_widths.md).
//
// The scaled forms (attention_fast_scaled.hip includes this file with D3DP_FAST_SCALED_TU defined): the same three kernels for a FAST16
// context under D3DP_FAST16_RANGE=scale, whose q, k and v rows hold 2^-s times their value (ctx.h BlockDev::r_qkv).  S^T then comes out
// at 2^-2s, so the exponent scale is a RUN-TIME argument `escale` = HD^-0.5 2^(2s) that every kernel and launcher template below carries
// (with a tag parameter that keeps their symbols apart); nothing else moves -- scores and sums are fp32, the probabilities are at
// most 1, and O^T leaves at v's scale.  Here and in the padded forms the AF_ESC_ macros expand to nothing.
#ifdef D3DP_FAST_PAD_TU
#define AF_HDT_PARAM , int HDT
#define AF_HDT_ARG , HDT
#define AF_SCALE (HDT == 24 ? 0.20412414523193151f : HDT == 40 ? 0.15811388300841897f : HDT == 48 ? 0.14433756729740643f : 0.1336306209562122f)
#define AF_ESC_PARAM
#define AF_ESC_ARG
#elif defined(D3DP_FAST_SCALED_TU)
#define AF_HDT_PARAM , int SCALED
#define AF_HDT_ARG , SCALED
#define AF_SCALE escale
#define AF_ESC_PARAM , float escale
#define AF_ESC_ARG , escale
#else
#define AF_HDT_PARAM
#define AF_HDT_ARG
#define AF_SCALE (HD == 64 ? 0.125f : HD == 32 ? 0.17677669529663689f : 0.25f)
#define AF_ESC_PARAM
#define AF_ESC_ARG
#endif

namespace {

// What follows from the head dim: bytes per K / V row, log2 of its 16-byte slots, and the fragments of S^T = K Q^T -- NQ per
// 16-row tile and operand, `frag` = QW elements per lane each (HD = 16: the x4 operand of the 16-deep MFMA).
template <typename E, int HD> struct Head {
  static_assert(HD == 64 || HD == 32, "head dim");
  typedef typename Op2<E>::x8 frag;
  static constexpr int ROWB = 2 * HD, LS = HD == 64 ? 3 : 2, NQ = HD / 32, QW = 8;
};
template <typename E> struct Head<E, 16> {
  typedef typename Op2<E>::x4 frag;
  static constexpr int ROWB = 32, LS = 1, NQ = 1, QW = 4;
};
// the Q fragments of query row `qrow` (this head's HD columns): d = QW fg .. + QW - 1 [and 32 further, HD = 64]
template <typename E, int HD>
__device__ __forceinline__ void load_q(const E* qrow, int fg, typename Head<E, HD>::frag (&q)[Head<E, HD>::NQ]) {
  typedef typename Head<E, HD>::frag frag;
  const E* qsrc = qrow + fg * Head<E, HD>::QW;
  q[0] = *reinterpret_cast<const frag*>(qsrc);
  if constexpr (HD == 64) q[1] = *reinterpret_cast<const frag*>(qsrc + 32);
}

template <typename E, int HD, int NKT, int C0>
__device__ __forceinline__ void pv_chunks(const FragBasesT<HD>& fb, const typename Op2<E>::x8 (&pf)[NKT / 2], f32x4 (&o)[HD / 16]) {
  if constexpr (C0 < NKT / 2) {
#pragma unroll
    for (int dn = 0; dn < HD / 16; ++dn)
      o[dn] = Op2<E>::mfma(load_vt_frag<C0, E, HD>(fb.v[dn]), pf[C0], o[dn]);
    if (C0 & 1) __builtin_amdgcn_sched_barrier(0);
    pv_chunks<E, HD, NKT, C0 + 1>(fb, pf, o);
  }
}

// One 16-query tile against NKT 16-key tiles resident in LDS.  q: the tile's Q fragments (HD = 64: d 0..31 / 32..63).
// Returns O^T accumulators (HD / 16 channel tiles) and the softmax denominator of query (lane & 15).
// ONLINE (the chunked-key kernel below): the resident keys are one chunk of a longer row.  `mrun` is the running row maximum
// in base-2 logit units (-inf before the first chunk); the probabilities are formed against the larger of it and this chunk's
// maximum, and `o` / `denom` -- the sums over the earlier chunks -- are rescaled to that maximum and added to.
template <typename E, int HD, int NKT, bool ONLINE AF_HDT_PARAM>
__device__ __forceinline__ void attn_tile(const FragBasesT<HD>& fb, const typename Head<E, HD>::frag (&q)[Head<E, HD>::NQ], int n,
                                          int lane, f32x4 (&o)[HD / 16], float& denom, float& mrun AF_ESC_PARAM) {
  using e8 = typename Op2<E>::x8;
  using kfrag = typename Head<E, HD>::frag;
  constexpr int TILE = 16 * Head<E, HD>::ROWB;           // bytes of one 16-key tile of the K image
  const int fg = lane >> 4;
#ifdef D3DP_FAST_PAD_TU
  static_assert((HD == 32 && HDT == 24) || (HD == 64 && (HDT == 40 || HDT == 48 || HDT == 56)), "AF_SCALE holds these true head dims");
#endif
  const float cexp = AF_SCALE * 1.44269504088896340736f;   // HD^-0.5 * log2(e) (padded heads: of the true head dim)
  f32x4 s[NKT];
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    const kfrag k0 = *reinterpret_cast<const kfrag*>(fb.k0 + t * TILE);
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    if constexpr (HD == 64) {
      const kfrag k1 = *reinterpret_cast<const kfrag*>(fb.k1 + t * TILE);
      a = Op2<E>::mfma(k0, q[0], a);
      a = Op2<E>::mfma(k1, q[1], a);
    } else {
      a = Op2<E>::mfma(k0, q[0], a);                     // (HD = 16: the 16-deep instruction)
    }
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
    for (int dn = 0; dn < HD / 16; ++dn) o[dn] *= alpha;
  } else {
    denom = sum;
#pragma unroll
    for (int dn = 0; dn < HD / 16; ++dn) o[dn] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  pv_chunks<E, HD, NKT, 0>(fb, pf, o);
}
template <typename E, int HD, int NKT AF_HDT_PARAM>
__device__ __forceinline__ void attn_tile(const FragBasesT<HD>& fb, const typename Head<E, HD>::frag (&q)[Head<E, HD>::NQ], int n,
                                          int lane, f32x4 (&o)[HD / 16], float& denom AF_ESC_PARAM) {
  float m = 0.f;
  attn_tile<E, HD, NKT, false AF_HDT_ARG>(fb, q, n, lane, o, denom, m AF_ESC_ARG);
}

// rows [0, n) of K and V (2 HD bytes per row for this head = HD / 8 16-byte slots) -> swizzled LDS images; rows [n, NK) zeroed.
template <int NK, int NTHREADS, int HD, typename E>
__device__ __forceinline__ void stage_kv(const E* __restrict__ kbase, size_t row_stride, int n, char* KS, char* VS,
                                         int tid, int C) {
  constexpr int LS = Head<E, HD>::LS, ROWB = Head<E, HD>::ROWB;
  for (int idx = tid; idx < (NK << LS); idx += NTHREADS) {
    const int row = idx >> LS, slot = idx & ((1 << LS) - 1);
    float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
    if (row < n) {
      const E* src = kbase + (size_t)row * row_stride + slot * 8;
      kv = *reinterpret_cast<const float4*>(src);
      vv = *reinterpret_cast<const float4*>(src + C);
    }
    *reinterpret_cast<float4*>(KS + row * ROWB + ((slot ^ k_slot_swizzle<HD>(row)) << 4)) = kv;
    *reinterpret_cast<float4*>(VS + row * ROWB + ((slot ^ v_slot_swizzle<HD>(row)) << 4)) = vv;
  }
}

template <typename E, int HD, int NKT AF_HDT_PARAM>   // temporal axis: one workgroup per (sequence, head), 8 waves share the K/V images
__global__ __launch_bounds__(512, 4) void attn_temporal2_bf16_kernel(const E* __restrict__ qkv, E* __restrict__ out,
                                                                     SeqMap map, int C, int heads AF_ESC_PARAM) {
  using e4 = typename Op2<E>::x4;
  using H = Head<E, HD>;
  constexpr int NK = 16 * NKT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* KS = smem;
  char* VS = smem + NK * H::ROWB;
  const int n = map.n_tok;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int seq = blockIdx.x / heads, head = blockIdx.x % heads;
  const int base = ta_seq_base(map, seq);
  const int ts = map.tok_stride;
  const size_t ld = (size_t)3 * C;
  const E* qbase = qkv + (size_t)base * ld + (size_t)head * HD;
  // This wave's Q fragments for ALL of its query tiles are requested before K/V staging, so their HBM latency
  // overlaps the staging loads instead of being paid once per tile in the compute loop.
  const int fi = lane & 15, fg = lane >> 4;
  const int n_qt = (n + 15) >> 4;
  constexpr int QPW = (NKT + 7) / 8;                 // query tiles per wave
  typename H::frag qf[QPW][H::NQ];
#pragma unroll
  for (int i = 0; i < QPW; ++i) {
    const int q = min((wave + 8 * i) * 16 + fi, n - 1);
    load_q<E, HD>(qbase + (size_t)q * ts * ld, fg, qf[i]);
  }
  stage_kv<NK, 512, HD>(qbase + C, (size_t)ts * ld, n, KS, VS, tid, C);
  const FragBasesT<HD> fb = make_frag_bases<HD>(KS, VS, lane);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < QPW; ++i) {
    const int qt = wave + 8 * i;
    if (qt >= n_qt) break;
    const int q = qt * 16 + fi;
    f32x4 o[HD / 16];
    float denom;
    attn_tile<E, HD, NKT AF_HDT_ARG>(fb, qf[i], n, lane, o, denom AF_ESC_ARG);
    if (q < n) {
      const float inv = 1.0f / denom;
      E* dst = out + (size_t)(base + q * ts) * C + head * HD + fg * 4;
#pragma unroll
      for (int dn = 0; dn < HD / 16; ++dn) {
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
template <typename E, int HD, int NKT AF_HDT_PARAM>
__global__ __launch_bounds__(512, NKT == 8 ? 4 : 2) void attn_long2_bf16_kernel(const E* __restrict__ qkv, E* __restrict__ out,
                                                                                  SeqMap map, int C, int heads, int groups,
                                                                                  int n_work AF_ESC_PARAM) {
  using e4 = typename Op2<E>::x4;
  using H = Head<E, HD>;
  // a pass of the 512 threads moves RPP rows; NLD passes per chunk (HD = 16, chunks of 128 keys: half a pass, PART)
  constexpr int NK = 16 * NKT, IMG = NK * H::ROWB, BUF = 2 * IMG, LS = H::LS, RPP = 512 >> LS, NLD = (NK + RPP - 1) / RPP;
  constexpr bool PART = NK % RPP != 0;
  extern __shared__ __attribute__((aligned(16))) char smem[];       // two buffers of [K image | V image]
  const int n = map.n_tok;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fi = lane & 15, fg = lane >> 4;
  const int ts = map.tok_stride;
  const size_t ld = (size_t)3 * C, rs = (size_t)ts * ld;
  const int n_chunks = (n + NK - 1) / NK;
  float4 kr[NLD], vr[NLD];
  // Staging: thread `tid` moves 16-byte slot (tid & 7) of rows (tid >> 3) + 64 u of a chunk (HD = 64; a row has HD / 8 slots, so
  // slot tid & 3 of rows (tid >> 2) + 128 u at 32 and slot tid & 1 of row tid >> 1 at 16, where the threads whose row lies past
  // the chunk move nothing), so everything that depends on the thread is one 32-bit element offset into the rows
  // ((RPP - 1) tok_stride 3 C + 56 = 96768 / 97536 / 97920 tok_stride + 56 at C = 512 / 256 / 128: < 2^31 for every shape the
  // library takes) and one byte offset into each image (the swizzles have period 16 rows); the rest is wave-uniform.
  const int r0 = tid >> LS, slot = tid & ((1 << LS) - 1);
  const unsigned goff = (unsigned)r0 * (unsigned)rs + slot * 8;
  const int koff = r0 * H::ROWB + ((slot ^ k_slot_swizzle<HD>(r0)) << 4);
  const int voff = IMG + r0 * H::ROWB + ((slot ^ v_slot_swizzle<HD>(r0)) << 4);
  // rows k0 .. k0 + NK - 1 of K and V -> registers (rows >= n: zeros) ...
  auto fetch = [&](const E* kbase, int k0) {
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      kr[u] = make_float4(0.f, 0.f, 0.f, 0.f); vr[u] = kr[u];
      if (k0 + RPP * u + r0 < n && (!PART || RPP * u + r0 < NK)) {
        const E* src = kbase + (size_t)(k0 + RPP * u) * rs + goff;
        kr[u] = *reinterpret_cast<const float4*>(src);
        vr[u] = *reinterpret_cast<const float4*>(src + C);
      }
    }
  };
  // ... and from there into one buffer's swizzled images (stage_kv's layouts)
  auto commit = [&](char* buf) {
#pragma unroll
    for (int u = 0; u < NLD; ++u) {                      // (a pass is RPP rows of 2 HD bytes = 8192 bytes of an image)
      if (!PART || RPP * u + r0 < NK) {
        *reinterpret_cast<float4*>(buf + koff + u * 8192) = kr[u];
        *reinterpret_cast<float4*>(buf + voff + u * 8192) = vr[u];
      }
    }
  };
  for (int unit = blockIdx.x; unit < n_work; unit += gridDim.x) {
    const int prob = unit / groups, group = unit - prob * groups;
    const int seq = prob / heads, head = prob - seq * heads;
    const int base = ta_seq_base(map, seq);
    const E* qbase = qkv + (size_t)base * ld + (size_t)head * HD;
    const int qt = group * 8 + wave;
    const bool active = qt * 16 < n;                     // (wave-uniform)
    const int q = qt * 16 + fi;
    typename H::frag qf[H::NQ] = {};
    if (active) load_q<E, HD>(qbase + (size_t)min(q, n - 1) * rs, fg, qf);
    fetch(qbase + C, 0);
    __syncthreads();                                     // every wave is done with the previous unit's images
    commit(smem);
    float mrun = -INFINITY, lrun = 0.f;                  // running row maximum (base-2 logit units) and denominator
    f32x4 o[HD / 16];
#pragma unroll
    for (int dn = 0; dn < HD / 16; ++dn) o[dn] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < n_chunks; ++c) {
      __syncthreads();                                   // buffer c & 1 is complete; every wave has left buffer (c + 1) & 1
      if (c + 1 < n_chunks) fetch(qbase + C, (c + 1) * NK);          // in flight under this chunk's MFMAs
      if (active) {
        const int off = (c & 1) * BUF, rem = n - c * NK; // (rem >= 1: the chunk holds a key, its maximum is finite)
        const FragBasesT<HD> fb = make_frag_bases<HD>(smem + off, smem + off + IMG, lane);
        attn_tile<E, HD, NKT, true AF_HDT_ARG>(fb, qf, rem, lane, o, lrun, mrun AF_ESC_ARG);
      }
      if (c + 1 < n_chunks) commit(smem + ((c + 1) & 1) * BUF);
    }
    if (active && q < n) {
      const float inv = 1.0f / lrun;
      E* dst = out + (size_t)(base + q * ts) * C + head * HD + fg * 4;
#pragma unroll
      for (int dn = 0; dn < HD / 16; ++dn) {
        e4 r = {(E)(o[dn][0] * inv), (E)(o[dn][1] * inv), (E)(o[dn][2] * inv), (E)(o[dn][3] * inv)};
        *reinterpret_cast<e4*>(dst + dn * 16) = r;
      }
    }
  }
}

// spatial axis (<= 32 tokens per sequence): one WAVE per (sequence, head) with a private K/V image of 32 rows each (8 KiB at
// head dim 64, 4 / 2 KiB at 32 / 16); a 256-thread workgroup covers 4 heads of one sequence.
template <typename E, int HD AF_HDT_PARAM>
__global__ __launch_bounds__(256) void attn_spatial_bf16_kernel(const E* __restrict__ qkv, E* __restrict__ out,
                                                                int n_prob, SeqMap map, int C, int heads AF_ESC_PARAM) {
  using e4 = typename Op2<E>::x4;
  using H = Head<E, HD>;
  constexpr int IMG = 32 * H::ROWB;
  __shared__ __attribute__((aligned(16))) char smem[4 * 2 * IMG];
  const int n = map.n_tok;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pid = blockIdx.x * 4 + wave;
  if (pid >= n_prob) return;
  const int seq = pid / heads, head = pid % heads;
  const int base = ta_seq_base(map, seq);
  const int ts = map.tok_stride;
  const size_t ld = (size_t)3 * C;
  const E* qbase = qkv + (size_t)base * ld + (size_t)head * HD;
  char* KS = smem + wave * 2 * IMG;
  char* VS = KS + IMG;
  // the query fragments of both 16-row tiles are requested BEFORE the K/V staging so that their HBM latency overlaps
  // it (the kernel is latency/HBM-bound: one small problem per wave)
  const int fi = lane & 15, fg = lane >> 4;
  const int n_qt = (n + 15) >> 4;
  typename H::frag qf[2][H::NQ];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) load_q<E, HD>(qbase + (size_t)min(qt * 16 + fi, n - 1) * ts * ld, fg, qf[qt]);
  stage_kv<32, 64, HD>(qbase + C, (size_t)ts * ld, n, KS, VS, lane, C);
  const FragBasesT<HD> fb = make_frag_bases<HD>(KS, VS, lane);
  // (wave-private LDS image: the LDS pipe executes one wave's accesses in order, no barrier needed)
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    if (qt >= n_qt) break;
    const int q = qt * 16 + fi;
    f32x4 o[HD / 16];
    float denom;
    attn_tile<E, HD, 2 AF_HDT_ARG>(fb, qf[qt], n, lane, o, denom AF_ESC_ARG);
    if (q < n) {
      const float inv = 1.0f / denom;
      E* dst = out + (size_t)(base + q * ts) * C + head * HD + fg * 4;
#pragma unroll
      for (int dn = 0; dn < HD / 16; ++dn) {
        e4 r = {(E)(o[dn][0] * inv), (E)(o[dn][1] * inv), (E)(o[dn][2] * inv), (E)(o[dn][3] * inv)};
        *reinterpret_cast<e4*>(dst + dn * 16) = r;
      }
    }
  }
}

template <typename E, int HD, int NKT AF_HDT_PARAM>
int launch_temporal2(const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads, hipStream_t st AF_ESC_PARAM) {
  constexpr int NK = 16 * NKT;
  const size_t lds = (size_t)NK * 2 * Head<E, HD>::ROWB;           // the K and the V image
  auto kern = attn_temporal2_bf16_kernel<E, HD, NKT AF_HDT_ARG>;
  static PerDeviceOnce once;                          // (one per template instantiation = per kernel)
  if (once.get([&](int) { return d3dp_lds_opt_in(reinterpret_cast<const void*>(kern), 160 * 1024); }) < 0) return -3;
  hipLaunchKernelGGL(kern, dim3(n_seq * heads), dim3(512), lds, st, (const E*)qkv, (E*)out, map, C, heads AF_ESC_ARG);
  return 0;
}

// n_tok > 256: the chunked-key kernel; a persistent grid of two workgroups per CU (64 KiB of LDS each at head dim 64, 32 / 16 KiB
// at 32 / 16: the register budget of its launch bounds, not the LDS, is what holds two)
template <typename E, int HD AF_HDT_PARAM>
int launch_long2(const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads, hipStream_t st AF_ESC_PARAM) {
  constexpr int NKT = D3DP_FAST_LONG_NKT;
  static_assert(NKT == 8 || NKT == 16, "chunks of 128 or 256 keys");
  const int groups = ((map.n_tok + 15) / 16 + 7) / 8, n_work = n_seq * heads * groups;
  auto kern = attn_long2_bf16_kernel<E, HD, NKT AF_HDT_ARG>;
  static PerDeviceOnce once;                          // (one per template instantiation = per kernel)
  const int cus = once.get([&](int dev) {
    const int r = d3dp_lds_opt_in(reinterpret_cast<const void*>(kern), 160 * 1024);
    return r < 0 ? r : d3dp_cu_count(dev);
  });
  if (cus < 0) return -3;
  const int wgs = (NKT == 8 ? 2 : 1) * cus;
  const size_t lds = (size_t)NKT * 16 * 4 * Head<E, HD>::ROWB;     // two buffers of a K and a V image
  hipLaunchKernelGGL(kern, dim3(n_work < wgs ? n_work : wgs), dim3(512), lds, st, (const E*)qkv, (E*)out, map, C, heads, groups,
                     n_work AF_ESC_ARG);
  return 0;
}

template <typename E, int HD AF_HDT_PARAM>
int attn_temporal2(const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads, hipStream_t st AF_ESC_PARAM) {
  const int n = map.n_tok;
  if (n > 256) return launch_long2<E, HD AF_HDT_ARG>(qkv, out, n_seq, map, C, heads, st AF_ESC_ARG);
  if (n <= 32) return launch_temporal2<E, HD, 2 AF_HDT_ARG>(qkv, out, n_seq, map, C, heads, st AF_ESC_ARG);
  if (n <= 64) return launch_temporal2<E, HD, 4 AF_HDT_ARG>(qkv, out, n_seq, map, C, heads, st AF_ESC_ARG);
  if (n <= 128) return launch_temporal2<E, HD, 8 AF_HDT_ARG>(qkv, out, n_seq, map, C, heads, st AF_ESC_ARG);
  return launch_temporal2<E, HD, 16 AF_HDT_ARG>(qkv, out, n_seq, map, C, heads, st AF_ESC_ARG);
}

template <typename E, int HD AF_HDT_PARAM>
int attn_spatial(const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads, hipStream_t st AF_ESC_PARAM) {
  const int n_prob = n_seq * heads;
  hipLaunchKernelGGL((attn_spatial_bf16_kernel<E, HD AF_HDT_ARG>), dim3((n_prob + 3) / 4), dim3(256), 0, st, (const E*)qkv, (E*)out, n_prob, map,
                     C, heads AF_ESC_ARG);
  return 0;
}

}  // namespace

#ifdef D3DP_FAST_PAD_TU
// rows of C = heads x hdp columns per third, hdp = 32 with hd_true = 24 or hdp = 64 with hd_true in {40, 48, 56}; axis 0: the spatial
// kernel (<= 32 tokens), otherwise the whole-sequence / chunked-key kernels (<= 1024 tokens, any SeqMap); -2 for any other shape
#define AF_PAD(HD_, HDT_)                                                                                                        \
  return axis == 0 ? (f16 ? attn_spatial<_Float16, HD_, HDT_>(qkv, out, n_seq, map, C, heads, st)                                \
                          : attn_spatial<__bf16, HD_, HDT_>(qkv, out, n_seq, map, C, heads, st))                                 \
                   : (f16 ? attn_temporal2<_Float16, HD_, HDT_>(qkv, out, n_seq, map, C, heads, st)                              \
                          : attn_temporal2<__bf16, HD_, HDT_>(qkv, out, n_seq, map, C, heads, st));
int d3dp_attn_fast_padded(int axis, const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads, hipStream_t st, int f16,
                          int hd_true) {
  if (heads < 1 || C % heads || map.n_tok < 1 || map.n_tok > (axis == 0 ? 32 : 1024)) return -2;
  const int hdp = C / heads;
  if (hdp == 32 && hd_true == 24) { AF_PAD(32, 24) }
  if (hdp == 64 && hd_true == 40) { AF_PAD(64, 40) }
  if (hdp == 64 && hd_true == 48) { AF_PAD(64, 48) }
  if (hdp == 64 && hd_true == 56) { AF_PAD(64, 56) }
  return -2;
}
#undef AF_PAD
#elif defined(D3DP_FAST_SCALED_TU)
// fp16 rows whose q, k and v hold 2^-s times their value: the kernels above with the exponent scale (C / heads)^-0.5 x `emul`, emul =
// 2^(2s).  Head dim 64, 32 or 16; axis 0: the spatial kernel (<= 32 tokens), otherwise the whole-sequence / chunked-key kernels
// (<= 1024 tokens, any SeqMap); -2 for any other shape
int d3dp_attn_fast_scaled(int axis, const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads, hipStream_t st, float emul) {
  if (heads < 1 || C % heads || map.n_tok < 1 || map.n_tok > (axis == 0 ? 32 : 1024)) return -2;
  switch (C / heads) {
    case 64: return axis == 0 ? attn_spatial<_Float16, 64, 1>(qkv, out, n_seq, map, C, heads, st, 0.125f * emul)
                              : attn_temporal2<_Float16, 64, 1>(qkv, out, n_seq, map, C, heads, st, 0.125f * emul);
    case 32: return axis == 0 ? attn_spatial<_Float16, 32, 1>(qkv, out, n_seq, map, C, heads, st, 0.17677669529663689f * emul)
                              : attn_temporal2<_Float16, 32, 1>(qkv, out, n_seq, map, C, heads, st, 0.17677669529663689f * emul);
    case 16: return axis == 0 ? attn_spatial<_Float16, 16, 1>(qkv, out, n_seq, map, C, heads, st, 0.25f * emul)
                              : attn_temporal2<_Float16, 16, 1>(qkv, out, n_seq, map, C, heads, st, 0.25f * emul);
  }
  return -2;
}
#else
// (f16: 0 = bf16 rows in and out, 1 = IEEE fp16.  Head dim 64, 32 or 16.  Any SeqMap: <= 256 tokens the whole-sequence kernel, up
//  to 1024 the chunked-key one.  hd_true: kernels.h)
int d3dp_launch_attn_temporal_bf16(const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads,
                                   hipStream_t st, int f16, int hd_true) {
  if (heads < 1 || C % heads || map.n_tok > 1024 || map.n_tok < 1) return -2;
  if (hd_true && hd_true != C / heads) return d3dp_attn_fast_padded(1, qkv, out, n_seq, map, C, heads, st, f16, hd_true);
  switch (C / heads) {
    case 64: return f16 ? attn_temporal2<_Float16, 64>(qkv, out, n_seq, map, C, heads, st) : attn_temporal2<__bf16, 64>(qkv, out, n_seq, map, C, heads, st);
    case 32: return f16 ? attn_temporal2<_Float16, 32>(qkv, out, n_seq, map, C, heads, st) : attn_temporal2<__bf16, 32>(qkv, out, n_seq, map, C, heads, st);
    case 16: return f16 ? attn_temporal2<_Float16, 16>(qkv, out, n_seq, map, C, heads, st) : attn_temporal2<__bf16, 16>(qkv, out, n_seq, map, C, heads, st);
  }
  return -2;
}

// spatial axis on MFMA (bf16 or, f16 == 1, IEEE fp16 rows; head dim 64, 32 or 16, <= 32 tokens per sequence)
int d3dp_launch_attn_spatial_bf16(const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads, hipStream_t st, int f16,
                                  int hd_true) {
  if (heads < 1 || C % heads || map.n_tok > 32 || map.n_tok < 1) return -2;
  if (hd_true && hd_true != C / heads) return d3dp_attn_fast_padded(0, qkv, out, n_seq, map, C, heads, st, f16, hd_true);
  switch (C / heads) {
    case 64: return f16 ? attn_spatial<_Float16, 64>(qkv, out, n_seq, map, C, heads, st) : attn_spatial<__bf16, 64>(qkv, out, n_seq, map, C, heads, st);
    case 32: return f16 ? attn_spatial<_Float16, 32>(qkv, out, n_seq, map, C, heads, st) : attn_spatial<__bf16, 32>(qkv, out, n_seq, map, C, heads, st);
    case 16: return f16 ? attn_spatial<_Float16, 16>(qkv, out, n_seq, map, C, heads, st) : attn_spatial<__bf16, 16>(qkv, out, n_seq, map, C, heads, st);
  }
  return -2;
}
#endif
#undef AF_HDT_PARAM
#undef AF_HDT_ARG
#undef AF_SCALE
#undef AF_ESC_PARAM
#undef AF_ESC_ARG
