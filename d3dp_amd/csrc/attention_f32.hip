// Multi-head attention of the MixSTE2 blocks, softmax(q k^T * hd^-0.5) v per (sequence, head) (reference common/mixste.py:63-79),
// with fp32 ARITHMETIC.  Sequences (17 joints of one frame / F frames of one joint) are addressed through SeqMap strides
// (kernels.h) in the one physical token layout (bh, f, n, c): the reference's transposes never happen.  The 2-byte matrix-core
// kernels are in attention_fast.hip, the split-fp16 ones of EXACT mode in attention_x2.hip.
//
//   attn_rows_kernel         : fp32 VALU, one thread per query row, K / V of the problem broadcast from LDS in chunks of <= 256
//                              keys under an online softmax.  Rows in: fp32, bf16 or fp16; out: the same type, or (fp32 in) three
//                              split-bf16 / two split-fp16 planes.  What attention() in capi_denoise.hip sends here is whatever no
//                              matrix-core kernel takes: every context whose head dim is not 64 (widths outside {64 .. 512} on
//                              the run-time head dim form); the spatial axis of D3DP_EXACT_IMPL=f32|bf16x3; a D3DP_LONG_ATTN=rows
//                              context beyond 256 frames (and, FAST / FAST16, beyond 32 joints).  The training step calls it for
//                              the attentions its split-fp16 kernels (train_attn.hip) do not run, with `amax`; d3dp_op_attention
//                              for impl 0.
//                              Limits: head dim 8 / 16 / 32 / 64, or (fp32 rows in and out) any multiple of 4 up to 128; n_tok >= 1;
//                              the K / V images of a workgroup within the CU's 160 KiB of LDS.
//   attn_temporal_f32_kernel : v_mfma_f32_16x16x4_f32 (bitwise an fp32 fmaf chain), fp32 rows in, the whole score row-block in
//                              registers.  The temporal axis of D3DP_EXACT_IMPL=f32|bf16x3 contexts -- the cross-checks of EXACT --
//                              of a training step without the split-fp16 attention and of d3dp_op_attention impl 1 on fp32 rows.
//                              Limits: head dim 64, 1 .. 256 tokens, act 0 / 2 / 3 (fp32 / split-bf16 / split-fp16 out).
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "ta_common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// generic fp32-VALU attention: thread per query row
// ------------------------------------------------------------------------------------------------
template <typename T> struct Vec16;   // 16-byte vector of T
template <> struct Vec16<float> { static constexpr int N = 4; };
template <> struct Vec16<bf16> { static constexpr int N = 8; };
template <> struct Vec16<f16> { static constexpr int N = 8; };

template <typename T, int N>
__device__ __forceinline__ void ld_vec(const T* p, float* v) {
  if constexpr (N == 4) {
    float4 a = *reinterpret_cast<const float4*>(p);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  } else {
    load8(p, v);                                       // (T: bf16 or f16)
  }
}

// OUT3: write the result as three split-bf16 planes (`plane` elements apart) instead of T -- the A operand
// format of the bf16x3 EXACT-mode Linear.
// Any sequence length: a thread owns the query rows row, row + TPP, ... of its problem, and K / V pass through LDS in
// chunks of `kchunk` keys under the online softmax (one chunk = the whole sequence up to 256 tokens, which is every BASELINE
// configuration; longer clips -- `-f 351`, reference common/arguments.py:58 -- run here instead of being refused).
// amax (optional): absmax of the fp32 output, one atomicMax per workgroup (the training step's proj operand scale).
// GEN (round 6: any head dim the reference's `-cs` / 8 heads gives, common/arguments.py:49): HD is the register capacity, the
// head dim itself the run-time `hd_rt` (a multiple of the 16-byte vector, <= HD); the 16-byte slots behind it hold zeros in
// q / K / V and are not stored.  Instantiated for fp32 rows only (the fp32 implementation of the widths outside {64 .. 512}).
template <typename T, int HD, int TPP, int OUTS, bool GEN = false>   // OUTS: 0 = T out, 3 = three split-bf16 planes, 2 = two split-fp16 planes
__global__ __launch_bounds__(256) void attn_rows_kernel(const T* __restrict__ qkv, void* __restrict__ out_v, int n_prob,
                                                        SeqMap map, int C, int heads, size_t plane, int kchunk,
                                                        unsigned* __restrict__ amax, int hd_rt) {
  static_assert(!GEN || (OUTS == 0 && sizeof(T) == 4), "the run-time head dim form exists for fp32 rows");
  const int hd = GEN ? hd_rt : HD;
  constexpr int PPB = 256 / TPP;
  constexpr int VN = Vec16<T>::N;                 // elements per 16-byte vector
  constexpr int LDR = HD + VN;                    // padded LDS row (elements)
  constexpr int CH = (HD >= VN) ? HD / VN : 1;    // 16-byte chunks per row
  static_assert(HD % VN == 0, "head dim must be a multiple of the 16-byte vector");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  T* smem = reinterpret_cast<T*>(smem_raw);

  const int n = map.n_tok;
  const int tid = threadIdx.x;
  const int lp = tid / TPP, row = tid % TPP;
  const int pid = blockIdx.x * PPB + lp;
  const bool live = pid < n_prob;
  const int seq = live ? pid / heads : 0, head = live ? pid % heads : 0;
  const int base = ta_seq_base(map, seq);
  T* Ks = smem + (size_t)lp * 2 * kchunk * LDR;
  T* Vs = Ks + (size_t)kchunk * LDR;
  const float scale = 1.0f / sqrtf((float)hd);
  float am = 0.f;

  for (int q0 = 0; q0 < n; q0 += TPP) {
    const bool act = live && q0 + row < n;
    const size_t tok = (size_t)(base + (act ? q0 + row : 0) * map.tok_stride);
    float q[HD], o[HD];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (!GEN || c * VN < hd) ld_vec<T, VN>(qkv + tok * 3 * C + head * hd + c * VN, q + c * VN);
      else {
#pragma unroll
        for (int e = 0; e < VN; ++e) q[c * VN + e] = 0.f;
      }
    }
#pragma unroll
    for (int d = 0; d < HD; ++d) o[d] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int k0 = 0; k0 < n; k0 += kchunk) {
      const int nk = min(kchunk, n - k0);
      if (k0 > 0 || q0 > 0) __syncthreads();          // every thread is done with the chunk the images still hold
      if (live) {
        for (int u = row; u < nk * CH; u += TPP) {
          const int j = u / CH, c = u % CH;
          const T* src = qkv + (size_t)(base + (k0 + j) * map.tok_stride) * 3 * C + C + head * hd + c * VN;
          const bool in = !GEN || c * VN < hd;
          *reinterpret_cast<float4*>(Ks + j * LDR + c * VN) = in ? *reinterpret_cast<const float4*>(src) : make_float4(0.f, 0.f, 0.f, 0.f);
          *reinterpret_cast<float4*>(Vs + j * LDR + c * VN) = in ? *reinterpret_cast<const float4*>(src + C) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
      __syncthreads();
      if (!act) continue;
      // online softmax over groups of KB keys: KB independent score accumulators per pass (the dot products are latency
      // chains; with one wave per SIMD in the 243-key configuration nothing else hides them)
      constexpr int KB = 4;
      for (int j0 = 0; j0 < nk; j0 += KB) {
        float sc[KB];
#pragma unroll
        for (int u = 0; u < KB; ++u) sc[u] = 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
#pragma unroll
          for (int u = 0; u < KB; ++u) {
            const int j = min(j0 + u, nk - 1);
            float kv[VN];
            ld_vec<T, VN>(Ks + j * LDR + c * VN, kv);
#pragma unroll
            for (int e = 0; e < VN; ++e) sc[u] = fmaf(q[c * VN + e], kv[e], sc[u]);
          }
        }
        float gm = m;
#pragma unroll
        for (int u = 0; u < KB; ++u) {
          sc[u] = (j0 + u < nk) ? sc[u] * scale : -INFINITY;
          gm = fmaxf(gm, sc[u]);
        }
        if (gm > m) {
          const float f = expf(m - gm);
          l *= f;
#pragma unroll
          for (int d = 0; d < HD; ++d) o[d] *= f;
          m = gm;
        }
        float p[KB];
#pragma unroll
        for (int u = 0; u < KB; ++u) { p[u] = expf(sc[u] - m); l += p[u]; }
#pragma unroll
        for (int c = 0; c < CH; ++c) {
#pragma unroll
          for (int u = 0; u < KB; ++u) {
            const int j = min(j0 + u, nk - 1);
            float vv[VN];
            ld_vec<T, VN>(Vs + j * LDR + c * VN, vv);
#pragma unroll
            for (int e = 0; e < VN; ++e) o[c * VN + e] = fmaf(p[u], vv[e], o[c * VN + e]);
          }
        }
      }
    }
    if (!act) continue;
    const float inv = 1.0f / l;
    if constexpr (OUTS == 2) {
      f16* dst = reinterpret_cast<f16*>(out_v) + (size_t)tok * (2 * C);   // h2i row (common.h)
#pragma unroll
      for (int c = 0; c < HD / 4; ++c) {
        f16x4 p0, p1;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          f16 a0, a1;
          split2h(o[c * 4 + e] * inv, a0, a1);
          p0[e] = a0; p1[e] = a1;
        }
        const int hc = h2i_col(head * HD + c * 4);
        *reinterpret_cast<f16x4*>(dst + hc) = p0;
        *reinterpret_cast<f16x4*>(dst + hc + kH2iLo) = p1;
      }
    } else if constexpr (OUTS == 3) {
      bf16* dst = reinterpret_cast<bf16*>(out_v) + tok * C + head * HD;
#pragma unroll
      for (int c = 0; c < HD / 4; ++c) {
        bf16x4 p0, p1, p2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          bf16 a0, a1, a2;
          split3(o[c * 4 + e] * inv, a0, a1, a2);
          p0[e] = a0; p1[e] = a1; p2[e] = a2;
        }
        *reinterpret_cast<bf16x4*>(dst + c * 4) = p0;
        *reinterpret_cast<bf16x4*>(dst + plane + c * 4) = p1;
        *reinterpret_cast<bf16x4*>(dst + 2 * plane + c * 4) = p2;
      }
    } else {
      T* dst = reinterpret_cast<T*>(out_v) + tok * C + head * hd;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        if (GEN && c * VN >= hd) continue;
        float r[VN];
#pragma unroll
        for (int e = 0; e < VN; ++e) { r[e] = o[c * VN + e] * inv; am = fmaxf(am, fabsf(r[e])); }
        if constexpr (VN == 4) *reinterpret_cast<float4*>(dst + c * 4) = make_float4(r[0], r[1], r[2], r[3]);
        else store8(dst + c * 8, r);
      }
    }
  }
  if (amax) {
    // (in the DYNAMIC allocation, behind the images: a static array would push a 160 KiB opt-in over the CU's LDS)
    float* part_amax = reinterpret_cast<float*>(smem + (size_t)PPB * 2 * kchunk * LDR);
    am = wave_max(am);
    if ((threadIdx.x & 63) == 0) part_amax[threadIdx.x >> 6] = am;
    __syncthreads();
    if (threadIdx.x == 0)
      atomicMax(amax, __float_as_uint(fmaxf(fmaxf(part_amax[0], part_amax[1]), fmaxf(part_amax[2], part_amax[3]))));
  }
}

template <typename T, int HD, int TPP, int OUTS, bool GEN = false>
int launch_rows(const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads, size_t plane, unsigned* amax, hipStream_t st) {
  constexpr int PPB = 256 / TPP;
  constexpr int LDR = HD + Vec16<T>::N;
  const int n_prob = n_seq * heads;
  int kchunk = map.n_tok < 256 ? map.n_tok : 256;
  if (GEN) {                                           // a 128-wide head: the K / V images of 256 keys do not fit the CU's LDS
    const int fit = (int)((160 * 1024 - 16) / ((size_t)PPB * 2 * LDR * sizeof(T)));
    if (fit < 1) return -2;
    if (kchunk > fit) kchunk = fit >= 128 ? 128 : fit;
  }
  const size_t lds = (size_t)PPB * 2 * kchunk * LDR * sizeof(T) + 16;   // (+ the four absmax partials)
  if (lds > 160 * 1024) return -2;
  auto kern = attn_rows_kernel<T, HD, TPP, OUTS, GEN>;
  static PerDeviceOnce once;                          // (one per template instantiation = per kernel)
  if (once.get([&](int) { return d3dp_lds_opt_in(reinterpret_cast<const void*>(kern), 160 * 1024); }) < 0) return -3;
  hipLaunchKernelGGL(kern, dim3((n_prob + PPB - 1) / PPB), dim3(256), lds, st, (const T*)qkv, out, n_prob, map, C, heads,
                     plane, kchunk, amax, C / heads);
  return 0;
}

template <typename T, int OUTS>
int dispatch_rows(const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads, size_t plane, unsigned* amax, hipStream_t st) {
  const int hd = C / heads;
  const bool small = map.n_tok <= 32;
  if (map.n_tok < 1) return -2;
#define ROWS_CASE(HD_)                                                                                          \
  case HD_: return small ? launch_rows<T, HD_, 32, OUTS>(qkv, out, n_seq, map, C, heads, plane, amax, st)       \
                         : launch_rows<T, HD_, 256, OUTS>(qkv, out, n_seq, map, C, heads, plane, amax, st);
  switch (hd) {
    ROWS_CASE(64) ROWS_CASE(32) ROWS_CASE(16) ROWS_CASE(8)
    default: break;
  }
#undef ROWS_CASE
  // any other head dim (a multiple of 4 up to 128): the run-time form, fp32 rows in and out
  if constexpr (std::is_same<T, float>::value && OUTS == 0) {
    if (hd < 4 || hd % 4 || hd > 128 || hd * heads != C) return -2;
#define ROWS_GEN(HD_)                                                                                                       \
  {                                                                                                                         \
    if (small) {                                                                                                            \
      const int r = launch_rows<T, HD_, 32, OUTS, true>(qkv, out, n_seq, map, C, heads, plane, amax, st);                   \
      if (r != -2) return r;                          /* (-2: eight problems' images do not fit the LDS) */                 \
    }                                                                                                                       \
    return launch_rows<T, HD_, 256, OUTS, true>(qkv, out, n_seq, map, C, heads, plane, amax, st);                           \
  }
    if (hd <= 16) ROWS_GEN(16)
    if (hd <= 32) ROWS_GEN(32)
    if (hd <= 64) ROWS_GEN(64)
    ROWS_GEN(128)
#undef ROWS_GEN
  }
  return -2;
}

// ------------------------------------------------------------------------------------------------
// EXACT-mode temporal attention on the fp32 matrix cores (v_mfma_f32_16x16x4_f32: bitwise an fp32 fmaf chain).
// Same dataflow as the bf16 kernel (attention_fast.hip) -- S^T = K Q^T so the probabilities are already the B operand of O^T = V^T P^T --
// with fp32 K/V images in LDS (row strides 65 / 68 floats: conflict-free ds_read_b32 fragments), the whole score
// row-block in registers, two-pass fp32 softmax.  Output: fp32, or three split-bf16 planes (OUT3) for the bf16x3
// Linear that follows.
// ------------------------------------------------------------------------------------------------
constexpr int LDKF = 65, LDVF = 68;

// A workgroup = eight waves = eight consecutive query tiles of one (sequence, head) problem; grid = problems x ceil(tiles / 8):
// 544 problems of 16 tiles (the configs[4] training batch) quantise to three rounds of one 139-KiB workgroup per CU, 1,088
// half problems to 4.25 half rounds, and two waves per SIMD cover each other's LDS waits (four waves walking four tiles each:
// 178 us per launch).
constexpr int TF32_WAVES = 8;
template <int NKT, int OUTS>
__global__ __launch_bounds__(TF32_WAVES * 64) void attn_temporal_f32_kernel(const float* __restrict__ qkv, void* __restrict__ out_v,
                                                                         SeqMap map, int C, int heads, size_t plane, int groups) {
  constexpr int NK = 16 * NKT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* KS = reinterpret_cast<float*>(smem);
  float* VS = KS + NK * LDKF + 3;          // keep V rows 16-byte aligned (NK*65 + 3 is a multiple of 4 for NK % 16 == 0)
  const int n = map.n_tok;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int prob = blockIdx.x / groups, group = blockIdx.x % groups;
  const int seq = prob / heads, head = prob % heads;
  const int base = ta_seq_base(map, seq);
  const int ts = map.tok_stride;
  const size_t ld = (size_t)3 * C;
  const float* qbase = qkv + (size_t)base * ld + (size_t)head * 64;
  const int fi = lane & 15, fg = lane >> 4;
  const int n_qt = (n + 15) >> 4;

  // stage K (scalar stores, stride 65) and V (float4 stores, stride 68); zero the padding rows of V
  for (int idx = tid; idx < NK * 16; idx += TF32_WAVES * 64) {
    const int row = idx >> 4, c4 = (idx & 15) * 4;
    float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
    if (row < n) {
      const float* src = qbase + (size_t)row * ts * ld + c4;
      kv = *reinterpret_cast<const float4*>(src + C);
      vv = *reinterpret_cast<const float4*>(src + 2 * C);
    }
    float* kd = KS + row * LDKF + c4;
    kd[0] = kv.x; kd[1] = kv.y; kd[2] = kv.z; kd[3] = kv.w;
    *reinterpret_cast<float4*>(VS + row * LDVF + c4) = vv;
  }
  __syncthreads();
  const float cexp = 0.125f * 1.44269504088896340736f;
  for (int qt = group * TF32_WAVES + wave; qt < n_qt; qt = n_qt) {   // (one tile per wave)
    const int q = qt * 16 + fi;
    // contraction index of MFMA step kk for lane group g is d = 16 g + kk (K fragments use the same map)
    const float* qsrc = qbase + (size_t)min(q, n - 1) * ts * ld + fg * 16;
    float qv[16];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float4 a = *reinterpret_cast<const float4*>(qsrc + c * 4);
      qv[c * 4] = a.x; qv[c * 4 + 1] = a.y; qv[c * 4 + 2] = a.z; qv[c * 4 + 3] = a.w;
    }
    f32x4 s[NKT];
#pragma unroll
    for (int t = 0; t < NKT; ++t) {
      const float* kr = KS + (t * 16 + fi) * LDKF + fg * 16;
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) a = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[kk], qv[kk], a, 0, 0, 0);
      s[t] = a;                                   // S^T[key = 16t + 4 fg + r][query fi]
      __builtin_amdgcn_sched_barrier(0);          // bound the ds_read hoisting window (VGPR pressure)
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
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < NKT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        // exp(x) with x = (s - max) / 8 in natural units: exp2f keeps one rounding of the scaled argument
        s[t][r] = exp2f((s[t][r] - mx) * cexp);
        sum += s[t][r];
      }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    f32x4 o[4];
#pragma unroll
    for (int dn = 0; dn < 4; ++dn) o[dn] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NKT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* vr = VS + (t * 16 + 4 * fg + r) * LDVF + fi;   // V[key][dn*16 + fi]
#pragma unroll
        for (int dn = 0; dn < 4; ++dn) o[dn] = __builtin_amdgcn_mfma_f32_16x16x4f32(vr[dn * 16], s[t][r], o[dn], 0, 0, 0);
        if (r == 3) __builtin_amdgcn_sched_barrier(0);
      }
    if (q < n) {
      const float inv = 1.0f / sum;
      const size_t off = (size_t)(base + q * ts) * C + head * 64 + fg * 4;
#pragma unroll
      for (int dn = 0; dn < 4; ++dn) {
        float r4[4] = {o[dn][0] * inv, o[dn][1] * inv, o[dn][2] * inv, o[dn][3] * inv};
        if constexpr (OUTS == 2) {                      // h2i row (common.h)
          f16* dst = reinterpret_cast<f16*>(out_v) + (size_t)(base + q * ts) * (2 * C) + h2i_col(head * 64 + fg * 4 + dn * 16);
          f16x4 p0, p1;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            f16 a0, a1;
            split2h(r4[e], a0, a1);
            p0[e] = a0; p1[e] = a1;
          }
          *reinterpret_cast<f16x4*>(dst) = p0;
          *reinterpret_cast<f16x4*>(dst + kH2iLo) = p1;
        } else if constexpr (OUTS == 3) {
          bf16* dst = reinterpret_cast<bf16*>(out_v) + off + dn * 16;
          bf16x4 p0, p1, p2;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            bf16 a0, a1, a2;
            split3(r4[e], a0, a1, a2);
            p0[e] = a0; p1[e] = a1; p2[e] = a2;
          }
          *reinterpret_cast<bf16x4*>(dst) = p0;
          *reinterpret_cast<bf16x4*>(dst + plane) = p1;
          *reinterpret_cast<bf16x4*>(dst + 2 * plane) = p2;
        } else {
          *reinterpret_cast<float4*>(reinterpret_cast<float*>(out_v) + off + dn * 16) = make_float4(r4[0], r4[1], r4[2], r4[3]);
        }
      }
    }
  }
}

template <int NKT, int OUTS>
int launch_temporal_f32(const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads, size_t plane, hipStream_t st) {
  constexpr int NK = 16 * NKT;
  const size_t lds = (size_t)(NK * LDKF + 3 + NK * LDVF) * 4 + 16;
  auto kern = attn_temporal_f32_kernel<NKT, OUTS>;
  static PerDeviceOnce once;                          // (one per template instantiation = per kernel)
  if (once.get([&](int) { return d3dp_lds_opt_in(reinterpret_cast<const void*>(kern), 160 * 1024); }) < 0) return -3;
  const int groups = ((map.n_tok + 15) / 16 + TF32_WAVES - 1) / TF32_WAVES;
  hipLaunchKernelGGL(kern, dim3(n_seq * heads * groups), dim3(TF32_WAVES * 64), lds, st, (const float*)qkv, out, map, C, heads, plane,
                     groups);
  return 0;
}

}  // namespace

// act: 0 = fp32 in/out, 1 = bf16 in/out, 2 = fp32 in, split-bf16 planes out, 3 = fp32 in, split-fp16 planes out,
//      4 = IEEE fp16 in/out
// (amax: fp32 output only -- its absmax, see the kernel)
int d3dp_launch_attn_rows(int act, const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads, hipStream_t st,
                          unsigned* amax) {
  const size_t plane = (size_t)n_seq * map.n_tok * C;
  if (act != 0 && amax) return -1;
  if (act == 1) return dispatch_rows<bf16, 0>(qkv, out, n_seq, map, C, heads, plane, nullptr, st);
  if (act == 4) return dispatch_rows<f16, 0>(qkv, out, n_seq, map, C, heads, plane, nullptr, st);
  if (act == 2) return dispatch_rows<float, 3>(qkv, out, n_seq, map, C, heads, plane, nullptr, st);
  if (act == 3) return dispatch_rows<float, 2>(qkv, out, n_seq, map, C, heads, plane, nullptr, st);
  return dispatch_rows<float, 0>(qkv, out, n_seq, map, C, heads, plane, amax, st);
}

// EXACT-mode temporal axis on the fp32 matrix cores (head dim 64); act 0 -> fp32 out, 2 -> split-bf16 planes out,
// 3 -> split-fp16 planes out
int d3dp_launch_attn_temporal_f32(int act, const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads,
                                  hipStream_t st) {
  if (C / heads != 64 || map.n_tok > 256 || map.n_tok < 1 || (act != 0 && act != 2 && act != 3)) return -2;
  const size_t plane = (size_t)n_seq * map.n_tok * C;
  const int n = map.n_tok;
#define TF32_CASE(NKT_)                                                                                       \
  return act == 3 ? launch_temporal_f32<NKT_, 2>(qkv, out, n_seq, map, C, heads, plane, st)                   \
       : act == 2 ? launch_temporal_f32<NKT_, 3>(qkv, out, n_seq, map, C, heads, plane, st)                   \
                  : launch_temporal_f32<NKT_, 0>(qkv, out, n_seq, map, C, heads, plane, st);
  if (n <= 32) { TF32_CASE(2) }
  if (n <= 64) { TF32_CASE(4) }
  if (n <= 128) { TF32_CASE(8) }
  TF32_CASE(16)
#undef TF32_CASE
}
