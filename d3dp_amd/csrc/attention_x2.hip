// EXACT-mode attention on the fp16 matrix cores: split-fp16 operands (a hi and a lo fp16 plane per value), three
// v_mfma_f32_16x16x32_f16 passes per product -- the scheme of the EXACT Linear (gemm_x2.hip) -- fp32 accumulation and softmax.
// Input: the PACKED qkv rows the qkv Linear writes in this mode (gemm_x2.hip, EPI_QKV_PACK), 12 C bytes per token:
//     q fp32 [C] | k hi [C] | k lo [C] | v hi [C] | v lo [C]      (fp16 planes of the value x act_scale, 16 by default)
// (whole-C planes: the row format does not depend on the head dim; head h owns columns h HD .. h HD + HD - 1 of each)
// so K and V are already MFMA operands and the query fragments are split in registers.  S^T = Kl.Qh + Kh.Ql + Kh.Qh (the operand
// scales folded into the exponent constant); the probabilities are split into fp16 pairs x 1024 (the +10 in the exponent bias
// of every softmax below) and O^T = Vl.Ph + Vh.Pl + Vh.Ph; the output leaves as fp32 rows (act 0) or as the two fp16 planes
// the proj Linear consumes (act 3).
// Every kernel is a template on the head dim HD: 64 (the default, `-cs 512`), 32 or 16 (`-cs` 256 / 128 with the model's 8
// heads) -- the k-depth of S^T (two 16x16x32 MFMAs per pass and key tile, one, or one 16-deep v_mfma_f32_16x16x16_f16) and the
// HD / 16 output-channel tiles of O^T; see X2Head below.  No lane reads a column of another head.  Head dim 8 (half the
// narrowest k-depth) and the training step's attention (train_attn.hip: head dim 64) are not here.
//
//   attn_spatial_x2_kernel       : axis 0 with <= 32 tokens per sequence: one wave per (sequence, head), K fragments straight
//                                  from the packed rows, V through a private LDS image (attn_frag.h).
//   attn_temporal_x2_kernel      : any SeqMap up to 256 tokens: persistent workgroups, K and V by LDS-DMA into the images of
//                                  attn_frag.h, the whole score row in registers, two-pass softmax.  5.3x fewer matrix-pipe cycles
//                                  than the fp32-MFMA kernel it replaced (16x16x4 f32: 32 cycles for 2 Kflop; three 16x16x32 f16:
//                                  48 cycles for 16 Kflop).
//   attn_temporal_x2_long_kernel : 257 tokens and more (the library stops at 1024): keys in chunks of 128 under an online
//                                  softmax, on the images and helpers of ta_common.h.
//   qkv_pack_x2_kernel           : fp32 qkv rows -> packed rows, for d3dp_op_attention, whose C-ABI input is the fp32 layout.
//
// attention() in capi_denoise.hip sends both axes of an EXACT context here (act 3) when it runs the split-fp16 implementation -- the
// default; D3DP_EXACT_IMPL=f32|bf16x3 does not -- at head dims 64, 32 and 16, unless D3DP_LONG_ATTN=rows keeps the fp32 row kernel
// (attention_f32.hip): for a clip of more than 256 frames at head dim 64, for every shape at head dims 32 and 16;
// d3dp_op_attention with impl 2 (act 0).  d3dp_launch_attn_x2 refuses (-2) any other
// head dim, act or a scale that is not positive.
//
// Build switches, all off in the product and head dim 64 only: the measured-negative forms of the temporal kernel that DESIGN.md section 7 cites and
// tests/test_abi.py keeps compiling, and one instrumented build.  The code only they use is in attention_x2_variants.h; here
// is each switch's default and the sites that select.
//   -DD3DP_ATTN_OVERLAP=1 : two tiles per wave: the softmax of one tile between the matrix instructions of the other (tile 0's
//                           under tile 1's scores, tile 1's under tile 0's P.V); bit-identical results.  MEASURED
//                           (profiles/r04_attn_timeline.md): the score phase loses 2 k cycles, the P.V phase gains them, a problem
//                           takes 30.55 k cycles in either form -- set by something both share, not by where the VALU work sits.
//   -DD3DP_ATTN_KPIPE=1   : the next key-tile pair's K fragments into the registers the current pair frees (attn_scores_x2_pair).
//   -DD3DP_ATTN_MIXLO=1   : the lo halves of the probabilities by v_fma_mixlo_f16 / v_fma_mixhi_f16 (x2_lo_pair_mix).
//   -DD3DP_ATTN_W16=1     : 241 .. 256 frames on attn_temporal_x2_w16_kernel, sixteen waves of one tile each.
//   -DD3DP_ATTN_STAMP=1   : cycle stamps at the temporal kernel's phase boundaries (see there; tools/attn_stamps.py).
#include "common.h"
#include "kernels.h"
#include "ta_common.h"
#include "attn_frag.h"

#ifndef D3DP_ATTN_OVERLAP
#define D3DP_ATTN_OVERLAP 0
#endif
#ifndef D3DP_ATTN_KPIPE
#define D3DP_ATTN_KPIPE 0
#endif
#ifndef D3DP_ATTN_MIXLO
#define D3DP_ATTN_MIXLO 0
#endif
#ifndef D3DP_ATTN_W16
#define D3DP_ATTN_W16 0
#endif
#ifndef D3DP_ATTN_STAMP
#define D3DP_ATTN_STAMP 0
#endif

namespace {

__device__ __forceinline__ f16x8 as_f16x8(bf16x8 v) { return __builtin_bit_cast(f16x8, v); }

// Operand scales of the split-fp16 attention kernels (kernel argument; wave-uniform).  q is split in registers at `q`; the
// k / v planes of the packed rows were written at that same scale by the qkv Linear; `cexp` = hd^-0.5 log2(e) / (q scale x
// k scale) folds both into the softmax exponent; `onorm` = 1 / v scale brings O^T back to its true scale; `oplane` = the scale
// at which a plane output is split (that of v: |o| <= max |v|).  Everything is 2^4-based unless capi_weights.hip lowered the scale of
// a block whose proven operand range asks for it (d3dp_exact_range_bound).
// The true-scale value is formed FIRST and the (power-of-two, hence exact) plane scale applied inside the split on purpose:
// with  x = o * (1 / denom)  handed to the split directly, hipcc (ROCm 7.2) folds the fp16 conversion of the INEXACT product
// into v_fma_mixlo_f16 for the lo half -- f16(o * inv) rounded once from the exact product -- while the stored hi half is
// v_cvt_pk_f16_f32 of the fp32-rounded product: wherever the two roundings disagree (about 1 element in 2^13) hi + lo is off
// by a whole fp16 ulp of hi, and the denoiser's error against the reference tripled (run c5: 6.4e-4 -> 1.8e-3 mm).  The
// exact scaling in between makes both halves round the same number.
struct X2Scales { float q, cexp, onorm, oplane; };

// What follows from the head dim HD, a template parameter of every kernel below (64 -- the default, `-cs 512` -- 32 or 16: `-cs`
// 256 / 128 with the model's 8 heads).  It is the k-depth of S^T: two 16x16x32 MFMAs per pass and key tile at 64, one at 32, and at
// 16 ONE 16-deep MFMA (v_mfma_f32_16x16x16_f16, Op2<f16>'s x4 form: lane (i, g) holds d = 4 g .. 4 g + 3 of row i, 8 bytes, so no
// lane addresses a column outside its head and nothing is padded: a 16-byte slot there is HALF a head's row).  And HD / 16 is the
// number of output-channel tiles of O^T.  A K or V row of one plane is ROWB = 2 HD bytes = 2^LS 16-byte slots, in the packed rows
// and in LDS (images and swizzles: attn_frag.h); a query row is NQL 16-byte loads per lane.
template <int HD> struct X2Head {
  static_assert(HD == 64 || HD == 32, "head dim");
  typedef f16x8 frag;
  static constexpr int ROWB = 2 * HD, LS = HD == 64 ? 3 : 2, NQ = HD / 32, NQL = HD / 16;
};
template <> struct X2Head<16> {
  typedef f16x4 frag;
  static constexpr int ROWB = 32, LS = 1, NQ = 1, NQL = 1;
};

// key chunks [C0, C1) of O^T += V^T P^T (32 keys per chunk).  Software-pipelined by hand: the fragments of chunk c+1 are
// read before the MFMAs of chunk c, and the twelve MFMAs of a chunk go pass by pass over the four channel tiles, so that
// two MFMAs on the same accumulator are four apart (issued back to back each waits out the previous one's latency:
// with two waves per SIMD the kernel spent 39 % of its wave cycles in such issue stalls).
// (HD / 16 channel tiles: at head dims 32 and 16 two MFMAs on the same accumulator are two apart / back to back -- there the
// other waves of the SIMD, of which the smaller images and register sets allow more, cover the latency instead)
template <int C0, int HD>
__device__ __forceinline__ void load_v_frags_x2(const FragBasesT<HD>& fb, int plane, f16x8 (&vh)[HD / 16], f16x8 (&vl)[HD / 16]) {
#pragma unroll
  for (int dn = 0; dn < HD / 16; ++dn) {
    vh[dn] = load_vt_frag<C0, f16, HD>(fb.v[dn]);
    vl[dn] = load_vt_frag<C0, f16, HD>(fb.v[dn] + plane);
  }
}
template <int NKT, int C0, int C1 = NKT / 2, int HD>
__device__ __forceinline__ void pv_chunks_x2_rec(const FragBasesT<HD>& fb, int plane, const f16x8 (&ph)[NKT / 2],
                                                 const f16x8 (&pl)[NKT / 2], f32x4 (&o)[HD / 16], const f16x8 (&vh)[HD / 16],
                                                 const f16x8 (&vl)[HD / 16]) {
  constexpr int ND = HD / 16;
  f16x8 nh[ND], nl[ND];
  if constexpr (C0 + 1 < C1) load_v_frags_x2<C0 + 1>(fb, plane, nh, nl);
  __builtin_amdgcn_sched_barrier(0);                   // (the reads stay in front of the MFMAs that cover their latency)
#pragma unroll
  for (int dn = 0; dn < ND; ++dn) o[dn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vl[dn], ph[C0], o[dn], 0, 0, 0);
#pragma unroll
  for (int dn = 0; dn < ND; ++dn) o[dn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh[dn], pl[C0], o[dn], 0, 0, 0);
#pragma unroll
  for (int dn = 0; dn < ND; ++dn) o[dn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh[dn], ph[C0], o[dn], 0, 0, 0);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (C0 + 1 < C1) pv_chunks_x2_rec<NKT, C0 + 1, C1>(fb, plane, ph, pl, o, nh, nl);
}
template <int NKT, int C0, int C1 = NKT / 2, int HD>
__device__ __forceinline__ void pv_chunks_x2(const FragBasesT<HD>& fb, int plane, const f16x8 (&ph)[NKT / 2],
                                             const f16x8 (&pl)[NKT / 2], f32x4 (&o)[HD / 16]) {
  if constexpr (C0 < C1) {
    f16x8 vh[HD / 16], vl[HD / 16];
    load_v_frags_x2<C0>(fb, plane, vh, vl);
    pv_chunks_x2_rec<NKT, C0, C1>(fb, plane, ph, pl, o, vh, vl);
  }
}

// the same product one channel tile after the other (8 fragment registers live instead of 32: the spatial kernel, whose
// occupancy -- five waves per SIMD at <= 96 registers -- matters more to it than MFMA issue order)
template <int C0, int HD>
__device__ __forceinline__ void pv_chunk_x2_seq(const FragBasesT<HD>& fb, int plane, const f16x8& ph, const f16x8& pl,
                                                f32x4 (&o)[HD / 16]) {
#pragma unroll
  for (int dn = 0; dn < HD / 16; ++dn) {
    const f16x8 vh = load_vt_frag<C0, f16, HD>(fb.v[dn]);
    const f16x8 vl = load_vt_frag<C0, f16, HD>(fb.v[dn] + plane);
    o[dn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vl, ph, o[dn], 0, 0, 0);
    o[dn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, pl, o[dn], 0, 0, 0);
    o[dn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, ph, o[dn], 0, 0, 0);
  }
}

__device__ __forceinline__ void x2_split4(const f32x4 a, f16x4& hi, f16x4& lo, float sc) {
#pragma unroll
  for (int e = 0; e < 4; ++e) { f16 h, l; split2h_scaled(a[e] * sc, h, l); hi[e] = h; lo[e] = l; }
}

// this lane's query fragments, split: HD fp32 of row q (`qrow`: the head's first column) over the four lane groups -- d = fg*8 .. +7
// (and 32 + fg*8 .. +7 at head dim 64); d = fg*4 .. +3 at head dim 16, the k order of the 16-deep MFMA
template <int HD>
__device__ __forceinline__ void load_q_x2(const float* qrow, int fg, typename X2Head<HD>::frag (&qh)[X2Head<HD>::NQ],
                                          typename X2Head<HD>::frag (&ql)[X2Head<HD>::NQ], float sc) {
  if constexpr (HD == 16) {
    x2_split4(*reinterpret_cast<const f32x4*>(qrow + fg * 4), qh[0], ql[0], sc);
  } else {
#pragma unroll
    for (int half = 0; half < X2Head<HD>::NQ; ++half) {
      const float* p = qrow + half * 32 + fg * 8;
      ta_split8(*reinterpret_cast<const float4*>(p), *reinterpret_cast<const float4*>(p + 4), qh[half], ql[half], sc);
    }
  }
}

// this lane's K fragments of key row `krow` (packed row, the head's first column: hi plane at krow, lo plane C halves further):
// already operands
template <int HD>
__device__ __forceinline__ void load_k_x2(const f16* krow, int C, int fg, typename X2Head<HD>::frag (&kh)[X2Head<HD>::NQ],
                                          typename X2Head<HD>::frag (&kl)[X2Head<HD>::NQ]) {
  typedef typename X2Head<HD>::frag frag;
  constexpr int QW = HD == 16 ? 4 : 8;
#pragma unroll
  for (int half = 0; half < X2Head<HD>::NQ; ++half) {
    kh[half] = *reinterpret_cast<const frag*>(krow + half * 32 + fg * QW);
    kl[half] = *reinterpret_cast<const frag*>(krow + C + half * 32 + fg * QW);
  }
}

// head dims 32 and 16: S^T of one key tile = Kl.Qh + Kh.Ql + Kh.Qh, one MFMA per pass (the small terms first)
template <typename F>
__device__ __forceinline__ f32x4 x2_tile_scores(const F& kh, const F& kl, const F& qh, const F& ql) {
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  a = Op2<f16>::mfma(kl, qh, a);
  a = Op2<f16>::mfma(kh, ql, a);
  return Op2<f16>::mfma(kh, qh, a);
}

// O^T accumulators -> out row `tok` (fp32 [T][C], or the h2i layout of the proj Linear's operand, common.h): lane holds
// channels col + dn*16 + (0..3), dn < HD / 16, col = head*HD + 4 fg.  `inv` = onorm / (1024 x softmax denominator): o * inv is the TRUE-scale
// value; plane outputs are split at `oplane` (see X2Scales for why in this order)
template <int OUTS, int ND>
__device__ __forceinline__ void store_o_x2(const f32x4 (&o)[ND], float inv, void* out_v, size_t tok, int C, int col,
                                           float oplane) {
#pragma unroll
  for (int dn = 0; dn < ND; ++dn) {
    const float r4[4] = {o[dn][0] * inv, o[dn][1] * inv, o[dn][2] * inv, o[dn][3] * inv};
    if constexpr (OUTS == 2) {
      f16x4 p0, p1;
#pragma unroll
      for (int e = 0; e < 4; ++e) { f16 a0, a1; split2h_scaled(r4[e] * oplane, a0, a1); p0[e] = a0; p1[e] = a1; }
      // ONE 16-byte store per lane instead of two of 8 bytes (the store side of these latency-bound
      // kernels).  Lanes l and l ^ 16 hold neighbouring 4-channel groups of the same row (fg even / odd): v_permlane16_swap
      // exchanges the odd 16-lane rows of its first operand with the even rows of its second, so with (hi, lo) as operands the
      // even-row lane ends up with both hi halves -- 8 consecutive channels of the hi slot -- and the odd-row lane with both
      // lo halves.  (Both lanes share `lane & 15`, i.e. the caller's q < n predicate.)
      const uint2 h = __builtin_bit_cast(uint2, p0), l = __builtin_bit_cast(uint2, p1);
      const auto sx = __builtin_amdgcn_permlane16_swap(h.x, l.x, false, false);
      const auto sy = __builtin_amdgcn_permlane16_swap(h.y, l.y, false, false);
      using u32x4 = unsigned __attribute__((ext_vector_type(4)));
      const u32x4 out16 = {sx[0], sy[0], sx[1], sy[1]};  // even row: hi own | hi partner; odd row: lo partner | lo own
      const bool oddrow = (col >> 2) & 1;                // fg odd (col = head HD + 4 fg)
      const int c8 = (col & ~7) + dn * 16;               // first of the pair's 8 channels
      f16* dst = reinterpret_cast<f16*>(out_v) + tok * (2 * C) + h2i_col(c8) + (oddrow ? kH2iLo : 0);
      *reinterpret_cast<u32x4*>(dst) = out16;
    } else {
      *reinterpret_cast<float4*>(reinterpret_cast<float*>(out_v) + tok * C + col + dn * 16) = make_float4(r4[0], r4[1], r4[2], r4[3]);
    }
  }
}

// One LDS-DMA wave-instruction: lane l's 16 bytes at `g` -> LDS bytes [lds + 16 l, +16) (`lds` wave-uniform).  Issued as
// inline assembly on purpose: for the builtin the compiler (a) holds every later ds_read that might alias the destination
// behind vmcnt(0) and (b) marks the instruction as a FLAT access of two address spaces, after which it stops counting
// and turns EVERY vector-memory wait of the kernel into vmcnt(0) -- both would serialise the pipeline below, whose
// ordering is carried by explicit counted waits and barriers instead.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"          // (the expected "clobber list contains reserved registers" note for m0)
__device__ __forceinline__ void lds_dma16(const char* g, const char* lds) {
  const unsigned la = (unsigned)(__UINTPTR_TYPE__)LPTR(lds);
  // m0 is declared clobbered (the compiler answers with "clobber list contains reserved registers" and
  // re-materialises m0 before each of its own uses, of which these kernels have none): no instruction is added to the
  // hand-counted pipeline
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(la) : "memory", "m0");
}
#pragma clang diagnostic pop

// 16-byte global load the compiler does not track (it would wait for it with counts that ignore the LDS-DMA operations
// queued behind it, i.e. far too early): the caller waits with wait_vmcnt and then passes the registers through settle().
__device__ __forceinline__ f32x4 gload16_untracked(const float* p) {
  f32x4 r;
  asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(r) : "v"(p) : "memory");
  return r;
}
__device__ __forceinline__ void settle(f32x4& r) { asm volatile("" : "+v"(r)); }
// The same load INTO the registers `r` already occupies (head dims 32 and 16, whose query registers are few): as an in-out operand
// the destination is live from the previous problem's query on, so the compiler cannot lend it to the address arithmetic in
// front of the load either -- harmless, but it is what the ISA scan of tests/test_abi.py, which reads the problem loop's blocks
// in layout order, takes for a write inside the load's in-flight window.
__device__ __forceinline__ void gload16_untracked_into(f32x4& r, const float* p) {
  asm volatile("global_load_dwordx4 %0, %1, off" : "+v"(r) : "v"(p) : "memory");
}

// s_waitcnt vmcnt(v) with the other counters left alone (gfx9 encoding: vmcnt [3:0] + [15:14], expcnt [6:4], lgkmcnt [11:8])
template <int V>
__device__ __forceinline__ void wait_vmcnt() { __builtin_amdgcn_s_waitcnt((V & 15) | (7 << 4) | (15 << 8) | ((V >> 4) << 14)); }

#if D3DP_ATTN_OVERLAP || D3DP_ATTN_MIXLO || D3DP_ATTN_W16
#include "attention_x2_variants.h"                       // (here: its code calls the helpers above and is called from below)
#endif

// Softmax of one 16-query tile's score row s (S^T fragments: lane holds keys 16 t + 4 fg + r of query lane & 15) and
// the split of the probabilities into fp16 pairs (x 1024); `denom` = 1024 x the softmax denominator of query (lane & 15).
template <int NKT, bool MASK_ANY_TILE>
__device__ __forceinline__ void softmax_split_x2(f32x4 (&s)[NKT], int n, int lane, f16x8 (&ph)[NKT / 2], f16x8 (&pl)[NKT / 2],
                                                 float& denom, float cexp) {
  const int fg = lane >> 4;                            // cexp = hd^-0.5 log2(e) / (q scale x k scale), X2Scales
  // keys >= n are masked.  The usual case (n in the last key tile: MASK_ANY_TILE = false, chosen by the launcher) touches
  // that tile only; the per-element selects of the general form were a third of this kernel's VALU instructions, and
  // their 64 loop-invariant lane masks cost registers.
  if constexpr (!MASK_ANY_TILE) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (16 * (NKT - 1) + 4 * fg + r >= n) s[NKT - 1][r] = -INFINITY;
  } else {
#pragma unroll
    for (int t = 0; t < NKT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (16 * t + 4 * fg + r >= n) s[t][r] = -INFINITY;
  }
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[t][r]);
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  // p * 1024 = exp2(s cexp - mx cexp + 10): one fma and the bare v_exp_f32 per element (arguments <= 10; a probability
  // below 2^-126 becomes 0 instead of a denormal); the denominator is accumulated at the same scale.
  const float nb = fmaf(-mx, cexp, 10.0f);
  float sum4[2] = {0.f, 0.f};                          // two independent chains
#if D3DP_ATTN_MIXLO
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    using f16x2v = _Float16 __attribute__((ext_vector_type(2)));
    unsigned hp[2], lp[2];
#pragma unroll
    for (int r = 0; r < 4; r += 2) {
      const float y0 = __builtin_amdgcn_exp2f(fmaf(s[t][r], cexp, nb)), y1 = __builtin_amdgcn_exp2f(fmaf(s[t][r + 1], cexp, nb));
      sum4[0] += y0;
      sum4[1] += y1;
      const f16x2v h2 = {(f16)y0, (f16)y1};
      hp[r >> 1] = __builtin_bit_cast(unsigned, h2);
      lp[r >> 1] = x2_lo_pair_mix(y0, y1, hp[r >> 1]);
    }
    using u32x4v = unsigned __attribute__((ext_vector_type(4)));
    u32x4v hv = __builtin_bit_cast(u32x4v, ph[t >> 1]), lv = __builtin_bit_cast(u32x4v, pl[t >> 1]);
    hv[(t & 1) * 2] = hp[0]; hv[(t & 1) * 2 + 1] = hp[1];
    lv[(t & 1) * 2] = lp[0]; lv[(t & 1) * 2 + 1] = lp[1];
    ph[t >> 1] = __builtin_bit_cast(f16x8, hv);
    pl[t >> 1] = __builtin_bit_cast(f16x8, lv);
  }
#else
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float y = __builtin_amdgcn_exp2f(fmaf(s[t][r], cexp, nb));
      sum4[r & 1] += y;
      const f16 h = (f16)y;
      ph[t >> 1][(t & 1) * 4 + r] = h;
      pl[t >> 1][(t & 1) * 4 + r] = (f16)fmaf(y, 1.0f, -(float)h);
    }
  }
#endif
  float sum = sum4[0] + sum4[1];
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  denom = sum;                                         // = 1024 x the softmax denominator
}

// Scores and softmax of one 16-query tile against NKT 16-key tiles resident in LDS.  fb: fragment bases into the K hi
// image (the lo image is `plane` bytes further).  qh/ql: the tile's query fragments (d 0..31, 32..63), values x 16.
// Returns the probabilities as split-fp16 B operands (x 1024) and 1024 x the softmax denominator of query (lane & 15).
template <int NKT, bool MASK_ANY_TILE>
__device__ __forceinline__ void attn_scores_x2(const FragBases& fb, int plane, const f16x8 (&qh)[2], const f16x8 (&ql)[2],
                                               int n, int lane, f16x8 (&ph)[NKT / 2], f16x8 (&pl)[NKT / 2], float& denom,
                                               float cexp) {
  // S^T, two key tiles at a time with their MFMAs interleaved (two independent accumulator chains) and the fragments
  // of the next pair already on their way from LDS (see pv_chunks_x2)
  f32x4 s[NKT];
  auto read_k = [&](int t, f16x8 (&k)[4]) {
    k[0] = *reinterpret_cast<const f16x8*>(fb.k0 + plane + t * 2048);   // lo, d 0..31
    k[1] = *reinterpret_cast<const f16x8*>(fb.k1 + plane + t * 2048);   // lo, d 32..63
    k[2] = *reinterpret_cast<const f16x8*>(fb.k0 + t * 2048);           // hi
    k[3] = *reinterpret_cast<const f16x8*>(fb.k1 + t * 2048);
  };
  // PF = 1: the lo-plane fragments of the NEXT pair are read before this pair's MFMAs (16 registers; prefetching all
  // four fragments per tile does not fit the 256 registers of the two-tile temporal kernel)
  f16x8 kc[2][4], kn[2][2];
  read_k(0, kc[0]);
  read_k(1, kc[1]);
#pragma unroll
  for (int t = 0; t < NKT; t += 2) {
    if (t + 2 < NKT) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        kn[j][0] = *reinterpret_cast<const f16x8*>(fb.k0 + plane + (t + 2 + j) * 2048);
        kn[j][1] = *reinterpret_cast<const f16x8*>(fb.k1 + plane + (t + 2 + j) * 2048);
      }
    }
    __builtin_amdgcn_sched_barrier(0);                 // (the reads stay in front of the MFMAs that cover their latency)
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
    a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kc[0][0], qh[0], a, 0, 0, 0);
    b = __builtin_amdgcn_mfma_f32_16x16x32_f16(kc[1][0], qh[0], b, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kc[0][1], qh[1], a, 0, 0, 0);
    b = __builtin_amdgcn_mfma_f32_16x16x32_f16(kc[1][1], qh[1], b, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kc[0][2], ql[0], a, 0, 0, 0);
    b = __builtin_amdgcn_mfma_f32_16x16x32_f16(kc[1][2], ql[0], b, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kc[0][3], ql[1], a, 0, 0, 0);
    b = __builtin_amdgcn_mfma_f32_16x16x32_f16(kc[1][3], ql[1], b, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kc[0][2], qh[0], a, 0, 0, 0);
    b = __builtin_amdgcn_mfma_f32_16x16x32_f16(kc[1][2], qh[0], b, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kc[0][3], qh[1], a, 0, 0, 0);
    b = __builtin_amdgcn_mfma_f32_16x16x32_f16(kc[1][3], qh[1], b, 0, 0, 0);
    s[t] = a; s[t + 1] = b;
    if (t + 2 < NKT) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        kc[j][0] = kn[j][0]; kc[j][1] = kn[j][1];
        kc[j][2] = *reinterpret_cast<const f16x8*>(fb.k0 + (t + 2 + j) * 2048);
        kc[j][3] = *reinterpret_cast<const f16x8*>(fb.k1 + (t + 2 + j) * 2048);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  softmax_split_x2<NKT, MASK_ANY_TILE>(s, n, lane, ph, pl, denom, cexp);
}

// The same for BOTH 16-query tiles of a wave at once (temporal kernel, two tiles per wave): every K fragment is read from
// LDS once for the two tiles (half the fragment reads) and the MFMAs run as FOUR independent accumulator chains (two query
// tiles x two key tiles), so two MFMAs on the same accumulator are four instructions apart instead of two -- half of this
// kernel's wave cycles were issue stalls behind dependent MFMAs with the matrix pipes 29 % busy (profiles/r03_attn_pmc.md).
template <int NKT, bool MASK_ANY_TILE>
__device__ __forceinline__ void attn_scores_x2_pair(const FragBases& fb, int plane, const f16x8 (&qh)[2][2],
                                                    const f16x8 (&ql)[2][2], int n, int lane, f16x8 (&ph)[2][NKT / 2],
                                                    f16x8 (&pl)[2][NKT / 2], float (&denom)[2], float cexp) {
  f32x4 s0[NKT], s1[NKT];
  auto read_k = [&](int t, f16x8 (&k)[4]) {
    k[0] = *reinterpret_cast<const f16x8*>(fb.k0 + plane + t * 2048);   // lo, d 0..31
    k[1] = *reinterpret_cast<const f16x8*>(fb.k1 + plane + t * 2048);   // lo, d 32..63
    k[2] = *reinterpret_cast<const f16x8*>(fb.k0 + t * 2048);           // hi
    k[3] = *reinterpret_cast<const f16x8*>(fb.k1 + t * 2048);
  };
  // No registers are left for a prefetch of the next pair's fragments (s0 + s1 hold 128).  -DD3DP_ATTN_KPIPE=1 is the
  // prefetch that needs none -- a pair's lo fragments are dead after its first eight MFMAs and its hi fragments after its
  // last, so the next pair's are requested into the same registers behind MFMA 8 and MFMA 24 instead of all eight in front
  // of the pair's MFMAs, where the compiler puts them.  Measured (run a2, interleaved): no difference (625 against
  // 626 us for the micro-benchmark's repack + kernel) -- the other wave of the SIMD already covers those LDS round trips.
  f16x8 kc[2][4];
#define X2_PAIR_TERM(KI, Q, D)                                                                  \
    a0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(kc[0][KI], Q[0][D], a0, 0, 0, 0);               \
    b0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(kc[1][KI], Q[0][D], b0, 0, 0, 0);               \
    a1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(kc[0][KI], Q[1][D], a1, 0, 0, 0);               \
    b1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(kc[1][KI], Q[1][D], b1, 0, 0, 0);
#if D3DP_ATTN_KPIPE
  auto read_lo = [&](int t, f16x8 (&k)[4]) {
    k[0] = *reinterpret_cast<const f16x8*>(fb.k0 + plane + t * 2048);
    k[1] = *reinterpret_cast<const f16x8*>(fb.k1 + plane + t * 2048);
  };
  auto read_hi = [&](int t, f16x8 (&k)[4]) {
    k[2] = *reinterpret_cast<const f16x8*>(fb.k0 + t * 2048);
    k[3] = *reinterpret_cast<const f16x8*>(fb.k1 + t * 2048);
  };
  read_k(0, kc[0]);
  read_k(1, kc[1]);
#endif
#pragma unroll
  for (int t = 0; t < NKT; t += 2) {
#if !D3DP_ATTN_KPIPE
    read_k(t, kc[0]);
    read_k(t + 1, kc[1]);
#endif
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, b0 = a0, a1 = a0, b1 = a0;
    // K fragment index / query operand of the six product terms: Kl.Qh (d 0..31, 32..63), Kh.Ql, Kh.Qh
    X2_PAIR_TERM(0, qh, 0)
    X2_PAIR_TERM(1, qh, 1)
#if D3DP_ATTN_KPIPE
    __builtin_amdgcn_sched_barrier(0);
    if (t + 2 < NKT) { read_lo(t + 2, kc[0]); read_lo(t + 3, kc[1]); }
    __builtin_amdgcn_sched_barrier(0);
#endif
    X2_PAIR_TERM(2, ql, 0)
    X2_PAIR_TERM(3, ql, 1)
    X2_PAIR_TERM(2, qh, 0)
    X2_PAIR_TERM(3, qh, 1)
#if D3DP_ATTN_KPIPE
    __builtin_amdgcn_sched_barrier(0);
    if (t + 2 < NKT) { read_hi(t + 2, kc[0]); read_hi(t + 3, kc[1]); }
    __builtin_amdgcn_sched_barrier(0);
#endif
    s0[t] = a0; s0[t + 1] = b0; s1[t] = a1; s1[t + 1] = b1;
  }
#undef X2_PAIR_TERM
  softmax_split_x2<NKT, MASK_ANY_TILE>(s0, n, lane, ph[0], pl[0], denom[0], cexp);
  softmax_split_x2<NKT, MASK_ANY_TILE>(s1, n, lane, ph[1], pl[1], denom[1], cexp);
}

// Head dims 32 and 16: the same two functions with ONE K fragment per plane and key tile (fb.k0; tile t 16 rows of 2 HD bytes
// further) and one MFMA per pass: a key-tile pair is 4 fragment reads and 6 MFMAs (12 for the two query tiles of a wave), a
// quarter / an eighth of the LDS bytes of head dim 64.  The compiler places the reads; a scheduling barrier every two pairs bounds
// how far it hoists them.
template <int HD, int NKT, bool MASK_ANY_TILE>
__device__ __forceinline__ void attn_scores_x2_hd(const FragBasesT<HD>& fb, int plane, const typename X2Head<HD>::frag& qh,
                                                  const typename X2Head<HD>::frag& ql, int n, int lane, f16x8 (&ph)[NKT / 2],
                                                  f16x8 (&pl)[NKT / 2], float& denom, float cexp) {
  typedef typename X2Head<HD>::frag frag;
  constexpr int TILE = 16 * X2Head<HD>::ROWB;
  f32x4 s[NKT];
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    const frag kl = *reinterpret_cast<const frag*>(fb.k0 + plane + t * TILE);
    const frag kh = *reinterpret_cast<const frag*>(fb.k0 + t * TILE);
    s[t] = x2_tile_scores(kh, kl, qh, ql);
    if ((t & 3) == 3) __builtin_amdgcn_sched_barrier(0);
  }
  softmax_split_x2<NKT, MASK_ANY_TILE>(s, n, lane, ph, pl, denom, cexp);
}
template <int HD, int NKT, bool MASK_ANY_TILE>
__device__ __forceinline__ void attn_scores_x2_pair_hd(const FragBasesT<HD>& fb, int plane, const typename X2Head<HD>::frag (&qh)[2],
                                                       const typename X2Head<HD>::frag (&ql)[2], int n, int lane,
                                                       f16x8 (&ph)[2][NKT / 2], f16x8 (&pl)[2][NKT / 2], float (&denom)[2],
                                                       float cexp) {
  typedef typename X2Head<HD>::frag frag;
  constexpr int TILE = 16 * X2Head<HD>::ROWB;
  f32x4 s0[NKT], s1[NKT];
#pragma unroll
  for (int t = 0; t < NKT; t += 2) {
    const frag kla = *reinterpret_cast<const frag*>(fb.k0 + plane + t * TILE);
    const frag klb = *reinterpret_cast<const frag*>(fb.k0 + plane + (t + 1) * TILE);
    const frag kha = *reinterpret_cast<const frag*>(fb.k0 + t * TILE);
    const frag khb = *reinterpret_cast<const frag*>(fb.k0 + (t + 1) * TILE);
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, b0 = a0, a1 = a0, b1 = a0;   // four independent chains, as above
#define X2_PAIR_TERM_HD(KA, KB, Q)                                  \
    a0 = Op2<f16>::mfma(KA, Q[0], a0); b0 = Op2<f16>::mfma(KB, Q[0], b0); \
    a1 = Op2<f16>::mfma(KA, Q[1], a1); b1 = Op2<f16>::mfma(KB, Q[1], b1);
    X2_PAIR_TERM_HD(kla, klb, qh)
    X2_PAIR_TERM_HD(kha, khb, ql)
    X2_PAIR_TERM_HD(kha, khb, qh)
#undef X2_PAIR_TERM_HD
    s0[t] = a0; s0[t + 1] = b0; s1[t] = a1; s1[t + 1] = b1;
    if ((t & 3) == 2) __builtin_amdgcn_sched_barrier(0);
  }
  softmax_split_x2<NKT, MASK_ANY_TILE>(s0, n, lane, ph[0], pl[0], denom[0], cexp);
  softmax_split_x2<NKT, MASK_ANY_TILE>(s1, n, lane, ph[1], pl[1], denom[1], cexp);
}

// temporal axis: PERSISTENT workgroups (one per CU: the four planes of 256 keys fill 128 KiB of LDS), 8 waves, each wave
// TPW = 1 or 2 16-query tiles of the current (sequence, head) problem (two waves per SIMD -> 256 registers per wave:
// the score row, the probabilities of both tiles and the prefetched queries of the next problem all stay in registers).
// K and V arrive by LDS-DMA straight from the packed qkv rows (8 rows x 128 B per wave-instruction, the image swizzle
// applied on the global side; 16 rows x 64 B at head dim 32, 32 rows x 32 B at 16, where the images are a half / a quarter of
// that and more workgroups share a CU: launch_temporal_x2) and are double-buffered in TIME, not in space:
//     K(p+1) streams in while problem p multiplies P.V,   V(p+1) while problem p+1 computes its scores.
//   top:  vmcnt(V pieces) -> K(p), q(p) landed        barrier 1     scores + softmax
//         vmcnt(0)        -> V(p) landed              barrier 2     (every wave is done with the K image)  issue K(p+1)
//         P.V (q(p+1) requested on the way), store O  barrier 3     (every wave is done with the V image)  issue V(p+1)
// The vmcnt(2 PER) at the top is exact: vector memory operations of a wave retire in order and the 2 PER youngest are
// the V pieces.
// measurement build (-DD3DP_ATTN_STAMP=1): s_memtime at the phase boundaries of the first 16 problems of workgroups 0..3,
// every wave's lane 0 -> d3dp_attn_stamps[wg][wave][problem][8] (read back by d3dp_debug_attn_stamps)
#if D3DP_ATTN_STAMP
__device__ unsigned long long d3dp_attn_stamps[4 * 8 * 16 * 8];
#define ATTN_STAMP(k)                                                                                          \
  do {                                                                                                         \
    if (blockIdx.x < 4 && iter < 16 && lane == 0)                                                              \
      d3dp_attn_stamps[((blockIdx.x * 8 + wave) * 16 + iter) * 8 + (k)] = __builtin_readcyclecounter();        \
  } while (0)
#else
#define ATTN_STAMP(k) do { } while (0)
#endif
template <int NKT, int OUTS, bool MASK_ANY_TILE, int HD = 64>
__global__ __launch_bounds__(512) void attn_temporal_x2_kernel(const float* __restrict__ qkv, void* __restrict__ out_v,
                                                               SeqMap map, int C, int heads, size_t plane_elems,
                                                               int n_prob, X2Scales sc) {
  using H = X2Head<HD>;
  constexpr int NW = 8;
  constexpr int TPW = (NKT + NW - 1) / NW;             // query tiles per wave
  constexpr int NK = 16 * NKT;
  constexpr int PLANE = NK * H::ROWB;
  constexpr int NPC = PLANE / 1024;                    // DMA pieces of a plane (1 KiB each): 2 NKT at head dim 64, NKT, NKT / 2
  constexpr int PER = (NPC + NW - 1) / NW;             // DMA pieces per wave and plane
  constexpr int ND = HD / 16;                          // channel tiles of O^T
  __shared__ __attribute__((aligned(16))) char kimg[2 * PLANE];
  __shared__ __attribute__((aligned(16))) char vimg[2 * PLANE];
  const int n = map.n_tok;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ts = map.tok_stride;
  const size_t ldb = (size_t)12 * C;                   // bytes per packed token row
  const int n_qt = (n + 15) >> 4;
  const float inv_scale = sc.onorm;                    // O^T is scaled by (v scale) x 1024, the denominator by 1024

  // DMA piece `pc` of a plane = image rows 8 pc .. 8 pc + 7; a lane moves the 16-byte slot that belongs at position
  // (lane & 7) of row 8 pc + (lane >> 3): K slot s sits at s ^ ((row >> 1) & 7), V slot s at s ^ (((row >> 1) & 3) << 1)
  // (head dim 64.  In general a piece is 64 >> LS rows of 2^LS slots under the swizzles of attn_frag.h, and every slot a lane
  // asks for lies inside its head's 2 HD bytes of the plane)
  auto problem_row0 = [&](int p, int& head) -> const char* {
    const int seq = p / heads;
    head = p - seq * heads;
    return reinterpret_cast<const char*>(qkv) + (size_t)ta_seq_base(map, seq) * ldb;
  };
  // (per-lane source offsets are re-derived at every use from a copy of the lane id the compiler cannot see through:
  // hoisted out of the problem loop they are ~40 live registers, which spills -- and scratch traffic shares vmcnt)
  auto opaque = [](int x) { asm volatile("" : "+v"(x)); return x; };
  auto issue_kv = [&](const char* row0, int head, int is_v) {
    const int l = opaque(lane);
    const char* g = row0 + (is_v ? 8 : 4) * C + head * H::ROWB;
    char* img = is_v ? vimg : kimg;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int pc = min(wave + j * NW, NPC - 1);      // (surplus pieces repeat the last one: same bytes, same place)
      const int row = pc * (64 >> H::LS) + (l >> H::LS);
      const int sw = is_v ? v_slot_swizzle<HD>(row) : k_slot_swizzle<HD>(row);
      // rows >= n: a copy of the last row (finite values; their scores are masked, their probabilities are 0)
      const char* gj = g + (unsigned)(min(row, n - 1) * ts) * (unsigned)ldb + (((l & ((1 << H::LS) - 1)) ^ sw) << 4);
      lds_dma16(gj, img + pc * 1024);
      lds_dma16(gj + 2 * C, img + PLANE + pc * 1024);
    }
  };
  // raw query fragments of the next problem.  (Not zero-initialised on purpose: the compiler would place the zeroing of
  // the lanes / tiles that load nothing right behind the untracked loads, inside their in-flight window, which the ISA scan
  // of tests/test_abi.py forbids.  A wave whose second tile does not exist -- 129..240 frames -- runs the paired score path
  // on whatever these registers hold and never stores the result.)
  f32x4 qr[TPW][H::NQL];
  auto load_q_raw = [&](const char* row0, int head) {
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
      const int qt = wave + u * NW;
      // (head dims 32 and 16: every wave loads, for every tile and, behind the last problem, once more from the rows of that
      // problem -- row min(q, n - 1) always exists.  Branch-free, the loads sit in the loop body's own block, in front of the
      // counted wait in layout order too, which is how the ISA scan of tests/test_abi.py reads the kernel.)
      if (HD != 64 || qt < n_qt) {
        const int l = opaque(lane);
        const int q = qt * 16 + (l & 15);
        // (head dim 16: the lane's four values d = 4 fg .. 4 fg + 3, one load; 32: d = 8 fg .. + 7; 64: those and 32 further)
        const float* qrow = reinterpret_cast<const float*>(row0 + (size_t)min(q, n - 1) * ts * ldb) + head * HD + (l >> 4) * (HD == 16 ? 4 : 8);
        if constexpr (HD == 64) {
          qr[u][0] = gload16_untracked(qrow);
          qr[u][1] = gload16_untracked(qrow + 4);
          qr[u][2] = gload16_untracked(qrow + 32);
          qr[u][3] = gload16_untracked(qrow + 36);
        } else {
          gload16_untracked_into(qr[u][0], qrow);
          if constexpr (HD == 32) gload16_untracked_into(qr[u][1], qrow + 4);
        }
      }
    }
  };
  // (head dims 32 and 16) tile u's raw query registers -> its split fragments; called behind the counted wait
  [[maybe_unused]] auto split_q_raw = [&](int u, typename H::frag& qh, typename H::frag& ql) {
    if constexpr (HD == 32) {
      settle(qr[u][0]); settle(qr[u][1]);
      ta_split8(make_float4(qr[u][0][0], qr[u][0][1], qr[u][0][2], qr[u][0][3]),
                make_float4(qr[u][1][0], qr[u][1][1], qr[u][1][2], qr[u][1][3]), qh, ql, sc.q);
    } else if constexpr (HD == 16) {
      settle(qr[u][0]);
      x2_split4(qr[u][0], qh, ql, sc.q);
    }
  };

  int p = blockIdx.x;
  if (p >= n_prob) return;
  // waves w and w + 4 share a SIMD and run the same phases between the same barriers: the static priority lets one of
  // them take the matrix pipe first, after which its softmax (VALU) runs beside the other's MFMAs (measured: 563 vs
  // 568 ms per step without it -- within noise; starting odd workgroups half a problem late changed nothing either)
  if ((wave >> 2) & 1) __builtin_amdgcn_s_setprio(1);
  int head;
  const char* row0 = problem_row0(p, head);
  issue_kv(row0, head, 0);
  load_q_raw(row0, head);
  issue_kv(row0, head, 1);
  [[maybe_unused]] int iter = 0;
  for (;; ++iter) {
    ATTN_STAMP(0);
    wait_vmcnt<2 * PER>();
    ATTN_STAMP(1);
    __builtin_amdgcn_s_barrier();                      // 1: the K image of problem p is complete
    ATTN_STAMP(2);
    f16x8 ph[TPW][NKT / 2], pl[TPW][NKT / 2];
    float denom[TPW];
    // (fragment bases re-derived per phase from the opaque lane id: the four V bases are not live during the scores)
    const FragBasesT<HD> fbk = make_frag_bases<HD>(kimg, vimg, opaque(lane));
    // (D3DP_ATTN_OVERLAP not with per-element masks in every key tile -- 225..240 frames on 16 key tiles: their lane masks push
    //  the overlapped form past 256 registers; those lengths keep the paired form)
    constexpr bool OVL = HD == 64 && TPW == 2 && D3DP_ATTN_OVERLAP && !MASK_ANY_TILE;   // (the build switches: head dim 64 only)
    [[maybe_unused]] f32x4 s1[OVL ? NKT : 1];          // OVL: tile 1's masked score row, turned into probabilities during tile 0's P.V
    [[maybe_unused]] float nb1 = 0.f;
#if D3DP_ATTN_OVERLAP
    if constexpr (OVL) {
      f16x8 qh[2][2], ql[2][2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        float4 qf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          settle(qr[u][i]);                            // (after the counted wait above)
          qf[i] = make_float4(qr[u][i][0], qr[u][i][1], qr[u][i][2], qr[u][i][3]);
        }
        ta_split8(qf[0], qf[1], qh[u][0], ql[u][0], sc.q);
        ta_split8(qf[2], qf[3], qh[u][1], ql[u][1], sc.q);
      }
      f32x4 s0[NKT];
      f32x4 none_s[1];
      f16x8 none_p[1];
      float sum0[2] = {0.f, 0.f};
      x2_scores_rows<NKT, false>(fbk, PLANE, qh[0], ql[0], s0, none_s, 0.f, sc.cexp, none_p, none_p, sum0);
      const float nb0 = x2_mask_rowmax<NKT, MASK_ANY_TILE>(s0, n, lane, sc.cexp);
      // tile 1's scores (a wave without a second tile computes them on whatever its registers hold and never stores the
      // result) with tile 0's softmax between the MFMAs
      x2_scores_rows<NKT, true>(fbk, PLANE, qh[1], ql[1], s1, s0, nb0, sc.cexp, ph[0], pl[0], sum0);
      denom[0] = x2_denominator(sum0);
      nb1 = x2_mask_rowmax<NKT, MASK_ANY_TILE>(s1, n, lane, sc.cexp);
    } else
#endif
    if constexpr (HD != 64) {                            // (the same two cases as below, one fragment per tile and operand)
      if constexpr (TPW == 2) {
        typename H::frag qh[2], ql[2];
        split_q_raw(0, qh[0], ql[0]);
        split_q_raw(1, qh[1], ql[1]);
        attn_scores_x2_pair_hd<HD, NKT, MASK_ANY_TILE>(fbk, PLANE, qh, ql, n, lane, ph, pl, denom, sc.cexp);
      } else {
        denom[0] = 1.f;
        if (wave < n_qt) {
          typename H::frag qh, ql;
          split_q_raw(0, qh, ql);
          attn_scores_x2_hd<HD, NKT, MASK_ANY_TILE>(fbk, PLANE, qh, ql, n, lane, ph[0], pl[0], denom[0], sc.cexp);
        }
      }
    } else if constexpr (TPW == 2) {
      // both query tiles of the wave in one pass over K (a wave whose second tile does not exist computes it on whatever its
      // registers hold and never stores it: one code path, no second register allocation)
      f16x8 qh[2][2], ql[2][2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        float4 qf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          settle(qr[u][i]);                            // (after the counted wait above)
          qf[i] = make_float4(qr[u][i][0], qr[u][i][1], qr[u][i][2], qr[u][i][3]);
        }
        ta_split8(qf[0], qf[1], qh[u][0], ql[u][0], sc.q);
        ta_split8(qf[2], qf[3], qh[u][1], ql[u][1], sc.q);
      }
      attn_scores_x2_pair<NKT, MASK_ANY_TILE>(fbk, PLANE, qh, ql, n, lane, ph, pl, denom, sc.cexp);
    } else {                                           // one tile per wave (up to 128 keys)
      denom[0] = 1.f;
      if (wave < n_qt) {
        f16x8 qh[2], ql[2];
        float4 qf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          settle(qr[0][i]);                            // (after the counted wait above)
          qf[i] = make_float4(qr[0][i][0], qr[0][i][1], qr[0][i][2], qr[0][i][3]);
        }
        ta_split8(qf[0], qf[1], qh[0], ql[0], sc.q);
        ta_split8(qf[2], qf[3], qh[1], ql[1], sc.q);
        attn_scores_x2<NKT, MASK_ANY_TILE>(fbk, PLANE, qh, ql, n, lane, ph[0], pl[0], denom[0], sc.cexp);
      }
    }
    ATTN_STAMP(3);
    wait_vmcnt<0>();
    ATTN_STAMP(4);
    __builtin_amdgcn_s_barrier();                      // 2: V image complete; nobody reads the K image any more
    ATTN_STAMP(5);
    const int pn = p + gridDim.x;
    const bool has_next = pn < n_prob;
    int head_n = 0;
    const char* row0_n = row0;
    if (has_next) {
      row0_n = problem_row0(pn, head_n);
      issue_kv(row0_n, head_n, 0);
    }
    const int tok0 = ta_seq_base(map, p / heads);
    const FragBasesT<HD> fb = make_frag_bases<HD>(kimg, vimg, opaque(lane));
#if D3DP_ATTN_OVERLAP
    if constexpr (OVL) {                               // tile 0's P.V with tile 1's softmax between its MFMAs
      f32x4 o[4];
#pragma unroll
      for (int dn = 0; dn < 4; ++dn) o[dn] = (f32x4){0.f, 0.f, 0.f, 0.f};
      float sum1[2] = {0.f, 0.f};
      x2_pv_overlap<NKT>(fb, PLANE, ph[0], pl[0], o, s1, nb1, sc.cexp, ph[1], pl[1], sum1);
      denom[1] = x2_denominator(sum1);
      const int l = opaque(lane);
      const int q = wave * 16 + (l & 15);
      if (q < n)
        store_o_x2<OUTS>(o, inv_scale / denom[0], out_v, (size_t)(tok0 + q * ts), C, head * 64 + (l >> 4) * 4, sc.oplane);
    }
#endif
#pragma unroll
    for (int u = OVL ? 1 : 0; u < TPW; ++u) {
      // the next problem's queries: requested before the LAST tile's P.V (with two tiles the probabilities of both are
      // live during the first one's, and 32 more registers there would spill)
      if (u == TPW - 1 && (has_next || HD != 64)) load_q_raw(row0_n, head_n);   // (row0_n = row0, head 0 behind the last problem)
      const int qt = wave + u * NW;
      if (qt < n_qt) {
        f32x4 o[ND];
#pragma unroll
        for (int dn = 0; dn < ND; ++dn) o[dn] = (f32x4){0.f, 0.f, 0.f, 0.f};
        pv_chunks_x2<NKT, 0>(fb, PLANE, ph[u], pl[u], o);
        const int l = opaque(lane);
        const int q = qt * 16 + (l & 15);
        if (q < n)
          store_o_x2<OUTS>(o, inv_scale / denom[u], out_v, (size_t)(tok0 + q * ts), C, head * HD + (l >> 4) * 4, sc.oplane);
      }
    }
    if (!has_next) break;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    ATTN_STAMP(6);
    __builtin_amdgcn_s_barrier();                      // 3: nobody reads the V image any more
    ATTN_STAMP(7);
    issue_kv(row0_n, head_n, 1);
    p = pn; row0 = row0_n; head = head_n;
  }
}

// ------------------------------------------------------------------------------------------------
// Temporal axis of clips LONGER than 256 frames (reference common/arguments.py:58 `-f`; round 6).  The
// persistent kernel above holds the K and V images of a whole sequence in LDS (256 keys = 128 KiB) and forms a query's softmax
// over the complete score row; beyond 256 frames round 5 sent both attentions to the chunked fp32 VALU row kernel -- measured at
// F = 351: 53 % of the sampler's time, ten times the cost per FLOP of the 243-frame path.  Here: the flash form on the same
// split-fp16 operands and packed qkv rows.  A work unit = one (sequence, head) problem x one group of eight 16-query tiles (one
// per wave); the keys pass through LDS in chunks of 128 (K and V hi / lo images in the one-swizzle layout of ta_common.h: 64 KiB,
// two workgroups per CU) under an online softmax in base-2 units -- running row maximum, denominator and O^T per query in
// registers, rescaled whenever a key pair raises the maximum -- exactly the forward kernel of the training step
// (train_attn.hip tattn_fwd_kernel) with the key range cut into chunks and its operands taken from the packed rows: K and V are
// ALREADY split (the qkv Linear's epilogue), so staging is sixteen-byte copies, no arithmetic.  Any length up to the library's
// 1024 frames; results differ from the two-pass kernel only in the rounding of the rescaled partial sums (fp32-class either way).
// Head dims 32 and 16: the same loop on the K and V images of attn_frag.h (rows of 2 HD bytes, a swizzle each: K is only ever
// read by rows here and V only transposed, so the one-swizzle image that serves both, which the training step needs, buys
// nothing): 32 / 16 KiB of LDS, one K fragment per plane and tile, HD / 16 channel tiles.
template <int OUTS, int HD = 64>
__global__ __launch_bounds__(512) void attn_temporal_x2_long_kernel(const float* __restrict__ qkv, void* __restrict__ out_v,
                                                                    SeqMap map, int C, int heads, int groups, int n_work,
                                                                    X2Scales sc) {
  using H = X2Head<HD>;
  constexpr int NW = 8, NKC = 128, NKT = NKC / 16, PLANE = NKC * H::ROWB, ND = HD / 16;
  __shared__ __attribute__((aligned(16))) char kimg[2 * PLANE];
  __shared__ __attribute__((aligned(16))) char vimg[2 * PLANE];
  const int n = map.n_tok;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fi = lane & 15, fg = lane >> 4;
  const size_t ldb = (size_t)12 * C, rsb = (size_t)map.tok_stride * ldb;   // bytes per packed token row / between two tokens of a sequence
  using u32x4 = unsigned __attribute__((ext_vector_type(4)));
  // rows k0 .. k0 + NKC - 1 of one packed operand (byte offset `off` inside a row: hi plane; lo plane 2 C bytes further) -> its
  // hi / lo images; keys >= n: zero rows (their scores are masked, their probabilities 0: V must be finite there)
  [[maybe_unused]] auto stage = [&](const char* row0, int off, int k0, char* img) {   // (head dim 64)
#pragma unroll
    for (int i0 = 0; i0 < NKC * 8; i0 += 2 * 512) {
      u32x4 h[2], l[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int idx = i0 + u * 512 + tid, row = idx >> 3, slot = idx & 7;
        h[u] = (u32x4){0u, 0u, 0u, 0u}; l[u] = h[u];
        if (k0 + row < n) {
          const char* p = row0 + (size_t)(k0 + row) * rsb + off + slot * 16;
          h[u] = *reinterpret_cast<const u32x4*>(p);
          l[u] = *reinterpret_cast<const u32x4*>(p + 2 * C);
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int idx = i0 + u * 512 + tid, row = idx >> 3, slot = idx & 7;
        const int o = row * 128 + ((slot ^ ta_sw(row)) << 4);
        *reinterpret_cast<u32x4*>(img + o) = h[u];
        *reinterpret_cast<u32x4*>(img + PLANE + o) = l[u];
      }
    }
  };
  // head dims 32 and 16: a chunk's K and V planes are 1024 / 512 slots in all -- two per thread and plane pair (K slot `tid`, V slot
  // `tid`) at 32; one at 16, where waves 0..3 move K and waves 4..7 V.  All four loads of a thread are in flight before its stores.
  [[maybe_unused]] auto stage_hd = [&](const char* row0, int head, int k0) {
    constexpr int LS = H::LS;
    const int idx = HD == 32 ? tid : (tid & 255), row = idx >> LS, slot = idx & ((1 << LS) - 1);
    const bool second = tid >= 256;                      // (wave-uniform; head dim 16: this thread moves V)
    u32x4 r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (u32x4){0u, 0u, 0u, 0u};
    if (k0 + row < n) {
      const char* p = row0 + (size_t)(k0 + row) * rsb + head * H::ROWB + slot * 16;
      if constexpr (HD == 32) {
        r[0] = *reinterpret_cast<const u32x4*>(p + 4 * C);
        r[1] = *reinterpret_cast<const u32x4*>(p + 6 * C);
        r[2] = *reinterpret_cast<const u32x4*>(p + 8 * C);
        r[3] = *reinterpret_cast<const u32x4*>(p + 10 * C);
      } else {
        p += second ? 8 * C : 4 * C;
        r[0] = *reinterpret_cast<const u32x4*>(p);
        r[1] = *reinterpret_cast<const u32x4*>(p + 2 * C);
      }
    }
    const int ko = row * H::ROWB + ((slot ^ k_slot_swizzle<HD>(row)) << 4), vo = row * H::ROWB + ((slot ^ v_slot_swizzle<HD>(row)) << 4);
    if constexpr (HD == 32) {
      *reinterpret_cast<u32x4*>(kimg + ko) = r[0];
      *reinterpret_cast<u32x4*>(kimg + PLANE + ko) = r[1];
      *reinterpret_cast<u32x4*>(vimg + vo) = r[2];
      *reinterpret_cast<u32x4*>(vimg + PLANE + vo) = r[3];
    } else {
      char* img = second ? vimg + vo : kimg + ko;
      *reinterpret_cast<u32x4*>(img) = r[0];
      *reinterpret_cast<u32x4*>(img + PLANE) = r[1];
    }
  };
  [[maybe_unused]] const TAFrag fk = ta_frag(kimg, lane), fv = ta_frag(vimg, lane);   // (head dim 64)
  [[maybe_unused]] const FragBasesT<HD> fb = make_frag_bases<HD>(kimg, vimg, lane);   // (head dims 32 and 16)
  for (int unit = blockIdx.x; unit < n_work; unit += gridDim.x) {
    const int prob = unit / groups, group = unit - prob * groups;
    const int seq = prob / heads, head = prob - seq * heads;
    const int tok0 = ta_seq_base(map, seq);
    const char* row0 = reinterpret_cast<const char*>(qkv) + (size_t)tok0 * ldb;
    const int qt = group * NW + wave;
    const bool active = qt * 16 < n;                     // (wave-uniform)
    const int q = qt * 16 + fi;
    typename H::frag qh[H::NQ], ql[H::NQ];
    if (active) {
      const float* qrow = reinterpret_cast<const float*>(row0 + (size_t)min(q, n - 1) * rsb) + head * HD;
      if constexpr (HD == 64) ta_load_row_op(qrow, fg, sc.q, qh, ql);
      else load_q_x2<HD>(qrow, fg, qh, ql, sc.q);
    }
    float mrun = -INFINITY, lrun = 0.f;                  // running row maximum (base-2 logit units), 1024 x running denominator
    f32x4 o[ND];
#pragma unroll
    for (int dn = 0; dn < ND; ++dn) o[dn] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < n; k0 += NKC) {
      __syncthreads();                                   // every wave is done with the previous chunk's (or unit's) images
      if constexpr (HD == 64) {
        stage(row0, 4 * C + head * 128, k0, kimg);
        stage(row0, 8 * C + head * 128, k0, vimg);
      } else {
        stage_hd(row0, head, k0);
      }
      __syncthreads();
      if (!active) continue;
#pragma unroll
      for (int t = 0; t < NKT; t += 2) {
        if (k0 + 16 * t >= n) break;                     // (uniform: the rest of the chunk lies behind the sequence)
        f32x4 a, b;
        if constexpr (HD == 64) {
          ta_rows_pair<PLANE>(fk, t, qh, ql, a, b);      // S^T [key][query], raw: x sc.cexp = logits in base-2 units
        } else {
          typedef typename H::frag frag;
          constexpr int TILE = 16 * H::ROWB;
          const frag kla = *reinterpret_cast<const frag*>(fb.k0 + PLANE + t * TILE), kha = *reinterpret_cast<const frag*>(fb.k0 + t * TILE);
          const frag klb = *reinterpret_cast<const frag*>(fb.k0 + PLANE + (t + 1) * TILE), khb = *reinterpret_cast<const frag*>(fb.k0 + (t + 1) * TILE);
          a = x2_tile_scores(kha, kla, qh[0], ql[0]);
          b = x2_tile_scores(khb, klb, qh[0], ql[0]);
        }
        float sv[8];
#pragma unroll
        for (int r = 0; r < 4; ++r) { sv[r] = a[r] * sc.cexp; sv[4 + r] = b[r] * sc.cexp; }
        if (k0 + 16 * (t + 2) > n) {                     // (uniform: only the sequence's last pair holds keys >= n)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (k0 + 16 * t + 4 * fg + r >= n) sv[r] = -INFINITY;
            if (k0 + 16 * (t + 1) + 4 * fg + r >= n) sv[4 + r] = -INFINITY;
          }
        }
        float mx = sv[0];
#pragma unroll
        for (int e = 1; e < 8; ++e) mx = fmaxf(mx, sv[e]);
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mnew = fmaxf(mrun, mx);              // (finite from the first pair on: key 0 exists)
        const float alpha = __builtin_amdgcn_exp2f(mrun - mnew);
        mrun = mnew;
        float psum = 0.f;
        f16x8 ph, pl;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float y = __builtin_amdgcn_exp2f(sv[e] - mnew + 10.0f);   // p x 1024
          psum += y;
          const f16 hh = (f16)y;
          ph[e] = hh;
          pl[e] = (f16)fmaf(y, 1.0f, -(float)hh);
        }
        psum += __shfl_xor(psum, 16, 64);
        psum += __shfl_xor(psum, 32, 64);
        lrun = fmaf(lrun, alpha, psum);
#pragma unroll
        for (int dn = 0; dn < ND; ++dn) o[dn] *= alpha;
        if constexpr (HD == 64) {
          ta_tr_chunk<PLANE>(fv, t >> 1, ph, pl, o);     // O^T[d][query] += V^T P^T
        } else {
          FragBasesT<HD> fc = fb;                        // (key chunk t / 2: 32 rows further)
#pragma unroll
          for (int dn = 0; dn < ND; ++dn) fc.v[dn] += (t >> 1) * 32 * H::ROWB;
          pv_chunk_x2_seq<0>(fc, PLANE, ph, pl, o);
        }
      }
    }
    // o = (v scale) x 1024 x sum_j p_j v_j against the running maximum; lrun = 1024 x sum_j p_j
    if (active && q < n)
      store_o_x2<OUTS>(o, sc.onorm / lrun, out_v, (size_t)(tok0 + q * map.tok_stride), C, head * HD + fg * 4, sc.oplane);
  }
}

// spatial axis (<= 32 tokens per sequence): one WAVE per (sequence, head).  The K fragments of its two 16-key tiles are
// loaded straight from the packed rows into the MFMA operand layout (lane (key, g) <- 2 x 16 contiguous bytes of each K
// plane); only V goes through LDS (its fragments are transposed reads): a private 8 KiB image (V hi, V lo: 32 rows x
// 128 B each), so a 256-thread workgroup needs 32 KiB and five of them fit a CU -- this kernel is latency / HBM-bound
// (8 KB per token), and with K staged as well (16 KiB per wave, two workgroups per CU) it ran at 3.8 TB/s.
// Head dims 32 and 16: one K fragment per plane and tile (8 bytes per lane at 16), V images of 64- / 32-byte rows: 16 / 8 KiB per
// workgroup, so the registers and the 2048 threads of a CU bound the occupancy, not the LDS.
template <int OUTS, int HD = 64>
__global__ __launch_bounds__(256) void attn_spatial_x2_kernel(const float* __restrict__ qkv, void* __restrict__ out_v,
                                                              int n_prob, SeqMap map, int C, int heads, size_t plane_elems,
                                                              X2Scales sc) {
  using H = X2Head<HD>;
  constexpr int PLANE = 32 * H::ROWB, NQ = H::NQ, ND = HD / 16;
  __shared__ __attribute__((aligned(16))) char smem[4 * 2 * PLANE];
  const int n = map.n_tok;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pid = blockIdx.x * 4 + wave;
  if (pid >= n_prob) return;
  const int seq = pid / heads, head = pid % heads;
  const int base = ta_seq_base(map, seq);
  const int ts = map.tok_stride;
  const size_t ldb = (size_t)12 * C;                   // bytes per packed token row: q fp32 | k hi | k lo | v hi | v lo
  const char* rows = reinterpret_cast<const char*>(qkv) + (size_t)base * ldb;
  char* img = smem + wave * 2 * PLANE;
  const int fi = lane & 15, fg = lane >> 4;
  const int n_qt = (n + 15) >> 4;
  // every global request of the problem is issued before anything is consumed: both query tiles, both key tiles, V
  typename H::frag qh[2][NQ], ql[2][NQ], kh[2][NQ], kl[2][NQ];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const char* row = rows + (size_t)min(t * 16 + fi, n - 1) * ts * ldb;
    load_q_x2<HD>(reinterpret_cast<const float*>(row) + head * HD, fg, qh[t], ql[t], sc.q);
    load_k_x2<HD>(reinterpret_cast<const f16*>(row + 4 * C) + head * HD, C, fg, kh[t], kl[t]);
  }
  for (int idx = lane; idx < (32 << H::LS); idx += 64) {   // V rows -> hi / lo images (rows >= n zeroed)
    const int row = idx >> H::LS, slot = idx & ((1 << H::LS) - 1);
    f16x8 vh = {}, vl = {};
    if (row < n) {
      const f16* src = reinterpret_cast<const f16*>(rows + (size_t)row * ts * ldb + 8 * C) + head * HD + slot * 8;
      vh = *reinterpret_cast<const f16x8*>(src);
      vl = *reinterpret_cast<const f16x8*>(src + C);
    }
    const int vo = row * H::ROWB + ((slot ^ v_slot_swizzle<HD>(row)) << 4);
    *reinterpret_cast<f16x8*>(img + vo) = vh;
    *reinterpret_cast<f16x8*>(img + PLANE + vo) = vl;
  }
  const FragBasesT<HD> fb = make_frag_bases<HD>(img, img, lane);   // only the V bases are used
  // (wave-private LDS image: the LDS pipe executes one wave's accesses in order, no barrier needed)
  const float inv_scale = sc.onorm;                    // O^T is scaled by (v scale) x 1024, `sum` by 1024
  const float cexp = sc.cexp;
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    if (qt >= n_qt) break;
    const int q = qt * 16 + fi;
    f32x4 s[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {                      // S^T tile t: keys 16 t + 4 fg + r, query fi
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      if constexpr (HD == 64) {
        a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kl[t][0], qh[qt][0], a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kl[t][1], qh[qt][1], a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh[t][0], ql[qt][0], a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh[t][1], ql[qt][1], a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh[t][0], qh[qt][0], a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh[t][1], qh[qt][1], a, 0, 0, 0);
      } else {
        a = x2_tile_scores(kh[t][0], kl[t][0], qh[qt][0], ql[qt][0]);
      }
      s[t] = a;
    }
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (16 * t + 4 * fg + r >= n) s[t][r] = -INFINITY;
        mx = fmaxf(mx, s[t][r]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float nb = fmaf(-mx, cexp, 10.0f);          // p * 1024 = exp2(s cexp - mx cexp + 10), as attn_scores_x2
    float sum = 0.f;
    f16x8 ph[1], pl[1];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float y = __builtin_amdgcn_exp2f(fmaf(s[t][r], cexp, nb));
        sum += y;
        const f16 h = (f16)y;
        ph[0][t * 4 + r] = h;
        pl[0][t * 4 + r] = (f16)fmaf(y, 1.0f, -(float)h);
      }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    f32x4 o[ND];
#pragma unroll
    for (int dn = 0; dn < ND; ++dn) o[dn] = (f32x4){0.f, 0.f, 0.f, 0.f};
    pv_chunk_x2_seq<0>(fb, PLANE, ph[0], pl[0], o);
    if (q < n) store_o_x2<OUTS>(o, inv_scale / sum, out_v, (size_t)(base + q * ts), C, head * HD + fg * 4, sc.oplane);
  }
}

// fp32 qkv rows [T, 3C] -> the packed rows of the split-fp16 attention kernels (what the qkv Linear writes directly with
// EPI_QKV_PACK); used by d3dp_op_attention, whose C-ABI input is the plain fp32 layout.
__global__ void qkv_pack_x2_kernel(const float* __restrict__ src, char* __restrict__ dst, size_t T, int C, float sc) {
  const size_t total = T * (size_t)(3 * C / 4);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t t = i / (3 * C / 4);
    const int c = (int)(i - t * (3 * C / 4)) * 4, region = c / C, cn = c - region * C;
    const float4 v = *reinterpret_cast<const float4*>(src + t * 3 * C + c);
    char* row = dst + t * 12 * C;
    if (region == 0) {
      *reinterpret_cast<float4*>(row + cn * 4) = v;
    } else {
      const float a[4] = {v.x, v.y, v.z, v.w};
      f16x4 ph, pl;
#pragma unroll
      for (int e = 0; e < 4; ++e) { f16 h, l; split2h_scaled(a[e] * sc, h, l); ph[e] = h; pl[e] = l; }
      *reinterpret_cast<f16x4*>(row + region * 4 * C + cn * 2) = ph;
      *reinterpret_cast<f16x4*>(row + region * 4 * C + 2 * C + cn * 2) = pl;
    }
  }
}

// Resident workgroups per CU of a persistent kernel at head dims 32 and 16.  At head dim 64 the images decide (one 128 KiB
// workgroup of the 256-key kernel, two of 64 KiB); a half- or quarter-size image leaves that to the registers (a 512-thread
// workgroup is two waves per SIMD: floor(floor(512 / registers) / 2) of them) and the CU's 2048 threads, and a persistent grid
// larger than what is resident would run its surplus workgroups as a second, mostly idle round.  The runtime does that
// arithmetic on the compiled kernel; `at_most` (the LDS and thread bound) stands where it gives no answer.
template <typename K>
int x2_resident_per_cu(K kern, int threads, int at_most) {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(kern), threads, 0) != hipSuccess) {
    (void)hipGetLastError();
    return at_most;
  }
  return nb < 1 ? 1 : nb < at_most ? nb : at_most;
}

template <int NKT, int OUTS, int HD>
int launch_temporal_x2(const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads, size_t plane, X2Scales sc,
                       hipStream_t st) {
  constexpr int NK = 16 * NKT;
  const size_t lds = (size_t)NK * X2Head<HD>::ROWB * 4;   // static LDS of the kernel (K and V images, two planes each)
  constexpr int NW = 8;
  // (n inside the last key tile -- F = 243, 27 -- needs masking in that tile only)
  const bool last_only = map.n_tok > 16 * (NKT - 1);
  auto kern = last_only ? attn_temporal_x2_kernel<NKT, OUTS, false, HD> : attn_temporal_x2_kernel<NKT, OUTS, true, HD>;
  static PerDeviceOnce once[2];                        // (head dims 32 and 16: per kernel, their register counts differ)
  const int n_wg = once[HD == 64 || last_only].get([&](int dev) {
    int per_cu = (int)((160 * 1024) / lds) < 2048 / (NW * 64) ? (int)((160 * 1024) / lds) : 2048 / (NW * 64);
    if constexpr (HD != 64) per_cu = x2_resident_per_cu(kern, NW * 64, per_cu);
    const int cus = d3dp_cu_count(dev);
    return cus < 0 ? cus : cus * per_cu;               // persistent: as many workgroups as fit the chip
  });
  if (n_wg < 0) return -3;
  const int n_prob = n_seq * heads;
#if D3DP_ATTN_W16
  if constexpr (NKT == 16 && HD == 64) {
    if (map.n_tok > 16 * (NKT - 1)) {
      hipLaunchKernelGGL((attn_temporal_x2_w16_kernel<OUTS>), dim3(n_prob < n_wg ? n_prob : n_wg), dim3(1024), 0, st,
                         (const float*)qkv, out, map, C, heads, plane, n_prob, sc);
      return 0;
    }
  }
#endif
  hipLaunchKernelGGL(kern, dim3(n_prob < n_wg ? n_prob : n_wg), dim3(NW * 64), 0, st, (const float*)qkv, out, map, C,
                     heads, plane, n_prob, sc);
  return 0;
}

// one head dim's three kernels: axis 0 with <= 32 tokens per sequence: one wave per problem; otherwise the persistent
// whole-sequence kernel (<= 256 tokens) or the chunked-key form (longer)
template <int HD>
int launch_attn_x2_hd(int act, int axis, const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads, float act_scale,
                      hipStream_t st, int hd_true) {
  const size_t plane = (size_t)n_seq * map.n_tok * C;
  const int n = map.n_tok;
  // (padded heads: the columns hd_true .. HD - 1 of every head are exact zeros in q, k and v, and the exponent is the true head dim's)
  const float rsq = hd_true > 0 && hd_true != HD ? (float)(1.0 / sqrt((double)hd_true))
                                                 : (HD == 64 ? 0.125f : HD == 32 ? 0.17677669529663689f : 0.25f);
  const X2Scales sc = {act_scale, rsq * 1.44269504088896340736f / (act_scale * act_scale),
                       1.0f / act_scale, act_scale};   // cexp: hd^-0.5 log2(e) / (q scale x k scale)
  if (axis == 0 && n <= 32) {                          // (more than 32 joints: the kernels below take any SeqMap)
    const int n_prob = n_seq * heads;
    if (act == 3) hipLaunchKernelGGL((attn_spatial_x2_kernel<2, HD>), dim3((n_prob + 3) / 4), dim3(256), 0, st, (const float*)qkv, out, n_prob, map, C, heads, plane, sc);
    else hipLaunchKernelGGL((attn_spatial_x2_kernel<0, HD>), dim3((n_prob + 3) / 4), dim3(256), 0, st, (const float*)qkv, out, n_prob, map, C, heads, plane, sc);
    return 0;
  }
  if (n > 256) {                                       // long clips: keys in chunks of 128 under an online softmax (see the kernel)
    const int groups = ((n + 15) / 16 + 7) / 8, n_work = n_seq * heads * groups;
    static PerDeviceOnce once[2];                      // (per kernel: act 0 / act 3)
    const int wgs = once[act == 3].get([&](int dev) {
      const int cus = d3dp_cu_count(dev);
      int per_cu = 2;                                  // head dim 64: two 64 KiB workgroups per CU
      if constexpr (HD != 64)                          // 32 / 16 KiB: the registers and the CU's 2048 threads decide
        per_cu = act == 3 ? x2_resident_per_cu(attn_temporal_x2_long_kernel<2, HD>, 512, 4) : x2_resident_per_cu(attn_temporal_x2_long_kernel<0, HD>, 512, 4);
      return cus < 0 ? cus : cus * per_cu;
    });
    if (wgs < 0) return -3;
    const dim3 grid(n_work < wgs ? n_work : wgs), blk(512);
    if (act == 3) hipLaunchKernelGGL((attn_temporal_x2_long_kernel<2, HD>), grid, blk, 0, st, (const float*)qkv, out, map, C, heads, groups, n_work, sc);
    else hipLaunchKernelGGL((attn_temporal_x2_long_kernel<0, HD>), grid, blk, 0, st, (const float*)qkv, out, map, C, heads, groups, n_work, sc);
    return 0;
  }
#define X2_CASE(NKT_)                                                                                         \
  return act == 3 ? launch_temporal_x2<NKT_, 2, HD>(qkv, out, n_seq, map, C, heads, plane, sc, st)            \
                  : launch_temporal_x2<NKT_, 0, HD>(qkv, out, n_seq, map, C, heads, plane, sc, st);
  if (n <= 32) { X2_CASE(2) }
  if (n <= 64) { X2_CASE(4) }
  if (n <= 128) { X2_CASE(8) }
  X2_CASE(16)
#undef X2_CASE
}

}  // namespace

// EXACT-mode attention on the fp16 matrix cores (split-fp16 operands; head dim 64, 32 or 16) over PACKED qkv rows (see above).
// act 0 -> fp32 out, 3 -> two fp16 planes out (the EXACT Linear's operand format).  axis 0 with <= 32 tokens per sequence:
// one wave per problem; otherwise the persistent whole-sequence kernel (<= 256 tokens) or the chunked-key form (longer).
void d3dp_launch_qkv_pack_x2(const float* src, void* dst, size_t T, int C, float act_scale, hipStream_t st) {
  const size_t total = T * (size_t)(3 * C / 4);
  const unsigned blocks = (unsigned)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  hipLaunchKernelGGL(qkv_pack_x2_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, st, src, (char*)dst, T, C, act_scale);
}

// act_scale: the power of two q, k, v (and, for act == 3, the output planes) are scaled by -- kActScale unless the block's
// proven operand range asked for less (capi_weights.hip).  With 16 the arithmetic is bit for bit that of the constant-scale kernels.
int d3dp_launch_attn_x2(int act, int axis, const void* qkv, void* out, int n_seq, SeqMap map, int C, int heads,
                        float act_scale, hipStream_t st, int hd_true) {
  if (heads < 1 || C % heads || map.n_tok < 1 || (act != 0 && act != 3) || !(act_scale > 0.f) || hd_true < 0 || hd_true > C / heads) return -2;
  switch (C / heads) {
    case 64: return launch_attn_x2_hd<64>(act, axis, qkv, out, n_seq, map, C, heads, act_scale, st, hd_true);
    case 32: return launch_attn_x2_hd<32>(act, axis, qkv, out, n_seq, map, C, heads, act_scale, st, hd_true);
    case 16: return launch_attn_x2_hd<16>(act, axis, qkv, out, n_seq, map, C, heads, act_scale, st, hd_true);
  }
  return -2;
}

#if D3DP_ATTN_STAMP
extern "C" __attribute__((visibility("default"))) int d3dp_debug_attn_stamps(unsigned long long* dst) {
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(d3dp_attn_stamps), sizeof(unsigned long long) * 4 * 8 * 16 * 8);
}
#endif
