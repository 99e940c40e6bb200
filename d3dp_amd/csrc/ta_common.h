// Device helpers shared by the split-fp16 attention kernels that keep their K / V (Q / dO) operands as hi / lo IMAGES in LDS under
// ONE swizzle serving row reads and transposed reads alike: the training step's attention (train_attn.hip) and the long-clip
// temporal attention of inference (attention_x2.hip, attn_temporal_x2_long_kernel: more than 256 frames).  ta_seq_base, ta_split8
// and v4bf16_t are the one definition for every attention source (attention_f32.hip, attention_fast.hip, attn_frag.h too).
// LDS image of a [n][64] matrix: two planes (hi | lo) of 128-byte rows, 16-byte slot s of row r at s ^ (((r >> 1) & 3) << 1) --
// conflict-free for the transposed fragment reads (ds_read_b64_tr_b16: 4 rows x 32 B per 16 lanes) AND for the row fragment
// reads (ds_read_b128, whose lane groups pair rows {0-3, 12-15} of one slot with rows {4-11} of the neighbouring one).
//
// Head dims 32 and 16 (HD is a template parameter that defaults to 64; the HD = 64 forms are the expressions the images were first
// written with, and attention_x2.hip's long-clip kernel uses only those).  A row is 2 HD bytes = HD / 8 slots, so the 256-byte bank
// row all three reads bank on ((addr / 4) mod 64) holds 4 / 8 rows.  attn_frag.h keeps a K swizzle (row reads) and a V swizzle
// (transposed reads) per head dim; the training kernels read ONE image both ways, so one swizzle has to serve both:
//   HD = 32 (64-byte rows, 4 slots): slot ^= ((row >> 2) & 1) << 1 -- attn_frag.h's V swizzle.
//     Transposed read (a 32-lane half = 8 rows 8h .. 8h + 7, the 32-byte chunk dn = slots 2 dn, 2 dn + 1 of each): rows r and r + 4
//     share a quarter (64 bytes) of a bank row; the XOR on the slot's HIGH bit sends them to different 32-byte chunks of it, so the
//     eight rows cover 8 x 32 = 256 different bytes.  (The low bit is untouched: a lane's 8 bytes stay at (qd & 1) 8 of slot qd >> 1.)
//     Row read (ds_read_b128, lane (fi, fg) reads slot fg of row fi): a 16-lane group holds, per quarter of the bank row, rows r
//     and r + 12 at one fg and rows r + 4 and r + 8 at fg ^ 1 (r = 0 .. 3).  The XOR is 0 for r and r + 8, 2 for r + 4 and r + 12:
//     slots {fg, fg ^ 2, fg ^ 3, fg ^ 1} -- four different ones.  (attn_frag.h's K swizzle, ((row >> 3) & 1) << 1, gives the same
//     set for the row read but leaves rows r and r + 4 of a transposed half on one chunk: 2-way.)
//   HD = 16 (32-byte rows, 2 slots): slot ^= (row >> 3) & 1 -- attn_frag.h's K swizzle.
//     Row read (ds_read_b64 of the 8 bytes d = 4 fg .. 4 fg + 3, banked per 32-lane half): a half reads slot fg >> 1 of rows 0 .. 15;
//     rows r and r + 8 share an eighth (32 bytes) of the bank row and the XOR puts them on its two different slots.
//     Transposed read: the 8 rows of a half are one whole bank row, every byte of it read once whichever way a row's two slots are
//     ordered (the XOR is uniform over rows 8h .. 8h + 7); the lane's address carries the XOR: slot (qd >> 1) ^ sw, byte (qd & 1) 8.
//   Both computed with the bank rule above for every lane group of both tiles / both halves of a chunk: 1 address per bank.  Not
//   confirmed with the SQ_LDS_BANK_CONFLICT counter; a conflict would cost time, not correctness.
// Every swizzle has a period of at most 16 rows, so it depends on the lane only: a fragment address is base register + immediate
// (tile t at + t 16 (2 HD) bytes, chunk c at + c 32 (2 HD), a transposed fragment's second read 16 (2 HD) further).
#pragma once
#include "common.h"
#include "kernels.h"

namespace {

constexpr float kLog2e = 1.44269504088896340736f;
typedef __bf16 v4bf16_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int ta_seq_base(const SeqMap& m, int s) {
  return (s / m.inner) * m.outer_stride + (s % m.inner) * m.inner_stride;
}
template <int HD = 64> __device__ __forceinline__ int ta_sw(int row) {
  static_assert(HD == 64 || HD == 32 || HD == 16, "head dim");
  if constexpr (HD == 64) return ((row >> 1) & 3) << 1;
  else if constexpr (HD == 32) return ((row >> 2) & 1) << 1;
  else return (row >> 3) & 1;
}
// What follows from the head dim: the register operand of the row products is NQ fragments per plane -- two 32-deep f16x8 at 64, one
// at 32, and at 16 ONE 16-deep f16x4 (v_mfma_f32_16x16x16_f16: lane (i, g) holds d = 4 g .. 4 g + 3, nothing padded, as X2Head<16> of
// attention_x2.hip); the transposed products have HD / 16 channel tiles; the softmax scale is HD^-0.5.
template <int HD> struct TAHead {
  static_assert(HD == 64 || HD == 32, "head dim");
  typedef f16x8 frag;
  static constexpr int ROWB = 2 * HD, NQ = HD / 32, ND = HD / 16;
  static constexpr float SCALE = HD == 64 ? 0.125f : 0.17677669529663688110f;
};
template <> struct TAHead<16> {
  typedef f16x4 frag;
  static constexpr int ROWB = 32, NQ = 1, ND = 1;
  static constexpr float SCALE = 0.25f;
};
// PADDED heads (PAD = true in the staging functions below and in the kernels of train_attn.hip): the true head dim hdt is a
// multiple of 8 below the image head dim HD (24 -> 32; 40 / 48 / 56 -> 64).  Global memory keeps the true layout -- head h starts
// at channel h hdt -- and only the LDS images and the register operands are HD wide: an 8-channel slot at or behind hdt is never
// loaded (it would be the neighbouring head, or lie behind the row for the last head of v) and holds exact zeros, so every
// product over channels adds zeros and every accumulator of a pad channel is an exact zero.  The softmax exponent is hdt^-0.5.
// (selected as BITS: the head dim is uniform, so the selects run on the scalar unit and the result stays in a scalar register --
//  computed as a float it would occupy a vector register in kernels that have none to spare.  ta_dispatch admits these four only.)
__device__ __forceinline__ float ta_true_scale(int hdt) {
  const unsigned bits = hdt == 24 ? 0x3e5105ecu : hdt == 40 ? 0x3e21e89bu : hdt == 48 ? 0x3e13cd3au : 0x3e08d677u;   // 24, 40, 48, 56 ^-0.5
  return __uint_as_float(bits);
}

// scale of a split operand from its absmax slot (as gemm_x2.hip dyn_scale): the largest magnitude lands in [2^13, 2^14)
__device__ __forceinline__ float ta_scale(const unsigned* amax) {
  const float m = __uint_as_float(amax[0]);
  if (!(m > 0.f) || !(m < INFINITY)) return 1.0f;
  int e;
  frexpf(m, &e);
  return ldexpf(1.0f, 14 - e);
}
__device__ __forceinline__ float ta_opaque(float x) { asm volatile("" : "+v"(x)); return x; }

__device__ __forceinline__ void ta_split8(const float4 a, const float4 b, f16x8& hi, f16x8& lo, float sc) {
  const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
  for (int e = 0; e < 8; ++e) { f16 h, l; split2h_scaled(v[e] * sc, h, l); hi[e] = h; lo[e] = l; }
}
// PASSES (template parameter of everything below that holds three-pass logic, default 3): the fp16-MFMA passes per product.
//   3: x 2^s = hi + lo, lo.hi + hi.lo + hi.hi into one fp32 accumulator; an image is two planes (hi | lo).
//   1 (train_attn_1p.hip, D3DP_TRAIN_ATTN_PASSES=1): the hi value alone -- the operand rounded ONCE to fp16 at its scale -- one MFMA
//      chain per product, and an image is ONE plane: no lo value is formed, stored or read anywhere.
// ta_planes is the ONE constant the kernels' image offsets and the launcher's LDS sizes both derive the plane count from: a mismatch
// between the two would be an out-of-bounds LDS access, not a wrong digit.
constexpr int ta_planes(int passes) { return passes == 1 ? 1 : 2; }
// the hi halves of ta_split8 alone: fp16(v sc)
__device__ __forceinline__ void ta_round8(const float4 a, const float4 b, f16x8& hi, float sc) {
  const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
  for (int e = 0; e < 8; ++e) hi[e] = (f16)(v[e] * sc);
}

// rows [0, n) x HD channels of an fp32 matrix (row stride `rs` floats) -> the hi / lo images (values x sc); rows [n, NK)
// zero.  Four 16-byte slots per thread and pass, all loads of a pass in flight before the first conversion.
// PAD: the matrix has hdt < HD channels; the slots behind them are not loaded and hold zeros.
template <int NK, int NT, int HD = 64, bool PAD = false, int PASSES = 3>
__device__ __forceinline__ void ta_stage(const float* __restrict__ src, size_t rs, int n, float sc, char* img, int tid, int hdt = HD) {
  constexpr int ROWB = 2 * HD, SL = HD / 8, LS = HD == 64 ? 3 : HD == 32 ? 2 : 1;   // bytes / 16-byte slots (2^LS) of an image row
  constexpr int PLANE = NK * ROWB;
  constexpr int ITEMS = NK * SL;                       // 16-byte slots of one plane
#ifdef D3DP_TA_PROBE                                   // timing probe (results INVALID): 1 = no staging at all, 2 = loads without the split
  if (D3DP_TA_PROBE == 1 && sc != -12345.f) return;
#endif
  for (int i0 = 0; i0 < ITEMS; i0 += 4 * NT) {
    float4 a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = i0 + u * NT + tid, row = idx >> LS, slot = idx & (SL - 1);
      a[u] = make_float4(0.f, 0.f, 0.f, 0.f); b[u] = a[u];
      if (idx < ITEMS && row < n && (!PAD || slot * 8 < hdt)) {
        const float* p = src + (size_t)row * rs + slot * 8;
        a[u] = *reinterpret_cast<const float4*>(p);
        b[u] = *reinterpret_cast<const float4*>(p + 4);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = i0 + u * NT + tid, row = idx >> LS, slot = idx & (SL - 1);
      if (idx < ITEMS) {
        if constexpr (PASSES == 1) {                   // one plane: the value rounded once
          f16x8 hi;
          ta_round8(a[u], b[u], hi, sc);
          *reinterpret_cast<f16x8*>(img + row * ROWB + ((slot ^ ta_sw<HD>(row)) << 4)) = hi;
        } else {
        f16x8 hi, lo;
#if defined(D3DP_TA_PROBE) && D3DP_TA_PROBE == 2
        hi = __builtin_bit_cast(f16x8, a[u]); lo = __builtin_bit_cast(f16x8, b[u]);
        if (sc == -12345.f)
#endif
        ta_split8(a[u], b[u], hi, lo, sc);
        const int off = row * ROWB + ((slot ^ ta_sw<HD>(row)) << 4);
        *reinterpret_cast<f16x8*>(img + off) = hi;
        *reinterpret_cast<f16x8*>(img + PLANE + off) = lo;
        }
      }
    }
  }
}

// The same for NS matrices at once: every matrix's loads of a pass are in flight before the first conversion -- ONE exposed memory round
// trip per chunk instead of one per operand (round 6: with the operands staged one after the other the loads' latency, not the
// split arithmetic, was 20 - 40 % of the training attention kernels: D3DP_TA_PROBE builds).  rows [0, n) valid for all of them.
template <int NK, int NT, int NS, int HD = 64, bool PAD = false, int PASSES = 3>
__device__ __forceinline__ void ta_stage_many(const float* const (&src)[NS], const size_t (&rs)[NS], const float (&sc)[NS],
                                              char* const (&img)[NS], int n, int tid, int hdt = HD) {
  constexpr int ROWB = 2 * HD, SL = HD / 8, LS = HD == 64 ? 3 : HD == 32 ? 2 : 1;
  constexpr int PLANE = NK * ROWB;
  constexpr int ITEMS = NK * SL;
#ifdef D3DP_TA_PROBE
  if (D3DP_TA_PROBE == 1 && sc[0] != -12345.f) return;
#endif
  for (int i0 = 0; i0 < ITEMS; i0 += 4 * NT) {
    float4 a[NS][4], b[NS][4];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int idx = i0 + u * NT + tid, row = idx >> LS, slot = idx & (SL - 1);
        a[s][u] = make_float4(0.f, 0.f, 0.f, 0.f); b[s][u] = a[s][u];
        if (idx < ITEMS && row < n && (!PAD || slot * 8 < hdt)) {
          const float* p = src[s] + (size_t)row * rs[s] + slot * 8;
          a[s][u] = *reinterpret_cast<const float4*>(p);
          b[s][u] = *reinterpret_cast<const float4*>(p + 4);
        }
      }
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int idx = i0 + u * NT + tid, row = idx >> LS, slot = idx & (SL - 1);
        if (idx < ITEMS) {
          if constexpr (PASSES == 1) {
            f16x8 hi;
            ta_round8(a[s][u], b[s][u], hi, sc[s]);
            *reinterpret_cast<f16x8*>(img[s] + row * ROWB + ((slot ^ ta_sw<HD>(row)) << 4)) = hi;
          } else {
          f16x8 hi, lo;
#if defined(D3DP_TA_PROBE) && D3DP_TA_PROBE == 2
          hi = __builtin_bit_cast(f16x8, a[s][u]); lo = __builtin_bit_cast(f16x8, b[s][u]);
          if (sc[0] == -12345.f)
#endif
          ta_split8(a[s][u], b[s][u], hi, lo, sc[s]);
          const int off = row * ROWB + ((slot ^ ta_sw<HD>(row)) << 4);
          *reinterpret_cast<f16x8*>(img[s] + off) = hi;
          *reinterpret_cast<f16x8*>(img[s] + PLANE + off) = lo;
          }
        }
      }
  }
}

// per-lane fragment addresses inside an image (hi plane; the lo plane is PLANE bytes further)
//   r0 / r1 : ROW fragment -- image row (16 t + lane & 15), channels 8 fg .. + 7 (r0) and 32 + 8 fg .. + 7 (r1); tile t at + t 2048
//   t[dn]   : TRANSPOSED fragment -- channel dn 16 + (lane & 15), image rows 32 c + 4 fg + {0..3} (first read) and + 16 (second,
//             2048 bytes further); chunk c at + c 4096.  (attn_frag.h make_frag_bases, V image)
//   (offsets at HD = 64; they halve with the row at 32 and again at 16.  HD = 32: r0 alone, channels 8 fg .. + 7.  HD = 16: r0 = the 8
//    bytes d = 4 fg .. 4 fg + 3 of the row.  There r1 = r0, unused.)
template <int HD> struct TAFragT { const char* r0; const char* r1; const char* t[HD / 16]; };
typedef TAFragT<64> TAFrag;
template <int HD = 64>
__device__ __forceinline__ TAFragT<HD> ta_frag(const char* img, int lane) {
  TAFragT<HD> f;
  const int fi = lane & 15, fg = lane >> 4;
  const int sw = ta_sw<HD>(fi);                        // (independent of the tile: rows advance in multiples of 16)
  if constexpr (HD == 64) {
    f.r0 = img + fi * 128 + ((fg ^ sw) << 4);
    f.r1 = img + fi * 128 + (((4 + fg) ^ sw) << 4);
    const int j = fi >> 2, qd = fi & 3, row = 4 * fg + j;
    const int vs = (row >> 1) & 3;
#pragma unroll
    for (int dn = 0; dn < 4; ++dn) f.t[dn] = img + row * 128 + ((dn ^ vs) << 5) + qd * 8;
  } else {
    constexpr int ROWB = 2 * HD;
    if constexpr (HD == 32) f.r0 = img + fi * ROWB + ((fg ^ sw) << 4);
    else f.r0 = img + fi * ROWB + (((fg >> 1) ^ sw) << 4) + (fg & 1) * 8;
    f.r1 = f.r0;
    // (the lane's 8 bytes: half qd & 1 of slot 2 dn + (qd >> 1), the slot swizzled as the staging loops wrote it)
    const int j = fi >> 2, qd = fi & 3, row = 4 * fg + j;
#pragma unroll
    for (int dn = 0; dn < HD / 16; ++dn) f.t[dn] = img + row * ROWB + (((2 * dn + (qd >> 1)) ^ ta_sw<HD>(row)) << 4) + (qd & 1) * 8;
  }
  return f;
}
template <int HD = 64>
__device__ __forceinline__ f16x8 ta_tr(const char* p) {
  const v4bf16_t a = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) v4bf16_t*)(p));
  const v4bf16_t b = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) v4bf16_t*)(p + 32 * HD));
  typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
  return __builtin_bit_cast(f16x8, (bf16x8_t){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]});
}
#define TA_MFMA(A, B, ACC) ACC = __builtin_amdgcn_mfma_f32_16x16x32_f16((A), (B), (ACC), 0, 0, 0)
#define TA_MFMA16(A, B, ACC) ACC = __builtin_amdgcn_mfma_f32_16x16x16f16((A), (B), (ACC), 0, 0, 0)

// the two 16-row tiles t, t + 1 of  (image rows) x (a register operand): acc_a / acc_b [row 16 t' + 4 fg + r][column lane & 15]
//   = sum_d img[row][d] x[column][d]  -- lo.hi + hi.lo + hi.hi over the two 32-deep halves of d (HD = 64), the one 32-deep MFMA
//   (HD = 32) or the one 16-deep MFMA (HD = 16) per pass.
// PASSES = 1: hi.hi alone; xl is not read and nothing PLANE bytes behind a fragment is.
template <int PLANE, int HD = 64, int PASSES = 3>
__device__ __forceinline__ void ta_rows_pair(const TAFragT<HD>& f, int t, const typename TAHead<HD>::frag (&xh)[TAHead<HD>::NQ],
                                             const typename TAHead<HD>::frag (&xl)[TAHead<HD>::NQ], f32x4& a, f32x4& b) {
  constexpr int TILE = 32 * HD;                        // 16 rows
  if constexpr (PASSES == 1) {
    typedef typename TAHead<HD>::frag frag;
    const char* p0 = f.r0 + t * TILE;
    const frag ah0 = *reinterpret_cast<const frag*>(p0), bh0 = *reinterpret_cast<const frag*>(p0 + TILE);
    a = (f32x4){0.f, 0.f, 0.f, 0.f}; b = a;
    if constexpr (HD == 64) {
      const char* p1 = f.r1 + t * TILE;
      const frag ah1 = *reinterpret_cast<const frag*>(p1), bh1 = *reinterpret_cast<const frag*>(p1 + TILE);
      TA_MFMA(ah0, xh[0], a); TA_MFMA(bh0, xh[0], b);
      TA_MFMA(ah1, xh[1], a); TA_MFMA(bh1, xh[1], b);
    } else if constexpr (HD == 32) {
      TA_MFMA(ah0, xh[0], a); TA_MFMA(bh0, xh[0], b);
    } else {
      TA_MFMA16(ah0, xh[0], a); TA_MFMA16(bh0, xh[0], b);
    }
  } else if constexpr (HD == 64) {
    const char* p0 = f.r0 + t * 2048;
    const char* p1 = f.r1 + t * 2048;
    const f16x8 al0 = *reinterpret_cast<const f16x8*>(p0 + PLANE), al1 = *reinterpret_cast<const f16x8*>(p1 + PLANE);
    const f16x8 bl0 = *reinterpret_cast<const f16x8*>(p0 + 2048 + PLANE), bl1 = *reinterpret_cast<const f16x8*>(p1 + 2048 + PLANE);
    const f16x8 ah0 = *reinterpret_cast<const f16x8*>(p0), ah1 = *reinterpret_cast<const f16x8*>(p1);
    const f16x8 bh0 = *reinterpret_cast<const f16x8*>(p0 + 2048), bh1 = *reinterpret_cast<const f16x8*>(p1 + 2048);
    a = (f32x4){0.f, 0.f, 0.f, 0.f}; b = a;
    TA_MFMA(al0, xh[0], a); TA_MFMA(bl0, xh[0], b);
    TA_MFMA(al1, xh[1], a); TA_MFMA(bl1, xh[1], b);
    TA_MFMA(ah0, xl[0], a); TA_MFMA(bh0, xl[0], b);
    TA_MFMA(ah1, xl[1], a); TA_MFMA(bh1, xl[1], b);
    TA_MFMA(ah0, xh[0], a); TA_MFMA(bh0, xh[0], b);
    TA_MFMA(ah1, xh[1], a); TA_MFMA(bh1, xh[1], b);
  } else {
    typedef typename TAHead<HD>::frag frag;
    const char* p0 = f.r0 + t * TILE;
    const frag al = *reinterpret_cast<const frag*>(p0 + PLANE), bl = *reinterpret_cast<const frag*>(p0 + TILE + PLANE);
    const frag ah = *reinterpret_cast<const frag*>(p0), bh = *reinterpret_cast<const frag*>(p0 + TILE);
    a = (f32x4){0.f, 0.f, 0.f, 0.f}; b = a;
    if constexpr (HD == 32) {
      TA_MFMA(al, xh[0], a); TA_MFMA(bl, xh[0], b);
      TA_MFMA(ah, xl[0], a); TA_MFMA(bh, xl[0], b);
      TA_MFMA(ah, xh[0], a); TA_MFMA(bh, xh[0], b);
    } else {
      TA_MFMA16(al, xh[0], a); TA_MFMA16(bl, xh[0], b);
      TA_MFMA16(ah, xl[0], a); TA_MFMA16(bh, xl[0], b);
      TA_MFMA16(ah, xh[0], a); TA_MFMA16(bh, xh[0], b);
    }
  }
}
// acc[dn][channel dn 16 + 4 fg + i][column] += sum over the 32 image rows of chunk c of img[row][channel] y[row][column]
// (y as a split register operand in the k order of the transposed fragments: rows 4 fg + r of tile 2 c, then of tile 2 c + 1)
// HD / 16 channel tiles, 32-deep MFMAs at every head dim.
// PASSES = 1: hi.hi alone; yl is not read.
template <int PLANE, int HD = 64, int PASSES = 3>
__device__ __forceinline__ void ta_tr_chunk(const TAFragT<HD>& f, int c, const f16x8& yh, const f16x8& yl, f32x4 (&acc)[HD / 16]) {
  constexpr int ND = HD / 16, CHUNK = 64 * HD;         // 32 rows
  if constexpr (PASSES == 1) {
    f16x8 t1[ND];
#pragma unroll
    for (int dn = 0; dn < ND; ++dn) t1[dn] = ta_tr<HD>(f.t[dn] + c * CHUNK);
#pragma unroll
    for (int dn = 0; dn < ND; ++dn) TA_MFMA(t1[dn], yh, acc[dn]);
    return;
  }
  f16x8 th[ND], tl[ND];
#pragma unroll
  for (int dn = 0; dn < ND; ++dn) { th[dn] = ta_tr<HD>(f.t[dn] + c * CHUNK); tl[dn] = ta_tr<HD>(f.t[dn] + c * CHUNK + PLANE); }
#pragma unroll
  for (int dn = 0; dn < ND; ++dn) TA_MFMA(tl[dn], yh, acc[dn]);
#pragma unroll
  for (int dn = 0; dn < ND; ++dn) TA_MFMA(th[dn], yl, acc[dn]);
#pragma unroll
  for (int dn = 0; dn < ND; ++dn) TA_MFMA(th[dn], yh, acc[dn]);
}

// this lane's HD / 4 values of a [.][HD] fp32 row as a split register operand (column operand of ta_rows_pair): channels
// 8 fg .. + 7 and 32 + 8 fg .. + 7 (HD = 64), 8 fg .. + 7 (HD = 32), 4 fg .. + 3 (HD = 16)
// (PAD: the row has hdt < HD channels; a group of 8 at or behind hdt is not loaded and is zero)
// PASSES = 1: h alone, l is left untouched.
template <int HD = 64, bool PAD = false, int PASSES = 3>
__device__ __forceinline__ void ta_load_row_op(const float* row, int fg, float sc, typename TAHead<HD>::frag (&h)[TAHead<HD>::NQ],
                                               typename TAHead<HD>::frag (&l)[TAHead<HD>::NQ], int hdt = HD) {
  static_assert(!PAD || HD >= 32, "padded heads: 8-channel groups");
  static_assert(!PAD || PASSES == 3, "padded heads: no one-pass form");
  if constexpr (PASSES == 1) {
    if constexpr (HD == 16) {
      const float4 v = *reinterpret_cast<const float4*>(row + fg * 4);
      const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) h[0][e] = (f16)(x[e] * sc);
    } else {
#pragma unroll
      for (int half = 0; half < TAHead<HD>::NQ; ++half) {
        const float* p = row + half * 32 + fg * 8;
        ta_round8(*reinterpret_cast<const float4*>(p), *reinterpret_cast<const float4*>(p + 4), h[half], sc);
      }
    }
  } else if constexpr (HD == 16) {
    const float4 v = *reinterpret_cast<const float4*>(row + fg * 4);
    const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) { f16 hh, ll; split2h_scaled(x[e] * sc, hh, ll); h[0][e] = hh; l[0][e] = ll; }
  } else {
#pragma unroll
    for (int half = 0; half < TAHead<HD>::NQ; ++half) {
      const float* p = row + half * 32 + fg * 8;
      if constexpr (PAD) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if ((HD == 64 && half == 0) || half * 32 + fg * 8 < hdt) {   // (HD 64: hdt >= 40, the first half lies inside every head)
          a = *reinterpret_cast<const float4*>(p); b = *reinterpret_cast<const float4*>(p + 4);
        }
        ta_split8(a, b, h[half], l[half], sc);
      } else ta_split8(*reinterpret_cast<const float4*>(p), *reinterpret_cast<const float4*>(p + 4), h[half], l[half], sc);
    }
  }
}
// eight values (two tiles x four rows) -> one split register operand at the power of two 2^(140 - eb) (eb: biased exponent
// the caller keeps >= that of the largest magnitude: |y| 2^(140 - eb) < 2^14)
// (PASSES = 1: h = fp16(y 2^(140 - eb)) alone, l untouched)
template <int PASSES = 3>
__device__ __forceinline__ void ta_split_run(const float (&y)[8], int eb, f16x8& h, f16x8& l) {
  const float sc = __uint_as_float((unsigned)(267 - eb) << 23);
  if constexpr (PASSES == 1) {
#pragma unroll
    for (int e = 0; e < 8; ++e) h[e] = (f16)(y[e] * sc);
    return;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float v = ta_opaque(y[e] * sc);              // (opaque: both halves must round the SAME number)
    const f16 hh = (f16)v;
    h[e] = hh;
    l[e] = (f16)(v - (float)hh);
  }
}
// biased exponent of max |y[e]| over the lane's eight values and the four lanes that share its column
__device__ __forceinline__ int ta_exp_of_max(const float (&y)[8]) {
  float m = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf(y[e]));
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  return (int)(__float_as_uint(m) >> 23);
}

}  // namespace
