// LDS images and MFMA fragment addresses shared by the two-pass matrix-core attention kernels: the FAST / FAST16 kernels
// (attention_fast.hip, one 2-byte plane per operand; head dims 64, 32 and 16) and the EXACT split-fp16 kernels (attention_x2.hip,
// the same head dims, a hi and a lo plane of the same layout `plane` bytes apart).  No transposes anywhere; at head dim 64:
//   K rows sit in LDS row-major (128 B per key) with the 16-byte-slot XOR swizzle ds_read_b128 wants;
//   V rows sit row-major too, swizzled at 32-byte-chunk granularity, and are consumed with
//   ds_read_b64_tr_b16: within each 16-lane group the instruction returns, to lane i, column i of the
//   4-key x 16-column block the group's lanes point at (lanes 4j..4j+3 -> key j) -- exactly the
//   "8 consecutive keys of one output channel" fragment the O^T = V^T P^T MFMA needs.  (Mapping measured on
//   gfx950 with tools/probe_tr.hip.)
// (The chunked-key split-fp16 kernel at head dim 64 and the training attention use the one-swizzle images of ta_common.h instead.)
#pragma once
#include "common.h"
#include "ta_common.h"

namespace {

// Head dims 32 and 16 (HD is a template parameter that defaults to 64, and the HD = 64 forms below are the
// expressions the images were first written with).  A K or V row is 2 HD bytes = HD / 8 16-byte slots, so the 256-byte bank
// row that ds_read_b128, ds_read_b64 and ds_read_b64_tr_b16 all bank on ((addr / 4) mod 64) holds 2 / 4 / 8 rows.  The
// swizzles are XORs on the 16-byte slot index of a row, as functions of the row:
//   K, HD = 64 (128-B rows, 8 slots): slot ^= (row >> 1) & 7.  ds_read_b128 is served in 16-lane groups {0-3, 12-15, 20-27},
//     {4-11, 16-19, 28-31} (+32): in the first, rows 0-3 and 12-15 read slot fg = 0 and rows 4-11 slot 1; rows 2p, 2p + 1 lie
//     in opposite halves of the bank row and the XOR sends the eight pairs to eight different slots of their half.
//   K, HD = 32 (64-B rows, 4 slots; one 16x16x32 MFMA: lane (fi, fg) reads row fi, slot fg): rows r, r + 4, r + 8, r + 12 share
//     a quarter of the bank row.  A group holds, per quarter, rows r and r + 12 at one fg and rows r + 4 and r + 8 at fg ^ 1;
//     slot ^= ((row >> 3) & 1) << 1 sends them to slots {fg, fg ^ 2, fg ^ 1, fg ^ 3}: four different ones, conflict-free.
//   K, HD = 16 (32-B rows, 2 slots; one 16x16x16 MFMA: lane (fi, fg) reads the 8 bytes d = 4 fg .. 4 fg + 3 of row fi with
//     ds_read_b64, which banks per 32-lane half): a half reads the same 16-byte slot (fg >> 1) of rows 0 .. 15, and rows r, r + 8
//     share an eighth of the bank row: slot ^= (row >> 3) & 1 puts them on its two different slots, conflict-free.
//   V, HD = 64: 32-byte chunk (16 channels) ^= (row >> 1) & 3.  A 32-lane half of ds_read_b64_tr_b16 reads one chunk of the 8
//     rows 8h .. 8h + 7; rows 2p, 2p + 1 are the halves of a bank row, the XOR spreads the four pairs over its four chunks.
//   V, HD = 32 (two chunks per row, four rows per bank row): rows r and r + 4 of the half share 64 bytes: chunk ^= (row >> 2) & 1.
//   V, HD = 16 (one chunk per row): the 8 rows of a half ARE one bank row.  No swizzle.
// Every swizzle has a period of at most 16 rows, so it depends on the lane only and a fragment address stays
// base register + compile-time immediate: K tile t at + t 16 (2 HD) bytes, V key chunk c at + c 32 (2 HD), its second half
// 16 (2 HD) further.
template <int HD> __device__ __forceinline__ int k_slot_swizzle(int row) {
  static_assert(HD == 64 || HD == 32 || HD == 16, "head dim");
  if constexpr (HD == 64) return (row >> 1) & 7;
  else if constexpr (HD == 32) return ((row >> 3) & 1) << 1;
  else return (row >> 3) & 1;
}
template <int HD> __device__ __forceinline__ int v_slot_swizzle(int row) {
  if constexpr (HD == 64) return ((row >> 1) & 3) << 1;
  else if constexpr (HD == 32) return ((row >> 2) & 1) << 1;
  else return 0;
}

// Per-lane LDS base addresses of the K and V^T fragments.  Both swizzles depend only on the lane (not on the key
// tile), so every fragment read in the tile loop is  base register + compile-time immediate.
template <int HD = 64>
struct FragBasesT {
  const char* k0;            // K row (lane&15), d-slot  (lane>>4)      ; tile t at +t*2048   (HD = 16: the 8 bytes d = 4 (lane>>4) ..)
  const char* k1;            // K row (lane&15), d-slot 4+(lane>>4)                           (HD = 64 only; else = k0, unused)
  const char* v[HD / 16];    // V row 4g+j, 32-B chunk dn (swizzled), + qd*8 ; key chunk c at +c*4096, second half +2048
                             // (offsets at HD = 64: 128-byte rows; they halve with the row at 32 and again at 16)
};
typedef FragBasesT<64> FragBases;
template <int HD = 64>
__device__ __forceinline__ FragBasesT<HD> make_frag_bases(const char* KS, const char* VS, int lane) {
  FragBasesT<HD> fb;
  const int fi = lane & 15, fg = lane >> 4;
  const int j = fi >> 2, qd = fi & 3, key = 4 * fg + j;
  if constexpr (HD == 64) {
    const int sw = (fi >> 1) & 7;                       // ((16t + fi) >> 1) & 7 is independent of t
    fb.k0 = KS + fi * 128 + ((fg ^ sw) << 4);
    fb.k1 = KS + fi * 128 + (((4 + fg) ^ sw) << 4);
    const int vs = (key >> 1) & 3;                      // ((32c [+16] + key) >> 1) & 3 is independent of c
#pragma unroll
    for (int dn = 0; dn < 4; ++dn) fb.v[dn] = VS + key * 128 + ((dn ^ vs) << 5) + qd * 8;
  } else {
    if constexpr (HD == 32) fb.k0 = KS + fi * 64 + ((fg ^ k_slot_swizzle<32>(fi)) << 4);
    else fb.k0 = KS + fi * 32 + (((fg >> 1) ^ k_slot_swizzle<16>(fi)) << 4) + (fg & 1) * 8;
    fb.k1 = fb.k0;
#pragma unroll
    for (int dn = 0; dn < HD / 16; ++dn) fb.v[dn] = VS + key * (2 * HD) + (((2 * dn) ^ v_slot_swizzle<HD>(key)) << 4) + qd * 8;
  }
  return fb;
}

// V^T fragment (MFMA A operand) for output channels dn*16 + (lane&15), keys {32c + 4g + j} and {32c + 16 + 4g + j}
// (E: the element type of the result; the transposing read moves 16-bit payloads whatever they mean, so the bf16 builtin
//  serves both and the fp16 form is a bit cast of its result)
template <int C0, typename E = bf16, int HD = 64>
__device__ __forceinline__ typename Op2<E>::x8 load_vt_frag(const char* vb) {
  constexpr int HALF = 16 * 2 * HD;                     // 16 keys
  const v4bf16_t a = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) v4bf16_t*)(vb + C0 * 2 * HALF));
  const v4bf16_t b = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) v4bf16_t*)(vb + C0 * 2 * HALF + HALF));
  return __builtin_bit_cast(typename Op2<E>::x8, (bf16x8){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]});
}

}  // namespace
