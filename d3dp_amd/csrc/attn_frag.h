// LDS images and MFMA fragment addresses shared by the two-pass matrix-core attention kernels at head dim 64: the FAST / FAST16
// kernels (attention_fast.hip, one 2-byte plane per operand) and the EXACT split-fp16 kernels (attention_x2.hip, a hi and a lo
// plane of the same layout `plane` bytes apart).  No transposes anywhere:
//   K rows sit in LDS row-major (128 B per key) with the 16-byte-slot XOR swizzle ds_read_b128 wants;
//   V rows sit row-major too, swizzled at 32-byte-chunk granularity, and are consumed with
//   ds_read_b64_tr_b16: within each 16-lane group the instruction returns, to lane i, column i of the
//   4-key x 16-column block the group's lanes point at (lanes 4j..4j+3 -> key j) -- exactly the
//   "8 consecutive keys of one output channel" fragment the O^T = V^T P^T MFMA needs.  (Mapping measured on
//   gfx950 with tools/probe_tr.hip.)
// (The chunked-key split-fp16 kernel and the training attention use the one-swizzle images of ta_common.h instead.)
#pragma once
#include "common.h"
#include "ta_common.h"

namespace {

// Per-lane LDS base addresses of the K and V^T fragments.  Both swizzles depend only on the lane (not on the key
// tile), so every fragment read in the tile loop is  base register + compile-time immediate.
struct FragBases {
  const char* k0;      // K row (lane&15), d-slot  (lane>>4)      ; tile t at +t*2048
  const char* k1;      // K row (lane&15), d-slot 4+(lane>>4)
  const char* v[4];    // V row 4g+j, 32-B chunk dn (swizzled), + qd*8 ; key chunk c at +c*4096, second half +2048
};
__device__ __forceinline__ FragBases make_frag_bases(const char* KS, const char* VS, int lane) {
  FragBases fb;
  const int fi = lane & 15, fg = lane >> 4;
  const int sw = (fi >> 1) & 7;                       // ((16t + fi) >> 1) & 7 is independent of t
  fb.k0 = KS + fi * 128 + ((fg ^ sw) << 4);
  fb.k1 = KS + fi * 128 + (((4 + fg) ^ sw) << 4);
  const int j = fi >> 2, qd = fi & 3, key = 4 * fg + j;
  const int vs = (key >> 1) & 3;                      // ((32c [+16] + key) >> 1) & 3 is independent of c
#pragma unroll
  for (int dn = 0; dn < 4; ++dn) fb.v[dn] = VS + key * 128 + ((dn ^ vs) << 5) + qd * 8;
  return fb;
}

// V^T fragment (MFMA A operand) for output channels dn*16 + (lane&15), keys {32c + 4g + j} and {32c + 16 + 4g + j}
// (E: the element type of the result; the transposing read moves 16-bit payloads whatever they mean, so the bf16 builtin
//  serves both and the fp16 form is a bit cast of its result)
template <int C0, typename E = bf16>
__device__ __forceinline__ typename Op2<E>::x8 load_vt_frag(const char* vb) {
  const v4bf16_t a = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) v4bf16_t*)(vb + C0 * 4096));
  const v4bf16_t b = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) v4bf16_t*)(vb + C0 * 4096 + 2048));
  return __builtin_bit_cast(typename Op2<E>::x8, (bf16x8){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]});
}

}  // namespace
