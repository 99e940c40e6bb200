// Tile geometry and LDS image shared by the split-fp16 Linear kernels: gemm_x2.hip (the product EXACT Linear and, in a
// -DD3DP_X2_VARIANTS=1 build, its experimental forms) and gemm_x2_train.hip (the training step's Linear).
#pragma once
#include "common.h"

namespace {

constexpr int XBM = 256, XBN = 128, XBK = 32;
constexpr int XA_BYTES = XBM * 128;                  // 32 KiB: 256 rows x (64 B hi | 64 B lo)
constexpr int XW_BYTES = XBN * 128;                  // 16 KiB
constexpr int XSTAGE = XA_BYTES + XW_BYTES;          // 48 KiB
constexpr int XNSTAGE = 3;
constexpr int XBIAS_MAX = 2048;                      // floats of bias kept in LDS
constexpr int XROWSTAT = XNSTAGE * XSTAGE + XBIAS_MAX * 4;   // EPI_GELU_LN: 2 x [256 rows][mean, rstd] (tile t in buffer t & 1)
constexpr int XLDS = XROWSTAT + 2 * XBM * 8;             // 156 KiB
constexpr int XNCW = 8;                              // compute waves (4 x 2); waves 8..11 are loaders

// LDS image of a slab: 128-byte rows = 8 slots of 16 B (q = 4 plane + k-group of 8 columns); slot q of row r lives at
// physical slot q ^ ((r >> 1) & 7).  A fragment read (lane: row fi, k-group fg, one plane) is then conflict-free: the four
// 16-lane groups of ds_read_b128 ({0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32) each cover 8 rows of one
// k-group and 8 rows of the next, and (row & 1) 8 + (q ^ (row >> 1 & 7)) takes 16 different values on them.
__device__ __forceinline__ int swz128(int row, int q) { return q ^ ((row >> 1) & 7); }

// W row carried by LDS row q of a 64-column strip: MFMA tile ni = q>>4, operand row i = q&15 -> output column 4 i + ni
__device__ __forceinline__ int colperm(int q) { return (q & 15) * 4 + (q >> 4); }

}  // namespace

// the k-step barrier of these kernels: raw (no waitcnt in front of it; every kernel waits on exactly the counter it needs)
#define X2_BARRIER() asm volatile("s_barrier" ::: "memory")
