// The training step's Linear layers on split-fp16 operands (the scheme of gemm_x2.hip with operand scales that live on the
// device): gemm_f16x2_dyn_kernel (forward, dgrad, split-K wgrad), gemm_f16x2_tn_kernel (wgrad straight from the row forms),
// the passes that write their operands (split2h_*_dyn, dyprep, rowprep*, gelu_rowprep, wprep_*) and the ordered sums of
// their partial products (sum_partials_*).  Tile geometry and LDS image: gemm_x2_tile.h.
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "gemm_x2_tile.h"
#include "kernels.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// The training step's Linear (forward, dgrad and the split-K wgrad of SURVEY.md row A13) on the same three-pass split-fp16
// scheme: out_z[M, N] = (A2 . W2^T over the k-steps of chunk z) x dynA[0] x dynW[0] (+ bias), fp32 out.
//   * operand scales are DEVICE values: gradients have no range known on the host, so every operand is split at the power
//     of two its own absmax asks for (split2h_dyn_kernel / split2h_t_dyn_kernel below write 1 / scale next to the planes) and
//     this kernel reads the two factors -- no host synchronisation anywhere in the step;
//   * Z chunks of the contraction (k-steps z NKz .. (z + 1) NKz - 1 of rows of 2 Kfull fp16) go to Z x tiles work items:
//     a weight gradient in its transposed-operand form (shapes the TN kernel below does not take) contracts over the 16,524
//     tokens of a batch into at most 24 output tiles, far too few for 256 CUs unsplit; the partial results are summed in a
//     fixed order by sum_partials_kernel (deterministic, unlike the fp32-atomic split-K of the fp32-MFMA path this replaces);
//   * rem_m0 (optional; Z = 1 launches): the rows behind the last whole 256-row tile as 16 x 64 blocks -- see the compute waves.
// Structure: the lock-step kernel of gemm_x2.hip (gemm_f16x2_kernel) without the lagged MFMAs and with the plain fp32 epilogue (8 + 4 waves, 256 x 128 x 32
// tiles, 3-stage LDS-DMA ring, one barrier per k-step).
//   * amax_out (optional; Z = 1 launches): the output's absmax (amax_pos: its largest positive value), one atomicMax per
//     workgroup -- the operand scale of whatever split-fp16 kernel consumes the output next (the training attention kernels:
//     q / k / v and dO; the fc2 operand GELU(fc1 output): gelu_rowprep_kernel), without an absmax pass.
//   * PASSES (template parameter): 3 = the split scheme above; 1 = the one-pass route of
//     D3DP_TRAIN_PASSES=1 -- the compute waves issue the hi x hi MFMA alone and never read the lo halves (offAl / offWl in LDS, the
//     second 64 bytes of a line in the remainder blocks).  The hi plane of an operand IS that tensor rounded to fp16 at its own
//     power-of-two scale, so the product is fp16 operands, fp32 accumulation, same k order, same scales and epilogue.  The loaders
//     are the same: whole 128-byte h2i lines, of which this form uses the first 64 bytes.
//   * HI (template parameter; PASSES = 1 alone): the operands are hi-only rows of D3DP_TRAIN_ROWS=hi ("h1": Kfull plain fp16 per row,
//     a 128-byte line = 64 consecutive k).  Same pieces, swizzle and ring; a STAGE carries 256 x 128 x 64 -- two k-steps -- and the
//     compute waves issue per (mi, ni) the MFMA of the fragments at offA / offW (k 0..31 of the stage) and then the one at offA ^ 64 /
//     offW ^ 64 (k 32..63): the lanes' k values, their fragment positions and the order of the k-steps per accumulator are those of
//     the PASSES = 1 form on h2i rows, with half the barriers, waits and staged bytes per product.  NKz stays in k-steps of 32 (even).
template <int PASSES, bool HI = false>
__global__ __launch_bounds__(768) void gemm_f16x2_dyn_kernel(const f16* __restrict__ A2, const f16* __restrict__ W2,
                                                             const float* __restrict__ bias, const float* __restrict__ dynA,
                                                             const float* __restrict__ dynW, float* __restrict__ out, int M,
                                                             int N, int Kfull, int NKz, int tiles_n, int tiles_per_z,
                                                             int total_items, unsigned* __restrict__ amax_out, int amax_pos,
                                                             int rem_m0) {
  static_assert(PASSES == 1 || PASSES == 3, "one pass (hi x hi) or the three-pass split scheme");
  static_assert(!HI || PASSES == 1, "hi-only rows hold no lo halves");
  constexpr int RS = HI ? 1 : 2;                       // fp16 elements of an operand row per column of the contraction
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int G = gridDim.x;
  const int L = xcd_remap(blockIdx.x, G);
  const int n_my = (total_items - L + G - 1) / G;      // work items L, L+G, ...: item = z tiles_per_z + tile
  const int NS = HI ? NKz >> 1 : NKz;                  // stages (128-byte lines of a row) per work item
  const int gtot = n_my * NS;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (gtot <= 0) return;
  // remainder rows (rem_m0 > 0, Z = 1): blocks of 16 rows x 64 columns, block b to workgroup b mod G -- see the end of the kernel
  const int rem_cg = (N + 63) >> 6;
  const int rem_blocks = rem_m0 > 0 ? ((M - rem_m0 + 15) >> 4) * rem_cg : 0;

  if (wave >= XNCW) {
    const int lw = wave - XNCW;
    const int lr = lane >> 3, lq = lane & 7;
    int ti = 0, ks = 0, slot = 0;
    const f16* pa[8];
    const f16* pw[4];
    auto issue = [&]() {
      if (ks == 0) {
        const int item = L + ti * G;
        const int z = item / tiles_per_z, t = item - z * tiles_per_z;
        const int m0 = (t / tiles_n) * XBM, n0 = (t % tiles_n) * XBN;
        const size_t k0 = (size_t)z * NS * (2 * XBK);    // first k-step of the chunk, in fp16 elements of an h2i (HI: h1) row
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int row = (lw * 8 + i) * 8 + lr;
          pa[i] = A2 + (size_t)min(m0 + row, M - 1) * (RS * Kfull) + k0 + swz128(row, lq) * 8;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = (lw * 4 + i) * 8 + lr;
          const int wrow = (row & 64) + colperm(row & 63);
          pw[i] = W2 + (size_t)min(n0 + wrow, N - 1) * (RS * Kfull) + k0 + swz128(row, lq) * 8;
        }
      }
      char* base = smem + slot * XSTAGE;
      const int ko = ks * (2 * XBK);
#pragma unroll
      for (int i = 0; i < 8; ++i) __builtin_amdgcn_global_load_lds(GPTR(pa[i] + ko), LPTR(base + (lw * 8 + i) * 1024), 16, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        __builtin_amdgcn_global_load_lds(GPTR(pw[i] + ko), LPTR(base + XA_BYTES + (lw * 4 + i) * 1024), 16, 0, 0);
      if (++ks == NS) { ks = 0; ++ti; }
      slot = (slot == XNSTAGE - 1) ? 0 : slot + 1;
    };
    issue();
    if (gtot > 1) issue();
    // (the compute waves' remainder blocks, two barriers each: FIRST, while these two stages are in flight -- see below)
    for (int b = L; b < rem_blocks; b += G) { X2_BARRIER(); X2_BARRIER(); }
    for (int g = 0; g < gtot; ++g) {
      if (g + 1 < gtot) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      X2_BARRIER();
      if (g + 2 < gtot) issue();
    }
    if (amax_out) X2_BARRIER();                        // (the compute waves' absmax hand-over below)
    return;
  }

  const int wr = wave >> 1, wc = wave & 1;
  const int fi = lane & 15, fg = lane >> 4;
  const int offA = (wr * 64 + fi) * 128 + swz128(fi, fg) * 16, offAl = offA ^ 64;
  const int offW = XA_BYTES + (wc * 64 + fi) * 128 + swz128(fi, fg) * 16, offWl = offW ^ 64;
  const float unscale = dynA[0] * dynW[0];             // 1 / (scale of A x scale of W): powers of two, exact
  __builtin_amdgcn_s_setprio(1);
  float am = 0.f;
  int slot = 0;
  // The remainder rows.  The configs[4] batch has M = 16,524 = 64 x 256 + 140 rows: as a 65th row of 256 x 128 tiles the last 140
  // rows cost every forward / dgrad product a whole extra round of the persistent loop with 4 - 12 of the 256 CUs busy (12 us
  // of a 35 - 70 us product; round 4 sent them to a second, split-K launch plus a sum kernel where the contraction was long
  // enough -- no cheaper).  Here the tiles cover the first rem_m0 = 256 q rows only -- a whole number of rounds when q x tiles_n is
  // a multiple of the CU count, as 64 x {4, 8, 12} is -- and the rows behind them are cut into 16 x 64 blocks, one per workgroup
  // (140 rows x 512 .. 1536 columns: 72 .. 216 blocks, every CU busy once more for a few microseconds): the eight compute waves
  // split the contraction (NKz / 8 k-steps each, fragments straight from global memory -- 64 KiB per block, no LDS staging),
  // exchange their partial accumulators through LDS and wave 0 adds them in wave order (deterministic), applies scale and bias
  // and stores.  The blocks come FIRST: the loader waves have just requested the first two stages of the first tile and the
  // compute waves would wait for them anyway -- the exchange uses the third stage of the ring, which the loaders fill only
  // after the first k-step's barrier.  Same MFMA triple per k-step as the tiles, same fp32 accumulation: the only difference to a
  // tile's result is the grouping of the k-steps into eight partial sums.
  if (rem_blocks > 0) {
    const int ksw = NKz / XNCW;                        // k-steps per wave (launcher: NKz % 16 == 0, so an even number)
    f32x4* xch = reinterpret_cast<f32x4*>(smem + (XNSTAGE - 1) * XSTAGE);
#pragma unroll 1
    for (int b = L; b < rem_blocks; b += G) {
      const int m0 = rem_m0 + (b / rem_cg) * 16, nb0 = (b % rem_cg) * 64;
      const size_t kofs = (size_t)wave * ksw * (RS * XBK) + fg * 8;   // (HI: the same k-steps, 32 elements each)
      const f16* ap = A2 + (size_t)min(m0 + fi, M - 1) * (RS * Kfull) + kofs;
      const f16* wp[4];
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) wp[ni] = W2 + (size_t)min(nb0 + 4 * fi + ni, N - 1) * (RS * Kfull) + kofs;
      f32x4 pacc[4];
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) pacc[ni] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
      for (int ks = 0; ks < ksw; ks += 2) {
        f16x8 ah[2], al[2], wh[2][4], wl[2][4];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int o = (ks + u) * (RS * XBK);
          ah[u] = *reinterpret_cast<const f16x8*>(ap + o);
          if constexpr (PASSES == 3) al[u] = *reinterpret_cast<const f16x8*>(ap + o + XBK);
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) {
            wh[u][ni] = *reinterpret_cast<const f16x8*>(wp[ni] + o);
            if constexpr (PASSES == 3) wl[u][ni] = *reinterpret_cast<const f16x8*>(wp[ni] + o + XBK);
          }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          if constexpr (PASSES == 3) {
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) pacc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[u], wl[u][ni], pacc[ni], 0, 0, 0);
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) pacc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[u], wh[u][ni], pacc[ni], 0, 0, 0);
          }
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) pacc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[u], wh[u][ni], pacc[ni], 0, 0, 0);
        }
      }
      X2_BARRIER();                                    // nobody reads the previous block's partial sums any more
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) xch[(wave * 4 + ni) * 64 + lane] = pacc[ni];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      X2_BARRIER();
      if (wave == 0) {
        f32x4 sum[4];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          sum[ni] = xch[ni * 64 + lane];
#pragma unroll
          for (int w = 1; w < XNCW; ++w) sum[ni] += xch[(w * 4 + ni) * 64 + lane];
        }
        const int nb = nb0 + 4 * fi;
        if (nb < N) {
          float4 bz = {0.f, 0.f, 0.f, 0.f};
          if (bias != nullptr) bz = *reinterpret_cast<const float4*>(bias + nb);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = m0 + 4 * fg + r;
            if (m < M) {
              const f32x4 v = {fmaf(sum[0][r], unscale, bz.x), fmaf(sum[1][r], unscale, bz.y), fmaf(sum[2][r], unscale, bz.z),
                               fmaf(sum[3][r], unscale, bz.w)};
              *reinterpret_cast<f32x4*>(out + (size_t)m * N + nb) = v;
              am = amax_pos ? fmaxf(am, fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])))
                            : fmaxf(am, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
            }
          }
        }
      }
    }
  }
#pragma unroll 1
  for (int ti = 0; ti < n_my; ++ti) {
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int ks = 0; ks < NS; ++ks) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      X2_BARRIER();
      const char* sb = smem + slot * XSTAGE;
      slot = (slot == XNSTAGE - 1) ? 0 : slot + 1;
      f16x8 wf[4][2];
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int pl = 0; pl < (PASSES == 3 || HI ? 2 : 1); ++pl)   // (HI: pl = the second k-step of the stage)
          wf[ni][pl] = *reinterpret_cast<const f16x8*>(sb + (pl ? offWl : offW) + ni * 2048);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const f16x8 ah = *reinterpret_cast<const f16x8*>(sb + offA + mi * 2048);
        if constexpr (HI) {
          const f16x8 a2 = *reinterpret_cast<const f16x8*>(sb + offAl + mi * 2048);
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, wf[ni][0], acc[mi][ni], 0, 0, 0);   // k 0..31
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2, wf[ni][1], acc[mi][ni], 0, 0, 0);   // k 32..63
          continue;
        }
        if constexpr (PASSES == 3) {
          const f16x8 al = *reinterpret_cast<const f16x8*>(sb + offAl + mi * 2048);
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, wf[ni][1], acc[mi][ni], 0, 0, 0);
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, wf[ni][0], acc[mi][ni], 0, 0, 0);
        }
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, wf[ni][0], acc[mi][ni], 0, 0, 0);
      }
    }
    // epilogue: lane holds out[pm0 + mi*16 + r][nb + ni]; one 16-byte store per (mi, r)
    const int item = L + ti * G;
    const int z = item / tiles_per_z, t = item - z * tiles_per_z;
    const int pm0 = (t / tiles_n) * XBM + wr * 64 + 4 * fg, nb = (t % tiles_n) * XBN + wc * 64 + 4 * fi;
    if (nb < N) {                                      // (N % 4 == 0: a lane's four columns exist together)
      float4 bz = {0.f, 0.f, 0.f, 0.f};
      if (bias != nullptr) bz = *reinterpret_cast<const float4*>(bias + nb);
      float* o = out + (size_t)z * M * N + nb;
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = pm0 + mi * 16 + r;
          if (m < M) {
            const f32x4 v = {fmaf(acc[mi][0][r], unscale, bz.x), fmaf(acc[mi][1][r], unscale, bz.y),
                             fmaf(acc[mi][2][r], unscale, bz.z), fmaf(acc[mi][3][r], unscale, bz.w)};
            *reinterpret_cast<f32x4*>(o + (size_t)m * N) = v;
            // (amax_pos: the largest POSITIVE value instead of the largest magnitude -- what bounds GELU of this output)
            am = amax_pos ? fmaxf(am, fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])))
                          : fmaxf(am, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
          }
        }
    }
  }
  if (amax_out) {                                      // (uniform: a kernel argument)
    float* part = reinterpret_cast<float*>(smem + XNSTAGE * XSTAGE);   // behind the ring, which slower waves may still be reading
    am = wave_max(am);
    if (lane == 0) part[wave] = am;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    X2_BARRIER();
    if (wave == 0 && lane == 0) {
      float m = part[0];
#pragma unroll
      for (int w = 1; w < XNCW; ++w) m = fmaxf(m, part[w]);
      atomicMax(amax_out, __float_as_uint(m));
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The training step's weight gradient  dW[N, K] = dY[T, N]^T X[T, K]  straight from the ROW forms of its two operands (the "TN"
// form): out_z[n][k] = sum over the tokens t of chunk z of A2[t][n] W2[t][k], x dynA[0] x dynW[0].
// Round 4 fed wgrad the TRANSPOSED forms [features][2 Tp] through gemm_f16x2_dyn_kernel above, which every forward Linear's input and
// every dY had to be written out in a second time by a tile transpose (dyprep_kernel: 9.8 GB and 3.5 ms of the configs[4] step,
// its scattered 128-byte writes at 2.8 TB/s).  Here the contraction runs over ROWS of the operands: a k-step is 32 token rows,
// the A slab 32 rows x 256 features (1 KiB per row = 8 h2i blocks, ONE LDS-DMA wave-instruction), the W slab 32 rows x 128
// features (512 B per row, two rows per instruction) -- the same 48 KiB per stage, 12 pieces per loader wave and k-step as the
// dyn kernel above, and the same 8 + 4 waves, 3-stage ring and barrier structure.  The fragments an MFMA wants -- 8 consecutive
// TOKENS of one feature -- are columns of the slab: ds_read_b64_tr_b16 (the transposed fragment read of attn_frag.h's V
// image: 4 token rows x 16 features per 16 lanes) delivers them; lane group g holds the tokens {4 g + j} and {16 + 4 g + j} of
// the k-step for BOTH operands, so the k order of the two fragments agrees.  LDS swizzle: 16-byte slot s of token row r sits at
// s ^ ((r & 7) << 1): the eight rows a transposed read touches per cycle land in eight different 32-byte bank groups (the rows
// are 1 KiB / 512 B apart: unswizzled they would all hit the same one).
// Rows T .. Tp - 1 of both operands must exist and be ZERO (dyprep_kernel writes them).  Output: a lane holds
// out[n = .. + 4 g + r][k = .. + 16 ni + i] -- 4-byte stores, 64 contiguous bytes per 16 lanes; the partial tiles are small (N K
// floats per chunk) and summed by sum_partials_kernel.
// Several products in one launch (D3dpTnTable, kernels.h): the four weight gradients of a block -- fc2, fc1, proj, qkv: 8 + 16 + 16 +
// 24 = 64 output tiles at configs[4] -- contract over the SAME token rows, so their tiles form one list and the split count is
// chosen for the list: Z = 4 chunks of 130 k-steps x 64 tiles = 256 equal work items, one per CU.  Launched one by one each
// product had to be cut into Z = 10 .. 32 chunks to fill the chip by itself: 32 MB of partial tiles written and read again per
// product (one 128 KiB tile per CU whatever the shape) and a pipeline ramp and a store phase per 17 .. 52 k-steps -- together about
// as long as the products' matrix work.  Merged, a block writes 32 MB of partial tiles ONCE and ramps once per 130 k-steps.
__device__ __forceinline__ int tn_find(const D3dpTnTable& tb, int t) {
  int i = 0;
#pragma unroll
  for (int j = 1; j < D3DP_TN_MAX; ++j)
    if (j < tb.n && t >= tb.p[j].tile0) i = j;
  return i;
}
// PASSES: as gemm_f16x2_dyn_kernel -- 1 = hi x hi alone, the lo planes of the slabs (pl = 1) are never read from LDS.
// HI (PASSES = 1 alone; D3DP_TRAIN_ROWS=hi): both operands are hi-only rows [Tp][N] / [Tp][K].  The k-step stays 32 token rows, so Tp,
// the split count, the product table, the partial tiles and their ordered sum keep their grouping; the slab rows halve -- A 512 B
// (256 features), W 256 B (128 features): 24 KiB per stage in the same 3-stage ring (72 KiB), as 16 A pieces of two rows and 8 W
// pieces of four rows, 1 KiB each: SIX LDS-DMA instructions per loader wave and k-step instead of twelve.  16-byte slot s (8
// features) of token row r sits at s ^ ((r & 7) << 1) as before: the rows are still whole multiples of 256 B apart, so the eight rows
// a transposed read touches per cycle land in eight different 32-byte bank groups; the lanes of a fragment read point at the same
// tokens and features as in the split form, so every MFMA sees the same values in the same positions.
constexpr int XTN_HI_A = 32 * 512, XTN_HI_STAGE = XTN_HI_A + 32 * 256;   // 16 KiB + 8 KiB per k-step
template <int PASSES, bool HI = false>
__global__ __launch_bounds__(768) void gemm_f16x2_tn_kernel(D3dpTnTable tb, int NKz, int tiles_per_z, int total_items) {
  static_assert(PASSES == 1 || PASSES == 3, "one pass (hi x hi) or the three-pass split scheme");
  static_assert(!HI || PASSES == 1, "hi-only rows hold no lo halves");
  constexpr int STAGE = HI ? XTN_HI_STAGE : XSTAGE, A_BYTES = HI ? XTN_HI_A : XA_BYTES, A_ROW = HI ? 512 : 1024, W_ROW = HI ? 256 : 512;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int G = gridDim.x;
  const int L = xcd_remap(blockIdx.x, G);
  const int n_my = (total_items - L + G - 1) / G;      // work items L, L+G, ...: item = z tiles_per_z + tile (of the merged list)
  const int gtot = n_my * NKz;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (gtot <= 0) return;

  if (wave >= XNCW) {
    // ---------------------------------------------------------------- loader waves: 8 A pieces + 4 W pieces per k-step each
    const int lw = wave - XNCW;
    int ti = 0, ks = 0, slot = 0;
    const f16* pa;                                     // this lane's source of A piece 0 of the current item (k-step 0)
    const f16* pw;
    size_t a_row = 0, w_row = 0;                       // fp16 elements per operand row
    auto issue = [&]() {
      if (ks == 0) {
        const int item = L + ti * G;
        const int z = item / tiles_per_z, tt = item - z * tiles_per_z;
        const D3dpTnProduct& P = tb.p[tn_find(tb, tt)];
        const int t = tt - P.tile0;
        const int n0 = (t / P.tiles_k) * XBM, k0 = (t % P.tiles_k) * XBN;
        const size_t t0 = (size_t)z * NKz * XBK;       // first token row of the chunk
        a_row = (size_t)(HI ? 1 : 2) * P.N; w_row = (size_t)(HI ? 1 : 2) * P.K;
        // A piece i = token row lw 8 + i of the k-step (1 KiB: features n0 .. n0 + 255); lane l fetches logical slot l ^ swz
        // (N % 256 == 0 and K % 128 == 0: the launcher sends other shapes to gemm_f16x2_dyn_kernel)
        pa = (const f16*)P.A2 + (t0 + lw * 8) * a_row + (size_t)n0 * (HI ? 1 : 2);
        pw = (const f16*)P.W2 + (t0 + lw * 8) * w_row + (size_t)k0 * (HI ? 1 : 2);
      }
      char* base = smem + slot * STAGE;
      const size_t ro = (size_t)ks * XBK;              // token rows into the chunk
      if constexpr (HI) {
        // this wave's token rows lw 8 .. lw 8 + 7 of the k-step: A pieces of two rows (32 lanes each), W pieces of four (16 lanes each)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int rr = 2 * i + (lane >> 5);              // row within the wave's eight; (lw 8 + rr) & 7 == rr
          __builtin_amdgcn_global_load_lds(GPTR(pa + (ro + rr) * a_row + (((lane & 31) ^ (rr << 1)) << 3)),
                                           LPTR(base + (lw * 8 + 2 * i) * 512), 16, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int rr = 4 * i + (lane >> 4);
          __builtin_amdgcn_global_load_lds(GPTR(pw + (ro + rr) * w_row + (((lane & 15) ^ (rr << 1)) << 3)),
                                           LPTR(base + A_BYTES + (lw * 8 + 4 * i) * 256), 16, 0, 0);
        }
      } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int r = lw * 8 + i;                      // token row of the k-step; r & 7 == i
        __builtin_amdgcn_global_load_lds(GPTR(pa + (ro + i) * a_row + ((lane ^ (i << 1)) << 3)), LPTR(base + r * 1024), 16, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = lw * 8 + 2 * i + (lane >> 5);    // two token rows per piece: lanes 0-31 / 32-63
        const int l32 = lane & 31;
        __builtin_amdgcn_global_load_lds(GPTR(pw + (ro + 2 * i + (lane >> 5)) * w_row + ((l32 ^ ((r & 7) << 1)) << 3)),
                                         LPTR(base + XA_BYTES + (lw * 8 + 2 * i) * 512), 16, 0, 0);
      }
      }
      if (++ks == NKz) { ks = 0; ++ti; }
      slot = (slot == XNSTAGE - 1) ? 0 : slot + 1;
    };
    issue();
    if (gtot > 1) issue();
    for (int g = 0; g < gtot; ++g) {
      if (g + 1 < gtot) { if constexpr (HI) asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); }
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      X2_BARRIER();
      if (g + 2 < gtot) issue();
    }
    return;
  }

  // -------------------------------------------------------------------- compute waves: 64 (n) x 64 (k) of the 256 x 128 tile
  const int wr = wave >> 1, wc = wave & 1;
  const int fi = lane & 15, fg = lane >> 4;
  const int j = fi >> 2, qd = fi & 3, row = 4 * fg + j;        // transposed read: lanes 4 j .. 4 j + 3 point at token row 4 fg + j
  // slot of the 16 features (mi / ni) x plane inside a token row: block b = wr 2 + (mi >> 1) (A) / wc 2 + (ni >> 1) (W),
  // slot = b 8 + plane 4 + (mi & 1) 2 + (qd >> 1); the swizzle of rows `row` and `row + 16` is the same (r & 7)
  // (HI: no plane bit -- slot = b 4 + (mi & 1) 2 + (qd >> 1) of a 512 B / 256 B row)
  auto a_off = [&](int mi, int pl) {
    if constexpr (HI) return row * 512 + (((((wr * 2 + (mi >> 1)) << 2) | ((mi & 1) << 1) | (qd >> 1)) ^ ((row & 7) << 1)) << 4) + ((qd & 1) << 3);
    else return row * 1024 + (((((wr * 2 + (mi >> 1)) << 3) | (pl << 2) | ((mi & 1) << 1) | (qd >> 1)) ^ ((row & 7) << 1)) << 4) + ((qd & 1) << 3);
  };
  auto w_off = [&](int ni, int pl) {
    if constexpr (HI) return A_BYTES + row * 256 + (((((wc * 2 + (ni >> 1)) << 2) | ((ni & 1) << 1) | (qd >> 1)) ^ ((row & 7) << 1)) << 4) + ((qd & 1) << 3);
    else return XA_BYTES + row * 512 + (((((wc * 2 + (ni >> 1)) << 3) | (pl << 2) | ((ni & 1) << 1) | (qd >> 1)) ^ ((row & 7) << 1)) << 4) + ((qd & 1) << 3);
  };
  typedef __bf16 v4bf __attribute__((ext_vector_type(4)));
  typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
  auto tr8 = [&](const char* p, int second) {         // 8 tokens of one feature: rows 4 fg + {0..3} and 16 + 4 fg + {0..3}
    const v4bf a = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) v4bf*)(p));
    const v4bf b = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) v4bf*)(p + second));
    return __builtin_bit_cast(f16x8, (v8bf){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]});
  };
  int offA[4][2], offW[4][2];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) { offA[m][pl] = a_off(m, pl); offW[m][pl] = w_off(m, pl); }
  __builtin_amdgcn_s_setprio(1);
  int slot = 0;
#pragma unroll 1
  for (int ti = 0; ti < n_my; ++ti) {
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) acc[i][jj] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int ks = 0; ks < NKz; ++ks) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      X2_BARRIER();
      const char* sb = smem + slot * STAGE;
      slot = (slot == XNSTAGE - 1) ? 0 : slot + 1;
      f16x8 wf[4][2];
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int pl = 0; pl < (PASSES == 3 ? 2 : 1); ++pl) wf[ni][pl] = tr8(sb + offW[ni][pl], 16 * W_ROW);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const f16x8 ah = tr8(sb + offA[mi][0], 16 * A_ROW);
        if constexpr (PASSES == 3) {
          const f16x8 al = tr8(sb + offA[mi][1], 16 * A_ROW);
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, wf[ni][1], acc[mi][ni], 0, 0, 0);
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, wf[ni][0], acc[mi][ni], 0, 0, 0);
        }
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, wf[ni][0], acc[mi][ni], 0, 0, 0);
      }
    }
    // epilogue: lane holds out[nn = n0 + wr 64 + mi 16 + 4 fg + r][kk = k0 + wc 64 + ni 16 + fi]
    const int item = L + ti * G;
    const int z = item / tiles_per_z, tt = item - z * tiles_per_z;
    const D3dpTnProduct& P = tb.p[tn_find(tb, tt)];
    const int t = tt - P.tile0, K = P.K;
    const int n0 = (t / P.tiles_k) * XBM, k0 = (t % P.tiles_k) * XBN;
    const float unscale = P.dynA[0] * P.dynW[0];
    float* o = P.out + (size_t)z * P.N * K + (size_t)(n0 + wr * 64 + 4 * fg) * K + k0 + wc * 64 + fi;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) o[(size_t)(mi * 16 + r) * K + ni * 16] = acc[mi][ni][r] * unscale;
  }
}

// scale of a split operand from its absmax (bit pattern of a non-negative float, absmax_kernel): the power of two that
// puts the largest magnitude in [2^13, 2^14) (as capi_weights.hip does for the inference weights); 1 for an all-zero tensor
__device__ __forceinline__ float dyn_scale(unsigned amax_bits) {
  const float m = __uint_as_float(amax_bits);
  if (!(m > 0.f) || !(m < INFINITY)) return 1.0f;
  int e;
  frexpf(m, &e);                                       // m = f 2^e, f in [0.5, 1)
  return ldexpf(1.0f, 14 - e);
}

// HI (template parameter of the operand kernels below; D3DP_TRAIN_ROWS=hi): the destination rows are hi-only, [.][C] plain fp16 with
// column c at offset c -- the hi value of split2h_scaled at the same scale, no lo value and no store of one.

// src [R][C] fp32 -> dst [R][2 Cpad] h2i (columns C .. Cpad - 1 zero), scale from the tensor's absmax; unscale[0] = 1 / scale.
// A thread owns 8 consecutive columns (C % 8 == 0, Cpad % 32 == 0): two 16-byte loads, one 16-byte store per plane.
template <bool HI = false>
__global__ void split2h_dyn_kernel(const float* __restrict__ s, f16* __restrict__ d, int R, int C, int Cpad,
                                   const unsigned* __restrict__ amax, float* __restrict__ unscale) {
  const float sc = dyn_scale(amax[0]);
  if (blockIdx.x == 0 && threadIdx.x == 0) unscale[0] = 1.0f / sc;
  const int G8 = Cpad / 8;
  const size_t n = (size_t)R * G8;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / G8;
    const int c = (int)(i - r * G8) * 8;
    f16x8 hi = {}, lo = {};
    if (c < C) {
      const float4 a = *reinterpret_cast<const float4*>(s + r * C + c), b = *reinterpret_cast<const float4*>(s + r * C + c + 4);
      const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
      for (int e = 0; e < 8; ++e) { f16 h, l; split2h_scaled(v[e] * sc, h, l); hi[e] = h; lo[e] = l; }
    }
    f16* row = HI ? d + r * (size_t)Cpad + c : d + r * 2 * (size_t)Cpad + h2i_col(c);
    *reinterpret_cast<f16x8*>(row) = hi;
    if constexpr (!HI) *reinterpret_cast<f16x8*>(row + kH2iLo) = lo;
  }
}

// src [R][C] fp32 -> dst [C][2 Rpad] h2i: the TRANSPOSE as a split operand (rows R .. Rpad - 1 zero).  32 x 32 tiles through LDS;
// one tile = one 128-byte h2i block (hi of 32 source rows | lo of the same) of 32 destination rows.
__global__ __launch_bounds__(256) void split2h_t_dyn_kernel(const float* __restrict__ s, f16* __restrict__ d, int R, int C,
                                                            int Rpad, const unsigned* __restrict__ amax,
                                                            float* __restrict__ unscale) {
  __shared__ float tile[32][33];
  const float sc = dyn_scale(amax[0]);
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) unscale[0] = 1.0f / sc;
  const int r0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = ty; k < 32; k += 8) {
    const int r = r0 + k, c = c0 + tx;
    tile[k][tx] = (r < R && c < C) ? s[(size_t)r * C + c] * sc : 0.f;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int c = c0 + k;                              // destination row; tx = source row within the block
    if (c < C) {
      f16 a, b;
      split2h_scaled(tile[tx][k], a, b);
      f16* blk = d + (size_t)c * 2 * Rpad + (size_t)blockIdx.x * 64;
      blk[tx] = a;
      blk[32 + tx] = b;
    }
  }
}

// One pass over an fp32 matrix src [R][C] for everything the training step needs from it as a split-fp16 operand: the row
// form [R][2 C] (a forward Linear's / dgrad's operand), the transposed form [C][2 Rpad] (wgrad's operand; rows R .. Rpad - 1
// zero) and, for a gradient dY, its column sums (the bias gradient) -- as three kernels (split2h_dyn, split2h_t_dyn, colsum)
// the same tensor was read three times.  blockIdx.y = a strip of 32 columns; a workgroup takes tiles of DY_ROWS rows x 32
// columns (one tile per workgroup at the configs[4] size: every workgroup resident at once): SIX 16-byte loads per thread in
// flight (round 4: one load per thread on 512 workgroups -- two per CU -- which left the kernel latency-bound at 2.7 TB/s),
// and every store instruction writes WHOLE 128-byte lines of both outputs: the row form as one 16-byte store per lane
// (neighbouring lanes swap their hi / lo halves by DPP: even lane -> 8 columns of hi, odd lane -> lo), the transposed form
// through LDS with lanes 0-3 of an 8-lane group writing the hi half and lanes 4-7 the lo half of ONE line (8 source rows of
// one destination row and plane per lane).  Column sums: this workgroup's rows into row blockIdx.x of `colpart` (gridDim.x
// rows of C floats, summed in a fixed order by d3dp_train_reduce_many: no float atomics).  C % 32 == 0, Rpad % 32 == 0.
constexpr int DY_SUB = 6, DY_ROWS = 32 * DY_SUB;      // 192 rows per tile
__global__ __launch_bounds__(256) void dyprep_kernel(const float* __restrict__ s, f16* __restrict__ drow, f16* __restrict__ dcol,
                                                     float* __restrict__ colpart, int R, int C, int Rpad,
                                                     const unsigned* __restrict__ amax, float* __restrict__ unscale) {
  __shared__ float tile[DY_ROWS][33];
  const float sc = dyn_scale(amax[0]);
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) unscale[0] = 1.0f / sc;
  const int c0 = blockIdx.y * 32;
  const int tr = threadIdx.x >> 3, tj = threadIdx.x & 7, tq = tj * 4;   // phase 1: source row u 32 + tr, columns tq .. tq + 3
  const int nblk = Rpad / 32;                           // 32-row blocks of the transposed form
  const bool odd = tj & 1;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int rt = blockIdx.x; rt * DY_SUB < nblk; rt += gridDim.x) {
    float4 v[DY_SUB];
#pragma unroll
    for (int u = 0; u < DY_SUB; ++u) {
      const int r = rt * DY_ROWS + u * 32 + tr;
      v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < R) v[u] = *reinterpret_cast<const float4*>(s + (size_t)r * C + c0 + tq);
    }
    __syncthreads();                                    // (the previous tile's transposed reads are done)
#pragma unroll
    for (int u = 0; u < DY_SUB; ++u) {
      const int r = rt * DY_ROWS + u * 32 + tr;
      acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w;
      const float vs[4] = {v[u].x * sc, v[u].y * sc, v[u].z * sc, v[u].w * sc};
      float* trow = &tile[u * 32 + tr][tq];
      trow[0] = vs[0]; trow[1] = vs[1]; trow[2] = vs[2]; trow[3] = vs[3];
      // row form: the 128-byte h2i block of row r, columns c0 .. c0 + 31 -- lanes 2 j / 2 j + 1 hold columns 8 j .. 8 j + 7:
      // the even lane stores both hi halves, the odd lane both lo halves (quad_perm [1,0,3,2]: the value of lane ^ 1)
      f16x4 hi, lo;
#pragma unroll
      for (int e = 0; e < 4; ++e) { f16 h, l; split2h_scaled(vs[e], h, l); hi[e] = h; lo[e] = l; }
      const uint2 hh = __builtin_bit_cast(uint2, hi), ll = __builtin_bit_cast(uint2, lo);
      const uint2 send = odd ? hh : ll;
      uint2 recv;
      recv.x = __builtin_amdgcn_update_dpp(0, (int)send.x, 0xB1, 0xF, 0xF, false);
      recv.y = __builtin_amdgcn_update_dpp(0, (int)send.y, 0xB1, 0xF, 0xF, false);
      using u32x4 = unsigned __attribute__((ext_vector_type(4)));
      const u32x4 o16 = odd ? (u32x4){recv.x, recv.y, ll.x, ll.y} : (u32x4){hh.x, hh.y, recv.x, recv.y};
      if (r < R) {
        f16* blk = drow + (size_t)r * 2 * C + (size_t)blockIdx.y * 64 + (tq & ~7) + (odd ? 32 : 0);
        *reinterpret_cast<u32x4*>(blk) = o16;
      }
    }
    __syncthreads();
    // transposed form: destination row c0 + tr; lanes tj 0-3 write the hi half, tj 4-7 the lo half of the line of block u
    {
      const int g8 = tj & 3;
      const bool lo_half = tj >= 4;
#pragma unroll
      for (int u = 0; u < DY_SUB; ++u) {
        if (rt * DY_SUB + u < nblk) {
          f16x8 o;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float x = tile[u * 32 + g8 * 8 + e][tr];
            const f16 h = (f16)x;
            o[e] = lo_half ? (f16)(x - (float)h) : h;
          }
          f16* blk = dcol + (size_t)(c0 + tr) * 2 * Rpad + (size_t)(rt * DY_SUB + u) * 64 + (lo_half ? 32 : 0) + g8 * 8;
          *reinterpret_cast<f16x8*>(blk) = o;
        }
      }
    }
  }
  if (colpart) {
    __syncthreads();
    float* cs = &tile[0][0];                             // [32][33] of the tile buffer
    cs[tr * 33 + tq] = acc.x; cs[tr * 33 + tq + 1] = acc.y; cs[tr * 33 + tq + 2] = acc.z; cs[tr * 33 + tq + 3] = acc.w;
    __syncthreads();
    if (threadIdx.x < 32) {
      float t = 0.f;
#pragma unroll 8
      for (int j = 0; j < 32; ++j) t += cs[j * 33 + threadIdx.x];
      colpart[(size_t)blockIdx.x * C + c0 + threadIdx.x] = t;
    }
  }
}

// The ROW form alone, as a streaming pass over whole rows (the TN weight-gradient kernel above reads both of its operands in
// this form, so nothing is transposed): src [R][C] fp32 -> drow [Rpad][2 C] h2i (rows R .. Rpad - 1 ZERO: the TN kernel
// contracts over them) and, for a gradient, its column sums as gridDim.x partial rows of C floats (fixed-order reduction by
// d3dp_train_reduce_many).  A thread owns 8 consecutive columns (two 16-byte loads, one 16-byte store per plane) of the rows
// r = 4 blockIdx.x + (tid >> 6), + 4 gridDim.x, ...: reads and writes are contiguous in memory -- unlike the tile transpose of
// dyprep_kernel, whose 128-byte pieces land 66 KB apart.  C % 32 == 0, C <= 1536 (P = ceil(C / 512) column passes per row).
// mask (optional): per-sample DropPath scales -- row r is multiplied by mask[sample(r)] first (sample = r / J on the spatial
// axis, (r / (F J)) J + r % J on the temporal one): the backward pass then never stores the scaled gradient, only its absmax.
// GELU (gelu_pre [R][C]: the fc1 output of the forward pass): src is d hidden and the operand is d h_pre = src x gelu'(gelu_pre),
// formed here instead of by a pass of its own (gelu_bwd_kernel: a read of both tensors and a write of the product that only this
// kernel read again).  `amax` then holds the absmax of SRC (left by the fc2 dgrad's epilogue) and the operand scale follows
// from the bound |gelu'| <= 1.13: at most one binade below the scale of the true absmax whenever the largest |src| sits where
// gelu' >= 0.57, and never an overflow -- the two fp16 planes keep 22 bits below whatever power of two is chosen.
template <int P, bool GELU, bool HI = false>
__global__ __launch_bounds__(256) void rowprep_kernel(const float* __restrict__ s, f16* __restrict__ drow, float* __restrict__ colpart,
                                                      int R, int Rpad, int C, const unsigned* __restrict__ amax,
                                                      float* __restrict__ unscale, const float* __restrict__ mask, int axis, int F,
                                                      int J, const float* __restrict__ gelu_pre) {
  __shared__ float cs[4][P * 512];
  const float sc = GELU ? dyn_scale(__float_as_uint(__uint_as_float(amax[0]) * kGeluGradMax)) : dyn_scale(amax[0]);
  if (blockIdx.x == 0 && threadIdx.x == 0) unscale[0] = 1.0f / sc;
  const int l = threadIdx.x & 63, rl = threadIdx.x >> 6;
  float acc[P][8];
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[p][e] = 0.f;
  constexpr int U = P == 1 ? 4 : 2;                    // rows per wave and iteration: 8 loads of 16 bytes in flight per thread
  const int rstep = gridDim.x * 4;
  for (int r0 = blockIdx.x * 4 + rl; r0 < Rpad; r0 += rstep * U) {
    float4 a[U][P], b[U][P], ga[GELU ? U : 1][P], gb[GELU ? U : 1][P];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const int r = r0 + u * rstep, c = p * 512 + l * 8;
        a[u][p] = make_float4(0.f, 0.f, 0.f, 0.f); b[u][p] = a[u][p];
        if constexpr (GELU) { ga[u][p] = a[u][p]; gb[u][p] = a[u][p]; }
        if (r < R && c < C) {
          a[u][p] = *reinterpret_cast<const float4*>(s + (size_t)r * C + c);
          b[u][p] = *reinterpret_cast<const float4*>(s + (size_t)r * C + c + 4);
          if constexpr (GELU) {
            ga[u][p] = *reinterpret_cast<const float4*>(gelu_pre + (size_t)r * C + c);
            gb[u][p] = *reinterpret_cast<const float4*>(gelu_pre + (size_t)r * C + c + 4);
          }
        }
      }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const int r = r0 + u * rstep, c = p * 512 + l * 8;
        if (r < Rpad && c < C) {
          float mk = 1.0f;
          if (mask && r < R) mk = mask[axis == 0 ? r / J : (r / (F * J)) * J + r % J];
          float v[8] = {a[u][p].x * mk, a[u][p].y * mk, a[u][p].z * mk, a[u][p].w * mk,
                        b[u][p].x * mk, b[u][p].y * mk, b[u][p].z * mk, b[u][p].w * mk};
          if constexpr (GELU) {
            const float g[8] = {ga[u][p].x, ga[u][p].y, ga[u][p].z, ga[u][p].w, gb[u][p].x, gb[u][p].y, gb[u][p].z, gb[u][p].w};
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] *= gelu_grad_rational(g[e]);
          }
          f16x8 hi, lo;
#pragma unroll
          for (int e = 0; e < 8; ++e) { acc[p][e] += v[e]; f16 h, lw; split2h_scaled(v[e] * sc, h, lw); hi[e] = h; lo[e] = lw; }
          f16* row = HI ? drow + (size_t)r * C + c : drow + (size_t)r * 2 * C + h2i_col(c);
          *reinterpret_cast<f16x8*>(row) = hi;
          if constexpr (!HI) *reinterpret_cast<f16x8*>(row + kH2iLo) = lo;
        }
      }
  }
  if (colpart) {
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
      for (int e = 0; e < 8; ++e) cs[rl][p * 512 + l * 8 + e] = acc[p][e];
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256)
      colpart[(size_t)blockIdx.x * C + c] = ((cs[0][c] + cs[1][c]) + cs[2][c]) + cs[3][c];
  }
}

// The row form of a LayerNorm's OUTPUT from its INPUT: drow [Rpad][2 C] = split(LN(src [R][C]; w, b, eps)) (rows R .. Rpad - 1
// zero), the scale from `amax` -- which the kernel that produced src left there as the absmax of this very LayerNorm output,
// computed on the fly and not stored.  The forward pass of the training step then never writes the fp32 normalised activation
// (its only reader was this operand pass).  One wave per row, a lane owns 8 consecutive columns (C <= 512, C % 8 == 0).
template <bool HI = false>
__global__ __launch_bounds__(256) void rowprep_ln_kernel(const float* __restrict__ s, const float* __restrict__ w,
                                                         const float* __restrict__ b, float eps, f16* __restrict__ drow, int R,
                                                         int Rpad, int C, const unsigned* __restrict__ amax,
                                                         float* __restrict__ unscale) {
  const float sc = dyn_scale(amax[0]);
  if (blockIdx.x == 0 && threadIdx.x == 0) unscale[0] = 1.0f / sc;
  const int l = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = l * 8;
  const bool on = c < C;
  float wl[8], bl[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { wl[e] = on ? w[c + e] : 0.f; bl[e] = on ? b[c + e] : 0.f; }
  const int rstep = gridDim.x * 4;
  const float invC = 1.0f / (float)C;
  constexpr int U = 4;                                   // rows per wave and iteration: their loads and reductions interleave
  for (int r0 = blockIdx.x * 4 + rl; r0 < Rpad; r0 += U * rstep) {
    float v[U][8];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int r = r0 + u * rstep;
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), bb = a;
      if (r < R && on) {
        a = *reinterpret_cast<const float4*>(s + (size_t)r * C + c);
        bb = *reinterpret_cast<const float4*>(s + (size_t)r * C + c + 4);
      }
      v[u][0] = a.x; v[u][1] = a.y; v[u][2] = a.z; v[u][3] = a.w; v[u][4] = bb.x; v[u][5] = bb.y; v[u][6] = bb.z; v[u][7] = bb.w;
    }
    float mean[U], rstd[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float sm = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) sm += v[u][e];
      mean[u] = sm;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
      for (int u = 0; u < U; ++u) mean[u] += __shfl_xor(mean[u], o, 64);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      mean[u] *= invC;
      float q = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = on ? v[u][e] - mean[u] : 0.f; q = fmaf(d, d, q); }
      rstd[u] = q;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
      for (int u = 0; u < U; ++u) rstd[u] += __shfl_xor(rstd[u], o, 64);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int r = r0 + u * rstep;
      if (r < Rpad && on) {
        const float rs = 1.0f / sqrtf(rstd[u] * invC + eps);
        f16x8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float y = r < R ? fmaf((v[u][e] - mean[u]) * rs, wl[e], bl[e]) : 0.f;
          f16 h, lw;
          split2h_scaled(y * sc, h, lw);
          hi[e] = h; lo[e] = lw;
        }
        f16* row = HI ? drow + (size_t)r * C + c : drow + (size_t)r * 2 * C + h2i_col(c);
        *reinterpret_cast<f16x8*>(row) = hi;
        if constexpr (!HI) *reinterpret_cast<f16x8*>(row + kH2iLo) = lo;
      }
    }
  }
}

// The fc2 operand of the training step straight from the fc1 output:  drow [Rpad][2 C] (h2i, rows R .. Rpad - 1 zero) =
// split(GELU(src)) -- without the fp32 hidden tensor in between (round 4: gelu_fwd wrote it, the operand pass read it again).
// The operand scale needs max |GELU(x)| BEFORE the first element is written; it follows from the largest positive x alone,
// which the fc1 Linear's epilogue leaves in `pmax` (gemm_f16x2_dyn_kernel, amax_pos): GELU is increasing on x > -0.75 and
// |GELU(x)| <= 0.17 for x < 0, so max |GELU| = max(GELU(pmax), at most 0.17) -- exact whenever GELU(pmax) >= 0.17, and the
// same power of two otherwise unless every activation is tiny.  Writes amax_out[0] (the bits of that bound) and unscale[0].
template <bool HI = false>
__global__ __launch_bounds__(256) void gelu_rowprep_kernel(const float* __restrict__ s, f16* __restrict__ drow, int R, int Rpad,
                                                           int C, const unsigned* __restrict__ pmax, unsigned* __restrict__ amax_out,
                                                           float* __restrict__ unscale) {
  const float pm = __uint_as_float(pmax[0]);
  const float bound = fmaxf(gelu_erf_rational(pm), 0.17004f);
  const float sc = dyn_scale(__float_as_uint(bound));
  if (blockIdx.x == 0 && threadIdx.x == 0) { unscale[0] = 1.0f / sc; amax_out[0] = __float_as_uint(bound); }
  const int G8 = C / 8;
  const size_t n = (size_t)Rpad * G8, stride = (size_t)gridDim.x * 256;
  for (size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x; i0 < n; i0 += 2 * stride) {
    float4 a[2], b[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const size_t i = i0 + u * stride;
      const size_t r = i / G8;
      const int c = (int)(i - r * G8) * 8;
      a[u] = make_float4(0.f, 0.f, 0.f, 0.f); b[u] = a[u];
      if (i < n && r < (size_t)R) {
        a[u] = *reinterpret_cast<const float4*>(s + r * C + c);
        b[u] = *reinterpret_cast<const float4*>(s + r * C + c + 4);
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const size_t i = i0 + u * stride;
      if (i < n) {
        const size_t r = i / G8;
        const int c = (int)(i - r * G8) * 8;
        const float v[8] = {a[u].x, a[u].y, a[u].z, a[u].w, b[u].x, b[u].y, b[u].z, b[u].w};
        f16x8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float g = r < (size_t)R ? gelu_erf_rational(v[e]) : 0.f;
          f16 h, l;
          split2h_scaled(g * sc, h, l);
          hi[e] = h; lo[e] = l;
        }
        f16* row = HI ? drow + r * (size_t)C + c : drow + r * 2 * (size_t)C + h2i_col(c);
        *reinterpret_cast<f16x8*>(row) = hi;
        if constexpr (!HI) *reinterpret_cast<f16x8*>(row + kH2iLo) = lo;
      }
    }
  }
}

// ---- the training step's weight operands, all Linears of the model in three launches ------------------------------------
// (per-weight launches of absmax / split2h_dyn / split2h_t_dyn: 192 launches of 5 - 6 us for 100 MB of weights per step)
// blockIdx.y = the weight; a workgroup row strides over that weight only.
__global__ __launch_bounds__(256) void wprep_absmax_kernel(D3dpWPrepTable tb, unsigned* __restrict__ amax) {
  __shared__ float part[4];
  const D3dpWPrepItem it = tb.it[blockIdx.y];
  const size_t n4 = (size_t)it.N * it.K / 4, stride = (size_t)gridDim.x * blockDim.x;
  const float4* s4 = reinterpret_cast<const float4*>(it.w);
  float m = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 v = s4[i];
    m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(amax + it.slot, __float_as_uint(fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]))));
}
// rows form [N][2 K] (the forward operand) of every weight: the loop of split2h_dyn_kernel
template <bool HI = false>
__global__ __launch_bounds__(256) void wprep_rows_kernel(D3dpWPrepTable tb, f16* __restrict__ base, const unsigned* __restrict__ amax,
                                                         float* __restrict__ unscale) {
  const D3dpWPrepItem it = tb.it[blockIdx.y];
  const float sc = dyn_scale(amax[it.slot]);
  if (blockIdx.x == 0 && threadIdx.x == 0) unscale[it.slot] = 1.0f / sc;
  f16* d = base + 2 * it.off;                           // (HI too: the start of the same region, half used)
  const int G8 = it.K / 8;
  const size_t n = (size_t)it.N * G8;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / G8;
    const int c = (int)(i - r * G8) * 8;
    const float4 a = *reinterpret_cast<const float4*>(it.w + r * it.K + c), b = *reinterpret_cast<const float4*>(it.w + r * it.K + c + 4);
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    f16x8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; ++e) { f16 h, l; split2h_scaled(v[e] * sc, h, l); hi[e] = h; lo[e] = l; }
    f16* row = HI ? d + r * (size_t)it.K + c : d + r * 2 * (size_t)it.K + h2i_col(c);
    *reinterpret_cast<f16x8*>(row) = hi;
    if constexpr (!HI) *reinterpret_cast<f16x8*>(row + kH2iLo) = lo;
  }
}
// transposed form [K][2 N] (the dgrad operand) of every weight: the tiles of split2h_t_dyn_kernel, strided over by a
// workgroup row (N % 32 == 0, K % 32 == 0)
// (HI: [K][N] hi-only -- source row r0 + tx lands at column r0 + tx of destination row c0 + k)
template <bool HI = false>
__global__ __launch_bounds__(256) void wprep_cols_kernel(D3dpWPrepTable tb, f16* __restrict__ base, const unsigned* __restrict__ amax) {
  __shared__ float tile[32][33];
  const D3dpWPrepItem it = tb.it[blockIdx.y];
  const float sc = dyn_scale(amax[it.slot]);
  f16* d = base + 2 * it.off;                           // (HI too: the start of the same region, half used)
  const int tr = it.N / 32, tc = it.K / 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int tI = blockIdx.x; tI < tr * tc; tI += gridDim.x) {
    const int r0 = (tI / tc) * 32, c0 = (tI % tc) * 32;
    __syncthreads();
    for (int k = ty; k < 32; k += 8) tile[k][tx] = it.w[(size_t)(r0 + k) * it.K + c0 + tx] * sc;
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
      f16 a, b;
      split2h_scaled(tile[tx][k], a, b);
      if constexpr (HI) {
        d[(size_t)(c0 + k) * it.N + r0 + tx] = a;
      } else {
        f16* blk = d + (size_t)(c0 + k) * 2 * it.N + (size_t)(r0 / 32) * 64;
        blk[tx] = a;
        blk[32 + tx] = b;
      }
    }
  }
}

// out[i] = sum_z part[z n + i] in the order z = 0, 1, ... (the deterministic end of a split-K product)
// A thread owns four consecutive outputs (n % 4 == 0) and keeps eight partials in flight: the partial tiles of a weight gradient
// are 32 MB (one 256 x 128 tile per CU) whatever its shape, and the one-load-at-a-time form of this kernel read them at 1.9 TB/s.
__global__ __launch_bounds__(256) void sum_partials_kernel(const float4* __restrict__ part, float4* __restrict__ out, size_t n4, int Z) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const float4* p = part + i;
    float4 a = p[0];
    int z = 1;
    for (; z + 8 <= Z; z += 8) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(z + u) * n4];
#pragma unroll
      for (int u = 0; u < 8; ++u) { a.x += v[u].x; a.y += v[u].y; a.z += v[u].z; a.w += v[u].w; }
    }
    for (; z < Z; ++z) {
      const float4 v = p[(size_t)z * n4];
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    out[i] = a;
  }
}

// the same for up to D3DP_TN_MAX products at once (blockIdx.y = the product; Z partials each, as d3dp_launch_linear_f16x2_tn_many leaves them)
__global__ __launch_bounds__(256) void sum_partials_many_kernel(D3dpSumTable tb) {
  const float4* part = reinterpret_cast<const float4*>(tb.part[blockIdx.y]);
  float4* out = reinterpret_cast<float4*>(tb.out[blockIdx.y]);
  const size_t n4 = tb.n4[blockIdx.y];
  const int Z = tb.Z;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float4* p = part + i;
    float4 a = p[0];
    int z = 1;
    for (; z + 4 <= Z; z += 4) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = p[(size_t)(z + u) * n4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { a.x += v[u].x; a.y += v[u].y; a.z += v[u].z; a.w += v[u].w; }
    }
    for (; z < Z; ++z) {
      const float4 v = p[(size_t)z * n4];
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    out[i] = a;
  }
}

// out[r][c] = sum_z part[z][r][c] + bias[c]   (the split-K remainder rows of a training Linear; bias may be null)
// (amax: optional absmax slot of these rows, as gemm_f16x2_dyn_kernel's)
__global__ __launch_bounds__(256) void sum_partials_bias_kernel(const float* __restrict__ part, const float* __restrict__ bias,
                                                                float* __restrict__ out, size_t n, int N, int Z,
                                                                unsigned* __restrict__ amax, int amax_pos) {
  __shared__ float pm[4];
  float m = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float a = part[i];
    for (int z = 1; z < Z; ++z) a += part[(size_t)z * n + i];
    a = bias ? a + bias[i % N] : a;
    out[i] = a;
    m = fmaxf(m, amax_pos ? a : fabsf(a));
  }
  if (amax) {
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) pm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(amax, __float_as_uint(fmaxf(fmaxf(pm[0], pm[1]), fmaxf(pm[2], pm[3]))));
  }
}

}  // namespace

// ---- training-step launchers (gemm_f16x2_dyn_kernel and its operand kernels) ---------------------------------------
// out_z[M, N] = A2 (chunk z) . W2 (chunk z)^T x dynA x dynW (+ bias): Kfull = Z NKz 32 columns per operand row
int d3dp_launch_linear_f16x2_dyn(const void* A2, const void* W2, const float* bias, const float* dynA, const float* dynW,
                                 float* out, int M, int N, int Kfull, int Z, hipStream_t st, unsigned* amax_out, int amax_pos,
                                 int rem_blocks, int passes, int rows_hi) {
  if (M <= 0 || N % 4 != 0 || Z < 1 || Kfull % (XBK * Z) != 0 || (amax_out && Z != 1) || (passes != 1 && passes != 3)) return -1;
  // hi-only rows: a stage is a 128-byte line of 64 k, so every chunk of the contraction is a whole number of k-step PAIRS -- the
  // grouping of the one-pass form on split rows is kept or the launch is refused, never regrouped
  if (rows_hi && (passes != 1 || Kfull % (2 * XBK * Z) != 0)) return -1;
  const int NKz = Kfull / XBK / Z;
  // rem_blocks: the rows behind the last whole 256-row tile as 16 x 64 blocks at the end of the kernel (see there)
  const bool rem = rem_blocks && Z == 1 && M > XBM && M % XBM != 0 && NKz % (2 * XNCW) == 0;
  const int tm = rem ? M / XBM : (M + XBM - 1) / XBM, tn = (N + XBN - 1) / XBN;
  static PerDeviceOnce once, once1, once_hi;           // (one opt-in per kernel: the one-pass twins ask when they are first launched)
  const auto kern = rows_hi ? gemm_f16x2_dyn_kernel<1, true> : passes == 1 ? gemm_f16x2_dyn_kernel<1> : gemm_f16x2_dyn_kernel<3>;
  const int cus = (rows_hi ? once_hi : passes == 1 ? once1 : once).get([&](int dev) {
    return d3dp_lds_opt_in(reinterpret_cast<const void*>(kern), XNSTAGE * XSTAGE + 64) < 0 ? -3 : d3dp_cu_count(dev);
  });
  if (cus < 0) return -3;
  const int items = tm * tn * Z, grid = items < cus ? items : cus;
  hipLaunchKernelGGL(kern, dim3(grid), dim3((XNCW + 4) * 64), XNSTAGE * XSTAGE + 64, st, (const f16*)A2,
                     (const f16*)W2, bias, dynA, dynW, out, M, N, Kfull, NKz, tn, tm * tn, items, amax_out, amax_pos,
                     rem ? tm * XBM : 0);
  return 0;
}

void d3dp_launch_split2_dyn(const float* src, void* dst, int R, int C, int Cpad, const unsigned* amax, float* unscale,
                            hipStream_t st, int rows_hi) {
  const size_t n = (size_t)R * (Cpad / 8);
  const unsigned blocks = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL((rows_hi ? split2h_dyn_kernel<true> : split2h_dyn_kernel<false>), dim3(blocks ? blocks : 1), dim3(256), 0, st, src, (f16*)dst, R, C, Cpad, amax, unscale);
}

void d3dp_launch_split2_t_dyn(const float* src, void* dst, int R, int C, int Rpad, const unsigned* amax, float* unscale,
                              hipStream_t st) {
  hipLaunchKernelGGL(split2h_t_dyn_kernel, dim3(Rpad / 32, (C + 31) / 32), dim3(256), 0, st, src, (f16*)dst, R, C, Rpad, amax,
                     unscale);
}

int d3dp_launch_dyprep(const float* src, void* drow, void* dcol, float* colpart, int R, int C, int Rpad, const unsigned* amax,
                       float* unscale, hipStream_t st) {
  if (C % 32 != 0 || Rpad % 32 != 0 || Rpad < R) return -1;
  // one 192-row tile per workgroup where that needs at most D3DP_DYPREP_ROWS of them (configs[4]: 87 x C / 32 workgroups, all
  // resident at once); `colpart` always receives D3DP_DYPREP_ROWS rows (workgroup rows without a tile write zeros)
  hipLaunchKernelGGL(dyprep_kernel, dim3(D3DP_DYPREP_ROWS, C / 32), dim3(256), 0, st, src, (f16*)drow, (f16*)dcol, colpart, R, C, Rpad, amax, unscale);
  return 0;
}

// the row form alone (+ column sums): see rowprep_kernel.  *rows = partial rows written to colpart (<= D3DP_ROWPREP_ROWS)
int d3dp_launch_rowprep_ln(const float* src, const float* w, const float* b, float eps, void* drow, int R, int Rpad, int C,
                           const unsigned* amax, float* unscale, hipStream_t st, int rows_hi) {
  if (C % 32 != 0 || C > 512 || Rpad < R || !w || !b) return -1;
  int g = (Rpad + 3) / 4;
  if (g > 1024) g = 1024;
  hipLaunchKernelGGL((rows_hi ? rowprep_ln_kernel<true> : rowprep_ln_kernel<false>), dim3(g), dim3(256), 0, st, src, w, b, eps, (f16*)drow, R, Rpad, C, amax, unscale);
  return 0;
}

int d3dp_launch_rowprep(const float* src, void* drow, float* colpart, int* rows, int R, int Rpad, int C, const unsigned* amax,
                        float* unscale, hipStream_t st, const float* mask, int axis, int F, int J, const float* gelu_pre, int rows_hi) {
  if (C % 32 != 0 || Rpad < R || C > 1536) return -1;      // (P = ceil(C / 512) column passes; a lane whose 8 columns lie behind C idles)
  int g = (Rpad + 3) / 4;
  const int cap = colpart ? D3DP_ROWPREP_ROWS : 1024;   // (every workgroup leaves one partial row of column sums)
  if (g > cap) g = cap;
  if (rows) *rows = g;
  const int P = (C + 511) / 512;
  f16* d = (f16*)drow;
  if (mask && (J < 1 || F < 1)) return -1;
#define D3DP_ROWPREP(PP, GG) hipLaunchKernelGGL((rows_hi ? rowprep_kernel<PP, GG, true> : rowprep_kernel<PP, GG, false>), dim3(g), dim3(256), 0, st, src, d, colpart, R, Rpad, C, amax, unscale, mask, axis, F, J, gelu_pre)
  if (gelu_pre) {
    if (P == 1) D3DP_ROWPREP(1, true); else if (P == 2) D3DP_ROWPREP(2, true); else D3DP_ROWPREP(3, true);
  } else {
    if (P == 1) D3DP_ROWPREP(1, false); else if (P == 2) D3DP_ROWPREP(2, false); else D3DP_ROWPREP(3, false);
  }
#undef D3DP_ROWPREP
  return 0;
}

int d3dp_launch_gelu_rowprep(const float* src, void* drow, int R, int Rpad, int C, const unsigned* pmax, unsigned* amax_out,
                             float* unscale, hipStream_t st, int rows_hi) {
  if (C % 32 != 0 || Rpad < R) return -1;
  const size_t n = (size_t)Rpad * (C / 8);
  const unsigned blocks = (unsigned)((n + 511) / 512 < 2048 ? (n + 511) / 512 : 2048);
  hipLaunchKernelGGL((rows_hi ? gelu_rowprep_kernel<true> : gelu_rowprep_kernel<false>), dim3(blocks ? blocks : 1), dim3(256), 0, st, src, (f16*)drow, R, Rpad, C, pmax, amax_out, unscale);
  return 0;
}

// out_z[N, K] = sum over the token rows of chunk z of A2[t][n] W2[t][k], x dynA x dynW: Tp = Z NKz 32 rows per operand (rows
// beyond the real ones zero), N % 256 == 0, K % 128 == 0 (d3dp_tn_applies)
static_assert(XBM == D3DP_TN_TILE_N && XBN == D3DP_TN_TILE_K, "train_plan.h: the tile d3dp_tn_applies asks whole multiples of");
// n products over the same Tp token rows in one launch: out_p,z[N_p, K_p] (z = 0 .. Z - 1, N_p K_p floats apart)
int d3dp_launch_linear_f16x2_tn_many(const D3dpTnProduct* prods, int n, int Tp, int Z, hipStream_t st, int passes, int rows_hi) {
  if (n < 1 || n > D3DP_TN_MAX || Z < 1 || Tp % (XBK * Z) != 0 || (passes != 1 && passes != 3) || (rows_hi && passes != 1)) return -1;
  D3dpTnTable tb{};
  tb.n = n;
  int tiles = 0;
  for (int i = 0; i < n; ++i) {
    tb.p[i] = prods[i];
    if (!d3dp_tn_applies(tb.p[i].N, tb.p[i].K)) return -1;
    tb.p[i].tiles_k = tb.p[i].K / XBN;
    tb.p[i].tile0 = tiles;
    tiles += (tb.p[i].N / XBM) * tb.p[i].tiles_k;
  }
  const int NKz = Tp / XBK / Z;
  static PerDeviceOnce once, once1, once_hi;
  const auto kern = rows_hi ? gemm_f16x2_tn_kernel<1, true> : passes == 1 ? gemm_f16x2_tn_kernel<1> : gemm_f16x2_tn_kernel<3>;
  const int lds = XNSTAGE * (rows_hi ? XTN_HI_STAGE : XSTAGE);
  const int cus = (rows_hi ? once_hi : passes == 1 ? once1 : once).get([&](int dev) {
    return d3dp_lds_opt_in(reinterpret_cast<const void*>(kern), lds) < 0 ? -3 : d3dp_cu_count(dev);
  });
  if (cus < 0) return -3;
  const int items = tiles * Z, grid = items < cus ? items : cus;
  hipLaunchKernelGGL(kern, dim3(grid), dim3((XNCW + 4) * 64), lds, st, tb, NKz, tiles, items);
  return 0;
}
int d3dp_launch_linear_f16x2_tn(const void* A2, const void* W2, const float* dynA, const float* dynW, float* out, int N, int K,
                                int Tp, int Z, hipStream_t st, int passes, int rows_hi) {
  const D3dpTnProduct one{A2, W2, dynA, dynW, out, N, K, 0, 0};
  return d3dp_launch_linear_f16x2_tn_many(&one, 1, Tp, Z, st, passes, rows_hi);
}

int d3dp_launch_wprep(const D3dpWPrepTable& tb, void* rows_base, void* cols_base, unsigned* amax, float* unscale, hipStream_t st,
                      int rows_hi) {
  if (tb.n < 1 || tb.n > D3DP_WPREP_MAX) return -1;
  for (int i = 0; i < tb.n; ++i)
    if (tb.it[i].N % 32 != 0 || tb.it[i].K % 32 != 0) return -1;
  hipLaunchKernelGGL(wprep_absmax_kernel, dim3(16, tb.n), dim3(256), 0, st, tb, amax);
  hipLaunchKernelGGL((rows_hi ? wprep_rows_kernel<true> : wprep_rows_kernel<false>), dim3(32, tb.n), dim3(256), 0, st, tb, (f16*)rows_base, (const unsigned*)amax, unscale);
  hipLaunchKernelGGL((rows_hi ? wprep_cols_kernel<true> : wprep_cols_kernel<false>), dim3(32, tb.n), dim3(256), 0, st, tb, (f16*)cols_base, (const unsigned*)amax);
  return 0;
}

void d3dp_launch_sum_partials_bias(const float* part, const float* bias, float* out, size_t n, int N, int Z, hipStream_t st,
                                   unsigned* amax, int amax_pos) {
  const unsigned cap = amax ? 256 : 2048;              // (with an absmax: one atomic per workgroup)
  const unsigned blocks = (unsigned)((n + 255) / 256 < cap ? (n + 255) / 256 : cap);
  hipLaunchKernelGGL(sum_partials_bias_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, st, part, bias, out, n, N, Z, amax, amax_pos);
}
void d3dp_launch_sum_partials_many(const D3dpSumTable& tb, hipStream_t st) {
  size_t most = 0;
  for (int i = 0; i < tb.n; ++i) most = tb.n4[i] > most ? tb.n4[i] : most;
  const unsigned blocks = (unsigned)((most + 255) / 256 < 1024 ? (most + 255) / 256 : 1024);
  hipLaunchKernelGGL(sum_partials_many_kernel, dim3(blocks ? blocks : 1, tb.n), dim3(256), 0, st, tb);
}
void d3dp_launch_sum_partials(const float* part, float* out, size_t n, int Z, hipStream_t st) {
  const size_t n4 = n / 4;                               // (n = N K of a Linear: a multiple of 4)
  const unsigned blocks = (unsigned)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048);
  hipLaunchKernelGGL(sum_partials_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, st, reinterpret_cast<const float4*>(part),
                     reinterpret_cast<float4*>(out), n4, Z);
}
