// EXACT-mode Linear layers on the fp16 matrix cores:  out[M,N] = epi((A . W^T) + bias), fp32-class accuracy.
// (reference: every nn.Linear on the path -- common/mixste.py:65 qkv, :80 proj, :38-41 fc1/fc2 -- which the reference
//  evaluates in fp32.)
//
// Operands are "f16x2" pairs (common.h): x 2^s = hi + lo, two fp16 values per element, A2 [M][K] (s = 4, fixed) and
// W2 [N][K] (s per matrix: max |w| 2^s in [2^13, 2^14)) in the LINE-INTERLEAVED layout "h2i" (common.h): a row is K/32
// blocks of 128 bytes, block kb = [hi of columns 32 kb .. 32 kb + 31 | lo of the same columns], so ONE k-step of ONE row --
// both planes -- is ONE 128-byte line.  `unscale` = 2^-(s_a + s_w) undoes both scales.  Per output element
// three v_mfma_f32_16x16x32_f16 passes into one fp32 accumulator,
//     acc += Wl.Ah + Wh.Al + Wh.Ah            out = acc unscale + bias,
// the lo.lo pass being below fp32 resolution (tools/err_budget_split.py;
// tests/test_hip_parity.py::test_linear_split_f16_is_fp32_class: mean error below torch's own fp32 matmul).
//
// Structure (the FAST kernel's, gemm.hip): persistent, 256x128 output tile per workgroup pass, BK = 32, 8 compute waves
// (4 x 2, 64x64 each = 4x4 MFMA tiles: 48 MFMA + 16 ds_read_b128 per k-step) + 4 LOADER waves.  Workgroups (<= one per
// CU) walk tiles L, L+G, ...; the A and W slabs (hi | lo of 32 columns per row: 48 KiB per k-step) stream through a 3-stage LDS ring
// as one continuous sequence of k-steps across tile boundaries.  Only the loader waves issue global_load_lds
// (1 KiB pieces of 8 rows x 128 B = 8 whole lines, 12 per wave and k-step; round 2 had two separate planes and pieces of
// 16 rows x 64 B = 16 half lines: the kernel is bound by the line-request rate of the CU's vector memory path,
// profiles/r03_gemm_l2_prefetch.md, and the interleaved layout halves the requests for the same bytes) and wait on
// vmcnt (counted: one k-step stays in flight across
// every barrier); measured on the two earlier structures of this kernel in which every wave loaded AND computed
// (profiles/r02_gemm_x2_structures_pmc.md): half of all wave cycles were issue stalls with the matrix pipe a third
// busy -- an LDS-DMA costs 100-185 issue cycles beside ds_reads -- so the compute waves must not carry them, and the
// 168-register budget of a 12-wave workgroup is why there is ONE accumulator set (lo planes unscaled) instead of a
// separate accumulator for the cross terms.  One raw s_barrier per k-step.  Compute waves never wait on vmcnt, so
// their epilogue stores (which also count in vmcnt) cannot stall the operand pipeline; the loaders keep prefetching
// the next tile's slabs while the epilogue runs.
// Output stores: the activation fragment is the MFMA A operand, so a lane holds C[row 4 fg + r][column fi] of each 16x16
// tile, and the loader permutes the W rows of a 64-column strip (LDS row ni*16 + i carries column 4 i + ni) so that the
// lane's four tiles ni are four CONSECUTIVE columns: one 16-byte store per (mi, r) in which the 16 lanes of a group cover
// 256 contiguous bytes of ONE row -- every store instruction writes whole 128-byte lines.  (First version: transposed
// product, 16 columns per lane, each store instruction touching 64 different lines with 16 bytes: the tile-end store
// tail cost 11-17 us per 256x128 tile against 18-22 us for its 16 k-steps, fitted over the four Linear shapes.)
//   EPI_BIAS     -> fp32 out (feeds the residual-adding row kernels)
//   EPI_GELU     -> GELU (rational erf, common.h) re-split into the h2i rows of the fc2 operand
//   EPI_QKV_PACK -> q fp32, k and v as fp16 planes: the packed rows the split-fp16 attention kernels read (attention_x2.hip)
//   EPI_RESID    -> x += A W^T + b in place on the fp32 residual stream (proj, fc2: mixste.py:113-115)
//   EPI_RESID_NORM -> EPI_RESID behind a DEFERRED LayerNorm of the residual row: x = LN(x) + A W^T + b, the LayerNorm's (mean, rstd)
//                   per row left by the row kernel in front (pointwise.hip ln2_defer_kernel), its gamma / beta behind the bias: the
//                   proj Linear behind a block boundary, whose norm pair then does not rewrite x
//   EPI_RESID_LN -> the same as EPI_RESID, and the sum leaves a second time as the NEXT Linear's split-fp16 operand (un-normalised) together
//                   with (mean, M2) of each 64-column slice of each row: the statistics of the LayerNorm that follows
//   EPI_GELU_LN  -> EPI_GELU of a Linear with that LayerNorm folded in: LN(x) W^T + b = rstd (x W'^T - mean c1) + c2 with
//                   W' = W diag(gamma), c1 = W' 1, c2 = W beta + b -- norm2 + fc1 (mixste.py:115) without a row kernel in between
// Plane outputs leave as ONE 16-byte store per lane too (neighbouring lanes swap halves, store_planes_paired).
// The kernel is closed by measurement, and the compile-time switches it was measured with are gone from the source; their
// results are the record:
//   timing probes (loads / stores / MFMAs / barriers compiled out one at a time, staggered workgroup starts) and what they say
//     about the clock the chip sustains under this instruction mix: profiles/r02_gemm_probes.md, r03_gemm_probes.md, r04_gemm_probes.md;
//   cache-policy bits on the loaders' LDS-DMA (nt / sc0 / sc1): no gain, profiles/r06_nt_a_loads_ab.md;
//   the number of MFMAs lagged across the barrier (all twelve of row block 3 instead of eight: +-0) and a raised loader-wave
//     priority (+-0): the tables of DESIGN.md section 7; the k-loop without lagged MFMAs: profiles/r02_gemm_probes.md;
//   scalar instead of packed GELU in the fc1 epilogue: profiles/r05_fc1_epilogue_isa.md; plain instead of nontemporal output
//     stores: profiles/r02_gemm_pmc.md.
// The training step's Linear (gemm_x2_train.hip) shares the tile geometry and LDS image of this kernel (gemm_x2_tile.h).
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "common.h"
#include "gemm_x2_tile.h"
#include "kernels.h"

// -DD3DP_X2_VARIANTS=1 (tools/build_variant.sh variants ...; `make variants`): also build the MEASURED-NEGATIVE forms of this
// Linear (gemm_x2_variants.h) -- the ping-pong, wide (256 x 256) and row-class skewed kernels and the norm2-folding epilogues (EPI_RESID_LN /
// EPI_GELU_LN), DESIGN.md section 7 -- behind their D3DP_X2_PP / D3DP_X2_WIDE / D3DP_X2_SKEW / D3DP_FOLD_LN switches.  The
// product library is built without them: asking it for one fails loudly (d3dp_create: D3DP_ENOTSUP).
#ifndef D3DP_X2_VARIANTS
#define D3DP_X2_VARIANTS 0
#endif

// Output stores carry the nontemporal hint: the tile round's 4 MiB of output per XCD is not read again on that XCD
// and otherwise pushes the weight matrix out of the 4 MiB L2 between rounds (FETCH_SIZE measurement in DESIGN.md).
#define OUT_STORE(ptr, val) __builtin_nontemporal_store((val), (ptr))

namespace {

// Two fp16 planes of a 4-column group per lane -> ONE 16-byte store per lane: lanes 2j / 2j+1 hold neighbouring column
// groups of the same row; the even lane collects both hi halves (8 columns of the hi plane), the odd lane both lo halves.
// `dst`: where this lane's 16 bytes go (even lanes: own columns in the hi plane; odd lanes: the even neighbour's columns
// in the lo plane).
__device__ __forceinline__ void store_planes_paired(char* dst, f16x4 ph, f16x4 pl, bool odd, bool live) {
  const uint2 h = __builtin_bit_cast(uint2, ph), l = __builtin_bit_cast(uint2, pl);
  const uint2 send = odd ? h : l;
  uint2 recv;                                          // quad_perm [1,0,3,2]: the value of lane ^ 1
  recv.x = __builtin_amdgcn_update_dpp(0, (int)send.x, 0xB1, 0xF, 0xF, false);
  recv.y = __builtin_amdgcn_update_dpp(0, (int)send.y, 0xB1, 0xF, 0xF, false);
  using u32x4 = unsigned __attribute__((ext_vector_type(4)));
  const u32x4 out = odd ? (u32x4){recv.x, recv.y, l.x, l.y} : (u32x4){h.x, h.y, recv.x, recv.y};
  if (live) OUT_STORE(reinterpret_cast<u32x4*>(dst), out);
}

// TAG 1: the qkv Linear feeding the split-fp16 attention kernels -- packed output rows (see the epilogue); as its own
// kernel symbol rocprofv3 --stats also reports it separately from the proj Linear, which shares EPI with it.
template <int EPI, int TAG>
__global__ __launch_bounds__(768) void gemm_f16x2_kernel(const f16* __restrict__ A2, const f16* __restrict__ W2,
                                                         const float* __restrict__ bias, float unscale, float oscale,
                                                         float* __restrict__ outf, f16* __restrict__ out2,
                                                         float* __restrict__ aux, unsigned* __restrict__ flag, int M,
                                                         int N, int K, int tiles_n_arg, int total_tiles) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sbias = reinterpret_cast<float*>(smem + XNSTAGE * XSTAGE);
  const int G = gridDim.x;
  const int L = xcd_remap(blockIdx.x, G);
  const int n_my = (total_tiles - L + G - 1) / G;      // tiles L, L+G, ...
  const int NK = K / XBK;
  const int gtot = n_my * NK;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // tiles_n_arg < 0: the tiles from the LAST row of tiles to the first (X2_TILES_LAST_TO_FIRST: proj, whose consumer -- the
  // norm2 row kernel -- then starts on the rows written last)
  const int tiles_n = tiles_n_arg < 0 ? -tiles_n_arg : tiles_n_arg;
  const int t_flip = tiles_n_arg < 0 ? total_tiles - 1 : 0, t_sign = tiles_n_arg < 0 ? -1 : 1;
  auto tile_of = [&](int ti_) { return t_flip + t_sign * (L + ti_ * G); };

  for (int i = tid; i < (EPI == EPI_GELU_LN ? 2 * N : EPI == EPI_RESID_NORM ? 3 * N : N); i += (XNCW + 4) * 64) sbias[i] = bias[i];   // (GELU_LN: c2 | c1; RESID_NORM: b | gamma | beta)
  __syncthreads();

  if (wave >= XNCW) {
    // ------------------------------------------------------------------ loader waves
    const int lw = wave - XNCW;
    const int lr = lane >> 3, lq = lane & 7;           // row within an 8-row piece, physical 16-byte slot
    int ti = 0, ks = 0, slot = 0;                      // (tile, k-step, ring slot) of the next slab to issue
    const f16* pa[8];                                  // this lane's source slots of the current tile (k-step 0)
    const f16* pw[4];
    auto issue = [&]() {
      if (ks == 0) {                                   // new tile: row pointers once per tile, not per k-step
        const int t = tile_of(ti);
        const int m0 = (t / tiles_n) * XBM, n0 = (t % tiles_n) * XBN;
#pragma unroll
        for (int i = 0; i < 8; ++i) {                  // A pieces 8 lw .. 8 lw + 7 (8 rows each)
          const int row = (lw * 8 + i) * 8 + lr;
          pa[i] = A2 + (size_t)min(m0 + row, M - 1) * (2 * K) + swz128(row, lq) * 8;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {                  // W pieces 4 lw .. 4 lw + 3
          const int row = (lw * 4 + i) * 8 + lr;                        // LDS row of the W slab
          const int wrow = (row & 64) + colperm(row & 63);              // output column it carries
          pw[i] = W2 + (size_t)min(n0 + wrow, N - 1) * (2 * K) + swz128(row, lq) * 8;
        }
      }
      if constexpr (EPI == EPI_GELU_LN || EPI == EPI_RESID_NORM) {
        // the tile's 256 (mean, rstd) pairs: 2 KiB = two pieces, by loader wave 0, the OLDEST operations of this k-step
        // (every counted wait below then covers them); buffer ti & 1 -- the epilogue of tile ti - 1 may still be reading
        if (ks == 0 && lw == 0) {
          const int t = tile_of(ti);
          const float* rs = aux + (size_t)(t / tiles_n) * XBM * 2 + lane * 4;     // (aux has 256 rows of slack: no clamp)
          char* dst = smem + XROWSTAT + (ti & 1) * (XBM * 8);
          __builtin_amdgcn_global_load_lds(GPTR(rs), LPTR(dst), 16, 0, 0);
          __builtin_amdgcn_global_load_lds(GPTR(rs + 256), LPTR(dst + 1024), 16, 0, 0);
        }
      }
      char* base = smem + slot * XSTAGE;
      const int ko = ks * (2 * XBK);                   // one k-step of a row = 64 fp16 (hi | lo)
#pragma unroll
      for (int i = 0; i < 8; ++i)
        __builtin_amdgcn_global_load_lds(GPTR(pa[i] + ko), LPTR(base + (lw * 8 + i) * 1024), 16, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        __builtin_amdgcn_global_load_lds(GPTR(pw[i] + ko), LPTR(base + XA_BYTES + (lw * 4 + i) * 1024), 16, 0, 0);
      if (++ks == NK) { ks = 0; ++ti; }
      slot = (slot == XNSTAGE - 1) ? 0 : slot + 1;
    };
    if (gtot > 0) issue();
    if (gtot > 1) issue();
    for (int g = 0; g < gtot; ++g) {
      // 12 glds per loader wave per k-step: loads(g) landed, loads(g+1) stay in flight
      if (g + 1 < gtot) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      X2_BARRIER();
      if (g + 2 < gtot) issue();                       // into the slot of k-step g-1: every wave has passed barrier g
    }
    return;
  }

  // -------------------------------------------------------------------- compute waves
  const int wr = wave >> 1, wc = wave & 1;
  const int fi = lane & 15, fg = lane >> 4;
  // per-lane fragment offsets inside a stage (the swizzle depends on the lane only: rows advance in multiples of 16);
  // the lo plane's slot is the hi plane's ^ 4, i.e. byte offset ^ 64
  const int offA = (wr * 64 + fi) * 128 + swz128(fi, fg) * 16, offAl = offA ^ 64;
  const int offW = XA_BYTES + (wc * 64 + fi) * 128 + swz128(fi, fg) * 16, offWl = offW ^ 64;
  f32x4 acc[4][4];
  __builtin_amdgcn_s_setprio(1);
  int slot = 0;
  for (int ti = 0; ti < n_my; ++ti) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // The last two products of row block 3 (al.wh, ah.wh: 8 MFMAs) are issued AFTER the next k-step's barrier, behind
    // that step's first fragment reads: they cover the LDS latency that otherwise idles the matrix pipe after every
    // barrier release (all waves of the workgroup read at once).  Their operands stay in 24 registers across the
    // barrier; the k-loop is unrolled by two so that the two fragment sets swap roles without register copies.
    f16x8 wfa[4][2], wfb[4][2], taa[2], tab[2];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) wfb[ni][0] = wfb[ni][1] = (f16x8){};
    tab[0] = tab[1] = (f16x8){};
    auto kstep = [&](f16x8 (&wf)[4][2], f16x8 (&ta)[2], const f16x8 (&pw)[4][2], const f16x8 (&pa)[2]) {
      __builtin_amdgcn_s_waitcnt(0xc07f);              // lgkmcnt(0): this wave has read everything it wanted from the old slot
      X2_BARRIER();
      __builtin_amdgcn_sched_barrier(0);
      const char* sb = smem + slot * XSTAGE;
      slot = (slot == XNSTAGE - 1) ? 0 : slot + 1;
      f16x8 ah[2], al[2];
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
          wf[ni][pl] = *reinterpret_cast<const f16x8*>(sb + (pl ? offWl : offW) + ni * 2048);
      ah[0] = *reinterpret_cast<const f16x8*>(sb + offA);
      al[0] = *reinterpret_cast<const f16x8*>(sb + offAl);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[3][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pa[1], pw[ni][0], acc[3][ni], 0, 0, 0);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[3][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pa[0], pw[ni][0], acc[3][ni], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int mi = 0; mi < 3; ++mi) {
        const int b = mi & 1;
        if (mi < 2) {                                  // next row block's fragments while this one multiplies
          ah[b ^ 1] = *reinterpret_cast<const f16x8*>(sb + offA + (mi + 1) * 2048);
          al[b ^ 1] = *reinterpret_cast<const f16x8*>(sb + offAl + (mi + 1) * 2048);
        } else {
          ta[0] = *reinterpret_cast<const f16x8*>(sb + offA + 3 * 2048);
          ta[1] = *reinterpret_cast<const f16x8*>(sb + offAl + 3 * 2048);
        }
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[b], wf[ni][1], acc[mi][ni], 0, 0, 0);
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[b], wf[ni][0], acc[mi][ni], 0, 0, 0);
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[b], wf[ni][0], acc[mi][ni], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[3][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ta[0], wf[ni][1], acc[3][ni], 0, 0, 0);
    };
#pragma unroll 1
    for (int ks = 0; ks < NK; ks += 2) {               // NK is even (K % 64 == 0, checked by the launcher)
      kstep(wfa, taa, wfb, tab);
      kstep(wfb, tab, wfa, taa);
    }
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[3][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(tab[1], wfb[ni][0], acc[3][ni], 0, 0, 0);
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[3][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(tab[0], wfb[ni][0], acc[3][ni], 0, 0, 0);
    // ---- tile epilogue: lane holds out[m = pm0 + mi*16 + r][n = nb + ni], pm0 = tile row + wr*64 + 4 fg, nb = tile column
    // + wc*64 + 4 fi.  Every store address is  uniform base + 32-bit lane offset  (the launcher refuses outputs of 4 GiB or
    // more), advanced row by row: per-row 64-bit address arithmetic was most of the epilogue's VALU work, and it runs
    // with the matrix pipes idle.
    const int t = tile_of(ti);
    const int pm0 = (t / tiles_n) * XBM + wr * 64 + 4 * fg, nb = (t % tiles_n) * XBN + wc * 64 + 4 * fi;
    if (nb < N) {
      const float4 bz = *reinterpret_cast<const float4*>(sbias + nb);
      const bool odd = fi & 1;
      unsigned off, pitch;
      bool planes;                                     // split the values and store fp16 planes (else fp32)
      char* base = reinterpret_cast<char*>(outf);
      const int c0 = nb & ~7;                          // h2i rows: 4 N bytes per row; the lane pair's 8 columns start at c0:
      const unsigned offp = (unsigned)pm0 * (N * 4) + (c0 >> 5) * 128 + (c0 & 31) * 2 + (odd ? 64 : 0);   // even lane -> hi slot, odd -> lo
      if constexpr (EPI == EPI_GELU || EPI == EPI_GELU_LN) {   // the fc2 operand
        base = reinterpret_cast<char*>(out2);
        pitch = N * 4; planes = true;
        off = offp - (unsigned)pm0 * pitch;
      } else if constexpr (TAG == 1) {
        // packed qkv row (12 C bytes, C = N / 3): q fp32 | k hi | k lo | v hi | v lo (fp16 planes x 16) -- the
        // K / V operand images of the split-fp16 attention kernels, which copy them into LDS without touching them
        const int C = N / 3, region = nb / C, cn = nb - region * C;      // a wave's 64 columns lie in one region
        pitch = N * 4; planes = region != 0;
        off = planes ? region * 4 * C + cn * 2 + (odd ? 2 * C - 8 : 0) : cn * 4;
      } else {
        pitch = N * 4; planes = false;
        off = nb * 4;
      }
      off += (unsigned)pm0 * pitch;
      const int rows = M - pm0;                        // row k = mi*16 + r of this lane exists iff k < rows
      [[maybe_unused]] float4 c1z = {};
      [[maybe_unused]] const float* srow = nullptr;
      if constexpr (EPI == EPI_GELU_LN) {
        c1z = *reinterpret_cast<const float4*>(sbias + N + nb);
        srow = reinterpret_cast<const float*>(smem + XROWSTAT + (ti & 1) * (XBM * 8)) + (wr * 64 + 4 * fg) * 2;
      }
      [[maybe_unused]] float4 gmz = {}, btz = {};      // EPI_RESID_NORM: gamma / beta of the lane's four columns
      if constexpr (EPI == EPI_RESID_NORM) {
        gmz = *reinterpret_cast<const float4*>(sbias + N + nb);
        btz = *reinterpret_cast<const float4*>(sbias + 2 * N + nb);
        srow = reinterpret_cast<const float*>(smem + XROWSTAT + (ti & 1) * (XBM * 8)) + (wr * 64 + 4 * fg) * 2;
      }
      auto value = [&](int mi, int r, int e) {
        const float bze = e == 0 ? bz.x : e == 1 ? bz.y : e == 2 ? bz.z : bz.w;
        if constexpr (EPI == EPI_GELU_LN) {            // rstd (x W'^T - mean c1) + c2
          const float2 st = *reinterpret_cast<const float2*>(srow + (mi * 16 + r) * 2);
          const float c1e = e == 0 ? c1z.x : e == 1 ? c1z.y : e == 2 ? c1z.z : c1z.w;
          return fmaf(st.y, fmaf(acc[mi][e][r], unscale, -(st.x * c1e)), bze);
        } else {
          return fmaf(acc[mi][e][r], unscale, bze);
        }
      };
      auto store_rows = [&](auto planes_c, auto checked_c) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int k = mi * 16 + r;
            const bool live = !decltype(checked_c)::value || k < rows;
            char* dst = base + (off + (unsigned)k * pitch);
            if constexpr (decltype(planes_c)::value) {
              f16x4 ph, pl;
              float v[4] = {value(mi, r, 0), value(mi, r, 1), value(mi, r, 2), value(mi, r, 3)};
              if constexpr (EPI == EPI_GELU || EPI == EPI_GELU_LN) {
                // two elements at a time on v_pk_fma_f32 (the epilogue runs with no MFMA in flight): -45 ms of the 1387 ms
                // fc1 class per step
                const f32x2 g0 = gelu_erf_rational2((f32x2){v[0], v[1]}), g1 = gelu_erf_rational2((f32x2){v[2], v[3]});
                v[0] = g0.x; v[1] = g0.y; v[2] = g1.x; v[3] = g1.y;
              }
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                f16 h, l;
                split2h_scaled(v[e] * oscale, h, l);       // (oscale: the consumer's operand scale, 2^4 unless capi_weights.hip lowered it)
                ph[e] = h; pl[e] = l;
              }
              store_planes_paired(dst, ph, pl, odd, live);
            } else if constexpr (EPI != EPI_RESID && EPI != EPI_RESID_LN && EPI != EPI_RESID_NORM) {
              if (live) OUT_STORE(reinterpret_cast<f32x4*>(dst), ((f32x4){value(mi, r, 0), value(mi, r, 1), value(mi, r, 2), value(mi, r, 3)}));
            }
          }
        if constexpr (EPI == EPI_RESID && !decltype(planes_c)::value) {
          // x += A W^T + b in place (the residual stream): all sixteen reads of the tile in flight before the first add
          f32x4 res[4][4];
#pragma unroll
          for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int k = mi * 16 + r;
              const bool live = !decltype(checked_c)::value || k < rows;
              res[mi][r] = (f32x4){0.f, 0.f, 0.f, 0.f};
              if (live) res[mi][r] = *reinterpret_cast<const f32x4*>(base + (off + (unsigned)k * pitch));
            }
#pragma unroll
          for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int k = mi * 16 + r;
              const bool live = !decltype(checked_c)::value || k < rows;
              const f32x4 v = {res[mi][r][0] + value(mi, r, 0), res[mi][r][1] + value(mi, r, 1),
                               res[mi][r][2] + value(mi, r, 2), res[mi][r][3] + value(mi, r, 3)};
              if (live) *reinterpret_cast<f32x4*>(base + (off + (unsigned)k * pitch)) = v;   // (re-read by the next row kernel: no nt hint)
            }
        }
        if constexpr (EPI == EPI_RESID_NORM && !decltype(planes_c)::value) {
          // x = LN(x) + A W^T + b in place.  gamma, beta and a row's statistics beside the accumulators leave room for twelve of
          // the sixteen row reads (168 registers, 12-wave workgroup): row blocks 0 - 2 are in flight before the first add, and row
          // block 3 is read into block 0's registers once block 0 has left.
          f32x4 res[3][4];
          auto read_block = [&](int mi, f32x4 (&dstv)[4]) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int k = mi * 16 + r;
              const bool live = !decltype(checked_c)::value || k < rows;
              dstv[r] = (f32x4){0.f, 0.f, 0.f, 0.f};
              if (live) dstv[r] = *reinterpret_cast<const f32x4*>(base + (off + (unsigned)k * pitch));
            }
          };
#pragma unroll
          for (int mi = 0; mi < 3; ++mi) read_block(mi, res[mi]);
#pragma unroll
          for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int k = mi * 16 + r;
              const bool live = !decltype(checked_c)::value || k < rows;
              // the deferred LayerNorm of the residual row, as Row<C>::norm (pointwise.hip) writes it: subtract, multiply, fma --
              // on the x the row kernel read and the (mean, rstd) it left, so the bits it would have stored over x
              const float2 st = *reinterpret_cast<const float2*>(srow + k * 2);
              const f32x4 x = res[mi % 3][r];
              const f32x4 v = {fmaf((x[0] - st.x) * st.y, gmz.x, btz.x) + value(mi, r, 0), fmaf((x[1] - st.x) * st.y, gmz.y, btz.y) + value(mi, r, 1),
                               fmaf((x[2] - st.x) * st.y, gmz.z, btz.z) + value(mi, r, 2), fmaf((x[3] - st.x) * st.y, gmz.w, btz.w) + value(mi, r, 3)};
              if (live) *reinterpret_cast<f32x4*>(base + (off + (unsigned)k * pitch)) = v;   // (re-read by the next row kernel: no nt hint)
            }
            if (mi == 0) {
              __builtin_amdgcn_sched_barrier(0);
              read_block(3, res[0]);
            }
          }
        }
        if constexpr (EPI == EPI_RESID_LN && !decltype(planes_c)::value) {
          // x += A W^T + b in place, in two halves of eight rows per lane (the sums stay in registers for what follows, and
          // sixteen reads + sixteen sums + the accumulators would not fit the 168 registers of a 12-wave workgroup); each
          // sum leaves a second time as the next Linear's operand (un-normalised, x 16, h2i), and the 16 lanes of a row
          // group, which hold a row's 64 values, reduce (mean, M2) of this wave's slice of every row: two passes in registers,
          // butterfly over the DPP row (xor 1, xor 2, half mirror, mirror: every lane ends with the sum)
          auto rowsum16 = [](float x) {
            x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, false));
            x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x4E, 0xF, 0xF, false));
            x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x141, 0xF, 0xF, false));
            x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x140, 0xF, 0xF, false));
            return x;
          };
          const int S = (N + 63) >> 6, slice = nb >> 6;
          float* sdst = aux + ((size_t)pm0 * S + slice) * 2;
          bool over = false;
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            f32x4 res[2][4];
#pragma unroll
            for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int k = (half * 2 + m2) * 16 + r;
                const bool live = !decltype(checked_c)::value || k < rows;
                res[m2][r] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (live) res[m2][r] = *reinterpret_cast<const f32x4*>(base + (off + (unsigned)k * pitch));
              }
#pragma unroll
            for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int mi = half * 2 + m2, k = mi * 16 + r;
                const bool live = !decltype(checked_c)::value || k < rows;
                const f32x4 v = {res[m2][r][0] + value(mi, r, 0), res[m2][r][1] + value(mi, r, 1),
                                 res[m2][r][2] + value(mi, r, 2), res[m2][r][3] + value(mi, r, 3)};
                if (live) *reinterpret_cast<f32x4*>(base + (off + (unsigned)k * pitch)) = v;
                f16x4 ph, pl;
#pragma unroll
                for (int e = 0; e < 4; ++e) { f16 h, l; split2h_scaled(v[e] * oscale, h, l); ph[e] = h; pl[e] = l; }
                store_planes_paired(reinterpret_cast<char*>(out2) + (offp + (unsigned)k * (N * 4)), ph, pl, odd, live);
                // exact range check of the un-normalised operand (its magnitude has no useful bound from the weights alone)
                over |= !(fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))) * oscale < 65504.0f);
                const float mean = rowsum16((v[0] + v[1]) + (v[2] + v[3])) * (1.0f / 64.0f);
                const float d0 = v[0] - mean, d1 = v[1] - mean, d2 = v[2] - mean, d3 = v[3] - mean;
                const float q2 = rowsum16(fmaf(d0, d0, d1 * d1) + fmaf(d2, d2, d3 * d3));
                if (live && fi == 0) *reinterpret_cast<float2*>(sdst + (size_t)k * S * 2) = make_float2(mean, q2);
              }
          }
          if (__builtin_expect(__any(over), 0) && lane == 0) atomicOr(flag, 2u);   // d3dp_status: operand left the split range
        }
      };
      using T_ = std::true_type; using F_ = std::false_type;
      constexpr bool kPlanesOnly = EPI == EPI_GELU || EPI == EPI_GELU_LN;
      if (rows >= 64) {                                // (all but the last row of tiles)
        if (planes) { if constexpr (kPlanesOnly || TAG == 1) store_rows(T_{}, F_{}); }
        else { if constexpr (!kPlanesOnly) store_rows(F_{}, F_{}); }
      } else {
        if (planes) { if constexpr (kPlanesOnly || TAG == 1) store_rows(T_{}, T_{}); }
        else { if constexpr (!kPlanesOnly) store_rows(F_{}, T_{}); }
      }
    }
  }
}

// src[i] * scale -> h2i layout (common.h): blocks of 32 elements, dst[64 b .. 64 b + 31] = hi, dst[64 b + 32 .. 64 b + 63] = lo
// of elements 32 b .. 32 b + 31 (n % 32 == 0; any row length that is a multiple of 32)
__global__ void split2h_kernel(const float* __restrict__ s, f16* __restrict__ d, size_t n, float scale) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    f16 a, b;
    split2h_scaled(s[i] * scale, a, b);
    const size_t o = (i >> 5) * 64 + (i & 31);
    d[o] = a; d[o + 32] = b;
  }
}

// out[0] = max |src[i]| (as the bit pattern of a non-negative float: integer max == float max); out pre-zeroed.
// One atomic per WORKGROUP (the training step calls this three hundred times per step: with one atomic per wave the 4,096
// same-address atomics of a 34 MB tensor took 56 us, five times the read itself -- profiles/r04_train_step_kernel_stats.md)
__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ s, size_t n, unsigned* __restrict__ out) {
  __shared__ float part[4];
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  float m = 0.f;
  const size_t n4 = n / 4;
  const float4* s4 = reinterpret_cast<const float4*>(s);   // (operands are 16-byte aligned: whole tensors)
  auto amax4 = [](const float4 v) { return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))); };
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {         // four independent 16-byte loads in flight per thread
    const float4 v0 = s4[i], v1 = s4[i + stride], v2 = s4[i + 2 * stride], v3 = s4[i + 3 * stride];
    m = fmaxf(m, fmaxf(fmaxf(amax4(v0), amax4(v1)), fmaxf(amax4(v2), amax4(v3))));
  }
  for (; i < n4; i += stride) m = fmaxf(m, amax4(s4[i]));
  for (size_t j = n4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) m = fmaxf(m, fabsf(s[j]));
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(out, __float_as_uint(fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]))));
}

// see kernels.h (d3dp_launch_rowbound): one wave per row of W; fp32 sums of non-negative terms, rounded UP by a margin
// that covers their accumulated rounding (K <= 2048 terms: relative error < 2^-12)
__global__ void rowbound_kernel(const float* __restrict__ W, const float* __restrict__ gamma, const float* __restrict__ beta,
                                const float* __restrict__ bias, int N, int K, float sq, unsigned* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (n >= N) return;
  float a = 0.f, inmax = 0.f;
  for (int k = lane; k < K; k += 64) {
    const float in = fmaf(sq, fabsf(gamma[k]), fabsf(beta[k]));
    inmax = fmaxf(inmax, in);
    a = fmaf(fabsf(W[(size_t)n * K + k]), in, a);
  }
  a = wave_sum(a);
  inmax = wave_max(inmax);
  if (lane == 0) {
    atomicMax(out, __float_as_uint((a + fabsf(bias[n])) * 1.001f));
    atomicMax(out + 1, __float_as_uint(inmax * 1.001f));
  }
}

__global__ void nonfinite_flag_kernel(const float* __restrict__ x, size_t n, unsigned* __restrict__ flag) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  bool bad = false;
  for (; i < n; i += stride) bad |= !(fabsf(x[i]) <= 3.0e38f);
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

}  // namespace

bool d3dp_x2_variants_built() { return D3DP_X2_VARIANTS != 0; }

// The experimental kernels with their dispatcher x2_variants_launch, d3dp_x2_skew_applies and the two norm2-folding launchers;
// the product library answers for them: the schedule never applies, and capi_denoise.hip never reaches the launchers without a
// variants build.
#if D3DP_X2_VARIANTS
#include "gemm_x2_variants.h"
#else
bool d3dp_x2_skew_applies(int, int, int, int, int, int) { return false; }
void d3dp_launch_ln_combine(const float*, float*, int, int, float, hipStream_t) {}
void d3dp_launch_fold_ln(const float*, const float*, const float*, const float*, float*, float*, int, int, hipStream_t) {}
#endif

// out = epi((A W^T) unscale + bias) with A2/W2 split-fp16 operands in the h2i layout; EPI_BIAS: fp32 `outf`; EPI_GELU: `out2` in the h2i layout [M][N] (the fc2 operand);
// EPI_QKV_PACK (N = 3 C, C % 64 == 0): `outf` rows of 12 C bytes = q fp32 | k hi | k lo | v hi | v lo (fp16 x 16);
// EPI_RESID: `outf` [M, N] fp32 is read and written (outf += ...).
// EPI_RESID_NORM: the same with outf's rows normalised first: bias = [b | gamma | beta], aux = [M + 256][2] (mean, rstd) per row.
// `unscale` = 1 / (scale of the A planes * scale of the W planes).
// K must be a multiple of 64: the k-loop is unrolled by two k-steps of 32 (the lagged products alternate between two
// register sets), and the loader / compute waves count barriers per k-step.
// skew_d: 0 = the plain schedule; 1, 2, 4 = the row-class skewed kernel with its parked class leaving in that many k-steps
// (EPI_QKV_PACK and EPI_GELU only; falls back to the plain kernel where the schedule does not apply: see d3dp_x2_skew_applies)
int d3dp_launch_linear_f16x2(int epi, const void* A2, const void* W2, const float* bias, float unscale, float oscale,
                             float* outf, void* out2, float* aux, unsigned* flag, int M, int N, int K, hipStream_t st,
                             int skew_d, int pingpong) {
  const bool reverse = (pingpong & X2_TILES_LAST_TO_FIRST) != 0;   // (the plain kernel only)
  pingpong &= 0xff;
  if (K % (2 * XBK) != 0 || N % 4 != 0 || N > XBIAS_MAX || M <= 0) return -1;
  if ((size_t)M * N * 4 >= ((size_t)1 << 32)) return -1;   // 32-bit byte offsets in the epilogue
  if (epi != EPI_BIAS && epi != EPI_GELU && epi != EPI_QKV_PACK && epi != EPI_RESID && epi != EPI_RESID_LN &&
      epi != EPI_GELU_LN && epi != EPI_RESID_NORM) return -1;
  // the row statistics come through the two LDS buffers of EPI_GELU_LN (see below for the k-loop condition); b | gamma | beta in the bias area
  if (epi == EPI_RESID_NORM && (!aux || 3 * N > XBIAS_MAX || K / XBK < XNSTAGE)) return -1;
  if ((epi == EPI_RESID_LN || epi == EPI_GELU_LN) && (!aux || !out2)) return -1;
  if (epi == EPI_RESID_LN && !flag) return -1;
  if (epi == EPI_RESID_LN && N % 64 != 0) return -1;    // whole 64-column slices: every compute wave's columns exist
  if (epi == EPI_GELU_LN && 2 * N > XBIAS_MAX) return -1;   // c2 | c1 in the bias area
  if (epi == EPI_QKV_PACK && (N % 3 != 0 || (N / 3) % 64 != 0)) return -1;
  // h2i output rows are whole 32-column blocks of [hi | lo]: with N % 32 != 0 the lo half of the last block would land in
  // the next row; EPI_GELU_LN keeps two row-statistics buffers, which a k-loop shorter than the 3-stage
  // ring lets the loaders overwrite while the previous tile's epilogue reads them
  if ((epi == EPI_GELU || epi == EPI_GELU_LN || epi == EPI_RESID_LN) && N % 32 != 0) return -1;
  if (epi == EPI_GELU_LN && K / XBK < XNSTAGE) return -1;
  const int tm = (M + XBM - 1) / XBM, tn = (N + XBN - 1) / XBN;
  using KernT = void (*)(const f16*, const f16*, const float*, float, float, float*, f16*, float*, unsigned*, int, int, int, int, int);
#if D3DP_X2_VARIANTS
  constexpr int NKERN = 7;
  static const KernT kerns[NKERN] = {gemm_f16x2_kernel<EPI_BIAS, 0>, gemm_f16x2_kernel<EPI_BIAS, 1>,
                                     gemm_f16x2_kernel<EPI_GELU, 0>, gemm_f16x2_kernel<EPI_RESID, 0>,
                                     gemm_f16x2_kernel<EPI_RESID_NORM, 0>,
                                     gemm_f16x2_kernel<EPI_RESID_LN, 0>, gemm_f16x2_kernel<EPI_GELU_LN, 0>};
#else
  // the product library: the five epilogues the denoiser runs; everything else is a -DD3DP_X2_VARIANTS=1 build
  if (epi == EPI_RESID_LN || epi == EPI_GELU_LN || skew_d != 0 || pingpong != 0) return -2;
  constexpr int NKERN = 5;
  static const KernT kerns[NKERN] = {gemm_f16x2_kernel<EPI_BIAS, 0>, gemm_f16x2_kernel<EPI_BIAS, 1>,
                                     gemm_f16x2_kernel<EPI_GELU, 0>, gemm_f16x2_kernel<EPI_RESID, 0>,
                                     gemm_f16x2_kernel<EPI_RESID_NORM, 0>};
#endif
  // per DEVICE: the 156 KiB dynamic-LDS opt-in of every instantiation and the CU count (one process may drive several
  // devices: nn.DataParallel callers)
  static PerDeviceOnce once;
  const int cus = once.get([&](int dev) {
    for (int k = 0; k < NKERN; ++k)
      if (d3dp_lds_opt_in(reinterpret_cast<const void*>(kerns[k]), XLDS) < 0) return -3;
    return d3dp_cu_count(dev);
  });
  if (cus < 0) return -3;
  const int total = tm * tn, grid = total < cus ? total : cus;
#if D3DP_X2_VARIANTS
  // the experiment the call asks for, if any, takes it; otherwise (1) the plain kernel below
  const int taken = x2_variants_launch(epi, A2, W2, bias, unscale, oscale, outf, out2, aux, flag, M, N, K, st, skew_d, pingpong, cus);
  if (taken <= 0) return taken;
#endif
  const KernT kern = kerns[epi == EPI_GELU ? 2 : epi == EPI_RESID ? 3 : epi == EPI_QKV_PACK ? 1 : epi == EPI_RESID_NORM ? 4
                           : epi == EPI_RESID_LN ? 5 : epi == EPI_GELU_LN ? 6 : 0];   // (5, 6: the product library has refused them above)
  hipLaunchKernelGGL(kern, dim3(grid), dim3((XNCW + 4) * 64), XLDS, st, (const f16*)A2, (const f16*)W2, bias, unscale, oscale, outf,
                     (f16*)out2, aux, flag, M, N, K, reverse ? -tn : tn, total);
  return 0;
}

void d3dp_launch_split2(const float* src, void* dst, size_t n, float scale, hipStream_t st) {
  const unsigned blocks = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(split2h_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, st, src, (f16*)dst, n, scale);
}

void d3dp_launch_rowbound(const float* W, const float* gamma, const float* beta, const float* bias, int N, int K,
                          unsigned* out, hipStream_t st) {
  hipLaunchKernelGGL(rowbound_kernel, dim3((N + 3) / 4), dim3(256), 0, st, W, gamma, beta, bias, N, K,
                     sqrtf((float)(K - 1)) * 1.0001f, out);
}

void d3dp_launch_absmax(const float* src, size_t n, unsigned* out, hipStream_t st) {
  const unsigned blocks = (unsigned)((n / 4 + 255) / 256 < 512 ? (n / 4 + 255) / 256 : 512);
  hipLaunchKernelGGL(absmax_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, st, src, n, out);
}

void d3dp_launch_nonfinite_flag(const float* x, size_t n, unsigned* flag, hipStream_t st) {
  const unsigned blocks = (unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
  hipLaunchKernelGGL(nonfinite_flag_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, st, x, n, flag);
}

