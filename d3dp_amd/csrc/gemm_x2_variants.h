// The MEASURED-NEGATIVE forms of the EXACT Linear: the ping-pong, wide (256 x 256) and row-class skewed
// kernels, the kernels that go with the norm2-folding epilogues (EPI_RESID_LN / EPI_GELU_LN of gemm_f16x2_kernel), and the code
// that launches them.  Not a translation unit of its own: gemm_x2.hip includes this file, at file scope behind its own kernels,
// in a -DD3DP_X2_VARIANTS=1 build only (`make variants`: lib/variants/libd3dp_variants.so) -- the kernels here call
// x2_epilogue_at and instantiate gemm_f16x2_kernel's LayerNorm-folding epilogues.  The product library has none of this.
#pragma once

namespace {

// The tile epilogue of gemm_f16x2_kernel as a function, for a wave's 64 x 64 block at an explicit position: lane rows
// pm0 + mi*16 + r, lane columns nb .. nb+3 (the ping-pong kernel calls it from two places, the wide kernel for two blocks).
// gemm_f16x2_kernel keeps its own inline copy: calling this function from it changes the instruction stream of its EPI_GELU
// instantiation (profiles/gemm_x2_split_isa.md), and that kernel's code is closed by measurement.  An edit to one copy is an
// edit to both.  `ti`: the workgroup's running tile index, `rs_row`: the block's first lane row inside the tile (EPI_GELU_LN's
// row statistics: buffer parity and row); `sbias` may be LDS or global; `bias_regs`: the lane's four biases where the caller
// already holds them.
template <int EPI, int TAG>
__device__ __forceinline__ void x2_epilogue_at(f32x4 (&acc)[4][4], const int pm0, const int nb, int ti, int M, int N, int rs_row,
                                               int fi, int lane, float unscale, float oscale, float* __restrict__ outf,
                                               f16* __restrict__ out2, float* __restrict__ aux, unsigned* __restrict__ flag,
                                               const float* sbias, char* smem, const f32x4* bias_regs = nullptr) {
  // ---- tile epilogue: lane holds out[m = pm0 + mi*16 + r][n = nb + ni], pm0 = tile row + wr*64 + 4 fg, nb = tile column
  // + wc*64 + 4 fi.  Every store address is  uniform base + 32-bit lane offset  (the launcher refuses outputs of 4 GiB or
  // more), advanced row by row: per-row 64-bit address arithmetic was most of the epilogue's VALU work, and it runs
  // with the matrix pipes idle.
  if (nb < N) {
    const float4 bz = bias_regs ? make_float4((*bias_regs)[0], (*bias_regs)[1], (*bias_regs)[2], (*bias_regs)[3])
                                : *reinterpret_cast<const float4*>(sbias + nb);
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
      srow = reinterpret_cast<const float*>(smem + XROWSTAT + (ti & 1) * (XBM * 8)) + rs_row * 2;
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
          } else if constexpr (EPI != EPI_RESID && EPI != EPI_RESID_LN) {
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

// x2_epilogue_at for the block of compute wave (wr, wc) of tile `t`, as gemm_f16x2_kernel places it
template <int EPI, int TAG>
__device__ __forceinline__ void x2_tile_epilogue(f32x4 (&acc)[4][4], int t, int ti, int tiles_n, int M, int N, int wr, int wc,
                                                 int fi, int fg, int lane, float unscale, float oscale, float* __restrict__ outf,
                                                 f16* __restrict__ out2, float* __restrict__ aux, unsigned* __restrict__ flag,
                                                 const float* sbias, char* smem) {
  x2_epilogue_at<EPI, TAG>(acc, (t / tiles_n) * XBM + wr * 64 + 4 * fg, (t % tiles_n) * XBN + wc * 64 + 4 * fi, ti, M, N,
                           wr * 64 + 4 * fg, fi, lane, unscale, oscale, outf, out2, aux, flag, sbias, smem);
}

// ---------------------------------------------------------------------------------------------------------------------
// PING-PONG form of the same Linear: the two compute waves of a SIMD work half a k-step apart.
//
// Measured on gemm_f16x2_kernel (gemm_x2.hip) with its loads AND its epilogue compiled out (profiles/r04_gemm_probes.md): 463 us for
// the qkv shape at M = 128,960 = 1.22 us per k-step, of which the matrix pipe needs 96 MFMAs x 16 = 1536 cycles (0.85 us at the 1.8 GHz
// the chip holds here).  All
// eight compute waves pass the k-step's barrier together, all read their fragments from LDS together (the pipe idles), then
// both waves of every SIMD push their 48 MFMAs through the one pipe together: the pipe is never fed during the read phase.
// Here the compute waves form two teams -- X = waves 0..3, Y = waves 4..7: one wave of each per SIMD (waves go to SIMDs round
// robin) -- and a k-step has TWO barriers, A and B:
//     phase a (after A_g):  X reads ALL its fragments of slab g           | Y multiplies slab g - 1 (48 MFMAs, the pipe to itself)
//     phase b (after B_g):  X multiplies slab g                           | Y reads all its fragments of slab g
// so while one team waits for LDS the other owns the matrix pipe.  A wave holds one k-step's fragments (16 x 16 bytes per lane)
// instead of streaming the A fragments behind the MFMAs: nothing reads slab g after phase b(g), the ring and the loaders'
// schedule (slab g + 2 issued behind A_g, landed by A_{g+2}) are those of gemm_f16x2_kernel; the lagged MFMAs are gone (they
// existed to cover the read phase).  A tile's epilogue falls into the team's read phase at the start of its next tile, beside
// the other team's MFMAs (team Y: after the MFMAs of its last k-step, in phase a).
template <int EPI, int TAG>
__global__ __launch_bounds__(768) void gemm_f16x2_pp_kernel(const f16* __restrict__ A2, const f16* __restrict__ W2,
                                                            const float* __restrict__ bias, float unscale, float oscale,
                                                            float* __restrict__ outf, f16* __restrict__ out2,
                                                            float* __restrict__ aux, unsigned* __restrict__ flag, int M,
                                                            int N, int K, int tiles_n, int total_tiles) {
  static_assert(EPI == EPI_BIAS || EPI == EPI_GELU || EPI == EPI_RESID, "the LayerNorm-folding epilogues keep gemm_f16x2_kernel");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sbias = reinterpret_cast<float*>(smem + XNSTAGE * XSTAGE);
  const int G = gridDim.x;
  const int L = xcd_remap(blockIdx.x, G);
  const int n_my = (total_tiles - L + G - 1) / G;      // tiles L, L+G, ...
  const int NK = K / XBK;
  const int gtot = n_my * NK;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  for (int i = tid; i < N; i += (XNCW + 4) * 64) sbias[i] = bias[i];
  __syncthreads();
  if (gtot == 0) return;

  if (wave >= XNCW) {
    // ------------------------------------------------------------------ loader waves (as gemm_f16x2_kernel's, two barriers per k-step)
    const int lw = wave - XNCW;
    const int lr = lane >> 3, lq = lane & 7;
    int ti = 0, ks = 0, slot = 0;
    const f16* pa[8];
    const f16* pw[4];
    auto issue = [&]() {
      if (ks == 0) {
        const int t = L + ti * G;
        const int m0 = (t / tiles_n) * XBM, n0 = (t % tiles_n) * XBN;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int row = (lw * 8 + i) * 8 + lr;
          pa[i] = A2 + (size_t)min(m0 + row, M - 1) * (2 * K) + swz128(row, lq) * 8;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = (lw * 4 + i) * 8 + lr;
          const int wrow = (row & 64) + colperm(row & 63);
          pw[i] = W2 + (size_t)min(n0 + wrow, N - 1) * (2 * K) + swz128(row, lq) * 8;
        }
      }
      char* base = smem + slot * XSTAGE;
      const int ko = ks * (2 * XBK);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        __builtin_amdgcn_global_load_lds(GPTR(pa[i] + ko), LPTR(base + (lw * 8 + i) * 1024), 16, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        __builtin_amdgcn_global_load_lds(GPTR(pw[i] + ko), LPTR(base + XA_BYTES + (lw * 4 + i) * 1024), 16, 0, 0);
      if (++ks == NK) { ks = 0; ++ti; }
      slot = (slot == XNSTAGE - 1) ? 0 : slot + 1;
    };
    issue();
    if (gtot > 1) issue();
    for (int g = 0; g < gtot; ++g) {
      if (g + 1 < gtot) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      X2_BARRIER();                                    // A_g: slab g has landed; nobody reads slab g - 1 any more
      if (g + 2 < gtot) issue();                       // slab g + 2 into the slot of slab g - 1
      X2_BARRIER();                                    // B_g
    }
    return;
  }

  // -------------------------------------------------------------------- compute waves
  const int team = wave >> 2;                          // 0 = X, 1 = Y
  const int wr = wave >> 1, wc = wave & 1;
  const int fi = lane & 15, fg = lane >> 4;
  const int offA = (wr * 64 + fi) * 128 + swz128(fi, fg) * 16, offAl = offA ^ 64;
  const int offW = XA_BYTES + (wc * 64 + fi) * 128 + swz128(fi, fg) * 16, offWl = offW ^ 64;
  f32x4 acc[4][4];
  f16x8 wf[4][2], ah[4], al[4];                        // one k-step's fragments
  __builtin_amdgcn_s_setprio(1);
  int slot = 0;
  auto zero_acc = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  };
  auto read_all = [&]() {
    const char* sb = smem + slot * XSTAGE;
    slot = (slot == XNSTAGE - 1) ? 0 : slot + 1;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int pl = 0; pl < 2; ++pl)
        wf[ni][pl] = *reinterpret_cast<const f16x8*>(sb + (pl ? offWl : offW) + ni * 2048);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      ah[mi] = *reinterpret_cast<const f16x8*>(sb + offA + mi * 2048);
      al[mi] = *reinterpret_cast<const f16x8*>(sb + offAl + mi * 2048);
    }
  };
  auto mfma_all = [&]() {
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      // small terms first; the three products of one output tile are four MFMAs apart (no back-to-back dependency)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[mi], wf[ni][1], acc[mi][ni], 0, 0, 0);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[mi], wf[ni][0], acc[mi][ni], 0, 0, 0);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[mi], wf[ni][0], acc[mi][ni], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  auto epilogue = [&](int ti) {
    x2_tile_epilogue<EPI, TAG>(acc, L + ti * G, ti, tiles_n, M, N, wr, wc, fi, fg, lane, unscale, oscale, outf, out2, aux, flag,
                               sbias, smem);
  };

  // (one pass more than there are k-steps: the last tile's epilogue runs where every other tile's does, so the epilogue is
  //  instantiated once per team -- two more copies of it cost registers the kernel does not have)
  if (team == 0) {
    int ks = 0, ti = 0;
#pragma unroll 1
    for (int g = 0; g <= gtot; ++g) {
      if (g < gtot) X2_BARRIER();                      // A_g
      if (ks == 0) {
        if (g > 0) epilogue(ti - 1);                   // the finished tile leaves beside team Y's MFMAs
        zero_acc();
      }
      if (g == gtot) break;
      read_all();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      X2_BARRIER();                                    // B_g
      mfma_all();
      if (++ks == NK) { ks = 0; ++ti; }
    }
  } else {
    int ks = 0, ti = 0;
#pragma unroll 1
    for (int g = 0; g <= gtot; ++g) {
      if (g < gtot) X2_BARRIER();                      // A_g
      if (g > 0) mfma_all();                           // slab g - 1
      if (ks == 0) {
        if (g > 0) epilogue(ti - 1);
        zero_acc();
      }
      if (g == gtot) break;
      X2_BARRIER();                                    // B_g
      read_all();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (++ks == NK) { ks = 0; ++ti; }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// WIDE form of the same Linear: 256 x 256 tile, eight waves of 256 registers, no loader waves.
//
// An experiment (profiles/r04_gemm_probes.md section 4): per MFMA a 64 x 128 register tile per wave (128 accumulator registers,
// 64 for the eight W fragments it keeps for the whole k-step) reads 0.75 x the LDS bytes of gemm_f16x2_kernel (gemm_x2.hip),
// receives 0.67 x the LDS-DMA bytes, fetches A half as often and passes half as many barriers.  That needs the 256 registers
// of a two-waves-per-SIMD workgroup, so nothing is left for loader waves: every wave issues its own share of the k-step's
// LDS-DMA (4 A pieces + 4 W pieces of 8 rows) in inline assembly and waits for it with counted vmcnt; the epilogue's
// stores pass through the same counter and are counted with it (x2_epilogue_at issues exactly 16 stores per 64 x 64
// block of a full tile).  MEASURED: ties with gemm_f16x2_kernel within 3 % as built, without loads, without epilogue
// and without both -- the Linear's time is its MFMA count at the clock the power budget allows, not its LDS traffic.
// Kept behind D3DP_X2_WIDE=1 (and epi | 4096 of d3dp_op_linear_x2), off.
//   LDS: A ring 3 x 32 KiB at 0, W ring 2 x 32 KiB at 96 KiB = 160 KiB; the bias is read from global memory.
//   per k-step g:  wait own A(g), W(g) | barrier | issue W(g+1) -> W slot of g-1, A(g+2) -> A slot of g-1 | 96 MFMAs
// Requires N % 256 == 0 and K % 32 == 0.  The products meet every accumulator in the order of the plain kernel
// (k ascending; ah.wl, al.wh, ah.wh): results are bit-identical to it.
constexpr int WBN = 256;
constexpr int WA_STAGES = 3, WW_STAGES = 2;
constexpr int WW_BYTES = WBN * 128;                  // 32 KiB
constexpr int WW_BASE = WA_STAGES * XA_BYTES;        // 96 KiB
constexpr int WLDS = WW_BASE + WW_STAGES * WW_BYTES; // 160 KiB

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"          // (the expected "clobber list contains reserved registers" note for m0)
// one LDS-DMA wave-instruction in the  uniform base + 32-bit lane offset  form: lane l's 16 bytes at base + off -> LDS
// bytes [lds + 16 l, +16).  Inline assembly for the reasons given at lds_dma16 in attention_x2.hip: the builtin makes the
// compiler turn every vector-memory wait of the kernel into vmcnt(0).
__device__ __forceinline__ void wide_dma16(unsigned off, const char* base, unsigned lds) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(off), "s"(base), "s"(lds) : "memory", "m0");
}
#pragma clang diagnostic pop
// 16-byte global load the compiler does not track (it would wait for it with vmcnt(0) counted without the LDS-DMA operations
// around it); the caller waits with wide_wait_vmcnt and passes the registers through wide_settle.
__device__ __forceinline__ f32x4 wide_gload16(const float* p) {
  f32x4 r;
  asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(r) : "v"(p) : "memory");
  return r;
}
__device__ __forceinline__ void wide_settle(f32x4& r) { asm volatile("" : "+v"(r)); }
template <int V>
__device__ __forceinline__ void wide_wait_vmcnt() { __builtin_amdgcn_s_waitcnt((V & 15) | (7 << 4) | (15 << 8) | ((V >> 4) << 14)); }

template <int EPI, int TAG>
__global__ __launch_bounds__(512) void gemm_f16x2_wide_kernel(const f16* __restrict__ A2, const f16* __restrict__ W2,
                                                              const float* __restrict__ bias, float unscale, float oscale,
                                                              float* __restrict__ outf, f16* __restrict__ out2,
                                                              float* __restrict__ aux, unsigned* __restrict__ flag, int M,
                                                              int N, int K, int tiles_n, int total_tiles) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int G = gridDim.x;
  const int L = xcd_remap(blockIdx.x, G);
  const int n_my = (total_tiles - L + G - 1) / G;      // tiles L, L+G, ...
  const int NK = K / XBK;
  const int gtot = n_my * NK;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  const int fi = lane & 15, fg = lane >> 4;
  const int lr = lane >> 3, lq = lane & 7;             // loader role: row within an 8-row piece, physical 16-byte slot
  const unsigned lds0 = (unsigned)(__UINTPTR_TYPE__)LPTR(smem);
  const unsigned rowbytes = (unsigned)K * 4;           // one operand row: K x (hi | lo) fp16

  // ---- this wave's share of the loads: pieces 4 wave .. 4 wave + 3 of the A slab and of the W slab
  unsigned voffW[4], voffA[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (wave * 4 + i) * 8 + lr;                            // LDS row of the W slab
    const int wrow = (row & ~63) + colperm(row & 63);                   // output column (inside the tile) it carries
    voffW[i] = (unsigned)wrow * rowbytes + swz128(row, lq) * 16;        // (N % 256 == 0: no clamp)
  }
  int tiA = 0, ksA = 0, slotA = 0, tiW = 0, ksW = 0, slotW = 0;         // (tile, k-step, ring slot) of the next slab to issue
  const char* baseA = nullptr;
  const char* baseW = nullptr;
  auto issueA = [&]() {
    if (ksA == 0) {
      const int t = L + tiA * G;
      const int m0 = (t / tiles_n) * XBM;
      baseA = reinterpret_cast<const char*>(A2) + (size_t)m0 * rowbytes;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = (wave * 4 + i) * 8 + lr;
        voffA[i] = (unsigned)min(row, M - 1 - m0) * rowbytes + swz128(row, lq) * 16;
      }
    }
    const char* b = baseA + ksA * (4 * XBK);           // one k-step of a row = 64 fp16 = 128 B
    const unsigned dst = lds0 + slotA * XA_BYTES + wave * 4096;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      wide_dma16(voffA[i], b, dst + i * 1024);
    if (++ksA == NK) { ksA = 0; ++tiA; }
    slotA = (slotA == WA_STAGES - 1) ? 0 : slotA + 1;
  };
  auto issueW = [&]() {
    if (ksW == 0) {
      const int t = L + tiW * G;
      baseW = reinterpret_cast<const char*>(W2) + (size_t)((t % tiles_n) * WBN) * rowbytes;
    }
    const char* b = baseW + ksW * (4 * XBK);
    const unsigned dst = lds0 + WW_BASE + slotW * WW_BYTES + wave * 4096;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      wide_dma16(voffW[i], b, dst + i * 1024);
    if (++ksW == NK) { ksW = 0; ++tiW; }
    slotW ^= 1;
  };

  // per-lane fragment offsets (the swizzle depends on the lane only: rows advance in multiples of 16; lo plane = offset ^ 64)
  const int offA = (wr * 64 + fi) * 128 + swz128(fi, fg) * 16, offAl = offA ^ 64;
  const int offW = WW_BASE + (wc * 128 + fi) * 128 + swz128(fi, fg) * 16, offWl = offW ^ 64;
  f32x4 acc[2][4][4];                                  // [column half][mi][ni]: two 64 x 64 blocks as the epilogue wants them

  if (gtot > 0) { issueA(); issueW(); }
  if (gtot > 1) issueA();
  int g = 0, cslotA = 0, cslotW = 0;
  bool after_full_tile = false;                        // the previous k-step ended with the 32 stores of a full tile
#pragma unroll 1
  for (int ti = 0; ti < n_my; ++ti) {
    const int t = L + ti * G;
    const int m0 = (t / tiles_n) * XBM, nb0 = (t % tiles_n) * WBN + wc * 128 + 4 * fi;   // (nb0: this lane's first column)
    f32x4 bz[2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[h][i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int ks = 0; ks < NK; ++ks, ++g) {
      // own loads of slab g landed; younger operations that may stay in flight: A(g+1) (4) and, right behind a full
      // tile's epilogue, its 32 stores.  (Behind a partial tile the number of stores issued is not known: the strict
      // count is always safe -- the stores are the youngest operations.)
      if (g + 1 >= gtot) wide_wait_vmcnt<0>();
      else if (after_full_tile) wide_wait_vmcnt<36>();
      else wide_wait_vmcnt<4>();
      after_full_tile = false;
      __builtin_amdgcn_s_waitcnt(0xc07f);              // lgkmcnt(0): this wave has read everything it wanted from the old slots
      X2_BARRIER();
      if (g + 1 < gtot) issueW();                      // into the slots of k-step g-1: every wave has passed barrier g
      if (g + 2 < gtot) issueA();
      if (ks == NK - 1) {                              // the tile's bias, a k-step ahead of its use (youngest operations)
        bz[0] = wide_gload16(bias + nb0);
        bz[1] = wide_gload16(bias + nb0 + 64);
      }
      __builtin_amdgcn_sched_barrier(0);
      const char* sa = smem + cslotA * XA_BYTES;
      const char* sw = smem + cslotW * WW_BYTES;
      cslotA = (cslotA == WA_STAGES - 1) ? 0 : cslotA + 1;
      cslotW ^= 1;
      f16x8 wf[8][2], ah[2], al[2];
      ah[0] = *reinterpret_cast<const f16x8*>(sa + offA);
      al[0] = *reinterpret_cast<const f16x8*>(sa + offAl);
#pragma unroll
      for (int nj = 0; nj < 8; ++nj) {
        wf[nj][1] = *reinterpret_cast<const f16x8*>(sw + offWl + nj * 2048);
        wf[nj][0] = *reinterpret_cast<const f16x8*>(sw + offW + nj * 2048);
      }
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const int b = mi & 1;
        if (mi < 3) {                                  // next row block's fragments while this one multiplies
          ah[b ^ 1] = *reinterpret_cast<const f16x8*>(sa + offA + (mi + 1) * 2048);
          al[b ^ 1] = *reinterpret_cast<const f16x8*>(sa + offAl + (mi + 1) * 2048);
        }
        if (mi == 0) {
          // column-major through the first row block: its first MFMAs need 4 of the 18 fragment reads, not 10
#pragma unroll
          for (int nj = 0; nj < 8; ++nj) {
            f32x4& c = acc[nj >> 2][0][nj & 3];
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[0], wf[nj][1], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[0], wf[nj][0], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[0], wf[nj][0], c, 0, 0, 0);
          }
        } else {
#pragma unroll
          for (int nj = 0; nj < 8; ++nj)
            acc[nj >> 2][mi][nj & 3] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[b], wf[nj][1], acc[nj >> 2][mi][nj & 3], 0, 0, 0);
#pragma unroll
          for (int nj = 0; nj < 8; ++nj)
            acc[nj >> 2][mi][nj & 3] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[b], wf[nj][0], acc[nj >> 2][mi][nj & 3], 0, 0, 0);
#pragma unroll
          for (int nj = 0; nj < 8; ++nj)
            acc[nj >> 2][mi][nj & 3] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[b], wf[nj][0], acc[nj >> 2][mi][nj & 3], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // everything this wave has in flight was issued a k-step ago or earlier: the loads of the next two k-steps and the bias
    wide_wait_vmcnt<0>();
    wide_settle(bz[0]);
    wide_settle(bz[1]);
#pragma unroll
    for (int h = 0; h < 2; ++h)
      x2_epilogue_at<EPI, TAG>(acc[h], m0 + wr * 64 + 4 * fg, nb0 + h * 64, ti, M, N, 0, fi, lane, unscale, oscale, outf, out2,
                               aux, flag, bias, smem, &bz[h]);
    after_full_tile = m0 + XBM <= M;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The same Linear with a ROW-CLASS SKEWED schedule: a tile's epilogue runs UNDER the k-loop of the next tile.
//
// In gemm_f16x2_kernel all eight compute waves reach a tile's epilogue together (one s_barrier per k-step keeps them in
// lock-step), so its VALU work and stores -- 12 % of the qkv Linear, 27 % of fc1 with its GELU (profiles/r03_gemm_probes.md)
// -- run with the matrix pipes idle; parking a finished 256 x 128 tile beside the next one's accumulators would take 64 more
// registers than a 12-wave workgroup has.  Here the four 16-row blocks of a wave's 64 rows (row class c = 0..3) end their
// tiles at DIFFERENT k-steps: class c switches to its next tile when ks == c D.  Sums over k commute, so class c simply
// runs the k-steps of a tile in the rotated order c D, ..., NK - 1, 0, ..., c D - 1; all classes still consume the SAME W
// slab in every k-step (consecutive tiles of a workgroup lie in one 128-column strip), and only the A rows of class c
// belong to another tile for a while -- a matter of which rows the loader waves fetch.  At most ONE class is between tiles
// at any time: its 16 finished values per lane are PARKED (16 registers) and leave over the next D k-steps, 4 / D output
// rows per k-step, their VALU work and stores issued between that k-step's 48 MFMAs.
//   registers  Which accumulator block parks must not be a run-time choice (selecting acc[c] dynamically costs the register
//              allocator ~40 registers of copies, and unrolling a whole tile round spills as well): the block that parks is
//              always accumulator block 0.  After it parks, the blocks shift down (acc[p] <- acc[p + 1], acc[3] <- 0: 40
//              v_mov per D k-steps) and the LOADERS rotate the LDS image to match: with rot = number of parks so far, LDS
//              row slot p of every 64-row group holds the rows of class (p + rot) & 3.  The compute code is static.
//   schedule   workgroup L owns strip L % tiles_n and the row-tile range [lo, hi) of its row group L / tiles_n (Q = G /
//              tiles_n row groups; G - Q tiles_n workgroups idle).  Round ti = NK k-steps; class c works on tile ti (ks >= c D)
//              or ti - 1.  (hi - lo) full rounds and a flush of 3 D k-steps: in the first c D steps class c has no tile yet
//              (its sums are discarded), in the flush the classes that are done multiply rows nobody stores -- 1.5 D k-steps
//              of matrix work lost per launch and workgroup, against one exposed epilogue per tile.
//   loaders    A piece i of loader wave lw lands in LDS rows lw 64 + 8 i .. + 7 (row slot i >> 1) as before; it FETCHES the
//              rows of class ((i >> 1) + rot) & 3, from tile ti or ti - 1 as that class stands; pointers re-derived at the
//              four park steps of a round.  W pieces: one strip for the whole launch.  Ring, barriers, vmcnt: unchanged.
//   numerics   the rotation changes the ORDER of a row's fp32 partial sums with its row class: ctx.h seq_pitch() pads every sequence
//              to a multiple of 64 rows (d3dp_ctx::seq_pitch), which makes the class a function of the token's index in its
//              sequence -- results stay bit-identical across batch compositions, pass splits and ranks.
// Built for the two Linears whose epilogue is pure register work: EPI_BIAS / TAG 1 (qkv, packed rows) and EPI_GELU (fc1).
// proj / fc2 (x += ..., their epilogue waits on loads of the residual rows) keep gemm_f16x2_kernel.
template <int EPI, int TAG, int D>
__global__ __launch_bounds__(768) void gemm_f16x2_skew_kernel(const f16* __restrict__ A2, const f16* __restrict__ W2,
                                                              const float* __restrict__ bias, float unscale, float oscale,
                                                              float* __restrict__ outf, f16* __restrict__ out2, int M, int N,
                                                              int K, int tiles_n, int tm, int Q) {
  static_assert(D == 1 || D == 2 || D == 4, "a parked class leaves in D k-steps, 4 / D rows per k-step");
  static_assert(EPI == EPI_GELU || (EPI == EPI_BIAS && TAG == 1), "epilogues without loads only");
  constexpr int RPK = 4 / D;                           // output rows (of the parked class) per k-step
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sbias = reinterpret_cast<float*>(smem + XNSTAGE * XSTAGE);
  const int G = gridDim.x;
  const int L = xcd_remap(blockIdx.x, G);
  const int strip = L % tiles_n, rg = L / tiles_n;
  const int lo = rg < Q ? (int)((long)rg * tm / Q) : 0, hi = rg < Q ? (int)((long)(rg + 1) * tm / Q) : 0;
  const int n_tiles = hi - lo;
  const int NK = K / XBK;                              // >= 4 D (launcher)
  const int gtot = n_tiles > 0 ? n_tiles * NK + 3 * D : 0;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  for (int i = tid; i < N; i += (XNCW + 4) * 64) sbias[i] = bias[i];
  __syncthreads();
  if (gtot == 0) return;

  if (wave >= XNCW) {
    // ------------------------------------------------------------------ loader waves
    const int lw = wave - XNCW;
    const int lr = lane >> 3, lq = lane & 7;
    const f16* pa[8];
    const f16* pw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = (lw * 4 + i) * 8 + lr;
      const int wrow = (row & 64) + colperm(row & 63);
      pw[i] = W2 + (size_t)min(strip * XBN + wrow, N - 1) * (2 * K) + swz128(row, lq) * 8;
    }
    int ti = 0, ks = 0, slot = 0;                      // (round, k-step, ring slot) of the next slab to issue
    auto issue = [&]() {
      if ((ks & (D - 1)) == 0 && ks < 4 * D) {         // a park step: the LDS image rotates and one class changes tile
        const int rot = (ks / D + 1) & 3;              // parks so far, mod 4, once this step's park is done
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int cls = ((i >> 1) + rot) & 3;        // the class whose rows row slot i >> 1 holds from this k-step on
          int j = ks >= cls * D ? ti : ti - 1;         // that class has switched to tile ti in this round, or has not yet
          j = min(max(j, 0), n_tiles - 1);             // (before its first tile / after its last: any valid rows)
          const int lds_row = (lw * 8 + i) * 8 + lr;   // where the piece lands (the swizzle goes by the LDS row)
          const int row = lw * 64 + cls * 16 + (i & 1) * 8 + lr;
          pa[i] = A2 + (size_t)min((lo + j) * XBM + row, M - 1) * (2 * K) + swz128(lds_row, lq) * 8;
        }
      }
      char* base = smem + slot * XSTAGE;
      const int ko = ks * (2 * XBK);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        __builtin_amdgcn_global_load_lds(GPTR(pa[i] + ko), LPTR(base + (lw * 8 + i) * 1024), 16, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        __builtin_amdgcn_global_load_lds(GPTR(pw[i] + ko), LPTR(base + XA_BYTES + (lw * 4 + i) * 1024), 16, 0, 0);
      if (++ks == NK) { ks = 0; ++ti; }
      slot = (slot == XNSTAGE - 1) ? 0 : slot + 1;
    };
    issue();
    if (gtot > 1) issue();
    for (int g = 0; g < gtot; ++g) {
      if (g + 1 < gtot) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      X2_BARRIER();
      if (g + 2 < gtot) issue();
    }
    return;
  }

  // -------------------------------------------------------------------- compute waves
  const int wr = wave >> 1, wc = wave & 1;
  const int fi = lane & 15, fg = lane >> 4;
  const int offA = (wr * 64 + fi) * 128 + swz128(fi, fg) * 16, offAl = offA ^ 64;
  const int offW = XA_BYTES + (wc * 64 + fi) * 128 + swz128(fi, fg) * 16, offWl = offW ^ 64;
  __builtin_amdgcn_s_setprio(1);

  // what does not change over the launch: this lane's four output columns nb .. nb + 3 of the workgroup's strip.  (A wave's
  // 64 columns lie in one region of the packed qkv row: `planes` is wave-uniform.)
  const int nbw = strip * XBN + wc * 64;               // wave-uniform
  const int nb = nbw + 4 * fi;
  const bool cols_live = nb < N;
  const bool odd = fi & 1;
  const unsigned pitch = (unsigned)N * 4;              // bytes per output row in every form (fp32 [N], h2i [2 N] fp16, packed 12 C)
  bool planes;
  unsigned coff;
  char* base;
  {
    const int c0 = nb & ~7;
    if constexpr (EPI == EPI_GELU) {                   // the fc2 operand, h2i: even lane -> hi slot of the pair's 8 columns, odd -> lo
      base = reinterpret_cast<char*>(out2);
      planes = true;
      coff = (c0 >> 5) * 128 + (c0 & 31) * 2 + (odd ? 64 : 0);
    } else {                                           // packed qkv row: q fp32 | k hi | k lo | v hi | v lo
      base = reinterpret_cast<char*>(outf);
      const int C = N / 3, region = nbw / C, cn = nb - region * C;
      planes = region != 0;
      coff = planes ? region * 4 * C + cn * 2 + (odd ? 2 * C - 8 : 0) : cn * 4;
    }
  }
  const int row0 = wr * 64 + 4 * fg;                   // this lane's row (r = 0) of row class 0 inside a tile

  f32x4 acc[4][4];                                     // acc[p]: the class whose rows LDS row slot p holds ((p + rot) & 3)
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  f32x4 park[4];                                       // the class between tiles: park[ni][r]
#pragma unroll
  for (int j = 0; j < 4; ++j) park[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  unsigned joff = 0;                                   // byte offset of row r = 0 of the parked class (+ coff)
  int jrows = 0;                                       // its rows r < jrows exist (<= 0: nothing to store)
  float4 jbz = {};                                     // the lane's four biases, re-read at every park

  // value e of output row r of the parked class, through the epilogue's arithmetic (the lane's four biases are re-read
  // from LDS in every k-step that needs them -- one ds_read_b128 -- instead of living in registers across the k-loop)
  const float* bias4 = sbias + min(nb, N - 4);
  auto value = [&](int r, int e, const float4& bz) {
    return fmaf(park[e][r], unscale, e == 0 ? bz.x : e == 1 ? bz.y : e == 2 ? bz.z : bz.w);
  };
  // one output row of the parked class: 4 values per lane -> one 16-byte store per lane
  auto store_row = [&](int r, float (&v)[4]) {
    const bool live = cols_live && r < jrows;
    char* dst = base + (joff + (unsigned)r * pitch);
    if (planes) {
      f16x4 ph, pl;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        f16 h, l;
        split2h_scaled(v[e] * oscale, h, l);
        ph[e] = h; pl[e] = l;
      }
      store_planes_paired(dst, ph, pl, odd, live);
    } else {
      if (live) OUT_STORE(reinterpret_cast<f32x4*>(dst), ((f32x4){v[0], v[1], v[2], v[3]}));
    }
  };
  // the class in accumulator block 0 changes tile: park it, shift the blocks down, start its next tile from zero in block 3
  // (the loaders rotate the LDS image by one row slot at the same k-step)
  auto park_and_shift = [&](int cls, int tile) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      park[j] = acc[0][j];
      acc[0][j] = acc[1][j]; acc[1][j] = acc[2][j]; acc[2][j] = acc[3][j];
      acc[3][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    const int m_row = (lo + tile) * XBM + row0 + cls * 16;      // tile < 0 (no tile finished yet): nothing is stored
    jrows = tile >= 0 ? M - m_row : 0;
    joff = (unsigned)m_row * pitch + coff;
    jbz = *reinterpret_cast<const float4*>(bias4);
  };

  int slot = 0;
  // one k-step; JOB: RPK rows of the parked class leave beside its MFMAs (a compile-time flag: a run-time branch inside the
  // k-step would cut its MFMAs and the epilogue's VALU into separate scheduling regions); r0 = first of those rows
  auto kstep = [&](auto job_c, int r0) {
    constexpr bool JOB = decltype(job_c)::value;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    X2_BARRIER();
    __builtin_amdgcn_sched_barrier(0);
    const char* sb = smem + slot * XSTAGE;
    slot = (slot == XNSTAGE - 1) ? 0 : slot + 1;
    f16x8 wf[4][2], ah[2], al[2];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int pl = 0; pl < 2; ++pl)
        wf[ni][pl] = *reinterpret_cast<const f16x8*>(sb + (pl ? offWl : offW) + ni * 2048);
    ah[0] = *reinterpret_cast<const f16x8*>(sb + offA);
    al[0] = *reinterpret_cast<const f16x8*>(sb + offAl);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (JOB) {
      // the leaving rows of this k-step, whole, in ONE packet right behind the k-step's fragment reads and in front of its first
      // MFMA -- the window in which every wave of the workgroup waits for LDS after the barrier anyway (nothing here depends on
      // the reads).  Measured: interleaved with the MFMAs of the four row blocks the same work cost as much as an exposed
      // epilogue.
#pragma unroll
      for (int rr = 0; rr < RPK; ++rr) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = value(r0 + rr, e, jbz);
          if constexpr (EPI == EPI_GELU) v[e] = gelu_erf_rational(v[e]);
        }
        store_row(r0 + rr, v);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const int b = mi & 1;
      if (mi < 3) {                                    // next block's fragments while this one multiplies
        ah[b ^ 1] = *reinterpret_cast<const f16x8*>(sb + offA + (mi + 1) * 2048);
        al[b ^ 1] = *reinterpret_cast<const f16x8*>(sb + offAl + (mi + 1) * 2048);
      }
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[b], wf[ni][1], acc[mi][ni], 0, 0, 0);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[b], wf[ni][0], acc[mi][ni], 0, 0, 0);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[b], wf[ni][0], acc[mi][ni], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  const int rest = NK - 4 * D;                         // k-steps of a round in which no class is between tiles
#pragma unroll 1
  for (int ti = 0; ti <= n_tiles; ++ti) {
    const int ngrp = ti < n_tiles ? 4 : 3;             // (the flush: classes 0..2 leave in 3 D k-steps; class 3 after the loop)
#pragma unroll 1
    for (int grp = 0; grp < ngrp; ++grp) {
      park_and_shift(grp, ti - 1);                     // class grp has just finished tile ti - 1
#pragma unroll
      for (int s = 0; s < D; ++s) kstep(std::true_type{}, s * RPK);   // (the row index must be a constant: park[e][r])
    }
    if (ti < n_tiles) {
#pragma unroll 1
      for (int s = 0; s < rest; ++s) kstep(std::false_type{}, 0);
    }
  }
  // the last class (3) of the last tile sits in accumulator block 0 by now: nothing left to hide it under
  {
    park_and_shift(3, n_tiles - 1);
    const float4 bz = *reinterpret_cast<const float4*>(bias4);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = value(r, e, bz);
        if constexpr (EPI == EPI_GELU) v[e] = gelu_erf_rational(v[e]);
      }
      store_row(r, v);
    }
  }
}

// rowstat[m] = (mean, 1 / sqrt(var + eps)) of row m from its S slices of 64 (mean_i, M2_i): mean = avg of means,
// M2 = sum M2_i + 64 sum (mean_i - mean)^2 (the exact pairwise update for equal counts), var = M2 / (64 S)
__global__ void ln_combine_kernel(const float* __restrict__ sl, float* __restrict__ rowstat, int M, int S, float eps) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const float2* p = reinterpret_cast<const float2*>(sl) + (size_t)m * S;
  float mean = 0.f;
  for (int i = 0; i < S; ++i) mean += p[i].x;
  mean *= 1.0f / (float)S;
  float m2 = 0.f;
  for (int i = 0; i < S; ++i) { const float d = p[i].x - mean; m2 += fmaf(64.0f * d, d, p[i].y); }
  const float rstd = 1.0f / sqrtf(m2 * (1.0f / (64.0f * (float)S)) + eps);
  reinterpret_cast<float2*>(rowstat)[m] = make_float2(mean, rstd);
}

// one wave per output row n: Wp[n][k] = W[n][k] gamma[k]; c12[n] = sum_k W[n][k] beta[k] + bias[n]; c12[N + n] = sum_k Wp[n][k]
// (sums in fp64: they stand in for fp32 dot products of the reference, and are computed once per weight load)
__global__ void fold_ln_kernel(const float* __restrict__ W, const float* __restrict__ gamma, const float* __restrict__ beta,
                               const float* __restrict__ bias, float* __restrict__ Wp, float* __restrict__ c12, int N, int K) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (n >= N) return;
  double s1 = 0.0, s2 = 0.0;
  for (int k = lane; k < K; k += 64) {
    const float w = W[(size_t)n * K + k], wp = w * gamma[k];
    Wp[(size_t)n * K + k] = wp;
    s1 += (double)wp;
    s2 += (double)w * (double)beta[k];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
  if (lane == 0) { c12[n] = (float)(s2 + (double)bias[n]); c12[N + n] = (float)s1; }
}

}  // namespace

// whether d3dp_launch_linear_f16x2 runs the row-class skewed kernel for this call (kernels.h)
bool d3dp_x2_skew_applies(int epi, int M, int N, int K, int skew_d, int n_cu) {
  if (skew_d != 1 && skew_d != 2 && skew_d != 4) return false;
  if (epi != EPI_QKV_PACK && epi != EPI_GELU) return false;
  const int tn = (N + XBN - 1) / XBN, tm = (M + XBM - 1) / XBM;
  if (K % XBK != 0 || K / XBK < 4 * skew_d) return false;   // four classes, D k-steps apart, inside one tile round
  if (N % XBN != 0) return false;                        // whole strips (the denoiser's 1536 and 1024)
  (void)tm;
  return n_cu / tn >= 1;                                 // (any M: with fewer row tiles than row groups, fewer groups work --
                                                         //  the schedule, and with it the summation order, must not depend on M)
}

// d3dp_launch_linear_f16x2 offers every call (already checked; `cus`: the device's CU count) to the experiments: 0 = launched,
// < 0 = error, 1 = not asked for or not applicable to the shape -- the caller launches the plain kernel.
static int x2_variants_launch(int epi, const void* A2, const void* W2, const float* bias, float unscale, float oscale, float* outf,
                              void* out2, float* aux, unsigned* flag, int M, int N, int K, hipStream_t st, int skew_d, int pingpong,
                              int cus) {
  using KernT = void (*)(const f16*, const f16*, const float*, float, float, float*, f16*, float*, unsigned*, int, int, int, int, int);
  const int tm = (M + XBM - 1) / XBM, tn = (N + XBN - 1) / XBN;
  const int total = tm * tn, grid = total < cus ? total : cus;
  if (d3dp_x2_skew_applies(epi, M, N, K, skew_d, cus)) {
    using SkewT = void (*)(const f16*, const f16*, const float*, float, float, float*, f16*, int, int, int, int, int, int);
    static const SkewT skews[6] = {gemm_f16x2_skew_kernel<EPI_BIAS, 1, 1>, gemm_f16x2_skew_kernel<EPI_BIAS, 1, 2>,
                                   gemm_f16x2_skew_kernel<EPI_BIAS, 1, 4>, gemm_f16x2_skew_kernel<EPI_GELU, 0, 1>,
                                   gemm_f16x2_skew_kernel<EPI_GELU, 0, 2>, gemm_f16x2_skew_kernel<EPI_GELU, 0, 4>};
    static PerDeviceOnce once_skew;
    if (once_skew.get([&](int) {
          for (int k = 0; k < 6; ++k)
            if (d3dp_lds_opt_in(reinterpret_cast<const void*>(skews[k]), XLDS) < 0) return -3;
          return 1;
        }) < 0) return -3;
    const int Q = cus / tn < tm ? cus / tn : tm;         // row groups: Q tn workgroups work, the others idle
    const SkewT kern = skews[(epi == EPI_GELU ? 3 : 0) + (skew_d == 1 ? 0 : skew_d == 2 ? 1 : 2)];
    hipLaunchKernelGGL(kern, dim3(cus), dim3((XNCW + 4) * 64), XLDS, st, (const f16*)A2, (const f16*)W2, bias, unscale, oscale,
                       outf, (f16*)out2, M, N, K, tn, tm, Q);
    return 0;
  }
  if (pingpong == 2 && N % WBN == 0 && (epi == EPI_BIAS || epi == EPI_QKV_PACK || epi == EPI_GELU || epi == EPI_RESID)) {
    static const KernT wides[4] = {gemm_f16x2_wide_kernel<EPI_BIAS, 0>, gemm_f16x2_wide_kernel<EPI_BIAS, 1>,
                                   gemm_f16x2_wide_kernel<EPI_GELU, 0>, gemm_f16x2_wide_kernel<EPI_RESID, 0>};
    static PerDeviceOnce once_wide;
    if (once_wide.get([&](int) {
          for (int k = 0; k < 4; ++k)
            if (d3dp_lds_opt_in(reinterpret_cast<const void*>(wides[k]), WLDS) < 0) return -3;
          return 1;
        }) < 0) return -3;
    const int tw = N / WBN, totw = tm * tw;
    const KernT kern = wides[epi == EPI_GELU ? 2 : epi == EPI_RESID ? 3 : epi == EPI_QKV_PACK ? 1 : 0];
    hipLaunchKernelGGL(kern, dim3(totw < cus ? totw : cus), dim3(512), WLDS, st, (const f16*)A2, (const f16*)W2, bias, unscale,
                       oscale, outf, (f16*)out2, aux, flag, M, N, K, tw, totw);
    return 0;
  }
  if (pingpong == 1 && (epi == EPI_BIAS || epi == EPI_QKV_PACK || epi == EPI_GELU || epi == EPI_RESID)) {
    static const KernT pps[4] = {gemm_f16x2_pp_kernel<EPI_BIAS, 0>, gemm_f16x2_pp_kernel<EPI_BIAS, 1>,
                                 gemm_f16x2_pp_kernel<EPI_GELU, 0>, gemm_f16x2_pp_kernel<EPI_RESID, 0>};
    static PerDeviceOnce once_pp;
    if (once_pp.get([&](int) {
          for (int k = 0; k < 4; ++k)
            if (d3dp_lds_opt_in(reinterpret_cast<const void*>(pps[k]), XLDS) < 0) return -3;
          return 1;
        }) < 0) return -3;
    const KernT kern = pps[epi == EPI_GELU ? 2 : epi == EPI_RESID ? 3 : epi == EPI_QKV_PACK ? 1 : 0];
    hipLaunchKernelGGL(kern, dim3(grid), dim3((XNCW + 4) * 64), XLDS, st, (const f16*)A2, (const f16*)W2, bias, unscale, oscale,
                       outf, (f16*)out2, aux, flag, M, N, K, tn, total);
    return 0;
  }
  return 1;
}

// norm2 folded into proj / fc1 (kernels.h)
void d3dp_launch_ln_combine(const float* slices, float* rowstat, int M, int C, float eps, hipStream_t st) {
  hipLaunchKernelGGL(ln_combine_kernel, dim3((M + 255) / 256), dim3(256), 0, st, slices, rowstat, M, (C + 63) / 64, eps);
}

void d3dp_launch_fold_ln(const float* W, const float* gamma, const float* beta, const float* bias, float* Wp, float* c12,
                         int N, int K, hipStream_t st) {
  hipLaunchKernelGGL(fold_ln_kernel, dim3((N + 3) / 4), dim3(256), 0, st, W, gamma, beta, bias, Wp, c12, N, K);
}
