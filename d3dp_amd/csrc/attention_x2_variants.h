// The MEASURED-NEGATIVE forms of the EXACT temporal attention kernel (profiles/r04_attn_timeline.md), as far
// as they are separate code: what -DD3DP_ATTN_MIXLO=1, -DD3DP_ATTN_OVERLAP=1 and -DD3DP_ATTN_W16=1 add to attention_x2.hip.
// Not a translation unit of its own: attention_x2.hip includes this file INSIDE its anonymous namespace, behind the helpers the
// code here calls (load_v_frags_x2, pv_chunk_x2_seq, store_o_x2, lds_dma16, wait_vmcnt) and in front of the kernel that selects
// it, and only when one of the three switches is set.  The product library has none of this; tests/test_abi.py holds each
// switch to a build without register spills.  (-DD3DP_ATTN_KPIPE=1 is inline in attn_scores_x2_pair: separating it would
// mean a second copy of the pair loop.)
#pragma once

// -DD3DP_ATTN_MIXLO=1 (measurement build): the lo halves of a pair of probabilities by v_fma_mixlo_f16 / v_fma_mixhi_f16 --
// f16(y - hi) rounded once from the exact difference, which is what convert-back, subtract and convert compute in three
// instructions per element, written straight into the packed register: 3 vector instructions per pair instead of 6.
__device__ __forceinline__ unsigned x2_lo_pair_mix(float y0, float y1, unsigned hpair) {
  unsigned d;
  asm("v_fma_mixlo_f16 %0, %1, 1.0, -%3 op_sel_hi:[0,0,1]\n\t"
      "v_fma_mixhi_f16 %0, %2, 1.0, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
      : "=&v"(d) : "v"(y0), "v"(y1), "v"(hpair));
  return d;
}

// ---- the same softmax in pieces, for the overlapped form of the temporal kernel (D3DP_ATTN_OVERLAP) ------------------------
// mask + row maximum of a score row -> the exponent bias nb (p x 1024 = exp2(s cexp + nb))
template <int NKT, bool MASK_ANY_TILE>
__device__ __forceinline__ float x2_mask_rowmax(f32x4 (&s)[NKT], int n, int lane, float cexp) {
  const int fg = lane >> 4;
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
  return fmaf(-mx, cexp, 10.0f);
}
// key tiles t, t + 1 (t even) of a masked score row -> one split-fp16 B operand pair; the two partial sums continue the
// chains of softmax_split_x2 (same order of additions: slices taken in ascending t give the same denominator bit for bit)
__device__ __forceinline__ void x2_softmax_slice(const f32x4& sa, const f32x4& sb, float nb, float cexp, f16x8& ph, f16x8& pl,
                                                 float (&sum2)[2]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float y = __builtin_amdgcn_exp2f(fmaf(sa[r], cexp, nb));
    sum2[r & 1] += y;
    const f16 h = (f16)y;
    ph[r] = h;
    pl[r] = (f16)fmaf(y, 1.0f, -(float)h);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float y = __builtin_amdgcn_exp2f(fmaf(sb[r], cexp, nb));
    sum2[r & 1] += y;
    const f16 h = (f16)y;
    ph[4 + r] = h;
    pl[4 + r] = (f16)fmaf(y, 1.0f, -(float)h);
  }
}
__device__ __forceinline__ float x2_denominator(const float (&sum2)[2]) {
  float sum = sum2[0] + sum2[1];
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  return sum;
}
// S^T of one query tile (the loop of attn_scores_x2, attention_x2.hip); with OVL the softmax slices of ANOTHER tile's finished score row
// `sp` ride between the MFMAs: the wave's VALU work runs in the shadow of its own matrix instructions instead of after them.
template <int NKT, bool OVL>
__device__ __forceinline__ void x2_scores_rows(const FragBases& fb, int plane, const f16x8 (&qh)[2], const f16x8 (&ql)[2],
                                               f32x4 (&s)[NKT], const f32x4 (&sp)[OVL ? NKT : 1], float nbp, float cexp,
                                               f16x8 (&php)[OVL ? NKT / 2 : 1], f16x8 (&plp)[OVL ? NKT / 2 : 1], float (&sump)[2]) {
  auto read_k = [&](int t, f16x8 (&k)[4]) {
    k[0] = *reinterpret_cast<const f16x8*>(fb.k0 + plane + t * 2048);   // lo, d 0..31
    k[1] = *reinterpret_cast<const f16x8*>(fb.k1 + plane + t * 2048);   // lo, d 32..63
    k[2] = *reinterpret_cast<const f16x8*>(fb.k0 + t * 2048);           // hi
    k[3] = *reinterpret_cast<const f16x8*>(fb.k1 + t * 2048);
  };
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
    if constexpr (OVL) {
      x2_softmax_slice(sp[t], sp[t + 1], nbp, cexp, php[t >> 1], plp[t >> 1], sump);
    }
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
}
// O^T += V^T P^T of one tile (the pipeline of pv_chunks_x2) with the softmax slices of the OTHER tile's score row `sp` between
// the MFMAs of each key chunk: chunk c of this product needs this tile's probabilities only, which are complete.
template <int NKT, int C0>
__device__ __forceinline__ void x2_pv_overlap_rec(const FragBases& fb, int plane, const f16x8 (&ph)[NKT / 2],
                                                  const f16x8 (&pl)[NKT / 2], f32x4 (&o)[4], const f16x8 (&vh)[4],
                                                  const f16x8 (&vl)[4], const f32x4 (&sp)[NKT], float nbp, float cexp,
                                                  f16x8 (&php)[NKT / 2], f16x8 (&plp)[NKT / 2], float (&sump)[2]) {
  f16x8 nh[4], nl[4];
  if constexpr (C0 + 1 < NKT / 2) load_v_frags_x2<C0 + 1>(fb, plane, nh, nl);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int dn = 0; dn < 4; ++dn) o[dn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vl[dn], ph[C0], o[dn], 0, 0, 0);
#pragma unroll
  for (int dn = 0; dn < 4; ++dn) o[dn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh[dn], pl[C0], o[dn], 0, 0, 0);
#pragma unroll
  for (int dn = 0; dn < 4; ++dn) o[dn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh[dn], ph[C0], o[dn], 0, 0, 0);
  x2_softmax_slice(sp[2 * C0], sp[2 * C0 + 1], nbp, cexp, php[C0], plp[C0], sump);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (C0 + 1 < NKT / 2) x2_pv_overlap_rec<NKT, C0 + 1>(fb, plane, ph, pl, o, nh, nl, sp, nbp, cexp, php, plp, sump);
}
template <int NKT>
__device__ __forceinline__ void x2_pv_overlap(const FragBases& fb, int plane, const f16x8 (&ph)[NKT / 2], const f16x8 (&pl)[NKT / 2],
                                              f32x4 (&o)[4], const f32x4 (&sp)[NKT], float nbp, float cexp, f16x8 (&php)[NKT / 2],
                                              f16x8 (&plp)[NKT / 2], float (&sump)[2]) {
  f16x8 vh[4], vl[4];
  load_v_frags_x2<0>(fb, plane, vh, vl);
  x2_pv_overlap_rec<NKT, 0>(fb, plane, ph, pl, o, vh, vl, sp, nbp, cexp, php, plp, sump);
}

// ------------------------------------------------------------------------------------------------
// -DD3DP_ATTN_W16=1 (measurement build; not part of the default library): the temporal split-fp16 kernel as SIXTEEN waves
// of at most 128 registers, one 16-query tile each, the score row in two halves of 128 keys with an online softmax --
// the form VERDICT r3 item 3 named beside progressive DMA.  Four waves per SIMD instead of two cover each other's LDS and
// MFMA latencies (profiles/r04_attn_timeline.md: that, not memory and not the vector-instruction count, is what the
// two-wave form lacks); the price is the order S0, P0.V, S1, P1.V: K(p+1) can only stream in under P1.V and V(p+1) under
// the next problem's S0, every wave reads the whole K / V image for one tile instead of two, and the probabilities of
// the first half are formed against the first half's row maximum and rescaled (one more rounding on that half of O and
// of the denominator: not bit-identical to the two-pass kernel).  256 keys (241..256 frames) only.
#if D3DP_ATTN_W16
// S^T of one query tile against HT key tiles, ONE key tile (four fragments, one accumulator chain of six MFMAs) at a time and
// no register prefetch: the other three waves of the SIMD cover the fragment reads and the chain's latency, and 128
// registers have room for neither a second tile's fragments nor a prefetch
template <int HT>
__device__ __forceinline__ void x2_scores_lean(const FragBases& fb, int plane, const f16x8 (&qh)[2], const f16x8 (&ql)[2],
                                               f32x4 (&s)[HT]) {
#pragma unroll
  for (int t = 0; t < HT; ++t) {
    const f16x8 kl0 = *reinterpret_cast<const f16x8*>(fb.k0 + plane + t * 2048);   // lo, d 0..31
    const f16x8 kl1 = *reinterpret_cast<const f16x8*>(fb.k1 + plane + t * 2048);   // lo, d 32..63
    const f16x8 kh0 = *reinterpret_cast<const f16x8*>(fb.k0 + t * 2048);           // hi
    const f16x8 kh1 = *reinterpret_cast<const f16x8*>(fb.k1 + t * 2048);
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kl0, qh[0], a, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kl1, qh[1], a, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh0, ql[0], a, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh1, ql[1], a, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh0, qh[0], a, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh1, qh[1], a, 0, 0, 0);
    s[t] = a;
    if (t & 1) __builtin_amdgcn_sched_barrier(0);
  }
}
template <int OUTS>
__global__ __launch_bounds__(1024) void attn_temporal_x2_w16_kernel(const float* __restrict__ qkv, void* __restrict__ out_v,
                                                                    SeqMap map, int C, int heads, size_t plane_elems,
                                                                    int n_prob, X2Scales sc) {
  constexpr int NKT = 16, NW = 16, NK = 256, PLANE = NK * 128, HT = NKT / 2;   // HT: key tiles per half
  __shared__ __attribute__((aligned(16))) char kimg[2 * PLANE];
  __shared__ __attribute__((aligned(16))) char vimg[2 * PLANE];
  const int n = map.n_tok;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ts = map.tok_stride;
  const size_t ldb = (size_t)12 * C;
  const float inv_scale = sc.onorm;
  auto opaque = [](int x) { asm volatile("" : "+v"(x)); return x; };
  auto problem_row0 = [&](int p, int& head) -> const char* {
    const int seq = p / heads;
    head = p - seq * heads;
    return reinterpret_cast<const char*>(qkv) + (size_t)ta_seq_base(map, seq) * ldb;
  };
  auto issue_kv = [&](const char* row0, int head, int is_v) {   // pieces wave and wave + 16 of both planes: 4 LDS-DMA
    const int l = opaque(lane);
    const char* g = row0 + (is_v ? 8 : 4) * C + head * 128;
    char* img = is_v ? vimg : kimg;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int pc = wave + j * NW;
      const int row = pc * 8 + (l >> 3);
      const int sw = is_v ? (((row >> 1) & 3) << 1) : ((row >> 1) & 7);
      const char* gj = g + (unsigned)(min(row, n - 1) * ts) * (unsigned)ldb + (((l & 7) ^ sw) << 4);
      lds_dma16(gj, img + pc * 1024);
      lds_dma16(gj + 2 * C, img + PLANE + pc * 1024);
    }
  };
  // The queries by ORDINARY loads (a spill next to a load the compiler does not track would save stale data, and 128 registers
  // are spill territory): requested behind K(p+1), raw in 16 registers through the last P.V, split before the output stores.
  // The compiler waits for them with vmcnt(0), which also covers the older K(p+1) pieces -- landed long before -- and
  // nothing younger: V(p+1) is issued after that point.
  auto load_q = [&](const char* row0, int head, float4 (&qv)[4]) {
    const int l = opaque(lane);
    const int q = wave * 16 + (l & 15);
    const float* qrow = reinterpret_cast<const float*>(row0 + (size_t)min(q, n - 1) * ts * ldb) + head * 64 + (l >> 4) * 8;
    qv[0] = *reinterpret_cast<const float4*>(qrow);
    qv[1] = *reinterpret_cast<const float4*>(qrow + 4);
    qv[2] = *reinterpret_cast<const float4*>(qrow + 32);
    qv[3] = *reinterpret_cast<const float4*>(qrow + 36);
  };
  auto rowmax8 = [&](const f32x4 (&s)[HT]) {
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < HT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[t][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    return fmaxf(mx, __shfl_xor(mx, 32, 64));
  };

  int p = blockIdx.x;
  if (p >= n_prob) return;
  int head;
  const char* row0 = problem_row0(p, head);
  issue_kv(row0, head, 0);
  f16x8 qh[2], ql[2];
  {
    float4 qv[4];
    load_q(row0, head, qv);
    ta_split8(qv[0], qv[1], qh[0], ql[0], sc.q);
    ta_split8(qv[2], qv[3], qh[1], ql[1], sc.q);
  }
  issue_kv(row0, head, 1);
  for (;;) {
    wait_vmcnt<4>();                                   // K(p) landed; the four V pieces may be in flight
    __builtin_amdgcn_s_barrier();                      // 1: K image complete
    f32x4 s[HT];
    f16x8 ph[HT / 2], pl[HT / 2];
    f32x4 o[4];
#pragma unroll
    for (int dn = 0; dn < 4; ++dn) o[dn] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // ---- first half: keys 0..127   (fragment bases re-derived per phase from the opaque lane id: none stays live across phases)
    {
      const FragBases fb = make_frag_bases(kimg, vimg, opaque(lane));
      x2_scores_lean<HT>(fb, PLANE, qh, ql, s);
    }
    const float m0 = rowmax8(s);
    float lsum[2] = {0.f, 0.f};
    {
      const float nb = fmaf(-m0, sc.cexp, 10.0f);
#pragma unroll
      for (int t = 0; t < HT; t += 2) x2_softmax_slice(s[t], s[t + 1], nb, sc.cexp, ph[t >> 1], pl[t >> 1], lsum);
    }
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();                      // 2: V image complete
    {
      const FragBases fb = make_frag_bases(kimg, vimg, opaque(lane));
      pv_chunk_x2_seq<0>(fb, PLANE, ph[0], pl[0], o);
      pv_chunk_x2_seq<1>(fb, PLANE, ph[1], pl[1], o);
      pv_chunk_x2_seq<2>(fb, PLANE, ph[2], pl[2], o);
      pv_chunk_x2_seq<3>(fb, PLANE, ph[3], pl[3], o);
    }
    // ---- second half: keys 128..255 (the tail of the last tile masked)
    {
      const FragBases fb = make_frag_bases(kimg + HT * 2048, vimg, opaque(lane));
      x2_scores_lean<HT>(fb, PLANE, qh, ql, s);
    }
    {
      const int fg = lane >> 4;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (16 * (NKT - 1) + 4 * fg + r >= n) s[HT - 1][r] = -INFINITY;
    }
    const float m = fmaxf(m0, rowmax8(s));
    __builtin_amdgcn_s_barrier();                      // 3: nobody reads the K image any more
    const int pn = p + gridDim.x;
    const bool has_next = pn < n_prob;
    int head_n = 0;
    const char* row0_n = row0;
    float4 qn[4];
    if (has_next) {
      row0_n = problem_row0(pn, head_n);
      issue_kv(row0_n, head_n, 0);
      load_q(row0_n, head_n, qn);
    }
    {
      const float resc = __builtin_amdgcn_exp2f((m0 - m) * sc.cexp);       // <= 1; exactly 1 where the first half holds the maximum
#pragma unroll
      for (int dn = 0; dn < 4; ++dn) o[dn] *= resc;
      lsum[0] *= resc; lsum[1] *= resc;
      const float nb = fmaf(-m, sc.cexp, 10.0f);
#pragma unroll
      for (int t = 0; t < HT; t += 2) x2_softmax_slice(s[t], s[t + 1], nb, sc.cexp, ph[t >> 1], pl[t >> 1], lsum);
    }
    {
      const FragBases fb = make_frag_bases(kimg, vimg + 4 * 4096, opaque(lane));
      pv_chunk_x2_seq<0>(fb, PLANE, ph[0], pl[0], o);
      pv_chunk_x2_seq<1>(fb, PLANE, ph[1], pl[1], o);
      pv_chunk_x2_seq<2>(fb, PLANE, ph[2], pl[2], o);
      pv_chunk_x2_seq<3>(fb, PLANE, ph[3], pl[3], o);
    }
    if (has_next) {                                    // (the current queries are dead: the next problem's take their registers)
      ta_split8(qn[0], qn[1], qh[0], ql[0], sc.q);
      ta_split8(qn[2], qn[3], qh[1], ql[1], sc.q);
    }
    {
      const float denom = x2_denominator(lsum);
      const int tok0 = ta_seq_base(map, p / heads);
      const int l = opaque(lane);
      const int q = wave * 16 + (l & 15);
      if (q < n)
        store_o_x2<OUTS>(o, inv_scale / denom, out_v, (size_t)(tok0 + q * ts), C, head * 64 + (l >> 4) * 4, sc.oplane);
    }
    if (!has_next) break;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                      // 4: nobody reads the V image any more
    issue_kv(row0_n, head_n, 1);
    p = pn; row0 = row0_n; head = head_n;
  }
}
#endif
