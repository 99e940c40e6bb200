// The single-op test hooks of libd3dp_hip.so (include/d3dp_hip.h, "test hooks"): one kernel launcher each behind a C entry
// point, so that the tests can hold a kernel against its reference without a context.  Nothing here is on the product's path.
#include "ctx.h"

extern "C" {

// test hook (include/d3dp_hip.h, "test hooks"): the training step's split-fp16 Linear alone, out[M, N] = A[M, K] W[N, K]^T + bias on fp32
// device operands -- absmax, operand passes and gemm_f16x2_dyn_kernel as the step launches them.  tail: 0 = the rows behind the
// last whole 256-row tile as one more row of tiles, 1 = as 16 x 64 blocks at the end of the kernel; | 16 = the one-pass
// instantiation (hi x hi alone: what D3DP_TRAIN_PASSES=1 launches); | 16 | 32 = that product on hi-only operand rows (what
// D3DP_TRAIN_ROWS=hi launches: split2h_dyn_kernel's and gemm_f16x2_dyn_kernel's HI forms; K % 64 == 0); 32 without 16 and any other
// bit are refused.  amax_out: optional pre-zeroed device slot (amax_pos: see kernels.h).  Allocates its operand buffers and synchronises the stream.
int d3dp_debug_train_linear(const float* A, const float* W, const float* bias, float* out, int32_t M, int32_t N, int32_t K,
                            int32_t tail, unsigned* amax_out, int32_t amax_pos, void* stream) {
  if (!A || !W || !out || M < 1 || N < 4 || N % 4 || K < 32 || K % 32) return d3dp_fail(D3DP_EINVAL, "d3dp_debug_train_linear: bad argument");
  if ((tail & ~49) || (tail & 48) == 32)
    return d3dp_fail(D3DP_EINVAL, "d3dp_debug_train_linear: tail = %d (bit 0: remainder rows as 16 x 64 blocks, bit 4: one pass, bit 5 beside "
                             "bit 4: hi-only operand rows)", tail);
  const int passes = (tail & 16) ? 1 : 3, rows_hi = (tail & 32) ? 1 : 0;
  if (rows_hi && K % 64)
    return d3dp_fail(D3DP_EINVAL, "d3dp_debug_train_linear: K = %d under tail | 32: hi-only operand rows are read in whole 128-byte lines of "
                             "64 columns (K %% 64 == 0)", K);
  tail &= 1;
  hipStream_t st = (hipStream_t)stream;
  char* buf = nullptr;
  const size_t a_bytes = (size_t)M * K * 4, w_bytes = (size_t)N * K * 4;
  HIP_TRY(hipMalloc((void**)&buf, a_bytes + w_bytes + 64));
  unsigned* amax = reinterpret_cast<unsigned*>(buf + a_bytes + w_bytes);
  float* uns = reinterpret_cast<float*>(amax + 8);
  int rc = hipMemsetAsync(amax, 0, 64, st) == hipSuccess ? 0 : -3;
  if (!rc) {
    d3dp_launch_absmax(A, (size_t)M * K, amax, st);
    d3dp_launch_absmax(W, (size_t)N * K, amax + 1, st);
    d3dp_launch_split2_dyn(A, buf, M, K, K, amax, uns, st, rows_hi);
    d3dp_launch_split2_dyn(W, buf + a_bytes, N, K, K, amax + 1, uns + 1, st, rows_hi);
    rc = d3dp_launch_linear_f16x2_dyn(buf, buf + a_bytes, bias, uns, uns + 1, out, M, N, K, 1, st, amax_out, amax_pos, tail, passes, rows_hi);
  }
  const hipError_t e = hipStreamSynchronize(st);
  (void)hipFree(buf);
  if (rc) return d3dp_fail(rc == -3 ? D3DP_EHIP : D3DP_EINVAL, "d3dp_debug_train_linear: launch refused (%d)", rc);
  if (e != hipSuccess) return d3dp_fail(D3DP_EHIP, "d3dp_debug_train_linear: %s", hipGetErrorString(e));
  return 0;
}

int d3dp_op_linear(int32_t mode, int32_t epi, const void* A, const void* W, const float* bias, void* out, int32_t M,
                   int32_t N, int32_t K, void* stream) {
  if (!A || !W || !bias || !out) return d3dp_fail(D3DP_EINVAL, "d3dp_op_linear: null argument");
  if (mode == 4 && (epi & 32)) {
    // epi | 32 | (r_in << 8) | (r_out << 12) on fp16 operands: the scaled form of the streaming kernel (gemm_stream_scaled.hip) as a
    // FAST16 context under D3DP_FAST16_RANGE=scale launches it (capi_denoise.hip linear_f16) -- A holds 2^-r_in times its value, the fp16
    // rows leave at 2^-r_out; r_in, r_out in 0 .. 8 (the cap of the contexts).  EPI_GELU takes r_in = 0 (its A is a LayerNorm output).
    const int e = epi & 3, r_in = (epi >> 8) & 15, r_out = (epi >> 12) & 15;
    if ((e != EPI_BIAS && e != EPI_GELU) || (epi & ~(3 | 32 | 0xff00)) || r_in > 8 || r_out > 8 || (e == EPI_GELU && r_in))
      return d3dp_fail(D3DP_EINVAL, "d3dp_op_linear: the scaled form takes epi 0 or 1 | 32 | (r_in << 8) | (r_out << 12) with r_in, r_out "
                                    "<= 8 and r_in = 0 under epi 1; got %d", epi);
    LAUNCH_TRY(d3dp_linear_stream_scaled(e, A, W, bias, out, M, N, K, (hipStream_t)stream, ldexpf(1.f, r_in - r_out), ldexpf(1.f, -r_out),
                                         ldexpf(1.f, r_out)));
  }
  else if (mode == D3DP_MODE_FAST || mode == 4) {
    // epi 0/1: the persistent streaming kernel the denoiser uses (epi | 16 selects its fp32-output form); mode 4: on fp16 operands
    const int e = epi & 3, f32 = (epi & 16) != 0;
    if (e == EPI_RESID || (epi & ~19)) return d3dp_fail(D3DP_EINVAL, "d3dp_op_linear: FAST mode has epilogues 0, 1 and 0|16");
    LAUNCH_TRY(d3dp_launch_linear_bf16_stream(e, f32, A, W, bias, out, M, N, K, (hipStream_t)stream, mode == 4));
  }
  else if (mode == 2) {
    // split-bf16: A, W are three bf16 planes each (d3dp_op_split3); epi 0 -> fp32 out, epi 1 -> three bf16 planes out
    LAUNCH_TRY(d3dp_launch_linear_bf16x3(epi, A, W, bias, (float*)out, out, M, N, K, (hipStream_t)stream));
  }

  else LAUNCH_TRY(d3dp_launch_linear_f32(epi, (const float*)A, (const float*)W, bias, (float*)out, M, N, K, (hipStream_t)stream));
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

int d3dp_op_split3(const float* src, void* dst, size_t n, void* stream) {
  if (!src || !dst) return d3dp_fail(D3DP_EINVAL, "d3dp_op_split3: null argument");
  d3dp_launch_split3(src, dst, n, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

int d3dp_op_linear_x2(int32_t epi, const void* A2, const void* W2, const float* bias, float w_scale, void* out, int32_t M,
                      int32_t N, int32_t K, void* stream) {
  if (!A2 || !W2 || !bias || !out || !(w_scale > 0.f)) return d3dp_fail(D3DP_EINVAL, "d3dp_op_linear_x2: bad argument");
  const int skew_d = (epi >> 8) & 7;                     // epi | (D << 8), D = 1, 2, 4: the skewed schedule (epi 1 and 4)
  const int pingpong = (epi >> 12) & 1 ? 2 : (epi >> 11) & 1;   // epi | 2048: the ping-pong form, | 4096: the wide form (bit-identical results)
  if ((skew_d || pingpong) && !d3dp_x2_variants_built())
    return d3dp_fail(D3DP_ENOTSUP, "d3dp_op_linear_x2: epi flags %d select an experiment kernel this library was built without "
                              "(make -C d3dp_amd/csrc variants)", epi & ~0xff);
  epi &= 255;
  if (epi == EPI_RESID_LN || epi == EPI_GELU_LN || epi == EPI_RESID_NORM) return d3dp_fail(D3DP_EINVAL, "d3dp_op_linear_x2: epilogues 5 / 6 / 7 are internal to d3dp_denoise");
  if (skew_d) {
    int dev = 0;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    if (!d3dp_x2_skew_applies(epi, M, N, K, skew_d, prop.multiProcessorCount))
      return d3dp_fail(D3DP_EINVAL, "d3dp_op_linear_x2: the skewed schedule (D = %d) does not apply to epi %d, M = %d, N = %d, K = %d", skew_d, epi, M, N, K);
  }
  LAUNCH_TRY(d3dp_launch_linear_f16x2(epi, A2, W2, bias, kActUnscale / w_scale, kActScale, (float*)out, out, nullptr, nullptr, M, N, K, (hipStream_t)stream, skew_d, pingpong));
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

int d3dp_op_split2(const float* src, void* dst, size_t n, float scale, void* stream) {
  if (!src || !dst) return d3dp_fail(D3DP_EINVAL, "d3dp_op_split2: null argument");
  if (n % 32 != 0) return d3dp_fail(D3DP_EINVAL, "d3dp_op_split2: n = %zu is not a multiple of 32 (the h2i layout is made of whole 32-column blocks)", n);
  d3dp_launch_split2(src, dst, n, scale, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

int d3dp_op_attention(int32_t act_bf16, int32_t impl, int32_t axis, const void* qkv, void* out, int32_t n_bh, int32_t F,
                      int32_t J, int32_t C, int32_t heads, void* stream) {
  if (!qkv || !out || n_bh < 1) return d3dp_fail(D3DP_EINVAL, "d3dp_op_attention: bad argument");
  hipStream_t st = (hipStream_t)stream;
  if (act_bf16 != 0 && act_bf16 != 1 && act_bf16 != 4) return d3dp_fail(D3DP_EINVAL, "act_bf16 must be 0, 1 or 4 (fp16)");
  const int f16 = act_bf16 == 4;
  // impl = 1 | (s << 16), s = 1 .. 8, on fp16 rows: the scaled forms of the FAST16 attention kernels (attention_fast_scaled.hip) as a
  // context under D3DP_FAST16_RANGE=scale launches them -- q, k and v hold 2^-s times their value, `out` leaves at v's scale.  (Any
  // other value with bits above 7 set goes on to the check of the padded forms, as before.)
  if (f16 && (impl & 0xffff) == 1 && (impl >> 16) >= 1 && (impl >> 16) <= 8) {
    const int s = impl >> 16;
    if (heads < 1 || C % heads || !mfma_head_dim(C / heads))
      return d3dp_fail(D3DP_ENOTSUP, "impl 1 | (s << 16) takes fp16 rows of head dims 64, 32 and 16; C=%d heads=%d is head dim %d", C, heads,
                       heads > 0 ? C / heads : 0);
    if (axis == 0 && J > 256) return d3dp_fail(D3DP_ENOTSUP, "MFMA spatial attention takes up to 256 joints; J=%d", J);
    if (axis == 0) LAUNCH_TRY(d3dp_attn_fast_scaled(J <= 32 ? 0 : 1, qkv, out, n_bh * F, spatial_map(F, J), C, heads, st, ldexpf(1.f, 2 * s)));
    else LAUNCH_TRY(d3dp_attn_fast_scaled(1, qkv, out, n_bh * J, temporal_map(F, J), C, heads, st, ldexpf(1.f, 2 * s)));
    HIP_TRY(hipGetLastError());
    return D3DP_OK;
  }
  // impl = 1 | (true head dim << 8) on 2-byte rows: the padded forms of the FAST attention kernels (attention_fast_pad.hip) -- C / heads is
  // the padded head dim 32 / 64, whose columns beyond the true head dim are zeros in `qkv` and come back as zeros in `out`
  const int hd_true = (impl & 255) == 1 ? impl >> 8 : 0;
  if (hd_true) {
    impl = 1;
    const int hdp = heads > 0 && C % heads == 0 ? C / heads : 0;
    if (!act_bf16 || !((hdp == 32 && hd_true == 24) || (hdp == 64 && (hd_true == 40 || hd_true == 48 || hd_true == 56))))
      return d3dp_fail(D3DP_ENOTSUP, "impl 1 | (true head dim << 8) takes 2-byte rows of head dim 32 holding 24 or 64 holding 40 / 48 / 56; C=%d "
                                "heads=%d true head dim %d is not one", C, heads, hd_true);
  }
  if (impl == 2) {       // EXACT mode: split-fp16 operands on the fp16 matrix cores, fp32 in / fp32 out
    if (act_bf16) return d3dp_fail(D3DP_EINVAL, "split-fp16 attention takes fp32 activations");
    // (refused here, before the temporary exists and the repack kernel runs)
    if (heads < 1 || C % heads || !mfma_head_dim(C / heads))
      return d3dp_fail(D3DP_ENOTSUP, "impl 2 (split-fp16 attention) takes head dims 64, 32 and 16; C=%d heads=%d is head dim %d (the row "
                                "kernel, impl 0, takes it)", C, heads, heads > 0 ? C / heads : 0);
    // the kernels read the packed rows the EXACT qkv Linear writes: repack the fp32 rows into a stream-ordered temporary
    void* packed = nullptr;
    const size_t T = (size_t)n_bh * F * J;
    HIP_TRY(hipMallocAsync(&packed, T * 12 * (size_t)C, st));
    d3dp_launch_qkv_pack_x2((const float*)qkv, packed, T, C, kActScale, st);
    const int rc = d3dp_launch_attn_x2(0, axis, packed, out, axis == 0 ? n_bh * F : n_bh * J,
                                       axis == 0 ? spatial_map(F, J) : temporal_map(F, J), C, heads, kActScale, st);
    HIP_TRY(hipFreeAsync(packed, st));
    LAUNCH_TRY(rc);
  } else if (impl == 1 && act_bf16 && (heads < 1 || C % heads || !mfma_head_dim(C / heads))) {
    return d3dp_fail(D3DP_ENOTSUP, "impl 1 on 2-byte rows takes head dims 64, 32 and 16; C=%d heads=%d is head dim %d (the row kernel, "
                              "impl 0, takes it)", C, heads, heads > 0 ? C / heads : 0);
  } else if (axis == 0 && impl == 1) {
    if (!act_bf16) return d3dp_fail(D3DP_EINVAL, "MFMA spatial attention needs bf16 activations");
    if (J <= 32) LAUNCH_TRY(d3dp_launch_attn_spatial_bf16(qkv, out, n_bh * F, spatial_map(F, J), C, heads, st, f16, hd_true));
    else if (J > 256) return d3dp_fail(D3DP_ENOTSUP, "MFMA spatial attention takes up to 256 joints; J=%d", J);
    else LAUNCH_TRY(d3dp_launch_attn_temporal_bf16(qkv, out, n_bh * F, spatial_map(F, J), C, heads, st, f16, hd_true));   // whole-sequence kernel
  } else if (axis == 0) LAUNCH_TRY(d3dp_launch_attn_rows(act_bf16, qkv, out, n_bh * F, spatial_map(F, J), C, heads, st));
  else if (impl == 1 && !act_bf16) {
    LAUNCH_TRY(d3dp_launch_attn_temporal_f32(0, qkv, out, n_bh * J, temporal_map(F, J), C, heads, st));   // fp32 MFMA
  } else if (impl == 1) {
    if (!act_bf16) return d3dp_fail(D3DP_EINVAL, "MFMA temporal attention needs bf16 activations");
    LAUNCH_TRY(d3dp_launch_attn_temporal_bf16(qkv, out, n_bh * J, temporal_map(F, J), C, heads, st, f16, hd_true));
  } else LAUNCH_TRY(d3dp_launch_attn_rows(act_bf16, qkv, out, n_bh * J, temporal_map(F, J), C, heads, st));
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

int d3dp_op_layernorm(int32_t out_bf16, const float* x, const float* w, const float* b, float eps, void* out, int32_t T,
                      int32_t C, void* stream) {
  if (!x || !w || !b || !out) return d3dp_fail(D3DP_EINVAL, "d3dp_op_layernorm: null argument");
  LAUNCH_TRY(d3dp_launch_ln(out_bf16, const_cast<float*>(x), nullptr, 0, w, b, eps, out, T, C, (hipStream_t)stream));
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

int d3dp_op_to_bf16(const float* src, void* dst, size_t n, void* stream) {
  if (!src || !dst) return d3dp_fail(D3DP_EINVAL, "d3dp_op_to_bf16: null argument");
  d3dp_launch_to_bf16(src, dst, n, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

}  // extern "C"
