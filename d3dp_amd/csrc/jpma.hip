// JPMA: joint-wise reprojection-based multi-hypothesis aggregation, the consumer of the sampler's (and, on N GPUs,
// the all-gather's) output -- SURVEY.md §8(f) row N1.  One fused pass replaces the reference's chain of
// (B,K,H,F,J,*) temporaries (main.py:700-712 root zeroing + trajectory add, camera.py:30-60 project_to_2d,
// loss.py:54-76 per-joint argmin of the 2D error over hypotheses + gather; main_3dhp.py:797-835 materialises the
// aggregated poses the same way).
//
// One thread per (b, k, f, j): loops over the H hypotheses (stride F*J*3 floats: coalesced across threads), keeps the
// first minimum like torch.min, writes the selected 3D joint and, optionally, the 3D errors needed for the four
// metrics.  HBM-bound: reads B*K*H*F*J*3 floats once.
#include "common.h"
#include "kernels.h"

namespace {

// torch.clamp semantics (camera.py:44): NaN stays NaN (0 / 0 at a zero depth) -- fminf / fmaxf alone would make it -1
__device__ __forceinline__ float clamp1(float v) { return v != v ? v : fminf(fmaxf(v, -1.f), 1.f); }

// torch.min semantics (loss.py:39,67) for a running minimum that STARTS at hypothesis 0: a later value replaces it when
// it is smaller, or when it is the first NaN; a NaN, once held, stays.  Ties and an all-+inf row keep the first index.
__device__ __forceinline__ bool min_takes(float e, float best) { return e < best || (e != e && best == best); }

// The selection below is INDEX work: it must pick the hypothesis the reference picks, so every float operation is
// written out in the reference's order with explicit single roundings (__fmul_rn / __fadd_rn are never contracted into
// fma), and the two Euclidean norms follow torch.norm's CPU kernel, which accumulates squares with fma:
// sqrt(fma(x1, x1, x0 * x0)) and sqrt(fma(x2, x2, fma(x1, x1, x0 * x0))).  Checked bit for bit against torch on the
// host (200 k random points per expression) and, on the GPU, against fixtures g5 / g11 with exact equality.
__device__ __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float norm2(float a, float b) { return sqrtf(fmaf(b, b, mul(a, a))); }
__device__ __forceinline__ float norm3(float a, float b, float c) { return sqrtf(fmaf(c, c, fmaf(b, b, mul(a, a)))); }

// Human3.6M projection with radial + tangential distortion, camera.py:30-60 (same fp32 operation order:
// r2 = sum(XX^2); radial = 1 + sum(k * (r2, r2^2, r2^3)); tan = sum(p * XX); f * (XX * (radial + tan) + p * r2) + c)
__device__ __forceinline__ void project(const float* X, const float* cam, float& u, float& v) {
  const float xx = clamp1(X[0] / X[2]), yy = clamp1(X[1] / X[2]);
  const float r2 = add(mul(xx, xx), mul(yy, yy));
  const float r4 = mul(r2, r2), r6 = mul(r4, r2);
  const float radial = add(1.f, add(add(mul(cam[4], r2), mul(cam[5], r4)), mul(cam[6], r6)));
  const float tan = add(mul(cam[7], xx), mul(cam[8], yy));
  const float rt = add(radial, tan);
  u = add(mul(cam[0], add(mul(xx, rt), mul(cam[7], r2))), cam[2]);
  v = add(mul(cam[1], add(mul(yy, rt), mul(cam[8], r2))), cam[3]);
}

__global__ __launch_bounds__(256) void jpma_kernel(const float* __restrict__ pred, const float* __restrict__ traj,
                                                   const float* __restrict__ cam, const float* __restrict__ gt2d,
                                                   const float* __restrict__ gt3d, float* __restrict__ agg,
                                                   int* __restrict__ sel, float* __restrict__ err_sel,
                                                   float* __restrict__ err_min, float* __restrict__ win,
                                                   float* __restrict__ jbest, float* __restrict__ mean, int h_offset,
                                                   int B, int K, int H, int F, int J, int root_joint, int linear,
                                                   int h_inner, size_t outer_stride) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t FJ = (size_t)F * J, total = (size_t)B * K * FJ;
  if (i >= total) return;
  const size_t fj = i % FJ, bk = i / FJ, b = bk / K;
  const int j = (int)(fj % J);
  const size_t f = fj / J;
  float c[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) c[q] = cam[q];
  const float* tr = traj + (b * F + f) * 3;
  const float g2u = gt2d[(b * FJ + fj) * 2], g2v = gt2d[(b * FJ + fj) * 2 + 1];
  float g3[3] = {0.f, 0.f, 0.f};
  if (gt3d != nullptr) { g3[0] = gt3d[(b * FJ + fj) * 3]; g3[1] = gt3d[(b * FJ + fj) * 3 + 1]; g3[2] = gt3d[(b * FJ + fj) * 3 + 2]; }
  // hypothesis h = r h_inner + hl lives at pred[r outer_stride + ((bk h_inner + hl) FJ + fj) 3]: h_inner = H (one contiguous
  // (B,K,H,F,J,3) tensor) or the per-rank count of an all-gather result (R,B,K,H_local,F,J,3) consumed in place
  const float* p = pred + (bk * h_inner * FJ + fj) * 3;
  float best2 = INFINITY, bx = 0.f, by = 0.f, bz = 0.f, best3 = 0.f, min3 = INFINITY;
  float mx = 0.f, my = 0.f, mz = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;      // pose of the smallest 3D error; running sum
  int bh = 0;
  for (int h = 0, hl = 0; h < H; ++h, ++hl, p += FJ * 3) {
    if (hl == h_inner) { hl = 0; p += outer_stride - (size_t)h_inner * FJ * 3; }      // next rank's block
    float x[3] = {p[0], p[1], p[2]};
    if (j == root_joint) { x[0] = 0.f; x[1] = 0.f; x[2] = 0.f; }          // main.py:700 (joint 0), main_3dhp.py:777 (14)
    const float a[3] = {add(x[0], tr[0]), add(x[1], tr[1]), add(x[2], tr[2])};   // main.py:706-707
    float u, v;
    if (linear) {                                                         // camera.py:62-83 project_to_2d_linear
      u = add(mul(c[0], clamp1(a[0] / a[2])), c[2]);
      v = add(mul(c[1], clamp1(a[1] / a[2])), c[3]);
    } else {
      project(a, c, u, v);
    }
    const float e2 = norm2(u - g2u, v - g2v);                             // loss.py:66 torch.norm
    const float e3 = norm3(x[0] - g3[0], x[1] - g3[1], x[2] - g3[2]);     // loss.py:65
    if (h == 0 || min_takes(e3, min3)) { min3 = e3; mx = x[0]; my = x[1]; mz = x[2]; }
    sx += x[0]; sy += x[1]; sz += x[2];
    if (h == 0 || min_takes(e2, best2)) { best2 = e2; bh = h; bx = x[0]; by = x[1]; bz = x[2]; best3 = e3; }
  }
  if (agg != nullptr) { agg[i * 3] = bx; agg[i * 3 + 1] = by; agg[i * 3 + 2] = bz; }
  if (sel != nullptr) sel[i] = bh;
  if (err_sel != nullptr) err_sel[i] = best3;     // J_Agg per-joint error (loss.py:70-72)
  if (err_min != nullptr) err_min[i] = min3;      // J_Best per-joint error (loss.py:38-41)
  if (jbest != nullptr) { jbest[i * 3] = mx; jbest[i * 3 + 1] = my; jbest[i * 3 + 2] = mz; }   // main_3dhp.py:798-801
  if (mean != nullptr) { mean[i * 3] = sx / H; mean[i * 3 + 1] = sy / H; mean[i * 3 + 2] = sz / H; }   // P-Agg pose
  if (win != nullptr) {                           // this rank's winner for the reduced exchange
    win[i * 5] = best2; win[i * 5 + 1] = bx; win[i * 5 + 2] = by; win[i * 5 + 3] = bz;
    win[i * 5 + 4] = __int_as_float(h_offset + bh);
  }
}

}  // namespace

int d3dp_launch_jpma(const float* pred, const float* traj, const float* cam, const float* gt2d, const float* gt3d,
                     float* agg, int* sel, float* err_sel, float* err_min, float* win, float* jbest, float* mean,
                     int h_offset, int B, int K, int H, int F, int J, int root_joint, int linear, hipStream_t st,
                     int h_inner, size_t outer_stride) {
  if (h_inner <= 0) h_inner = H;
  if (H % h_inner != 0) return -1;
  const size_t total = (size_t)B * K * F * J;
  hipLaunchKernelGGL(jpma_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, pred, traj, cam, gt2d, gt3d,
                     agg, sel, err_sel, err_min, win, jbest, mean, h_offset, B, K, H, F, J, root_joint, linear, h_inner, outer_stride);
  return 0;
}
