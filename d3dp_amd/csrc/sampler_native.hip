// The kernels d3dp_sample adds to sampler.hip's (include/d3dp_hip.h, "the whole sampler"): the counter-based normal generator, the
// flip post-step with its noise generated in registers, the non-flip forms of the pre- and post-step, and the set-up kernel of a
// call.  All elementwise, HBM-trivial, plain C++ with vector stores; what matters is the arithmetic:
//   - the flip post-step is ddim_post_kernel's (sampler.hip), expression for expression and in its order, with noise[e] replaced by
//     the generator's value for (seed, draw, e);
//   - the non-flip forms are d3dp_amd/model.py's ddim_sample (reference diffusionpose.py:171-212 made to run) at ITS rounding
//     points: there the update x_start c_xstart + c pred_noise + sigma noise adds an fp32 product, an fp64 product (pred_noise
//     stays fp64: the schedule buffers promote it) and an fp32 product, left to right in fp64 -- img is an fp64 tensor from the
//     second step on, and the clamp and the division of the next pre-step run in fp64 before the one rounding to the denoiser's
//     fp32 input.  So the non-flip img lives in the workspace as fp64.  The first step's img is an fp32 tensor: its clamp bound is
//     the double 1.1 scale rounded to fp32, and its fp32 division equals the fp64 one rounded once more (53 >= 2 x 24 + 2);
//   - like sampler.hip this file is compiled with -ffp-contract=off (Makefile): no product and sum below may fuse.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace {

__device__ __forceinline__ float clampf(float x, float lo, float hi) { return x != x ? x : fminf(fmaxf(x, lo), hi); }
__device__ __forceinline__ double clampd(double x, double lo, double hi) { return x != x ? x : fmin(fmax(x, lo), hi); }
// (sampler.hip: the reference's bound is the Python double 1.1 * scale rounded ONCE to fp32)
__device__ __forceinline__ float clamp_bound(float scale) { return (float)(1.1 * (double)scale); }

// ---- Philox4x32-10 (Salmon et al., SC'11; the constants of Random123) ----------------------------------------------------------
// key (seed low, seed high), counter (q, draw, 0, 0): the four words of quad q = e >> 2.  Ten rounds, the key bumped between them.
struct Quad { unsigned w[4]; };

__device__ __forceinline__ Quad philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Quad{{c0, c1, c2, c3}};
}

__device__ __forceinline__ Quad quad_of(unsigned long long seed, unsigned draw, unsigned q) {
  return philox4x32_10(q, draw, 0u, 0u, (unsigned)seed, (unsigned)(seed >> 32));
}

// u = ((x >> 8) + 0.5f) 2^-24 in fp32: at least 2^-25, so the logarithm is finite.  (The sum is rounded to fp32: above 2^23 the
// half ties to even, and x >> 8 = 2^24 - 1 gives u = 1, a radius of 0 or an angle of 2 pi -- never a zero under the logarithm.)
__device__ __forceinline__ float unit_of(unsigned x) { return ((float)(x >> 8) + 0.5f) * 5.9604644775390625e-8f; }

// lane l of a quad: (n0, n1) = sqrt(-2 ln u0) (cos 2 pi u1, sin 2 pi u1), (n2, n3) likewise from (u2, u3)
// (selects, not an indexed read: `l` is a run-time value in the post-steps and the words must stay in registers)
__device__ __forceinline__ float normal_of(unsigned w0, unsigned w1, unsigned w2, unsigned w3, int l) {
  const float r = sqrtf(-2.0f * logf(unit_of((l & 2) ? w2 : w0)));
  const float a = 6.2831855f * unit_of((l & 2) ? w3 : w1);
  return r * ((l & 1) ? sinf(a) : cosf(a));
}
__device__ __forceinline__ float normal_of(const Quad& q, int l) { return normal_of(q.w[0], q.w[1], q.w[2], q.w[3], l); }

// The three noise values of row i (elements 3 i .. 3 i + 2: one or two quads)
__device__ __forceinline__ void normal_row(unsigned long long seed, unsigned draw, size_t i, float& n0, float& n1, float& n2) {
  const size_t e0 = i * 3;
  const unsigned qa = (unsigned)(e0 >> 2), qb = (unsigned)((e0 + 2) >> 2);
  const Quad a = quad_of(seed, draw, qa);
  const Quad b = quad_of(seed, draw, qb);          // (qb == qa for one row in four: the same words again)
  const bool a1 = (unsigned)((e0 + 1) >> 2) == qa;
  n0 = normal_of(a.w[0], a.w[1], a.w[2], a.w[3], (int)(e0 & 3));
  n1 = normal_of(a1 ? a.w[0] : b.w[0], a1 ? a.w[1] : b.w[1], a1 ? a.w[2] : b.w[2], a1 ? a.w[3] : b.w[3], (int)((e0 + 1) & 3));
  n2 = normal_of(b.w[0], b.w[1], b.w[2], b.w[3], (int)((e0 + 2) & 3));
}

// out[e] = the generator's normal for (seed, draw, e); bits[e] (optional) = the Philox word behind it.  One thread per quad.
__global__ __launch_bounds__(256) void randn_kernel(unsigned long long seed, unsigned draw, float* __restrict__ out,
                                                    unsigned* __restrict__ bits, size_t n) {
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q * 4 >= n) return;
  const Quad w = quad_of(seed, draw, (unsigned)q);
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    const size_t e = q * 4 + l;
    if (e < n) {
      out[e] = normal_of(w, l);
      if (bits) bits[e] = w.w[l];
    }
  }
}

// The per-call set-up.  One thread index serves three ranges:
//   img      the initial img, n elements, four per thread: noise0[e] where the caller injects noise, else draw 0 of the generator;
//            fp32 with flip, fp64 without (see the head of this file);
//   trows    the timestep rows [k0 + kk][nb] int64 of the steps of this launch (`t`: their timesteps, by value);
//   x2cat    x2d followed by x2d_flip as ONE (2 B, F, J, 2) tensor, the denoiser's input of a flip call (nx2 elements; 0 without).
struct StepTimes { long long t[64]; };

__global__ __launch_bounds__(256) void sample_setup_kernel(const float* __restrict__ noise0, unsigned long long seed, float* __restrict__ img32,
                                                           double* __restrict__ img64, size_t n, long long* __restrict__ trows,
                                                           StepTimes t, int n_t, int nb, const float* __restrict__ x2d,
                                                           const float* __restrict__ x2f, float* __restrict__ x2cat, size_t nx2_half) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i * 4 < n) {
    Quad w{};
    if (!noise0) w = quad_of(seed, 0u, (unsigned)i);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const size_t e = i * 4 + l;
      if (e < n) {
        const float v = noise0 ? noise0[e] : normal_of(w, l);
        if (img64) img64[e] = (double)v;
        else img32[e] = v;
      }
    }
  }
  if (i < (size_t)n_t * nb) trows[i] = t.t[i / nb];
  if (i < 2 * nx2_half) x2cat[i] = i < nx2_half ? x2d[i] : x2f[i - nx2_half];
}

// ddim_post_kernel (sampler.hip) with the noise of (seed, draw) generated in registers: same expressions, same order.
// (img_next may be img, as there: neither is declared restrict here)
__global__ __launch_bounds__(256) void ddim_post_gen_kernel(const float* __restrict__ pred2, const float* img,
                                                            unsigned long long seed, unsigned draw, const int* __restrict__ perm,
                                                            float scale, double sqrt_recip, double sqrt_recipm1, float c_xstart,
                                                            float c_noise, float sigma, int last, float* __restrict__ x_start,
                                                            size_t xs_bstride, float* img_next, size_t total,
                                                            size_t per_b_rows, int J) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const float lim = clamp_bound(scale);
  const int j = (int)(i % J);
  const size_t src = total + (i - j + perm[j]);
  const size_t b = i / per_b_rows, r = i % per_b_rows;
  float n0 = 0.f, n1 = 0.f, n2 = 0.f;
  if (!last) normal_row(seed, draw, i, n0, n1, n2);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float pf = pred2[src * 3 + c];
    if (c == 0) pf = -pf;
    const float pred = __fadd_rn(pred2[i * 3 + c], pf) / 2.0f;
    const float xs = clampf(__fmul_rn(pred, scale), -lim, lim);
    x_start[b * xs_bstride + r * 3 + c] = xs;
    if (!last) {
      const float x = img[i * 3 + c];
      const float pn = (float)((sqrt_recip * (double)x - (double)xs) / sqrt_recipm1);
      const float v = __fadd_rn(__fadd_rn(__fmul_rn(xs, c_xstart), __fmul_rn(c_noise, pn)), __fmul_rn(sigma, c == 0 ? n0 : c == 1 ? n1 : n2));
      img_next[i * 3 + c] = v;
    }
  }
}

// x_t = float(clamp(img, +-1.1 s) / s) without flip (model.py ddim_sample).  first: img holds fp32 values (the initial noise) and
// the reference clamps an fp32 tensor -- the bound is fp32(1.1 s); afterwards img is fp64 and so is the bound.
__global__ __launch_bounds__(256) void ddim_pre_noflip_kernel(const double* __restrict__ img, float* __restrict__ xt, float scale,
                                                              int first, size_t n) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const double lim = first ? (double)clamp_bound(scale) : 1.1 * (double)scale;
  xt[e] = (float)(clampd(img[e], -lim, lim) / (double)scale);
}

// x_start = clamp(pred s, +-1.1 s) (fp32); unless last:
//   pred_noise = (sqrt_recip img - x_start) / sqrt_recipm1                                      (fp64, kept)
//   img_next   = (double(x_start c_xstart) + c_noise64 pred_noise) + double(sigma noise)        (the two outer products in fp32)
// noise: the injected tensor, or null for the generator's (seed, draw).  One thread per row of 3, like the flip form, so that
// both read the generator the same way.
__global__ __launch_bounds__(256) void ddim_post_noflip_kernel(const float* __restrict__ pred, const double* img,
                                                               const float* __restrict__ noise, unsigned long long seed, unsigned draw,
                                                               float scale, double sqrt_recip, double sqrt_recipm1, float c_xstart,
                                                               double c_noise64, float sigma, int last, float* __restrict__ x_start,
                                                               size_t xs_bstride, double* img_next, size_t total,
                                                               size_t per_b_rows) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const float lim = clamp_bound(scale);
  const size_t b = i / per_b_rows, r = i % per_b_rows;
  float n0 = 0.f, n1 = 0.f, n2 = 0.f;
  if (!last) {
    if (noise) {
      n0 = noise[i * 3];
      n1 = noise[i * 3 + 1];
      n2 = noise[i * 3 + 2];
    } else {
      normal_row(seed, draw, i, n0, n1, n2);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float xs = clampf(__fmul_rn(pred[i * 3 + c], scale), -lim, lim);
    x_start[b * xs_bstride + r * 3 + c] = xs;
    if (!last) {
      const double pn = (sqrt_recip * img[i * 3 + c] - (double)xs) / sqrt_recipm1;
      const double v = ((double)__fmul_rn(xs, c_xstart) + c_noise64 * pn) + (double)__fmul_rn(sigma, c == 0 ? n0 : c == 1 ? n1 : n2);
      img_next[i * 3 + c] = v;
    }
  }
}

inline unsigned blocks_of(size_t threads) { return (unsigned)((threads + 255) / 256); }

}  // namespace

int d3dp_launch_randn(unsigned long long seed, unsigned draw, float* out, unsigned* bits, size_t n, hipStream_t st) {
  if (n == 0) return 0;
  if (((n - 1) >> 2) >> 32) return -1;
  hipLaunchKernelGGL(randn_kernel, dim3(blocks_of((n + 3) / 4)), dim3(256), 0, st, seed, draw, out, bits, n);
  return 0;
}

int d3dp_launch_sample_setup(const float* noise0, unsigned long long seed, float* img32, double* img64, size_t n, long long* trows,
                             const long long* t, int k0, int n_t, int nb, const float* x2d, const float* x2f, float* x2cat,
                             size_t nx2_half, hipStream_t st) {
  if (n_t < 0 || n_t > 64 || nb < 1) return -1;
  StepTimes tt{};
  for (int k = 0; k < n_t; ++k) tt.t[k] = t[k0 + k];
  // (a launch behind the first writes timestep rows alone: n = 0, nx2_half = 0)
  const size_t threads = std::max(std::max((n + 3) / 4, (size_t)n_t * nb), 2 * nx2_half);
  if (threads == 0) return 0;
  hipLaunchKernelGGL(sample_setup_kernel, dim3(blocks_of(threads)), dim3(256), 0, st, noise0, seed, img32, img64, n,
                     trows + (size_t)k0 * nb, tt, n_t, nb, x2d, x2f, x2cat, nx2_half);
  return 0;
}

int d3dp_launch_ddim_post_gen(const float* pred2, const float* img, unsigned long long seed, unsigned draw, const int* perm, float scale,
                              double sqrt_recip, double sqrt_recipm1, float c_xstart, float c_noise, float sigma, int last,
                              float* x_start, size_t xs_bstride, float* img_next, int B, int per_b, int J, hipStream_t st) {
  const size_t total = (size_t)B * per_b / 3;
  hipLaunchKernelGGL(ddim_post_gen_kernel, dim3(blocks_of(total)), dim3(256), 0, st, pred2, img, seed, draw, perm, scale,
                     sqrt_recip, sqrt_recipm1, c_xstart, c_noise, sigma, last, x_start, xs_bstride, img_next, total,
                     (size_t)per_b / 3, J);
  return 0;
}

int d3dp_launch_ddim_pre_noflip(const double* img, float* xt, float scale, int first, int B, int per_b, hipStream_t st) {
  const size_t n = (size_t)B * per_b;
  hipLaunchKernelGGL(ddim_pre_noflip_kernel, dim3(blocks_of(n)), dim3(256), 0, st, img, xt, scale, first, n);
  return 0;
}

int d3dp_launch_ddim_post_noflip(const float* pred, const double* img, const float* noise, unsigned long long seed, unsigned draw,
                                 float scale, double sqrt_recip, double sqrt_recipm1, float c_xstart, double c_noise64, float sigma,
                                 int last, float* x_start, size_t xs_bstride, double* img_next, int B, int per_b, hipStream_t st) {
  const size_t total = (size_t)B * per_b / 3;
  hipLaunchKernelGGL(ddim_post_noflip_kernel, dim3(blocks_of(total)), dim3(256), 0, st, pred, img, noise, seed, draw, scale,
                     sqrt_recip, sqrt_recipm1, c_xstart, c_noise64, sigma, last, x_start, xs_bstride, img_next, total,
                     (size_t)per_b / 3);
  return 0;
}
