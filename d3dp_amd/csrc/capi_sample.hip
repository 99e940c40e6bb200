// The whole DDIM sampler behind one C entry point (include/d3dp_hip.h, "the whole sampler as one call"): d3dp_ddim_steps (the pure
// arithmetic of sampler_plan.h), the workspace layout of a d3dp_sample call (SampleLayout: one function serves the size query and
// the carve), d3dp_sample itself -- every refusal first, then one set-up launch and per step pre-step, d3dp_denoise, post-step, all
// on the caller's stream -- and the single operators behind it: d3dp_op_randn (the generator alone) and the non-flip pre- / post-step.
#include <vector>

#include "ctx.h"
#include "sampler_plan.h"

namespace {

// The caller's workspace of a d3dp_sample call.  nb: the denoiser's batch (2B with flip: x2d | x2d_flip).
struct SampleLayout {
  size_t img, xt2, pred2, trows, x2cat, denoise, denoise_bytes, total;
  int nb;
  int rc;
  SampleLayout(const d3dp_ctx* c, int B, int H, int K, int flip) {
    const d3dp_cfg& g = c->cfg;
    nb = flip ? 2 * B : B;
    const size_t per_b = (size_t)H * g.frames * g.joints * 3;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes); return o; };
    img = take((size_t)B * per_b * (flip ? 4 : 8));
    xt2 = take((size_t)nb * per_b * 4);
    pred2 = take((size_t)nb * per_b * 4);
    trows = take((size_t)K * nb * 8);
    x2cat = take(flip ? (size_t)nb * g.frames * g.joints * 2 * 4 : 0);
    denoise = off;
    denoise_bytes = 0;
    rc = d3dp_workspace_bytes(c, nb, H, &denoise_bytes);
    total = off + denoise_bytes;
  }
};

// B H F J 3 elements and 2B of them must fit the `int` element counts of the launchers
bool shape_fits(const d3dp_ctx* c, int B, int H) {
  const d3dp_cfg& g = c->cfg;
  const unsigned long long n = 2ull * (unsigned long long)B * H * g.frames * g.joints * 3;
  return n < (1ull << 31);
}

}  // namespace

extern "C" {

int d3dp_ddim_steps(const double* alphas_cumprod, int32_t T, int32_t K, double eta, d3dp_ddim_step* out) {
  return plan_ddim_steps(alphas_cumprod, nullptr, nullptr, T, K, eta, out);
}

int d3dp_op_randn(uint64_t seed, uint32_t draw, float* out, uint32_t* bits, size_t n, void* hip_stream) {
  if (!out) return d3dp_fail(D3DP_EINVAL, "d3dp_op_randn: out is null");
  if (n > 0 && (((n - 1) >> 2) >> 32))
    return d3dp_fail(D3DP_EINVAL, "d3dp_op_randn: n = %zu: element index >> 2 does not fit the generator's 32-bit counter word", n);
  LAUNCH_TRY(d3dp_launch_randn(seed, draw, out, bits, n, (hipStream_t)hip_stream));
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

int d3dp_op_ddim_pre_noflip(const double* img, float* xt, float scale, int32_t first, int32_t B, int32_t H, int32_t F, int32_t J,
                            void* hip_stream) {
  if (!img || !xt || B < 1 || H < 1 || F < 1 || J < 1) return d3dp_fail(D3DP_EINVAL, "d3dp_op_ddim_pre_noflip: bad argument");
  LAUNCH_TRY(d3dp_launch_ddim_pre_noflip(img, xt, scale, first != 0, B, H * F * J * 3, (hipStream_t)hip_stream));
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

int d3dp_op_ddim_post_noflip(const float* pred, const double* img, const float* noise, uint64_t seed, uint32_t draw, float scale,
                             double sqrt_recip, double sqrt_recipm1, float c_xstart, double c_noise64, float sigma, int32_t last,
                             float* x_start, size_t xs_bstride, double* img_next, int32_t B, int32_t H, int32_t F, int32_t J,
                             void* hip_stream) {
  if (!pred || !x_start || B < 1 || H < 1 || F < 1 || J < 1) return d3dp_fail(D3DP_EINVAL, "d3dp_op_ddim_post_noflip: bad argument");
  if (!last && (!img || !img_next)) return d3dp_fail(D3DP_EINVAL, "d3dp_op_ddim_post_noflip: img / img_next required unless last");
  LAUNCH_TRY(d3dp_launch_ddim_post_noflip(pred, img, noise, seed, draw, scale, sqrt_recip, sqrt_recipm1, c_xstart, c_noise64, sigma,
                                          last != 0, x_start, xs_bstride, img_next, B, H * F * J * 3, (hipStream_t)hip_stream));
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

int d3dp_sample_workspace_bytes(const d3dp_ctx* c, int32_t B, int32_t H, int32_t K, int32_t flip, size_t* bytes) {
  if (!c || !bytes || B < 1 || H < 1 || K < 1) return d3dp_fail(D3DP_EINVAL, "d3dp_sample_workspace_bytes: bad argument");
  if (!shape_fits(c, B, H)) return d3dp_fail(D3DP_EINVAL, "d3dp_sample_workspace_bytes: B = %d, H = %d: 2 B H F J 3 elements exceed 2^31", B, H);
  const SampleLayout L(c, B, H, K, flip);
  if (L.rc != D3DP_OK) return L.rc;
  *bytes = L.total;
  return D3DP_OK;
}

int d3dp_sample(d3dp_ctx* c, const float* x2d, const float* x2d_flip, const int32_t* perm, float scale, const d3dp_ddim_step* steps,
                int32_t K, const float* noise, uint64_t seed, float* preds, int32_t B, int32_t H, int32_t flip, void* ws,
                size_t ws_bytes, void* hip_stream) {
  // ---- every refusal, before anything is launched ----
  if (!c) return d3dp_fail(D3DP_EINVAL, "d3dp_sample: ctx is null");
  if (c->train())
    return d3dp_fail(D3DP_EINVAL, "d3dp_sample: a D3DP_MODE_TRAIN context does not sample (mode = %d; EXACT, FAST and FAST16 contexts do)", c->cfg.mode);
  if (!x2d || !preds || !ws) return d3dp_fail(D3DP_EINVAL, "d3dp_sample: %s is null", !x2d ? "x2d" : !preds ? "preds" : "ws");
  if (B < 1 || H < 1) return d3dp_fail(D3DP_EINVAL, "d3dp_sample: B = %d, H = %d (both at least 1)", B, H);
  if (const int rc = check_ddim_steps(steps, K); rc != D3DP_OK) return rc;
  if (flip && !x2d_flip) return d3dp_fail(D3DP_EINVAL, "d3dp_sample: x2d_flip is null with flip = %d", flip);
  if (!flip && x2d_flip) return d3dp_fail(D3DP_EINVAL, "d3dp_sample: x2d_flip is given with flip = 0");
  if (flip && !perm) return d3dp_fail(D3DP_EINVAL, "d3dp_sample: perm is null with flip = %d", flip);
  if (!shape_fits(c, B, H)) return d3dp_fail(D3DP_EINVAL, "d3dp_sample: B = %d, H = %d: 2 B H F J 3 elements exceed 2^31", B, H);
  if (!c->weights_set) return d3dp_fail(D3DP_ESTATE, "d3dp_sample: weights not set");
  const d3dp_cfg& g = c->cfg;
  const int per_b = H * g.frames * g.joints * 3, J = g.joints;
  const size_t n = (size_t)B * per_b;
  if (!noise && (((n - 1) >> 2) >> 32))
    return d3dp_fail(D3DP_EINVAL, "d3dp_sample: B H F J 3 = %zu elements: element index >> 2 does not fit the generator's 32-bit counter word", n);
  const SampleLayout L(c, B, H, K, flip);
  if (L.rc != D3DP_OK) return L.rc;
  if (ws_bytes < L.total) return d3dp_fail(D3DP_ESTATE, "d3dp_sample: ws_bytes = %zu < required %zu bytes", ws_bytes, L.total);

  hipStream_t st = (hipStream_t)hip_stream;
  char* const w = (char*)ws;
  float *img32 = flip ? (float*)(w + L.img) : nullptr, *xt2 = (float*)(w + L.xt2), *pred2 = (float*)(w + L.pred2);
  double* img64 = flip ? nullptr : (double*)(w + L.img);
  long long* trows = (long long*)(w + L.trows);
  float* x2cat = flip ? (float*)(w + L.x2cat) : nullptr;
  const int nb = L.nb;

  {
    Scope s(c, P_OTHER, st);
    std::vector<long long> t((size_t)K);
    for (int k = 0; k < K; ++k) t[k] = steps[k].t;
    const size_t nx2_half = flip ? (size_t)B * g.frames * J * 2 : 0;
    for (int k0 = 0; k0 < K; k0 += 64)      // (one launch up to 64 steps; each further launch writes 64 more timestep rows)
      LAUNCH_TRY(d3dp_launch_sample_setup(noise, seed, img32, img64, k0 == 0 ? n : 0, trows, t.data(), k0, std::min(64, K - k0), nb, x2d,
                                          x2d_flip, x2cat, k0 == 0 ? nx2_half : 0, st));
  }
  for (int k = 0; k < K; ++k) {
    const d3dp_ddim_step& s = steps[k];
    {
      Scope sc(c, P_OTHER, st);
      if (flip) LAUNCH_TRY(d3dp_launch_ddim_pre(img32, xt2, perm, scale, B, per_b, J, st));
      else LAUNCH_TRY(d3dp_launch_ddim_pre_noflip(img64, xt2, scale, k == 0, B, per_b, st));
    }
    if (const int rc = d3dp_denoise(c, flip ? x2cat : x2d, xt2, (const int64_t*)(trows + (size_t)k * nb), pred2, nb, H, w + L.denoise,
                                    L.denoise_bytes, hip_stream);
        rc != D3DP_OK)
      return rc;
    {
      Scope sc(c, P_OTHER, st);
      float* const xs = preds + (size_t)k * per_b;
      const size_t xs_bstride = (size_t)K * per_b;
      const float* nz = noise && !s.last ? noise + (size_t)(k + 1) * n : nullptr;   // (draw k + 1; the final step draws none)
      const unsigned draw = (unsigned)(k + 1);
      if (flip && noise)
        LAUNCH_TRY(d3dp_launch_ddim_post(pred2, img32, nz, perm, scale, s.sqrt_recip, s.sqrt_recipm1, s.c_xstart, s.c_noise, s.sigma, s.last,
                                         xs, xs_bstride, img32, B, per_b, J, st));
      else if (flip)
        LAUNCH_TRY(d3dp_launch_ddim_post_gen(pred2, img32, seed, draw, perm, scale, s.sqrt_recip, s.sqrt_recipm1, s.c_xstart, s.c_noise,
                                             s.sigma, s.last, xs, xs_bstride, img32, B, per_b, J, st));
      else
        LAUNCH_TRY(d3dp_launch_ddim_post_noflip(pred2, img64, nz, seed, draw, scale, s.sqrt_recip, s.sqrt_recipm1, s.c_xstart, s.c_noise64,
                                                s.sigma, s.last, xs, xs_bstride, img64, B, per_b, st));
    }
  }
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

}  // extern "C"
