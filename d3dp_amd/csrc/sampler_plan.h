// What d3dp_ddim_steps computes and what d3dp_sample decides before it launches anything: the DDIM step table of a (T, K, eta)
// schedule -- D3DP.time_pairs() and the host coefficient arithmetic of d3dp_amd/model.py, bit for bit -- and the checks of a step
// table handed to d3dp_sample.  Pure host arithmetic over a caller's alphas_cumprod: no HIP here, so that any machine can check
// it (tests/test_sampler_plan_host.py through tests/sampler_plan_driver.cpp).
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/d3dp_hip.h"

// The one error function (capi.hip; declared in ctx_plan.h too): formats d3dp_last_error()'s message and returns `code`
int d3dp_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// torch.linspace(-1, T - 1, steps = K + 1) in float32, element i, then .int(): torch's two-sided formula -- step = (end - start) /
// (steps - 1) rounded once; below the middle start + step i, from it on end - step (steps - 1 - i); product and sum each rounded to
// float32 on their own (the volatiles keep a compiler from contracting them into an fma or carrying extra precision) -- and the
// truncation toward zero of the conversion.
inline int32_t ddim_linspace_int(int32_t T, int32_t K, int32_t i) {
  const int32_t steps = K + 1;
  const float start = -1.0f, end = (float)(T - 1);
  volatile float step = (end - start) / (float)(steps - 1);
  volatile float prod;
  volatile float v;
  if (i < steps / 2) {
    prod = step * (float)i;
    v = start + prod;
  } else {
    prod = step * (float)(steps - 1 - i);
    v = end - prod;
  }
  return (int32_t)v;
}

// The step table.  Step k runs at time = times[K - k] and moves to time_next = times[K - k - 1] (the reversed list of
// D3DP.time_pairs()); the last step alone has time_next < 0.  Per step, from the caller's alphas_cumprod (never re-derived from
// the cosine schedule: libm's cos need not be torch's):
//   sqrt_recip   = sqrt(1 / ac[time])           the buffers sqrt_recip_alphas_cumprod / sqrt_recipm1_alphas_cumprod
//   sqrt_recipm1 = sqrt(1 / ac[time] - 1)       (diffusionpose.py:109-110), one correct rounding per operation
//   sigma   = eta sqrt((1 - a / a') (1 - a') / (1 - a)),  a = ac[time], a' = ac[time_next]      (diffusionpose.py:248-249)
//   c_noise = sqrt(1 - a' - sigma^2),  c_xstart = sqrt(a')
// The three coefficients are Python doubles in ddim_sample_flip (math.sqrt: correctly rounded, like std::sqrt), so they equal
// Python's bit for bit.  The two buffers are torch TENSORS, and torch's CPU sqrt of an fp64 tensor is not correctly rounded: it
// differs from sqrt() in the last bit at 14 + 9 of the 1000 entries of the cosine schedule (about 0.7 % of random inputs).  The
// Python sampler reads the buffers, which also travel in every checkpoint: a host that holds them hands them in (sr, srm1: [T],
// or null) and the table carries THEIR entries; without them the fields are the correctly rounded values.
// ddim_sample_flip forms sigma^2 as the Python expression sg ** 2, which is libm's pow(sg, 2.0), while ddim_sample forms it on
// fp64 tensors, where torch's pow takes the exponent 2 as sigma * sigma.  A correctly rounded pow gives the product's bits, but
// libm does not promise one, so the table carries both: c_noise (float, pow: what d3dp_ddim_post receives) and c_noise64 (double,
// product: the 0-dim fp64 tensor the non-flip update multiplies the fp64 noise prediction with -- ddim_sample computes it on the
// DEVICE, whose fp64 division and sqrt are correctly rounded; tests/test_hip_sampler_native.py holds the table to the device's
// values).  The exponent goes through a volatile so that no compiler rewrites the call.
inline int plan_ddim_steps(const double* ac, const double* sr, const double* srm1, int32_t T, int32_t K, double eta, d3dp_ddim_step* out) {
  if (!ac || !out) return d3dp_fail(D3DP_EINVAL, "d3dp_ddim_steps: null argument");
  if (T < 1) return d3dp_fail(D3DP_EINVAL, "d3dp_ddim_steps: T = %d (the schedule has at least one timestep)", T);
  if (K < 1) return d3dp_fail(D3DP_EINVAL, "d3dp_ddim_steps: K = %d (at least one sampling step)", K);
  if (K > T) return d3dp_fail(D3DP_EINVAL, "d3dp_ddim_steps: K = %d sampling steps of a schedule of T = %d", K, T);
  volatile double two = 2.0;
  for (int32_t k = 0; k < K; ++k) {
    const int32_t time = ddim_linspace_int(T, K, K - k), time_next = ddim_linspace_int(T, K, K - k - 1);
    if (time < 0 || time >= T || time_next >= T)
      return d3dp_fail(D3DP_EINVAL, "d3dp_ddim_steps: step %d runs at time %d -> %d outside the schedule of T = %d", k, time, time_next, T);
    d3dp_ddim_step& s = out[k];
    s.t = time;
    s.sqrt_recip = sr ? sr[time] : std::sqrt(1.0 / ac[time]);
    s.sqrt_recipm1 = srm1 ? srm1[time] : std::sqrt(1.0 / ac[time] - 1.0);
    s.last = time_next < 0 ? 1 : 0;
    if (s.last) {
      s.c_xstart = s.c_noise = s.sigma = 0.0f;
      s.c_noise64 = 0.0;
      continue;
    }
    const double alpha = ac[time], alpha_next = ac[time_next];
    const double sg = eta * std::sqrt((1.0 - alpha / alpha_next) * (1.0 - alpha_next) / (1.0 - alpha));
    s.c_noise = (float)std::sqrt(1.0 - alpha_next - std::pow(sg, two));
    s.c_noise64 = std::sqrt(1.0 - alpha_next - sg * sg);
    s.c_xstart = (float)std::sqrt(alpha_next);
    s.sigma = (float)sg;
  }
  return D3DP_OK;
}

// A step table as d3dp_sample takes it: `last` set at the final step and nowhere else, timesteps that index a schedule.
inline int check_ddim_steps(const d3dp_ddim_step* steps, int32_t K) {
  if (K < 1) return d3dp_fail(D3DP_EINVAL, "d3dp_sample: K = %d (at least one sampling step)", K);
  if (!steps) return d3dp_fail(D3DP_EINVAL, "d3dp_sample: steps is null");
  for (int32_t k = 0; k < K; ++k) {
    if (steps[k].t < 0) return d3dp_fail(D3DP_EINVAL, "d3dp_sample: steps[%d].t = %lld is negative", k, (long long)steps[k].t);
    if ((steps[k].last != 0) != (k == K - 1))
      return d3dp_fail(D3DP_EINVAL, "d3dp_sample: steps[%d].last = %d (set at the final step, %d, and nowhere else)", k, steps[k].last, K - 1);
  }
  return D3DP_OK;
}
