// C-ABI layer of libd3dp_hip.so (see include/d3dp_hip.h), part 1 of 5: the per-thread error state, the context's life (d3dp_create:
// plan, find the device, allocate -- the plan and the one reader of the environment switches behind it are ctx_plan.h's --,
// d3dp_destroy), the profile and status calls and the thin wrappers of the sampler / JPMA kernels.  The rest of the layer, one
// concern per file over the shared types of ctx.h:
//   capi_weights.hip  d3dp_set_weights: range proofs and weight packing      capi_ops.hip    the single-op test hooks
//   capi_denoise.hip  the inference schedule, workspace layout, attention route   capi_train.hip  the training step
// D3DP_FAST_F16 (common.h; `make fastf16`) is read in this file alone.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "ctx.h"

namespace {
thread_local std::string g_err;
const char* kClassNames[D3DP_PROFILE_CLASSES] = {"gemm_qkv", "gemm_proj", "gemm_fc1", "gemm_fc2", "attn_spatial",
                                                 "attn_temporal", "layernorm", "norm_pair", "embed_ln", "head",
                                                 "time_mlp", "other",
                                                 "train_linear", "train_wgrad", "train_attn_fwd_spatial", "train_attn_fwd_temporal",
                                                 "train_attn_bwd_q_spatial", "train_attn_bwd_q_temporal", "train_attn_bwd_kv_spatial",
                                                 "train_attn_bwd_kv_temporal", "train_operand_pass", "train_ln_fwd", "train_ln_bwd",
                                                 "train_other", "event_pair_overhead"};
}  // namespace

int d3dp_fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int d3dp_set_error(int code, const char* msg) { return d3dp_fail(code, "%s", msg); }
int d3dp_check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return d3dp_fail(D3DP_EHIP, "%s: %s", what, hipGetErrorString(e));
  return D3DP_OK;
}

extern "C" {

int d3dp_abi_version(void) { return D3DP_ABI_VERSION; }
// test hook (include/d3dp_hip.h, "test hooks"): 1 if this library carries the experiment kernels of gemm_x2.hip
int d3dp_debug_x2_variants(void) { return d3dp_x2_variants_built() ? 1 : 0; }
const char* d3dp_last_error(void) { return g_err.c_str(); }
const char* d3dp_profile_class_name(int32_t cls) {
  return (cls >= 0 && cls < D3DP_PROFILE_CLASSES) ? kClassNames[cls] : "";
}

int d3dp_create(const d3dp_cfg* cfg, d3dp_ctx** out) {
  if (!cfg || !out) return d3dp_fail(D3DP_EINVAL, "d3dp_create: null argument");
  CtxPlan plan;
  if (const int rc = plan_context(*cfg, CtxEnv::from_process(), d3dp_x2_variants_built(), &plan); rc != D3DP_OK) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return d3dp_fail(D3DP_EHIP, "no HIP device visible: libd3dp_hip has no CPU fallback");
  d3dp_ctx* c = new d3dp_ctx();
  static_cast<CtxPlan&>(*c) = plan;
  c->cfg = *cfg;
  c->exact_impl = plan.exact_impl_req;
  c->fast_f16 = c->fast16() ? 1 : (c->fast() ? D3DP_FAST_F16 : 0);   // (FAST16: until d3dp_set_weights has seen the weights)
  HIP_TRY(hipGetDevice(&c->device));
  {
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, c->device));
    c->n_cu = prop.multiProcessorCount;
  }
  if (hipMalloc((void**)&c->d_flag, sizeof(unsigned)) != hipSuccess || hipMemset(c->d_flag, 0, sizeof(unsigned)) != hipSuccess) {
    delete c;
    return d3dp_fail(D3DP_EHIP, "d3dp_create: cannot allocate the status word");
  }
  // The second stream of d3dp_train_backward and its events are made HERE, not on the first step: d3dp_train_backward then creates
  // nothing, and even a context's first step keeps the header's "does not allocate" (tests/test_hip_streams.py).
  // (exactly the contexts whose backward pass forks: split-fp16 Linears and D3DP_TRAIN_OVERLAP not 0)
  if (plan_train_path(*c, c->cfg).needs_aux) {
    bool ok = hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) == hipSuccess;
    for (hipEvent_t& e : c->ev_done) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
      (void)d3dp_destroy(c);
      return d3dp_fail(D3DP_EHIP, "d3dp_create: cannot create the training step's second stream and its events");
    }
  }
  *out = c;
  return D3DP_OK;
}

int d3dp_destroy(d3dp_ctx* c) {
  if (!c) return D3DP_OK;
  for (auto& e : c->pool) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  if (c->arena) (void)hipFree(c->arena);
  if (c->d_flag) (void)hipFree(c->d_flag);
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  for (hipEvent_t e : c->ev_done)
    if (e) (void)hipEventDestroy(e);
  if (c->aux) (void)hipStreamDestroy(c->aux);
  delete c;
  return D3DP_OK;
}

int d3dp_status(d3dp_ctx* c, int32_t* nonfinite) {
  if (!c || !nonfinite) return d3dp_fail(D3DP_EINVAL, "d3dp_status: null argument");
  unsigned v = 0;
  HIP_TRY(hipDeviceSynchronize());                     // every d3dp_denoise issued so far has written its verdict
  HIP_TRY(hipMemcpy(&v, c->d_flag, sizeof v, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(c->d_flag, 0, sizeof v));
  *nonfinite = (int32_t)(v != 0u);                     // bit 0: inf / nan in an output; bit 1: an operand left the split range
  return D3DP_OK;
}

int d3dp_ddim_pre(const float* img, float* xt2, const int32_t* perm, float scale, int32_t B, int32_t H, int32_t F,
                  int32_t J, void* stream) {
  if (!img || !xt2 || !perm || B < 1) return d3dp_fail(D3DP_EINVAL, "d3dp_ddim_pre: bad argument");
  LAUNCH_TRY(d3dp_launch_ddim_pre(img, xt2, perm, scale, B, H * F * J * 3, J, (hipStream_t)stream));
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

int d3dp_ddim_post(const float* pred2, const float* img, const float* noise, const int32_t* perm, float scale,
                   double sqrt_recip, double sqrt_recipm1, float c_xstart, float c_noise, float sigma, int32_t last,
                   float* x_start, size_t xs_bstride, float* img_next, int32_t B, int32_t H, int32_t F, int32_t J,
                   void* stream) {
  if (!pred2 || !perm || !x_start || B < 1) return d3dp_fail(D3DP_EINVAL, "d3dp_ddim_post: bad argument");
  if (!last && (!img || !noise || !img_next)) return d3dp_fail(D3DP_EINVAL, "d3dp_ddim_post: img/noise/img_next required");
  LAUNCH_TRY(d3dp_launch_ddim_post(pred2, img, noise, perm, scale, sqrt_recip, sqrt_recipm1, c_xstart, c_noise, sigma,
                                   last, x_start, xs_bstride, img_next, B, H * F * J * 3, J, (hipStream_t)stream));
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

int d3dp_q_sample(const float* x0, const float* noise, const double* a, const double* s, float scale, float* out,
                  int32_t B, int32_t per_b, void* stream) {
  if (!x0 || !noise || !a || !s || !out || B < 1 || per_b < 1) return d3dp_fail(D3DP_EINVAL, "d3dp_q_sample: bad argument");
  LAUNCH_TRY(d3dp_launch_q_sample(x0, noise, a, s, scale, out, B, per_b, (hipStream_t)stream));
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

int d3dp_jpma(const float* pred, const float* traj, const float* cam, const float* gt2d, const float* gt3d, float* agg,
              int32_t* sel, float* err_sel, float* err_min, int32_t B, int32_t K, int32_t H, int32_t F, int32_t J,
              int32_t zero_root, void* stream) {
  if (!pred || !traj || !cam || !gt2d || !agg || B < 1 || K < 1 || H < 1)
    return d3dp_fail(D3DP_EINVAL, "d3dp_jpma: bad argument");
  if ((err_sel || err_min) && !gt3d) return d3dp_fail(D3DP_EINVAL, "d3dp_jpma: error outputs need gt3d");
  LAUNCH_TRY(d3dp_launch_jpma(pred, traj, cam, gt2d, gt3d, agg, sel, err_sel, err_min, nullptr, nullptr, nullptr, 0, B,
                              K, H, F, J, zero_root ? 0 : -1, 0, (hipStream_t)stream));
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

int d3dp_jpma_gathered(const float* gathered, const float* traj, const float* cam, const float* gt2d, const float* gt3d,
                       float* agg, int32_t* sel, float* err_sel, float* err_min, int32_t R, int32_t B, int32_t K,
                       int32_t H_local, int32_t F, int32_t J, int32_t zero_root, void* stream) {
  if (!gathered || !traj || !cam || !gt2d || !agg || R < 1 || B < 1 || K < 1 || H_local < 1)
    return d3dp_fail(D3DP_EINVAL, "d3dp_jpma_gathered: bad argument");
  if ((err_sel || err_min) && !gt3d) return d3dp_fail(D3DP_EINVAL, "d3dp_jpma_gathered: error outputs need gt3d");
  LAUNCH_TRY(d3dp_launch_jpma(gathered, traj, cam, gt2d, gt3d, agg, sel, err_sel, err_min, nullptr, nullptr, nullptr, 0, B,
                              K, R * H_local, F, J, zero_root ? 0 : -1, 0, (hipStream_t)stream, H_local,
                              (size_t)B * K * H_local * F * J * 3));
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

int d3dp_jpma_ex(const float* pred, const float* traj, const float* cam, const float* gt2d, const float* gt3d, float* agg,
                 int32_t* sel, float* err_sel, float* err_min, float* jbest, float* mean, int32_t B, int32_t K, int32_t H,
                 int32_t F, int32_t J, int32_t root_joint, int32_t linear_projection, void* stream) {
  if (!pred || !traj || !cam || !gt2d || B < 1 || K < 1 || H < 1 || root_joint >= J)
    return d3dp_fail(D3DP_EINVAL, "d3dp_jpma_ex: bad argument");
  if ((err_sel || err_min || jbest) && !gt3d) return d3dp_fail(D3DP_EINVAL, "d3dp_jpma_ex: error / J-Best outputs need gt3d");
  LAUNCH_TRY(d3dp_launch_jpma(pred, traj, cam, gt2d, gt3d, agg, sel, err_sel, err_min, nullptr, jbest, mean, 0, B, K, H,
                              F, J, root_joint, linear_projection, (hipStream_t)stream));
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

int d3dp_jpma_winners(const float* pred, const float* traj, const float* cam, const float* gt2d, float* win,
                      int32_t h_offset, int32_t B, int32_t K, int32_t H, int32_t F, int32_t J, int32_t zero_root,
                      void* stream) {
  if (!pred || !traj || !cam || !gt2d || !win || B < 1 || K < 1 || H < 1 || h_offset < 0)
    return d3dp_fail(D3DP_EINVAL, "d3dp_jpma_winners: bad argument");
  LAUNCH_TRY(d3dp_launch_jpma(pred, traj, cam, gt2d, nullptr, nullptr, nullptr, nullptr, nullptr, win, nullptr, nullptr,
                              h_offset, B, K, H, F, J, zero_root ? 0 : -1, 0, (hipStream_t)stream));
  HIP_TRY(hipGetLastError());
  return D3DP_OK;
}

int d3dp_profile_enable(d3dp_ctx* c, int32_t on) {
  if (!c) return d3dp_fail(D3DP_EINVAL, "null ctx");
  c->prof = on != 0;
  c->used = 0;
  memset(c->counts, 0, sizeof c->counts);
  for (auto& v : c->total_ms) v = 0.0;
  return D3DP_OK;
}

int d3dp_profile_read(d3dp_ctx* c, int64_t* counts, double* total_ms) {
  if (!c || !counts || !total_ms) return d3dp_fail(D3DP_EINVAL, "null argument");
  if (c->flush_events() != 0) return d3dp_fail(D3DP_EHIP, "event read failed");
  for (int i = 0; i < D3DP_PROFILE_CLASSES; ++i) { counts[i] = c->counts[i]; total_ms[i] = c->total_ms[i]; }
  memset(c->counts, 0, sizeof c->counts);
  for (auto& v : c->total_ms) v = 0.0;
  return D3DP_OK;
}

}  // extern "C"
