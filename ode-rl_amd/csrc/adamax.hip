// adamax.hip -- one-launch Adamax step over every parameter tensor of the model: Vid-ODE's optimizer (Vid-ODE/main.py:187
// `optim.Adamax(netG.parameters(), lr=opt.lr)`), on adam.hip's tensor tables and grid rule (adam_table.h).  HBM-bound elementwise
// work, 4 reads + 3 writes of 4 B per parameter.  Arithmetic in torch.optim.Adamax's order (single-tensor path, maximize off):
//   g += wd*p;  m = b1 m + (1-b1) g;  u = max(b2 u, |g| + eps);  p -= (lr/(1-b1^t)) * m / u
// The infinity norm u is a chain of single roundings (a product, a sum, a maximum), each written out so that nothing is contracted:
// it is torch's exp_inf bit for bit.  The maximum PROPAGATES NaN as torch.maximum does (fmaxf / v_max_f32 return the other operand,
// which would turn a NaN gradient into a plausible update): a NaN gradient leaves NaN in m, u and p of that element.  An infinite
// gradient leaves u = inf and m = +-inf, so m / u is NaN in that step, again as in torch.
//
// Clipping by global norm: odehip_grad_norm (adam.hip) leaves the coefficient on the device, adamax_clip_kernel reads it.  Plain
// launches in stream order, no atomics, no flags, no host read: two runs are bitwise equal.
#include <math.h>
#include <string.h>

#include "adam_table.h"
#include "odehip_internal.h"

namespace odehip {

// max(a, b) of torch.maximum: a NaN in either operand is the result (a > b is false when b is NaN, a != a picks a NaN a)
__device__ __forceinline__ float max_nan(float a, float b) { return (a > b || a != a) ? a : b; }

// one element: gv is the (clipped) gradient before weight decay
__device__ __forceinline__ void adamax_update(float* __restrict__ p, float* __restrict__ m, float* __restrict__ u, long long i, float gv,
                                              float lr_over_bc1, float b1, float b2, float eps, float wd) {
  const float pv = p[i];
  if (wd != 0.0f) gv = __fmaf_rn(wd, pv, gv);   // torch: grad.add(param, alpha=wd), skipped for wd == 0 (g's own bits)
  const float mv = b1 * m[i] + (1.0f - b1) * gv;
  const float uv = max_nan(__fmul_rn(b2, u[i]), __fadd_rn(fabsf(gv), eps));
  m[i] = mv;
  u[i] = uv;
  p[i] = pv - lr_over_bc1 * (mv / uv);
}

__global__ __launch_bounds__(256) void adamax_kernel(AdamTable t, float lr_over_bc1, float b1, float b2, float eps, float wd) {
  const int k = blockIdx.y;
  float* __restrict__ p = t.p[k];
  const float* __restrict__ g = t.g[k];
  float* __restrict__ m = t.m[k];
  float* __restrict__ u = t.v[k];
  const long long n = t.n[k];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    adamax_update(p, m, u, i, g[i], lr_over_bc1, b1, b2, eps, wd);
}

// adamax_kernel on the clipped gradient g * coef, which is also written back (p.grad then holds what torch's clip_grad_norm_ leaves);
// the product is rounded on its own, so coef == 1 gives adamax_kernel's bits
__global__ __launch_bounds__(256) void adamax_clip_kernel(AdamTable t, const float* __restrict__ coef_dev, float lr_over_bc1, float b1,
                                                          float b2, float eps, float wd) {
  const int k = blockIdx.y;
  float* __restrict__ p = t.p[k];
  float* __restrict__ g = const_cast<float*>(t.g[k]);
  float* __restrict__ m = t.m[k];
  float* __restrict__ u = t.v[k];
  const long long n = t.n[k];
  const float coef = coef_dev[0];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float gs = __fmul_rn(g[i], coef);
    g[i] = gs;
    adamax_update(p, m, u, i, gs, lr_over_bc1, b1, b2, eps, wd);
  }
}

// both entry points: coef_dev null = the unclipped step, which (as odehip_adam_step) takes no null tensor pointer at all; the
// clipped one lets a tensor of 0 elements have none
static int adamax_launch(float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_inf, const long long* numel,
                         int n_tensors, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                         const float* coef_dev, void* stream, const char* who) {
  ODEHIP_REQUIRE(step >= 1, "%s: step counts from 1 (got %d)", who, step);
  const float lr_over_bc1 = (float)((double)lr / (1.0 - pow((double)beta1, step)));
  for (int o = 0; o < n_tensors; o += kAdamChunk) {
    AdamTable t;
    memset(&t, 0, sizeof(t));
    const int m = n_tensors - o < kAdamChunk ? n_tensors - o : kAdamChunk;
    long long nmax = 0;
    for (int i = 0; i < m; ++i) {
      ODEHIP_REQUIRE(numel[o + i] >= 0 && ((params[o + i] && grads[o + i] && exp_avg[o + i] && exp_inf[o + i]) ||
                                            (coef_dev && numel[o + i] == 0)),
                     "%s: tensor %d has a null pointer", who, o + i);
      t.p[i] = params[o + i];
      t.g[i] = grads[o + i];
      t.m[i] = exp_avg[o + i];
      t.v[i] = exp_inf[o + i];
      t.n[i] = numel[o + i];
      nmax = numel[o + i] > nmax ? numel[o + i] : nmax;
    }
    if (coef_dev)
      hipLaunchKernelGGL(adamax_clip_kernel, dim3(update_blocks(nmax), m), dim3(256), 0, (hipStream_t)stream, t, coef_dev, lr_over_bc1,
                         beta1, beta2, eps, weight_decay);
    else
      hipLaunchKernelGGL(adamax_kernel, dim3(update_blocks(nmax), m), dim3(256), 0, (hipStream_t)stream, t, lr_over_bc1, beta1, beta2,
                         eps, weight_decay);
  }
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}

}  // namespace odehip

using namespace odehip;

extern "C" int odehip_adamax_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_inf,
                                  const long long* numel, int n_tensors, float lr, float beta1, float beta2, float eps,
                                  float weight_decay, int step, void* stream) {
  ODEHIP_REQUIRE(params && grads && exp_avg && exp_inf && numel && n_tensors >= 0, "adamax_step: null pointer");
  return adamax_launch(params, const_cast<float* const*>(grads), exp_avg, exp_inf, numel, n_tensors, lr, beta1, beta2, eps, weight_decay,
                       step, nullptr, stream, "adamax_step");
}

extern "C" int odehip_adamax_step_clipped(float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_inf,
                                          const long long* numel, int n_tensors, float lr, float beta1, float beta2, float eps,
                                          float weight_decay, int step, const float* coef_dev, void* stream) {
  ODEHIP_REQUIRE(params && grads && exp_avg && exp_inf && numel && coef_dev && n_tensors >= 0, "adamax_step_clipped: null pointer");
  return adamax_launch(params, grads, exp_avg, exp_inf, numel, n_tensors, lr, beta1, beta2, eps, weight_decay, step, coef_dev, stream,
                       "adamax_step_clipped");
}
