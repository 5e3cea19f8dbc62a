// optim_step.hip -- the one-launch optimizer steps over every parameter tensor of the model, and gradient clipping by global norm.
// HBM-bound elementwise work: 4 reads + 3 writes of 4 B per parameter; the ODEConvGRU model has 1.04 M parameters in 40 tensors, so
// the point is ONE launch per 24 tensors instead of a launch per tensor and op.
//
// Adam (train_test.py:24,205 `optim.Adam(model.parameters(), lr=opt.lr)`), torch.optim.Adam's order, amsgrad off:
//   g += wd*p;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g*g;  p -= (lr/(1-b1^t)) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
// Adamax (Vid-ODE/main.py:187 `optim.Adamax(netG.parameters(), lr=opt.lr)`), torch.optim.Adamax's order, single-tensor path, maximize off:
//   g += wd*p;  m = b1 m + (1-b1) g;  u = max(b2 u, |g| + eps);  p -= (lr/(1-b1^t)) * m / u
// The infinity norm u is a chain of single roundings (a product, a sum, a maximum), each written out so that nothing is contracted:
// it is torch's exp_inf bit for bit.  The maximum PROPAGATES NaN as torch.maximum does (fmaxf / v_max_f32 return the other operand,
// which would turn a NaN gradient into a plausible update): a NaN gradient leaves NaN in m, u and p of that element.  An infinite
// gradient leaves u = inf and m = +-inf, so m / u is NaN in that step, again as in torch.
//
// Gradient clipping by global norm (train_test.py:187-195 `clip_grad_norm_(model.parameters(), opt.clip)`) rides on the same tensor
// tables.  A global norm needs every workgroup's partial sum before any parameter may move; here STREAM ORDER between plain launches
// is that barrier: grad_sqsum_kernel (one float64 partial per workgroup, plain stores) -> grad_norm_finish_kernel (one workgroup:
// reduce.h's ordered sum of the partials, then total_norm, coef, clipped_norm as three floats on the device) -> a clipping update
// kernel or grad_scale_kernel, which read coef from that buffer.  No cooperative launch, no flag one kernel waits on, no atomics, no
// host read: two runs are bitwise equal and nothing can hang.  coef is torch's expression in fp32, clamp(reciprocal(total_norm + 1e-6)
// * max_norm, max = 1): a NaN norm gives a NaN coefficient (error_if_nonfinite=False), an Inf norm a coefficient of 0.
#include <math.h>
#include <string.h>

#include "odehip_internal.h"
#include "reduce.h"

namespace odehip {

constexpr int kAdamChunk = 24;  // tensors per launch (pointers travel as kernel arguments)
struct AdamTable {
  float* p[kAdamChunk];
  float* g[kAdamChunk];   // written only by the clipping kernels
  float* m[kAdamChunk];
  float* v[kAdamChunk];   // the second state tensor: Adam's exp_avg_sq, Adamax's exp_inf
  long long n[kAdamChunk];
};
struct GradTable {
  float* g[kAdamChunk];
  long long n[kAdamChunk];
};

// workgroups per tensor of an elementwise launch over a chunk whose largest tensor has nmax elements
static inline int update_blocks(long long nmax) {
  const long long b = (nmax + 255) / 256;
  return b < 1 ? 1 : (b > 1024 ? 1024 : (int)b);
}

// ---- the update rules: one element; gv is the (clipped) gradient before weight decay ------------------------------------------------

__device__ __forceinline__ void adam_update(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, long long i, float gv,
                                            float lr_over_bc1, float inv_sqrt_bc2, float b1, float b2, float eps, float wd) {
  // every rounding is written out: which products the compiler fuses into an fma depends on the code around the expression, and
  // these are the ones the step has always had (the bits of the checkpoints and of the tests' tolerances)
  const float pv = p[i];
  gv = __fmaf_rn(wd, pv, gv);
  const float mv = __fmaf_rn(1.0f - b1, gv, __fmul_rn(b1, m[i]));
  const float vv = __fadd_rn(__fmul_rn(b2, v[i]), __fmul_rn(__fmul_rn(1.0f - b2, gv), gv));
  m[i] = mv;
  v[i] = vv;
  p[i] = __fmaf_rn(-lr_over_bc1, mv / __fmaf_rn(sqrtf(vv), inv_sqrt_bc2, eps), pv);
}

// max(a, b) of torch.maximum: a NaN in either operand is the result (a > b is false when b is NaN, a != a picks a NaN a)
__device__ __forceinline__ float max_nan(float a, float b) { return (a > b || a != a) ? a : b; }

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

// a rule = the step's scalars as they travel to the kernel, and the update they drive
struct AdamRule {
  float lr_over_bc1, inv_sqrt_bc2, b1, b2, eps, wd;
  __device__ __forceinline__ void update(float* p, float* m, float* v, long long i, float gv) const {
    adam_update(p, m, v, i, gv, lr_over_bc1, inv_sqrt_bc2, b1, b2, eps, wd);
  }
};
struct AdamaxRule {
  float lr_over_bc1, b1, b2, eps, wd;
  __device__ __forceinline__ void update(float* p, float* m, float* u, long long i, float gv) const {
    adamax_update(p, m, u, i, gv, lr_over_bc1, b1, b2, eps, wd);
  }
};

// kClip: the step on the clipped gradient g * coef, which is also written back (p.grad then holds what torch's clip_grad_norm_
// leaves); the product is rounded on its own (no contraction into the weight-decay fma), so coef == 1 gives the unclipped step's bits
template <typename Rule, bool kClip>
__global__ __launch_bounds__(256) void optim_update_kernel(AdamTable t, const float* __restrict__ coef_dev, Rule rule) {
  const int k = blockIdx.y;
  float* __restrict__ p = t.p[k];
  float* __restrict__ g = t.g[k];
  float* __restrict__ m = t.m[k];
  float* __restrict__ v = t.v[k];
  const long long n = t.n[k];
  const float coef = kClip ? coef_dev[0] : 1.0f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    float gs = g[i];
    if (kClip) {
      gs = __fmul_rn(gs, coef);
      g[i] = gs;
    }
    rule.update(p, m, v, i, gs);
  }
}

// ---- clipping by global norm -------------------------------------------------------------------------------------------------

constexpr int kNormThreads = 256;
constexpr int kNormMaxBlocks = 32;   // workgroups per tensor of the sum of squares (the updates: 1024): the finish adds the partials serially

static inline int norm_blocks(long long nmax) {
  const long long b = (nmax + kNormThreads - 1) / kNormThreads;
  return b < 1 ? 1 : (b > kNormMaxBlocks ? kNormMaxBlocks : (int)b);
}
// partials (one double each) of a whole call: per chunk of kAdamChunk tensors, tensors x workgroups -- a function of the sizes alone
static inline long long norm_partials(const long long* numel, int n_tensors) {
  long long total = 0;
  for (int o = 0; o < n_tensors; o += kAdamChunk) {
    const int m = n_tensors - o < kAdamChunk ? n_tensors - o : kAdamChunk;
    long long nmax = 0;
    for (int i = 0; i < m; ++i) nmax = numel[o + i] > nmax ? numel[o + i] : nmax;
    total += (long long)m * norm_blocks(nmax);
  }
  return total;
}

// sum of g*g in float64: a thread adds its elements in ascending order, then reduce.h's workgroup sum is the workgroup's partial.
// A tensor of 0 elements (or a workgroup past a short tensor) writes 0.
__global__ __launch_bounds__(kNormThreads) void grad_sqsum_kernel(GradTable t, double* __restrict__ partials) {
  __shared__ double red[kNormThreads / 64];
  const int k = blockIdx.y;
  const float* __restrict__ g = t.g[k];
  const long long n = t.n[k];
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * kNormThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kNormThreads) {
    const double v = (double)g[i];
    acc += v * v;
  }
  const double s = group_sum<kNormThreads>(acc, red);
  if (threadIdx.x == 0) partials[(long long)k * gridDim.x + blockIdx.x] = s;
}

// one workgroup: reduce.h's ordered sum of every partial, then the three floats
__global__ __launch_bounds__(kNormThreads) void grad_norm_finish_kernel(const double* __restrict__ partials, long long n_partials,
                                                                        float max_norm, float* __restrict__ out3) {
  __shared__ double stage[kSumMaxGroups];
  const double s = ordered_sum<kNormThreads>(partials, n_partials, stage);
  if (threadIdx.x == 0) {
    const float total = (float)sqrt(s);
    const float c = __fmul_rn(1.0f / (total + 1e-6f), max_norm);   // torch: max_norm / tensor == tensor.reciprocal() * max_norm
    const float coef = c > 1.0f ? 1.0f : c;                        // not fminf: a NaN stays a NaN (conv_common.h::relu_f)
    out3[0] = total;
    out3[1] = coef;
    out3[2] = __fmul_rn(total, coef);
  }
}

__global__ __launch_bounds__(256) void grad_scale_kernel(GradTable t, const float* __restrict__ coef_dev) {
  const int k = blockIdx.y;
  float* __restrict__ g = t.g[k];
  const long long n = t.n[k];
  const float coef = coef_dev[0];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) g[i] = __fmul_rn(g[i], coef);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------

// one chunk of a gradient table; a tensor of 0 elements may have a null pointer (torch hands out none for it)
static int fill_grad_table(GradTable& t, float* const* grads, const long long* numel, int o, int m, long long* nmax, const char* who) {
  memset(&t, 0, sizeof(t));
  *nmax = 0;
  for (int i = 0; i < m; ++i) {
    ODEHIP_REQUIRE(numel[o + i] >= 0 && (grads[o + i] || numel[o + i] == 0), "%s: tensor %d has a null pointer or a negative size", who,
                   o + i);
    t.g[i] = grads[o + i];
    t.n[i] = numel[o + i];
    *nmax = numel[o + i] > *nmax ? numel[o + i] : *nmax;
  }
  return ODEHIP_OK;
}

// one chunk of an optimizer table.  The unclipped steps take no null tensor pointer at all; the clipped ones (allow_empty) let a
// tensor of 0 elements have none, as fill_grad_table does.
static int fill_adam_table(AdamTable& t, float* const* params, float* const* grads, float* const* exp_avg, float* const* state2,
                           const long long* numel, int o, int m, bool allow_empty, long long* nmax, const char* who) {
  memset(&t, 0, sizeof(t));
  *nmax = 0;
  for (int i = 0; i < m; ++i) {
    ODEHIP_REQUIRE(numel[o + i] >= 0 && ((params[o + i] && grads[o + i] && exp_avg[o + i] && state2[o + i]) ||
                                          (allow_empty && numel[o + i] == 0)),
                   "%s: tensor %d has a null pointer", who, o + i);
    t.p[i] = params[o + i];
    t.g[i] = grads[o + i];
    t.m[i] = exp_avg[o + i];
    t.v[i] = state2[o + i];
    t.n[i] = numel[o + i];
    *nmax = numel[o + i] > *nmax ? numel[o + i] : *nmax;
  }
  return ODEHIP_OK;
}

// lr / (1 - b1^t), the step size of both rules
static inline float lr_over_bc1(float lr, float beta1, int step) { return (float)((double)lr / (1.0 - pow((double)beta1, step))); }

// all four steps: a launch per chunk of kAdamChunk tensors; coef_dev null = the unclipped step
template <typename Rule>
static int optim_launch(const char* who, float* const* params, float* const* grads, float* const* exp_avg, float* const* state2,
                        const long long* numel, int n_tensors, const Rule& rule, const float* coef_dev, void* stream) {
  for (int o = 0; o < n_tensors; o += kAdamChunk) {
    AdamTable t;
    const int m = n_tensors - o < kAdamChunk ? n_tensors - o : kAdamChunk;
    long long nmax;
    if (int rc = fill_adam_table(t, params, grads, exp_avg, state2, numel, o, m, coef_dev != nullptr, &nmax, who)) return rc;
    const dim3 grid(update_blocks(nmax), m);
    if (coef_dev) hipLaunchKernelGGL((optim_update_kernel<Rule, true>), grid, dim3(256), 0, (hipStream_t)stream, t, coef_dev, rule);
    else hipLaunchKernelGGL((optim_update_kernel<Rule, false>), grid, dim3(256), 0, (hipStream_t)stream, t, coef_dev, rule);
  }
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}

static int adam_launch(const char* who, float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                       const long long* numel, int n_tensors, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                       const float* coef_dev, void* stream) {
  ODEHIP_REQUIRE(step >= 1, "%s: step counts from 1 (got %d)", who, step);
  const AdamRule rule{lr_over_bc1(lr, beta1, step), (float)(1.0 / sqrt(1.0 - pow((double)beta2, step))), beta1, beta2, eps, weight_decay};
  return optim_launch(who, params, grads, exp_avg, exp_avg_sq, numel, n_tensors, rule, coef_dev, stream);
}

static int adamax_launch(const char* who, float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_inf,
                         const long long* numel, int n_tensors, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                         const float* coef_dev, void* stream) {
  ODEHIP_REQUIRE(step >= 1, "%s: step counts from 1 (got %d)", who, step);
  const AdamaxRule rule{lr_over_bc1(lr, beta1, step), beta1, beta2, eps, weight_decay};
  return optim_launch(who, params, grads, exp_avg, exp_inf, numel, n_tensors, rule, coef_dev, stream);
}

}  // namespace odehip

using namespace odehip;

extern "C" int odehip_adam_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                                const long long* numel, int n_tensors, float lr, float beta1, float beta2, float eps,
                                float weight_decay, int step, void* stream) {
  ODEHIP_REQUIRE(params && grads && exp_avg && exp_avg_sq && numel && n_tensors >= 0, "adam_step: null pointer");
  return adam_launch("adam_step", params, const_cast<float* const*>(grads), exp_avg, exp_avg_sq, numel, n_tensors, lr, beta1, beta2, eps,
                     weight_decay, step, nullptr, stream);
}

extern "C" int odehip_adam_step_clipped(float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                                        const long long* numel, int n_tensors, float lr, float beta1, float beta2, float eps,
                                        float weight_decay, int step, const float* coef_dev, void* stream) {
  ODEHIP_REQUIRE(params && grads && exp_avg && exp_avg_sq && numel && coef_dev && n_tensors >= 0, "adam_step_clipped: null pointer");
  return adam_launch("adam_step_clipped", params, grads, exp_avg, exp_avg_sq, numel, n_tensors, lr, beta1, beta2, eps, weight_decay, step,
                     coef_dev, stream);
}

extern "C" int odehip_adamax_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_inf,
                                  const long long* numel, int n_tensors, float lr, float beta1, float beta2, float eps,
                                  float weight_decay, int step, void* stream) {
  ODEHIP_REQUIRE(params && grads && exp_avg && exp_inf && numel && n_tensors >= 0, "adamax_step: null pointer");
  return adamax_launch("adamax_step", params, const_cast<float* const*>(grads), exp_avg, exp_inf, numel, n_tensors, lr, beta1, beta2, eps,
                       weight_decay, step, nullptr, stream);
}

extern "C" int odehip_adamax_step_clipped(float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_inf,
                                          const long long* numel, int n_tensors, float lr, float beta1, float beta2, float eps,
                                          float weight_decay, int step, const float* coef_dev, void* stream) {
  ODEHIP_REQUIRE(params && grads && exp_avg && exp_inf && numel && coef_dev && n_tensors >= 0, "adamax_step_clipped: null pointer");
  return adamax_launch("adamax_step_clipped", params, grads, exp_avg, exp_inf, numel, n_tensors, lr, beta1, beta2, eps, weight_decay,
                       step, coef_dev, stream);
}

extern "C" size_t odehip_grad_norm_workspace_bytes(int n_tensors, const long long* numel) {
  if (n_tensors <= 0 || !numel) return 0;
  return (size_t)norm_partials(numel, n_tensors) * sizeof(double);
}

extern "C" int odehip_grad_norm(const float* const* grads, const long long* numel, int n_tensors, float max_norm, void* partials_ws,
                                size_t ws_bytes, float* out3, void* stream) {
  ODEHIP_REQUIRE(grads && numel && out3 && n_tensors >= 0, "grad_norm: null pointer");
  ODEHIP_REQUIRE(max_norm >= 0.0f, "grad_norm: max_norm must be >= 0 (got %g)", (double)max_norm);   // false for a NaN too
  for (int i = 0; i < n_tensors; ++i) ODEHIP_REQUIRE(numel[i] >= 0, "grad_norm: tensor %d has a negative size", i);
  const long long n_partials = norm_partials(numel, n_tensors);
  ODEHIP_REQUIRE(n_partials == 0 || (partials_ws && ((uintptr_t)partials_ws & 7) == 0), "grad_norm: workspace is null or not 8-byte aligned");
  ODEHIP_REQUIRE(ws_bytes >= (size_t)n_partials * sizeof(double), "grad_norm: workspace of %zu bytes, %zu needed", ws_bytes,
                 (size_t)n_partials * sizeof(double));
  double* partials = (double*)partials_ws;
  long long base = 0;
  for (int o = 0; o < n_tensors; o += kAdamChunk) {
    GradTable t;
    const int m = n_tensors - o < kAdamChunk ? n_tensors - o : kAdamChunk;
    long long nmax;
    if (int rc = fill_grad_table(t, const_cast<float* const*>(grads), numel, o, m, &nmax, "grad_norm")) return rc;
    const int gx = norm_blocks(nmax);
    hipLaunchKernelGGL(grad_sqsum_kernel, dim3(gx, m), dim3(kNormThreads), 0, (hipStream_t)stream, t, partials + base);
    base += (long long)m * gx;
  }
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(kNormThreads), 0, (hipStream_t)stream, partials, n_partials, max_norm, out3);
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}

extern "C" int odehip_grad_scale(float* const* grads, const long long* numel, int n_tensors, const float* coef_dev, void* stream) {
  ODEHIP_REQUIRE(grads && numel && coef_dev && n_tensors >= 0, "grad_scale: null pointer");
  for (int o = 0; o < n_tensors; o += kAdamChunk) {
    GradTable t;
    const int m = n_tensors - o < kAdamChunk ? n_tensors - o : kAdamChunk;
    long long nmax;
    if (int rc = fill_grad_table(t, grads, numel, o, m, &nmax, "grad_scale")) return rc;
    hipLaunchKernelGGL(grad_scale_kernel, dim3(update_blocks(nmax), m), dim3(256), 0, (hipStream_t)stream, t, coef_dev);
  }
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}
