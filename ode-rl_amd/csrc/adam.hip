// adam.hip -- one-launch Adam step over every parameter tensor of the model (the optimizer step of
// train_test.py:24,205 `optim.Adam(model.parameters(), lr=opt.lr)`).  HBM-bound elementwise work: 4 reads + 3 writes of 4 B per
// parameter; the ODEConvGRU model has 1.04 M parameters in 40 tensors, so the point is ONE launch instead of a launch per
// tensor and op.  Arithmetic in torch.optim.Adam's order (amsgrad off):
//   g += wd*p;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g*g;  p -= (lr/(1-b1^t)) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
//
// Gradient clipping by global norm (train_test.py:187-195 `clip_grad_norm_(model.parameters(), opt.clip)`) rides on the same tensor
// tables.  A global norm needs every workgroup's partial sum before any parameter may move; here STREAM ORDER between plain launches
// is that barrier: grad_sqsum_kernel (one float64 partial per workgroup, plain stores) -> grad_norm_finish_kernel (one workgroup: the
// partials in index order, then total_norm, coef, clipped_norm as three floats on the device) -> adam_clip_kernel or grad_scale_kernel,
// which read coef from that buffer.  No cooperative launch, no flag one kernel waits on, no atomics, no host read: two runs are
// bitwise equal and nothing can hang.  coef is torch's expression in fp32, clamp(reciprocal(total_norm + 1e-6) * max_norm, max = 1):
// a NaN norm gives a NaN coefficient (error_if_nonfinite=False), an Inf norm a coefficient of 0.
#include <math.h>
#include <string.h>

#include "adam_table.h"
#include "odehip_internal.h"

namespace odehip {

__global__ __launch_bounds__(256) void adam_kernel(AdamTable t, float lr_over_bc1, float inv_sqrt_bc2, float b1, float b2, float eps,
                                                   float wd) {
  const int k = blockIdx.y;
  float* __restrict__ p = t.p[k];
  const float* __restrict__ g = t.g[k];
  float* __restrict__ m = t.m[k];
  float* __restrict__ v = t.v[k];
  const long long n = t.n[k];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float pv = p[i];
    const float gv = g[i] + wd * pv;
    const float mv = b1 * m[i] + (1.0f - b1) * gv;
    const float vv = b2 * v[i] + (1.0f - b2) * gv * gv;
    m[i] = mv;
    v[i] = vv;
    p[i] = pv - lr_over_bc1 * (mv / (sqrtf(vv) * inv_sqrt_bc2 + eps));
  }
}

// ---- clipping by global norm -------------------------------------------------------------------------------------------------

constexpr int kNormThreads = 256;
constexpr int kNormMaxBlocks = 32;   // workgroups per tensor of the sum of squares (Adam: 1024): the finish adds the partials serially
constexpr int kNormStage = 1024;     // partials the finish stages in LDS at a time
struct GradTable {
  float* g[kAdamChunk];
  long long n[kAdamChunk];
};

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

// sum of g*g in float64: a thread adds its elements in ascending order, a wave folds its 64 lanes by xor-shuffles, thread 0 adds the
// wave partials in wave order and stores the workgroup's partial.  A tensor of 0 elements (or a workgroup past a short tensor) writes 0.
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
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kNormThreads / 64; ++w) s += red[w];
    partials[(long long)k * gridDim.x + blockIdx.x] = s;
  }
}

// one workgroup: every partial in index order (staged through LDS kNormStage at a time, added by thread 0), then the three floats
__global__ __launch_bounds__(kNormThreads) void grad_norm_finish_kernel(const double* __restrict__ partials, long long n_partials,
                                                                        float max_norm, float* __restrict__ out3) {
  __shared__ double stage[kNormStage];
  double s = 0.0;
  for (long long base = 0; base < n_partials; base += kNormStage) {
    const int m = n_partials - base < kNormStage ? (int)(n_partials - base) : kNormStage;
    for (int i = threadIdx.x; i < m; i += kNormThreads) stage[i] = partials[base + i];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < m; ++i) s += stage[i];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float total = (float)sqrt(s);
    const float c = __fmul_rn(1.0f / (total + 1e-6f), max_norm);   // torch: max_norm / tensor == tensor.reciprocal() * max_norm
    const float coef = c > 1.0f ? 1.0f : c;                        // not fminf: a NaN stays a NaN (conv_common.h::relu_f)
    out3[0] = total;
    out3[1] = coef;
    out3[2] = __fmul_rn(total, coef);
  }
}

// adam_kernel on the clipped gradient g * coef, which is also written back (p.grad then holds what torch's clip_grad_norm_ leaves);
// the product is rounded on its own (no contraction into the weight-decay fma), so coef == 1 gives adam_kernel's bits
__global__ __launch_bounds__(256) void adam_clip_kernel(AdamTable t, const float* __restrict__ coef_dev, float lr_over_bc1,
                                                        float inv_sqrt_bc2, float b1, float b2, float eps, float wd) {
  const int k = blockIdx.y;
  float* __restrict__ p = t.p[k];
  float* __restrict__ g = const_cast<float*>(t.g[k]);
  float* __restrict__ m = t.m[k];
  float* __restrict__ v = t.v[k];
  const long long n = t.n[k];
  const float coef = coef_dev[0];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float pv = p[i];
    const float gs = __fmul_rn(g[i], coef);
    g[i] = gs;
    const float gv = gs + wd * pv;
    const float mv = b1 * m[i] + (1.0f - b1) * gv;
    const float vv = b2 * v[i] + (1.0f - b2) * gv * gv;
    m[i] = mv;
    v[i] = vv;
    p[i] = pv - lr_over_bc1 * (mv / (sqrtf(vv) * inv_sqrt_bc2 + eps));
  }
}

__global__ __launch_bounds__(256) void grad_scale_kernel(GradTable t, const float* __restrict__ coef_dev) {
  const int k = blockIdx.y;
  float* __restrict__ g = t.g[k];
  const long long n = t.n[k];
  const float coef = coef_dev[0];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) g[i] = __fmul_rn(g[i], coef);
}

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

}  // namespace odehip

using namespace odehip;

extern "C" int odehip_adam_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                                const long long* numel, int n_tensors, float lr, float beta1, float beta2, float eps,
                                float weight_decay, int step, void* stream) {
  ODEHIP_REQUIRE(params && grads && exp_avg && exp_avg_sq && numel && n_tensors >= 0, "adam_step: null pointer");
  ODEHIP_REQUIRE(step >= 1, "adam_step: step counts from 1 (got %d)", step);
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  const float lr_over_bc1 = (float)((double)lr / bc1), inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  for (int o = 0; o < n_tensors; o += kAdamChunk) {
    AdamTable t;
    memset(&t, 0, sizeof(t));
    const int m = n_tensors - o < kAdamChunk ? n_tensors - o : kAdamChunk;
    long long nmax = 0;
    for (int i = 0; i < m; ++i) {
      ODEHIP_REQUIRE(params[o + i] && grads[o + i] && exp_avg[o + i] && exp_avg_sq[o + i] && numel[o + i] >= 0,
                     "adam_step: tensor %d has a null pointer", o + i);
      t.p[i] = params[o + i];
      t.g[i] = grads[o + i];
      t.m[i] = exp_avg[o + i];
      t.v[i] = exp_avg_sq[o + i];
      t.n[i] = numel[o + i];
      nmax = numel[o + i] > nmax ? numel[o + i] : nmax;
    }
    int gx = (int)((nmax + 255) / 256);
    gx = gx < 1 ? 1 : (gx > 1024 ? 1024 : gx);
    hipLaunchKernelGGL(adam_kernel, dim3(gx, m), dim3(256), 0, (hipStream_t)stream, t, lr_over_bc1, inv_sqrt_bc2, beta1, beta2, eps,
                       weight_decay);
  }
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
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

extern "C" int odehip_adam_step_clipped(float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                                        const long long* numel, int n_tensors, float lr, float beta1, float beta2, float eps,
                                        float weight_decay, int step, const float* coef_dev, void* stream) {
  ODEHIP_REQUIRE(params && grads && exp_avg && exp_avg_sq && numel && coef_dev && n_tensors >= 0, "adam_step_clipped: null pointer");
  ODEHIP_REQUIRE(step >= 1, "adam_step_clipped: step counts from 1 (got %d)", step);
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  const float lr_over_bc1 = (float)((double)lr / bc1), inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  for (int o = 0; o < n_tensors; o += kAdamChunk) {
    AdamTable t;
    memset(&t, 0, sizeof(t));
    const int m = n_tensors - o < kAdamChunk ? n_tensors - o : kAdamChunk;
    long long nmax = 0;
    for (int i = 0; i < m; ++i) {
      ODEHIP_REQUIRE(numel[o + i] >= 0 && ((params[o + i] && grads[o + i] && exp_avg[o + i] && exp_avg_sq[o + i]) || numel[o + i] == 0),
                     "adam_step_clipped: tensor %d has a null pointer", o + i);
      t.p[i] = params[o + i];
      t.g[i] = grads[o + i];
      t.m[i] = exp_avg[o + i];
      t.v[i] = exp_avg_sq[o + i];
      t.n[i] = numel[o + i];
      nmax = numel[o + i] > nmax ? numel[o + i] : nmax;
    }
    hipLaunchKernelGGL(adam_clip_kernel, dim3(update_blocks(nmax), m), dim3(256), 0, (hipStream_t)stream, t, coef_dev, lr_over_bc1, inv_sqrt_bc2, beta1,
                       beta2, eps, weight_decay);
  }
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}
