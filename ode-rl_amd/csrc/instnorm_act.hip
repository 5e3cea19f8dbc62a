// instnorm_act.hip -- InstanceNorm2d (no affine, biased variance, eps) + LeakyReLU(slope) of the discriminators' ConvNormAct blocks
// (models/gan.py) in one pass each way.  Planes are contiguous (planes, hw) = (N C, H W); slope 0 is the ReLU variant.
//
//   forward   xhat = (x - mean) rstd,  rstd = 1 / sqrt(var + eps),  y = xhat > 0 ? xhat : slope xhat;  mean, rstd (planes) are kept
//   backward  g' = xhat > 0 ? g : slope g,  grad_x = rstd (g' - mean(g') - xhat mean(g' xhat))      (xhat recomputed from x, mean, rstd)
//
// A plane of hw <= 1024 belongs to ONE wavefront and lives in its registers (up to 16 values per lane): one read and one write of the
// tensor forward, two reads and one write backward.  Larger planes belong to one workgroup that walks them three times (the second
// and third walk come from L2).  Nothing is shared between planes -- no atomics, no workspace -- so a NaN or Inf stays in its plane.
//
// Arithmetic.  The mean is the float64 sum of the plane divided by hw (a constant plane has exactly that constant as its mean, hence
// exactly zero output); the values are centred in float64 against it and rounded to fp32 once, so a large common offset costs no
// accuracy; the variance is the float64 sum of the squared centred values -- never E[x^2] - mean^2.  Sum order: a lane adds its
// values in slot order, then reduce.h's wave sum or (large planes) reduce.h's workgroup sum: a function of hw and of whether the
// tensors are 16-byte aligned, so two calls are bitwise equal.  The comparisons `xhat > 0` are false for NaN, as in torch's
// leaky_relu and leaky_relu_backward.
#include <math.h>
#include <stdint.h>

#include "odehip_internal.h"
#include "reduce.h"

namespace odehip {

typedef float f32x4n __attribute__((ext_vector_type(4)));

constexpr int kNormThreads = 256;
constexpr int kNormWaves = kNormThreads / 64;
constexpr int kNormWaveMax = 1024;   // largest plane one wavefront holds in registers

__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.0f ? v : slope * v; }

// ---- one wavefront per plane ----------------------------------------------------------------------------------------------------
// A lane holds NPL values.  VEC: slot group k (4 slots) is quad lane + 64 k of the plane (16-byte accesses; hw % 4 == 0, aligned
// base).  Scalar: slot k is element lane + 64 k.  Slots beyond the plane hold zeros and are never stored.

template <int NPL, bool VEC>
__device__ __forceinline__ void plane_load(const float* __restrict__ p, int hw, int lane, float (&v)[NPL], bool (&ok)[NPL]) {
  if constexpr (VEC) {
#pragma unroll
    for (int k = 0; k < NPL / 4; ++k) {
      const int q = lane + 64 * k;
      const bool in = 4 * q < hw;
      const f32x4n x = in ? ((const f32x4n*)p)[q] : f32x4n{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int i = 0; i < 4; ++i) v[4 * k + i] = x[i], ok[4 * k + i] = in;
    }
  } else {
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      const int e = lane + 64 * k;
      ok[k] = e < hw;
      v[k] = ok[k] ? p[e] : 0.0f;
    }
  }
}

template <int NPL, bool VEC>
__device__ __forceinline__ void plane_store(float* __restrict__ p, int hw, int lane, const float (&v)[NPL]) {
  if constexpr (VEC) {
#pragma unroll
    for (int k = 0; k < NPL / 4; ++k) {
      const int q = lane + 64 * k;
      if (4 * q < hw) ((f32x4n*)p)[q] = f32x4n{v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]};
    }
  } else {
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      const int e = lane + 64 * k;
      if (e < hw) p[e] = v[k];
    }
  }
}

template <int NPL, bool VEC>
__global__ __launch_bounds__(kNormThreads) void instnorm_lrelu_fwd_wave_kernel(const float* __restrict__ x, int planes, int hw, float eps,
                                                                               float slope, float* __restrict__ y, float* __restrict__ mean,
                                                                               float* __restrict__ rstd) {
  const int plane = blockIdx.x * kNormWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (plane >= planes) return;   // (whole waves leave: the shuffles below never straddle a plane)
  const long long base = (long long)plane * hw;
  float v[NPL];
  bool ok[NPL];
  plane_load<NPL, VEC>(x + base, hw, lane, v, ok);
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < NPL; ++k) s += (double)v[k];
  const double m = wave_sum(s) / (double)hw;
  double ss = 0.0;
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    v[k] = ok[k] ? (float)((double)v[k] - m) : 0.0f;
    ss += (double)v[k] * (double)v[k];
  }
  const float r = (float)(1.0 / sqrt(wave_sum(ss) / (double)hw + (double)eps));
#pragma unroll
  for (int k = 0; k < NPL; ++k) v[k] = lrelu(v[k] * r, slope);
  plane_store<NPL, VEC>(y + base, hw, lane, v);
  if (lane == 0) mean[plane] = (float)m, rstd[plane] = r;
}

template <int NPL, bool VEC>
__global__ __launch_bounds__(kNormThreads) void instnorm_lrelu_bwd_wave_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                                               const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                               int planes, int hw, float slope, float* __restrict__ gx) {
  const int plane = blockIdx.x * kNormWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (plane >= planes) return;
  const long long base = (long long)plane * hw;
  const float m = mean[plane], r = rstd[plane];
  float xh[NPL], g[NPL];
  bool ok[NPL];
  plane_load<NPL, VEC>(x + base, hw, lane, xh, ok);
  plane_load<NPL, VEC>(gy + base, hw, lane, g, ok);
  double s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    xh[k] = ok[k] ? (xh[k] - m) * r : 0.0f;
    g[k] = xh[k] > 0.0f ? g[k] : slope * g[k];
    s1 += (double)g[k];
    s2 += (double)g[k] * (double)xh[k];
  }
  const float m1 = (float)(wave_sum(s1) / (double)hw), m2 = (float)(wave_sum(s2) / (double)hw);
#pragma unroll
  for (int k = 0; k < NPL; ++k) g[k] = r * (g[k] - m1 - xh[k] * m2);
  plane_store<NPL, VEC>(gx + base, hw, lane, g);
}

// ---- one workgroup per plane (hw > 1024) ----------------------------------------------------------------------------------------

__global__ __launch_bounds__(kNormThreads) void instnorm_lrelu_fwd_group_kernel(const float* __restrict__ x, int hw, float eps, float slope,
                                                                                float* __restrict__ y, float* __restrict__ mean,
                                                                                float* __restrict__ rstd) {
  __shared__ double red[kNormWaves + 1];
  const long long base = (long long)blockIdx.x * hw;
  const float* const p = x + base;
  double s = 0.0;
  for (int e = threadIdx.x; e < hw; e += kNormThreads) s += (double)p[e];
  const double m = group_sum_all<kNormThreads>(s, red) / (double)hw;
  double ss = 0.0;
  for (int e = threadIdx.x; e < hw; e += kNormThreads) {
    const float d = (float)((double)p[e] - m);
    ss += (double)d * (double)d;
  }
  const float r = (float)(1.0 / sqrt(group_sum_all<kNormThreads>(ss, red) / (double)hw + (double)eps));
  for (int e = threadIdx.x; e < hw; e += kNormThreads) y[base + e] = lrelu((float)((double)p[e] - m) * r, slope);
  if (threadIdx.x == 0) mean[blockIdx.x] = (float)m, rstd[blockIdx.x] = r;
}

__global__ __launch_bounds__(kNormThreads) void instnorm_lrelu_bwd_group_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                                int hw, float slope, float* __restrict__ gx) {
  __shared__ double red[kNormWaves + 1];
  const long long base = (long long)blockIdx.x * hw;
  const float m = mean[blockIdx.x], r = rstd[blockIdx.x];
  double s1 = 0.0, s2 = 0.0;
  for (int e = threadIdx.x; e < hw; e += kNormThreads) {
    const float xh = (x[base + e] - m) * r, g = gy[base + e];
    const float gp = xh > 0.0f ? g : slope * g;
    s1 += (double)gp;
    s2 += (double)gp * (double)xh;
  }
  const float m1 = (float)(group_sum_all<kNormThreads>(s1, red) / (double)hw), m2 = (float)(group_sum_all<kNormThreads>(s2, red) / (double)hw);
  for (int e = threadIdx.x; e < hw; e += kNormThreads) {
    const float xh = (x[base + e] - m) * r, g = gy[base + e];
    gx[base + e] = r * ((xh > 0.0f ? g : slope * g) - m1 - xh * m2);
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------

// values per lane of the one-wave kernels for a plane of hw <= kNormWaveMax elements
static inline int norm_slots(int hw, bool vec) {
  const int need = (hw + 63) / 64;
  int npl = vec ? 4 : 1;
  while (npl < need) npl *= 2;
  return npl;
}

static int check_norm_shape(const char* who, int planes, int hw) {
  ODEHIP_REQUIRE(planes >= 1, "%s: planes (%d) must be at least 1", who, planes);
  ODEHIP_REQUIRE(hw >= 2, "%s: a plane of hw = %d elements has no variance (hw must be at least 2)", who, hw);
  return ODEHIP_OK;
}

#define NORM_DISPATCH(KERNEL, VEC, NPL, ...)                                                                                            \
  switch (NPL) {                                                                                                                        \
    case 1: hipLaunchKernelGGL((KERNEL<1, false>), grid, dim3(kNormThreads), 0, (hipStream_t)stream, __VA_ARGS__); break;                \
    case 2: hipLaunchKernelGGL((KERNEL<2, false>), grid, dim3(kNormThreads), 0, (hipStream_t)stream, __VA_ARGS__); break;                \
    case 4:                                                                                                                             \
      if (VEC) hipLaunchKernelGGL((KERNEL<4, true>), grid, dim3(kNormThreads), 0, (hipStream_t)stream, __VA_ARGS__);                     \
      else hipLaunchKernelGGL((KERNEL<4, false>), grid, dim3(kNormThreads), 0, (hipStream_t)stream, __VA_ARGS__);                        \
      break;                                                                                                                            \
    case 8:                                                                                                                             \
      if (VEC) hipLaunchKernelGGL((KERNEL<8, true>), grid, dim3(kNormThreads), 0, (hipStream_t)stream, __VA_ARGS__);                     \
      else hipLaunchKernelGGL((KERNEL<8, false>), grid, dim3(kNormThreads), 0, (hipStream_t)stream, __VA_ARGS__);                        \
      break;                                                                                                                            \
    default:                                                                                                                            \
      if (VEC) hipLaunchKernelGGL((KERNEL<16, true>), grid, dim3(kNormThreads), 0, (hipStream_t)stream, __VA_ARGS__);                    \
      else hipLaunchKernelGGL((KERNEL<16, false>), grid, dim3(kNormThreads), 0, (hipStream_t)stream, __VA_ARGS__);                       \
      break;                                                                                                                            \
  }

}  // namespace odehip

using namespace odehip;

extern "C" int odehip_instnorm_lrelu_forward(const float* x, int planes, int hw, float eps, float slope, float* y, float* mean, float* rstd,
                                             void* stream) {
  ODEHIP_REQUIRE(x && y && mean && rstd, "instnorm_lrelu_forward: null pointer");
  if (int rc = check_norm_shape("instnorm_lrelu_forward", planes, hw)) return rc;
  ODEHIP_REQUIRE(eps >= 0.0f, "instnorm_lrelu_forward: eps (%g) must not be negative", (double)eps);
  ODEHIP_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)mean | (uintptr_t)rstd) & 3) == 0, "instnorm_lrelu_forward: misaligned pointer (4 bytes)");
  if (hw > kNormWaveMax) {
    hipLaunchKernelGGL(instnorm_lrelu_fwd_group_kernel, dim3((unsigned)planes), dim3(kNormThreads), 0, (hipStream_t)stream, x, hw, eps, slope, y,
                       mean, rstd);
  } else {
    const bool vec = hw % 4 == 0 && hw > 64 && aligned16(x) && aligned16(y);
    const int npl = norm_slots(hw, vec);
    const dim3 grid((unsigned)((planes + kNormWaves - 1) / kNormWaves));
    NORM_DISPATCH(instnorm_lrelu_fwd_wave_kernel, vec, npl, x, planes, hw, eps, slope, y, mean, rstd)
  }
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}

extern "C" int odehip_instnorm_lrelu_backward(const float* grad_y, const float* x, const float* mean, const float* rstd, int planes, int hw,
                                              float slope, float* grad_x, void* stream) {
  ODEHIP_REQUIRE(grad_y && x && mean && rstd && grad_x, "instnorm_lrelu_backward: null pointer");
  if (int rc = check_norm_shape("instnorm_lrelu_backward", planes, hw)) return rc;
  ODEHIP_REQUIRE((((uintptr_t)grad_y | (uintptr_t)x | (uintptr_t)mean | (uintptr_t)rstd | (uintptr_t)grad_x) & 3) == 0,
                 "instnorm_lrelu_backward: misaligned pointer (4 bytes)");
  if (hw > kNormWaveMax) {
    hipLaunchKernelGGL(instnorm_lrelu_bwd_group_kernel, dim3((unsigned)planes), dim3(kNormThreads), 0, (hipStream_t)stream, grad_y, x, mean, rstd,
                       hw, slope, grad_x);
  } else {
    const bool vec = hw % 4 == 0 && hw > 64 && aligned16(grad_y) && aligned16(x) && aligned16(grad_x);
    const int npl = norm_slots(hw, vec);
    const dim3 grid((unsigned)((planes + kNormWaves - 1) / kNormWaves));
    NORM_DISPATCH(instnorm_lrelu_bwd_wave_kernel, vec, npl, grad_y, x, mean, rstd, planes, hw, slope, grad_x)
  }
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}
