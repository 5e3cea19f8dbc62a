// ssim_window.h -- the SSIM window that frame_metrics.hip (T = float) and png_metrics.hip (T = double) share.  The quantity is
// scikit-image's structural_similarity(x, y, data_range=R, gaussian_weights=True, use_sample_covariance=False) of a 2-D image:
//   window   sigma = 1.5, truncate = 3.5 -> radius int(3.5 * 1.5 + 0.5) = 5: 11 taps w_k ~ exp(-k^2 / (2 sigma^2)), normalised to
//            sum 1, applied along rows and then along columns;
//   moments  ux, uy, uxx, uyy, uxy = filtered x, y, x^2, y^2, x y;  vx = uxx - ux^2, vy = uyy - uy^2, vxy = uxy - ux uy;
//   S        = (2 ux uy + C1) (2 vxy + C2) / ((ux^2 + uy^2 + C1) (vx + vy + C2)),  C1 = (0.01 R)^2, C2 = (0.03 R)^2;
//   result   mean of S over the rows and columns from 5 to size - 6 (scikit-image crops (win_size - 1) / 2 = 5 pixels).
// A window centred there reads pixels inside the image only, so the filter's border mode (scipy's 'reflect') never reaches the
// result and the outer ring of S is not computed at all.
//
// A lane streams down its column: per input row the kernel forms the five row-filtered moments h (its own row filter: that is what
// differs between the two files) and ssim_fold_row folds them into eleven pending column sums held in registers,
// acc[k] <- w[k] h + acc[k + 1]; acc[0] is then the finished window of the output row ten rows up, and ssim_value its S.  Every
// step is one correctly rounded operation in a fixed order (explicit fmas, contraction off).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace odehip {

constexpr int kSsimRadius = 5;
constexpr int kSsimTaps = 2 * kSsimRadius + 1;
constexpr int kSsimCrop = kSsimRadius;   // S enters the mean from this row and column on

template <typename T>
struct SsimTaps {
  T w[kSsimRadius + 1];   // w[|k|], k = -5 .. 5
};

// scipy.ndimage's _gaussian_kernel1d, evaluated in fp64 and rounded to T once
template <typename T>
static inline SsimTaps<T> ssim_taps() {
  const double sigma = 1.5;
  double phi[kSsimRadius + 1], sum = 0.0;
  for (int k = 0; k <= kSsimRadius; ++k) {
    phi[k] = exp(-0.5 / (sigma * sigma) * (double)(k * k));
    sum += k ? 2.0 * phi[k] : phi[k];
  }
  SsimTaps<T> taps;
  for (int k = 0; k <= kSsimRadius; ++k) taps.w[k] = (T)(phi[k] / sum);
  return taps;
}

// C1 (k = 0.01) and C2 (k = 0.03) of a data range, in fp64 and rounded to T once
template <typename T>
static inline T ssim_constant(double k, double range) {
  return (T)((k * range) * (k * range));
}

__device__ __forceinline__ float ssim_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double ssim_fma(double a, double b, double c) { return fma(a, b, c); }

// acc[k]: the column sum of output row (row - 10 + k) so far; input row `row`, whose moments are h, is its tap 10 - k
template <typename T>
__device__ __forceinline__ void ssim_fold_row(T (&acc)[kSsimTaps][5], const T (&h)[5], const SsimTaps<T> taps) {
#pragma unroll
  for (int k = 0; k < kSsimTaps; ++k) {
    const T w = taps.w[k < kSsimRadius ? kSsimRadius - k : k - kSsimRadius];
#pragma unroll
    for (int m = 0; m < 5; ++m) acc[k][m] = ssim_fma(w, h[m], k + 1 < kSsimTaps ? acc[k + 1][m] : (T)0);
  }
}

// S of a finished window a = {ux, uy, uxx, uyy, uxy}
template <typename T>
__device__ __forceinline__ T ssim_value(const T (&a)[5], T c1, T c2) {
#pragma clang fp contract(off)
  const T ux = a[0], uy = a[1], uxx = a[2], uyy = a[3], uxy = a[4];
  const T vx = uxx - ux * ux;
  const T vy = uyy - uy * uy;
  const T vxy = uxy - ux * uy;
  const T a1 = (T)2 * ux * uy + c1, a2 = (T)2 * vxy + c2;
  const T b1 = ux * ux + uy * uy + c1, b2 = vx + vy + c2;
  return (a1 * a2) / (b1 * b2);
}

}  // namespace odehip
