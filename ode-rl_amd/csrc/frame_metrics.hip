// frame_metrics.hip -- per-frame evaluation metrics of a predicted sequence against the ground truth: squared error, MSE, PSNR and
// SSIM of every predicted frame, as the reference's test() computes them (train_test.py:104-117: F.mse_loss(...).item(), math.log10
// and utils.get_normalized_ssim, helpers/utils.py:254-271, per frame -- one host synchronisation and B scikit-image calls on the
// host per predicted frame).  Here: one launch over all (b, t) frames and a small one for the means over the batch, no host
// round trip.
//
// SSIM is the quantity defined in ssim_window.h (scikit-image's Gaussian-window structural_similarity) in float32, the mean of S over
// rows and columns 5 .. 58, averaged over the channels.
//
// Layout.  One 256-thread workgroup per frame (b, t); it walks the frame's channels.  Per channel both 64x64 planes go to LDS
// with 16-byte loads (2 x 16 KiB; the squared error is summed from the registers on the way).  Wave w owns the output rows
// 5 + {0..13, 14..27, 28..40, 41..53}[w], lane l the output column 5 + l (54 of 64 lanes; the others repeat column 58 and are
// left out of the sum).  A lane streams down its column: for every input row it forms the five row-filtered moments from 2 x 11 LDS
// words (consecutive lanes read consecutive words: conflict-free, 11 ordered fmas per moment) and folds them into ssim_window.h's
// pending column sums.  Nothing but the two input planes lives in LDS (33 KiB per workgroup: several workgroups per CU), at the
// price of row-filtering the ten halo rows of each wave twice (96 instead of 64 row passes per plane).  Every sum runs in a fixed
// order with explicit fmas; the frame's two sums are reduce.h's wave sum and then the four waves pairwise, (0 + 1) + (2 + 3): no
// atomics, two calls are bitwise equal.  NaN is not laundered: every pixel of a plane lies in some interior window, so one NaN reaches the
// frame's SSIM and squared error through plain arithmetic (the lane mask is a select on the lane index, never on the value).
#include <math.h>

#include "odehip_internal.h"
#include "reduce.h"
#include "ssim_window.h"

namespace odehip {

constexpr int kFrame = 64;                      // frames are 64 x 64 (the reference's `resolution` in every config)
constexpr int kPlane = kFrame * kFrame;
constexpr int kInterior = kFrame - 2 * kSsimRadius;   // 54 rows and columns of S enter the mean, from row and column kSsimCrop on

typedef float f32x4m __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void frame_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ truth, int channels,
                                                            SsimTaps<float> taps, float c1, float c2, float* __restrict__ sse,
                                                            float* __restrict__ ssim) {
#pragma clang fp contract(off)
  // x plane, y plane, then one row of reduction scratch
  __shared__ __attribute__((aligned(16))) float lds[2 * kPlane + kFrame];
  float* const sx = lds;
  float* const sy = lds + kPlane;
  float* const red = lds + 2 * kPlane;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_rows = wave < 2 ? 14 : 13;
  const int row0 = kSsimCrop + (wave < 2 ? 14 * wave : 28 + 13 * (wave - 2));   // first output row of this wave
  const bool counted = lane < kInterior;
  const int col = kSsimCrop + (counted ? lane : kInterior - 1);
  const long long frame = blockIdx.x;
  float sq = 0.0f, ss = 0.0f;
  for (int c = 0; c < channels; ++c) {
    const f32x4m* const px = (const f32x4m*)(pred + (frame * channels + c) * kPlane);
    const f32x4m* const py = (const f32x4m*)(truth + (frame * channels + c) * kPlane);
    if (c) __syncthreads();   // the previous channel's planes are still being read
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int q = tid + 256 * k;
      const f32x4m a = px[q], b = py[q];
      ((f32x4m*)sx)[q] = a;
      ((f32x4m*)sy)[q] = b;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = a[e] - b[e];
        sq = fmaf(d, d, sq);
      }
    }
    __syncthreads();
    float acc[kSsimTaps][5];
#pragma unroll
    for (int k = 0; k < kSsimTaps; ++k)
#pragma unroll
      for (int m = 0; m < 5; ++m) acc[k][m] = 0.0f;
    for (int i = 0; i < n_rows + 2 * kSsimRadius; ++i) {
      const int row = row0 - kSsimRadius + i;
      const float* const xr = sx + row * kFrame + col - kSsimRadius;
      const float* const yr = sy + row * kFrame + col - kSsimRadius;
      float h[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int d = 0; d < kSsimTaps; ++d) {
        const float w = taps.w[d < kSsimRadius ? kSsimRadius - d : d - kSsimRadius];
        const float xv = xr[d], yv = yr[d];
        h[0] = fmaf(w, xv, h[0]);
        h[1] = fmaf(w, yv, h[1]);
        h[2] = fmaf(w, xv * xv, h[2]);
        h[3] = fmaf(w, yv * yv, h[3]);
        h[4] = fmaf(w, xv * yv, h[4]);
      }
      ssim_fold_row(acc, h, taps);
      if (i >= 2 * kSsimRadius) {   // acc[0] is complete
        const float s = ssim_value(acc[0], c1, c2);
        ss += counted ? s : 0.0f;
      }
    }
  }
  sq = wave_sum(sq);
  ss = wave_sum(ss);
  if (lane == 0) {
    red[wave] = sq;
    red[4 + wave] = ss;
  }
  __syncthreads();
  if (tid == 0) {
    sse[frame] = (red[0] + red[1]) + (red[2] + red[3]);
    ssim[frame] = ((red[4] + red[5]) + (red[6] + red[7])) / (float)(kInterior * kInterior * channels);
  }
}

// means over the batch, one thread per predicted frame t, b in ascending order in fp64 (B terms each: nothing to parallelise)
__global__ __launch_bounds__(256) void frame_metrics_mean_kernel(const float* __restrict__ sse, const float* __restrict__ ssim, int batch,
                                                                 int n_frames, double elems, double range2, float* __restrict__ mse,
                                                                 float* __restrict__ psnr, float* __restrict__ ssim_t) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_frames) return;
  double e = 0.0, s = 0.0;
  for (int b = 0; b < batch; ++b) {
    e += (double)sse[(long long)b * n_frames + t];
    s += (double)ssim[(long long)b * n_frames + t];
  }
  const double m = e / elems;
  mse[t] = (float)m;
  psnr[t] = m == 0.0 ? INFINITY : (float)(10.0 * log10(range2 / m));   // a NaN mse takes the second branch and stays NaN
  ssim_t[t] = (float)(s / (double)batch);
}

}  // namespace odehip

using namespace odehip;

extern "C" int odehip_frame_metrics(const float* pred, const float* truth, int batch, int n_frames, int channels, int height, int width,
                                    float data_range, float* sse, float* ssim, float* mse, float* psnr, float* ssim_t, void* stream) {
  ODEHIP_REQUIRE(pred && truth && sse && ssim && mse && psnr && ssim_t, "frame_metrics: null pointer");
  ODEHIP_REQUIRE(batch >= 1 && n_frames >= 1, "frame_metrics: batch (%d) and n_frames (%d) must be at least 1", batch, n_frames);
  ODEHIP_REQUIRE((long long)batch * n_frames <= 0x7fffffffLL, "frame_metrics: batch * n_frames (%d x %d) exceeds the grid limit", batch, n_frames);
  ODEHIP_REQUIRE(data_range > 0.0f && isfinite(data_range), "frame_metrics: data_range must be positive and finite (got %g)", (double)data_range);
  ODEHIP_REQUIRE(height == kFrame && width == kFrame && (channels == 1 || channels == 3),
                 "frame_metrics: unsupported frame shape (channels %d, %d x %d): 1 or 3 channels of 64 x 64 only", channels, height, width);
  const double range = (double)data_range;
  hipLaunchKernelGGL(frame_metrics_kernel, dim3((unsigned)(batch * n_frames)), dim3(256), 0, (hipStream_t)stream, pred, truth, channels,
                     ssim_taps<float>(), ssim_constant<float>(0.01, range), ssim_constant<float>(0.03, range), sse, ssim);
  ODEHIP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(frame_metrics_mean_kernel, dim3((unsigned)((n_frames + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)sse,
                     (const float*)ssim, batch, n_frames, (double)batch * channels * kPlane, range * range, mse, psnr, ssim_t);
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}
