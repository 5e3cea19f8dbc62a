// png_metrics.hip -- upstream Vid-ODE's evaluation protocol (Vid-ODE/tester.py:49-78, visualize.save_test_images, evaluate.Evaluation)
// with nothing leaving the device.  Upstream de-normalises every predicted and true frame, writes it as an 8-bit PNG (torchvision's
// save_image), reads it back, converts it to 'L' luma with PIL, takes scikit-image's Gaussian SSIM at data_range 255 on the luma and
// the MSE of the 8-bit RGB image / 255 -- 2 B T files and one scikit-image call per file and batch.  Here: one launch over all (b, t)
// images, and a small second one that adds the batch to an accumulator over the test set.
//
// Per pixel, in float32 with one correctly rounded operation per step (fp contract off), upstream's chain:
//   denorm      v = (x + 1) / 2, then min(max(v, 0), 1)                                   (utils.denorm; only with `denorm`)
//   save_image  v * 255, then + 0.5, then clamp to [0, 255], then truncate to a byte      (mul(255).add_(0.5).clamp_(0, 255).to(uint8))
//   C == 1      the plane is replicated into R, G and B                                    (save_image writes RGB)
//   luma        L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 in integers               (PIL's convert('L'); R = G = B gives L = R)
// A PNG round trip is lossless, so these bytes are the file contents.
//   sse   = sum over the 3 S S RGB bytes of (byte_pred - byte_truth)^2: an exact integer (at most 3 * 128 * 128 * 255^2 = 3.2e9:
//           32-bit partials per wave, summed in 64 bits);  mse = sse / (255^2 * 3 S S) in float64.
//   ssim  = the quantity defined in ssim_window.h (sigma 1.5, 11 taps, C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2, mean over rows and
//           columns 5 .. S-6) on the two luma planes, every moment in float64: the bytes, their squares and products are
//           exact integers, so only the weighted sums round.  (float32 moments at data_range 255 lose the variance uxx - ux^2 to
//           cancellation.)
//
// Layout.  One 256-thread workgroup per image.  Pass 1: a thread takes four pixels of a row at a time (16-byte loads per channel),
// quantises both frames, adds the squared byte differences, writes the twelve RGB bytes of each frame (three 4-byte stores, optional)
// and the four luma bytes of each frame to LDS -- the luma stays in LDS as BYTES (2 S S bytes: 32 KiB at S = 128) and is converted on
// read.  Pass 2: the interior columns go to lanes (S = 128: two groups of 64 lanes, 118 columns), the interior rows to the remaining
// waves in strips (S = 32, 64: four strips; S = 128: two).  A lane streams down its column: per input row the five row-filtered
// moments -- mirrored taps are paired in integers first (x[-k] + x[k], x[-k]^2 + x[k]^2, ...: exact), so a row costs 6 instead of 11
// fmas per moment -- folded into ssim_window.h's pending column sums.  A strip row-filters its ten halo rows again.  Four
// consecutive lanes read the four bytes of one LDS word (a broadcast, no bank conflict).  Every sum runs in a fixed order; the
// image's sums are reduce.h's wave sum and then the four waves pairwise, (0 + 1) + (2 + 3): no atomics, two calls are bitwise equal.
//
// NaN is not laundered: a conversion to a byte would hide it, so it is detected by a comparison on the float (x != x) in either
// frame; the image's ssim and mse are then NaN, its sse -1, the NaN pixel's byte 0; no other image is touched.
#include <math.h>

#include "odehip_internal.h"
#include "reduce.h"
#include "ssim_window.h"

namespace odehip {

constexpr int kPngScratch = 256;           // bytes of reduction scratch in FRONT of the planes (the row above the first plane stays inside the allocation)

typedef float png_f32x4 __attribute__((ext_vector_type(4)));

// utils.denorm and torchvision's save_image on one value; a NaN gives byte 0 (the caller flags it)
__device__ __forceinline__ unsigned png_quantise(float x, bool denorm) {
#pragma clang fp contract(off)
  float v = x;
  if (denorm) {
    v = (v + 1.0f) / 2.0f;
    v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
  }
  v = v * 255.0f;
  v = v + 0.5f;
  v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
  return x != x ? 0u : (unsigned)(int)v;
}

// PIL's convert('L') (ImagingConvert rgb2l): ITU-R 601-2 in 16-bit fixed point, rounded
__device__ __forceinline__ unsigned png_luma(unsigned r, unsigned g, unsigned b) {
  return (19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16;
}

// four pixels of one frame: C planes -> RGB bytes rgb[c][e]; returns whether one of the values was NaN
template <int S, int C>
__device__ __forceinline__ bool png_quad(const float* __restrict__ frame, int q, bool denorm, unsigned (&rgb)[3][4]) {
  bool bad = false;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const png_f32x4 a = ((const png_f32x4*)(frame + c * S * S))[q];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      bad |= a[e] != a[e];
      rgb[c][e] = png_quantise(a[e], denorm);
    }
  }
  if (C == 1) {
#pragma unroll
    for (int e = 0; e < 4; ++e) rgb[1][e] = rgb[2][e] = rgb[0][e];
  }
  return bad;
}

// the twelve RGB bytes of four pixels (pixel-major: PNG order) as three 4-byte stores, and their four luma bytes as one word
__device__ __forceinline__ unsigned png_emit(const unsigned (&rgb)[3][4], unsigned* __restrict__ bytes_out) {
  if (bytes_out) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      unsigned word = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int n = 4 * j + k;   // byte n of the twelve: pixel n / 3, channel n % 3
        word |= rgb[n % 3][n / 3] << (8 * k);
      }
      bytes_out[j] = word;
    }
  }
  unsigned l = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) l |= png_luma(rgb[0][e], rgb[1][e], rgb[2][e]) << (8 * e);
  return l;
}

template <int S, int C>
__global__ __launch_bounds__(256) void png_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ truth, int denorm,
                                                          SsimTaps<double> taps, double c1, double c2, long long* __restrict__ sse,
                                                          double* __restrict__ mse, double* __restrict__ ssim,
                                                          unsigned char* __restrict__ pred_bytes, unsigned char* __restrict__ truth_bytes) {
#pragma clang fp contract(off)
  constexpr int kPix = S * S;
  constexpr int kInterior = S - 2 * kSsimRadius;            // rows and columns of S that enter the mean
  constexpr int kColGroups = (kInterior + 63) / 64;         // 64 interior columns per wave
  constexpr int kStrips = 4 / kColGroups;                   // the other waves split the interior rows
  static_assert(kColGroups * kStrips == 4 && kPix % 1024 == 0, "four waves, whole quads per thread");
  // reduction scratch, then the luma plane of pred, then the one of truth
  __shared__ __attribute__((aligned(16))) unsigned char lds[kPngScratch + 2 * kPix];
  double* const red_ss = (double*)lds;                      // [4]
  unsigned* const red_sq = (unsigned*)(lds + 32);           // [4]
  unsigned* const red_bad = (unsigned*)(lds + 48);          // [4]
  unsigned char* const sx = lds + kPngScratch;
  unsigned char* const sy = sx + kPix;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long image = blockIdx.x;
  const float* const px = pred + image * (C * kPix);
  const float* const py = truth + image * (C * kPix);
  unsigned* const bx = pred_bytes ? (unsigned*)(pred_bytes + image * (3 * kPix)) : nullptr;
  unsigned* const by = truth_bytes ? (unsigned*)(truth_bytes + image * (3 * kPix)) : nullptr;

  // ---- pass 1: bytes, squared byte differences, luma planes
  unsigned sq = 0;
  bool bad = false;
#pragma unroll 2   // (two quads of loads in flight; unrolled further the loads of a 128 x 128 x 3 image crowd out the column sums of pass 2)
  for (int k = 0; k < kPix / 1024; ++k) {
    const int q = tid + 256 * k;
    unsigned a[3][4], b[3][4];
    bad |= png_quad<S, C>(px, q, denorm != 0, a);
    bad |= png_quad<S, C>(py, q, denorm != 0, b);
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int d = (int)a[c][e] - (int)b[c][e];
        sq += (unsigned)(d * d);
      }
    ((unsigned*)sx)[q] = png_emit(a, bx ? bx + 3 * q : nullptr);
    ((unsigned*)sy)[q] = png_emit(b, by ? by + 3 * q : nullptr);
  }
  sq = wave_sum(sq);                                         // at most 3 * 128 * 128 * 255^2 / 4 per wave: fits 32 bits
  const bool wave_bad = __any(bad);
  if (lane == 0) {
    red_sq[wave] = sq;
    red_bad[wave] = wave_bad ? 1u : 0u;
  }
  __syncthreads();
  if (red_bad[0] | red_bad[1] | red_bad[2] | red_bad[3]) {   // the same for every thread of the workgroup
    if (tid == 0) {
      sse[image] = -1;
      mse[image] = (double)NAN;
      ssim[image] = (double)NAN;
    }
    return;
  }

  // ---- pass 2: SSIM of the luma planes, float64
  const int group = wave % kColGroups, strip = wave / kColGroups;
  const int n_rows = kInterior / kStrips + (strip < kInterior % kStrips ? 1 : 0);
  const int first = strip * (kInterior / kStrips) + (strip < kInterior % kStrips ? strip : kInterior % kStrips);
  const int row0 = kSsimCrop + first;                        // first output row of this wave
  const int j = 64 * group + lane;
  const bool counted = j < kInterior;
  const int col = kSsimCrop + (counted ? j : kInterior - 1);
  double acc[kSsimTaps][5];
#pragma unroll
  for (int k = 0; k < kSsimTaps; ++k)
#pragma unroll
    for (int m = 0; m < 5; ++m) acc[k][m] = 0.0;
  double ss = 0.0;
  for (int i = 0; i < n_rows + 2 * kSsimRadius; ++i) {
    const int row = row0 - kSsimRadius + i;
    const unsigned char* const xr = sx + row * S + col - kSsimRadius;
    const unsigned char* const yr = sy + row * S + col - kSsimRadius;
    unsigned xv[kSsimTaps], yv[kSsimTaps];
#pragma unroll
    for (int d = 0; d < kSsimTaps; ++d) {
      xv[d] = xr[d];
      yv[d] = yr[d];
    }
    const unsigned xc = xv[kSsimRadius], yc = yv[kSsimRadius];
    double h[5] = {taps.w[0] * (double)xc, taps.w[0] * (double)yc, taps.w[0] * (double)(xc * xc), taps.w[0] * (double)(yc * yc),
                   taps.w[0] * (double)(xc * yc)};
#pragma unroll
    for (int k = kSsimRadius; k >= 1; --k) {                 // the two taps at distance k share a weight: paired in integers, exactly
      const unsigned xa = xv[kSsimRadius - k], xb = xv[kSsimRadius + k], ya = yv[kSsimRadius - k], yb = yv[kSsimRadius + k];
      h[0] = fma(taps.w[k], (double)(xa + xb), h[0]);
      h[1] = fma(taps.w[k], (double)(ya + yb), h[1]);
      h[2] = fma(taps.w[k], (double)(xa * xa + xb * xb), h[2]);
      h[3] = fma(taps.w[k], (double)(ya * ya + yb * yb), h[3]);
      h[4] = fma(taps.w[k], (double)(xa * ya + xb * yb), h[4]);
    }
    // ssim_window.h's ssim_fold_row, written out: through the helper the compiler lays this float64 loop out differently, which
    // costs 1 - 2 % at 64 images of 3 channels.  acc[k]: the column sum of output row (row - 10 + k) so far; this input row is its tap 10 - k
#pragma unroll
    for (int k = 0; k < kSsimTaps; ++k) {
      const double w = taps.w[k < kSsimRadius ? kSsimRadius - k : k - kSsimRadius];
#pragma unroll
      for (int m = 0; m < 5; ++m) acc[k][m] = fma(w, h[m], k + 1 < kSsimTaps ? acc[k + 1][m] : 0.0);
    }
    if (i >= 2 * kSsimRadius) {   // acc[0] is complete
      const double s = ssim_value(acc[0], c1, c2);
      ss += counted ? s : 0.0;
    }
  }
  ss = wave_sum(ss);
  if (lane == 0) red_ss[wave] = ss;
  __syncthreads();
  if (tid == 0) {
    const long long total = ((long long)red_sq[0] + (long long)red_sq[1]) + ((long long)red_sq[2] + (long long)red_sq[3]);
    sse[image] = total;
    mse[image] = (double)total / (255.0 * 255.0 * 3.0 * (double)kPix);
    ssim[image] = ((red_ss[0] + red_ss[1]) + (red_ss[2] + red_ss[3])) / (double)(kInterior * kInterior);
  }
}

// the accumulator over a test set: {sum of ssim, sum of mse} in float64 and the image count.  One wave; the n values are loaded 64
// at a time and every lane adds them in ascending order (a broadcast per value), continuing the running sums of the earlier calls,
// so the sums are those of ONE ascending pass over all images however the set was split into batches.
__global__ __launch_bounds__(64) void png_metrics_accumulate_kernel(const double* __restrict__ ssim, const double* __restrict__ mse, long long n,
                                                                    double* __restrict__ sums, long long* __restrict__ count) {
  const int lane = threadIdx.x;
  double s = sums[0], m = sums[1];
  for (long long base = 0; base < n; base += 64) {
    const bool have = base + lane < n;
    const double sv = have ? ssim[base + lane] : 0.0, mv = have ? mse[base + lane] : 0.0;
    const int len = n - base < 64 ? (int)(n - base) : 64;
    for (int k = 0; k < len; ++k) {
      s += __shfl(sv, k, 64);
      m += __shfl(mv, k, 64);
    }
  }
  if (lane == 0) {
    const long long seen = *count;
    sums[0] = s;
    sums[1] = m;
    *count = seen + n;
  }
}

template <int S>
static int png_launch(const float* pred, const float* truth, int images, int channels, int denorm, const SsimTaps<double>& taps, double c1, double c2,
                      long long* sse, double* mse, double* ssim, unsigned char* pred_bytes, unsigned char* truth_bytes, hipStream_t stream) {
  if (channels == 1)
    hipLaunchKernelGGL((png_metrics_kernel<S, 1>), dim3((unsigned)images), dim3(256), 0, stream, pred, truth, denorm, taps, c1, c2, sse, mse, ssim,
                       pred_bytes, truth_bytes);
  else
    hipLaunchKernelGGL((png_metrics_kernel<S, 3>), dim3((unsigned)images), dim3(256), 0, stream, pred, truth, denorm, taps, c1, c2, sse, mse, ssim,
                       pred_bytes, truth_bytes);
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}

}  // namespace odehip

using namespace odehip;

extern "C" int odehip_png_metrics(const float* pred, const float* truth, int batch, int n_frames, int channels, int size, int denorm,
                                  long long* sse, double* mse, double* ssim, unsigned char* pred_bytes, unsigned char* truth_bytes,
                                  void* accum, void* stream) {
  ODEHIP_REQUIRE(pred && truth && sse && mse && ssim, "png_metrics: null pointer");
  ODEHIP_REQUIRE(batch >= 1 && n_frames >= 1, "png_metrics: batch (%d) and n_frames (%d) must be at least 1", batch, n_frames);
  ODEHIP_REQUIRE((long long)batch * n_frames <= 0x7fffffffLL, "png_metrics: batch * n_frames (%d x %d) exceeds the grid limit", batch, n_frames);
  ODEHIP_REQUIRE((channels == 1 || channels == 3) && (size == 32 || size == 64 || size == 128),
                 "png_metrics: unsupported frame shape (channels %d, %d x %d): 1 or 3 channels of 32 x 32, 64 x 64 or 128 x 128 only", channels, size,
                 size);
  ODEHIP_REQUIRE((pred_bytes != nullptr) == (truth_bytes != nullptr), "png_metrics: pred_bytes and truth_bytes go together (both or neither)");
  ODEHIP_REQUIRE(((uintptr_t)pred | (uintptr_t)truth) % 16 == 0, "png_metrics: pred and truth must be 16-byte aligned");
  ODEHIP_REQUIRE(((uintptr_t)sse | (uintptr_t)mse | (uintptr_t)ssim | (uintptr_t)accum) % 8 == 0 && ((uintptr_t)pred_bytes | (uintptr_t)truth_bytes) % 4 == 0,
                 "png_metrics: sse, mse, ssim and accum must be 8-byte aligned, the byte outputs 4-byte aligned");
  const SsimTaps<double> taps = ssim_taps<double>();
  const double c1 = ssim_constant<double>(0.01, 255.0), c2 = ssim_constant<double>(0.03, 255.0);
  const int images = batch * n_frames;
  int rc;
  if (size == 32)
    rc = png_launch<32>(pred, truth, images, channels, denorm, taps, c1, c2, sse, mse, ssim, pred_bytes, truth_bytes, (hipStream_t)stream);
  else if (size == 64)
    rc = png_launch<64>(pred, truth, images, channels, denorm, taps, c1, c2, sse, mse, ssim, pred_bytes, truth_bytes, (hipStream_t)stream);
  else
    rc = png_launch<128>(pred, truth, images, channels, denorm, taps, c1, c2, sse, mse, ssim, pred_bytes, truth_bytes, (hipStream_t)stream);
  if (rc != ODEHIP_OK) return rc;
  if (accum) {
    hipLaunchKernelGGL(png_metrics_accumulate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)ssim, (const double*)mse,
                       (long long)images, (double*)accum, (long long*)accum + 2);
    ODEHIP_CHECK_HIP(hipGetLastError());
  }
  return ODEHIP_OK;
}
