// gan.hip -- what surrounds the discriminators' convolutions in the adversarial step (models/gan.py): the sequences the sequence
// discriminator judges, forward and backward, and the LSGAN terms.  Enqueue-only, no host round trip, no atomics.
//
// Sequence assembly.  input_real (b, t_in, P) and frames (b, t, P), P = c h w, give out (t b, L, P): row i b + n holds L frames.
//   extrapolation  L = max(t, t_in + 1);  keep_i = max(0, t_in - i) observed frames, l_i = keep_i + i + 1, pad_i = L - l_i:
//                  row = [zeros x pad_i] ++ input_real[n, i:] ++ frames[n, :i+1]
//   interpolation  t_in == t, L = t:  row = input_real[n] with frame i replaced by frames[n, i]
// Forward is a gather over the output, backward a gather over grad_frames: grad_frames[n, j] is the sum of its copies in the rows
// i = j .. t-1 (one copy per row; interpolation: row j alone), added in ascending i in fp32.  input_real gets no gradient.
//
// LSGAN.  out = mean (pred - target)^2: every difference, square and sum in float64 from the fp32 input, rounded to fp32 once.
// Sum order: a thread adds its elements in ascending order, then reduce.h's workgroup sum, and the second launch is reduce.h's
// ordered sum of the workgroup partials -- a function of n alone, so two calls are bitwise equal.  Forward: partials, then a
// one-workgroup final (as frame_loss.hip); backward: one launch,
// grad = fl32(grad_out 2 (pred - target) / n) with the quotient taken in float64.
#include <math.h>
#include <stdint.h>

#include "odehip_internal.h"
#include "reduce.h"

namespace odehip {

typedef float f32x4g __attribute__((ext_vector_type(4)));

constexpr int kGanThreads = 256;
constexpr long long kGanMaxBlocks = 8192;

struct SeqArgs {
  int b, t_in, t, L, interp;
  long long fe;   // elements of a frame in units of T (P or P / 4)
};

// where slot s of row i (sample n) comes from: 0 = zeros, 1 = input_real frame *f, 2 = frames frame *f
__device__ __forceinline__ int seq_source(const SeqArgs& a, int i, int s, int* f) {
  if (a.interp) {
    *f = s;
    return s == i ? 2 : 1;
  }
  const int keep = a.t_in > i ? a.t_in - i : 0;
  const int k = s - (a.L - (keep + i + 1));
  if (k < 0) return 0;
  if (k < keep) {
    *f = i + k;
    return 1;
  }
  *f = k - keep;
  return 2;
}

template <typename T>
__global__ __launch_bounds__(kGanThreads) void seq_assemble_kernel(const T* __restrict__ input_real, const T* __restrict__ frames, SeqArgs a,
                                                                   long long total, T* __restrict__ out) {
  const long long stride = (long long)gridDim.x * kGanThreads;
  for (long long idx = (long long)blockIdx.x * kGanThreads + threadIdx.x; idx < total; idx += stride) {
    const long long item = idx / a.fe, off = idx - item * a.fe;
    const int row = (int)(item / a.L), s = (int)(item - (long long)row * a.L);
    const int i = row / a.b, n = row - i * a.b;
    int f = 0;
    const int src = seq_source(a, i, s, &f);
    T v = T{};
    if (src == 1) v = input_real[((long long)n * a.t_in + f) * a.fe + off];
    else if (src == 2) v = frames[((long long)n * a.t + f) * a.fe + off];
    out[idx] = v;
  }
}

template <typename T>
__global__ __launch_bounds__(kGanThreads) void seq_assemble_backward_kernel(const T* __restrict__ grad_out, SeqArgs a, long long total,
                                                                            T* __restrict__ grad_frames) {
#pragma clang fp contract(off)
  const long long stride = (long long)gridDim.x * kGanThreads;
  for (long long idx = (long long)blockIdx.x * kGanThreads + threadIdx.x; idx < total; idx += stride) {
    const long long item = idx / a.fe, off = idx - item * a.fe;
    const int n = (int)(item / a.t), j = (int)(item - (long long)n * a.t);
    T acc = T{};
    const int last = a.interp ? j : a.t - 1;
    for (int i = j; i <= last; ++i) {   // frames[n, j] sits in row i at slot pad_i + keep_i + j = L - (i + 1) + j (interpolation: slot j)
      const int s = a.interp ? j : a.L - (i + 1) + j;
      const T g = grad_out[(((long long)i * a.b + n) * a.L + s) * a.fe + off];
      acc = i == j ? g : acc + g;
    }
    grad_frames[idx] = acc;
  }
}

// ---- LSGAN ----------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kGanThreads) void lsgan_partial_kernel(const float* __restrict__ pred, long long n, double target,
                                                                    double* __restrict__ partials) {
  __shared__ double red[kGanThreads / 64];
  const long long stride = (long long)gridDim.x * kGanThreads;
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * kGanThreads + threadIdx.x; i < n; i += stride) {
    const double d = (double)pred[i] - target;
    acc += d * d;
  }
  const double t = group_sum<kGanThreads>(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

__global__ __launch_bounds__(kGanThreads) void lsgan_final_kernel(const double* __restrict__ partials, int n_partials, double n_elems,
                                                                  float* __restrict__ out) {
  __shared__ double stage[kSumMaxGroups];
  const double s = ordered_sum<kGanThreads>(partials, n_partials, stage);
  if (threadIdx.x == 0) out[0] = (float)(s / n_elems);
}

__global__ __launch_bounds__(kGanThreads) void lsgan_backward_kernel(const float* __restrict__ grad_out, const float* __restrict__ pred,
                                                                     long long n, double target, float* __restrict__ grad) {
  const double scale = 2.0 * (double)grad_out[0] / (double)n;
  const long long stride = (long long)gridDim.x * kGanThreads;
  for (long long i = (long long)blockIdx.x * kGanThreads + threadIdx.x; i < n; i += stride) grad[i] = (float)(scale * ((double)pred[i] - target));
}

// ---- host side ------------------------------------------------------------------------------------------------------------------

static inline unsigned gan_blocks(long long total) {
  const long long g = (total + kGanThreads - 1) / kGanThreads;
  return (unsigned)(g > kGanMaxBlocks ? kGanMaxBlocks : g);
}

static int fill_seq_args(const char* who, SeqArgs* a, int batch, int t_in, int t, long long frame_elems, int interp) {
  ODEHIP_REQUIRE(batch >= 1 && t_in >= 1 && t >= 1 && frame_elems >= 1,
                 "%s: batch (%d), t_in (%d), t (%d) and frame_elems (%lld) must be at least 1", who, batch, t_in, t, frame_elems);
  ODEHIP_REQUIRE(interp == 0 || interp == 1, "%s: interp must be 0 (extrapolation) or 1 (interpolation), got %d", who, interp);
  ODEHIP_REQUIRE(!interp || t_in == t, "%s: the interpolation form needs t_in == t, got %d and %d", who, t_in, t);
  const int L = interp ? t : (t > t_in + 1 ? t : t_in + 1);
  ODEHIP_REQUIRE((long long)t * batch <= 0x7fffffffLL && (double)t * batch * L * (double)frame_elems < 9.0e18,
                 "%s: t * batch * L * frame_elems (%d x %d x %d x %lld) is too large", who, t, batch, L, frame_elems);
  a->b = batch, a->t_in = t_in, a->t = t, a->L = L, a->interp = interp, a->fe = frame_elems;
  return ODEHIP_OK;
}

}  // namespace odehip

using namespace odehip;

extern "C" int odehip_gan_seq_assemble(const float* input_real, const float* frames, int batch, int t_in, int t, long long frame_elems,
                                       int interp, float* out, void* stream) {
  ODEHIP_REQUIRE(input_real && frames && out, "gan_seq_assemble: null pointer");
  SeqArgs a;
  if (int rc = fill_seq_args("gan_seq_assemble", &a, batch, t_in, t, frame_elems, interp)) return rc;
  ODEHIP_REQUIRE((((uintptr_t)input_real | (uintptr_t)frames | (uintptr_t)out) & 3) == 0, "gan_seq_assemble: misaligned pointer (4 bytes)");
  const long long items = (long long)t * batch * a.L;
  if (frame_elems % 4 == 0 && aligned16(input_real) && aligned16(frames) && aligned16(out)) {
    a.fe = frame_elems / 4;
    const long long total = items * a.fe;
    hipLaunchKernelGGL(seq_assemble_kernel<f32x4g>, dim3(gan_blocks(total)), dim3(kGanThreads), 0, (hipStream_t)stream,
                       (const f32x4g*)input_real, (const f32x4g*)frames, a, total, (f32x4g*)out);
  } else {
    const long long total = items * a.fe;
    hipLaunchKernelGGL(seq_assemble_kernel<float>, dim3(gan_blocks(total)), dim3(kGanThreads), 0, (hipStream_t)stream, input_real, frames, a,
                       total, out);
  }
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}

extern "C" int odehip_gan_seq_assemble_backward(const float* grad_out, int batch, int t_in, int t, long long frame_elems, int interp,
                                                float* grad_frames, void* stream) {
  ODEHIP_REQUIRE(grad_out && grad_frames, "gan_seq_assemble_backward: null pointer");
  SeqArgs a;
  if (int rc = fill_seq_args("gan_seq_assemble_backward", &a, batch, t_in, t, frame_elems, interp)) return rc;
  ODEHIP_REQUIRE((((uintptr_t)grad_out | (uintptr_t)grad_frames) & 3) == 0, "gan_seq_assemble_backward: misaligned pointer (4 bytes)");
  const long long items = (long long)batch * t;
  if (frame_elems % 4 == 0 && aligned16(grad_out) && aligned16(grad_frames)) {
    a.fe = frame_elems / 4;
    const long long total = items * a.fe;
    hipLaunchKernelGGL(seq_assemble_backward_kernel<f32x4g>, dim3(gan_blocks(total)), dim3(kGanThreads), 0, (hipStream_t)stream,
                       (const f32x4g*)grad_out, a, total, (f32x4g*)grad_frames);
  } else {
    const long long total = items * a.fe;
    hipLaunchKernelGGL(seq_assemble_backward_kernel<float>, dim3(gan_blocks(total)), dim3(kGanThreads), 0, (hipStream_t)stream, grad_out, a,
                       total, grad_frames);
  }
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}

extern "C" size_t odehip_loss_lsgan_workspace_bytes(long long n) {
  if (n < 1) return 0;
  return (size_t)sum_groups(n) * sizeof(double);
}

extern "C" int odehip_loss_lsgan(const float* pred, long long n, float target, float* out, void* workspace, void* stream) {
  ODEHIP_REQUIRE(pred && out && workspace, "loss_lsgan: null pointer");
  ODEHIP_REQUIRE(n >= 1, "loss_lsgan: n (%lld) must be at least 1", n);
  ODEHIP_REQUIRE((((uintptr_t)pred | (uintptr_t)out) & 3) == 0 && ((uintptr_t)workspace & 7) == 0,
                 "loss_lsgan: misaligned pred or out (4 bytes) or workspace (8 bytes)");
  const int groups = sum_groups(n);
  hipLaunchKernelGGL(lsgan_partial_kernel, dim3((unsigned)groups), dim3(kGanThreads), 0, (hipStream_t)stream, pred, n, (double)target,
                     (double*)workspace);
  ODEHIP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(lsgan_final_kernel, dim3(1), dim3(kGanThreads), 0, (hipStream_t)stream, (const double*)workspace, groups, (double)n, out);
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}

extern "C" int odehip_loss_lsgan_backward(const float* grad_out, const float* pred, long long n, float target, float* grad, void* stream) {
  ODEHIP_REQUIRE(grad_out && pred && grad, "loss_lsgan_backward: null pointer");
  ODEHIP_REQUIRE(n >= 1, "loss_lsgan_backward: n (%lld) must be at least 1", n);
  ODEHIP_REQUIRE((((uintptr_t)grad_out | (uintptr_t)pred | (uintptr_t)grad) & 3) == 0, "loss_lsgan_backward: misaligned pointer (4 bytes)");
  hipLaunchKernelGGL(lsgan_backward_kernel, dim3(gan_blocks(n)), dim3(kGanThreads), 0, (hipStream_t)stream, grad_out, pred, n, (double)target,
                     grad);
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}
