// frame_loss.hip -- the scalar training losses of the models and their backward, each one C ABI call: the MSE (+ KL term) of
// models/ODEConvGRU.py and models/ConvGRU.py, and the L1 pair of models/VidODE.py (reference :211-226).  No host round trip, no
// hidden allocation, no floating-point atomics.
//
//   MSE (+KL)  pred (K B, F) sample-major against truth (B, F): element i of pred row k B + b pairs with element i of truth row b
//              (the truth is never repeated in memory).  out = {mse + kl_weight kl_term, mse, kl_term},
//              mse = sum (p - t)^2 / (K B F), kl_term = kl_scale sum_b kl[b];  grad_pred = (p - t) (2 g / N), grad_kl[b] = g kl_weight kl_scale
//   L1 pair    pred, inter (B, n, P) against the n SELECTED frames of truth (B, T, P): s(b, j) = the j-th t with mask[b][t] != 0,
//              d(b, t) = truth[b][t] - (t > 0 ? truth[b][t - 1] : init[b]);  out = {l1_pred + l1_diff, l1_pred, l1_diff},
//              l1_pred = sum |pred[b][j] - truth[b][s]| / (B n P), l1_diff = sum |inter[b][j] - d(b, s)| / (B n P);
//              grad_pred = sgn(pred - truth_s) g / N, grad_inter = sgn(inter - d) g / N, sgn(0) = sgn(NaN) = 0 (torch.abs's backward)
//
// Arithmetic.  Every difference, square, absolute value and sum is formed in float64 from the fp32 inputs and rounded to fp32 once.
// Sum order: a thread adds its elements in ascending order (16-byte loads, the four elements of a quad in order), then reduce.h's
// workgroup sum, and the second launch is reduce.h's ordered sum of the workgroup partials.  Which elements a thread sees is a
// function of the sizes alone (sum_groups / l1_groups), never of the machine: two calls are bitwise equal, on any device.
//
// Launches.  Forward: partials, then a one-workgroup final (as frame_metrics.hip).  The single-launch form with an arrival ticket
// needs a zeroed word per call -- a memset node, i.e. a second launch all the same -- or a ticket the last workgroup resets, which
// one aborted launch leaves poisoned for every later call; two plain launches have neither problem.  Backward: one launch.
#include <math.h>
#include <stdint.h>

#include "odehip_internal.h"
#include "reduce.h"

namespace odehip {

typedef float f32x4l __attribute__((ext_vector_type(4)));

constexpr int kLossThreads = 256;
constexpr int kL1ChunkQuads = 1024;       // L1 pair: a work item is this many quads of one (b, j) frame (one 64 x 64 plane)

// N of the MSE: every element of every draw
static inline double mse_elems(int n_samples, int batch, long long row_elems) { return (double)n_samples * (double)batch * (double)row_elems; }
static inline int l1_chunks(int frame_elems) { return (frame_elems / 4 + kL1ChunkQuads - 1) / kL1ChunkQuads; }
static inline int l1_groups(long long items) { return items > kSumMaxGroups ? kSumMaxGroups : (int)items; }

// ---- MSE ------------------------------------------------------------------------------------------------------------------------

// the truth quad that pairs with pred quad q: pred row r = k B + b -> truth row b
__device__ __forceinline__ unsigned mse_truth_quad(unsigned q, unsigned row_quads, unsigned batch, int n_samples) {
  if (n_samples == 1) return q;
  const unsigned r = q / row_quads, i = q - r * row_quads;
  const unsigned b = r % batch;
  return b * row_quads + i;
}

__global__ __launch_bounds__(kLossThreads) void loss_mse_partial_kernel(const float* __restrict__ pred, const float* __restrict__ truth,
                                                                        unsigned quads, unsigned row_quads, unsigned batch, int n_samples,
                                                                        double* __restrict__ partials) {
  __shared__ double red[kLossThreads / 64];
  const unsigned stride = gridDim.x * kLossThreads;
  double acc = 0.0;
#pragma unroll 4
  for (unsigned q = blockIdx.x * kLossThreads + threadIdx.x; q < quads; q += stride) {
    const f32x4l p = ((const f32x4l*)pred)[q];
    const f32x4l t = ((const f32x4l*)truth)[mse_truth_quad(q, row_quads, batch, n_samples)];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double d = (double)p[i] - (double)t[i];
      acc += d * d;
    }
  }
  const double g = group_sum<kLossThreads>(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = g;
}

// one workgroup: the partials in workgroup order, kl[b] strided over the threads and folded like a workgroup partial
__global__ __launch_bounds__(kLossThreads) void loss_mse_final_kernel(const double* __restrict__ partials, int n_partials, double n_elems,
                                                                      const float* __restrict__ kl, int batch, double kl_scale,
                                                                      float kl_weight, float* __restrict__ out) {
  __shared__ double stage[kSumMaxGroups];
  __shared__ double red[kLossThreads / 64];
  double k = 0.0;
  if (kl)
    for (int b = threadIdx.x; b < batch; b += kLossThreads) k += (double)kl[b];
  k = group_sum<kLossThreads>(k, red);
  const double s = ordered_sum<kLossThreads>(partials, n_partials, stage);
  if (threadIdx.x == 0) {
    const double mse = s / n_elems, kl_term = kl ? k * kl_scale : 0.0;
    out[0] = (float)(kl ? mse + (double)kl_weight * kl_term : mse);
    out[1] = (float)mse;
    out[2] = (float)kl_term;
  }
}

__global__ __launch_bounds__(kLossThreads) void loss_mse_backward_kernel(const float* __restrict__ grad_out, const float* __restrict__ pred,
                                                                         const float* __restrict__ truth, unsigned quads, unsigned row_quads,
                                                                         unsigned batch, int n_samples, double n_elems, double kl_scale,
                                                                         float kl_weight, float* __restrict__ grad_pred,
                                                                         float* __restrict__ grad_kl) {
#pragma clang fp contract(off)
  const double g = (double)grad_out[0];
  const float scale = (float)(2.0 * g / n_elems);
  const unsigned stride = gridDim.x * kLossThreads, first = blockIdx.x * kLossThreads + threadIdx.x;
  if (grad_kl) {
    const float gk = (float)(g * (double)kl_weight * kl_scale);
    for (unsigned b = first; b < batch; b += stride) grad_kl[b] = gk;
  }
#pragma unroll 4
  for (unsigned q = first; q < quads; q += stride) {
    const f32x4l p = ((const f32x4l*)pred)[q];
    const f32x4l t = ((const f32x4l*)truth)[mse_truth_quad(q, row_quads, batch, n_samples)];
    ((f32x4l*)grad_pred)[q] = (p - t) * scale;
  }
}

// ---- VidODE L1 pair -------------------------------------------------------------------------------------------------------------

struct L1Args {
  const float* pred;    // (B, n, P)
  const float* inter;   // (B, n, P) through inter_bs / inter_fs (elements)
  const float* truth;   // (B, T, P)
  const float* init;    // (B, P) through init_bs
  const void* mask;     // (B, T): float32 (mask_bytes 4) or uint8 / bool (mask_bytes 1); non-zero = selected
  long long inter_bs, inter_fs, init_bs;
  int batch, n_frames, n_sel, frame_quads, chunks, mask_bytes;
  long long items;      // batch * n_sel * chunks
};

// the j-th selected frame of mask row b, or -1 if the row selects fewer than j + 1 (every lane scans the same row: scalar loads)
__device__ __forceinline__ int l1_selected(const L1Args& a, int b, int j) {
  const long long row = (long long)b * a.n_frames;
  int s = -1, seen = 0;
  for (int t = 0; t < a.n_frames; ++t) {
    const bool on = a.mask_bytes == 4 ? ((const float*)a.mask)[row + t] != 0.0f : ((const unsigned char*)a.mask)[row + t] != 0;
    if (on) {
      if (seen == j && s < 0) s = t;
      ++seen;
    }
  }
  return s;
}

// what one work item walks: chunk `c` of frame (b, j) and the selected truth frame s
struct L1Item {
  int b, j, s, q0, q1;
};
__device__ __forceinline__ L1Item l1_item(const L1Args& a, long long item) {
  L1Item it;
  const long long f = item / a.chunks;
  const int c = (int)(item - f * a.chunks);
  it.b = (int)(f / a.n_sel);
  it.j = (int)(f - (long long)it.b * a.n_sel);
  it.s = l1_selected(a, it.b, it.j);
  it.q0 = c * kL1ChunkQuads;
  it.q1 = it.q0 + kL1ChunkQuads < a.frame_quads ? it.q0 + kL1ChunkQuads : a.frame_quads;
  return it;
}
// the four operand rows of frame (b, j) with selected frame s >= 0, as quad pointers
struct L1Rows {
  const f32x4l *p, *x, *t, *prev;
};
__device__ __forceinline__ L1Rows l1_rows(const L1Args& a, const L1Item& it) {
  L1Rows r;
  const long long fq = a.frame_quads;
  r.p = (const f32x4l*)a.pred + ((long long)it.b * a.n_sel + it.j) * fq;
  r.x = (const f32x4l*)(a.inter + it.b * a.inter_bs + it.j * a.inter_fs);
  r.t = (const f32x4l*)a.truth + ((long long)it.b * a.n_frames + it.s) * fq;
  r.prev = it.s > 0 ? r.t - fq : (const f32x4l*)(a.init + it.b * a.init_bs);
  return r;
}

__global__ __launch_bounds__(kLossThreads) void loss_l1_partial_kernel(L1Args a, double* __restrict__ partials) {
  __shared__ double red[kLossThreads / 64];
  double acc_p = 0.0, acc_d = 0.0;
  for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
    const L1Item it = l1_item(a, item);
    if (it.s < 0) {   // the row selects too few frames (uniform over the workgroup): nothing is read, the sums become NaN
      acc_p = acc_d = (double)NAN;
      continue;
    }
    const L1Rows r = l1_rows(a, it);
    for (int q = it.q0 + threadIdx.x; q < it.q1; q += kLossThreads) {
      const f32x4l p = r.p[q], x = r.x[q], t = r.t[q], v = r.prev[q];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double td = (double)t[i];
        acc_p += fabs((double)p[i] - td);
        acc_d += fabs((double)x[i] - (td - (double)v[i]));
      }
    }
  }
  const double gp = group_sum<kLossThreads>(acc_p, red);
  __syncthreads();   // red is used again
  const double gd = group_sum<kLossThreads>(acc_d, red);
  if (threadIdx.x == 0) {
    partials[2 * blockIdx.x] = gp;
    partials[2 * blockIdx.x + 1] = gd;
  }
}

__global__ __launch_bounds__(kLossThreads) void loss_l1_final_kernel(const double* __restrict__ partials, int n_partials, double n_elems,
                                                                     float* __restrict__ out) {
  // reduce.h's ordered sum of two interleaved series at once: thread 0's additions are the whole cost of this kernel, and two
  // ordered_sum calls would run the two dependent chains one after the other instead of side by side
  __shared__ double stage[2 * kSumMaxGroups];
  for (int i = threadIdx.x; i < 2 * n_partials; i += kLossThreads) stage[i] = partials[i];
  __syncthreads();
  if (threadIdx.x == 0) {
    double sp = 0.0, sd = 0.0;
    for (int i = 0; i < n_partials; ++i) {
      sp += stage[2 * i];
      sd += stage[2 * i + 1];
    }
    const double l1_pred = sp / n_elems, l1_diff = sd / n_elems;
    out[0] = (float)(l1_pred + l1_diff);
    out[1] = (float)l1_pred;
    out[2] = (float)l1_diff;
  }
}

// torch.abs's backward multiplies by sgn: 0 at 0 and at NaN, +-1 at +-inf
__device__ __forceinline__ float l1_sgn(double v) { return (float)((0.0 < v) - (v < 0.0)); }

__global__ __launch_bounds__(kLossThreads) void loss_l1_backward_kernel(L1Args a, const float* __restrict__ grad_out, double n_elems,
                                                                        float* __restrict__ grad_pred, float* __restrict__ grad_inter) {
#pragma clang fp contract(off)
  const float scale = (float)((double)grad_out[0] / n_elems);
  for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
    const L1Item it = l1_item(a, item);
    const long long out0 = ((long long)it.b * a.n_sel + it.j) * a.frame_quads;
    f32x4l* const gp = (f32x4l*)grad_pred + out0;
    f32x4l* const gx = (f32x4l*)grad_inter + out0;
    if (it.s < 0) {   // too few selected frames: the loss is NaN, and so is the gradient of the frames it could not pair
      const f32x4l nan4 = {NAN, NAN, NAN, NAN};
      for (int q = it.q0 + threadIdx.x; q < it.q1; q += kLossThreads) gp[q] = gx[q] = nan4;
      continue;
    }
    const L1Rows r = l1_rows(a, it);
    for (int q = it.q0 + threadIdx.x; q < it.q1; q += kLossThreads) {
      const f32x4l p = r.p[q], x = r.x[q], t = r.t[q], v = r.prev[q];
      f32x4l op, ox;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double td = (double)t[i];
        op[i] = l1_sgn((double)p[i] - td) * scale;
        ox[i] = l1_sgn((double)x[i] - (td - (double)v[i])) * scale;
      }
      gp[q] = op;
      gx[q] = ox;
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------

// 0 or ODEHIP_EINVAL (message set); *quads_out = the quads of pred
static int check_mse_shape(const char* who, int n_samples, int batch, long long row_elems, long long* quads_out) {
  ODEHIP_REQUIRE(n_samples >= 1 && batch >= 1 && row_elems >= 4, "%s: n_samples (%d), batch (%d) and row_elems (%lld) must be at least 1, 1 and 4",
                 who, n_samples, batch, row_elems);
  ODEHIP_REQUIRE(row_elems % 4 == 0, "%s: row_elems (%lld) must be a multiple of 4 (16-byte loads)", who, row_elems);
  const long long row_quads = row_elems / 4;
  ODEHIP_REQUIRE(row_quads <= 0x7fffffffLL / batch && row_quads * batch <= 0x7fffffffLL / n_samples,
                 "%s: n_samples * batch * row_elems (%d x %d x %lld) exceeds 2^33 elements", who, n_samples, batch, row_elems);
  *quads_out = row_quads * batch * n_samples;
  return ODEHIP_OK;
}

static int fill_l1_args(const char* who, L1Args* a, const float* pred, const float* inter, long long inter_bs, long long inter_fs,
                        const float* truth, const float* init, long long init_bs, const void* mask, int mask_is_byte, int batch, int n_frames,
                        int n_sel, int frame_elems) {
  ODEHIP_REQUIRE(pred && inter && truth && init && mask, "%s: null pointer", who);
  ODEHIP_REQUIRE(batch >= 1 && n_frames >= 1 && n_sel >= 1 && frame_elems >= 4,
                 "%s: batch (%d), n_frames (%d), n_sel (%d) and frame_elems (%d) must be at least 1, 1, 1 and 4", who, batch, n_frames, n_sel,
                 frame_elems);
  ODEHIP_REQUIRE(n_sel <= n_frames, "%s: n_sel (%d) exceeds n_frames (%d)", who, n_sel, n_frames);
  ODEHIP_REQUIRE(frame_elems % 4 == 0, "%s: frame_elems (%d) must be a multiple of 4 (16-byte loads)", who, frame_elems);
  ODEHIP_REQUIRE(mask_is_byte == 0 || mask_is_byte == 1, "%s: mask_is_byte must be 0 (float32) or 1 (uint8 / bool), got %d", who, mask_is_byte);
  ODEHIP_REQUIRE(aligned16(pred) && aligned16(inter) && aligned16(truth) && aligned16(init), "%s: pred, inter, truth and init must be 16-byte aligned", who);
  ODEHIP_REQUIRE(mask_is_byte || ((uintptr_t)mask & 3) == 0, "%s: a float32 mask must be 4-byte aligned", who);
  ODEHIP_REQUIRE(inter_fs >= frame_elems && inter_fs % 4 == 0 && inter_bs % 4 == 0 && inter_bs >= inter_fs * (n_sel - 1) + frame_elems,
                 "%s: inter strides (batch %lld, frame %lld) must be multiples of 4 that hold %d frames of %d elements", who, inter_bs, inter_fs,
                 n_sel, frame_elems);
  ODEHIP_REQUIRE(init_bs >= frame_elems && init_bs % 4 == 0, "%s: init batch stride (%lld) must be a multiple of 4 of at least frame_elems (%d)",
                 who, init_bs, frame_elems);
  ODEHIP_REQUIRE((long long)batch * n_frames * (frame_elems / 4) <= 0x7fffffffLL, "%s: batch * n_frames * frame_elems (%d x %d x %d) exceeds 2^33 elements",
                 who, batch, n_frames, frame_elems);
  a->pred = pred, a->inter = inter, a->truth = truth, a->init = init, a->mask = mask;
  a->inter_bs = inter_bs, a->inter_fs = inter_fs, a->init_bs = init_bs;
  a->batch = batch, a->n_frames = n_frames, a->n_sel = n_sel, a->frame_quads = frame_elems / 4;
  a->chunks = l1_chunks(frame_elems), a->mask_bytes = mask_is_byte ? 1 : 4;
  a->items = (long long)batch * n_sel * a->chunks;
  return ODEHIP_OK;
}

}  // namespace odehip

using namespace odehip;

extern "C" size_t odehip_loss_mse_workspace_bytes(int n_samples, int batch, long long row_elems) {
  if (n_samples < 1 || batch < 1 || row_elems < 4) return 0;
  return (size_t)sum_groups((row_elems / 4) * batch * n_samples) * sizeof(double);
}

extern "C" int odehip_loss_mse(const float* pred, const float* truth, int n_samples, int batch, long long row_elems, const float* kl,
                               double kl_scale, float kl_weight, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  ODEHIP_REQUIRE(pred && truth && out && workspace, "loss_mse: null pointer");
  long long quads;
  if (int rc = check_mse_shape("loss_mse", n_samples, batch, row_elems, &quads)) return rc;
  ODEHIP_REQUIRE(aligned16(pred) && aligned16(truth), "loss_mse: pred and truth must be 16-byte aligned");
  ODEHIP_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)kl & 3) == 0,
                 "loss_mse: misaligned workspace (8 bytes), out or kl (4 bytes)");
  const int groups = sum_groups(quads);
  ODEHIP_REQUIRE(workspace_bytes >= (size_t)groups * sizeof(double), "loss_mse: workspace of %zu bytes, %zu needed", workspace_bytes,
                 (size_t)groups * sizeof(double));
  hipLaunchKernelGGL(loss_mse_partial_kernel, dim3((unsigned)groups), dim3(kLossThreads), 0, (hipStream_t)stream, pred, truth, (unsigned)quads,
                     (unsigned)(row_elems / 4), (unsigned)batch, n_samples, (double*)workspace);
  ODEHIP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(loss_mse_final_kernel, dim3(1), dim3(kLossThreads), 0, (hipStream_t)stream, (const double*)workspace, groups,
                     mse_elems(n_samples, batch, row_elems), kl, batch, kl_scale, kl_weight, out);
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}

extern "C" int odehip_loss_mse_backward(const float* grad_out, const float* pred, const float* truth, int n_samples, int batch,
                                        long long row_elems, double kl_scale, float kl_weight, float* grad_pred, float* grad_kl, void* stream) {
  ODEHIP_REQUIRE(grad_out && pred && truth && grad_pred, "loss_mse_backward: null pointer");
  long long quads;
  if (int rc = check_mse_shape("loss_mse_backward", n_samples, batch, row_elems, &quads)) return rc;
  ODEHIP_REQUIRE(aligned16(pred) && aligned16(truth) && aligned16(grad_pred), "loss_mse_backward: pred, truth and grad_pred must be 16-byte aligned");
  ODEHIP_REQUIRE(((uintptr_t)grad_out & 3) == 0 && ((uintptr_t)grad_kl & 3) == 0, "loss_mse_backward: misaligned grad_out or grad_kl (4 bytes)");
  const long long groups = (quads + kLossThreads - 1) / kLossThreads;
  hipLaunchKernelGGL(loss_mse_backward_kernel, dim3((unsigned)(groups > 4096 ? 4096 : groups)), dim3(kLossThreads), 0, (hipStream_t)stream,
                     grad_out, pred, truth, (unsigned)quads, (unsigned)(row_elems / 4), (unsigned)batch, n_samples, mse_elems(n_samples, batch, row_elems), kl_scale,
                     kl_weight, grad_pred, grad_kl);
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}

extern "C" size_t odehip_loss_vidode_l1_workspace_bytes(int batch, int n_sel, int frame_elems) {
  if (batch < 1 || n_sel < 1 || frame_elems < 4) return 0;
  return (size_t)l1_groups((long long)batch * n_sel * l1_chunks(frame_elems)) * 2 * sizeof(double);
}

extern "C" int odehip_loss_vidode_l1(const float* pred, const float* inter, long long inter_batch_stride, long long inter_frame_stride,
                                     const float* truth, const float* init, long long init_batch_stride, const void* mask, int mask_is_byte,
                                     int batch, int n_frames, int n_sel, int frame_elems, float* out, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  L1Args a;
  if (int rc = fill_l1_args("loss_vidode_l1", &a, pred, inter, inter_batch_stride, inter_frame_stride, truth, init, init_batch_stride, mask,
                            mask_is_byte, batch, n_frames, n_sel, frame_elems))
    return rc;
  ODEHIP_REQUIRE(out && workspace && ((uintptr_t)workspace & 7) == 0 && ((uintptr_t)out & 3) == 0,
                 "loss_vidode_l1: null or misaligned out (4 bytes) or workspace (8 bytes)");
  const int groups = l1_groups(a.items);
  ODEHIP_REQUIRE(workspace_bytes >= (size_t)groups * 2 * sizeof(double), "loss_vidode_l1: workspace of %zu bytes, %zu needed", workspace_bytes,
                 (size_t)groups * 2 * sizeof(double));
  hipLaunchKernelGGL(loss_l1_partial_kernel, dim3((unsigned)groups), dim3(kLossThreads), 0, (hipStream_t)stream, a, (double*)workspace);
  ODEHIP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(loss_l1_final_kernel, dim3(1), dim3(kLossThreads), 0, (hipStream_t)stream, (const double*)workspace, groups,
                     (double)batch * n_sel * frame_elems, out);
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}

extern "C" int odehip_loss_vidode_l1_backward(const float* grad_out, const float* pred, const float* inter, long long inter_batch_stride,
                                              long long inter_frame_stride, const float* truth, const float* init, long long init_batch_stride,
                                              const void* mask, int mask_is_byte, int batch, int n_frames, int n_sel, int frame_elems,
                                              float* grad_pred, float* grad_inter, void* stream) {
  L1Args a;
  if (int rc = fill_l1_args("loss_vidode_l1_backward", &a, pred, inter, inter_batch_stride, inter_frame_stride, truth, init, init_batch_stride,
                            mask, mask_is_byte, batch, n_frames, n_sel, frame_elems))
    return rc;
  ODEHIP_REQUIRE(grad_out && grad_pred && grad_inter && aligned16(grad_pred) && aligned16(grad_inter) && ((uintptr_t)grad_out & 3) == 0,
                 "loss_vidode_l1_backward: null or misaligned grad_out (4 bytes), grad_pred or grad_inter (16 bytes)");
  const long long groups = a.items > 4096 ? 4096 : a.items;
  hipLaunchKernelGGL(loss_l1_backward_kernel, dim3((unsigned)groups), dim3(kLossThreads), 0, (hipStream_t)stream, a, grad_out,
                     (double)batch * n_sel * frame_elems, grad_pred, grad_inter);
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}
