// convgru_plain.hip -- the norm-free ConvGRU cell of upstream Vid-ODE (models/base_conv_gru.py:47-72) on Q4 tensors (gfx950).
//
//   (r, u) = sigmoid(conv3x3(cat(x, h)))        RESET first, UPDATE second (:57)
//   c      = tanh(conv3x3(cat(x, r*h)))
//   h'     = (1-u) h + u c                      then, with the step's observation mask m:  m h' + (1-m) h   (:69-70)
//
// A cell descriptor whose four gn_* pointers are all NULL is this cell (convgru.hip: cell_is_plain).  The convolutions, the
// input-gradient convolutions and the weight-gradient launches are the ones the GroupNorm cell uses; what differs is everything
// between them, which without a normalisation is pointwise: four kernels, one f32x4 quad (four channels of one pixel) per thread.
// Grid (channel quad, sample), 256 threads = the 256 pixels of a 16x16 map: the sample has its own axis, so the step's mask value is
// one uniform scalar per workgroup and the three branches on it do not diverge.
//
// Backward, with g the gradient at the blended state, g' = m g what the cell's chain is fed:
//   plain_update_bwd_kernel   g_u = g'(c-h), g_c = g' u;  writes g_cand_raw = g_c (1-c^2), the UPDATE half of g_gates_raw =
//                             g_u u(1-u), and gh = g'(1-u) + (1-m) g
//   (the candidate's two input-gradient convolutions give gx_c and g_rh)
//   plain_gates_bwd_kernel    g_r = g_rh h;  gh += g_rh r;  writes the RESET half of g_gates_raw = g_r r(1-r)
// r, u's derivative and c are recomputed from the saved convolution outputs: nothing but those is stored.  For m == 0 both kernels
// store exact zeros, not products with what the forward kept for that (frame, sample) -- the contract of
// odehip_odeconvgru_encode_train_masked.  No reduction happens here: the bias gradients are column sums of g_gates_raw / g_cand_raw,
// summed in a fixed order by the weight-gradient launches (wgrad.hip).  No float atomics.
#include "convgru_cell.h"

namespace odehip {

// gates_raw: (B, 2H) Q4, grid (2 * hq, B) with hq = H / 4.  Quads [0, hq) are the reset gate, the rest the update gate.  Writes
// u (B, H) and rh = r * h (B, H).
__global__ __launch_bounds__(256) void plain_gates_kernel(const float* __restrict__ gates_raw, const float* __restrict__ h,
                                                          float* __restrict__ u_out, float* __restrict__ rh_out, int hq) {
  const int q = blockIdx.x, b = blockIdx.y;
  const f32x4 s = sigmoid4(((const f32x4*)gates_raw)[((size_t)b * 2 * hq + q) * kPix + threadIdx.x]);
  const bool is_reset = q < hq;
  const size_t o = ((size_t)b * hq + (is_reset ? q : q - hq)) * kPix + threadIdx.x;
  if (is_reset) ((f32x4*)rh_out)[o] = s * ((const f32x4*)h)[o];
  else ((f32x4*)u_out)[o] = s;
}

// cand_raw, h, u: (B, H) Q4, grid (hq, B).  h' = (1-u) h + u tanh(cand_raw); optionally also written to an NCHW slot (latent_ys).
// kMasked: mask_b[b] = m.  m == 1: bit for bit what the unmasked instantiation writes; m == 0: h is copied and nothing the cell
// computed is read; otherwise m h' + (1-m) h in fp32.  The unmasked instantiation never reads mask_b.
template <bool kMasked>
__global__ __launch_bounds__(256) void plain_update_kernel(const float* __restrict__ cand_raw, const float* __restrict__ h,
                                                           const float* __restrict__ u, float* __restrict__ h_out,
                                                           float* __restrict__ h_out_nchw, long long nchw_batch_stride, int hq,
                                                           const float* __restrict__ mask_b) {
  const int q = blockIdx.x, b = blockIdx.y;
  const size_t o = ((size_t)b * hq + q) * kPix + threadIdx.x;
  const float m = kMasked ? mask_b[b] : 1.0f;
  const f32x4 hh = ((const f32x4*)h)[o];
  f32x4 r = hh;
  if (!(kMasked && m == 0.0f)) {
    const f32x4 c = tanh4(((const f32x4*)cand_raw)[o]);
    const f32x4 uu = ((const f32x4*)u)[o];
    r = (1.0f - uu) * hh + uu * c;
    if (kMasked && m != 1.0f) r = m * r + (1.0f - m) * hh;
  }
  ((f32x4*)h_out)[o] = r;
  if (h_out_nchw) {
    float* n = h_out_nchw + (size_t)b * nchw_batch_stride + (size_t)(q * 4) * kPix + threadIdx.x;
    n[0] = r.x; n[kPix] = r.y; n[2 * kPix] = r.z; n[3 * kPix] = r.w;
  }
}

// backward of the update and the blend; grid (hq, B).  gh: gradient at the blended state.  g_gates_raw: (B, 2H), only its update
// half (quads [hq, 2 hq)) is written here.
template <bool kMasked>
__global__ __launch_bounds__(256) void plain_update_bwd_kernel(const float* __restrict__ cand_raw, const float* __restrict__ gh,
                                                               const float* __restrict__ u, const float* __restrict__ h,
                                                               float* __restrict__ g_cand_raw, float* __restrict__ g_gates_raw,
                                                               float* __restrict__ gh_out, int hq, const float* __restrict__ mask_b) {
  const int q = blockIdx.x, b = blockIdx.y;
  const size_t o = ((size_t)b * hq + q) * kPix + threadIdx.x;
  const size_t ou = ((size_t)b * 2 * hq + hq + q) * kPix + threadIdx.x;
  const float m = kMasked ? mask_b[b] : 1.0f;
  const f32x4 g = ((const f32x4*)gh)[o];
  if (kMasked && m == 0.0f) {  // unobserved: the state went through unchanged, the cell's chain gets exact zeros
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    ((f32x4*)gh_out)[o] = g;
    ((f32x4*)g_cand_raw)[o] = zero;
    ((f32x4*)g_gates_raw)[ou] = zero;
    return;
  }
  const bool blend = kMasked && m != 1.0f;
  const f32x4 gc = blend ? m * g : g;  // what the cell's chain is fed
  const f32x4 c = tanh4(((const f32x4*)cand_raw)[o]);
  const f32x4 uu = ((const f32x4*)u)[o], hh = ((const f32x4*)h)[o];
  ((f32x4*)g_cand_raw)[o] = gc * uu * (1.0f - c * c);
  ((f32x4*)g_gates_raw)[ou] = gc * (c - hh) * uu * (1.0f - uu);
  f32x4 d = gc * (1.0f - uu);
  if (blend) d += (1.0f - m) * g;  // the part of the blend that bypasses the cell
  ((f32x4*)gh_out)[o] = d;
}

// backward of rh = r * h, r = sigmoid(reset half of gates_raw); grid (hq, B).  gh_io += g_rh r; writes the reset half of g_gates_raw.
// mask_b: the step's mask values or null.  m == 0: g_rh is the image of exact zeros, so gh_io stays and exact zeros are stored.
__global__ __launch_bounds__(256) void plain_gates_bwd_kernel(const float* __restrict__ gates_raw, const float* __restrict__ g_rh,
                                                              const float* __restrict__ h, float* __restrict__ gh_io,
                                                              float* __restrict__ g_gates_raw, int hq, const float* __restrict__ mask_b) {
  const int q = blockIdx.x, b = blockIdx.y;
  const size_t o = ((size_t)b * hq + q) * kPix + threadIdx.x;
  const size_t og = ((size_t)b * 2 * hq + q) * kPix + threadIdx.x;
  if (mask_b && mask_b[b] == 0.0f) {
    ((f32x4*)g_gates_raw)[og] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    return;
  }
  const f32x4 r = sigmoid4(((const f32x4*)gates_raw)[og]);
  const f32x4 g = ((const f32x4*)g_rh)[o];
  ((f32x4*)gh_io)[o] += g * r;
  ((f32x4*)g_gates_raw)[og] = g * ((const f32x4*)h)[o] * r * (1.0f - r);
}

// host-side handles (convgru.hip, convgru_backward.hip); hidden % 4 == 0 is the callers' check_cell
void launch_plain_gates(const float* gates_raw, const float* h, float* u, float* rh, int hidden, int batch, hipStream_t stream) {
  hipLaunchKernelGGL(plain_gates_kernel, dim3(2 * hidden / 4, batch), dim3(256), 0, stream, gates_raw, h, u, rh, hidden / 4);
}
void launch_plain_update(const float* cand_raw, const float* h, const float* u, float* h_out, float* h_out_nchw, long long nchw_batch_stride,
                         int hidden, int batch, const float* mask_b, hipStream_t stream) {
  if (mask_b)
    hipLaunchKernelGGL(plain_update_kernel<true>, dim3(hidden / 4, batch), dim3(256), 0, stream, cand_raw, h, u, h_out, h_out_nchw,
                       nchw_batch_stride, hidden / 4, mask_b);
  else
    hipLaunchKernelGGL(plain_update_kernel<false>, dim3(hidden / 4, batch), dim3(256), 0, stream, cand_raw, h, u, h_out, h_out_nchw,
                       nchw_batch_stride, hidden / 4, nullptr);
}
void launch_plain_update_bwd(const float* cand_raw, const float* gh, const float* u, const float* h, float* g_cand_raw, float* g_gates_raw,
                             float* gh_out, int hidden, int batch, const float* mask_b, hipStream_t stream) {
  if (mask_b)
    hipLaunchKernelGGL(plain_update_bwd_kernel<true>, dim3(hidden / 4, batch), dim3(256), 0, stream, cand_raw, gh, u, h, g_cand_raw,
                       g_gates_raw, gh_out, hidden / 4, mask_b);
  else
    hipLaunchKernelGGL(plain_update_bwd_kernel<false>, dim3(hidden / 4, batch), dim3(256), 0, stream, cand_raw, gh, u, h, g_cand_raw,
                       g_gates_raw, gh_out, hidden / 4, nullptr);
}
void launch_plain_gates_bwd(const float* gates_raw, const float* g_rh, const float* h, float* gh_io, float* g_gates_raw, int hidden,
                            int batch, const float* mask_b, hipStream_t stream) {
  hipLaunchKernelGGL(plain_gates_bwd_kernel, dim3(hidden / 4, batch), dim3(256), 0, stream, gates_raw, g_rh, h, gh_io, g_gates_raw,
                     hidden / 4, mask_b);
}

}  // namespace odehip
