// convgru_backward.hip -- training path of the ODE-ConvGRU encoder (gfx950): forward with everything the reverse sweep
// needs kept in the workspace, and the reverse sweep itself.  What `loss.backward()` computes through
// /root/reference/modules/ODEConvGRUCell.py:32-78 and /root/reference/modules/ConvGRUCell.py:72-82 (train_test.py:204).
//
// Per observed frame (reverse order):
//   forward   k = f_enc(h); h_ode = h + dt k; G = conv5(cat(x, h_ode)); (z, r) = sigmoid(GN(G)); rh = r*h_ode;
//             Cr = conv5(cat(x, rh)); c = tanh(GN(Cr)); h' = (1-z) h_ode + z c
//   backward  gn_update_bwd : gh' -> gCr (through tanh + GroupNorm), gz_pre = gh' (c-h_ode) z(1-z), gh_ode = gh' (1-z)
//             conv5^T(gCr)  : -> gx_c (frame part), g_rh (state part)           MFMA ring kernel, transposed+flipped slices
//             gn_gates_bwd  : -> gG (through sigmoid + GroupNorm); gh_ode += g_rh r
//             conv5^T(gG)   : -> gx = gx_c + . (frame gradient), seed = gh_ode + .   (fused in the conv epilogues)
//             f_enc^T chain : gh = seed + dt J_f(h)^T seed                    (3x3 dgrad kernels, ReLU mask fused)
//   at the end one weight-gradient launch per (layer, 64x64 tile) over ALL frames (wgrad.hip), a fixed-order reduction of
//   the per-(frame, sample) GroupNorm affine partials, and the Q4 -> NCHW conversion of the frame gradients.
// GroupNorm statistics, sigmoid/tanh outputs are recomputed from the saved pre-normalisation tensors inside the fused
// backward kernels (a 32-channel group of one sample lives in the registers of one workgroup) -- nothing but conv
// outputs is stored.  Deterministic: no float atomics.
// Observation mask (the *_masked entry points): the forward blends  state = m h' + (1-m) h_ode  in gn_update_kernel<kUpdMasked>; the sweep
// feeds the cell's chain m gh and adds (1-m) gh to gh_ode in gn_update_bwd_kernel<true>, nothing else changes.  For m == 0 that
// kernel stores exact zeros, so every later product of an unobserved (frame, sample) is 0 * (what the forward kept): exactly zero
// for finite frames.  Containment of a NON-FINITE unobserved frame is promised for the forward only -- here the input-gradient and
// weight-gradient products would multiply it by those zeros.
// Host step hint (the *_steps entry points): a step whose frame NO sample observed.  Forward: the Euler combine writes h_ode into the
// next state slot; the per-step h_ode / gates / z / rh / cand slots stay unwritten (the sweep does not read them).  Sweep: no cell
// kernel and no input-gradient convolution; the gradient at the state behind the step IS the seed of the Euler step's adjoint, so
// whoever produces it (the head, or the dynamics chain of the step behind) writes it straight into that step's seed slot, where the
// dynamics' weight-gradient table finds it; the frame's gradient slab is zero-filled.  The cell's weight-gradient tables list the
// observed steps only, and the GroupNorm partial rows of the others are zero-filled (the reduction keeps its T * B rows and its order).
// The norm-free cell (all four gn_* pointers NULL; upstream Vid-ODE's, reset gate first): forward and sweep are the same launches with
// plain_update_bwd_kernel / plain_gates_bwd_kernel (convgru_plain.hip) in place of the two GroupNorm kernels; no affine partials are
// written or reduced and the gn_* members of the gradient structs are not touched.
#include <string.h>

#include <vector>

#include "convgru_cell.h"
#include "persist.h"

namespace odehip {

// GroupNorm backward over one (sample, group): gy = gradient w.r.t. the affine output, xh = xhat.  Writes the per-channel
// partial sums of this sample (dgamma = sum_p gy*xh, dbeta = sum_p gy) and turns gy into the gradient w.r.t. the input.
__device__ __forceinline__ void gn_backward(f32x4 (&gy)[8], const f32x4 (&xh)[8], const float* gamma, int g, float rstd,
                                            float* dgamma_part, float* dbeta_part, float* sh, float* shc) {
  // per-channel sums over the 256 pixels: wave shuffle, then the four waves meet in LDS (64 values)
  float pg[32], pb[32];
#pragma unroll
  for (int q = 0; q < 8; ++q)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float a = gy[q][c] * xh[q][c], b = gy[q][c];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
      }
      pg[q * 4 + c] = a;
      pb[q * 4 + c] = b;
    }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      shc[w * 64 + i] = pg[i];
      shc[w * 64 + 32 + i] = pb[i];
    }
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const float v = (shc[threadIdx.x] + shc[64 + threadIdx.x]) + (shc[128 + threadIdx.x] + shc[192 + threadIdx.x]);
    if (threadIdx.x < 32) dgamma_part[g * 32 + threadIdx.x] = v;
    else dbeta_part[g * 32 + threadIdx.x - 32] = v;
  }
  float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const f32x4 ga = *(const f32x4*)(gamma + g * 32 + q * 4);
    gy[q] *= ga;  // dxhat
    s1 += (gy[q].x + gy[q].y) + (gy[q].z + gy[q].w);
    const f32x4 m = gy[q] * xh[q];
    s2 += (m.x + m.y) + (m.z + m.w);
  }
  const float m1 = block_sum<true>(s1, sh) * (1.0f / 8192.0f);
  const float m2 = block_sum<true>(s2, sh) * (1.0f / 8192.0f);
#pragma unroll
  for (int q = 0; q < 8; ++q) gy[q] = (gy[q] - m1 - xh[q] * m2) * rstd;
}

// backward of  h' = (1-z) h_ode + z tanh(GN(cand_raw))  for one (sample, group of 32 hidden channels)
// kMasked: mask_b[b] = m of the forward's blend  state = m h' + (1-m) h_ode  (uniform per workgroup); gh is the gradient at the
// blended state.  The cell's chain is fed m gh and h_ode receives (1-m) gh on top.  m == 1: the unmasked arithmetic, nothing
// added.  m == 0: gh_ode = gh itself and every other output of this workgroup (g_cand_raw, gz_pre, its dgamma / dbeta partial rows)
// is stored as exact zeros -- not as a product with what the forward kept, which may be non-finite for an unobserved frame.
template <bool kMasked>
__global__ __launch_bounds__(256) void gn_update_bwd_kernel(const float* __restrict__ cand_raw, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ gh,
                                                            const float* __restrict__ z, const float* __restrict__ h_ode,
                                                            float* __restrict__ g_cand_raw, float* __restrict__ gz_pre,
                                                            float* __restrict__ gh_ode, float* __restrict__ dgamma_part,
                                                            float* __restrict__ dbeta_part, int hid_groups,
                                                            const float* __restrict__ mask_b) {
  __shared__ float sh[4];
  __shared__ float shc[256];
  const int g = blockIdx.x, b = blockIdx.y;
  const int H = hid_groups * 32;
  f32x4 xh[8], gy[8], t[8];
  const float m = kMasked ? mask_b[b] : 1.0f;
  if (kMasked && m == 0.0f) {
    load_group(gh, b, hid_groups, g, gy);
    store_group(gh_ode, b, hid_groups, g, gy);
#pragma unroll
    for (int q = 0; q < 8; ++q) t[q] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    store_group(gz_pre, b, hid_groups, g, t);
    store_group(g_cand_raw, b, hid_groups, g, t);
    if (threadIdx.x < 32) dgamma_part[(size_t)b * H + g * 32 + threadIdx.x] = 0.0f;
    else if (threadIdx.x < 64) dbeta_part[(size_t)b * H + g * 32 + threadIdx.x - 32] = 0.0f;
    return;
  }
  load_group(cand_raw, b, hid_groups, g, xh);
  const float rstd = normalise(xh, sh);
  load_group(gh, b, hid_groups, g, gy);
  const bool blend = kMasked && m != 1.0f;
  if (blend) {
#pragma unroll
    for (int q = 0; q < 8; ++q) gy[q] *= m;  // what the cell's chain is fed
  }
  f32x4 zz[8], hh[8];
  load_group(z, b, hid_groups, g, zz);
  load_group(h_ode, b, hid_groups, g, hh);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const f32x4 ga = *(const f32x4*)(gamma + g * 32 + q * 4), be = *(const f32x4*)(beta + g * 32 + q * 4);
    const f32x4 cn = xh[q] * ga + be;
    const f32x4 c = {tanhf(cn.x), tanhf(cn.y), tanhf(cn.z), tanhf(cn.w)};  // not tanh4(cn): that call changes this kernel's schedule (+6 VGPRs)
    const f32x4 g0 = gy[q];
    t[q] = g0 * (c - hh[q]) * zz[q] * (1.0f - zz[q]);  // gradient w.r.t. the z pre-activation (after GroupNorm)
    hh[q] = g0 * (1.0f - zz[q]);                        // direct path to h_ode
    gy[q] = g0 * zz[q] * (1.0f - c * c);                // gradient w.r.t. GN(cand_raw)
  }
  store_group(gz_pre, b, hid_groups, g, t);
  store_group(gh_ode, b, hid_groups, g, hh);
  gn_backward(gy, xh, gamma, g, rstd, dgamma_part + (size_t)b * H, dbeta_part + (size_t)b * H, sh, shc);
  store_group(g_cand_raw, b, hid_groups, g, gy);
  if (blend) {  // the part of the blend that bypasses the cell: gh_ode += (1-m) gh, once the group's registers are free again
    const f32x4* gp = (const f32x4*)(gh + ((size_t)(b * hid_groups + g) * 8) * kPix * 4) + threadIdx.x;
    f32x4* p = (f32x4*)(gh_ode + ((size_t)(b * hid_groups + g) * 8) * kPix * 4) + threadIdx.x;  // this thread's own stores above
#pragma unroll
    for (int q = 0; q < 8; ++q) p[q * kPix] += (1.0f - m) * gp[q * kPix];
  }
}

// backward of  (z, r) = sigmoid(GN(gates_raw)), rh = r*h_ode  for one (sample, group of the 2*hidden gate channels)
__global__ __launch_bounds__(256) void gn_gates_bwd_kernel(const float* __restrict__ gates_raw, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ gz_pre,
                                                           const float* __restrict__ g_rh, const float* __restrict__ h_ode,
                                                           float* __restrict__ gh_ode, float* __restrict__ g_gates_raw,
                                                           float* __restrict__ dgamma_part, float* __restrict__ dbeta_part,
                                                           int hid_groups) {
  __shared__ float sh[4];
  __shared__ float shc[256];
  const int g = blockIdx.x, b = blockIdx.y;
  f32x4 xh[8], gy[8];
  load_group(gates_raw, b, 2 * hid_groups, g, xh);
  const float rstd = normalise(xh, sh);
  const bool is_z = g < hid_groups;
  if (is_z) {
    load_group(gz_pre, b, hid_groups, g, gy);
  } else {
    const int gh_i = g - hid_groups;
    f32x4 hh[8], acc[8];
    load_group(g_rh, b, hid_groups, gh_i, gy);
    load_group(h_ode, b, hid_groups, gh_i, hh);
    load_group(gh_ode, b, hid_groups, gh_i, acc);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const f32x4 ga = *(const f32x4*)(gamma + g * 32 + q * 4), be = *(const f32x4*)(beta + g * 32 + q * 4);
      const f32x4 n = xh[q] * ga + be;
      const f32x4 r = sigmoid4(n);
      acc[q] += gy[q] * r;                       // rh = r*h_ode: path to h_ode
      gy[q] = gy[q] * hh[q] * r * (1.0f - r);    // path to the r pre-activation
    }
    store_group(gh_ode, b, hid_groups, gh_i, acc);
  }
  const int G2 = 2 * hid_groups * 32;
  gn_backward(gy, xh, gamma, g, rstd, dgamma_part + (size_t)b * G2, dbeta_part + (size_t)b * G2, sh, shc);
  store_group(g_gates_raw, b, 2 * hid_groups, g, gy);
}

// (grad_mean, grad_std) NCHW + sign of the head's std half -> gradient of the head output (B, 2*out_ch) Q4
__global__ __launch_bounds__(256) void merge_mean_std_grad_kernel(const float* __restrict__ gmean, const float* __restrict__ gstd,
                                                                  const float* __restrict__ head_out, float* __restrict__ dst,
                                                                  int total, int out_quads) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int p = idx & 255, bq = idx >> 8, q = bq % (2 * out_quads), b = bq / (2 * out_quads);
  f32x4 v;
  if (q < out_quads) {
    const float* s = gmean + ((size_t)b * out_quads + q) * 4 * kPix + p;
    v = {s[0], s[kPix], s[2 * kPix], s[3 * kPix]};
  } else {
    const float* s = gstd + ((size_t)b * out_quads + (q - out_quads)) * 4 * kPix + p;
    const f32x4 o = *(const f32x4*)(head_out + (size_t)idx * 4);
    v = {s[0], s[kPix], s[2 * kPix], s[3 * kPix]};
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = o[c] > 0.0f ? v[c] : (o[c] < 0.0f ? -v[c] : 0.0f);  // d|x|/dx, 0 at 0 as torch
  }
  *(f32x4*)(dst + (size_t)idx * 4) = v;
}

// out[c] = sum_k part[k][c] in a fixed order: one workgroup per column, strided partial sums + a fixed LDS tree
__global__ __launch_bounds__(256) void reduce_rows_kernel(const float* __restrict__ part, int n_rows, int n_cols,
                                                          float* __restrict__ out) {
  __shared__ float sh[256];
  const int c = blockIdx.x;
  float s = 0.0f;
  for (int k = threadIdx.x; k < n_rows; k += 256) s += part[(size_t)k * n_cols + c];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[c] = sh[0];
}

// gh (Q4) += grad_latent[:, slot] (NCHW slice of a (B,T,C,16,16) tensor): the gradient that arrives through latent_ys
__global__ __launch_bounds__(256) void add_nchw_slice_to_q4_kernel(const float* __restrict__ src, long long batch_stride,
                                                                   float* __restrict__ dst, int total, int quads) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int p = idx & 255, bq = idx >> 8, b = bq / quads, q = bq - b * quads;
  const float* s = src + (size_t)b * batch_stride + (size_t)q * 4 * kPix + p;
  f32x4* d = (f32x4*)(dst + (size_t)idx * 4);
  *d += f32x4{s[0], s[kPix], s[2 * kPix], s[3 * kPix]};
}

int conv_bwd(const float* src, int cin, int cout, int ks, const float* wt, const void* w_bf16, const float* w_wino, int combine,
             const BwdArgs* bw, float* dst, int batch, hipStream_t stream) {
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.src1 = src;
  a.q1 = a.qin = cin / 4;
  a.qout = cout / 4;
  a.w_packed = wt;
  a.w_bf16 = w_bf16;
  a.w_wino = w_bf16 ? nullptr : w_wino;
  a.batch = batch;
  a.combine = combine;
  if (bw) a.bwd = *bw;
  a.dst = dst;
  return launch_conv(a, ks, stream);
}

int cell_backward_step(const odehip_convgru_cell* c, const CellDgradW& w, const CellBwdStep& s, const BwdArgs& frame_tgt,
                       const BwdArgs& state_tgt, int batch, hipStream_t stream) {
  const int H = c->hidden, I = c->input, ks = c->ks, HG = H / 32;
  const bool plain = cell_is_plain(c);  // no GroupNorm: the pointwise kernels of convgru_plain.hip, no affine partials
  auto dgrad = [&](const float* src, int cin, int cout, int j, const BwdArgs* bw, float* dst) {
    return conv_bwd(src, cin, cout, ks, w.packed[j], w.bf16[j], w.wino[j], bw ? 3 : 0, bw, dst, batch, stream);
  };
  int rc;
  if (plain)  // writes the update half of g_gates as well: gz_pre stays unused
    launch_plain_update_bwd(s.cand_raw, s.gh, s.z, s.h_prev, s.g_cand, s.g_gates, s.gh_prev, H, batch, s.mask_b, stream);
  else if (s.mask_b)
    hipLaunchKernelGGL(gn_update_bwd_kernel<true>, dim3(HG, batch), dim3(256), 0, stream, s.cand_raw, c->gn_can_w, c->gn_can_b, s.gh, s.z,
                       s.h_prev, s.g_cand, s.gz_pre, s.gh_prev, s.pgc_w, s.pgc_b, HG, s.mask_b);
  else
    hipLaunchKernelGGL(gn_update_bwd_kernel<false>, dim3(HG, batch), dim3(256), 0, stream, s.cand_raw, c->gn_can_w, c->gn_can_b, s.gh, s.z,
                       s.h_prev, s.g_cand, s.gz_pre, s.gh_prev, s.pgc_w, s.pgc_b, HG, nullptr);
  if (s.has_x && (rc = dgrad(s.g_cand, H, I, 2, nullptr, s.gx_c)) != ODEHIP_OK) return rc;
  if (s.has_h) {
    if ((rc = dgrad(s.g_cand, H, H, 3, nullptr, s.g_rh)) != ODEHIP_OK) return rc;
  } else {
    ODEHIP_CHECK_HIP(hipMemsetAsync(s.g_rh, 0, (size_t)batch * H * kPix * 4, stream));  // r * 0: nothing arrives at r, and no state lies further back
  }
  if (plain)
    launch_plain_gates_bwd(s.gates_raw, s.g_rh, s.h_prev, s.gh_prev, s.g_gates, H, batch, s.mask_b, stream);
  else
    hipLaunchKernelGGL(gn_gates_bwd_kernel, dim3(2 * HG, batch), dim3(256), 0, stream, s.gates_raw, c->gn_gates_w, c->gn_gates_b, s.gz_pre,
                       s.g_rh, s.h_prev, s.gh_prev, s.g_gates, s.pgg_w, s.pgg_b, HG);
  if (s.has_x && (rc = dgrad(s.g_gates, 2 * H, I, 0, &frame_tgt, nullptr)) != ODEHIP_OK) return rc;
  if (s.has_h && (rc = dgrad(s.g_gates, 2 * H, H, 1, &state_tgt, nullptr)) != ODEHIP_OK) return rc;
  return ODEHIP_OK;
}

void reduce_gn_partials(const float* pgg, const float* pgc, int rows, int hidden, float* gn_gates_w, float* gn_gates_b, float* gn_can_w,
                        float* gn_can_b, hipStream_t stream) {
  const int H = hidden;
  hipLaunchKernelGGL(reduce_rows_kernel, dim3(2 * H), dim3(256), 0, stream, pgg, rows, 2 * H, gn_gates_w);
  hipLaunchKernelGGL(reduce_rows_kernel, dim3(2 * H), dim3(256), 0, stream, pgg + (size_t)rows * 2 * H, rows, 2 * H, gn_gates_b);
  hipLaunchKernelGGL(reduce_rows_kernel, dim3(H), dim3(256), 0, stream, pgc, rows, H, gn_can_w);
  hipLaunchKernelGGL(reduce_rows_kernel, dim3(H), dim3(256), 0, stream, pgc + (size_t)rows * H, rows, H, gn_can_b);
}

}  // namespace odehip

using namespace odehip;

extern "C" size_t odehip_encoder_train_workspace_bytes(const odehip_encoder* e, int n_frames, int batch) {
  if (!e || n_frames <= 0 || batch <= 0 || e->f_enc.n_convs < 1) return 0;
  return EncLayout(e, n_frames, batch, true).total;
}

extern "C" int odehip_odeconvgru_encode_train(const odehip_encoder* e, const float* inputs_nchw, const double* t_host, int n_frames,
                                              int batch, int run_backwards, float* mean_nchw, float* std_nchw, float* latent_nchw,
                                              void* workspace, size_t workspace_bytes, void* stream_) {
  return odehip_odeconvgru_encode_train_masked(e, inputs_nchw, t_host, n_frames, batch, run_backwards, mean_nchw, std_nchw, latent_nchw,
                                               workspace, workspace_bytes, stream_, nullptr);
}

// mask_tb: (T, B) on the device, row i = the observation mask of FRAME i, or null = all observed.  Nothing of it is kept in the
// workspace: the backward call is handed the same pointer.
extern "C" int odehip_odeconvgru_encode_train_masked(const odehip_encoder* e, const float* inputs_nchw, const double* t_host, int n_frames,
                                                     int batch, int run_backwards, float* mean_nchw, float* std_nchw, float* latent_nchw,
                                                     void* workspace, size_t workspace_bytes, void* stream_, const float* mask_tb) {
  return odehip_odeconvgru_encode_train_steps(e, inputs_nchw, t_host, n_frames, batch, run_backwards, mean_nchw, std_nchw, latent_nchw,
                                              workspace, workspace_bytes, stream_, mask_tb, nullptr, nullptr);
}

// step_observed_host: T bytes on the host indexed by frame (0 = no sample observed it: the step keeps the state in front of the Euler
// step and the dynamics' hidden activations, nothing of the cell), or null; the backward call is given the same bytes.
extern "C" int odehip_odeconvgru_encode_train_steps(const odehip_encoder* e, const float* inputs_nchw, const double* t_host, int n_frames,
                                                    int batch, int run_backwards, float* mean_nchw, float* std_nchw, float* latent_nchw,
                                                    void* workspace, size_t workspace_bytes, void* stream_, const float* mask_tb,
                                                    const unsigned char* step_observed_host, int* cell_steps_run) {
  int rc = check_encoder(e, true, "odeconvgru_encode_train");
  if (rc != ODEHIP_OK) return rc;
  ODEHIP_REQUIRE(inputs_nchw && t_host && mean_nchw && std_nchw && workspace, "odeconvgru_encode_train: null pointer");
  ODEHIP_REQUIRE(n_frames >= 1 && n_frames <= 64 && batch > 0, "odeconvgru_encode_train: bad sizes (frames %d, batch %d)", n_frames, batch);
  const EncLayout L(e, n_frames, batch, true);
  ODEHIP_REQUIRE(workspace_bytes >= L.total, "odeconvgru_encode_train: workspace too small");
  return encoder_forward(e, L, workspace, inputs_nchw, t_host, run_backwards, mean_nchw, std_nchw, latent_nchw, mask_tb, step_observed_host,
                         cell_steps_run, (hipStream_t)stream_);
}

extern "C" int odehip_odeconvgru_encode_backward(const odehip_encoder* e, const odehip_encoder_bwd* eb, const double* t_host,
                                                 int n_frames, int batch, int run_backwards, const float* grad_mean_nchw,
                                                 const float* grad_std_nchw, const float* grad_latent_nchw, float* grad_inputs_nchw,
                                                 const odehip_encoder_grads* gr, void* workspace, size_t workspace_bytes, void* stream_) {
  return odehip_odeconvgru_encode_backward_masked(e, eb, t_host, n_frames, batch, run_backwards, grad_mean_nchw, grad_std_nchw,
                                                  grad_latent_nchw, grad_inputs_nchw, gr, workspace, workspace_bytes, stream_, nullptr);
}

// mask_tb: the pointer the forward call (odehip_odeconvgru_encode_train_masked) was given.  An unobserved (frame, sample) feeds the
// cell's chain exact zeros, so with finite frames its grad_inputs slice and its share of every parameter gradient are exact zeros.
// A NON-FINITE unobserved frame is contained by the forward only: the weight-gradient products multiply it by those zeros.
extern "C" int odehip_odeconvgru_encode_backward_masked(const odehip_encoder* e, const odehip_encoder_bwd* eb, const double* t_host,
                                                        int n_frames, int batch, int run_backwards, const float* grad_mean_nchw,
                                                        const float* grad_std_nchw, const float* grad_latent_nchw,
                                                        float* grad_inputs_nchw, const odehip_encoder_grads* gr, void* workspace,
                                                        size_t workspace_bytes, void* stream_, const float* mask_tb) {
  return odehip_odeconvgru_encode_backward_steps(e, eb, t_host, n_frames, batch, run_backwards, grad_mean_nchw, grad_std_nchw,
                                                 grad_latent_nchw, grad_inputs_nchw, gr, workspace, workspace_bytes, stream_, mask_tb, nullptr,
                                                 nullptr);
}

// step_observed_host: the bytes the forward call (odehip_odeconvgru_encode_train_steps) was given, or null.  A step whose frame nobody
// observed contributes nothing to the cell's gradients and reads nothing of its frame: no cell kernel runs for it.
extern "C" int odehip_odeconvgru_encode_backward_steps(const odehip_encoder* e, const odehip_encoder_bwd* eb, const double* t_host,
                                                       int n_frames, int batch, int run_backwards, const float* grad_mean_nchw,
                                                       const float* grad_std_nchw, const float* grad_latent_nchw,
                                                       float* grad_inputs_nchw, const odehip_encoder_grads* gr, void* workspace,
                                                       size_t workspace_bytes, void* stream_, const float* mask_tb,
                                                       const unsigned char* step_observed_host, int* cell_steps_run) {
  int rc = check_encoder(e, true, "odeconvgru_encode_backward");
  if (rc != ODEHIP_OK) return rc;
  ODEHIP_REQUIRE(eb && t_host && grad_mean_nchw && grad_std_nchw && grad_inputs_nchw && gr && workspace,
                 "odeconvgru_encode_backward: null pointer");
  ODEHIP_REQUIRE(eb->w_gates_dx && eb->w_gates_dh && eb->w_can_dx && eb->w_can_dh && eb->w_head0_t && eb->w_head1_t,
                 "odeconvgru_encode_backward: null transposed weight");
  ODEHIP_REQUIRE(n_frames >= 1 && n_frames <= 64 && batch > 0, "odeconvgru_encode_backward: bad sizes");
  const EncLayout L(e, n_frames, batch, true);
  ODEHIP_REQUIRE(workspace_bytes >= L.total, "odeconvgru_encode_backward: workspace too small");
  hipStream_t stream = (hipStream_t)stream_;
  void* ws = workspace;
  const int C = L.C, NH = L.NH, NL = e->f_enc.n_convs, T = n_frames, HH = e->head_hidden, OUT2 = 2 * e->out_ch, ks = e->cell.ks;
  const bool plain = cell_is_plain(&e->cell);  // no GroupNorm: no affine gradients
  ODEHIP_REQUIRE(plain || (gr->gn_gates_w && gr->gn_gates_b && gr->gn_can_w && gr->gn_can_b),
                 "odeconvgru_encode_backward: null GroupNorm gradient output");
  float* dts = L.p(ws, L.off_dts);
  // steps (in visiting order) whose cell ran; the gradient at the state behind step idx lives in one of two buffers, or, if that
  // step's cell did not run, in its seed slot (fh >= hs bytes): it is the seed of the Euler step's adjoint as it stands
  bool ran[64];
  int n_run = 0;
  for (int idx = 0; idx < T; ++idx) n_run += (ran[idx] = step_is_observed(step_observed_host, visited_frame(T, idx, run_backwards)));
  auto gh_home = [&](int idx) { return ran[idx] ? L.p(ws, L.off_gh + (size_t)((T - 1 - idx) & 1) * L.hs) : L.gp(ws, idx, NH); };
  float* gh = gh_home(T - 1);
  float* pgg = L.p(ws, L.off_pgg);  // [2][T*B][2C]: dgamma then dbeta partials of the gates GroupNorm
  float* pgc = L.p(ws, L.off_pgc);  // [2][T*B][C]
  const size_t pgg_half = (size_t)T * batch * 2 * C, pgc_half = (size_t)T * batch * C;
  if (!plain && n_run < T)  // the partial rows of the steps without a cell: exact zeros, as gn_update_bwd_kernel<true> stores for m == 0
    ODEHIP_CHECK_HIP(hipMemsetAsync(pgg, 0, L.off_tab - L.off_pgg, stream));
  const CellDgradW dw = dgrad_images(eb);

  // ---- head: |std|, 1x1 -> ReLU -> 1x1
  {
    const int total = batch * (OUT2 / 4) * kPix;
    hipLaunchKernelGGL(merge_mean_std_grad_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, grad_mean_nchw, grad_std_nchw,
                       L.p(ws, L.off_headout), L.p(ws, L.off_gheadout), total, e->out_ch / 4);
    BwdArgs w;
    memset(&w, 0, sizeof(w));
    w.mask_src = L.p(ws, L.off_headhid);
    w.sc_c = 1.0f;
    rc = conv_bwd(L.p(ws, L.off_gheadout), OUT2, HH, 1, eb->w_head1_t, nullptr, nullptr, 2, &w, L.p(ws, L.off_gheadhid), batch, stream);
    if (rc != ODEHIP_OK) return rc;
    rc = conv_bwd(L.p(ws, L.off_gheadhid), HH, C, 1, eb->w_head0_t, nullptr, nullptr, 0, nullptr, gh, batch, stream);
    if (rc != ODEHIP_OK) return rc;
  }

  // ---- frames, last processed first
  CatStep cat[64];  // the steps whose cell ran, in visiting order: the cell's weight-gradient tables list these
  for (int idx = 0, k = 0; idx < T; ++idx)
    if (ran[idx])
      cat[k++] = CatStep{L.per(ws, L.off_ggates, idx, 2 * L.hs), L.per(ws, L.off_gcand, idx, L.hs), L.frame(ws, visited_frame(T, idx, run_backwards)),
                         L.per(ws, L.off_hode, idx, L.hs), L.per(ws, L.off_rh, idx, L.hs)};
  for (int idx = T - 1; idx >= 0; --idx) {
    const int i = visited_frame(T, idx, run_backwards);
    if (grad_latent_nchw) {  // gh = gradient w.r.t. the state after the idx-th visited frame: + what arrives through latent_ys[:, idx]
      const int total = batch * (C / 4) * kPix;
      hipLaunchKernelGGL(add_nchw_slice_to_q4_kernel, dim3((total + 255) / 256), dim3(256), 0, stream,
                         grad_latent_nchw + (size_t)idx * C * kPix, (long long)T * C * kPix, gh, total, C / 4);
    }
    float* gh_next = idx > 0 ? gh_home(idx - 1) : L.p(ws, L.off_gh + (size_t)(T & 1) * L.hs);  // idx == 0: nobody reads it
    if (ran[idx]) {
      CellBwdStep s;
      s.cand_raw = L.per(ws, L.off_cand, idx, L.hs);
      s.z = L.per(ws, L.off_z, idx, L.hs);
      s.gates_raw = L.per(ws, L.off_gates, idx, 2 * L.hs);
      s.h_prev = L.per(ws, L.off_hode, idx, L.hs);  // the cell was given the Euler-advanced state
      s.gh = gh;
      s.g_cand = L.per(ws, L.off_gcand, idx, L.hs);
      s.g_gates = L.per(ws, L.off_ggates, idx, 2 * L.hs);
      s.gz_pre = L.p(ws, L.off_gzpre);
      s.gh_prev = L.p(ws, L.off_ghode);
      s.gx_c = L.p(ws, L.off_gxc);
      s.g_rh = L.p(ws, L.off_grh);
      s.pgc_w = pgc + (size_t)idx * batch * C;
      s.pgc_b = s.pgc_w + pgc_half;
      s.pgg_w = pgg + (size_t)idx * batch * 2 * C;
      s.pgg_b = s.pgg_w + pgg_half;
      s.mask_b = mask_tb ? mask_tb + (size_t)i * batch : nullptr;
      s.has_x = s.has_h = true;
      // gradient of observed frame i; seed of the encoder-dynamics chain = total gradient of h_ode
      rc = cell_backward_step(&e->cell, dw, s, bwd_target(L.per(ws, L.off_gx, i, L.hs), s.gx_c), bwd_target(L.gp(ws, idx, NH), s.gh_prev),
                              batch, stream);
      if (rc != ODEHIP_OK) return rc;
    } else {  // gh already sits in the seed slot; the frame's gradient is exactly zero
      ODEHIP_CHECK_HIP(hipMemsetAsync(L.per(ws, L.off_gx, i, L.hs), 0, (size_t)batch * C * kPix * 4, stream));
    }
    // h_ode = h + dt f(h):  gh = seed + dt J_f(h)^T seed
    {
      float* gpv[ODEHIP_MAX_LAYERS + 1];
      const float* hv[ODEHIP_MAX_LAYERS];
      for (int l = 0; l < L.NG; ++l) gpv[l] = L.gp(ws, idx, l);
      for (int l = 0; l + 1 < NL; ++l) hv[l] = L.hidden(ws, idx, l);
      ConvArgs a;
      memset(&a, 0, sizeof(a));
      a.combine = 3;
      a.bwd.n_targets = 1;
      a.bwd.h_ptr = dts + idx;
      a.bwd.tgt[0].out = gh_next;
      a.bwd.tgt[0].srcA = L.gp(ws, idx, NH);
      a.bwd.tgt[0].a_c = 1.0f;
      a.bwd.tgt[0].g_h = 1.0f;
      if ((rc = enqueue_dgrad_chain(&e->f_enc, &eb->f_dgrad, batch, gpv, hv, a, stream)) != ODEHIP_OK) return rc;
    }
    gh = gh_next;
  }
  rc = odehip_q4_to_nchw(L.p(ws, L.off_gx), grad_inputs_nchw, T * batch, C, stream);
  if (rc != ODEHIP_OK) return rc;

  // ---- weight gradients: one launch per (layer, 64x64 tile) over all frames
  // All tables (NL dynamics layers, 2 x 2 ConvGRU halves, 2 head layers; T entries each) are built first and go up in ONE
  // asynchronous copy (a fill launch per 256 bytes before: 21 launches of 5 us per backward pass).
  WgradPair* const table0 = (WgradPair*)L.p(ws, L.off_tab);
  float* slabs = L.p(ws, L.off_slab);
  std::vector<WgradPair> host((size_t)(NL + 6) * T);
  memset(host.data(), 0, host.size() * sizeof(WgradPair));
  for (int l = 0; l < NL; ++l)   // encoder dynamics (3x3), weight of frame idx = its Euler dt
    for (int idx = 0; idx < T; ++idx) {
      WgradPair& h = host[(size_t)l * T + idx];
      h.g = L.gp(ws, idx, wgrad_slot(&e->f_enc, l));
      h.a = l == 0 ? L.hstate(ws, idx) : L.hidden(ws, idx, l - 1);
      h.scale = frame_dt(t_host, T, idx, run_backwards);
    }
  cat_wgrad_entries(&host[(size_t)NL * T], T, cat, n_run);   // ConvGRU convs on cat(x, state): the steps whose cell ran
  {   // head 1x1 convs (one entry each)
    WgradPair& h1 = host[(size_t)(NL + 4) * T];
    h1.g = L.p(ws, L.off_gheadout);
    h1.a = L.p(ws, L.off_headhid);
    h1.scale = 1.0f;
    WgradPair& h0 = host[(size_t)(NL + 5) * T];
    h0.g = L.p(ws, L.off_gheadhid);
    h0.a = L.hstate(ws, T);
    h0.scale = 1.0f;
  }
  if ((rc = staged_upload(table0, host.data(), host.size() * sizeof(WgradPair), stream)) != ODEHIP_OK) return rc;
  for (int l = 0; l < NL; ++l) {
    // (fp32: 256 / batch workgroups per sample share the frames -- a batch of 4 with esplit 4 kept 240 CUs idle)
    rc = launch_wgrad(table0 + (size_t)l * T, T, batch, (&e->f_enc)->w_bf16[l] ? 4 : wgrad_esplit(batch, T), slabs, gr->f_w[l], gr->f_b[l],
                      e->f_enc.channels[l + 1], e->f_enc.channels[l], stream, (&e->f_enc)->w_bf16[l] != nullptr);
    if (rc != ODEHIP_OK) return rc;
  }
  for (int j = 0; j < 2; ++j) {   // gates, can: the two halves of the input are separate tensors
    const int g_ch = j == 0 ? 2 * C : C;
    float* jw = j == 0 ? gr->w_gates : gr->w_can;
    float* jb = j == 0 ? gr->b_gates : gr->b_can;
    if (n_run == 0) {  // no step ran the cell: no launch, the gradients are exact zeros
      ODEHIP_CHECK_HIP(hipMemsetAsync(jw, 0, (size_t)g_ch * 2 * C * ks * ks * 4, stream));
      ODEHIP_CHECK_HIP(hipMemsetAsync(jb, 0, (size_t)g_ch * 4, stream));
      continue;
    }
    for (int half = 0; half < 2; ++half) {
      const WgradPair* const table = table0 + (size_t)(NL + 2 * j + half) * T;
      const bool bf16 = ks == 5 && e->cell.w_gates_bf16;  // bf16 compute mode: operands rounded to bf16, fp32 accumulation
      rc = launch_wgrad_layer(table, n_run, batch, bf16 ? 4 : wgrad_esplit(batch, n_run), slabs, jw, jb, ks, g_ch, C, 2 * C, half * C, bf16,
                              half == 0, stream);
      if (rc != ODEHIP_OK) return rc;
    }
  }
  // head 1x1 convs
  rc = launch_wgrad_layer(table0 + (size_t)(NL + 4) * T, 1, batch, 4, slabs, gr->w_head1, gr->b_head1, 1, OUT2, HH, HH, 0, false, true, stream);
  if (rc != ODEHIP_OK) return rc;
  rc = launch_wgrad_layer(table0 + (size_t)(NL + 5) * T, 1, batch, 4, slabs, gr->w_head0, gr->b_head0, 1, HH, C, C, 0, false, true, stream);
  if (rc != ODEHIP_OK) return rc;
  if (!plain) reduce_gn_partials(pgg, pgc, T * batch, C, gr->gn_gates_w, gr->gn_gates_b, gr->gn_can_w, gr->gn_can_b, stream);
  ODEHIP_CHECK_HIP(hipGetLastError());
  if (cell_steps_run) *cell_steps_run = n_run;
  return ODEHIP_OK;
}

// ---- one ConvGRU step: backward of ConvGRUCell.forward(input_tensor, h_cur, seq_len = 1)   (modules/ConvGRUCell.py:55-86) ----
// Stateless: the step is recomputed from (x, h) inside the call (two convs), then reversed.
namespace odehip {
// Workspace of one ConvGRU-step backward; offsets are computed in ONE place for the size query and the call.
struct CellBwdLayout {
  size_t x, gx_c, gx_out, h, gates, z, rh, cand, hn, ghn, g_cand, g_gates, gz_pre, gh_ode, g_rh, gh, pg, table, slabs, total;
  CellBwdLayout(const odehip_convgru_cell* c, int batch) {
    const size_t hs = (size_t)batch * c->hidden * kPix * 4, xs = (size_t)batch * c->input * kPix * 4;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += al256(bytes); return r; };
    x = take(xs); gx_c = take(xs); gx_out = take(xs);
    h = take(hs); gates = take(2 * hs); z = take(hs); rh = take(hs); cand = take(hs); hn = take(hs); ghn = take(hs);
    g_cand = take(hs); g_gates = take(2 * hs); gz_pre = take(hs); gh_ode = take(hs); g_rh = take(hs); gh = take(hs);
    pg = take((size_t)6 * batch * c->hidden * 4);  // [dgamma_g | dbeta_g] (2H each) then [dgamma_c | dbeta_c] (H each), per sample
    table = take(4 * sizeof(WgradPair));           // the four cat-conv entries (a 256-byte slot)
    slabs = take(wgrad_slab_bytes(batch));
    total = o;
  }
};
}  // namespace odehip

extern "C" size_t odehip_convgru_cell_backward_workspace_bytes(const odehip_convgru_cell* c, int batch) {
  if (!c || batch <= 0 || c->hidden <= 0 || c->input <= 0) return 0;
  return CellBwdLayout(c, batch).total;
}

extern "C" int odehip_convgru_cell_backward(const odehip_convgru_cell* c, const odehip_convgru_cell_bwd* cb, const float* x_nchw,
                                            const float* h_nchw, const float* grad_h_next_nchw, float* grad_x_nchw,
                                            float* grad_h_nchw, const odehip_convgru_cell_grads* gr, int batch, void* workspace,
                                            size_t workspace_bytes, void* stream_) {
  int rc = check_cell(c);
  if (rc != ODEHIP_OK) return rc;
  ODEHIP_REQUIRE(cb && x_nchw && h_nchw && grad_h_next_nchw && grad_x_nchw && grad_h_nchw && gr && workspace && batch > 0,
                 "convgru_cell_backward: bad argument");
  ODEHIP_REQUIRE(cb->w_gates_dx && cb->w_gates_dh && cb->w_can_dx && cb->w_can_dh, "convgru_cell_backward: null transposed weight");
  ODEHIP_REQUIRE(c->input % 64 == 0 && c->hidden % 64 == 0, "convgru_cell_backward: input_dim and hidden_dim must be multiples of 64");
  ODEHIP_REQUIRE(workspace_bytes >= odehip_convgru_cell_backward_workspace_bytes(c, batch), "convgru_cell_backward: workspace too small");
  hipStream_t stream = (hipStream_t)stream_;
  const int H = c->hidden, I = c->input, ks = c->ks;
  const bool plain = cell_is_plain(c);
  ODEHIP_REQUIRE(plain || (gr->gn_gates_w && gr->gn_gates_b && gr->gn_can_w && gr->gn_can_b),
                 "convgru_cell_backward: null GroupNorm gradient output");
  const CellBwdLayout L(c, batch);
  auto at = [&](size_t off) { return (float*)((char*)workspace + off); };
  float *x = at(L.x), *gx_out = at(L.gx_out), *h = at(L.h), *rh = at(L.rh), *hn = at(L.hn), *ghn = at(L.ghn), *gh = at(L.gh), *pg = at(L.pg),
        *slabs = at(L.slabs);
  WgradPair* table = (WgradPair*)at(L.table);
  float* pgg = pg;
  float* pgc = pg + (size_t)2 * batch * 2 * H;

  if ((rc = odehip_nchw_to_q4(x_nchw, x, batch, I, stream)) != ODEHIP_OK) return rc;
  if ((rc = odehip_nchw_to_q4(h_nchw, h, batch, H, stream)) != ODEHIP_OK) return rc;
  if ((rc = odehip_nchw_to_q4(grad_h_next_nchw, ghn, batch, H, stream)) != ODEHIP_OK) return rc;
  CellBwdStep s;
  s.cand_raw = at(L.cand); s.z = at(L.z); s.gates_raw = at(L.gates); s.h_prev = h; s.gh = ghn;
  s.g_cand = at(L.g_cand); s.g_gates = at(L.g_gates);
  s.gz_pre = at(L.gz_pre); s.gh_prev = at(L.gh_ode); s.gx_c = at(L.gx_c); s.g_rh = at(L.g_rh);
  s.pgc_w = pgc; s.pgc_b = pgc + (size_t)batch * H; s.pgg_w = pgg; s.pgg_b = pgg + (size_t)batch * 2 * H;
  s.mask_b = nullptr;
  s.has_x = s.has_h = true;
  if ((rc = cell_forward_step(c, nullptr, x, h, hn, nullptr, 0, batch, at(L.gates), at(L.z), rh, at(L.cand), nullptr, stream)) != ODEHIP_OK) return rc;
  // gradient of x = can-conv part + gates-conv part; gradient of h likewise
  if ((rc = cell_backward_step(c, dgrad_images(cb), s, bwd_target(gx_out, s.gx_c), bwd_target(gh, s.gh_prev), batch, stream)) != ODEHIP_OK) return rc;
  if ((rc = odehip_q4_to_nchw(gx_out, grad_x_nchw, batch, I, stream)) != ODEHIP_OK) return rc;
  if ((rc = odehip_q4_to_nchw(gh, grad_h_nchw, batch, H, stream)) != ODEHIP_OK) return rc;

  WgradPair host[4];
  memset(host, 0, sizeof(host));
  const CatStep step = {s.g_gates, s.g_cand, x, h, rh};
  cat_wgrad_entries(host, 1, &step, 1);
  if ((rc = upload_bytes(table, host, sizeof(host), stream)) != ODEHIP_OK) return rc;
  for (int j = 0; j < 2; ++j)
    for (int half = 0; half < 2; ++half) {
      rc = launch_wgrad_layer(table + 2 * j + half, 1, batch, 4, slabs, j == 0 ? gr->w_gates : gr->w_can, j == 0 ? gr->b_gates : gr->b_can, ks,
                              j == 0 ? 2 * H : H, half == 0 ? I : H, I + H, half * I, ks == 5 && c->w_gates_bf16, half == 0, stream);
      if (rc != ODEHIP_OK) return rc;
    }
  if (!plain) reduce_gn_partials(pgg, pgc, batch, H, gr->gn_gates_w, gr->gn_gates_b, gr->gn_can_w, gr->gn_can_b, stream);
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}
