// convgru.hip -- the ODE-ConvGRU encoder on the device (gfx950).
//
// Restates /root/reference/modules/ODEConvGRUCell.py:32-78 (reverse-time loop: explicit-Euler step of the encoder
// dynamics, then a ConvGRU update with the encoded frame; 1x1 -> ReLU -> 1x1 head; split; |std|) and
// /root/reference/modules/ConvGRUCell.py:72-82 (z,r = sigmoid(GN(conv5x5(cat(x,h)))), z FIRST; cand =
// tanh(GN(conv5x5(cat(x, r*h)))); h' = (1-z) h + z cand).  GroupNorm: 32 channels per group (2*hid//32 and hid//32
// groups, ConvGRUCell.py:44,50), eps 1e-5, affine.
//
// Launch sequence per observed frame (all enqueue-only, no host sync -- the reference's three NaN/"first point"
// host checks per iteration, ODEConvGRUCell.py:56-64, are not reproduced):
//   5 x conv3x3 (f_enc, Euler combine fused: h_ode = h + dt*f(h))            conv_q4.hip
//   conv5x5(cat(x, h_ode)) -> gates_raw                                      conv_ring_kernel (two sources, no copy)
//   gn_gates_kernel: GroupNorm + sigmoid; writes z and r*h_ode                one workgroup per (sample, 32-ch group)
//   conv5x5(cat(x, r*h_ode)) -> cand_raw
//   gn_update_kernel: GroupNorm + tanh + h' = (1-z) h_ode + z cand
// Observation mask (odehip_odeconvgru_encode_masked; upstream Vid-ODE models/base_conv_gru.py:66-70, which the reference's cell takes
// and forgets): the state a step leaves is m h' + (1-m) h_ode with m = mask[frame, sample], decided inside gn_update_kernel<kUpdMasked>
// per workgroup.  The convolutions above run for every sample either way; without a mask the launches are gn_update_kernel<kUpdPlain>.
// Host step hint (odehip_odeconvgru_encode_steps): a step whose frame NO sample observed launches none of the four cell kernels -- the
// Euler combine writes h_ode straight into the next state buffer (the bits the update kernels copy for m == 0) and a wanted latent
// slot is filled by state_to_latent_kernel.
// In the Q4 layout a 32-channel group of one sample is 32 KiB contiguous, so a workgroup holds its whole group in
// registers (32 floats per thread): statistics are exact two-pass fp32, one HBM read, one write.
// A cell without GroupNorm (all four gn_* pointers NULL: upstream Vid-ODE's cell, reset gate first) runs the same convolutions with
// the pointwise kernels of convgru_plain.hip in place of gn_gates_kernel / gn_update_kernel.
#include <string.h>

#include "convgru_cell.h"

namespace odehip {

// gates_raw: (B, 2*hid) Q4.  Groups [0, hid/32) are z, the rest r.  Writes z (B,hid) and, with a state, rh = r * h (B,hid).
// HAS_H = false (a zero state) is launched over the z groups alone and reads no h.
template <bool HAS_H>
__global__ __launch_bounds__(256) void gn_gates_kernel(const float* __restrict__ gates_raw, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const float* __restrict__ h,
                                                       float* __restrict__ z_out, float* __restrict__ rh_out, int hid_groups) {
  __shared__ float sh[4];
  const int g = blockIdx.x, b = blockIdx.y;
  f32x4 v[8];
  load_group(gates_raw, b, 2 * hid_groups, g, v);
  group_norm(v, gamma, beta, g, 1e-5f, sh);
  const bool is_z = !HAS_H || g < hid_groups;
  const int gh = is_z ? g : g - hid_groups;
  const size_t base = ((size_t)(b * hid_groups + gh) * 8) * kPix;
  f32x4* out = (f32x4*)(is_z ? z_out : rh_out) + base + threadIdx.x;
  const f32x4* hp = (const f32x4*)h + base + threadIdx.x;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    f32x4 s = sigmoid4(v[q]);
    if (HAS_H && !is_z) s *= hp[q * kPix];
    out[q * kPix] = s;
  }
}

// cand_raw: (B,hid) Q4.  h' = (1 - z) h + z tanh(GN(cand_raw)); optionally also written to an NCHW slot (latent_ys, h_seq).
// kUpdMasked: mask_b[b] = m, the observation mask of this step's frame for sample b (one scalar per workgroup, so the branches
// are uniform).  m == 1: h' as above, bit for bit what the unmasked instantiation writes; m == 0: h is copied and nothing the
// cell computed is read; otherwise m h' + (1 - m) h.  Only kUpdMasked reads mask_b.
template <UpdateMode kMode>
__global__ __launch_bounds__(256) void gn_update_kernel(const float* __restrict__ cand_raw, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const float* __restrict__ h,
                                                        const float* __restrict__ z, float* __restrict__ h_out,
                                                        float* __restrict__ h_out_nchw, long long nchw_batch_stride,
                                                        int hid_groups, const float* __restrict__ mask_b) {
  constexpr bool kMasked = kMode == kUpdMasked;
  __shared__ float sh[4];
  const int g = blockIdx.x, b = blockIdx.y;
  const float m = kMasked ? mask_b[b] : 1.0f;
  if (kMasked && m == 0.0f) {  // unobserved: the Euler-advanced state goes on unchanged
    const size_t base = ((size_t)(b * hid_groups + g) * 8) * kPix;
    const f32x4* hp = (const f32x4*)h + base + threadIdx.x;
    f32x4* op = (f32x4*)h_out + base + threadIdx.x;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const f32x4 o = hp[q * kPix];
      op[q * kPix] = o;
      if (h_out_nchw) {
        float* n = h_out_nchw + (size_t)b * nchw_batch_stride + (size_t)(g * 32 + q * 4) * kPix + threadIdx.x;
        n[0] = o.x; n[kPix] = o.y; n[2 * kPix] = o.z; n[3 * kPix] = o.w;
      }
    }
    return;
  }
  f32x4 v[8];
  load_group(cand_raw, b, hid_groups, g, v);
  group_norm(v, gamma, beta, g, 1e-5f, sh);
  const size_t base = ((size_t)(b * hid_groups + g) * 8) * kPix;
  const f32x4* hp = (const f32x4*)h + base + threadIdx.x;
  const f32x4* zp = (const f32x4*)z + base + threadIdx.x;
  f32x4* op = (f32x4*)h_out + base + threadIdx.x;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const f32x4 c = tanh4(v[q]);
    const f32x4 zz = zp[q * kPix];
    const f32x4 hh = hp[q * kPix];
    f32x4 o = (1.0f - zz) * hh + zz * c;
    if (kMasked && m != 1.0f) o = m * o + (1.0f - m) * hh;
    op[q * kPix] = o;
    if (h_out_nchw) {
      float* n = h_out_nchw + (size_t)b * nchw_batch_stride + (size_t)(g * 32 + q * 4) * kPix + threadIdx.x;
      n[0] = o.x; n[kPix] = o.y; n[2 * kPix] = o.z; n[3 * kPix] = o.w;
    }
  }
}

// The update of a step of a SEQUENCE (convgru_sequence.hip): the same arithmetic as gn_update_kernel<kUpdPlain>, kept as a kernel of
// its own.  Its NCHW slot (the step's slot of h_seq) always exists and is dense (sample b at + b * hid * 256), so it has neither the
// null test nor the 64-bit stride multiply, and HAS_H = false (a zero state: h' = z tanh(.)) reads no h.  Folded into
// gn_update_kernel, a rollout of 190 steps at B = 4 and the training step of the ConvGRU baseline measured about 1 % slower than with
// this kernel (profiles/convgru_refactor.json, "speed_ms_alternating_rounds.first_attempt"); the results were the same bits either way.
template <bool HAS_H>
__global__ __launch_bounds__(256) void seq_update_kernel(const float* __restrict__ cand_raw, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, const float* __restrict__ h,
                                                         const float* __restrict__ z, float* __restrict__ h_out,
                                                         float* __restrict__ h_seq_slot, int hid_groups) {
  __shared__ float sh[4];
  const int g = blockIdx.x, b = blockIdx.y;
  f32x4 v[8];
  load_group(cand_raw, b, hid_groups, g, v);
  group_norm(v, gamma, beta, g, 1e-5f, sh);
  const size_t base = ((size_t)(b * hid_groups + g) * 8) * kPix;
  const f32x4* zp = (const f32x4*)z + base + threadIdx.x;
  f32x4* op = (f32x4*)h_out + base + threadIdx.x;
  float* n = h_seq_slot + ((size_t)b * hid_groups + g) * 32 * kPix + threadIdx.x;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const f32x4 c = {tanhf(v[q].x), tanhf(v[q].y), tanhf(v[q].z), tanhf(v[q].w)};
    const f32x4 zz = zp[q * kPix];
    f32x4 o = zz * c;
    if (HAS_H) o = (1.0f - zz) * ((const f32x4*)h + base + threadIdx.x)[q * kPix] + o;
    op[q * kPix] = o;
    float* nq = n + (size_t)q * 4 * kPix;
    nq[0] = o.x; nq[kPix] = o.y; nq[2 * kPix] = o.z; nq[3 * kPix] = o.w;
  }
}

// Q4 state (B,hid) -> its NCHW latent slot, for a step whose cell did not run: grid (hid / 4, B), one f32x4 per thread, the indexing of
// the update kernels' epilogue (quad g * 8 + q of sample b, pixel threadIdx.x).
__global__ __launch_bounds__(256) void state_to_latent_kernel(const float* __restrict__ h, float* __restrict__ h_out_nchw,
                                                              long long nchw_batch_stride, int hid_quads) {
  const int q = blockIdx.x, b = blockIdx.y;
  const f32x4 o = ((const f32x4*)h)[((size_t)b * hid_quads + q) * kPix + threadIdx.x];
  float* n = h_out_nchw + (size_t)b * nchw_batch_stride + (size_t)(q * 4) * kPix + threadIdx.x;
  n[0] = o.x; n[kPix] = o.y; n[2 * kPix] = o.z; n[3 * kPix] = o.w;
}

// head output (B, 2*out_ch) Q4 -> mean (B,out_ch) NCHW, std = |.| (B,out_ch) NCHW   (ODEConvGRUCell.py:35-36)
__global__ __launch_bounds__(256) void split_mean_std_kernel(const float* __restrict__ src, float* __restrict__ mean,
                                                             float* __restrict__ stdv, int total, int out_quads) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int p = idx & 255, bq = idx >> 8, q = bq % (2 * out_quads), b = bq / (2 * out_quads);
  f32x4 v = *(const f32x4*)(src + (size_t)idx * 4);
  float* d;
  if (q < out_quads) {
    d = mean + ((size_t)b * out_quads + q) * 4 * kPix + p;
  } else {
    d = stdv + ((size_t)b * out_quads + (q - out_quads)) * 4 * kPix + p;
    v = {fabsf(v.x), fabsf(v.y), fabsf(v.z), fabsf(v.w)};
  }
  d[0] = v.x; d[kPix] = v.y; d[2 * kPix] = v.z; d[3 * kPix] = v.w;
}

struct U32Pack {
  unsigned v[64];
};
__global__ void fill_u32_kernel(unsigned* dst, U32Pack p, int n) {
  if ((int)threadIdx.x < n) dst[threadIdx.x] = p.v[threadIdx.x];
}
int upload_bytes(void* dst, const void* src, size_t bytes, hipStream_t stream) {
  const unsigned* s = (const unsigned*)src;
  const int n = (int)(bytes / 4);
  for (int o = 0; o < n; o += 64) {
    U32Pack p;
    const int m = n - o < 64 ? n - o : 64;
    memcpy(p.v, s + o, (size_t)m * 4);
    hipLaunchKernelGGL(fill_u32_kernel, dim3(1), dim3(64), 0, stream, (unsigned*)dst + o, p, m);
  }
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}

// direct: the steps of a sequence (convgru_sequence.hip) go straight to the F(2x2,5x5) / bf16 5x5 launcher of the ONE image they
// carry.  This stays a branch of its own and is not folded into launch_conv: the weight halves have no packed form (launch_conv
// demands one and falls back to it), and launch_conv also stamps the debug fields and feeds a trajectory recorder -- other arguments
// to the same kernel than a sequence has ever launched.
int conv_layer(const float* src1, const float* src2, int cin1, int cin, int cout, int ks, const float* wp, const float* bias, float* dst,
               int relu, int batch, hipStream_t stream, const void* w_bf16, const float* w_wino, bool direct) {
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.src1 = src1;
  a.src2 = src2;
  a.q1 = cin1 / 4;
  a.qin = cin / 4;
  a.qout = cout / 4;
  a.w_packed = wp;
  a.w_bf16 = w_bf16;
  a.w_wino = w_wino;
  a.bias = bias;
  a.dst = dst;
  a.batch = batch;
  a.act = relu ? kActRelu : kActNone;
  if (!direct) return launch_conv(a, ks, stream);
  const int rc = a.w_bf16 ? launch_bf16_5x5(a, stream) : launch_wino5(a, stream);
  ODEHIP_REQUIRE(rc != 1, "convgru_sequence: no 5x5 kernel serves %d -> %d channels", cin, cout);
  return rc;
}

int check_cell(const odehip_convgru_cell* c) {
  ODEHIP_REQUIRE(c, "convgru: null cell descriptor");
  ODEHIP_REQUIRE(c->hidden > 0 && c->hidden % 32 == 0, "convgru: hidden_dim must be a multiple of 32 (GroupNorm groups of 32; got %d)", c->hidden);
  ODEHIP_REQUIRE(c->input > 0 && c->input % 8 == 0, "convgru: input_dim must be a multiple of 8 (got %d)", c->input);
  ODEHIP_REQUIRE(c->ks == 5 || c->ks == 3 || c->ks == 1, "convgru: kernel size %d unsupported", c->ks);
  // the four GroupNorm pointers: all given (the reference's cell) or all NULL (upstream Vid-ODE's norm-free cell, convgru_plain.hip)
  ODEHIP_REQUIRE(c->w_gates && c->b_gates && c->w_can && c->b_can &&
                     (cell_is_plain(c) || (c->gn_gates_w && c->gn_gates_b && c->gn_can_w && c->gn_can_b)),
                 "convgru: null parameter pointer");
  return ODEHIP_OK;
}

int cell_forward_step(const odehip_convgru_cell* c, const odehip_convgru_cell_halves* hv, const float* x, const float* h, float* h_out,
                      float* h_out_nchw, long long nchw_batch_stride, int batch, float* gates_raw, float* z, float* rh, float* cand_raw,
                      const float* mask_b, hipStream_t stream) {
  const int H = c->hidden, I = c->input, HG = H / 32;
  // the images of the two convolutions: -1 = the full weights over cat(x, state), else half j of hv over the one source there is
  const int j_gates = x && h ? -1 : (x ? 0 : 1);
  const int j_can = x && h ? -1 : (x ? 2 : 3);
  auto conv = [&](bool gates, int j, const float* state, float* dst) {
    const float* wp = gates ? c->w_gates : c->w_can;
    const void* wbf = gates ? c->w_gates_bf16 : c->w_can_bf16;
    const float* wwino = gates ? c->w_gates_wino : c->w_can_wino;
    if (hv) {  // a sequence: one image, chosen by the compute mode
      const bool bf = c->w_gates_bf16 != nullptr;
      wp = nullptr;
      wbf = bf ? (j < 0 ? wbf : hv->bf16[j]) : nullptr;
      wwino = bf ? nullptr : (j < 0 ? wwino : hv->wino[j]);
    }
    const float* s1 = x ? x : state;
    const int c1 = x ? I : H, c2 = x && h ? H : 0;
    return conv_layer(s1, c2 ? state : nullptr, c1, c1 + c2, (gates ? 2 : 1) * H, c->ks, wp, gates ? c->b_gates : c->b_can, dst, 0, batch,
                      stream, wbf, wwino, hv != nullptr);
  };
  int rc = conv(true, j_gates, h, gates_raw);
  if (rc != ODEHIP_OK) return rc;
  const bool plain = cell_is_plain(c);  // z then holds the update gate u
  if (plain) launch_plain_gates(gates_raw, h, z, rh, H, batch, stream);
  else if (h)
    hipLaunchKernelGGL(gn_gates_kernel<true>, dim3(2 * HG, batch), dim3(256), 0, stream, gates_raw, c->gn_gates_w, c->gn_gates_b, h, z, rh,
                       HG);
  else  // r * 0 is not formed: the z groups alone
    hipLaunchKernelGGL(gn_gates_kernel<false>, dim3(HG, batch), dim3(256), 0, stream, gates_raw, c->gn_gates_w, c->gn_gates_b, nullptr, z,
                       nullptr, HG);
  rc = conv(false, j_can, rh, cand_raw);
  if (rc != ODEHIP_OK) return rc;
  if (plain)
    launch_plain_update(cand_raw, h, z, h_out, h_out_nchw, nchw_batch_stride, H, batch, mask_b, stream);
  else if (hv) {  // a step of a sequence: its slot of h_seq, always there and dense
    ODEHIP_REQUIRE(h_out_nchw && nchw_batch_stride == (long long)H * kPix && !mask_b, "convgru_sequence: a step needs its dense h_seq slot and takes no mask");
    if (h)
      hipLaunchKernelGGL(seq_update_kernel<true>, dim3(HG, batch), dim3(256), 0, stream, cand_raw, c->gn_can_w, c->gn_can_b, h, z, h_out,
                         h_out_nchw, HG);
    else
      hipLaunchKernelGGL(seq_update_kernel<false>, dim3(HG, batch), dim3(256), 0, stream, cand_raw, c->gn_can_w, c->gn_can_b, nullptr, z,
                         h_out, h_out_nchw, HG);
  } else if (mask_b)
    hipLaunchKernelGGL(gn_update_kernel<kUpdMasked>, dim3(HG, batch), dim3(256), 0, stream, cand_raw, c->gn_can_w, c->gn_can_b, h, z, h_out,
                       h_out_nchw, nchw_batch_stride, HG, mask_b);
  else
    hipLaunchKernelGGL(gn_update_kernel<kUpdPlain>, dim3(HG, batch), dim3(256), 0, stream, cand_raw, c->gn_can_w, c->gn_can_b, h, z, h_out,
                       h_out_nchw, nchw_batch_stride, HG, nullptr);
  return ODEHIP_OK;  // the kernel launches' status is the caller's to ask for: per step in the encoder, once per sequence
}

void launch_state_to_latent(const float* h, float* h_out_nchw, long long nchw_batch_stride, int hidden, int batch, hipStream_t stream) {
  hipLaunchKernelGGL(state_to_latent_kernel, dim3(hidden / 4, batch), dim3(256), 0, stream, h, h_out_nchw, nchw_batch_stride, hidden / 4);
}

int check_encoder(const odehip_encoder* e, bool train, const char* who) {
  ODEHIP_REQUIRE(e, "%s: null descriptor", who);
  int rc = check_stack(&e->f_enc);
  if (rc != ODEHIP_OK) return rc;
  rc = check_cell(&e->cell);
  if (rc != ODEHIP_OK) return rc;
  const int C = e->cell.hidden;
  ODEHIP_REQUIRE(e->cell.input == C && e->f_enc.channels[0] == C && e->f_enc.channels[e->f_enc.n_convs] == C,
                 "%s: encoder dynamics and cell must share the channel count (%d)", who, C);
  ODEHIP_REQUIRE(e->head_hidden % 32 == 0 && e->out_ch % 16 == 0 && e->w_head0 && e->b_head0 && e->w_head1 && e->b_head1,
                 "%s: bad transform_z0 head", who);
  if (!train) return ODEHIP_OK;
  ODEHIP_REQUIRE(C % 64 == 0 && e->head_hidden % 64 == 0 && (2 * e->out_ch) % 64 == 0 && e->f_enc.ks == 3,
                 "%s: the training path needs channel counts that are multiples of 64 and 3x3 encoder dynamics", who);
  for (int l = 0; l <= e->f_enc.n_convs; ++l)
    ODEHIP_REQUIRE(e->f_enc.channels[l] % 64 == 0, "%s: encoder dynamics channels must be multiples of 64", who);
  return ODEHIP_OK;
}

// transform_z0: Conv1x1 -> ReLU -> Conv1x1, split, |std|
static int encoder_head(const odehip_encoder* e, const float* h, float* head_hid, float* head_out, float* mean_nchw, float* std_nchw,
                        int batch, hipStream_t stream) {
  const int C = e->cell.hidden;
  int rc = conv_layer(h, nullptr, C, C, e->head_hidden, 1, e->w_head0, e->b_head0, head_hid, 1, batch, stream);
  if (rc != ODEHIP_OK) return rc;
  rc = conv_layer(head_hid, nullptr, e->head_hidden, e->head_hidden, 2 * e->out_ch, 1, e->w_head1, e->b_head1, head_out, 0, batch, stream);
  if (rc != ODEHIP_OK) return rc;
  const int total = batch * (2 * e->out_ch / 4) * kPix;
  hipLaunchKernelGGL(split_mean_std_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, head_out, mean_nchw, std_nchw, total,
                     e->out_ch / 4);
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}

int encoder_forward(const odehip_encoder* e, const EncLayout& L, void* ws, const float* inputs_nchw, const double* t_host,
                    int run_backwards, float* mean_nchw, float* std_nchw, float* latent_nchw, const float* mask_tb,
                    const unsigned char* step_observed_host, int* cell_steps_run, hipStream_t stream) {
  const int T = L.T, batch = L.B, C = L.C;
  float dts_h[64];
  for (int idx = 0; idx < T; ++idx) dts_h[idx] = frame_dt(t_host, T, idx, run_backwards);
  int rc = upload_bytes(L.p(ws, L.off_dts), dts_h, (size_t)T * 4, stream);
  if (rc != ODEHIP_OK) return rc;
  rc = odehip_nchw_to_q4(inputs_nchw, L.frame(ws, 0), T * batch, C, stream);
  if (rc != ODEHIP_OK) return rc;
  ODEHIP_CHECK_HIP(hipMemsetAsync(L.hstate(ws, 0), 0, (size_t)batch * C * kPix * 4, stream));  // prev_input = zeros
  float* hidv[ODEHIP_MAX_LAYERS];
  int n_run = 0;
  for (int idx = 0; idx < T; ++idx) {
    const int i = visited_frame(T, idx, run_backwards);
    const bool observed = step_is_observed(step_observed_host, i);
    float* h_ode = L.per(ws, L.off_hode, idx, L.hs);
    // h_ode = h + dt * f_enc(h)
    CombineArgs c;
    memset(&c, 0, sizeof(c));
    c.k_scale = 1.0f;
    c.y = L.hstate(ws, idx);
    c.h_ptr = L.p(ws, L.off_dts) + idx;
    c.c1[0] = 1.0f;
    c.out1 = observed ? h_ode : L.hstate(ws, idx + 1);  // nobody observed frame i: the Euler-advanced state IS the next state
    if (L.train)  // the reverse sweep reads the dynamics' hidden activations of every step
      for (int l = 0; l < L.NH; ++l) hidv[l] = L.hidden(ws, idx, l);
    rc = enqueue_f_saving(&e->f_enc, L.hstate(ws, idx), batch, L.train ? hidv : nullptr, L.p(ws, L.off_ping), L.p(ws, L.off_pong), &c,
                          nullptr, nullptr, stream);
    if (rc != ODEHIP_OK) return rc;
    float* lat = latent_nchw ? latent_nchw + (size_t)idx * C * kPix : nullptr;  // latent_ys (B,T,C,H,W): slot idx of each sample
    if (!observed) {
      if (lat) launch_state_to_latent(L.hstate(ws, idx + 1), lat, (long long)T * C * kPix, C, batch, stream);
      continue;
    }
    ++n_run;
    rc = cell_forward_step(&e->cell, nullptr, L.frame(ws, i), h_ode, L.hstate(ws, idx + 1), lat, (long long)T * C * kPix, batch,
                           L.per(ws, L.off_gates, idx, 2 * L.hs), L.per(ws, L.off_z, idx, L.hs), L.per(ws, L.off_rh, idx, L.hs),
                           L.per(ws, L.off_cand, idx, L.hs), mask_tb ? mask_tb + (size_t)i * batch : nullptr, stream);
    if (rc != ODEHIP_OK) return rc;
    ODEHIP_CHECK_HIP(hipGetLastError());
  }
  rc = encoder_head(e, L.hstate(ws, T), L.p(ws, L.off_headhid), L.p(ws, L.off_headout), mean_nchw, std_nchw, batch, stream);
  if (rc != ODEHIP_OK) return rc;
  if (cell_steps_run) *cell_steps_run = n_run;
  return ODEHIP_OK;
}

}  // namespace odehip

using namespace odehip;

extern "C" size_t odehip_convgru_cell_workspace_bytes(const odehip_convgru_cell* c, int batch) {
  if (!c || batch <= 0) return 0;
  const size_t hs = al256((size_t)batch * c->hidden * kPix * 4);
  return al256((size_t)batch * c->input * kPix * 4) + 6 * hs;  // x, h, gates_raw(2), z, rh, cand_raw
}

// x: (B,input,16,16), h: (B,hidden,16,16) NCHW -> h_next NCHW      (ConvGRUCell.forward with seq_len = 1)
extern "C" int odehip_convgru_cell_forward(const odehip_convgru_cell* c, const float* x_nchw, const float* h_nchw,
                                           float* h_next_nchw, int batch, void* workspace, size_t workspace_bytes,
                                           void* stream_) {
  int rc = check_cell(c);
  if (rc != ODEHIP_OK) return rc;
  ODEHIP_REQUIRE(x_nchw && h_nchw && h_next_nchw && workspace && batch > 0, "convgru_cell_forward: bad argument");
  ODEHIP_REQUIRE(workspace_bytes >= odehip_convgru_cell_workspace_bytes(c, batch), "convgru_cell_forward: workspace too small");
  hipStream_t stream = (hipStream_t)stream_;
  char* base = (char*)workspace;
  size_t off = 0;
  auto take = [&](size_t bytes) { float* p = (float*)(base + off); off += al256(bytes); return p; };
  const size_t hs = (size_t)batch * c->hidden * kPix * 4;
  float* x = take((size_t)batch * c->input * kPix * 4);
  float* h = take(hs);
  float* gates = take(2 * hs);
  float* z = take(hs);
  float* rh = take(hs);
  float* cand = take(hs);
  rc = odehip_nchw_to_q4(x_nchw, x, batch, c->input, stream);
  if (rc != ODEHIP_OK) return rc;
  rc = odehip_nchw_to_q4(h_nchw, h, batch, c->hidden, stream);
  if (rc != ODEHIP_OK) return rc;
  // h' is written straight to NCHW; the Q4 copy goes to `gates` (free by then)
  rc = cell_forward_step(c, nullptr, x, h, gates, h_next_nchw, (long long)c->hidden * kPix, batch, gates, z, rh, cand, nullptr, stream);
  if (rc != ODEHIP_OK) return rc;
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}

extern "C" size_t odehip_encoder_workspace_bytes(const odehip_encoder* e, int n_frames, int batch) {
  if (!e || n_frames <= 0 || batch <= 0) return 0;
  return EncLayout(e, n_frames, batch, false).total;
}

extern "C" int odehip_odeconvgru_encode(const odehip_encoder* e, const float* inputs_nchw, const double* t_host, int n_frames,
                                        int batch, int run_backwards, float* mean_nchw, float* std_nchw, float* latent_nchw,
                                        void* workspace, size_t workspace_bytes, void* stream_) {
  return odehip_odeconvgru_encode_masked(e, inputs_nchw, t_host, n_frames, batch, run_backwards, mean_nchw, std_nchw, latent_nchw, workspace,
                                         workspace_bytes, stream_, nullptr);
}

extern "C" int odehip_odeconvgru_encode_masked(const odehip_encoder* e, const float* inputs_nchw, const double* t_host, int n_frames,
                                               int batch, int run_backwards, float* mean_nchw, float* std_nchw, float* latent_nchw,
                                               void* workspace, size_t workspace_bytes, void* stream_, const float* mask_tb) {
  return odehip_odeconvgru_encode_steps(e, inputs_nchw, t_host, n_frames, batch, run_backwards, mean_nchw, std_nchw, latent_nchw, workspace,
                                        workspace_bytes, stream_, mask_tb, nullptr, nullptr);
}

// mask_tb: (T, B) on the device, row i = the observation mask of FRAME i (whenever it is visited), or null = all observed.
// step_observed_host: T bytes on the host, byte i == 0 = no sample observed FRAME i (its step runs without the cell), or null = every
// step runs the cell.  cell_steps_run (host, may be null): the number of steps that did.
extern "C" int odehip_odeconvgru_encode_steps(const odehip_encoder* e, const float* inputs_nchw, const double* t_host, int n_frames,
                                              int batch, int run_backwards, float* mean_nchw, float* std_nchw, float* latent_nchw,
                                              void* workspace, size_t workspace_bytes, void* stream_, const float* mask_tb,
                                              const unsigned char* step_observed_host, int* cell_steps_run) {
  int rc = check_encoder(e, false, "odeconvgru_encode");
  if (rc != ODEHIP_OK) return rc;
  ODEHIP_REQUIRE(inputs_nchw && t_host && mean_nchw && std_nchw && workspace, "odeconvgru_encode: null pointer");
  ODEHIP_REQUIRE(n_frames >= 1 && n_frames <= 64 && batch > 0, "odeconvgru_encode: bad sizes (frames %d, batch %d)", n_frames, batch);
  const EncLayout L(e, n_frames, batch, false);
  ODEHIP_REQUIRE(workspace_bytes >= L.total, "odeconvgru_encode: workspace too small");
  return encoder_forward(e, L, workspace, inputs_nchw, t_host, run_backwards, mean_nchw, std_nchw, latent_nchw, mask_tb, step_observed_host,
                         cell_steps_run, (hipStream_t)stream_);
}
