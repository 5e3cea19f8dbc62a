// convgru_sequence.hip -- a whole ConvGRU sequence as one unit of work (gfx950): what the reference's ConvGRU baseline asks of its
// cell (models/ConvGRU.py:133-149 encoder: cell(frames, None, T_in); :225-242 decoder: cell(None, h, T_out), an autonomous rollout
// of 10 steps in training and 190 at test) and back-propagation through time over it.
//
// Step t (ConvGRUCell.py:72-82):  G = conv5(cat(x_t, h)); (z, r) = sigmoid(GN(G)); Cr = conv5(cat(x_t, r*h)); h' = (1-z) h + z tanh(GN(Cr))
//   x given, h given   the two-source launches of the single step (convgru.hip) -- same kernels, same weights, same results
//   x == NULL          cat(0, h): both convolutions are ONE-source launches over the state half W[:, input:] of the weights, packed
//                      on its own (hv->wino[1], [3]); K = hidden * 25 instead of (input + hidden) * 25, no zero frame exists anywhere
//   h == NULL, t == 0  cat(x_0, 0): one-source launches over the frame half (hv->wino[0], [2]); r*h is not formed (only the z groups
//                      of the gates are normalised) and h' = z tanh(GN(Cr)); nothing of the state buffers is read
// Every step writes its state twice from the update kernel's registers: Q4 (the next step's source) and NCHW into slot t of h_seq.
//
// Layouts.  Forward: [x Q4 (T) | h ping | h pong | gates_raw (2) | z | r*h | cand_raw].  Train keeps per step what the reverse sweep
// reads (h_t, gates_raw, z, r*h, cand_raw) and the sweep adds the gradients of the two conv outputs per step: the batched weight
// gradient needs them all at the end.  SeqLayout is the one place that knows the offsets.
//
// Reverse sweep, t = T-1 .. 0, gh = dL/dh_t (everything that arrives at slot t: grad_h_seq[t] + the recurrence):
//   gn_update_bwd : gh -> gCr, gz_pre, gh_prev = gh (1-z)                               (convgru_backward.hip kernels)
//   conv5^T(gCr)  : state half -> g_rh;  frame half -> gx_c (only with x)
//   gn_gates_bwd  : -> gG; gh_prev += g_rh r
//   conv5^T(gG)   : state half, epilogue dL/dh_{t-1} = gh_prev + . + grad_h_seq[t-1];  frame half -> gx_t = gx_c + . (only with x)
// A first step from a zero state has no state-half launches (g_rh = 0, nothing flows further back).  Then, per weight half and 64x64
// channel tile, one weight-gradient launch over ALL steps (steps x samples are the batch of the F(2x2,5x5)-domain kernel,
// wgrad_wino5.hip; slabs summed in a fixed order), and fixed-order sums of the per-(step, sample) GroupNorm partials.  No float atomics.
#include <string.h>

#include <vector>

#include "convgru_gn.h"
#include "persist.h"

namespace odehip {

// convgru_backward.hip
void launch_gn_update_bwd(const float* cand_raw, const float* gamma, const float* beta, const float* gh, const float* z, const float* h_prev,
                          float* g_cand_raw, float* gz_pre, float* gh_prev, float* dgamma_part, float* dbeta_part, int hidden, int batch,
                          hipStream_t stream);
void launch_gn_gates_bwd(const float* gates_raw, const float* gamma, const float* beta, const float* gz_pre, const float* g_rh,
                         const float* h_prev, float* gh_prev, float* g_gates_raw, float* dgamma_part, float* dbeta_part, int hidden,
                         int batch, hipStream_t stream);
void launch_reduce_rows(const float* part, int n_rows, int n_cols, float* out, hipStream_t stream);

// gates_raw (B, 2*hid) Q4 -> z (B,hid) and, with a state, rh = r * h.  HAS_H = false is launched over the z groups alone.
template <bool HAS_H>
__global__ __launch_bounds__(256) void seq_gates_kernel(const float* __restrict__ gates_raw, const float* __restrict__ gamma,
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
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    f32x4 s = {sigmoidf_(v[q].x), sigmoidf_(v[q].y), sigmoidf_(v[q].z), sigmoidf_(v[q].w)};
    if (HAS_H) {
      if (!is_z) s *= ((const f32x4*)h + base + threadIdx.x)[q * kPix];
    }
    out[q * kPix] = s;
  }
}

// cand_raw (B,hid) Q4 -> h' = (1 - z) h + z tanh(GN(cand_raw)) (HAS_H = false: h = 0, h' = z tanh(.)), written as Q4 (h_out) and into
// the step's NCHW slot of h_seq (sample b at h_seq_slot + b * hid * 256)
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

namespace {

struct SeqLayout {
  int T, B, H, I;
  bool has_x, train;
  size_t hs, xs;  // bytes of one state / frame tensor (256-aligned)
  size_t off_x, off_h, off_gates, off_z, off_rh, off_cand;   // forward (train: per step; h has T + 1 slots, slot t = the state BEFORE step t)
  size_t off_gseq, off_ggates, off_gcand, off_gx, off_gxc, off_gzpre, off_ghprev, off_grh, off_gh, off_gh0, off_pgg, off_pgc, off_tab,
      off_slab;
  size_t total;
  SeqLayout(const odehip_convgru_cell* c, int n_steps, int batch, bool has_x_, bool train_)
      : T(n_steps), B(batch), H(c->hidden), I(c->input), has_x(has_x_), train(train_) {
    hs = al256((size_t)B * H * kPix * 4);
    xs = al256((size_t)B * I * kPix * 4);
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += al256(bytes); return r; };
    const size_t per = train ? (size_t)T : 1;
    off_x = take(has_x ? (size_t)T * xs : 0);
    off_h = take(train ? (size_t)(T + 1) * hs : 2 * hs);
    off_gates = take(per * 2 * hs);
    off_z = take(per * hs);
    off_rh = take(per * hs);
    off_cand = take(per * hs);
    off_gseq = off_ggates = off_gcand = off_gx = off_gxc = off_gzpre = off_ghprev = off_grh = off_gh = off_gh0 = off_pgg = off_pgc = off_tab =
        off_slab = o;
    if (train) {
      off_gseq = take((size_t)T * hs);
      off_ggates = take((size_t)T * 2 * hs);
      off_gcand = take((size_t)T * hs);
      off_gx = take(has_x ? (size_t)T * xs : 0);
      off_gxc = take(has_x ? xs : 0);
      off_gzpre = take(hs);
      off_ghprev = take(hs);
      off_grh = take(hs);
      off_gh = take(2 * hs);
      off_gh0 = take(hs);
      off_pgg = take((size_t)2 * T * B * 2 * H * 4);   // [dgamma | dbeta][T*B][2H]
      off_pgc = take((size_t)2 * T * B * H * 4);
      off_tab = take((size_t)4 * T * sizeof(WgradPair));
      off_slab = take(wgrad_slab_bytes(B));
    }
    total = o;
  }
  float* p(void* ws, size_t off) const { return (float*)((char*)ws + off); }
  float* x(void* ws, int t) const { return p(ws, off_x + (size_t)t * xs); }
  float* h(void* ws, int k) const { return p(ws, off_h + (size_t)k * hs); }   // forward-only: k & 1
  float* step(void* ws, size_t off, int t, size_t bytes) const { return p(ws, off + (train ? (size_t)t * bytes : 0)); }
};

int check_sequence(const odehip_convgru_cell* c, const odehip_convgru_cell_halves* hv, int n_steps, int batch, bool has_x, bool has_h0, bool train, const char* who) {
  ODEHIP_REQUIRE(c, "%s: null cell descriptor", who);
  ODEHIP_REQUIRE(hv, "%s: null weight-halves descriptor", who);
  ODEHIP_REQUIRE(n_steps >= 1 && batch >= 1, "%s: n_steps and batch must be at least 1 (got %d, %d)", who, n_steps, batch);
  ODEHIP_REQUIRE(has_x || has_h0, "%s: x_seq and h0 are both NULL (a zero input from a zero state)", who);
  ODEHIP_REQUIRE(c->ks == 5 && c->hidden > 0 && c->hidden % 32 == 0 && c->input > 0 && c->input % 8 == 0,
                 "%s: the F(2x2,5x5) kernels serve ks = 5, input_dim %% 8 == 0, hidden_dim %% 32 == 0 (got ks %d, input %d, hidden %d)", who,
                 c->ks, c->input, c->hidden);
  ODEHIP_REQUIRE(!train || (c->hidden % 64 == 0 && c->input % 64 == 0),
                 "%s: the training path needs input_dim and hidden_dim that are multiples of 64 (got %d, %d)", who, c->input, c->hidden);
  ODEHIP_REQUIRE((long long)n_steps * batch <= (1 << 20), "%s: n_steps * batch too large", who);
  ODEHIP_REQUIRE(c->b_gates && c->gn_gates_w && c->gn_gates_b && c->b_can && c->gn_can_w && c->gn_can_b, "%s: null parameter pointer", who);
  const bool bf = c->w_gates_bf16 != nullptr;
  ODEHIP_REQUIRE(!bf || (c->w_can_bf16 && c->input % 16 == 0), "%s: bf16 mode needs both bf16 images and input_dim %% 16 == 0", who);
  auto half = [&](int j) { return bf ? hv->bf16[j] != nullptr : hv->wino[j] != nullptr; };
  const bool full = bf ? true : (c->w_gates_wino && c->w_can_wino);
  if (has_x && (has_h0 || n_steps > 1)) ODEHIP_REQUIRE(full, "%s: no F(2x2,5x5) form of the full weights (w_gates_wino / w_can_wino)", who);
  if (!has_x) ODEHIP_REQUIRE(half(1) && half(3), "%s: zero input needs the state-half images (halves 1 and 3 of odehip_convgru_cell_halves)", who);
  if (!has_h0) ODEHIP_REQUIRE(half(0) && half(2), "%s: a zero state needs the frame-half images (halves 0 and 2 of odehip_convgru_cell_halves)", who);
  return ODEHIP_OK;
}

// one 5x5 convolution of a step over one or two Q4 sources; `j` picks the images: -1 = the full weights, else half j of hv
int seq_conv(const odehip_convgru_cell* c, const odehip_convgru_cell_halves* hv, bool gates, int j, const float* s1, int c1, const float* s2, int c2, float* dst, int batch,
             hipStream_t stream) {
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.src1 = s1;
  a.src2 = s2;
  a.q1 = c1 / 4;
  a.qin = (c1 + c2) / 4;
  a.qout = (gates ? 2 : 1) * c->hidden / 4;
  a.bias = gates ? c->b_gates : c->b_can;
  a.dst = dst;
  a.batch = batch;
  a.act = kActNone;
  int rc;
  if (c->w_gates_bf16) {
    a.w_bf16 = j < 0 ? (gates ? c->w_gates_bf16 : c->w_can_bf16) : hv->bf16[j];
    rc = launch_bf16_5x5(a, stream);
  } else {
    a.w_wino = j < 0 ? (gates ? c->w_gates_wino : c->w_can_wino) : hv->wino[j];
    rc = launch_wino5(a, stream);
  }
  ODEHIP_REQUIRE(rc != 1, "convgru_sequence: no 5x5 kernel serves %d -> %d channels", c1 + c2, a.qout * 4);
  return rc;
}

int run_forward(const odehip_convgru_cell* c, const odehip_convgru_cell_halves* hv, const float* x_seq, const float* h0, int T, int batch, float* h_seq, void* ws, size_t ws_bytes,
                bool train, hipStream_t stream, const char* who) {
  int rc = check_sequence(c, hv, T, batch, x_seq != nullptr, h0 != nullptr, train, who);
  if (rc != ODEHIP_OK) return rc;
  ODEHIP_REQUIRE(h_seq && ws, "%s: null output or workspace", who);
  const SeqLayout L(c, T, batch, x_seq != nullptr, train);
  ODEHIP_REQUIRE(ws_bytes >= L.total, "%s: workspace too small (%zu < %zu bytes)", who, ws_bytes, L.total);
  const int H = c->hidden, I = c->input, HG = H / 32;
  if (x_seq && (rc = odehip_nchw_to_q4(x_seq, L.x(ws, 0), T * batch, I, stream)) != ODEHIP_OK) return rc;
  // the state before step t lives in slot t (train) / t & 1 (forward); without h0 slot 0 is read by nobody in the forward pass, the
  // reverse sweep reads it as the zero state it stands for
  auto hslot = [&](int k) { return L.h(ws, train ? k : (k & 1)); };
  if (h0) {
    if ((rc = odehip_nchw_to_q4(h0, hslot(0), batch, H, stream)) != ODEHIP_OK) return rc;
  } else if (train) {
    ODEHIP_CHECK_HIP(hipMemsetAsync(hslot(0), 0, L.hs, stream));
  }
  for (int t = 0; t < T; ++t) {
    const bool has_h = h0 || t > 0;
    const float* x = x_seq ? L.x(ws, t) : nullptr;
    const float* h = has_h ? hslot(t) : nullptr;
    float* gates = L.step(ws, L.off_gates, t, 2 * L.hs);
    float* z = L.step(ws, L.off_z, t, L.hs);
    float* rh = L.step(ws, L.off_rh, t, L.hs);
    float* cand = L.step(ws, L.off_cand, t, L.hs);
    float* slot = h_seq + (size_t)t * batch * H * kPix;
    if (x && has_h) rc = seq_conv(c, hv, true, -1, x, I, h, H, gates, batch, stream);
    else if (x) rc = seq_conv(c, hv, true, 0, x, I, nullptr, 0, gates, batch, stream);
    else rc = seq_conv(c, hv, true, 1, h, H, nullptr, 0, gates, batch, stream);
    if (rc != ODEHIP_OK) return rc;
    if (has_h)
      hipLaunchKernelGGL(seq_gates_kernel<true>, dim3(2 * HG, batch), dim3(256), 0, stream, gates, c->gn_gates_w, c->gn_gates_b, h, z, rh, HG);
    else
      hipLaunchKernelGGL(seq_gates_kernel<false>, dim3(HG, batch), dim3(256), 0, stream, gates, c->gn_gates_w, c->gn_gates_b, nullptr, z,
                         nullptr, HG);
    if (x && has_h) rc = seq_conv(c, hv, false, -1, x, I, rh, H, cand, batch, stream);
    else if (x) rc = seq_conv(c, hv, false, 2, x, I, nullptr, 0, cand, batch, stream);
    else rc = seq_conv(c, hv, false, 3, rh, H, nullptr, 0, cand, batch, stream);
    if (rc != ODEHIP_OK) return rc;
    if (has_h)
      hipLaunchKernelGGL(seq_update_kernel<true>, dim3(HG, batch), dim3(256), 0, stream, cand, c->gn_can_w, c->gn_can_b, h, z, hslot(t + 1),
                         slot, HG);
    else
      hipLaunchKernelGGL(seq_update_kernel<false>, dim3(HG, batch), dim3(256), 0, stream, cand, c->gn_can_w, c->gn_can_b, nullptr, z,
                         hslot(t + 1), slot, HG);
  }
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}

}  // namespace
}  // namespace odehip

using namespace odehip;

extern "C" size_t odehip_convgru_sequence_workspace_bytes(const odehip_convgru_cell* c, int n_steps, int batch, int has_x, int train) {
  if (!c || n_steps < 1 || batch < 1 || c->hidden <= 0 || c->input <= 0 || (long long)n_steps * batch > (1 << 20)) return 0;
  return SeqLayout(c, n_steps, batch, has_x != 0, train != 0).total;
}

extern "C" int odehip_convgru_sequence_forward(const odehip_convgru_cell* c, const odehip_convgru_cell_halves* hv, const float* x_seq_nchw, const float* h0_nchw, int n_steps,
                                               int batch, float* h_seq_nchw, void* workspace, size_t workspace_bytes, void* stream) {
  return run_forward(c, hv, x_seq_nchw, h0_nchw, n_steps, batch, h_seq_nchw, workspace, workspace_bytes, false, (hipStream_t)stream,
                     "convgru_sequence_forward");
}

extern "C" int odehip_convgru_sequence_train(const odehip_convgru_cell* c, const odehip_convgru_cell_halves* hv, const float* x_seq_nchw, const float* h0_nchw, int n_steps,
                                             int batch, float* h_seq_nchw, void* workspace, size_t workspace_bytes, void* stream) {
  return run_forward(c, hv, x_seq_nchw, h0_nchw, n_steps, batch, h_seq_nchw, workspace, workspace_bytes, true, (hipStream_t)stream,
                     "convgru_sequence_train");
}

extern "C" int odehip_convgru_sequence_backward(const odehip_convgru_cell* c, const odehip_convgru_cell_halves* hv,
                                                const odehip_convgru_cell_bwd* cb, int has_x_, int has_h0_,
                                                int n_steps, int batch, const float* grad_h_seq_nchw, float* grad_x_seq_nchw,
                                                float* grad_h0_nchw, const odehip_convgru_cell_grads* gr, void* workspace,
                                                size_t workspace_bytes, void* stream_) {
  const bool has_x = has_x_ != 0, has_h0 = has_h0_ != 0;
  const char* who = "convgru_sequence_backward";
  int rc = check_sequence(c, hv, n_steps, batch, has_x, has_h0, true, who);
  if (rc != ODEHIP_OK) return rc;
  ODEHIP_REQUIRE(cb && grad_h_seq_nchw && gr && workspace, "%s: null pointer", who);
  ODEHIP_REQUIRE((!has_x || grad_x_seq_nchw) && (!has_h0 || grad_h0_nchw), "%s: null gradient output", who);
  ODEHIP_REQUIRE(cb->w_gates_dh && cb->w_can_dh && (!has_x || (cb->w_gates_dx && cb->w_can_dx)), "%s: null transposed weight", who);
  ODEHIP_REQUIRE(gr->w_gates && gr->b_gates && gr->gn_gates_w && gr->gn_gates_b && gr->w_can && gr->b_can && gr->gn_can_w && gr->gn_can_b,
                 "%s: null parameter gradient", who);
  const int T = n_steps, H = c->hidden, I = c->input;
  const SeqLayout L(c, T, batch, has_x, true);
  ODEHIP_REQUIRE(workspace_bytes >= L.total, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, L.total);
  hipStream_t stream = (hipStream_t)stream_;
  void* ws = workspace;
  float* gz_pre = L.p(ws, L.off_gzpre);
  float* gh_prev = L.p(ws, L.off_ghprev);
  float* gx_c = L.p(ws, L.off_gxc);
  float* g_rh = L.p(ws, L.off_grh);
  float* gh0 = L.p(ws, L.off_gh0);
  float* pgg = L.p(ws, L.off_pgg);
  float* pgc = L.p(ws, L.off_pgc);
  const size_t pgg_half = (size_t)T * batch * 2 * H, pgc_half = (size_t)T * batch * H;
  const bool bf = c->w_gates_bf16 != nullptr;

  // input-gradient convolution of one weight half j (0 gates/x, 1 gates/h, 2 can/x, 3 can/h): plain store or a reverse-sweep target
  auto conv_bwd = [&](const float* src, int cin, int cout, int j, const BwdArgs* bw, float* dst) {
    const float* wt = j == 0 ? cb->w_gates_dx : (j == 1 ? cb->w_gates_dh : (j == 2 ? cb->w_can_dx : cb->w_can_dh));
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.src1 = src;
    a.q1 = a.qin = cin / 4;
    a.qout = cout / 4;
    a.w_packed = wt;
    a.w_bf16 = bf ? cb->bf16[j] : nullptr;
    a.w_wino = a.w_bf16 ? nullptr : cb->wino[j];
    a.batch = batch;
    a.combine = bw ? 3 : 0;
    if (bw) a.bwd = *bw;
    a.dst = dst;
    return launch_conv(a, 5, stream);
  };

  if ((rc = odehip_nchw_to_q4(grad_h_seq_nchw, L.p(ws, L.off_gseq), T * batch, H, stream)) != ODEHIP_OK) return rc;
  const float* gh = L.p(ws, L.off_gseq + (size_t)(T - 1) * L.hs);
  for (int t = T - 1; t >= 0; --t) {
    const bool has_h = has_h0 || t > 0;
    const float* h_prev = L.h(ws, t);   // zeros at t == 0 without h0 (written by the train call)
    float* g_cand = L.p(ws, L.off_gcand + (size_t)t * L.hs);
    float* g_gates = L.p(ws, L.off_ggates + (size_t)t * 2 * L.hs);
    launch_gn_update_bwd(L.p(ws, L.off_cand + (size_t)t * L.hs), c->gn_can_w, c->gn_can_b, gh, L.p(ws, L.off_z + (size_t)t * L.hs), h_prev,
                         g_cand, gz_pre, gh_prev, pgc + (size_t)t * batch * H, pgc + pgc_half + (size_t)t * batch * H, H, batch, stream);
    if (has_x && (rc = conv_bwd(g_cand, H, I, 2, nullptr, gx_c)) != ODEHIP_OK) return rc;
    if (has_h) {
      if ((rc = conv_bwd(g_cand, H, H, 3, nullptr, g_rh)) != ODEHIP_OK) return rc;
    } else {
      ODEHIP_CHECK_HIP(hipMemsetAsync(g_rh, 0, L.hs, stream));   // r * 0: nothing arrives at r, and no state lies further back
    }
    launch_gn_gates_bwd(L.p(ws, L.off_gates + (size_t)t * 2 * L.hs), c->gn_gates_w, c->gn_gates_b, gz_pre, g_rh, h_prev, gh_prev, g_gates,
                        pgg + (size_t)t * batch * 2 * H, pgg + pgg_half + (size_t)t * batch * 2 * H, H, batch, stream);
    BwdArgs w;
    memset(&w, 0, sizeof(w));
    w.n_targets = 1;
    w.tgt[0].a_c = 1.0f;
    w.tgt[0].g_c = 1.0f;
    if (has_x) {
      w.tgt[0].out = L.p(ws, L.off_gx + (size_t)t * L.xs);
      w.tgt[0].srcA = gx_c;
      if ((rc = conv_bwd(g_gates, 2 * H, I, 0, &w, nullptr)) != ODEHIP_OK) return rc;
    }
    if (has_h) {
      float* out = t > 0 ? L.p(ws, L.off_gh + (size_t)(t & 1) * L.hs) : gh0;
      w.tgt[0].out = out;
      w.tgt[0].srcA = gh_prev;
      if (t > 0) {   // what arrives at slot t - 1 from outside joins in the same epilogue
        w.tgt[0].srcB = L.p(ws, L.off_gseq + (size_t)(t - 1) * L.hs);
        w.tgt[0].b_c = 1.0f;
      }
      if ((rc = conv_bwd(g_gates, 2 * H, H, 1, &w, nullptr)) != ODEHIP_OK) return rc;
      gh = out;
    }
  }
  if (has_x && (rc = odehip_q4_to_nchw(L.p(ws, L.off_gx), grad_x_seq_nchw, T * batch, I, stream)) != ODEHIP_OK) return rc;
  if (has_h0 && (rc = odehip_q4_to_nchw(gh0, grad_h0_nchw, batch, H, stream)) != ODEHIP_OK) return rc;

  // ---- weight gradients: tables [gates/x | gates/h | can/x | can/h] x T, one upload; the state halves of a sequence that starts
  // from a zero state begin at step 1 (step 0 multiplies a zero state: it contributes nothing and its slot holds no r*h)
  WgradPair* const table0 = (WgradPair*)L.p(ws, L.off_tab);
  float* slabs = L.p(ws, L.off_slab);
  std::vector<WgradPair> host((size_t)4 * T);
  memset(host.data(), 0, host.size() * sizeof(WgradPair));
  for (int j = 0; j < 4; ++j)
    for (int t = 0; t < T; ++t) {
      WgradPair& e = host[(size_t)j * T + t];
      e.g = j < 2 ? L.p(ws, L.off_ggates + (size_t)t * 2 * L.hs) : L.p(ws, L.off_gcand + (size_t)t * L.hs);
      e.a = (j & 1) == 0 ? (has_x ? L.x(ws, t) : nullptr) : (j == 1 ? L.h(ws, t) : L.p(ws, L.off_rh + (size_t)t * L.hs));
      e.scale = 1.0f;
    }
  if ((rc = staged_upload(table0, host.data(), host.size() * sizeof(WgradPair), stream)) != ODEHIP_OK) return rc;
  const int t_first = has_h0 ? 0 : 1, n_state = T - t_first;
  for (int j = 0; j < 2; ++j) {   // gates, can
    const int g_ch = j == 0 ? 2 * H : H;
    float* dw = j == 0 ? gr->w_gates : gr->w_can;
    float* db = j == 0 ? gr->b_gates : gr->b_can;
    if (!has_x || n_state == 0)   // a half without a launch: exact zeros, as autograd gives for a zero operand
      ODEHIP_CHECK_HIP(hipMemsetAsync(dw, 0, (size_t)g_ch * (I + H) * 25 * 4, stream));
    for (int half = 0; half < 2; ++half) {
      if (half == 0 ? !has_x : n_state == 0) continue;
      const WgradPair* const table = table0 + (size_t)(2 * j + half) * T + (half == 1 ? t_first : 0);
      const int n_eval = half == 0 ? T : n_state, a_ch = half == 0 ? I : H;
      const bool bias_here = half == 0 || !has_x;   // the launches over ALL steps carry the bias sums
      rc = launch_wgrad_layer(table, n_eval, batch, bf ? 4 : wgrad_esplit(batch, n_eval), slabs, dw, db, 5, g_ch, a_ch, I + H, half * I, bf,
                              bias_here, stream);
      if (rc != ODEHIP_OK) return rc;
    }
  }
  launch_reduce_rows(pgg, T * batch, 2 * H, gr->gn_gates_w, stream);
  launch_reduce_rows(pgg + pgg_half, T * batch, 2 * H, gr->gn_gates_b, stream);
  launch_reduce_rows(pgc, T * batch, H, gr->gn_can_w, stream);
  launch_reduce_rows(pgc + pgc_half, T * batch, H, gr->gn_can_b, stream);
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}
