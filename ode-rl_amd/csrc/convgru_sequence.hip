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

#include "convgru_cell.h"
#include "persist.h"

namespace odehip {

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

int run_forward(const odehip_convgru_cell* c, const odehip_convgru_cell_halves* hv, const float* x_seq, const float* h0, int T, int batch, float* h_seq, void* ws, size_t ws_bytes,
                bool train, hipStream_t stream, const char* who) {
  int rc = check_sequence(c, hv, T, batch, x_seq != nullptr, h0 != nullptr, train, who);
  if (rc != ODEHIP_OK) return rc;
  ODEHIP_REQUIRE(h_seq && ws, "%s: null output or workspace", who);
  const SeqLayout L(c, T, batch, x_seq != nullptr, train);
  ODEHIP_REQUIRE(ws_bytes >= L.total, "%s: workspace too small (%zu < %zu bytes)", who, ws_bytes, L.total);
  const int H = c->hidden, I = c->input;
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
    float* slot = h_seq + (size_t)t * batch * H * kPix;
    rc = cell_forward_step(c, hv, x, h, hslot(t + 1), slot, (long long)H * kPix, batch, L.step(ws, L.off_gates, t, 2 * L.hs),
                           L.step(ws, L.off_z, t, L.hs), L.step(ws, L.off_rh, t, L.hs), L.step(ws, L.off_cand, t, L.hs), nullptr, stream);
    if (rc != ODEHIP_OK) return rc;
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
  float* gh0 = L.p(ws, L.off_gh0);
  float* pgg = L.p(ws, L.off_pgg);
  float* pgc = L.p(ws, L.off_pgc);
  const size_t pgg_half = (size_t)T * batch * 2 * H, pgc_half = (size_t)T * batch * H;
  const bool bf = c->w_gates_bf16 != nullptr;
  const CellDgradW dw = dgrad_images(cb, bf);   // the bf16 images only in bf16 mode

  if ((rc = odehip_nchw_to_q4(grad_h_seq_nchw, L.p(ws, L.off_gseq), T * batch, H, stream)) != ODEHIP_OK) return rc;
  const float* gh = L.p(ws, L.off_gseq + (size_t)(T - 1) * L.hs);
  std::vector<CatStep> cat((size_t)T);
  for (int t = T - 1; t >= 0; --t) {
    CellBwdStep s;
    s.cand_raw = L.p(ws, L.off_cand + (size_t)t * L.hs);
    s.z = L.p(ws, L.off_z + (size_t)t * L.hs);
    s.gates_raw = L.p(ws, L.off_gates + (size_t)t * 2 * L.hs);
    s.h_prev = L.h(ws, t);   // zeros at t == 0 without h0 (written by the train call)
    s.gh = gh;
    s.g_cand = L.p(ws, L.off_gcand + (size_t)t * L.hs);
    s.g_gates = L.p(ws, L.off_ggates + (size_t)t * 2 * L.hs);
    s.gz_pre = L.p(ws, L.off_gzpre);
    s.gh_prev = L.p(ws, L.off_ghprev);
    s.gx_c = L.p(ws, L.off_gxc);
    s.g_rh = L.p(ws, L.off_grh);
    s.pgc_w = pgc + (size_t)t * batch * H;
    s.pgc_b = s.pgc_w + pgc_half;
    s.pgg_w = pgg + (size_t)t * batch * 2 * H;
    s.pgg_b = s.pgg_w + pgg_half;
    s.mask_b = nullptr;
    s.has_x = has_x;
    s.has_h = has_h0 || t > 0;   // a first step from a zero state: nothing flows further back
    cat[t] = CatStep{s.g_gates, s.g_cand, has_x ? L.x(ws, t) : nullptr, s.h_prev, L.p(ws, L.off_rh + (size_t)t * L.hs)};
    // dL/dh_{t-1} = gh_prev + . + grad_h_seq[t-1]: what arrives at slot t - 1 from outside joins in the same epilogue
    float* out = t > 0 ? L.p(ws, L.off_gh + (size_t)(t & 1) * L.hs) : gh0;
    rc = cell_backward_step(c, dw, s, bwd_target(L.p(ws, L.off_gx + (size_t)t * L.xs), s.gx_c),
                            bwd_target(out, s.gh_prev, t > 0 ? L.p(ws, L.off_gseq + (size_t)(t - 1) * L.hs) : nullptr), batch, stream);
    if (rc != ODEHIP_OK) return rc;
    if (s.has_h) gh = out;
  }
  if (has_x && (rc = odehip_q4_to_nchw(L.p(ws, L.off_gx), grad_x_seq_nchw, T * batch, I, stream)) != ODEHIP_OK) return rc;
  if (has_h0 && (rc = odehip_q4_to_nchw(gh0, grad_h0_nchw, batch, H, stream)) != ODEHIP_OK) return rc;

  // ---- weight gradients: tables [gates/x | gates/h | can/x | can/h] x T, one upload; the state halves of a sequence that starts
  // from a zero state begin at step 1 (step 0 multiplies a zero state: it contributes nothing and its slot holds no r*h)
  WgradPair* const table0 = (WgradPair*)L.p(ws, L.off_tab);
  float* slabs = L.p(ws, L.off_slab);
  std::vector<WgradPair> host((size_t)4 * T);
  memset(host.data(), 0, host.size() * sizeof(WgradPair));
  cat_wgrad_entries(host.data(), T, cat.data(), T);
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
  reduce_gn_partials(pgg, pgc, T * batch, H, gr->gn_gates_w, gr->gn_gates_b, gr->gn_can_w, gr->gn_can_b, stream);
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}
