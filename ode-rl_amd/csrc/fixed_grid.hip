// fixed_grid.hip -- euler / midpoint / rk4(3/8) trajectories (torchdiffeq FixedGridODESolver, one step per output
// interval; call sites modules/DiffEqSolver.py:37,45-46 of the reference) and their BACKWARD passes.
//
// The methods live in ONE place, fixed_tableau.h: the tableaus and the three plans derived from them (stage combines, reverse-sweep
// targets, adjoint targets).  The drivers below are loops over stages that turn a plan's slots into workspace pointers; the bf16
// whole-trajectory kernels (fstack_bf16.hip, btraj_bf16.hip) read the same header.
//
// Backward = what the reference gets from `loss.backward()` (train_test.py:204): reverse-mode differentiation
// through every op of the discrete solver ("discretise-then-optimise"; the reference imports `odeint`, not
// `odeint_adjoint`: modules/DiffEqSolver.py:9).  Here it is an explicit reverse sweep:
//   * the forward pass (save_for_backward) keeps every layer input A[n][s][l] of every evaluation of f in the
//     workspace (HBM is 288 GB; B=64,T=10 needs 0.7 GB) -- nothing is recomputed;
//   * per evaluation, the input-gradient chain is the SAME MFMA conv kernel run on transposed+flipped weights
//     (odehip_pack_conv_weight(transpose_flip=1)) with the ReLU mask fused in the epilogue, and the reverse
//     Runge-Kutta bookkeeping (gy += gx, gk_j += c h gx, seed of the next interval) fused into the epilogue of
//     the chain's last conv -- no standalone elementwise kernels;
//   * all weight gradients are ONE launch per layer over all evaluations (wgrad.hip).
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "fixed_tableau.h"
#include "odehip_internal.h"
#include "persist.h"

namespace odehip {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kEsplit = 4;
constexpr int kMaxTimes = 4096;           // output times of one call (the step sizes travel in a stack buffer)
constexpr int kMaxWgradEvals = 32 * 64;   // evaluations one weight-gradient table (and the adjoint's weight list) holds
static_assert(kFixedMaxStages - 1 == 3, "the workspace keeps three stage derivatives (off_k) and three partial sums (off_gy, off_g2)");

// Everything lives in the caller's workspace; this is the one place that knows where.
struct FixedLayout {
  int T, B, C, S, NH, NG, save;  // NH = hidden activations per evaluation of f (n_convs - 1); NG = gradient slots (grad_slots)
  size_t st;                 // bytes of one (B,C,16,16) tensor
  size_t hid;                // bytes of one hidden activation (B,max_hidden,16,16)
  size_t off_h, off_ping, off_pong, off_xs, off_k, off_y, off_xin, off_hid, off_gp, off_go, off_gy, off_g2, off_tab, off_slab, off_psync, total;
  FixedLayout(const odehip_convstack* f, int batch, int n_times, int method, int save_) {
    T = n_times; B = batch; C = f->channels[0]; S = n_stages(method); NH = f->n_convs - 1; NG = grad_slots(f); save = save_;
    st = al256((size_t)B * C * kPix * 4);
    int cmax = 32;
    for (int i = 0; i <= f->n_convs; ++i) cmax = f->channels[i] > cmax ? f->channels[i] : cmax;
    hid = al256((size_t)B * cmax * kPix * 4);   // one slot fits any activation / gradient of the stack
    size_t o = 0;
    auto take = [&](size_t b) { size_t r = o; o += al256(b); return r; };
    off_h = take((size_t)T * 4);
    off_ping = take(hid);
    off_pong = take(hid);
    off_xs = take(st);
    off_k = take(3 * st);
    off_y = take((size_t)T * st);
    off_xin = off_hid = off_gp = off_go = off_gy = off_g2 = off_tab = off_slab = 0;
    off_psync = take(persist_sync_bytes(B));  // persistent kernel: flag line per sample + xcc_of[grid] + abort word
    if (save) {
      const size_t ne = (size_t)(T - 1) * S;
      off_xin = take(ne * st);             // stage inputs (slot s = 0 unused: it is y[n])
      off_hid = take(ne * NH * hid);       // ReLU outputs of every evaluation
      off_gp = take(ne * NG * hid);        // gradients w.r.t. every conv output (filled by the backward sweep)
      off_go = take((size_t)T * st);       // grad_out in Q4
      off_gy = take(st);
      off_g2 = take(2 * st);
      off_tab = take(ne * sizeof(WgradPair) * ODEHIP_MAX_LAYERS);   // one table per layer, uploaded together
      off_slab = take(wgrad_slab_bytes(B));
    }
    total = o;
  }
  float* p(void* ws, size_t off) const { return (float*)((char*)ws + off); }
  float* y(void* ws, int n) const { return p(ws, off_y + (size_t)n * st); }
  float* xin(void* ws, int n, int s) const { return s == 0 ? y(ws, n) : p(ws, off_xin + ((size_t)n * S + s) * st); }
  float* hidden(void* ws, int n, int s, int l) const { return p(ws, off_hid + (((size_t)n * S + s) * NH + l) * hid); }
  float* gp(void* ws, int n, int s, int l) const { return p(ws, off_gp + (((size_t)n * S + s) * NG + l) * hid); }
  float* go(void* ws, int j) const { return p(ws, off_go + (size_t)j * st); }
};

// out = (c_c + c_h*h) * in
__global__ __launch_bounds__(256) void scale_kernel(float* __restrict__ out, const float* __restrict__ in, float c_c, float c_h,
                                                    const float* h_ptr, long long n4) {
  const float c = c_c + c_h * (h_ptr ? *h_ptr : 0.0f);
  for (long long i = blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256)
    ((f32x4*)out)[i] = ((const f32x4*)in)[i] * c;
}

struct PtrPack {
  unsigned long long v[32];
};
__global__ void fill_u64_kernel(unsigned long long* dst, PtrPack p, int n) {
  if ((int)threadIdx.x < n) dst[threadIdx.x] = p.v[threadIdx.x];
}

// table[e] = {g0 + e*gs, a0 + e*as, scale 1}: the evaluations of one layer are evenly spaced in the workspace, so the table is
// built by one tiny launch instead of being shipped 32 values at a time through kernel arguments
__global__ void wgrad_table_kernel(WgradPair* table, int n_eval, const char* g0, unsigned long long gs, const char* a0,
                                   unsigned long long as) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_eval) return;
  WgradPair p;
  p.g = (const float*)(g0 + (size_t)e * gs);
  p.a = (const float*)(a0 + (size_t)e * as);
  p.scale = 1.0f;
  p.pad_[0] = p.pad_[1] = p.pad_[2] = 0.0f;
  table[e] = p;
}

static int check_common(const odehip_convstack* f, int method, const double* t_host, int n_times, int batch, const char* who) {
  int rc = check_stack(f);
  if (rc != ODEHIP_OK) return rc;
  ODEHIP_REQUIRE(is_fixed_method(method), "%s: method %d is not a fixed-grid method", who, method);
  ODEHIP_REQUIRE(t_host, "%s: null t", who);
  ODEHIP_REQUIRE(n_times >= 1 && n_times <= kMaxTimes && batch > 0, "%s: bad sizes (n_times %d, batch %d)", who, n_times, batch);
  ODEHIP_REQUIRE(f->channels[0] == f->channels[f->n_convs], "%s: f must map C -> C channels (%d -> %d)", who, f->channels[0],
                 f->channels[f->n_convs]);
  for (int i = 1; i < n_times; ++i)
    ODEHIP_REQUIRE(t_host[i] > t_host[i - 1], "%s: t must be strictly increasing (t[%d]=%g, t[%d]=%g)", who, i - 1, t_host[i - 1],
                   i, t_host[i]);
  return ODEHIP_OK;
}

// dW_l, db_l = sum over evaluations e = (n, s) of scale_e * wgrad(GP[n][s][l], A[n][s][l]); one launch per layer.
// A[n][s][0] is the stage input; for s = 0 that is y[n] (forward sweep), or stage0[n] where the caller says so (adjoint, integrating
// backwards: the state at the step's right end).
static int wgrad_all_layers(const odehip_convstack* f, const FixedLayout& L, void* ws, int n_times, int batch,
                            const float* const* stage0 /* host, T-1 entries or null */,
                            const float* eval_scale /* host, (T-1)*S entries or null = 1 */, float* const* grad_w,
                            float* const* grad_b, hipStream_t stream) {
  const int S = L.S, NL = f->n_convs;
  const int n_eval = (n_times - 1) * S;
  ODEHIP_REQUIRE(n_eval <= kMaxWgradEvals, "odeint backward: too many evaluations (%d)", n_eval);
  WgradPair* table = (WgradPair*)L.p(ws, L.off_tab);
  float* slabs = L.p(ws, L.off_slab);
  // the NL tables (g, a, scale per evaluation) travel in ONE asynchronous staged upload (25 kernel-argument uploads per training step before)
  std::vector<WgradPair> host((size_t)NL * n_eval);
  for (int l = 0; l < NL; ++l)
    for (int e = 0; e < n_eval; ++e) {
      const int n = e / S, s = e % S;
      WgradPair& p = host[(size_t)l * n_eval + e];
      p.g = L.gp(ws, n, s, wgrad_slot(f, l));
      p.a = l > 0 ? L.hidden(ws, n, s, l - 1) : (s > 0 ? L.xin(ws, n, s) : stage0 ? stage0[n] : L.y(ws, n));
      p.scale = eval_scale ? eval_scale[e] : 1.0f;
      p.pad_[0] = p.pad_[1] = p.pad_[2] = 0.0f;
    }
  int rc = staged_upload(table, host.data(), host.size() * sizeof(WgradPair), stream);
  if (rc != ODEHIP_OK) return rc;
  const int esplit = f->w_bf16[0] ? kEsplit : wgrad_esplit(batch, n_eval);
  for (int l = 0; l < NL && !(g_debug_flags & 32); ++l) {
    rc = launch_wgrad(table + (size_t)l * n_eval, n_eval, batch, esplit, slabs, grad_w[l], grad_b[l], f->channels[l + 1], f->channels[l], stream,
                      f->w_bf16[l] != nullptr);
    if (rc != ODEHIP_OK) return rc;
  }
  return ODEHIP_OK;
}

// step sizes: dt = t1 - t0 in float64, rounded to fp32 when it meets the state (torchdiffeq semantics).  sign = -1: the backward
// passes of a NEGATED solve.  A Runge-Kutta step sees the dynamics only as h * f, so dz/ds = -f(z) stepped by h is f stepped by -h:
// with -h in the step-size buffers every seed of a slope (all of them proportional to h), every weight of a weight gradient and
// every recomputed stage carries the sign of the negated dynamics, and the rows without h (gy += gx) carry none -- as they must
static void fill_step_sizes(float* hbuf, const double* t_host, int n_times, float sign = 1.0f) {
  for (int i = 0; i + 1 < n_times; ++i) hbuf[i] = sign * (float)(t_host[i + 1] - t_host[i]);
}

// the stacks the backward passes take (f checked by check_common)
static int check_backward_stack(const odehip_convstack* f, const char* who) {
  for (int l = 0; l <= f->n_convs; ++l)
    ODEHIP_REQUIRE(f->channels[l] % 64 == 0, "%s: channel counts must be multiples of 64 (channels[%d] = %d)", who, l, f->channels[l]);
  ODEHIP_REQUIRE(f->ks == 3, "%s: 3x3 dynamics only", who);
  return ODEHIP_OK;
}

// The CombineArgs of stage s from its plan: `base` carries y, h_ptr and k_scale, k[j] is where k_j is kept, x_next the next stage's
// input; the last stage writes the step result instead.
static CombineArgs stage_combine(const FixedCombine& p, int s, const CombineArgs& base, float* const* k, float* x_next, float* ynew,
                                 float* ynew_nchw) {
  CombineArgs c = base;
  c.n_prev = p.n_prev;
  for (int i = 0; i < p.n_prev; ++i) c.k_prev[i] = k[p.prev[i]];
  float* w = p.result ? c.c2 : c.c1;
  for (int i = 0; i <= p.n_prev; ++i) w[i] = p.c[i];
  if (p.keep_k) c.k_out = k[s];
  c.out1 = p.result ? nullptr : x_next;
  c.out2 = p.result ? ynew : nullptr;
  c.out2_nchw = p.result ? ynew_nchw : nullptr;
  return c;
}

// The BwdArgs of a chain from its plan: slot(i) resolves a plan's slot to its tensor; the interval's result (kSlotOut) also takes
// grad_out[n] = `go`, weighted like its source (null: a step that ends inside an output interval, where no gradient arrives)
template <class Slot>
static BwdArgs resolve_targets(const FixedTargets& p, const float* h_ptr, const float* go, Slot slot) {
  BwdArgs w;
  memset(&w, 0, sizeof(w));
  w.h_ptr = h_ptr;
  w.n_targets = p.n;
  for (int i = 0; i < p.n; ++i) {
    const FixedTarget& t = p.t[i];
    BwdTarget& b = w.tgt[i];
    b.out = slot(t.out); b.srcA = slot(t.src);
    b.a_c = t.a_c; b.a_h = t.a_h; b.g_c = t.g_c; b.g_h = t.g_h;
    if (t.out == kSlotOut && go) { b.srcB = go; b.b_c = t.a_c; b.b_h = t.a_h; }
  }
  return w;
}

}  // namespace odehip

using namespace odehip;

extern "C" size_t odehip_odeint_workspace_bytes(const odehip_convstack* f, int batch, int n_times, int method,
                                                int save_for_backward) {
  if (!f || batch <= 0 || n_times <= 0 || f->n_convs < 1) return 0;
  return FixedLayout(f, batch, n_times, method, save_for_backward).total;
}

// the saved tensors of a forward pass are bf16 "Q4h" written by the whole-trajectory launch (format 1) when: bf16 fused stack,
// every layer 64 -> 64, rk4, and the persistent switch is on
static bool bf16_trajectory_ok(const odehip_convstack* f, int method) {
  if (!f->w_fused || f->ks != 3 || g_debug_flags || !persist_switch_on()) return false;
  for (int l = 0; l <= f->n_convs; ++l)
    if (f->channels[l] != 64) return false;
  return is_fixed_method(method);
}

// who: the entry's name in its messages.  negated_saving: the caller is odehip_odeint_fixed_negated_saving, whose backward carries
// the sign; its stack must be one the backward takes (fp32 images, 3x3, channel counts that are multiples of 64)
static int fixed_forward(const odehip_convstack* f, int method, const float* z0_nchw, const double* t_host, int n_times, int batch,
                         float* out_nchw, int save_for_backward, int negate, void* workspace, size_t workspace_bytes,
                         int* saved_format_out, void* stream_, const char* who, bool negated_saving) {
  if (saved_format_out) *saved_format_out = 0;
  int rc = check_common(f, method, t_host, n_times, batch, who);
  ODEHIP_REQUIRE(negated_saving || !(negate && save_for_backward), "%s: backward through negated dynamics is not supported", who);
  if (rc != ODEHIP_OK) return rc;
  if (negated_saving && ((rc = check_fp32_stacks(f, nullptr, who)) != ODEHIP_OK || (rc = check_backward_stack(f, who)) != ODEHIP_OK)) return rc;
  ODEHIP_REQUIRE(z0_nchw && out_nchw && workspace, "%s: null pointer", who);
  ODEHIP_REQUIRE(saved_format_out || !save_for_backward, "%s: saved_format_out is required with save_for_backward", who);
  const FixedLayout L(f, batch, n_times, method, save_for_backward);
  ODEHIP_REQUIRE(workspace_bytes >= L.total, "%s: workspace too small (%zu < %zu)", who, workspace_bytes, L.total);
  hipStream_t stream = (hipStream_t)stream_;
  void* ws = workspace;
  const size_t st_b = (size_t)batch * L.C * kPix * 4, st_f = st_b / 4;
  float* hdev = L.p(ws, L.off_h);
  float *ping = L.p(ws, L.off_ping), *pong = L.p(ws, L.off_pong);
  float* k[3] = {L.p(ws, L.off_k), L.p(ws, L.off_k + L.st), L.p(ws, L.off_k + 2 * L.st)};

  float hbuf[kMaxTimes];
  fill_step_sizes(hbuf, t_host, n_times);
  // ONE prologue launch: solution[0] = y0, y0 in the kernels' layout, the step sizes on the device, the persistent launch's flags zeroed
  const bool h_in_prologue = n_times - 1 <= 64;
  unsigned* psync = (unsigned*)L.p(ws, L.off_psync);
  rc = traj_prologue(z0_nchw, L.y(ws, 0), out_nchw, batch, L.C, hbuf, h_in_prologue ? n_times - 1 : 0, hdev, psync,
                     (int)(persist_sync_bytes(batch) / 4), stream);
  if (rc != ODEHIP_OK) return rc;
  if (n_times == 1) return ODEHIP_OK;
  if (!h_in_prologue) {
    rc = upload_floats(hdev, hbuf, n_times - 1, stream);
    if (rc != ODEHIP_OK) return rc;
  }

  // bf16 compute, 64-channel stack: the whole trajectory as ONE launch with one workgroup per sample -- state and stage derivatives
  // in registers, activations in LDS (fstack_bf16.hip: ftraj_bf16_kernel).  A training forward (rk4) also saves every stage input
  // and hidden activation as bf16 for the one-launch reverse sweep (btraj_bf16.hip): saved format 1.
  if (bf16_trajectory_ok(f, method) && (!save_for_backward || (method == ODEHIP_RK4 && (n_times - 1) * L.S <= kMaxWgradEvals))) {
    if (save_for_backward) {
      rc = launch_ftraj_bf16_saving(f, z0_nchw, out_nchw, hdev, n_times, batch, L.p(ws, L.off_xin), L.st, L.p(ws, L.off_hid),
                                    (size_t)L.NH * L.hid, L.hid, stream);
      if (rc == ODEHIP_OK) *saved_format_out = 1;   // non-null: checked with the arguments, before anything was enqueued
    } else {
      rc = launch_ftraj_bf16(f, method, z0_nchw, out_nchw, hdev, n_times, batch, negate, stream);
    }
    if (rc == ODEHIP_OK) persist_count_launch();
    return rc;
  }

  // One launch for the whole trajectory when the dynamics are the 64-channel fp32 stack: the loop below then only RECORDS its
  // layers (with save_for_backward only the destinations of the hidden layers differ).
  PersistScope persist;
  if ((rc = persist.begin(f, nullptr, (n_times - 1) * L.S * f->n_convs)) != ODEHIP_OK) return rc;
  float* hidv[ODEHIP_MAX_LAYERS];
  FixedCombine plan[kFixedMaxStages];
  for (int s = 0; s < L.S; ++s) plan[s] = fixed_combine(fixed_tableau(method), s);
  auto enqueue_steps = [&]() -> int {
  for (int n = 0; n + 1 < n_times; ++n) {
    const float* y = L.y(ws, n);
    float* ynew = L.y(ws, n + 1);
    float* ynew_nchw = out_nchw + (size_t)(n + 1) * st_f;
    // stage input / hidden-activation buffers of stage s (distinct per evaluation when saving)
    auto xin = [&](int s) { return save_for_backward ? L.xin(ws, n, s) : L.p(ws, L.off_xs); };
    CombineArgs base;
    memset(&base, 0, sizeof(base));
    base.y = y;
    base.h_ptr = hdev + n;
    base.k_scale = negate ? -1.0f : 1.0f;
    for (int s = 0; s < L.S; ++s) {   // k_s = f(x_s); its epilogue forms x_{s+1}, or y[n+1] behind the last stage
      const CombineArgs c = stage_combine(plan[s], s, base, k, s + 1 < L.S ? xin(s + 1) : nullptr, ynew, ynew_nchw);
      for (int l = 0; l < L.NH && save_for_backward; ++l) hidv[l] = L.hidden(ws, n, s, l);
      rc = enqueue_f_saving(f, s == 0 ? y : xin(s), batch, save_for_backward ? hidv : nullptr, ping, pong, &c, nullptr, nullptr, stream);
      if (rc != ODEHIP_OK) return rc;
    }
  }
  return ODEHIP_OK;
  };
  rc = enqueue_steps();
  int rc2 = persist.finish(hbuf, hdev, out_nchw, batch, psync, f->ks, stream, /*sync_is_zero=*/true);
  if (rc == ODEHIP_OK && rc2 == ODEHIP_OK) {
    float* const regions[1] = {out_nchw};
    const size_t floats[1] = {(size_t)n_times * st_f};
    rc2 = persist.guard(regions, floats, 1, stream);
  }
  return rc != ODEHIP_OK ? rc : rc2;
}

extern "C" int odehip_odeint_fixed(const odehip_convstack* f, int method, const float* z0_nchw, const double* t_host,
                                   int n_times, int batch, float* out_nchw, int save_for_backward, int negate,
                                   void* workspace, size_t workspace_bytes, int* saved_format_out, void* stream_) {
  return fixed_forward(f, method, z0_nchw, t_host, n_times, batch, out_nchw, save_for_backward, negate, workspace, workspace_bytes,
                       saved_format_out, stream_, "odeint_fixed", false);
}

// ---------------------------------------------------------------------------------------------------------------
// What the two backward entries (reverse sweep, adjoint) share: the argument checks, the trivial one-time call, the input-gradient
// chain of one evaluation, and the tail behind the sweep.
//   f_dgrad: the stack of input-gradient convs, f_dgrad->w_packed[l] = pack(W_l, transpose_flip = 1), in the
//            forward layer order; bias pointers unused.
//   grad_out (T,B,C,16,16) NCHW -> grad_z0 (B,C,16,16) NCHW, grad_w[l] (OIHW), grad_b[l].
static int check_backward_args(const odehip_convstack* f, const odehip_convstack* f_dgrad, int method, const double* t_host, int n_times,
                               int batch, bool pointers, float* const* grad_w, float* const* grad_b, const char* who) {
  int rc = check_common(f, method, t_host, n_times, batch, who);
  if (rc != ODEHIP_OK) return rc;
  ODEHIP_REQUIRE(f_dgrad && pointers && grad_w && grad_b, "%s: null pointer", who);
  if ((rc = check_backward_stack(f, who)) != ODEHIP_OK) return rc;
  for (int l = 0; l < f->n_convs; ++l)
    ODEHIP_REQUIRE(f_dgrad->w_packed[l] && grad_w[l] && grad_b[l], "%s: layer %d has null pointers", who, l);
  return ODEHIP_OK;
}

struct BackwardPass {
  const odehip_convstack *f, *f_dgrad;
  const FixedLayout& L;
  void* ws;
  int n_times, batch;
  float* grad_z0_nchw;
  float* const* grad_w;
  float* const* grad_b;
  hipStream_t stream;
  float hbuf[kMaxTimes];   // the step sizes as the forward pass uploaded them

  // n_times == 1: the solution is y0 itself
  int trivial(const float* grad_out_nchw) const {
    ODEHIP_CHECK_HIP(hipMemcpyAsync(grad_z0_nchw, grad_out_nchw, (size_t)batch * L.C * kPix * 4, hipMemcpyDeviceToDevice, stream));
    for (int l = 0; l < f->n_convs; ++l) {
      ODEHIP_CHECK_HIP(hipMemsetAsync(grad_w[l], 0, (size_t)f->channels[l + 1] * f->channels[l] * 9 * 4, stream));
      ODEHIP_CHECK_HIP(hipMemsetAsync(grad_b[l], 0, (size_t)f->channels[l + 1] * 4, stream));
    }
    return ODEHIP_OK;
  }
  // input-gradient chain of evaluation (n, s): GP[n][s][NH] (the seed: gradient w.r.t. k_s / the adjoint A_s) -> ... -> gx = J_f(x_s)^T
  // seed, consumed by the targets of `last`
  int dgrad_chain(int n, int s, const BwdArgs& last) const {
    float* gpv[ODEHIP_MAX_LAYERS + 1];
    const float* hv[ODEHIP_MAX_LAYERS];
    for (int l = 0; l < L.NG; ++l) gpv[l] = L.gp(ws, n, s, l);
    for (int l = 0; l + 1 < f->n_convs; ++l) hv[l] = L.hidden(ws, n, s, l);
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.combine = 3;
    a.bwd = last;
    return enqueue_dgrad_chain(f, f_dgrad, batch, gpv, hv, a, stream);
  }
  // behind the sweep (rc: what recording it returned): the recorded launch, grad_z0 from the Q4 tensor `g`, the weight / bias
  // gradients -- one launch per layer over all (T-1)*S evaluations -- and the guard: every gradient is NaN-filled if the sweep ran
  // as a persistent launch that gave up
  int finish(PersistScope& persist, int rc, const float* g, const float* const* stage0, const float* eval_scale) const {
    const int rc2 = persist.finish(hbuf, L.p(ws, L.off_h), nullptr, batch, (unsigned*)L.p(ws, L.off_psync), f->ks, stream);
    if (rc != ODEHIP_OK || rc2 != ODEHIP_OK) return rc != ODEHIP_OK ? rc : rc2;
    rc = odehip_q4_to_nchw(g, grad_z0_nchw, batch, L.C, stream);
    if (rc != ODEHIP_OK) return rc;
    rc = wgrad_all_layers(f, L, ws, n_times, batch, stage0, eval_scale, grad_w, grad_b, stream);
    if (rc != ODEHIP_OK) return rc;
    float* regions[1 + 2 * ODEHIP_MAX_LAYERS] = {grad_z0_nchw};
    size_t floats[1 + 2 * ODEHIP_MAX_LAYERS] = {(size_t)batch * L.C * kPix};
    for (int l = 0; l < f->n_convs; ++l) {
      regions[1 + 2 * l] = grad_w[l];
      floats[1 + 2 * l] = (size_t)f->channels[l + 1] * f->channels[l] * f->ks * f->ks;
      regions[2 + 2 * l] = grad_b[l];
      floats[2 + 2 * l] = (size_t)f->channels[l + 1];
    }
    return persist.guard(regions, floats, 1 + 2 * f->n_convs, stream);
  }
};

// ---------------------------------------------------------------------------------------------------------------
// Backward of odehip_odeint_fixed(save_for_backward = 1) on the SAME workspace.
// sign = -1: the forward was the negated saving solve (fill_step_sizes)
static int fixed_backward(const odehip_convstack* f, const odehip_convstack* f_dgrad, int method, const double* t_host, int n_times,
                          int batch, const float* grad_out_nchw, float* grad_z0_nchw, float* const* grad_w, float* const* grad_b,
                          int saved_format, void* workspace, size_t workspace_bytes, void* stream_, float sign, const char* who) {
  int rc = check_backward_args(f, f_dgrad, method, t_host, n_times, batch, grad_out_nchw && grad_z0_nchw && workspace, grad_w, grad_b, who);
  if (rc != ODEHIP_OK) return rc;
  if (sign < 0.0f && (rc = check_fp32_stacks(f, f_dgrad, who)) != ODEHIP_OK) return rc;
  ODEHIP_REQUIRE(saved_format == 0 || saved_format == 1, "%s: unknown saved format %d", who, saved_format);
  const FixedLayout L(f, batch, n_times, method, 1);
  ODEHIP_REQUIRE(workspace_bytes >= L.total, "%s: workspace too small", who);
  hipStream_t stream = (hipStream_t)stream_;
  void* ws = workspace;
  const int NH = L.NH, S = L.S, NL = f->n_convs;
  float* hdev = L.p(ws, L.off_h);

  if (saved_format == 1 && n_times > 1) {
    // ---- the forward was the whole-trajectory bf16 launch: ONE launch for the reverse sweep (gradient state in registers, every
    // conv-output gradient stored as bf16 Q4h), then one weight-gradient launch per layer on the bf16 operands
    ODEHIP_REQUIRE(method == ODEHIP_RK4 && f->w_fused && f_dgrad->w_fused, "odeint_fixed_backward: saved format 1 belongs to the fused bf16 rk4 path");
    // The sweep occupies one CU per sample -- half the chip at 128 samples per GPU -- and the weight gradients only need what the
    // sweep has already written: the sweep is cut into up to four launches (its state crosses the cut in two state-sized tensors)
    // and the weight gradients of a finished segment run on a library-owned SIDE STREAM, on the idle CUs, while the next segment
    // is swept.  The concurrent weight-gradient launches are sized to the CUs the sweep leaves free (one workgroup per sample at
    // 128 samples) so that they cannot take the CUs the sweep's next launch needs; the last segment's run on the whole chip.  dW accumulates over the segments in order.
    // The side stream and its events are library state of ONE device (one process per GPU is the deployment model): created once
    // under a lock, bound to the device that was current then, and every later call must come from that device -- a call from
    // another one is refused instead of launching the weight gradients on the wrong device's stream.  Calls are serialised by the
    // caller (one host thread per process drives the library: SURVEY.md section 8b "Threading"); the lock only makes the lazy
    // creation itself safe.
    constexpr int kMaxSeg = 4;   // measured at B=128, T=40: 4 segments 9.3 ms, 6: 9.4, 8: 9.6, uncut 10.2
    static std::mutex side_mu;
    static hipStream_t side = nullptr;
    static int side_device = -1;
    static hipEvent_t ev_seg[kMaxSeg] = {}, ev_done = nullptr;
    {
      std::lock_guard<std::mutex> lk(side_mu);
      int cur_dev = -1;
      ODEHIP_CHECK_HIP(hipGetDevice(&cur_dev));
      if (!side) {
        int lo_pri = 0, hi_pri = 0;
        ODEHIP_CHECK_HIP(hipDeviceGetStreamPriorityRange(&lo_pri, &hi_pri));
        hipStream_t s_new = nullptr;
        ODEHIP_CHECK_HIP(hipStreamCreateWithPriority(&s_new, hipStreamNonBlocking, lo_pri));   // the sweep's launches go first
        for (int i = 0; i < kMaxSeg; ++i) ODEHIP_CHECK_HIP(hipEventCreateWithFlags(&ev_seg[i], hipEventDisableTiming));
        ODEHIP_CHECK_HIP(hipEventCreateWithFlags(&ev_done, hipEventDisableTiming));
        side_device = cur_dev;
        side = s_new;
      }
      ODEHIP_REQUIRE(cur_dev == side_device, "odeint_fixed_backward: the library's side stream belongs to device %d, this call runs on device %d "
                                               "(one process drives one GPU)", side_device, cur_dev);
    }
    const int n_steps = n_times - 1;
    const int n_eval = n_steps * S;
    ODEHIP_REQUIRE(n_eval <= kMaxWgradEvals, "odeint backward: too many evaluations (%d)", n_eval);
    int cus = 256;
    {
      int dev = 0;
      if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    }
    const int free_cus = cus - batch;                         // the sweep holds one CU per sample
    const int esplit_c = free_cus / batch < kEsplit ? free_cus / batch : kEsplit;   // concurrent weight-gradient workgroups per sample
    int n_seg = esplit_c >= 1 ? n_steps / 8 : 1;   // at least eight intervals per segment; no idle CUs: no cut
    n_seg = n_seg < 1 ? 1 : (n_seg > kMaxSeg ? kMaxSeg : n_seg);
    if (n_seg > n_steps) n_seg = n_steps;
    float* bias_part = L.p(ws, L.off_g2);                      // [segment][B][NL][64] fp32: fits the two state-sized scratch tensors
    float* state_g = L.go(ws, 0);                              // the per-launch path's Q4 copy of grad_out is not needed here:
    float* state_seed = L.go(ws, 1);                           // two of its T tensors carry the sweep's state across a cut
    WgradPair* table = (WgradPair*)L.p(ws, L.off_tab);
    float* slabs = L.p(ws, L.off_slab);
    int hi = n_steps;
    for (int k = 0; k < n_seg; ++k) {
      const int lo = (int)((long long)n_steps * (n_seg - 1 - k) / n_seg);
      rc = launch_btraj_bf16_rk4(f_dgrad, grad_out_nchw, grad_z0_nchw, hdev, n_times, batch, lo, hi, state_g, state_seed,
                                 L.p(ws, L.off_hid), (size_t)NH * L.hid, L.hid, L.p(ws, L.off_gp), (size_t)(NH + 1) * L.hid, L.hid,
                                 bias_part + (size_t)k * batch * NL * 64, stream);
      if (rc != ODEHIP_OK) return rc;
      const bool concurrent = n_seg > 1 && k + 1 < n_seg;     // another segment is swept while these weight gradients run
      hipStream_t ws_stream = n_seg > 1 ? side : stream;
      if (n_seg > 1) {
        ODEHIP_CHECK_HIP(hipEventRecord(ev_seg[k], stream));
        ODEHIP_CHECK_HIP(hipStreamWaitEvent(side, ev_seg[k], 0));
      }
      const int e_lo = lo * S, n_e = (hi - lo) * S;
      for (int l = 0; l < NL; ++l) {
        const char* g0 = (const char*)L.p(ws, L.off_gp) + ((size_t)e_lo * (NH + 1) + l) * L.hid;
        const char* a0 = l > 0 ? (const char*)L.p(ws, L.off_hid) + ((size_t)e_lo * NH + (l - 1)) * L.hid
                               : (const char*)L.p(ws, L.off_xin) + (size_t)e_lo * L.st;
        hipLaunchKernelGGL(wgrad_table_kernel, dim3((n_e + 255) / 256), dim3(256), 0, ws_stream, table, n_e, g0, (size_t)(NH + 1) * L.hid,
                           a0, l > 0 ? (size_t)NH * L.hid : L.st);
        rc = launch_wgrad_q4h(table, n_e, batch, concurrent ? (esplit_c >= 1 ? esplit_c : 1) : kEsplit, slabs, grad_w[l], /*accumulate=*/k > 0, ws_stream);
        if (rc != ODEHIP_OK) return rc;
      }
      hi = lo;
    }
    if (n_seg > 1) {   // the caller's stream continues only when the side stream is done with the workspace and the gradients
      ODEHIP_CHECK_HIP(hipEventRecord(ev_done, side));
      ODEHIP_CHECK_HIP(hipStreamWaitEvent(stream, ev_done, 0));
    }
    return launch_bias_reduce(bias_part, n_seg * batch, NL, grad_b, stream);
  }
  ODEHIP_REQUIRE(saved_format == 0 || n_times == 1, "odeint_fixed_backward: bad saved format");
  rc = odehip_nchw_to_q4(grad_out_nchw, L.go(ws, 0), n_times * batch, L.C, stream);
  if (rc != ODEHIP_OK) return rc;
  BackwardPass bp = {f, f_dgrad, L, ws, n_times, batch, grad_z0_nchw, grad_w, grad_b, stream, {}};
  if (n_times == 1) return bp.trivial(grad_out_nchw);
  fill_step_sizes(bp.hbuf, t_host, n_times, sign);
  // the forward left +h on the device (its combines carry k_scale = -1); the rows of this sweep read h through h_ptr
  if (sign < 0.0f && (rc = upload_floats(hdev, bp.hbuf, n_times - 1, stream)) != ODEHIP_OK) return rc;

  const FixedTableau& tab = fixed_tableau(method);
  FixedTargets plan[kFixedMaxStages];
  for (int s = 0; s < S; ++s) plan[s] = reverse_targets(tab, s);
  const float wlast = fixed_seed_weight(tab);   // weight of the last stage's k in the step
  float* gy = L.p(ws, L.off_gy);
  float* gbuf[2] = {L.p(ws, L.off_g2), L.p(ws, L.off_g2 + L.st)};
  // seed: gradient w.r.t. the last stage's k of the last interval = wlast * h * grad_out[T-1]
  hipLaunchKernelGGL(scale_kernel, dim3(1024), dim3(256), 0, stream, L.gp(ws, n_times - 2, S - 1, NH), L.go(ws, n_times - 1), 0.0f,
                     wlast, hdev + (n_times - 2), (long long)batch * L.C * kPix / 4);
  float* g = L.go(ws, n_times - 1);  // total gradient w.r.t. y[n+1]
  // the reverse sweep is nothing but conv launches (all bookkeeping lives in their epilogues): one persistent launch
  PersistScope persist;
  if ((rc = persist.begin(f, f_dgrad, (n_times - 1) * S * NL)) != ODEHIP_OK) return rc;
  auto sweep = [&]() -> int {
    for (int n = n_times - 2; n >= 0; --n) {
      float* gnext = gbuf[n & 1];
      auto slot = [&](int sl) -> float* {
        return sl >= 0 ? L.gp(ws, n, sl, NH) : sl == kSlotGy ? gy : sl == kSlotState ? g : sl == kSlotOut ? gnext : nullptr;
      };
      for (int s = S - 1; s >= 0; --s) {
        BwdArgs w = resolve_targets(plan[s], hdev + n, L.go(ws, n), slot);
        if (s == 0) {
          // the first stage's chain closes the interval, g(y[n]) = gy + gx + grad_out[n], and seeds the next one, which uses h[n-1]:
          // the same three terms, each weighted wlast * h
          w.h_ptr = n > 0 ? hdev + (n - 1) : nullptr;
          if (n > 0) {
            BwdTarget& seed = w.tgt[w.n_targets++] = w.tgt[0];
            seed.out = L.gp(ws, n - 1, S - 1, NH);
            seed.a_c = seed.b_c = seed.g_c = 0.0f;
            seed.a_h = seed.b_h = seed.g_h = wlast;
          }
        }
        if ((rc = bp.dgrad_chain(n, s, w)) != ODEHIP_OK) return rc;
      }
      g = gnext;
    }
    return ODEHIP_OK;
  };
  rc = sweep();   // moves g: read it only afterwards
  return bp.finish(persist, rc, g, nullptr, nullptr);
}

extern "C" int odehip_odeint_fixed_backward(const odehip_convstack* f, const odehip_convstack* f_dgrad, int method,
                                            const double* t_host, int n_times, int batch, const float* grad_out_nchw,
                                            float* grad_z0_nchw, float* const* grad_w, float* const* grad_b, int saved_format,
                                            void* workspace, size_t workspace_bytes, void* stream_) {
  return fixed_backward(f, f_dgrad, method, t_host, n_times, batch, grad_out_nchw, grad_z0_nchw, grad_w, grad_b, saved_format, workspace,
                        workspace_bytes, stream_, 1.0f, "odeint_fixed_backward");
}

// ---------------------------------------------------------------------------------------------------------------
// A negated solve under autograd (a strictly decreasing t: the caller passes -t).  The forward is odehip_odeint_fixed(negate = 1)
// with every activation kept; the backward is the reverse sweep above with -h for h.  The channel limits of the backward are
// checked by the forward already, so that a solve whose gradient cannot be formed stops before it runs.
extern "C" int odehip_odeint_fixed_negated_saving(const odehip_convstack* f, int method, const float* z0_nchw, const double* t_host,
                                                  int n_times, int batch, float* out_nchw, void* workspace, size_t workspace_bytes,
                                                  void* stream_) {
  int fmt = 0;
  return fixed_forward(f, method, z0_nchw, t_host, n_times, batch, out_nchw, 1, 1, workspace, workspace_bytes, &fmt, stream_,
                       "odeint_fixed_negated_saving", true);
}

extern "C" int odehip_odeint_fixed_negated_backward(const odehip_convstack* f, const odehip_convstack* f_dgrad, int method,
                                                    const double* t_host, int n_times, int batch, const float* grad_out_nchw,
                                                    float* grad_z0_nchw, float* const* grad_w, float* const* grad_b, void* workspace,
                                                    size_t workspace_bytes, void* stream_) {
  return fixed_backward(f, f_dgrad, method, t_host, n_times, batch, grad_out_nchw, grad_z0_nchw, grad_w, grad_b, 0, workspace,
                        workspace_bytes, stream_, -1.0f, "odeint_fixed_negated_backward");
}

// ---------------------------------------------------------------------------------------------------------------
// Adjoint backward (torchdiffeq `odeint_adjoint` semantics, _impl/adjoint.py; NEW capability -- the reference itself
// never uses it: modules/DiffEqSolver.py:9).  For i = T-1 .. 1 the augmented state (y, a_y, a_theta) is integrated
// from t[i] back to t[i-1] with the same fixed-grid method on the negated dynamics (torchdiffeq flips a decreasing
// time grid), y is then reset to the stored forward value y[i-1] and a_y += grad_out[i-1].
//   d a_y / dt     = -J_f(y)^T a_y          -> the dgrad chain (same MFMA conv kernel, transposed+flipped weights)
//   d a_theta / dt = -(df/dtheta)^T a_y     -> wgrad over every stage of every step, weighted dt*b_s, one launch
// The stages of y are recomputed from y[i] (nothing saved by the forward pass except the trajectory itself).
//
// The sweep runs over the steps of a BACKWARD GRID, given in increasing time: the output times and, with an internal grid
// (torchdiffeq hands `options` on to every backward interval), the points the caller placed between them.  Step n integrates from
// point n+1 back to point n.  Where point n is an output, y restarts there from the stored trajectory and a_y takes grad_out: the
// last stage's forward epilogue stores nothing.  Where it lies inside an interval, the solver's own y goes on: the last stage's
// epilogue writes y + dt sum_s b_s k'_s (the forward solve's result row) and a_y takes no grad_out term.  Either way a step is
// S * (NL forward + NL input-gradient) convolutions and nothing else.
// ---------------------------------------------------------------------------------------------------------------
namespace odehip {

// out_index[p]: the output time grid point p coincides with, or -1 inside an interval; null: the grid is t itself
static int adjoint_sweep(const odehip_convstack* f, const odehip_convstack* f_dgrad, int method, const double* grid_host, int n_grid,
                         const int* out_index, int n_times, int batch, const float* y_traj_nchw, const float* grad_out_nchw,
                         float* grad_z0_nchw, float* const* grad_w, float* const* grad_b, void* ws, const FixedLayout& L,
                         size_t off_traj, hipStream_t stream, float sign = 1.0f) {
  const int NH = L.NH, S = L.S, NL = f->n_convs;
  float* hdev = L.p(ws, L.off_h);
  float *ping = L.p(ws, L.off_ping), *pong = L.p(ws, L.off_pong);
  float* k[3] = {L.p(ws, L.off_k), L.p(ws, L.off_k + L.st), L.p(ws, L.off_k + 2 * L.st)};
  float* sums[3] = {L.p(ws, L.off_gy), L.p(ws, L.off_g2), L.p(ws, L.off_g2 + L.st)};   // Q_2, Q_3 and R: partial sums of the a_y stages

  int rc = odehip_nchw_to_q4(y_traj_nchw, L.p(ws, off_traj), n_times * batch, L.C, stream);
  if (rc != ODEHIP_OK) return rc;
  rc = odehip_nchw_to_q4(grad_out_nchw, L.go(ws, 0), n_times * batch, L.C, stream);
  if (rc != ODEHIP_OK) return rc;
  BackwardPass bp = {f, f_dgrad, L, ws, n_grid, batch, grad_z0_nchw, grad_w, grad_b, stream, {}};
  if (n_grid == 1) return bp.trivial(grad_out_nchw);
  // dt of the flipped grid, > 0.  sign = -1: the trajectory is a negated solve's; the negation (k_scale below) of the negated
  // dynamics is plain f, and with -dt in hdev and in the weights of the weight gradients all three parts of the state follow
  fill_step_sizes(bp.hbuf, grid_host, n_grid, sign);
  rc = upload_floats(hdev, bp.hbuf, n_grid - 1, stream);
  if (rc != ODEHIP_OK) return rc;

  auto output_of = [&](int p) { return out_index ? out_index[p] : p; };
  // y at grid point p: the stored trajectory at an output, else what the step that ended there left in the layout's y slot
  auto y_at = [&](int p) -> float* { return output_of(p) >= 0 ? L.p(ws, off_traj + (size_t)output_of(p) * L.st) : L.y(ws, p); };

  const FixedTableau& tab = fixed_tableau(method);
  FixedCombine fwd[kFixedMaxStages], carry[kFixedMaxStages];
  FixedTargets plan[kFixedMaxStages];
  for (int s = 0; s < S; ++s) {
    fwd[s] = fixed_combine(tab, s, /*with_result=*/false);
    carry[s] = fixed_combine(tab, s);
    plan[s] = adjoint_targets(tab, s);
  }
  // seed: a_y = grad_out[T-1] is the stage-1 adjoint of the last step
  ODEHIP_CHECK_HIP(hipMemcpyAsync(L.gp(ws, n_grid - 2, 0, NH), L.go(ws, n_times - 1), (size_t)batch * L.C * kPix * 4,
                                  hipMemcpyDeviceToDevice, stream));
  float scales[kMaxWgradEvals];
  std::vector<const float*> stage0((size_t)n_grid - 1);
  float* a_final = L.p(ws, L.off_xs);
  float* hidv[ODEHIP_MAX_LAYERS];
  // every step is conv launches only (recomputed stages + input-gradient chains, all bookkeeping in their epilogues)
  PersistScope persist;
  if ((rc = persist.begin(f, f_dgrad, (n_grid - 1) * S * NL * 2)) != ODEHIP_OK) return rc;
  auto sweep = [&]() -> int {
    for (int n = n_grid - 2; n >= 0; --n) {
      const float* y = stage0[n] = y_at(n + 1);              // integrate from point n+1 back to point n
      const bool interior = output_of(n) < 0;                // the step ends inside an output interval
      const float* go = interior ? nullptr : L.go(ws, output_of(n));
      float* a_next = n > 0 ? L.gp(ws, n - 1, 0, NH) : a_final;  // a_y at point n (+ grad_out there) seeds the next step
      auto slot = [&](int sl) -> float* {                    // stage 0's tensor is a_y at point n+1
        return sl >= kSlotQ ? sums[sl - kSlotQ - 2] : sl >= 0 ? L.gp(ws, n, sl, NH) : sl == kSlotState ? L.gp(ws, n, 0, NH)
                                                               : sl == kSlotR ? sums[2] : sl == kSlotOut ? a_next : nullptr;
      };
      CombineArgs last, base;
      memset(&last, 0, sizeof(last));
      last.k_scale = -1.0f;                                  // negated dynamics
      base = last;
      base.y = y;
      base.h_ptr = hdev + n;
      for (int s = 0; s < S; ++s) {
        scales[n * S + s] = bp.hbuf[n] * tab.b[s];
        // Y_{s+1} = y + dt sum_j a[s+1][j] k_j'.  Before an output the last stage only leaves its activations (y is reset to the
        // stored trajectory): its epilogue stores nothing, and with neither y nor a destination set it reads nothing either.  Inside
        // an interval the stages keep the k' the result row reads and the last one writes y at point n.
        CombineArgs c = last;
        if (interior) c = stage_combine(carry[s], s, base, k, s + 1 < S ? L.xin(ws, n, s + 1) : nullptr, L.y(ws, n), nullptr);
        else if (s + 1 < S) c = stage_combine(fwd[s], s, base, k, L.xin(ws, n, s + 1), nullptr, nullptr);
        for (int l = 0; l < NH; ++l) hidv[l] = L.hidden(ws, n, s, l);
        if ((rc = enqueue_f_saving(f, s == 0 ? y : L.xin(ws, n, s), batch, hidv, ping, pong, &c, nullptr, nullptr, stream)) != ODEHIP_OK)
          return rc;
        // K_s = J_f(Y_s)^T A_s, A_s = GP[n][s][NH]
        if ((rc = bp.dgrad_chain(n, s, resolve_targets(plan[s], hdev + n, go, slot))) != ODEHIP_OK) return rc;
      }
    }
    return ODEHIP_OK;
  };
  rc = sweep();
  return bp.finish(persist, rc, a_final, stage0.data(), scales);
}

// workspace of the sweep over n_grid points: the solver's layout for that many points; with interior points the Q4 trajectory sits
// behind it (without, it fills the layout's y slots)
static size_t adjoint_grid_bytes(const FixedLayout& L, int n_times) { return L.total + al256((size_t)n_times * L.st); }

}  // namespace odehip

// Workspace: odehip_odeint_workspace_bytes(..., save_for_backward = 1).
extern "C" int odehip_odeint_adjoint_backward(const odehip_convstack* f, const odehip_convstack* f_dgrad, int method,
                                              const double* t_host, int n_times, int batch, const float* y_traj_nchw,
                                              const float* grad_out_nchw, float* grad_z0_nchw, float* const* grad_w,
                                              float* const* grad_b, void* workspace, size_t workspace_bytes, void* stream_) {
  int rc = check_backward_args(f, f_dgrad, method, t_host, n_times, batch, y_traj_nchw && grad_out_nchw && grad_z0_nchw && workspace,
                               grad_w, grad_b, "odeint_adjoint_backward");
  if (rc != ODEHIP_OK) return rc;
  const FixedLayout L(f, batch, n_times, method, 1);
  ODEHIP_REQUIRE(workspace_bytes >= L.total, "odeint_adjoint_backward: workspace too small");
  ODEHIP_REQUIRE((n_times - 1) * L.S <= kMaxWgradEvals, "odeint_adjoint_backward: too many evaluations (%d)", (n_times - 1) * L.S);
  return adjoint_sweep(f, f_dgrad, method, t_host, n_times, nullptr, n_times, batch, y_traj_nchw, grad_out_nchw, grad_z0_nchw, grad_w,
                       grad_b, workspace, L, L.off_y, (hipStream_t)stream_);
}

// The adjoint backward of a NEGATED solve's trajectory (a strictly decreasing t; t_host is -t).  Workspace as above.
extern "C" int odehip_odeint_adjoint_backward_negated(const odehip_convstack* f, const odehip_convstack* f_dgrad, int method,
                                                      const double* t_host, int n_times, int batch, const float* y_traj_nchw,
                                                      const float* grad_out_nchw, float* grad_z0_nchw, float* const* grad_w,
                                                      float* const* grad_b, void* workspace, size_t workspace_bytes, void* stream_) {
  const char* who = "odeint_adjoint_backward_negated";
  int rc = check_backward_args(f, f_dgrad, method, t_host, n_times, batch, y_traj_nchw && grad_out_nchw && grad_z0_nchw && workspace,
                               grad_w, grad_b, who);
  if (rc != ODEHIP_OK) return rc;
  if ((rc = check_fp32_stacks(f, f_dgrad, who)) != ODEHIP_OK) return rc;
  const FixedLayout L(f, batch, n_times, method, 1);
  ODEHIP_REQUIRE(workspace_bytes >= L.total, "%s: workspace too small", who);
  ODEHIP_REQUIRE((n_times - 1) * L.S <= kMaxWgradEvals, "%s: too many evaluations (%d)", who, (n_times - 1) * L.S);
  return adjoint_sweep(f, f_dgrad, method, t_host, n_times, nullptr, n_times, batch, y_traj_nchw, grad_out_nchw, grad_z0_nchw, grad_w,
                       grad_b, workspace, L, L.off_y, (hipStream_t)stream_, -1.0f);
}

extern "C" size_t odehip_odeint_adjoint_grid_workspace_bytes(const odehip_convstack* f, int batch, int n_times, int n_grid, int method) {
  if (!f || batch <= 0 || n_times <= 0 || n_grid < n_times || f->n_convs < 1) return 0;
  return adjoint_grid_bytes(FixedLayout(f, batch, n_grid, method, 1), n_times);
}

// The adjoint backward on an internal grid.  grid_host: the n_grid points of every backward interval's grid, joined and in increasing
// time, from t[0] to t[T-1]; out_index[p]: the j with grid[p] == t[j], or -1 for a point inside an interval.  fp32 stacks only.
// Workspace: odehip_odeint_adjoint_grid_workspace_bytes.
extern "C" int odehip_odeint_adjoint_backward_on_grid(const odehip_convstack* f, const odehip_convstack* f_dgrad, int method,
                                                      const double* t_host, int n_times, const double* grid_host, int n_grid,
                                                      const int* out_index, int batch, const float* y_traj_nchw,
                                                      const float* grad_out_nchw, float* grad_z0_nchw, float* const* grad_w,
                                                      float* const* grad_b, void* workspace, size_t workspace_bytes, void* stream_) {
  const char* who = "odeint_adjoint_backward_on_grid";
  int rc = check_backward_args(f, f_dgrad, method, t_host, n_times, batch, y_traj_nchw && grad_out_nchw && grad_z0_nchw && workspace,
                               grad_w, grad_b, who);
  if (rc != ODEHIP_OK) return rc;
  ODEHIP_REQUIRE(grid_host && out_index, "%s: null grid", who);
  ODEHIP_REQUIRE(n_grid >= n_times && n_grid <= kMaxTimes, "%s: a grid of %d points cannot serve %d output times (at most %d points)", who,
                 n_grid, n_times, kMaxTimes);
  ODEHIP_REQUIRE(!f->w_fused && !f_dgrad->w_fused && !f->w_bf16[0], "%s: fp32 stacks only", who);
  const int S = n_stages(method);
  ODEHIP_REQUIRE((n_grid - 1) * S <= kMaxWgradEvals, "%s: too many evaluations (%d grid steps x %d stages = %d, at most %d)", who,
                 n_grid - 1, S, (n_grid - 1) * S, kMaxWgradEvals);
  int j = 0;   // the outputs appear in order, each on a grid point of its own time; the grid starts and ends on one
  for (int p = 0; p < n_grid; ++p) {
    ODEHIP_REQUIRE(p == 0 || grid_host[p] > grid_host[p - 1], "%s: the grid must be strictly increasing (grid[%d]=%g, grid[%d]=%g)", who,
                   p - 1, grid_host[p - 1], p, grid_host[p]);
    if (out_index[p] < 0) continue;
    ODEHIP_REQUIRE(j < n_times && out_index[p] == j && grid_host[p] == t_host[j], "%s: grid point %d (%g, output %d) is not output time %d",
                   who, p, grid_host[p], out_index[p], j);
    ++j;
  }
  ODEHIP_REQUIRE(j == n_times && out_index[0] == 0 && out_index[n_grid - 1] == n_times - 1,
                 "%s: the grid must start at t[0], end at t[%d] and hold every output time (%d of %d found)", who, n_times - 1, j, n_times);
  const FixedLayout L(f, batch, n_grid, method, 1);
  ODEHIP_REQUIRE(workspace_bytes >= adjoint_grid_bytes(L, n_times), "%s: workspace too small (%zu < %zu)", who, workspace_bytes,
                 adjoint_grid_bytes(L, n_times));
  return adjoint_sweep(f, f_dgrad, method, grid_host, n_grid, out_index, n_times, batch, y_traj_nchw, grad_out_nchw, grad_z0_nchw, grad_w,
                       grad_b, workspace, L, L.total, (hipStream_t)stream_);
}
