// adjoint_dopri5.hip -- adaptive (dopri5) adjoint backward: torchdiffeq `odeint_adjoint(..., method="dopri5",
// adjoint_options={"norm": "seminorm"})` semantics (_impl/adjoint.py).  New capability: the reference never uses the
// adjoint (/root/reference/modules/DiffEqSolver.py:9); BASELINE.json configs[2] asks for it.
//
// For i = T-1 .. 1 the augmented state (y, a_y, a_theta) is integrated from t[i] back to t[i-1] by a fresh dopri5 solve
// on the flipped time axis (negated dynamics): initial-step heuristic, attempted steps with the error ratio
//   max( rms(err_y / tol_y), rms(err_a / tol_a) )          (seminorm: the parameter block does not steer the steps)
// (or, with torchdiffeq's default MIXED norm, the max over y, a_y and every parameter tensor's own RMS);
// accept/reject and step-size update exactly as _adaptive_step/_optimal_step_size; the value at t[i-1] is the quartic
// dense output of the last accepted step.  y is then reset to the stored y[i-1] and a_y += grad_out[i-1].
//
// Per stage: f(Y_s) (conv stack, activations kept in the step's slot) and K^a_s = J_f(Y_s)^T A_s (dgrad chain, same MFMA
// conv kernels on transposed+flipped weights, ReLU mask fused); both last convs carry the Runge-Kutta stage combine and
// the error-norm partials in their epilogue.  a_theta is linear in the stages, so it is never integrated step by step:
// every accepted step contributes  sum_s w_s * wgrad(GP_s, A_s)  with w_s = dt*b_s (or dt*W_s(x) for the interpolated
// last step of an interval), and ONE wgrad launch per layer sums all of them at the end (wgrad.hip).
//
// Step control in this file is host-driven (one stream synchronisation per attempted step, as torchdiffeq itself does): an attempt
// is ~1 ms of GPU work, the sync costs ~30 us.  Accepted steps keep their slot (0.28 GB each at B=64); `max_accept`
// bounds the workspace.  The seminorm on a 64-channel fp32 stack is handed to the device-steered path (adjoint_device.hip) first, for
// either adaptive method; odehip_last_adjoint_controller() says which of the two took the last call.
#include <math.h>
#include <string.h>

#include <vector>

#include "odehip_internal.h"
#include "adjoint_layout.h"
#include "dopri5_reduce.h"

namespace odehip {

typedef float f32x4 __attribute__((ext_vector_type(4)));


// out = y + sum_j c[j]*k[j] (+ add)      (coefficients already include the step size)
struct AdjLin {
  const float* y;
  const float* k[ODEHIP_MAX_STAGES];
  float c[ODEHIP_MAX_STAGES];
  int n;
  const float* add;
  float* out;
};
__global__ __launch_bounds__(256) void adj_lincomb_kernel(AdjLin a, long long n4) {
  for (long long i = blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    f32x4 s = ((const f32x4*)a.y)[i];
    for (int j = 0; j < a.n; ++j) s += ((const f32x4*)a.k[j])[i] * a.c[j];
    if (a.add) s += ((const f32x4*)a.add)[i];
    ((f32x4*)a.out)[i] = s;
  }
}


// parameter block (mixed norm): tensor j = floats [off[j], off[j+1]) of the flattened parameter vector; one workgroup per tensor:
// out[j] = sum ((a - b) / (atol + rtol * max(|r0|, |r0 + d|)))^2      (b, d may be null)
struct ThetaSpans {
  int off[2 * ODEHIP_MAX_LAYERS + 1];
  int count;
};
__global__ __launch_bounds__(256) void theta_sumsq_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          const float* __restrict__ r0, const float* __restrict__ d, float atol,
                                                          float rtol, ThetaSpans sp, float* __restrict__ out) {
  __shared__ float sh[256];
  const int j = blockIdx.x;
  float s = 0.0f;
  for (int i = sp.off[j] + threadIdx.x; i < sp.off[j + 1]; i += 256) {
    const float r = r0[i];
    const float tol = atol + rtol * fmaxf(fabsf(r), d ? fabsf(r + d[i]) : fabsf(r));
    const float v = (a[i] - (b ? b[i] : 0.0f)) / tol;
    s += v * v;
  }
  sh[threadIdx.x] = s;
  const float sum = block_tree_sum(sh);
  if (threadIdx.x == 0) out[j] = sum;
}
// a += d
__global__ __launch_bounds__(256) void theta_add_kernel(float* __restrict__ a, const float* __restrict__ d, int n) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) a[i] += d[i];
}

static float* g_adj_host = nullptr;  // 256 B of pinned host memory for the per-attempt scalars
static int g_adj_controller = -1;    // who steered the last adaptive adjoint that got as far as its backward solves: 1 device, 0 host

}  // namespace odehip

using namespace odehip;

// (the slots of AdjLayout keep room for ODEHIP_MAX_STAGES stages whatever the method: a tableau with S stages uses the first S)
extern "C" size_t odehip_adjoint_adaptive_workspace_bytes(const odehip_convstack* f, int batch, int n_times, int max_accept, int method) {
  if (!f || batch <= 0 || n_times <= 0 || max_accept <= 0 || f->n_convs < 1 || !adaptive_tableau(method)) return 0;
  return AdjLayout(f, batch, n_times, max_accept).total;
}
extern "C" size_t odehip_adjoint_dopri5_workspace_bytes(const odehip_convstack* f, int batch, int n_times, int max_accept) {
  return odehip_adjoint_adaptive_workspace_bytes(f, batch, n_times, max_accept, ODEHIP_DOPRI5);
}

extern "C" int odehip_odeint_adjoint_dopri5_backward(const odehip_convstack* f, const odehip_convstack* f_dgrad,
                                                     const double* t_host, int n_times, int batch, float rtol, float atol,
                                                     const float* y_traj_nchw, const float* grad_out_nchw, float* grad_z0_nchw,
                                                     float* const* grad_w, float* const* grad_b, int max_accept, int mixed_norm,
                                                     int* stats_host, void* workspace, size_t workspace_bytes, void* stream_) {
  return odehip_odeint_adjoint_adaptive_backward(ODEHIP_DOPRI5, f, f_dgrad, t_host, n_times, batch, rtol, atol, y_traj_nchw, grad_out_nchw,
                                                 grad_z0_nchw, grad_w, grad_b, max_accept, mixed_norm, stats_host, workspace,
                                                 workspace_bytes, stream_);
}

extern "C" int odehip_last_adjoint_controller(void) { return g_adj_controller; }

// The host-driven loop below reads the tableau of the call's method (S stages; the comments count in dopri5's 7), and so does the
// device-steered seminorm path (adjoint_device.hip), which takes the seminorm calls of both methods where it is available.
extern "C" int odehip_odeint_adjoint_adaptive_backward(int method, const odehip_convstack* f, const odehip_convstack* f_dgrad,
                                                       const double* t_host, int n_times, int batch, float rtol, float atol,
                                                       const float* y_traj_nchw, const float* grad_out_nchw, float* grad_z0_nchw,
                                                       float* const* grad_w, float* const* grad_b, int max_accept, int mixed_norm,
                                                       int* stats_host, void* workspace, size_t workspace_bytes, void* stream_) {
  const char* const mname = adaptive_name(method);
  const Tableau* tbp = adaptive_tableau(method);
  ODEHIP_REQUIRE(tbp, "odeint_adjoint_adaptive_backward: unknown adaptive method code %d (ODEHIP_DOPRI5 or ODEHIP_BOSH3)", method);
  const Tableau& tb = *tbp;
  const int S = tb.stages;
  int rc = check_stack(f);
  if (rc != ODEHIP_OK) return rc;
  ODEHIP_REQUIRE(f_dgrad && t_host && y_traj_nchw && grad_out_nchw && grad_z0_nchw && grad_w && grad_b && workspace,
                 "odeint_adjoint_%s_backward: null pointer", mname);
  ODEHIP_REQUIRE(n_times >= 1 && batch > 0 && max_accept > 0, "odeint_adjoint_%s_backward: bad sizes", mname);
  ODEHIP_REQUIRE(rtol > 0 && atol >= 0, "odeint_adjoint_%s_backward: rtol must be > 0 and atol >= 0", mname);
  ODEHIP_REQUIRE(f->ks == 3 && f->channels[0] == f->channels[f->n_convs], "odeint_adjoint_%s_backward: 3x3 C -> C dynamics only", mname);
  for (int l = 0; l <= f->n_convs; ++l)
    ODEHIP_REQUIRE(f->channels[l] % 64 == 0, "odeint_adjoint_%s_backward: channel counts must be multiples of 64", mname);
  for (int i = 1; i < n_times; ++i)
    ODEHIP_REQUIRE(t_host[i] > t_host[i - 1], "odeint_adjoint_%s_backward: t must be strictly increasing", mname);
  const AdjLayout L(f, batch, n_times, max_accept);
  ODEHIP_REQUIRE(workspace_bytes >= L.total, "odeint_adjoint_%s_backward: workspace too small", mname);
  hipStream_t stream = (hipStream_t)stream_;
  void* ws = workspace;
  const int NH = L.g.NH, NL = f->n_convs;
  const size_t st_b = (size_t)batch * L.C * kPix * 4;
  const long long n4 = (long long)(st_b / 16);
  const double N = (double)(st_b / 4);
  if (!g_adj_host) ODEHIP_CHECK_HIP(hipHostMalloc((void**)&g_adj_host, 256, hipHostMallocDefault));

  float* hdev = L.p(ws, L.off_h);
  float* sums = L.p(ws, L.off_sums);
  float* ping = L.p(ws, L.off_ping);
  float* pong = L.p(ws, L.off_pong);
  float* ky[kMaxStages];
  float* ka[kMaxStages];
  for (int i = 0; i < kMaxStages; ++i) {
    ky[i] = L.p(ws, L.off_ky + (size_t)i * L.g.st);
    ka[i] = L.p(ws, L.off_ka + (size_t)i * L.g.st);
  }
  auto yq = [&](int n) { return L.p(ws, L.off_y + (size_t)n * L.g.st); };
  auto goq = [&](int n) { return L.p(ws, L.off_go + (size_t)n * L.g.st); };

  if (!mixed_norm && n_times > 1) {
    // seminorm on a 64-channel fp32 stack: step control on the device, evaluations on the adaptive persistent walk
    // (adjoint_device.hip); `ran` = 0 when that path is not available here -- the host loop below then takes the call.  The path reads
    // the call's tableau, so dopri5 and bosh3 take it under the same conditions.
    int ran = 0;
    rc = adjoint_adaptive_device(tb, f, f_dgrad, t_host, n_times, batch, rtol, atol, y_traj_nchw, grad_out_nchw, grad_z0_nchw, grad_w, grad_b,
                               max_accept, stats_host, workspace, workspace_bytes, stream, &ran);
    if (rc != ODEHIP_OK || ran) {   // (an error in there is the device path's too: it only returns ran = 0 with ODEHIP_OK)
      g_adj_controller = 1;
      return rc;
    }
  }
  g_adj_controller = 0;
  rc = odehip_nchw_to_q4(y_traj_nchw, yq(0), n_times * batch, L.C, stream);
  if (rc != ODEHIP_OK) return rc;
  rc = odehip_nchw_to_q4(grad_out_nchw, goq(0), n_times * batch, L.C, stream);
  if (rc != ODEHIP_OK) return rc;
  int nfe = 0, n_accept = 0, n_reject = 0;
  if (n_times == 1) {
    ODEHIP_CHECK_HIP(hipMemcpyAsync(grad_z0_nchw, grad_out_nchw, st_b, hipMemcpyDeviceToDevice, stream));
    for (int l = 0; l < NL; ++l) {
      ODEHIP_CHECK_HIP(hipMemsetAsync(grad_w[l], 0, (size_t)f->channels[l + 1] * f->channels[l] * 9 * 4, stream));
      ODEHIP_CHECK_HIP(hipMemsetAsync(grad_b[l], 0, (size_t)f->channels[l + 1] * 4, stream));
    }
    write_stats(stats_host, 0, 0, 0);
    return ODEHIP_OK;
  }

  // ---- helpers -------------------------------------------------------------------------------------------------
  float* hidv[ODEHIP_MAX_LAYERS];
  // aug dynamics at (Y, A) of (slot, stage): K^y = -f(Y) via `cy`, K^a = J^T A via `ca` (both CombineArgs epilogues)
  auto eval_aug = [&](int slot, int s, const float* Y, const CombineArgs& cy, const CombineArgs& ca) -> int {
    for (int l = 0; l < NH; ++l) hidv[l] = L.hidden(ws, slot, s, l);
    int r = enqueue_f_saving(f, Y, batch, hidv, ping, pong, &cy, nullptr, nullptr, stream);
    if (r != ODEHIP_OK) return r;
    float* gpv[ODEHIP_MAX_LAYERS + 1];
    for (int l = 0; l < L.g.NG; ++l) gpv[l] = L.gp(ws, slot, s, l);
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.combine = 1;
    a.cmb = ca;
    return enqueue_dgrad_chain(f, f_dgrad, batch, gpv, hidv, a, stream);
  };
  auto sumsq = [&](int j, const float* a, const float* b, const float* y) {
    hipLaunchKernelGGL(scaled_sumsq_kernel, dim3(256), dim3(256), 0, stream, a, b, y, atol, rtol, n4, L.part(ws, j));
  };
  // reduce `count` partial arrays and bring the sums to the host (one synchronisation)
  auto fetch = [&](int count, const int* which, const int* lens, float* out) -> int {
    SumSet ss;
    memset(&ss, 0, sizeof(ss));
    ss.count = count;
    for (int j = 0; j < count; ++j) {
      ss.p[j] = L.part(ws, which[j]);
      ss.n[j] = lens[j];
    }
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, stream, ss, sums, (const int*)nullptr);
    ODEHIP_CHECK_HIP(hipMemcpyAsync(g_adj_host, sums, (size_t)(mixed_norm ? 8 + 4 * NL : count) * 4, hipMemcpyDeviceToHost, stream));
    ODEHIP_CHECK_HIP(hipStreamSynchronize(stream));
    for (int j = 0; j < count; ++j) out[j] = g_adj_host[j];
    return ODEHIP_OK;
  };
  auto lincomb = [&](float* out, const float* y, int n, float* const* k, const float* c, const float* add) {
    AdjLin a;
    memset(&a, 0, sizeof(a));
    a.y = y;
    a.n = n;
    for (int j = 0; j < n; ++j) {
      a.k[j] = k[j];
      a.c[j] = c[j];
    }
    a.add = add;
    a.out = out;
    hipLaunchKernelGGL(adj_lincomb_kernel, dim3(1024), dim3(256), 0, stream, a, n4);
  };
  auto rms = [&](float s) { return sqrtf((float)((double)s / N)); };

  // ---- parameter block of the augmented state (mixed norm only)
  const int P = L.P, NT = 2 * NL;
  float* th_run = L.p(ws, L.off_theta);            // a_theta accumulated so far
  float* th_err = th_run + P;                      // error estimate of the attempt
  float* th_inc = th_err + P;                      // its increment h * sum b_s K_s (or the dense-output weights)
  float* th_k1 = th_inc + P;                       // K^theta at the interval start / at the Euler point of the initial-step search
  float* th_kf = th_k1 + P;
  ThetaSpans spans;
  memset(&spans, 0, sizeof(spans));
  spans.count = NT;
  {
    int o = 0;
    for (int l = 0; l < NL; ++l) {
      spans.off[2 * l] = o;
      o += f->channels[l + 1] * f->channels[l] * 9;
      spans.off[2 * l + 1] = o;
      o += f->channels[l + 1];
    }
    spans.off[NT] = o;
  }
  if (mixed_norm) ODEHIP_CHECK_HIP(hipMemsetAsync(th_run, 0, (size_t)P * 4, stream));
  struct StageRef {   // one stage evaluation in a weight-gradient sum
    int slot, stage;
    const float* x0;  // input of conv 0 of that evaluation
    float scale;
  };
  // entry i of layer l's table
  auto wgrad_pair = [&](WgradPair& p, const StageRef& e, int l) {
    L.g.wgrad_pair(p, L.slot(ws, e.slot), e.stage, l, wgrad_slot(f, l), e.x0, e.scale);
  };
  // out (flattened parameter layout) = sum_i scale_i * wgrad(evaluation i): one batched launch per layer
  auto theta_wgrad = [&](const StageRef* ev, int n_ev, float* out) -> int {
    WgradPair* tab = (WgradPair*)L.p(ws, L.off_tab);
    float* slab = L.p(ws, L.off_slab);
    for (int l = 0; l < NL; ++l) {
      WgradPair host[kMaxStages];
      for (int i = 0; i < n_ev; ++i) wgrad_pair(host[i], ev[i], l);
      float bits[kMaxStages * sizeof(WgradPair) / 4];
      memcpy(bits, host, (size_t)n_ev * sizeof(WgradPair));
      int r = upload_floats((float*)tab, bits, n_ev * (int)(sizeof(WgradPair) / 4), stream);
      if (r != ODEHIP_OK) return r;
      r = launch_wgrad(tab, n_ev, batch, 4, slab, out + spans.off[2 * l], out + spans.off[2 * l + 1], f->channels[l + 1],
                       f->channels[l], stream, f->w_bf16[l] != nullptr);
      if (r != ODEHIP_OK) return r;
    }
    return ODEHIP_OK;
  };
  // per-tensor sums of ((a - b) / tol)^2 into sums[8 .. 8+NT)
  auto theta_sums = [&](const float* a, const float* b, const float* r0, const float* d, int which) {  // -> sums[8 + which*NT ..)
    hipLaunchKernelGGL(theta_sumsq_kernel, dim3(NT), dim3(256), 0, stream, a, b, r0, d, atol, rtol, spans, sums + 8 + which * NT);
  };
  auto theta_rms_max = [&](const volatile float* host_sums) {
    float m = 0.0f;
    for (int j = 0; j < NT; ++j) m = fmaxf(m, sqrtf((float)((double)host_sums[j] / (double)(spans.off[j + 1] - spans.off[j]))));
    return m;
  };

  std::vector<StageRef> entries;

  const float* a_cur = goq(n_times - 1);
  int slot = 0;
  for (int n = n_times - 2; n >= 0; --n) {
    const float* y_cur = yq(n + 1);
    const double t_begin = -t_host[n + 1], t_end = -t_host[n];
    ODEHIP_REQUIRE(slot < L.max_slots, "odeint_adjoint_%s_backward: more than max_accept = %d accepted steps", mname, max_accept);
    // ---- k1 = aug dynamics at the interval start (fresh odeint in torchdiffeq): stage 0 of `slot`
    ODEHIP_CHECK_HIP(hipMemcpyAsync(L.gp(ws, slot, 0, NH), a_cur, st_b, hipMemcpyDeviceToDevice, stream));
    CombineArgs cy, ca;
    memset(&cy, 0, sizeof(cy));
    memset(&ca, 0, sizeof(ca));
    cy.k_scale = -1.0f;
    cy.k_out = ky[0];
    ca.k_scale = 1.0f;
    ca.k_out = ka[0];
    if ((rc = eval_aug(slot, 0, y_cur, cy, ca)) != ODEHIP_OK) return rc;
    int k1_slot = slot, k1_stage = 0;
    const float* k1_x0 = y_cur;
    nfe += 1;
    // ---- _select_initial_step on (y, a) with the seminorm
    sumsq(0, y_cur, nullptr, y_cur);
    sumsq(1, a_cur, nullptr, a_cur);
    sumsq(2, ky[0], nullptr, y_cur);
    sumsq(3, ka[0], nullptr, a_cur);
    if (mixed_norm) {  // parameter block: state a_theta, derivative K^theta_1 = wgrad at the interval start
      const StageRef e0 = {slot, 0, y_cur, 1.0f};
      if ((rc = theta_wgrad(&e0, 1, th_k1)) != ODEHIP_OK) return rc;
      theta_sums(th_run, nullptr, th_run, nullptr, 0);
      theta_sums(th_k1, nullptr, th_run, nullptr, 1);
    }
    {
      const int which[4] = {0, 1, 2, 3}, lens[4] = {256, 256, 256, 256};
      float s4[4];
      if ((rc = fetch(4, which, lens, s4)) != ODEHIP_OK) return rc;
      float d0 = fmaxf(rms(s4[0]), rms(s4[1])), d1 = fmaxf(rms(s4[2]), rms(s4[3]));
      if (mixed_norm) {
        d0 = fmaxf(d0, theta_rms_max(g_adj_host + 8));
        d1 = fmaxf(d1, theta_rms_max(g_adj_host + 8 + NT));
      }
      const float h0 = initial_step_h0(d0, d1);
      float* k0y[1] = {ky[0]};
      float* k0a[1] = {ka[0]};
      lincomb(L.xin(ws, slot, 1), y_cur, 1, k0y, &h0, nullptr);
      lincomb(L.gp(ws, slot, 1, NH), a_cur, 1, k0a, &h0, nullptr);
      cy.k_out = ky[1];
      ca.k_out = ka[1];
      if ((rc = eval_aug(slot, 1, L.xin(ws, slot, 1), cy, ca)) != ODEHIP_OK) return rc;
      nfe += 1;
      sumsq(0, ky[1], ky[0], y_cur);
      sumsq(1, ka[1], ka[0], a_cur);
      if (mixed_norm) {
        const StageRef e1 = {slot, 1, L.xin(ws, slot, 1), 1.0f};
        if ((rc = theta_wgrad(&e1, 1, th_kf)) != ODEHIP_OK) return rc;
        theta_sums(th_kf, th_k1, th_run, nullptr, 0);
      }
      float s2[2];
      if ((rc = fetch(2, which, lens, s2)) != ODEHIP_OK) return rc;
      float d2 = fmaxf(rms(s2[0]), rms(s2[1]));
      if (mixed_norm) d2 = fmaxf(d2, theta_rms_max(g_adj_host + 8));
      d2 /= h0;
      g_adj_host[32] = initial_step_dt(h0, d1, d2, tb.order);
    }
    double dt = (double)g_adj_host[32];
    double t_cur = t_begin;
    // ---- attempted steps until t_end is covered
    for (;;) {
      ODEHIP_REQUIRE(slot < L.max_slots, "odeint_adjoint_%s_backward: more than max_accept = %d accepted steps", mname, max_accept);
      ODEHIP_REQUIRE(t_cur + dt > t_cur, "odeint_adjoint_%s_backward: underflow in dt %g", mname, dt);
      const float h = (float)dt;
      if ((rc = upload_floats(hdev, &h, 1, stream)) != ODEHIP_OK) return rc;
      {  // stage-2 inputs from k1
        const float c = (float)tb.beta[0][0] * h;
        float* k0y[1] = {ky[0]};
        float* k0a[1] = {ka[0]};
        lincomb(L.xin(ws, slot, 1), y_cur, 1, k0y, &c, nullptr);
        lincomb(L.gp(ws, slot, 1, NH), a_cur, 1, k0a, &c, nullptr);
      }
      for (int s = 2; s <= S; ++s) {  // stage s lives at index s-1 of the slot; Y_{s+1}, A_{s+1} (s = 6: y1, a1; s = 7: error norms)
        const int nx = s < S ? s : S - 1;
        adaptive_stage_combine(tb, cy, s, y_cur, hdev, ky, L.xin(ws, slot, nx), L.part(ws, 4), rtol, atol);
        adaptive_stage_combine(tb, ca, s, a_cur, hdev, ka, L.gp(ws, slot, nx, NH), L.part(ws, 5), rtol, atol);
        cy.k_scale = -1.0f;
        ca.k_scale = 1.0f;
        if ((rc = eval_aug(slot, s - 1, L.xin(ws, slot, s - 1), cy, ca)) != ODEHIP_OK) return rc;
      }
      nfe += S - 1;
      StageRef ev[kMaxStages];
      ev[0] = StageRef{k1_slot, k1_stage, k1_x0, 0.0f};
      for (int s = 1; s < S; ++s) ev[s] = StageRef{slot, s, L.xin(ws, slot, s), 0.0f};
      if (mixed_norm) {  // parameter block of this attempt: error estimate and increment, both linear in the seven stages
        for (int s = 0; s < S; ++s) ev[s].scale = h * (float)tb.c_err[s];
        if ((rc = theta_wgrad(ev, S, th_err)) != ODEHIP_OK) return rc;
        for (int s = 0; s < S; ++s) ev[s].scale = h * (float)tb.c_sol[s];
        if ((rc = theta_wgrad(ev, S, th_inc)) != ODEHIP_OK) return rc;
        theta_sums(th_err, nullptr, th_run, th_inc, 0);
      }
      float e2[2];
      {
        const int which[2] = {4, 5}, lens[2] = {L.n_part, L.n_part};
        if ((rc = fetch(2, which, lens, e2)) != ODEHIP_OK) return rc;
      }
      float ratio = fmaxf(rms(e2[0]), rms(e2[1]));
      if (mixed_norm) ratio = fmaxf(ratio, theta_rms_max(g_adj_host + 8));
      ODEHIP_REQUIRE(ratio == ratio, "odeint_adjoint_%s_backward: non-finite error ratio", mname);
      const bool accept = ratio <= 1.0f;
      const double dtn = next_step_size(dt, ratio, tb.order);
      if (!accept) {
        ++n_reject;
        dt = dtn;
        continue;
      }
      ++n_accept;
      const double t_new = t_cur + dt;
      const bool final_step = t_new >= t_end;
      float w[kMaxStages];
      if (!final_step) {
        for (int s = 0; s < S; ++s) w[s] = (float)tb.c_sol[s] * h;
      } else {
        // dense output at x: a(x) - a0 = h * sum_s W_s(x) k_s  (the quartic of _interp_fit/_interp_evaluate, linear in k)
        const float x = (float)((t_end - t_cur) / (t_new - t_cur));
        for (int s = 0; s < S; ++s) w[s] = h * (float)dense_weight(tb, s, (double)x);
      }
      if (mixed_norm) {  // the parameter block is integrated step by step (its running value enters the next tolerance)
        if (final_step) {
          for (int s = 0; s < S; ++s) ev[s].scale = w[s];
          if ((rc = theta_wgrad(ev, S, th_inc)) != ODEHIP_OK) return rc;
        }
        hipLaunchKernelGGL(theta_add_kernel, dim3(64), dim3(256), 0, stream, th_run, th_inc, P);
      }
      for (int s = 0; s < S && !mixed_norm; ++s) {
        if (w[s] == 0.0f) continue;
        entries.push_back(ev[s]);
        entries.back().scale = w[s];
      }
      if (final_step) {
        float* a_next = L.p(ws, L.off_a2 + (size_t)(n & 1) * L.g.st);
        lincomb(a_next, a_cur, S, ka, w, goq(n));  // a(t[n]) + grad_out[n]
        a_cur = a_next;
        ++slot;
        break;
      }
      // FSAL: (y, a, k1) <- (y1, a1, k7)
      y_cur = L.xin(ws, slot, S - 1);
      a_cur = L.gp(ws, slot, S - 1, NH);
      float* t1 = ky[0]; ky[0] = ky[S - 1]; ky[S - 1] = t1;
      float* t2 = ka[0]; ka[0] = ka[S - 1]; ka[S - 1] = t2;
      k1_slot = slot; k1_stage = S - 1; k1_x0 = L.xin(ws, slot, S - 1);
      t_cur = t_new;
      dt = dtn;
      ++slot;
    }
  }
  rc = odehip_q4_to_nchw(a_cur, grad_z0_nchw, batch, L.C, stream);
  if (rc != ODEHIP_OK) return rc;

  if (mixed_norm) {  // a_theta was integrated step by step: hand it out in the parameters' shapes
    for (int l = 0; l < NL; ++l) {
      ODEHIP_CHECK_HIP(hipMemcpyAsync(grad_w[l], th_run + spans.off[2 * l], (size_t)(spans.off[2 * l + 1] - spans.off[2 * l]) * 4,
                                      hipMemcpyDeviceToDevice, stream));
      ODEHIP_CHECK_HIP(hipMemcpyAsync(grad_b[l], th_run + spans.off[2 * l + 1], (size_t)(spans.off[2 * l + 2] - spans.off[2 * l + 1]) * 4,
                                      hipMemcpyDeviceToDevice, stream));
    }
    write_stats(stats_host, nfe, n_accept, n_reject);
    return ODEHIP_OK;
  }
  // ---- seminorm: a_theta does not steer the steps, so ONE wgrad launch per layer over every recorded stage evaluation
  const int n_eval = (int)entries.size();
  WgradPair* table = (WgradPair*)L.p(ws, L.off_tab);
  float* slabs = L.p(ws, L.off_slab);
  std::vector<WgradPair> host(n_eval);
  for (int l = 0; l < NL; ++l) {
    for (int e = 0; e < n_eval; ++e) wgrad_pair(host[e], entries[e], l);
    ODEHIP_CHECK_HIP(hipMemcpyAsync(table, host.data(), (size_t)n_eval * sizeof(WgradPair), hipMemcpyHostToDevice, stream));
    ODEHIP_CHECK_HIP(hipStreamSynchronize(stream));
    rc = launch_wgrad(table, n_eval, batch, 4, slabs, grad_w[l], grad_b[l], f->channels[l + 1], f->channels[l], stream, f->w_bf16[l] != nullptr);
    if (rc != ODEHIP_OK) return rc;
  }
  write_stats(stats_host, nfe, n_accept, n_reject);
  return ODEHIP_OK;
}
