// adjoint_layout.h -- workspace layout of the adaptive adjoint (adjoint_dopri5.hip: host-driven; adjoint_device.hip: device-driven)
#pragma once
#include "odehip_internal.h"
#include "persist.h"

namespace odehip {

// One slot = everything the stage evaluations of one accepted step keep for the final weight-gradient launch:
//   [stage inputs: kMaxStages x st | hidden activations: kMaxStages x NH x hid | gradient slots: kMaxStages x NG x hid]
// kMaxStages stages wide whatever the method (a tableau of S stages uses the first S), so layouts do not depend on it.  The host loop,
// the device path's table builder and its controller kernel all take their byte offsets from these methods: a relocatable pointer of
// the device-driven path is class << 56 | one of them.
struct AdjSlotGeom {
  static constexpr int cap = kMaxStages;   // stages a slot has room for
  size_t st, hid;                          // bytes of a state tensor / of the widest hidden activation
  int NH, NG;                              // hidden activations (n_convs - 1) and gradient slots (grad_slots(f)) per evaluation
  ODEHIP_HD size_t xin(int s) const { return (size_t)s * st; }
  ODEHIP_HD size_t hidden(int s, int l) const { return cap * st + ((size_t)s * NH + l) * hid; }
  ODEHIP_HD size_t gp(int s, int l) const { return cap * st + (size_t)cap * NH * hid + ((size_t)s * NG + l) * hid; }
  ODEHIP_HD size_t slot_bytes() const { return cap * (st + (size_t)NH * hid + (size_t)NG * hid); }
  // Entry of layer l's weight-gradient table for evaluation `stage` of the slot at `base`, weighted `scale`: the gradient w.r.t. the
  // layer's output (gradient slot g_slot = wgrad_slot(f, l)) and the layer's input (x0 for conv 0, else the hidden activation in front)
  ODEHIP_HD void wgrad_pair(WgradPair& p, const char* base, int stage, int l, int g_slot, const float* x0, float scale) const {
    p.g = (const float*)(base + gp(stage, g_slot));
    p.a = l == 0 ? x0 : (const float*)(base + hidden(stage, l - 1));
    p.scale = scale;
    p.pad_[0] = p.pad_[1] = p.pad_[2] = 0.0f;
  }
};

struct AdjLayout {
  int T, B, C, max_slots, n_part;
  AdjSlotGeom g;
  size_t off_h, off_part, off_sums, off_ping, off_pong, off_y, off_go, off_a2, off_ky, off_ka, off_slots, off_tab, off_slab, off_theta, off_state, off_psync, off_wtab, total;
  int P;  // floats of the flattened parameter vector (w0, b0, w1, b1, ...)
  AdjLayout(const odehip_convstack* f, int batch, int n_times, int max_accept) {
    T = n_times; B = batch; C = f->channels[0]; max_slots = max_accept + 1;
    g.NH = f->n_convs - 1; g.NG = grad_slots(f);
    g.st = al256((size_t)B * C * kPix * 4);
    int cmax = 32;
    for (int i = 0; i <= f->n_convs; ++i) cmax = f->channels[i] > cmax ? f->channels[i] : cmax;
    g.hid = al256((size_t)B * cmax * kPix * 4);
    n_part = B * (C / 32) * 2 * 4;
    size_t o = 0;
    auto take = [&](size_t b) { size_t r = o; o += al256(b); return r; };
    off_h = take(256);
    off_part = take(8 * (size_t)part_stride() * 4);
    off_sums = take(256);
    off_ping = take(g.hid);
    off_pong = take(g.hid);
    off_y = take((size_t)T * g.st);
    off_go = take((size_t)T * g.st);
    off_a2 = take(2 * g.st);
    off_ky = take(kMaxStages * g.st);
    off_ka = take(kMaxStages * g.st);
    off_slots = take((size_t)max_slots * g.slot_bytes());
    off_tab = take((size_t)wtab_cap() * sizeof(WgradPair));
    off_slab = take(wgrad_slab_bytes(B));
    P = 0;
    for (int l = 0; l < f->n_convs; ++l) P += f->channels[l + 1] * f->channels[l] * 9 + f->channels[l + 1];
    off_theta = take((size_t)5 * P * 4);  // mixed norm: running a_theta, error estimate, increment, K^theta at the two initial-step points
    // device-driven path (adjoint_device.hip): controller state, the walk's flag area, one weight-gradient table per layer
    off_state = take(4096);
    off_psync = take(persist_sync_bytes(B));
    off_wtab = take((size_t)ODEHIP_MAX_LAYERS * wtab_cap() * sizeof(WgradPair));
    total = o;
  }
  int wtab_cap() const { return max_slots * kMaxStages; }   // entries of a weight-gradient table: every stage of every slot
  float* p(const void* ws, size_t off) const { return (float*)((char*)const_cast<void*>(ws) + off); }
  char* slot(const void* ws, int i) const { return (char*)p(ws, off_slots + (size_t)i * g.slot_bytes()); }
  float* xin(const void* ws, int i, int s) const { return (float*)(slot(ws, i) + g.xin(s)); }
  float* hidden(const void* ws, int i, int s, int l) const { return (float*)(slot(ws, i) + g.hidden(s, l)); }
  float* gp(const void* ws, int i, int s, int l) const { return (float*)(slot(ws, i) + g.gp(s, l)); }
  // floats per partial array: the per-layer kernels write n_part, the sixteen-workgroup walk 64 per sample (batch <= 16)
  int part_stride() const { return n_part > 1024 ? n_part : 1024; }
  float* part(const void* ws, int j) const { return p(ws, off_part + (size_t)j * part_stride() * 4); }
};

// adjoint_device.hip: the seminorm adjoint steered by a device-side controller on the adaptive persistent walk, for the tableau of the
// call; returns ODEHIP_OK and sets *ran = 1 when it took the call, *ran = 0 when the path is not available (the caller then runs the
// host loop)
int adjoint_adaptive_device(const Tableau& tb, const odehip_convstack* f, const odehip_convstack* f_dgrad, const double* t_host, int n_times,
                            int batch, float rtol, float atol, const float* y_traj_nchw, const float* grad_out_nchw, float* grad_z0_nchw,
                            float* const* grad_w, float* const* grad_b, int max_accept, int* stats_host, void* workspace,
                            size_t workspace_bytes, hipStream_t stream, int* ran);

}  // namespace odehip
