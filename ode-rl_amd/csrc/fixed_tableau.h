// fixed_tableau.h -- the Butcher tableaus of the fixed-grid methods (torchdiffeq _impl/fixed_grid.py: euler, midpoint, rk4 = the
// 3/8 rule) and the three plans every driver derives from them.  Plain C++17, no HIP: host code, constexpr device code and the
// stand-alone check of tests/test_fixed_tableau_cpu.py all read this one file.
//   x_s = y + h * sum_{j<s} a[s][j] k_j,   k_s = f(x_s),   y1 = y + h * sum_j b[j] k_j
// Readers: fixed_grid.hip (forward solve, reverse sweep, adjoint: the plans become CombineArgs / BwdTarget tables), fstack_bf16.hip
// (StageProgram: the forward plan as compile-time constants), btraj_bf16.hip (the rk4 reverse sweep written out in registers: it
// names the tableau's entries and mirrors reverse_targets()).  The entries are float expressions: rounded from double they could
// differ in the last bit.
#pragma once
#include "../../include/odecgru_hip.h"

namespace odehip {

constexpr int kFixedMaxStages = 4;
struct FixedTableau {
  int S;
  float a[kFixedMaxStages][kFixedMaxStages];   // strictly lower triangular
  float b[kFixedMaxStages];
};
constexpr int kFixedMethods = 3;
constexpr FixedTableau kFixedTableau[kFixedMethods] = {
    /* ODEHIP_EULER    */ {1, {}, {1.0f}},
    /* ODEHIP_MIDPOINT */ {2, {{}, {0.5f}}, {0.0f, 1.0f}},
    /* ODEHIP_RK4      */ {4, {{}, {1.0f / 3.0f}, {-(1.0f / 3.0f), 1.0f}, {1.0f, -1.0f, 1.0f}}, {0.125f, 0.375f, 0.375f, 0.125f}},
};
static_assert(ODEHIP_EULER == 0 && ODEHIP_MIDPOINT == 1 && ODEHIP_RK4 == 2, "kFixedTableau is indexed by the method code");
constexpr bool is_fixed_method(int method) { return method >= 0 && method < kFixedMethods; }
constexpr const FixedTableau& fixed_tableau(int method) { return kFixedTableau[method]; }
constexpr int n_stages(int method) { return is_fixed_method(method) ? kFixedTableau[method].S : 1; }

// true if row[0 .. s-1] has a non-zero entry: the sum the row stands for has been written before stage s adds to it
constexpr bool fixed_any_before(const float* row, int s) {
  for (int j = 0; j < s; ++j)
    if (row[j] != 0.0f) return true;
  return false;
}

// ---- forward: the stage combine behind k_s = f(x_s).  Stage s < S-1 forms x_{s+1} (row a[s+1]), the last one y1 (row b).  Earlier
// stages with a zero weight are left out (midpoint's result reads k_2 alone); the stage's own weight sits behind the kept ones.
struct FixedCombine {
  int n_prev;                      // earlier stages kept
  int prev[kFixedMaxStages];       // their indices, ascending
  float c[kFixedMaxStages + 1];    // their weights, then the stage's own at [n_prev]
  bool result;                     // the row is b: the combine writes y1
  bool keep_k;                     // a later combine of the same sweep reads k_s
};
// with_result = false: a sweep that only needs the stage inputs (the adjoint's recomputation): its last stage combines nothing and
// row b keeps no k alive
constexpr FixedCombine fixed_combine(const FixedTableau& T, int s, bool with_result = true) {
  FixedCombine p = {};
  if (s >= T.S) return p;
  p.result = s == T.S - 1;
  const float* row = p.result ? T.b : T.a[s + 1];
  for (int j = 0; j < s; ++j)
    if (row[j] != 0.0f) {
      p.prev[p.n_prev] = j;
      p.c[p.n_prev++] = row[j];
    }
  p.c[p.n_prev] = row[s];
  for (int m = s + 2; m < T.S; ++m) p.keep_k = p.keep_k || T.a[m][s] != 0.0f;
  p.keep_k = p.keep_k || (with_result && !p.result && T.b[s] != 0.0f);
  return p;
}

// ---- targets of an input-gradient chain's last conv: out = (a_c + a_h h) * src + (g_c + g_h h) * gx, gx = J_f(x_s)^T (chain seed).
// Slots instead of pointers, so that the plans can be checked without a device:
//   >= 0          the per-stage tensor of stage j (reverse sweep: gk_j = dL/dk_j; adjoint: A_j, the adjoint at stage j)
//   kSlotQ + m    adjoint: Q_m, the partial sum of A_m (m >= 2)
enum : int {
  kSlotNone = -1,    // no source: a zero weight contributes nothing, not 0 * src
  kSlotState = -2,   // the state at the interval's right end (reverse sweep: g = dL/dy_{n+1}; adjoint: a)
  kSlotGy = -3,      // reverse sweep: the running dL/dy_n
  kSlotR = -4,       // adjoint: the partial sum of the result
  kSlotOut = -5,     // the interval's result; the driver adds grad_out[n] to it (and, reverse sweep, seeds the next interval from it)
  kSlotQ = 8,
};
struct FixedTarget { int out, src; float a_c, a_h, g_c, g_h; };
struct FixedTargets { int n; FixedTarget t[4]; };   // BwdArgs::tgt holds four

// Reverse sweep (discretise-then-optimise), stages S-1 .. 0.  Stage s's chain is seeded with gk_s and yields gx_s:
//   gy (+)= gx_s, then gk_j (+)= a[s][j] h gx_s for j = s-1 .. 0 with a[s][j] != 0.
// gy reads g the first time; the first write of gk_j takes b[j] h g instead of gk_j (no source if b[j] == 0).  Stage 0 closes the
// interval: kSlotOut = gy + gx_0 (+ grad_out[n]).  gk_{S-1} = b[S-1] h g is the seed the driver forms when g is (fixed_seed_weight).
constexpr FixedTargets reverse_targets(const FixedTableau& T, int s) {
  FixedTargets p = {};
  p.t[p.n++] = FixedTarget{s == 0 ? kSlotOut : kSlotGy, s == T.S - 1 ? kSlotState : kSlotGy, 1.0f, 0.0f, 1.0f, 0.0f};
  for (int j = s - 1; j >= 0; --j) {
    if (T.a[s][j] == 0.0f) continue;
    bool written = false;
    for (int m = s + 1; m < T.S; ++m) written = written || T.a[m][j] != 0.0f;
    if (written) p.t[p.n++] = FixedTarget{j, j, 1.0f, 0.0f, 0.0f, T.a[s][j]};
    else if (T.b[j] != 0.0f) p.t[p.n++] = FixedTarget{j, kSlotState, 0.0f, T.b[j], 0.0f, T.a[s][j]};
    else p.t[p.n++] = FixedTarget{j, kSlotNone, 0.0f, 0.0f, 0.0f, T.a[s][j]};
  }
  return p;
}
constexpr float fixed_seed_weight(const FixedTableau& T) { return T.b[T.S - 1]; }

// Adjoint (optimise-then-discretise): one step of the same method on a' = J_f^T a, stages 0 .. S-1.  Stage s's chain is seeded with
// A_s (A_0 = a) and yields K_s; it writes, in this order, A_{s+1}, then Q_m (+)= a[m][s] h K_s for every later m with a[m][s] != 0,
// then R (+)= b[s] h K_s if b[s] != 0.  A sum reads a until it has been written and itself afterwards (A_{s+1} continues Q_{s+1}).
// The last stage writes kSlotOut = (R or a) + b[S-1] h K (+ grad_out[n]).  The parameter adjoint weighs evaluation s with h b[s].
constexpr FixedTargets adjoint_targets(const FixedTableau& T, int s) {
  FixedTargets p = {};
  const int r_src = fixed_any_before(T.b, s) ? kSlotR : kSlotState;
  if (s == T.S - 1) {
    p.t[p.n++] = FixedTarget{kSlotOut, r_src, 1.0f, 0.0f, 0.0f, T.b[s]};
    return p;
  }
  for (int m = s + 1; m < T.S; ++m)
    if (m == s + 1 || T.a[m][s] != 0.0f)
      p.t[p.n++] = FixedTarget{m == s + 1 ? m : kSlotQ + m, fixed_any_before(T.a[m], s) ? kSlotQ + m : kSlotState, 1.0f, 0.0f, 0.0f, T.a[m][s]};
  if (T.b[s] != 0.0f) p.t[p.n++] = FixedTarget{kSlotR, r_src, 1.0f, 0.0f, 0.0f, T.b[s]};
  return p;
}

// what the drivers' argument structs and workspaces can hold, and what the plans above take for granted
constexpr bool fixed_tableau_fits(const FixedTableau& T) {
  if (T.S < 1 || T.S > kFixedMaxStages || T.S > ODEHIP_MAX_STAGES) return false;
  for (int s = 0; s < T.S; ++s) {
    if (reverse_targets(T, s).n > 4 || adjoint_targets(T, s).n > 4) return false;   // BwdArgs::tgt[4]
    for (int j = s; j < kFixedMaxStages; ++j)
      if (T.a[s][j] != 0.0f) return false;   // explicit method
    if (s + 1 < T.S && T.a[s + 1][s] == 0.0f) return false;   // A_{s+1} is written by stage s's chain
    bool read = s == T.S - 1;
    for (int m = s + 1; m < T.S; ++m) read = read || T.a[m][s] != 0.0f;
    if (!read) return false;   // gk_s gets its first value (b[s] h g included) where a later stage reads k_s
  }
  return true;
}
static_assert(fixed_tableau_fits(kFixedTableau[0]) && fixed_tableau_fits(kFixedTableau[1]) && fixed_tableau_fits(kFixedTableau[2]), "a fixed-grid tableau does not fit the drivers");

}  // namespace odehip
