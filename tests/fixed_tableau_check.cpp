// Stand-alone check of ode-rl_amd/csrc/fixed_tableau.h (compiled and run by tests/test_fixed_tableau_cpu.py, host compiler only).
// The three plans are applied to the scalar ODE y' = lambda y in double, the way the kernels' epilogues apply them, and compared
// with the tableau's definition evaluated directly.  Slots the plans say nobody keeps are poisoned with NaN.
#include <cmath>
#include <cstdio>

#include "../ode-rl_amd/csrc/fixed_tableau.h"

using namespace odehip;

static int g_bad = 0;
static void expect(bool ok, const char* what, int method, double z) {
  if (!ok) {
    std::printf("FAIL method %d z %g: %s\n", method, z, what);
    ++g_bad;
  }
}
static bool close(double got, double want) { return std::fabs(got - want) <= 1e-6 * std::fabs(want); }

// out = (a_c + a_h h) src + (g_c + g_h h) gx, a missing source contributing nothing (conv_common.h, combine == 3)
static double apply(const FixedTarget& t, double h, double src, double gx) {
  double o = gx * ((double)t.g_c + (double)t.g_h * h);
  if (t.src != kSlotNone) o += src * ((double)t.a_c + (double)t.a_h * h);
  return o;
}

int main() {
  const double zs[] = {-1.0, -0.37, 0.05, 0.6, 1.0};
  const double h = 0.25, y0 = 1.3, kNaN = std::nan("");
  for (int method = 0; method < kFixedMethods; ++method) {
    const FixedTableau& T = fixed_tableau(method);
    const int S = T.S;
    expect(S == n_stages(method) && S == (method == ODEHIP_RK4 ? 4 : method == ODEHIP_MIDPOINT ? 2 : 1), "stage count", method, 0);
    for (double z : zs) {
      const double lam = z / h;
      // the definition, directly: P_s(z) = 1 + z sum_j a[s][j] P_j(z) (x_s = P_s y), R(z) = 1 + z sum_j b[j] P_j(z)
      auto stage_poly = [&](double zz, double* P) {
        double R = 1.0;
        for (int s = 0; s < S; ++s) {
          P[s] = 1.0;
          for (int j = 0; j < s; ++j) P[s] += zz * (double)T.a[s][j] * P[j];
          R += zz * (double)T.b[s] * P[s];
        }
        return R;
      };
      double Pp[kFixedMaxStages], Pm[kFixedMaxStages];
      const double R = stage_poly(z, Pp);
      stage_poly(-z, Pm);
      const double R_closed = method == ODEHIP_EULER ? 1 + z : method == ODEHIP_MIDPOINT ? 1 + z + z * z / 2
                                                                                          : 1 + z + z * z / 2 + z * z * z / 6 + z * z * z * z / 24;
      const double dR_closed = method == ODEHIP_EULER ? 1 : method == ODEHIP_MIDPOINT ? 1 + z : 1 + z + z * z / 2 + z * z * z / 6;
      expect(close(R, R_closed), "the tableau's stability polynomial", method, z);

      // ---- forward plan: k_s = lambda x_s, the combine forms x_{s+1} / y1; a k nobody keeps is lost
      double x[kFixedMaxStages + 1], k[kFixedMaxStages];
      x[0] = y0;
      for (int s = 0; s < S; ++s) {
        const FixedCombine p = fixed_combine(T, s);
        const double kc = lam * x[s];
        double sum = (double)p.c[p.n_prev] * kc;
        for (int i = 0; i < p.n_prev; ++i) {
          expect(p.prev[i] < s && (double)p.c[i] != 0.0 && (i == 0 || p.prev[i] > p.prev[i - 1]), "kept earlier stages: non-zero, ascending", method, z);
          sum += (double)p.c[i] * k[p.prev[i]];
        }
        x[s + 1] = y0 + h * sum;
        k[s] = p.keep_k ? kc : kNaN;
        expect(p.result == (s == S - 1), "only the last stage writes the result", method, z);
      }
      expect(close(x[S], R_closed * y0), "forward: y1 = R(z) y", method, z);

      // ---- reverse plan (dL/dy1 = 1, grad_out[n] = 0): dy1/dy0 = R(z), dy1/dlambda = sum_s gk_s x_s = h R'(z) y
      {
        double gk[kFixedMaxStages], gy = kNaN, out = kNaN, dlam = 0.0;
        const double g = 1.0;
        for (int s = 0; s < S; ++s) gk[s] = kNaN;
        gk[S - 1] = (double)fixed_seed_weight(T) * h * g;
        for (int s = S - 1; s >= 0; --s) {
          const FixedTargets p = reverse_targets(T, s);
          const double gx = lam * gk[s];
          dlam += gk[s] * x[s];
          expect(p.n >= 1 && p.n <= 4 && p.t[0].out == (s == 0 ? kSlotOut : kSlotGy), "reverse: gy first, at most 4 targets", method, z);
          double res[4];
          for (int i = 0; i < p.n; ++i) {
            const FixedTarget& t = p.t[i];
            if (i > 0) expect(t.out >= 0 && t.out < s && (i == 1 || t.out < p.t[i - 1].out) && T.a[s][t.out] != 0.0f, "reverse: gk_j for j = s-1 .. 0, non-zero a[s][j] only", method, z);
            if (t.src == kSlotNone) expect(t.a_c == 0.0f && t.a_h == 0.0f, "reverse: no source, no weight", method, z);
            if (t.src == kSlotState && i > 0) expect(t.a_h == T.b[t.out] && T.b[t.out] != 0.0f, "reverse: first write takes b[j] h g", method, z);
            const double src = t.src == kSlotState ? g : t.src == kSlotGy ? gy : t.src >= 0 ? gk[t.src] : 0.0;
            res[i] = apply(t, h, src, gx);
          }
          for (int i = 0; i < p.n; ++i) (p.t[i].out == kSlotGy ? gy : p.t[i].out == kSlotOut ? out : gk[p.t[i].out]) = res[i];
        }
        expect(close(out, R_closed), "reverse: dy1/dy0 = R(z)", method, z);
        expect(close(dlam, h * dR_closed * y0), "reverse: dy1/dlambda = h R'(z) y", method, z);
      }

      // ---- adjoint plan: one step of the method on a' = J^T a from t[n+1] back to t[n], stages of y recomputed from y1 with the
      // negated dynamics.  a_next = R(z) a.  The parameter sum is the optimise-then-discretise one, sum_s h b[s] A_s Y_s with
      // A_s = P_s(z) a and Y_s = P_s(-z) y1: the definition evaluated directly (it equals h R'(z) y only up to the method's order)
      {
        const double a = 1.0, y1 = R * y0;
        double A[kFixedMaxStages], Q[kFixedMaxStages], Rsum = kNaN, out = kNaN, Y[kFixedMaxStages + 1], kk[kFixedMaxStages];
        double dlam = 0.0, dlam_def = 0.0;
        for (int s = 0; s < S; ++s) A[s] = Q[s] = kNaN;
        A[0] = a;
        Y[0] = y1;
        for (int s = 0; s < S; ++s) {
          const FixedCombine c = fixed_combine(T, s, /*with_result=*/false);
          const double kc = -lam * Y[s];
          if (s + 1 < S) {
            double sum = (double)c.c[c.n_prev] * kc;
            for (int i = 0; i < c.n_prev; ++i) sum += (double)c.c[i] * kk[c.prev[i]];
            Y[s + 1] = y1 + h * sum;
          }
          kk[s] = c.keep_k ? kc : kNaN;
          const FixedTargets p = adjoint_targets(T, s);
          const double K = lam * A[s];
          const double scale = (double)((float)h * T.b[s]);   // scales[n S + s] = dt * b[s] in float
          dlam += scale * A[s] * Y[s];
          dlam_def += h * (double)T.b[s] * (Pp[s] * a) * (Pm[s] * y1);
          expect(p.n >= 1 && p.n <= 4 && p.t[0].out == (s == S - 1 ? kSlotOut : s + 1), "adjoint: A_{s+1} (or the result) first, at most 4 targets", method, z);
          double res[4];
          for (int i = 0; i < p.n; ++i) {
            const FixedTarget& t = p.t[i];
            expect(t.src != kSlotNone && t.a_c == 1.0f && t.a_h == 0.0f && t.g_c == 0.0f && (i == 0 || t.g_h != 0.0f), "adjoint: sums continue a or themselves; zero weights have no target", method, z);
            if (i > 0) expect(t.out == kSlotR ? i == p.n - 1 : (t.out > kSlotQ + s + 1 && t.out > p.t[i - 1].out), "adjoint: Q_m ascending, then R", method, z);
            const double src = t.src == kSlotState ? a : t.src == kSlotR ? Rsum : Q[t.src - kSlotQ];
            res[i] = apply(t, h, src, K);
          }
          for (int i = 0; i < p.n; ++i) {
            const int o = p.t[i].out;
            (o == kSlotOut ? out : o == kSlotR ? Rsum : o >= kSlotQ ? Q[o - kSlotQ] : A[o]) = res[i];
          }
        }
        expect(close(out, R_closed * a), "adjoint: a_next = R(z) a", method, z);
        expect(close(dlam, dlam_def), "adjoint: sum_s scales_s A_s Y_s", method, z);
      }
    }
  }
  // zero weights: midpoint's gk_1 has no source, its adjoint keeps no R before the last stage; rk4's widest lists have four targets
  expect(reverse_targets(fixed_tableau(ODEHIP_MIDPOINT), 1).t[1].src == kSlotNone, "midpoint: gk_1 has no source", ODEHIP_MIDPOINT, 0);
  expect(adjoint_targets(fixed_tableau(ODEHIP_MIDPOINT), 0).n == 1, "midpoint: stage 1 writes A_2 only", ODEHIP_MIDPOINT, 0);
  expect(fixed_combine(fixed_tableau(ODEHIP_MIDPOINT), 1).n_prev == 0 && !fixed_combine(fixed_tableau(ODEHIP_MIDPOINT), 0).keep_k,
         "midpoint: the result reads k_2 alone", ODEHIP_MIDPOINT, 0);
  expect(reverse_targets(fixed_tableau(ODEHIP_RK4), 3).n == 4 && adjoint_targets(fixed_tableau(ODEHIP_RK4), 0).n == 4, "rk4: four targets", ODEHIP_RK4, 0);
  if (!g_bad) std::printf("fixed_tableau: ok\n");
  return g_bad ? 1 : 0;
}
