// dopri5_control.h -- the adaptive solvers' tableaus (dopri5, bosh3) and the scalar decisions made with them, once: torchdiffeq
// 0.2.1's _select_initial_step (scalar part), _optimal_step_size and the dense-output weights of _interp_fit.  Host code, the forward
// solve's controller kernels (dopri5.hip), the device-controlled adjoint (adjoint_device.hip) and the stand-alone check of
// tests/adaptive_control_check.cpp all read this one file: it compiles in a .hip file and under a plain host C++17 compiler.
// What differs between the callers stays with them: the finite test on the error ratio, how max_steps is counted, what nfe starts
// at, the saving-slot bookkeeping and the mixed norm's extra maximum over the parameter tensors.
#pragma once
#include <math.h>

#include "../../include/odecgru_hip.h"   // the method codes
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define ODEHIP_HD __host__ __device__
#else
#define ODEHIP_HD
#endif

namespace odehip {

// ---- an embedded FSAL Runge-Kutta pair as data (torchdiffeq's _ButcherTableau, rows padded to the widest method).  S stages:
// k_1 .. k_S with k_s = f(y0 + h * sum_j beta[s-2][j] k_j); the last beta row equals c_sol, so the S-th stage input is y1 and
// k_S is the next step's k_1.  A further FSAL pair is one more table here (up to kMaxStages stages) and a method code.
constexpr int kMaxStages = ODEHIP_MAX_STAGES;
struct Tableau {
  const char* name;   // as torchdiffeq spells the method; the entry points' error messages carry it
  int stages;   // S
  int order;    // of the solution that is carried on: the step-size exponent is 1 / order, the initial step's too
  double beta[kMaxStages - 1][kMaxStages - 1];
  double c_sol[kMaxStages], c_err[kMaxStages], c_mid[kMaxStages];
};

// _select_initial_step, first half: d0 = norm(y0 / scale), d1 = norm(f0 / scale) -> the step h0 of the Euler point y0 + h0 f0
ODEHIP_HD inline float initial_step_h0(float d0, float d1) { return (d0 < 1e-5f || d1 < 1e-5f) ? 1e-6f : 0.01f * d0 / d1; }
// second half: d2 = norm((f(Euler point) - f0) / scale) / h0 -> the first step size.  torchdiffeq calls the heuristic with
// order - 1 and raises to 1 / (that + 1): the exponent is 1 / order
ODEHIP_HD inline float initial_step_dt(float h0, float d1, float d2, int order) {
  float h1;
  if (d1 <= 1e-15f && d2 <= 1e-15f) h1 = fmaxf(1e-6f, h0 * 1e-3f);
  else h1 = powf(0.01f / fmaxf(d1, d2), 1.0f / (float)order);
  return fminf(100.0f * h0, h1);
}

// _optimal_step_size: dt_next in float64 from the fp32 error ratio (safety 0.9, ifactor 10, dfactor 0.2 -- 1 after an accepted
// step; exponent 1 / order)
ODEHIP_HD inline double next_step_size(double dt, float ratio, int order) {
  double dtn;
  if (ratio == 0.0f) {
    dtn = dt * 10.0;
  } else {
    const double dfactor = ratio < 1.0f ? 1.0 : 0.2;
    dtn = dt * fmin(10.0, fmax(0.9 / pow((double)ratio, 1.0 / (double)order), dfactor));
  }
  return dtn;
}

// weight of stage s in the dense output at x: value(x) = y0 + h * sum_s dense_weight(s, x) * k_s   (the quartic of _interp_fit,
// f0 = k[0], f1 = k[last]); b = c_sol[s], m = c_mid[s] (passed in: device code keeps its own copy of the two rows)
ODEHIP_HD inline double dense_weight(int s, double x, double b, double m, int last) {
  const double d1 = s == 0 ? 1.0 : 0.0, d7 = s == last ? 1.0 : 0.0;
  const double A4 = 2.0 * (d7 - d1) - 8.0 * b + 16.0 * m;
  const double B3 = 5.0 * d1 - 3.0 * d7 + 14.0 * b - 32.0 * m;
  const double C2 = d7 - 4.0 * d1 - 5.0 * b + 16.0 * m;
  return x * d1 + x * x * C2 + x * x * x * B3 + x * x * x * x * A4;
}
inline double dense_weight(const Tableau& tb, int s, double x) { return dense_weight(s, x, tb.c_sol[s], tb.c_mid[s], tb.stages - 1); }

// Dormand-Prince 5(4) as torchdiffeq 0.2.1 holds it (_impl/dopri5.py): beta rows, c_sol (= last beta row, padded),
// c_error = c_sol - 4th-order weights, c_mid (dense-output midpoint weights)
inline constexpr Tableau kDopri5 = {
    "dopri5", 7, 5,
    {{1.0 / 5, 0, 0, 0, 0, 0},
     {3.0 / 40, 9.0 / 40, 0, 0, 0, 0},
     {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0, 0},
     {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0, 0},
     {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656, 0},
     {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84}},
    {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84, 0},
    {35.0 / 384 - 1951.0 / 21600, 0, 500.0 / 1113 - 22642.0 / 50085, 125.0 / 192 - 451.0 / 720, -2187.0 / 6784 + 12231.0 / 42400,
     11.0 / 84 - 649.0 / 6300, -1.0 / 60},
    {6025192743.0 / 30085553152.0 / 2, 0, 51252292925.0 / 65400821598.0 / 2, -2691868925.0 / 45128329728.0 / 2,
     187940372067.0 / 1594534317056.0 / 2, -1776094331.0 / 19743644256.0 / 2, 11237099.0 / 235043384.0 / 2},
};

// Bogacki-Shampine 3(2) as torchdiffeq 0.2.1 holds it (_impl/bosh3.py)
inline constexpr Tableau kBosh3 = {
    "bosh3", 4, 3,
    {{1.0 / 2}, {0, 3.0 / 4}, {2.0 / 9, 1.0 / 3, 4.0 / 9}},
    {2.0 / 9, 1.0 / 3, 4.0 / 9, 0},
    {2.0 / 9 - 7.0 / 24, 1.0 / 3 - 1.0 / 4, 4.0 / 9 - 1.0 / 3, -1.0 / 8},
    {0, 1.0 / 2, 0, 0},
};

// the tableau of an adaptive method code of the C ABI; null: not an adaptive method
inline const Tableau* adaptive_tableau(int method) {
  return method == ODEHIP_DOPRI5 ? &kDopri5 : (method == ODEHIP_BOSH3 ? &kBosh3 : nullptr);
}

// the method's name in the error messages of the entry points the two methods share (an unknown code is reported under dopri5's)
inline const char* adaptive_name(int method) {
  const Tableau* tb = adaptive_tableau(method);
  return tb ? tb->name : kDopri5.name;
}

}  // namespace odehip
