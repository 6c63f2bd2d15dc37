// A dense Levenberg-Marquardt loop of D <= 12 unknowns, callable from the host and from a whole workgroup on the device:
// Ceres 2.1 TrustRegionMinimizer + LevenbergMarquardtStrategy [EXT] with default Solver::Options (BaLmOptions of
// ba_device.h), the same restatement as ba_optimize_views_kernel (kernels_ba.hip).  The damped system
// (S H S + D^2/radius) s = -S g is solved by Cholesky of the normal equations instead of Ceres' DENSE_QR of [J; D]
// (DESIGN.md "Static multi-pose IMU calibration": the problems are tiny and well conditioned).
//
// eval(x, jac, &cost, H, g): cost = 0.5 sum r^2; with jac also H = J^T J (upper triangle packed row by row) and g = J^T r.
// It returns false when the residuals cannot be evaluated.  On the device every lane of the workgroup calls small_lm
// with the same values, so the control flow is uniform and eval may synchronise the workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include "ba_device.h"
#include "../../include/oicc_hip.h"

namespace oicc {

template <int D>
__host__ __device__ inline bool small_chol_solve(const double* H, const double* g, const double* scale, const double* D2, double* s) {
  double A[D][D], rhs[D];
  int e = 0;
  for (int i = 0; i < D; ++i) {
    for (int j = i; j < D; ++j) { const double v = H[e] * scale[i] * scale[j]; A[i][j] = v; A[j][i] = v; ++e; }
    A[i][i] += D2[i];
    rhs[i] = -g[i] * scale[i];
  }
  for (int j = 0; j < D; ++j) {
    double t = A[j][j];
    for (int k = 0; k < j; ++k) t -= A[j][k] * A[j][k];
    if (!(t > 0.0)) return false;
    const double l = sqrt(t);
    A[j][j] = l;
    for (int i = j + 1; i < D; ++i) {
      double u = A[i][j];
      for (int k = 0; k < j; ++k) u -= A[i][k] * A[j][k];
      A[i][j] = u / l;
    }
  }
  for (int i = 0; i < D; ++i) { double t = rhs[i]; for (int k = 0; k < i; ++k) t -= A[i][k] * rhs[k]; rhs[i] = t / A[i][i]; }
  for (int i = D - 1; i >= 0; --i) { double t = rhs[i]; for (int k = i + 1; k < D; ++k) t -= A[k][i] * rhs[k]; rhs[i] = t / A[i][i]; }
  for (int i = 0; i < D; ++i) { if (!(fabs(rhs[i]) <= DBL_MAX)) return false; s[i] = rhs[i]; }
  return true;
}

// Returns the OICC_SIMU_TERM_* reason; *iterations counts the trust-region iterations after iteration 0.
template <int D, class Eval>
__host__ __device__ inline int small_lm(const BaLmOptions& o, double* x, Eval& eval, int* iterations, double* final_cost) {
  constexpr int NH = D * (D + 1) / 2;
  double cost = 0.0, H[NH], g[D];
  *iterations = 0;
  if (!eval(x, true, &cost, H, g)) { *final_cost = cost; return OICC_SIMU_TERM_EVAL_FAILED; }
  double scale[D], diag[D], D2[D], step[D], cand[D];
  { int e = 0; for (int i = 0; i < D; ++i) { scale[i] = o.jacobi_scaling ? 1.0 / (1.0 + sqrt(H[e])) : 1.0; e += D - i; } }
  auto grad_max = [&]() { double m = 0.0; for (int i = 0; i < D; ++i) m = fmax(m, fabs(g[i])); return m; };
  auto norm_of = [&](const double* p) { double s = 0.0; for (int k = 0; k < D; ++k) s += p[k] * p[k]; return sqrt(s); };
  double radius = o.initial_radius, decrease_factor = 2.0, x_norm = norm_of(x);
  bool reuse_diagonal = false;
  int invalid = 0, iter = 0, term = OICC_SIMU_TERM_GRADIENT;
  if (grad_max() <= o.gradient_tolerance) { *final_cost = cost; return term; }
  for (;;) {
    if (iter >= o.max_iters) { term = OICC_SIMU_TERM_MAX_ITERATIONS; break; }
    if (radius <= o.min_radius) { term = OICC_SIMU_TERM_MIN_RADIUS; break; }
    ++iter;
    if (!reuse_diagonal) { int e = 0; for (int i = 0; i < D; ++i) { diag[i] = fmin(fmax(H[e] * scale[i] * scale[i], o.min_lm_diagonal), o.max_lm_diagonal); e += D - i; } }
    for (int i = 0; i < D; ++i) D2[i] = diag[i] / radius;
    bool ok = small_chol_solve<D>(H, g, scale, D2, step);
    double model = 0.0;
    if (ok) {
      for (int i = 0; i < D; ++i) model += 0.5 * step[i] * (D2[i] * step[i] - g[i] * scale[i]);
      ok = model > 0.0;
    }
    if (!ok) {
      if (++invalid >= o.max_invalid) { term = OICC_SIMU_TERM_INVALID_STEPS; break; }
      radius /= decrease_factor; decrease_factor *= 2.0; reuse_diagonal = true;
      continue;
    }
    invalid = 0;
    double step_sq = 0.0;
    for (int i = 0; i < D; ++i) { cand[i] = x[i] + step[i] * scale[i]; step_sq += (cand[i] - x[i]) * (cand[i] - x[i]); }
    double cand_cost = 0.0, Hd[NH], gd[D];
    if (!eval(cand, false, &cand_cost, Hd, gd)) cand_cost = DBL_MAX;
    const double step_norm = sqrt(step_sq), cost_change = cost - cand_cost, rel_dec = cost_change / model;
    if (step_norm <= o.parameter_tolerance * (x_norm + o.parameter_tolerance)) { term = OICC_SIMU_TERM_PARAMETER; break; }
    if (fabs(cost_change) <= o.function_tolerance * cost) { term = OICC_SIMU_TERM_FUNCTION; break; }
    if (rel_dec > o.min_relative_decrease) {
      for (int k = 0; k < D; ++k) x[k] = cand[k];
      x_norm = norm_of(x);
      eval(x, true, &cost, H, g);
      const double q = 2.0 * rel_dec - 1.0;
      radius = fmin(o.max_radius, radius / fmax(1.0 / 3.0, 1.0 - q * q * q));
      decrease_factor = 2.0; reuse_diagonal = false;
      if (grad_max() <= o.gradient_tolerance) { term = OICC_SIMU_TERM_GRADIENT; break; }
    } else {
      radius /= decrease_factor; decrease_factor *= 2.0; reuse_diagonal = true;
    }
  }
  *iterations = iter;
  *final_cost = cost;
  return term;
}

// Solver::Options defaults of Ceres 2.1 (what the reference's ceres::Solve calls get)
inline BaLmOptions ceres_default_lm_options() {
  BaLmOptions o;
  o.function_tolerance = 1e-6; o.parameter_tolerance = 1e-8; o.gradient_tolerance = 1e-10;
  o.initial_radius = 1e4; o.max_radius = 1e16; o.min_radius = 1e-32; o.min_relative_decrease = 1e-3;
  o.min_lm_diagonal = 1e-6; o.max_lm_diagonal = 1e32;
  o.jacobi_scaling = 1; o.max_invalid = 5; o.max_iters = 50;
  return o;
}

}  // namespace oicc
