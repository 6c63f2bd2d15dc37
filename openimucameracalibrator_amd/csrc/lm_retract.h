// The (+) retraction of one parameter block, x_cand = x (+) alpha (scale .* step_s), and the model-cost term of one tangent entry:
// the bodies lm_retract_kernel (kernels_solve.hip) and the fused tail of the last back-substitution launch (kernels_bcr.hip:
// bcri_backward2_retract_kernel) share, so that a candidate parameter is the same sequence of operations on the same inputs
// whichever launch wrote it.  d[] are entries of the scaled step (step_s), sc[] the Jacobi scales of the same entries.
// Both callers inline these bodies, and the compiler contracts multiply-adds where it inlines them (the library is built with the
// default -ffp-contract): that the two contexts contract alike is not guaranteed by the language but pinned by
// tests/test_gpu_fused_retract.py, which compares every bit.  (Switching contraction off here would make it hold by construction
// and change the last bits of every candidate the stand-alone kernel has produced so far; alpha stays a run-time value in both
// callers, so that neither folds alpha = 1 into a different expression.)
//
// LieLocalParameterization::Plus: SO3 knots T*exp(d) (ceres_local_param.h:84-92, so3.hpp:326-340,584-621), T_i_c SE3 with the
// coupled exp (se3.hpp:761-782), Euclidean blocks x + d, bias knots projected onto their box (impl.h:213-218), board points
// ceres::HomogeneousVectorParameterization(4)::Plus.
#pragma once
#include <hip/hip_runtime.h>
#include "oicc_device.h"
#include "spline_math.h"
#include "ba_math.h"   // homogeneous_plus4: the board points under SplineOptimFlags::POINTS

namespace oicc {

__device__ __forceinline__ void se3_exp_dev(const double a6[6], Quat* q, double t[3]) {
  const double om[3] = {a6[3], a6[4], a6[5]};
  double theta;
  *q = so3_exp(om, &theta);
  double V[9];
  if (theta < kSophusEps) {
    so3_matrix(*q, V);
  } else {
    const double tsq = theta * theta;
    double s, c; fast_sincos(theta, &s, &c);
    const double c1 = (1.0 - c) / tsq, c2 = (theta - s) / (tsq * theta);
    const double x = om[0], y = om[1], z = om[2];
    // I + c1 [om]x + c2 [om]x^2
    V[0] = 1.0 - c2 * (y * y + z * z); V[1] = -c1 * z + c2 * x * y;       V[2] = c1 * y + c2 * x * z;
    V[3] = c1 * z + c2 * x * y;        V[4] = 1.0 - c2 * (x * x + z * z); V[5] = -c1 * x + c2 * y * z;
    V[6] = -c1 * y + c2 * x * z;       V[7] = c1 * x + c2 * y * z;        V[8] = 1.0 - c2 * (x * x + y * y);
  }
  mat3_vec(V, a6, t);
}

// model cost change = 0.5 * d.(D2 d - g_s)  (from (H_s + D2) d = -g_s): the term of one tangent entry
__device__ __forceinline__ double lm_model_term(double d, double D2, double g, double sc) { return 0.5 * d * (D2 * d - g * sc); }

// SO(3) knot: q (*) exp(alpha scale .* d)
__device__ __forceinline__ Quat lm_retract_so3(const Quat& q, const double d[3], const double sc[3], double alpha) {
  const double om[3] = {alpha * (d[0] * sc[0]), alpha * (d[1] * sc[1]), alpha * (d[2] * sc[2])};
  return so3_mul(q, so3_exp(om));
}
__device__ __forceinline__ void lm_store_so3(const Quat& r, const double q0[4], double* q1, double& step_sq, double& x_sq) {
  const double rv[4] = {r.x, r.y, r.z, r.w};
  for (int c = 0; c < 4; ++c) { q1[c] = rv[c]; const double dd = rv[c] - q0[c]; step_sq += dd * dd; x_sq += q0[c] * q0[c]; }
}
// one entry of a Euclidean block (R^3 knots, gravity, line delay, IMU intrinsics)
__device__ __forceinline__ void lm_retract_eucl(double v0, double d, double sc, double alpha, double* out, double& step_sq, double& x_sq) {
  const double dd = alpha * (d * sc);
  const double v1 = v0 + dd; *out = v1; step_sq += (v1 - v0) * (v1 - v0); x_sq += v0 * v0;
}
// one entry of a bias knot, projected onto its box [-bound, bound]
__device__ __forceinline__ void lm_retract_box(double v0, double d, double sc, double alpha, double bound, double* out, double& step_sq, double& x_sq) {
  const double v1 = fmin(fmax(v0 + alpha * (d * sc), -bound), bound);
  *out = v1; step_sq += (v1 - v0) * (v1 - v0); x_sq += v0 * v0;
}
// board point (homogeneous 4-vector, 3 tangent entries)
__device__ __forceinline__ void lm_retract_point(const double X0[4], const double d[3], const double sc[3], double alpha, double* out, double& step_sq, double& x_sq) {
  const double d3[3] = {alpha * (d[0] * sc[0]), alpha * (d[1] * sc[1]), alpha * (d[2] * sc[2])};
  double X1[4]; homogeneous_plus4(X0, d3, X1);
  for (int c = 0; c < 4; ++c) { out[c] = X1[c]; const double dd = X1[c] - X0[c]; step_sq += dd * dd; x_sq += X0[c] * X0[c]; }
}
// T_i_c: [quaternion | translation], 6 tangent entries (translation first), the coupled SE(3) exponential
__device__ __forceinline__ void lm_retract_tic(const double T0[7], const double d[6], const double sc[6], double alpha, double* T1, double& step_sq, double& x_sq) {
  double a6[6];
  for (int c = 0; c < 6; ++c) a6[c] = alpha * (d[c] * sc[c]);
  Quat dq; double dt[3];
  se3_exp_dev(a6, &dq, dt);
  const Quat q{T0[0], T0[1], T0[2], T0[3]};
  double rt[3]; so3_rotate(q, dt, rt);
  const Quat r = so3_mul(q, dq);
  const double out[7] = {r.x, r.y, r.z, r.w, T0[4] + rt[0], T0[5] + rt[1], T0[6] + rt[2]};
  for (int c = 0; c < 7; ++c) { T1[c] = out[c]; const double dd = out[c] - T0[c]; step_sq += dd * dd; x_sq += T0[c] * T0[c]; }
}

}  // namespace oicc
