// Covariance estimation (kernels_covariance.hip, oicc_covariance.hip): device buffers and launchers.  Internal, not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include "oicc_device.h"

namespace oicc {

constexpr int kCovMaxHalfBandwidth = 120;   // the LDS window of the backward sweep (kernels_covariance.hip: 128 x 128 doubles)
constexpr int kCovMaxArrow = 63;            // arrow columns: one wave lane each, the limit of the cyclic reduction's border too

struct CovBuffers {
  double* s;        // [P]      s_i = 1 / sqrt(H_ii)
  double* Cs;       // [a][a]   scaled arrow corner
  double* Sc;       // [a][a]   Schur complement Cs - Y'Y
  double* Zaa;      // [a][a]   its inverse (scaled)
  double* cov_aa;   // [a][a]   arrow covariance
  double* zb;       // [Pb][3]  Bs^-1 entries (j+d, j), d = 0..2
  double* G;        // [Pb][a]  L^-T Y
  double* cov3;     // [Pb][3]  covariance entries (i+d, i), d = 0..2
  double* cross;    // [Pb][a]  covariance entries (i, Pb+q)
  double* zs_diag;  // [P]      diagonal of the scaled inverse
  int32_t* flags;   // [2]      smallest column with a diagonal that is not finite and positive | corner pivot failure
};

void launch_cov_build(const NormalEq& ne, const TangentLayout& tl, const CovBuffers& cb, double* Mb, double* Mt, double* Mc, hipStream_t st);
void launch_cov_corner(const TangentLayout& tl, const CovBuffers& cb, const double* Mt, hipStream_t st);
int launch_cov_sweep(const TangentLayout& tl, const CovBuffers& cb, const double* Mb, const double* Mt, hipStream_t st);   // -1: geometry not supported
void launch_cov_finish(const TangentLayout& tl, const CovBuffers& cb, hipStream_t st);

// view bundle adjustment, OICC_BA_POINTS: the inverse of every variable point's 3 x 3 block of the band (half bandwidth 2), one lane per point
void launch_ba_point_covariances(const double* band, const int32_t* point_tangent, int64_t n, double* cov9, hipStream_t st);

}  // namespace oicc
