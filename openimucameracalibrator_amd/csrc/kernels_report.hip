// Residual report of the spline problem (oicc_residual_report, host side oicc_report.hip): what every corner and every IMU sample
// misses by at the current parameters, UNWEIGHTED, and the per-view statistics a user reads first.  Residuals only: the item functions
// of block_items.h with JAC = false, no tiles, no LDS, no atomics.
//   report_views_kernel   one wave per view, one lane per corner (a view above 64 corners is walked in rounds of 64).  The view's own
//                         functor: rolling-shutter views with quirk Q1 or its rs_time_in_seconds fix, global-shutter views without the
//                         line-delay shift -- but no 1/sigma and no quirk Q2 zeroing: e = pi(p_c) - z in pixels.  Status per corner
//                         (0 used, 1 projection failed: the functor's 1e10 pair is kept as e, 2 gated: its true error is still written).
//                         Per view n_used (status 0), sum |e|^2 and max |e| over the used corners: every lane sums its own corners in
//                         round order, then one xor butterfly over the wave -- one order, bit-identical from run to run.
//   report_imu_kernel     one lane per sample (as trajectory_kernel): accelerometer R^T (a_w + g) - MS_a (a_m - b) [m/s^2], gyroscope
//                         omega - MS_g (omega_m - b) [rad/s].  Per wave the sums of r^2 and (w r)^2 of every axis (same butterfly) go
//                         to one row of `partials`; the host adds the rows in order.
#include <hip/hip_runtime.h>
#include "oicc_device.h"
#include "block_items.h"

namespace oicc {
namespace {

struct LocalSeg { const double* base; __device__ __forceinline__ const double* operator()(int i) const { return base + i * kSegStride; } };
struct GlobalR3 { const double* base; __device__ __forceinline__ const double* operator()(int j) const { return base + 3 * j; } };

// takes the residual, has no Jacobian rows (the item functions are instantiated with JAC = false: none of these is ever called)
template <int ROWS>
struct ResidualSink {
  double* r;
  __device__ __forceinline__ void res(const double* v) const { for (int k = 0; k < ROWS; ++k) r[k] = v[k]; }
  __device__ __forceinline__ void zero() const {}
  __device__ __forceinline__ void so3(int, const double*) const {}
  __device__ __forceinline__ void r3(const double*, const double*) const {}
  __device__ __forceinline__ void tic(const double*) const {}
  __device__ __forceinline__ void ld(const double*) const {}
  __device__ __forceinline__ void grav(const double*) const {}
  __device__ __forceinline__ void bias(const double*, const double*) const {}
  __device__ __forceinline__ void intr(int, const double*) const {}
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// the five segment tables of one SO(3) window from the knots themselves
__device__ __forceinline__ void window_segments(const double* q, double* seg) {
#pragma unroll
  for (int i = 0; i < 5; ++i)
    so3_segment_prepare(Quat{q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]}, Quat{q[4 * i + 4], q[4 * i + 5], q[4 * i + 6], q[4 * i + 7]}, seg + i * kSegStride);
}

__global__ void __launch_bounds__(256) report_views_kernel(EvalCtx ctx, ViewData vd, const uint8_t* gate, double* e_uv, uint8_t* status,
                                                           int32_t* n_used, double* sum_sq, double* max_e) {
  const int lane = threadIdx.x & 63;
  const int64_t v = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (v >= vd.n_views) return;   // (the whole wave)
  const double* x = ctx.x;
  ViewConst vc;
  view_const_init(vc, x + ctx.pl.tic);
  vc.ld = x[ctx.pl.ld];
  vc.sh_s = ctx.rs_time_in_seconds ? ctx.inv_so3_dt : 1.0; vc.sh_r = ctx.rs_time_in_seconds ? ctx.inv_r3_dt : 1.0;
  vc.inv_so3_dt = ctx.inv_so3_dt; vc.inv_r3_dt = ctx.inv_r3_dt; vc.cam_model = ctx.cam_model; vc.intr = ctx.intr;
  vc.gs_unit_loss = true;   // no quirk Q2 here: a global-shutter view reports its error too
  vc.spline_active = false; vc.tic_active = false; vc.ld_active = false;
  const int s_so3 = vd.view_s_so3[v], s_r3 = vd.view_s_r3[v];
  const double* q = x + ctx.pl.so3 + 4 * (int64_t)s_so3;
  double seg[5 * kSegStride];
  window_segments(q, seg);
  const Quat R0{q[0], q[1], q[2], q[3]};
  const GlobalR3 kr{x + ctx.pl.r3 + 3 * (int64_t)s_r3};
  const double u_so3 = vd.view_u_so3[v], u_r3 = vd.view_u_r3[v];
  const bool rs = vd.view_rs[v] != 0;
  const int64_t c0 = vd.view_c0[v], c1 = vd.view_c0[v + 1];
  int n = 0; double ss = 0.0, mx = 0.0;
  for (int64_t c = c0 + lane; c < c1; c += 64) {
    double r[2] = {0.0, 0.0};
    const ResidualSink<2> sink{r};
    view_item<false>(vc, R0, LocalSeg{seg}, kr, u_so3, u_r3, rs, vd.corner_u[c], vd.corner_v[c], 1.0, 1.0,
                     x + ctx.pl.pts + 4 * (int64_t)vd.corner_pt[c], sink);
    const bool failed = r[0] == 1e10 && r[1] == 1e10;   // ceres_calib_split_residuals.h:391-393
    const uint8_t st = failed ? 1 : (gate[c] ? 2 : 0);
    e_uv[2 * c] = r[0]; e_uv[2 * c + 1] = r[1]; status[c] = st;
    if (st == 0) { const double m2 = r[0] * r[0] + r[1] * r[1]; ++n; ss += m2; mx = fmax(mx, m2); }
  }
  n = wave_sum_int(n); ss = wave_sum(ss); mx = wave_max(mx);
  if (lane == 0) { n_used[v] = n; sum_sq[v] = ss; max_e[v] = sqrt(mx); }
}

// KIND 0 accelerometer, 1 gyroscope.  r3 [n][3] unweighted residuals, partials [ceil(n / 64)][6] = sum r^2 (x y z), sum (w r)^2 (x y z)
template <int KIND>
__global__ void __launch_bounds__(256) report_imu_kernel(EvalCtx ctx, ImuData id, double* r3, double* partials) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i - lane >= id.n) return;   // (the whole wave)
  const double* x = ctx.x;
  double r[3] = {0.0, 0.0, 0.0}, w = 0.0;
  if (i < id.n) {
    ImuConst ic;
    ic.inv_so3_dt = ctx.inv_so3_dt; ic.inv_r3_dt = ctx.inv_r3_dt;
    imu_const_init<KIND>(ic, x + (KIND == 0 ? ctx.pl.ai : ctx.pl.gi), x + ctx.pl.g);
    ic.spline_active = false; ic.g_active = false; ic.bias_active = false; ic.intr_active = false;
    const double* q = x + ctx.pl.so3 + 4 * (int64_t)id.s_so3[i];
    double seg[5 * kSegStride];
    window_segments(q, seg);
    const GlobalR3 kr{x + ctx.pl.r3 + 3 * (int64_t)(KIND == 0 ? id.s_r3[i] : 0)};
    const double* bk = x + (KIND == 0 ? ctx.pl.ab : ctx.pl.gb) + 3 * (int64_t)id.s_b[i];
    const double m[3] = {id.mx[i], id.my[i], id.mz[i]};
    const ResidualSink<3> sink{r};
    imu_item<KIND, false>(ic, Quat{q[0], q[1], q[2], q[3]}, LocalSeg{seg}, kr, id.u_so3[i], KIND == 0 ? id.u_r3[i] : 0.0, id.u_b[i], bk, m, 1.0, sink);
    r3[3 * i] = r[0]; r3[3 * i + 1] = r[1]; r3[3 * i + 2] = r[2];
    w = id.w[i];
  }
  double s[6];
#pragma unroll
  for (int k = 0; k < 3; ++k) { s[k] = wave_sum(r[k] * r[k]); const double wr = w * r[k]; s[3 + k] = wave_sum(wr * wr); }
  if (lane == 0) {
    double* o = partials + 6 * (i >> 6);
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = s[k];
  }
}

}  // namespace

// e_uv [n_corners][2], status [n_corners], n_used / sum_sq / max_e [n_views]; gate [n_corners] (1: the corner carries no weight)
void launch_report_views(const EvalCtx& ctx, const ViewData& vd, const uint8_t* gate, double* e_uv, uint8_t* status, int32_t* n_used,
                         double* sum_sq, double* max_e, hipStream_t st) {
  if (vd.n_views <= 0) return;
  const int grid = int((vd.n_views + 3) / 4);   // four waves = four views per workgroup
  hipLaunchKernelGGL(report_views_kernel, dim3(grid), dim3(256), 0, st, ctx, vd, gate, e_uv, status, n_used, sum_sq, max_e);
}
// kind 1 accelerometer, 2 gyroscope (the residual families of oicc_evaluate_blocks); partials: [(n + 63) / 64][6]
void launch_report_imu(const EvalCtx& ctx, const ImuData& id, int kind, double* r3, double* partials, hipStream_t st) {
  if (id.n <= 0) return;
  const int grid = int((id.n + 255) / 256);
  if (kind == 1) hipLaunchKernelGGL(report_imu_kernel<0>, dim3(grid), dim3(256), 0, st, ctx, id, r3, partials);
  else hipLaunchKernelGGL(report_imu_kernel<1>, dim3(grid), dim3(256), 0, st, ctx, id, r3, partials);
}

}  // namespace oicc
