// What the rolling-shutter rectification (rolling_shutter.hip) and the stabilisation (stabilization.hip) share: quaternions, the
// exponential of a gyro interval with a linear rate, the per-frame table of relative rotations and its kernel, R_rel at a row, the
// fixed point on the source row, and the host's judgement of an oicc_rs_scene with the frame windows.  Both units are compiled with
// -ffp-contract=off (csrc/Makefile): every sum here rounds as tests/rolling_shutter_restatement.py does.  The kernel is static and
// the host functions inline: each unit has its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>
#include "camera_device.h"

namespace oicc_rs {

using namespace oicc_camera;

constexpr int kMaxWindow = 256;          // gyro samples per frame window
constexpr int kEntry = 8;                // doubles per table entry: tau, Q' (w x y z), omega (x y z)
constexpr int kMaxEvaluations = 24;
constexpr double kRowTol = 1e-10;
constexpr int kFrameChunk = 32768;       // frames per launch (the grid's y dimension)

struct Q4 { double w, x, y, z; };

__device__ __forceinline__ Q4 qmul(const Q4& a, const Q4& b) {
  return Q4{((a.w * b.w - a.x * b.x) - a.y * b.y) - a.z * b.z, ((a.w * b.x + a.x * b.w) + a.y * b.z) - a.z * b.y,
            ((a.w * b.y - a.x * b.z) + a.y * b.w) + a.z * b.x, ((a.w * b.z + a.x * b.y) - a.y * b.x) + a.z * b.w};
}

// Exp of the rotation vector phi_j(s) = om0 s + (om1 - om0) s^2 / (2 dt): the rate is linear inside a gyro interval
__device__ __forceinline__ Q4 interval_exp(const double* om0, const double* om1, double dt, double s) {
  const double c = s * s / (2.0 * dt);
  const double p0 = om0[0] * s + (om1[0] - om0[0]) * c, p1 = om0[1] * s + (om1[1] - om0[1]) * c, p2 = om0[2] * s + (om1[2] - om0[2]) * c;
  const double th = sqrt((p0 * p0 + p1 * p1) + p2 * p2);
  const double half = th / 2.0;
  const double k = th < 1e-8 ? 0.5 - th * th / 48.0 : sin(half) / th;
  return Q4{cos(half), k * p0, k * p1, k * p2};
}

// R_rel(tau) from a frame's table (LDS or global): the interval j with tau_j <= tau, clipped to the window
__device__ __forceinline__ Q4 table_rotation(const double* tab, int count, double tau) {
  int lo = 0, hi = count - 1;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tab[mid * kEntry] <= tau) lo = mid; else hi = mid;
  }
  const double* e = tab + lo * kEntry;
  const Q4 q = {e[1], e[2], e[3], e[4]};
  return qmul(q, interval_exp(e + 5, e + kEntry + 5, e[kEntry] - e[0], tau - e[0]));
}

__device__ __forceinline__ void rotation_matrix(const Q4& q, double M[9]) {
  M[0] = 1.0 - 2.0 * (q.y * q.y + q.z * q.z); M[1] = 2.0 * (q.x * q.y - q.w * q.z); M[2] = 2.0 * (q.x * q.z + q.w * q.y);
  M[3] = 2.0 * (q.x * q.y + q.w * q.z); M[4] = 1.0 - 2.0 * (q.x * q.x + q.z * q.z); M[5] = 2.0 * (q.y * q.z - q.w * q.x);
  M[6] = 2.0 * (q.x * q.z - q.w * q.y); M[7] = 2.0 * (q.y * q.z + q.w * q.x); M[8] = 1.0 - 2.0 * (q.x * q.x + q.y * q.y);
}

struct RsParams {
  Camera src, dst;
  Rotation R;
  int src_w, src_h, dst_w, dst_h, src_closed_form, dst_closed_form;
  double line_delay, reference_row, time_offset;
};

__device__ __forceinline__ double row_tau(const RsParams& P, double row) {
  return (fmin(fmax(row, 0.0), double(P.src_h - 1)) - P.reference_row) * P.line_delay;
}

// gyro_t / rates: all samples (rates already in the camera frame); first / count: the frame's window.  table [frames][256][8].
static __global__ __launch_bounds__(64) void rs_frame_table_kernel(int num_frames, const double* __restrict__ gyro_t, const double* __restrict__ rates,
                                                                   const double* __restrict__ frame_t, const int64_t* __restrict__ first,
                                                                   const int32_t* __restrict__ count, double time_offset, double reference_delay,
                                                                   double* __restrict__ table) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= num_frames) return;
  const int n = count[k];
  if (n < 2) return;
  const double* t = gyro_t + first[k];
  const double* om = rates + 3 * first[k];
  double* tab = table + int64_t(k) * kMaxWindow * kEntry;
  const double tk = frame_t[k];
  // times as differences first: absolute times reach 1e4 s
  Q4 q = {1.0, 0.0, 0.0, 0.0};
  double tau = ((t[0] - tk) + time_offset) - reference_delay;
  int jr = 0;
  Q4 q_jr = q;
  double tau_jr = tau;
  for (int j = 0; j < n; ++j) {
    double* e = tab + j * kEntry;
    e[0] = tau; e[1] = q.w; e[2] = q.x; e[3] = q.y; e[4] = q.z; e[5] = om[3 * j]; e[6] = om[3 * j + 1]; e[7] = om[3 * j + 2];
    if (j <= n - 2 && (j == 0 || tau <= 0.0)) { jr = j; q_jr = q; tau_jr = tau; }     // the interval of t_ref, clipped to the window
    if (j + 1 < n) {
      const double next = ((t[j + 1] - tk) + time_offset) - reference_delay;
      q = qmul(q, interval_exp(om + 3 * j, om + 3 * j + 3, next - tau, next - tau));
      tau = next;
    }
  }
  const double dt = tab[(jr + 1) * kEntry] - tau_jr;
  const Q4 qref = qmul(q_jr, interval_exp(om + 3 * jr, om + 3 * jr + 3, dt, 0.0 - tau_jr));
  const Q4 inv = {qref.w, -qref.x, -qref.y, -qref.z};
  for (int j = 0; j < n; ++j) {
    double* e = tab + j * kEntry;
    const Q4 r = qmul(inv, Q4{e[1], e[2], e[3], e[4]});
    e[1] = r.w; e[2] = r.x; e[3] = r.y; e[4] = r.z;
  }
}

// The fixed point on the source row of one destination ray (x, y, 1), rotated by R (row-major: P.R of the call, or a frame's own in
// the stabilisation).  tab: the frame's table in LDS.
__device__ __forceinline__ bool solve_pixel(const RsParams& P, const double* R, const double* tab, int count, double x, double y, bool ok, double px[2],
                                            int& evaluations) {
  const double p[3] = {(R[0] * x + R[1] * y) + R[2], (R[3] * x + R[4] * y) + R[5], (R[6] * x + R[7] * y) + R[8]};
  px[0] = 0.0; px[1] = 0.0;
  evaluations = 0;
  ok = ok && p[2] > 0.0;
  if (!ok) return false;
  double row = P.reference_row;
  bool converged = false;
  for (int it = 0; it < kMaxEvaluations; ++it) {
    double M[9];
    rotation_matrix(table_rotation(tab, count, row_tau(P, row)), M);
    const double d[3] = {(M[0] * p[0] + M[3] * p[1]) + M[6] * p[2], (M[1] * p[0] + M[4] * p[1]) + M[7] * p[2], (M[2] * p[0] + M[5] * p[1]) + M[8] * p[2]};   // R_rel^T p
    ++evaluations;
    if (!(d[2] > 0.0) || !oicc::camera_project<false>(P.src.model, P.src.in, d, px, nullptr) || !isfinite(px[0]) || !isfinite(px[1])) return false;
    const double step = fabs(px[1] - row);
    row = px[1];
    if (step <= kRowTol * (1.0 + fabs(row))) { converged = true; break; }
  }
  return converged && px[0] >= 0.0 && px[0] <= double(P.src_w - 1) && px[1] >= 0.0 && px[1] <= double(P.src_h - 1);
}

// stages the table of frame blockIdx.y in LDS; false (for the whole workgroup) when the frame has none
__device__ __forceinline__ bool stage_table(const double* __restrict__ table, const int32_t* __restrict__ count, int frame, double* lds, int& n) {
  n = count[frame];
  if (n < 2) return false;
  const double* src = table + int64_t(frame) * kMaxWindow * kEntry;
  for (int i = threadIdx.x; i < n * kEntry; i += kThreads) lds[i] = src[i];
  __syncthreads();
  return true;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------

// What every entry judges before it looks for a device, and the frame windows, found by time comparisons only.
struct Judged {
  RsParams P;
  int num_frames = 0;
  int64_t num_gyro = 0;
  std::vector<double> rates_cam;       // [n][3]
  std::vector<int64_t> first;          // [frames] first window sample
  std::vector<int32_t> count, status;  // [frames] window samples (0 where status != 0), oicc frame status
};

inline bool all_finite(const double* a, int64_t n) {
  for (int64_t i = 0; i < n; ++i) if (!std::isfinite(a[i])) return false;
  return true;
}

inline int judge(const oicc_rs_scene* s, Judged* J) {
  if (!s) return OICC_ERR_INVALID_ARG;
  RsParams& P = J->P;
  if (!make_camera(s->src_model, s->src_intr, &P.src) || !make_camera(s->dst_model, s->dst_intr, &P.dst) || s->src_w < 1 || s->src_h < 1 ||
      s->dst_w < 1 || s->dst_h < 1 || int64_t(s->dst_w) * s->dst_h > kMaxLanes) return OICC_ERR_INVALID_ARG;
  P.R = Rotation{{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}};
  if (s->R9) {
    if (!all_finite(s->R9, 9)) return OICC_ERR_INVALID_ARG;
    for (int k = 0; k < 9; ++k) P.R.r[k] = s->R9[k];
  }
  if (s->num_gyro < 2 || !s->gyro_t || !s->gyro_rates || s->num_frames < 1 || !s->frame_t) return OICC_ERR_INVALID_ARG;
  if (!all_finite(s->gyro_t, s->num_gyro) || !all_finite(s->gyro_rates, 3 * s->num_gyro) || !all_finite(s->frame_t, s->num_frames) ||
      !all_finite(s->q_i_c, 4) || !std::isfinite(s->time_offset_imu_to_cam) || !std::isfinite(s->line_delay_s) ||
      !std::isfinite(s->reference_row)) return OICC_ERR_INVALID_ARG;
  for (int64_t j = 1; j < s->num_gyro; ++j) if (!(s->gyro_t[j] > s->gyro_t[j - 1])) return OICC_ERR_INVALID_ARG;
  const double* qi = s->q_i_c;
  const double norm = std::sqrt(((qi[0] * qi[0] + qi[1] * qi[1]) + qi[2] * qi[2]) + qi[3] * qi[3]);
  if (!(std::fabs(norm - 1.0) <= 1e-6)) return OICC_ERR_INVALID_ARG;
  P.src_w = s->src_w; P.src_h = s->src_h; P.dst_w = s->dst_w; P.dst_h = s->dst_h;
  P.src_closed_form = is_plain_pinhole(P.src); P.dst_closed_form = is_plain_pinhole(P.dst);
  P.line_delay = s->line_delay_s; P.reference_row = s->reference_row; P.time_offset = s->time_offset_imu_to_cam;
  J->num_frames = s->num_frames; J->num_gyro = s->num_gyro;
  // rates into the camera frame, once: T_i_c takes camera coordinates to IMU coordinates, so omega_c = R(q_i_c)^T omega_i
  {
    const double w = qi[0] / norm, x = qi[1] / norm, y = qi[2] / norm, z = qi[3] / norm;
    const double M[9] = {1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                         2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
                         2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)};
    J->rates_cam.resize(size_t(3 * s->num_gyro));
    for (int64_t j = 0; j < s->num_gyro; ++j) {
      const double* o = s->gyro_rates + 3 * j;
      for (int c = 0; c < 3; ++c) J->rates_cam[size_t(3 * j + c)] = (M[c] * o[0] + M[3 + c] * o[1]) + M[6 + c] * o[2];
    }
  }
  // windows: the row times of y in [0, src_h - 1] together with t_ref, relative to the frame time, against a_j = (t_j - t_k) + offset
  const double last = double(s->src_h - 1) * s->line_delay_s, ref = s->reference_row * s->line_delay_s;
  const double lo = std::min(std::min(0.0, last), ref), hi = std::max(std::max(0.0, last), ref);
  const int64_t n = s->num_gyro;
  J->first.assign(size_t(s->num_frames), 0); J->count.assign(size_t(s->num_frames), 0); J->status.assign(size_t(s->num_frames), 0);
  for (int k = 0; k < s->num_frames; ++k) {
    const double tk = s->frame_t[k], off = s->time_offset_imu_to_cam;
    auto a = [&](int64_t j) { return (s->gyro_t[j] - tk) + off; };
    if (lo < a(0) || hi > a(n - 1)) { J->status[size_t(k)] = 1; continue; }
    int64_t b = 0, e = n;                       // number of samples with a_j <= lo
    while (b < e) { const int64_t m = (b + e) / 2; if (a(m) <= lo) b = m + 1; else e = m; }
    const int64_t j0 = std::min(b - 1, n - 2);
    b = 0; e = n;                               // number of samples with a_j < hi
    while (b < e) { const int64_t m = (b + e) / 2; if (a(m) < hi) b = m + 1; else e = m; }
    const int64_t j1 = std::max(b, j0 + 1);
    if (j1 - j0 + 1 > kMaxWindow) { J->status[size_t(k)] = 2; continue; }
    J->first[size_t(k)] = j0; J->count[size_t(k)] = int32_t(j1 - j0 + 1);
  }
  return OICC_OK;
}

}  // namespace oicc_rs
