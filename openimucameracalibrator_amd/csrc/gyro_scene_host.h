// The host rules of the gyro warps (rolling_shutter.hip, stabilization.hip): everything the host decides by time comparisons before
// a device is looked for, the applied zoom, and the argument checks.  No HIP here, so that tests/gyro_scene_host_driver.cpp can
// drive every rule on the host alone, plain and under the sanitizers.  Times are differenced first, ((t_j - t_k) + offset) -
// reference delay: absolute times reach 1e4 s.  The units are compiled with -ffp-contract=off and so is the driver: every sum here
// rounds as the restatements in tests/ do.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>
#include "../../include/oicc_hip.h"

namespace oicc_rs {

constexpr int kMaxWindow = 256;          // gyro samples per frame window

inline bool all_finite(const double* a, int64_t n) {
  for (int64_t i = 0; i < n; ++i) if (!std::isfinite(a[i])) return false;
  return true;
}

// the time of the reference row behind row 0: one product, wherever it is needed
inline double reference_delay(double reference_row, double line_delay) { return reference_row * line_delay; }
inline double quaternion_norm(const double* q) { return std::sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]); }

// R(q / |q|), row-major, q = (w, x, y, z): the host's only copy of the formula (the device's is rotation_matrix)
inline void unit_rotation(const double* q, double M[9]) {
  const double norm = quaternion_norm(q);
  const double w = q[0] / norm, x = q[1] / norm, y = q[2] / norm, z = q[3] / norm;
  M[0] = 1.0 - 2.0 * (y * y + z * z); M[1] = 2.0 * (x * y - w * z); M[2] = 2.0 * (x * z + w * y);
  M[3] = 2.0 * (x * y + w * z); M[4] = 1.0 - 2.0 * (x * x + z * z); M[5] = 2.0 * (y * z - w * x);
  M[6] = 2.0 * (x * z - w * y); M[7] = 2.0 * (y * z + w * x); M[8] = 1.0 - 2.0 * (x * x + y * y);
}

// rates into the camera frame, once: T_i_c takes camera coordinates to IMU coordinates, so omega_c = R(q_i_c)^T omega_i.  out [n][3]
inline void rates_cam(int64_t n, const double* rates_imu, const double* q_i_c, double* out) {
  double M[9];
  unit_rotation(q_i_c, M);
  for (int64_t j = 0; j < n; ++j) {
    const double* o = rates_imu + 3 * j;
    for (int c = 0; c < 3; ++c) out[3 * j + c] = (M[c] * o[0] + M[3 + c] * o[1]) + M[6 + c] * o[2];
  }
}

// The frame windows: the row times of y in [0, src_h - 1] together with t_ref, relative to the frame time, against
// a_j = (t_j - t_k) + offset.  first / count [frames]: the window's samples (0 where status != 0); status: 0, 1 not covered by the
// gyro, 2 more than kMaxWindow samples.
inline void frame_windows(int64_t n, const double* gyro_t, int frames, const double* frame_t, double offset, double line_delay, double reference_row,
                          int src_h, int64_t* first, int32_t* count, int32_t* status) {
  const double last = double(src_h - 1) * line_delay, ref = reference_delay(reference_row, line_delay);
  const double lo = std::min(std::min(0.0, last), ref), hi = std::max(std::max(0.0, last), ref);
  for (int k = 0; k < frames; ++k) {
    first[k] = 0; count[k] = 0; status[k] = 0;
    const double tk = frame_t[k];
    auto a = [&](int64_t j) { return (gyro_t[j] - tk) + offset; };
    if (lo < a(0) || hi > a(n - 1)) { status[k] = 1; continue; }
    int64_t b = 0, e = n;                       // number of samples with a_j <= lo
    while (b < e) { const int64_t m = (b + e) / 2; if (a(m) <= lo) b = m + 1; else e = m; }
    const int64_t j0 = std::min(b - 1, n - 2);
    b = 0; e = n;                               // number of samples with a_j < hi
    while (b < e) { const int64_t m = (b + e) / 2; if (a(m) < hi) b = m + 1; else e = m; }
    const int64_t j1 = std::max(b, j0 + 1);
    if (j1 - j0 + 1 > kMaxWindow) { status[k] = 2; continue; }
    first[k] = j0; count[k] = int32_t(j1 - j0 + 1);
  }
}

// The path by time comparisons: tau_j = ((t_j - t_k) + offset) - refd, frame k on the path when tau_0 <= 0 <= tau_{n-1}.
// interval [frames]: the gyro interval of t_ref (0 off the path).  OICC_ERR_INVALID_ARG for on-path frames that are not contiguous.
inline int find_path(int64_t n, const double* gyro_t, int frames, const double* frame_t, double offset, double refd, int64_t* interval, int* first_out,
                     int* count_out) {
  int first = 0, count = 0;
  for (int k = 0; k < frames; ++k) {
    interval[k] = 0;
    auto tau = [&](int64_t j) { return ((gyro_t[j] - frame_t[k]) + offset) - refd; };
    if (tau(0) > 0.0 || tau(n - 1) < 0.0) continue;
    if (count == 0) first = k;
    if (first + count != k) return OICC_ERR_INVALID_ARG;      // contiguous by the order of the times; anything else is not a clip
    ++count;
    int64_t b = 0, e = n;                                       // number of samples with tau_j <= 0
    while (b < e) { const int64_t m = (b + e) / 2; if (tau(m) <= 0.0) b = m + 1; else e = m; }
    interval[k] = std::min(b - 1, n - 2);
  }
  *first_out = first; *count_out = count;
  return OICC_OK;
}

// The smoothing windows of the on-path frames [first, first + count), frame indices with both ends included (0 off the path):
// |frame_t[m] - frame_t[k]| <= 3 sigma, t_ref,m - t_ref,k = frame_t[m] - frame_t[k].  frame_t strictly increasing.
inline void smoothing_windows(int frames, const double* frame_t, int first, int count, double sigma, int32_t* win_lo, int32_t* win_hi) {
  for (int k = 0; k < frames; ++k) { win_lo[k] = 0; win_hi[k] = 0; }
  int lo = first, hi = first;
  for (int k = first; k < first + count; ++k) {
    while (frame_t[k] - frame_t[lo] > 3.0 * sigma) ++lo;
    if (hi < k) hi = k;
    while (hi + 1 < first + count && frame_t[hi + 1] - frame_t[k] <= 3.0 * sigma) ++hi;
    win_lo[k] = lo; win_hi[k] = hi;
  }
}

// What the host decides for the horizon lock, s_jk = ((accl_t[j] - frame_t[k]) + offset) - refd:
//   frame_of [na]         the last on-path frame with s_jk >= 0; -1 before the first reference time or behind the last
//   sample_interval [na]  the last gyro interval i <= n - 2 with tau_i(k) <= s_jk (0 for an unused sample)
//   win_lo, win_hi [frames]  the used samples with |s_jk| <= 3 sigma_g, both ends included; hi < lo: none
inline void level_windows(int64_t n, const double* gyro_t, int frames, const double* frame_t, double offset, double refd, int64_t na,
                          const double* accl_t, double gravity_sigma, int first, int count, int32_t* frame_of, int64_t* sample_interval,
                          int64_t* win_lo, int64_t* win_hi) {
  const double reach = 3.0 * gravity_sigma;
  auto s = [&](int64_t j, int k) { return ((accl_t[j] - frame_t[k]) + offset) - refd; };
  for (int64_t j = 0; j < na; ++j) { frame_of[j] = -1; sample_interval[j] = 0; }
  for (int k = 0; k < frames; ++k) { win_lo[k] = 0; win_hi[k] = -1; }
  if (count < 1) return;
  const int last = first + count - 1;
  int64_t used_lo = na, used_hi = -1;
  for (int64_t j = 0; j < na; ++j) {
    if (!(s(j, first) >= 0.0) || s(j, last) > 0.0) continue;
    int b = first, e = last + 1;                                 // number of on-path frames with s_jk >= 0, from `first`
    while (b < e) { const int m = (b + e) / 2; if (s(j, m) >= 0.0) b = m + 1; else e = m; }
    const int k = b - 1;
    const double sj = s(j, k);
    auto tau = [&](int64_t i) { return ((gyro_t[i] - frame_t[k]) + offset) - refd; };
    int64_t gb = 0, ge = n;                                      // number of gyro samples with tau_i <= s_jk
    while (gb < ge) { const int64_t m = (gb + ge) / 2; if (tau(m) <= sj) gb = m + 1; else ge = m; }
    frame_of[j] = k;
    sample_interval[j] = std::max<int64_t>(std::min(gb - 1, n - 2), 0);
    used_lo = std::min(used_lo, j); used_hi = j;
  }
  for (int k = first; k <= last && used_hi >= used_lo; ++k) {
    int64_t b = used_lo, e = used_hi + 1;                        // the first used sample with s_jk >= -reach
    while (b < e) { const int64_t m = (b + e) / 2; if (s(m, k) < -reach) b = m + 1; else e = m; }
    const int64_t lo = b;
    b = used_lo; e = used_hi + 1;                                // the number of used samples with s_jk <= reach, from used_lo
    while (b < e) { const int64_t m = (b + e) / 2; if (s(m, k) <= reach) b = m + 1; else e = m; }
    win_lo[k] = lo; win_hi[k] = b - 1;
  }
}

// The applied zoom from the required one: O(frames x window).  t [frames] strictly increasing, z [frames] (used where status is 0).
// mode 0: 1; 1: the maximum; 2: the running maximum over |dt| <= T, then its Gaussian mean (sigma T / 2) over the same window, held
// inside the window's own range, so that Z_k >= z_k survives the rounding of the mean.
inline void applied_zoom(int frames, const double* t, const double* z, const int32_t* status, const oicc_stab_options& o, double* Z, uint8_t* clamped) {
  std::vector<double> Y(size_t(frames), 1.0);
  if (o.zoom_mode == 1) {
    double m = -std::numeric_limits<double>::infinity();
    for (int k = 0; k < frames; ++k) if (status[k] == 0) m = std::max(m, z[k]);
    for (int k = 0; k < frames; ++k) Z[k] = m == -std::numeric_limits<double>::infinity() ? 1.0 : m;
  } else if (o.zoom_mode == 2) {
    const double T = o.zoom_window_s, sg = T / 2.0;
    int lo = 0, hi = 0;                       // the window [lo, hi) of frame k
    std::vector<int> wlo(size_t(frames), 0), whi(size_t(frames), 0);
    for (int k = 0; k < frames; ++k) {
      while (t[k] - t[lo] > T) ++lo;
      if (hi < k + 1) hi = k + 1;
      while (hi < frames && t[hi] - t[k] <= T) ++hi;
      wlo[size_t(k)] = lo; whi[size_t(k)] = hi;
      double m = -std::numeric_limits<double>::infinity();
      for (int j = lo; j < hi; ++j) if (status[j] == 0) m = std::max(m, z[j]);
      Y[size_t(k)] = m == -std::numeric_limits<double>::infinity() ? 1.0 : m;
    }
    for (int k = 0; k < frames; ++k) {
      double num = 0.0, den = 0.0, ymin = Y[size_t(k)], ymax = Y[size_t(k)];
      for (int j = wlo[size_t(k)]; j < whi[size_t(k)]; ++j) {
        const double dt = t[j] - t[k];
        const double g = sg > 0.0 ? std::exp(-(dt * dt) / (2.0 * (sg * sg))) : 1.0;
        num += g * Y[size_t(j)]; den += g;
        ymin = std::min(ymin, Y[size_t(j)]); ymax = std::max(ymax, Y[size_t(j)]);
      }
      const double mean = ymax == ymin ? ymin : num / den;         // inf among the Y: inf, not NaN
      Z[k] = std::isnan(mean) ? ymax : std::min(std::max(mean, ymin), ymax);
    }
  } else {
    for (int k = 0; k < frames; ++k) Z[k] = 1.0;
  }
  for (int k = 0; k < frames; ++k) {
    clamped[k] = Z[k] > o.max_zoom ? 1 : 0;
    if (clamped[k]) Z[k] = o.max_zoom;
  }
}

inline bool options_ok(const oicc_stab_options* o) {
  return o && std::isfinite(o->smoothing_sigma_s) && o->smoothing_sigma_s >= 0.0 && std::isfinite(o->max_correction_rad) && o->max_correction_rad >= 0.0 &&
         o->zoom_mode >= 0 && o->zoom_mode <= 2 && std::isfinite(o->zoom_window_s) && o->zoom_window_s >= 0.0 && std::isfinite(o->max_zoom) &&
         o->max_zoom >= 1.0;
}

inline bool level_ok(const oicc_stab_level* l) {
  if (!l || l->num_accl < 1 || !l->accl_t || !l->accl || !all_finite(l->accl_t, l->num_accl) || !all_finite(l->accl, 3 * l->num_accl)) return false;
  for (int64_t j = 1; j < l->num_accl; ++j) if (!(l->accl_t[j] > l->accl_t[j - 1])) return false;
  return std::isfinite(l->gravity_sigma_s) && l->gravity_sigma_s > 0.0 && std::isfinite(l->gravity_const) && l->gravity_const > 0.0 &&
         std::isfinite(l->accl_gate) && l->accl_gate >= 0.0 && l->lock >= 0.0 && l->lock <= 1.0 && std::isfinite(l->roll_rad);
}

// correction_q [frames][4] unit within 1e-6 (used as given), zoom [frames] finite and positive
inline bool plan_arrays_ok(const double* correction_q, const double* zoom, int frames) {
  if (!correction_q || !zoom || !all_finite(correction_q, 4 * int64_t(frames)) || !all_finite(zoom, frames)) return false;
  for (int k = 0; k < frames; ++k)
    if (!(std::fabs(quaternion_norm(correction_q + 4 * k) - 1.0) <= 1e-6) || !(zoom[k] > 0.0)) return false;
  return true;
}

}  // namespace oicc_rs
