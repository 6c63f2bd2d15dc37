// Host side of the rolling-shutter rectification for rectify_rolling_shutter.cpp, the C++ twin of
// openimucameracalibrator_amd/rolling_shutter.py and rectify_rolling_shutter.py: corrected gyroscope rates, frame times from file
// names, the result JSON of the spline calibration, and the scene every oicc_rs_* entry takes (include/oicc_hip.h, "rolling
// shutter"; DESIGN.md, "Rolling-shutter rectification").  Nothing here touches the device.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "cli_common.hpp"

namespace OpenICC {
namespace rolling_shutter {

// what the spline calibration writes into result.json and this tool reads back
struct ImuCameraResult {
  double q_i_c[4] = {1.0, 0.0, 0.0, 0.0};   // w, x, y, z
  double time_offset_imu_to_cam_s = 0.0, line_delay_s = 0.0;
};

inline bool ReadImuCameraResult(const std::string& path, ImuCameraResult* out, std::string* err) {
  oicc_json::Value j;
  if (!oicc_json::parse_file(path, &j)) { *err = "Could not open: " + path; return false; }
  for (const char* key : {"q_i_c", "time_offset_imu_to_cam_s", "calib_line_delay_us"})
    if (!j.contains(key)) { *err = path + " has no " + key; return false; }
  const oicc_json::Value& q = j.at("q_i_c");
  const char* const names[4] = {"w", "x", "y", "z"};
  for (int k = 0; k < 4; ++k) {
    if (!q.contains(names[k])) { *err = path + ": q_i_c has no " + names[k]; return false; }
    out->q_i_c[k] = q.at(names[k]).as_double();
  }
  out->time_offset_imu_to_cam_s = j.at("time_offset_imu_to_cam_s").as_double();
  out->line_delay_s = j.at("calib_line_delay_us").as_double() * 1e-6;
  return true;
}

// MS_g (omega_m - b), the correction of the gyroscope residual (imu_ms_matrix of the device code): t [n] seconds, rates [n][3]
inline void CorrectedGyro(const CameraTelemetryData& telemetry, const ThreeAxisSensorCalibParams& gyr, std::vector<double>* t,
                          std::vector<double>* rates) {
  const double* m = gyr.mis; const double* s = gyr.scale;
  const double MS[9] = {s[0], -m[0] * s[1], m[1] * s[2], m[3] * s[0], s[1], -m[2] * s[2], -m[4] * s[0], m[5] * s[1], s[2]};
  const size_t n = telemetry.gyroscope.size();
  t->resize(n); rates->resize(3 * n);
  for (size_t i = 0; i < n; ++i) {
    const ImuReading& r = telemetry.gyroscope[i];
    const double d[3] = {r.v[0] - gyr.bias[0], r.v[1] - gyr.bias[1], r.v[2] - gyr.bias[2]};
    (*t)[i] = r.t_s;
    for (int k = 0; k < 3; ++k) (*rates)[3 * i + size_t(k)] = (MS[3 * k] * d[0] + MS[3 * k + 1] * d[1]) + MS[3 * k + 2] * d[2];
  }
}

// MS_a (a_m - b_a), the correction of the accelerometer residual, in CorrectedGyro's order (the accelerometer's lower misalignments
// are 0): t [n] seconds, accl [n][3] in m/s^2, up at rest
inline void CorrectedAccl(const CameraTelemetryData& telemetry, const ThreeAxisSensorCalibParams& acc, std::vector<double>* t,
                          std::vector<double>* accl) {
  const double* m = acc.mis; const double* s = acc.scale;
  const double MS[9] = {s[0], -m[0] * s[1], m[1] * s[2], m[3] * s[0], s[1], -m[2] * s[2], -m[4] * s[0], m[5] * s[1], s[2]};
  const size_t n = telemetry.accelerometer.size();
  t->resize(n); accl->resize(3 * n);
  for (size_t i = 0; i < n; ++i) {
    const ImuReading& r = telemetry.accelerometer[i];
    const double d[3] = {r.v[0] - acc.bias[0], r.v[1] - acc.bias[1], r.v[2] - acc.bias[2]};
    (*t)[i] = r.t_s;
    for (int k = 0; k < 3; ++k) (*accl)[3 * i + size_t(k)] = (MS[3 * k] * d[0] + MS[3 * k + 1] * d[1]) + MS[3 * k + 2] * d[2];
  }
}

// "<timestamp_ns>.png" -> t = name_ns 1e-9 + t_offset_cam_s (the first img_timestamps_ns of the telemetry, or 0): the rule the
// calibration program applies to view keys.  false: the name is not a decimal number followed by .png
inline bool FrameTimeFromName(const std::string& name, double t_offset_cam_s, double* t) {
  if (name.size() <= 4 || name.compare(name.size() - 4, 4, ".png") != 0) return false;
  const std::string digits = name.substr(0, name.size() - 4);
  if (digits.size() > 19) return false;
  uint64_t ns = 0;
  for (char c : digits) {
    if (c < '0' || c > '9') return false;
    ns = ns * 10 + uint64_t(c - '0');
  }
  *t = double(ns) * 1e-9 + t_offset_cam_s;
  return true;
}

// Owns the arrays an oicc_rs_scene points to.
struct Scene {
  int src_model = 0, src_w = 0, src_h = 0, dst_model = 0, dst_w = 0, dst_h = 0;
  std::vector<double> src_intr, dst_intr, gyro_t, gyro_rates, frame_t;
  ImuCameraResult calib;
  double reference_row = 0.0;

  oicc_rs_scene c() const {
    oicc_rs_scene s;
    s.src_model = src_model; s.src_w = src_w; s.src_h = src_h; s.dst_model = dst_model; s.dst_w = dst_w; s.dst_h = dst_h;
    s.src_intr = src_intr.data(); s.dst_intr = dst_intr.data(); s.R9 = nullptr;
    s.num_gyro = int64_t(gyro_t.size()); s.gyro_t = gyro_t.data(); s.gyro_rates = gyro_rates.data();
    for (int k = 0; k < 4; ++k) s.q_i_c[k] = calib.q_i_c[k];
    s.time_offset_imu_to_cam = calib.time_offset_imu_to_cam_s;
    s.num_frames = int32_t(frame_t.size()); s.reserved = 0; s.frame_t = frame_t.data();
    s.line_delay_s = calib.line_delay_s; s.reference_row = reference_row;
    return s;
  }
};

inline const char* FrameStatusText(int status) {
  return status == 1 ? "no gyro coverage" : (status == 2 ? "more than 256 gyro samples in the frame's window" : "ok");
}

}  // namespace rolling_shutter
}  // namespace OpenICC
