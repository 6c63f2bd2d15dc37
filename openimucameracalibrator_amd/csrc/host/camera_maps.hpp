// Host side of the camera maps for undistort_images.cpp and convert_camera_model.cpp, the C++ twin of
// openimucameracalibrator_amd/camera_maps.py: the rectified pinhole of a camera and the conversion of a camera into another
// model.  The rays come from oicc_camera_unproject, the fit runs through the ViewBundleAdjuster facade of camera_calibrator.hpp
// and the figures over the full image come from oicc_camera_discrepancy ("Camera maps").
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <string>
#include <vector>

#include "camera_calibrator.hpp"
#include "json_min.hpp"

namespace OpenICC {
namespace camera_maps {

// read_camera_calibration (cli_common.hpp) reads a PINHOLE as the reference does, without radial terms; this project's files carry
// the two radial terms of a PINHOLE (write_camera_calibration), and a map or a conversion of that camera needs them.
inline bool ReadPinholeRadialTerms(const std::string& path, int model, std::vector<double>* intr) {
  if (model != OICC_CAM_PINHOLE) return true;
  oicc_json::Value src;
  if (!oicc_json::parse_file(path, &src)) return false;
  const oicc_json::Value& in = src.at("intrinsics");
  if (in.contains("radial_distortion_1")) (*intr)[5] = in.at("radial_distortion_1").as_double();
  if (in.contains("radial_distortion_2")) (*intr)[6] = in.at("radial_distortion_2").as_double();
  return true;
}

// A distortion-free PINHOLE of the same size with its principal point at ((w - 1) / 2, (h - 1) / 2): f0 = max(hw / x_in, hh / y_in)
// makes every destination pixel see the source (barrel-type cameras), f1 = min(hw / x_out, hh / y_out) keeps the whole source border;
// f = (1 - balance) f0 + balance f1.  x_in: smallest |x| over the left and right border columns, y_in: smallest |y| over the top
// and bottom rows, x_out / y_out: largest |x| / |y| over the whole border; pixels without a ray are ignored.
inline bool RectifiedPinhole(int device, int model, const std::vector<double>& intr, int w, int h, double balance, std::vector<double>* out,
                             std::string* err) {
  std::vector<double> uv;
  for (int side = 0; side < 2; ++side) for (int v = 0; v < h; ++v) { uv.push_back(side ? double(w - 1) : 0.0); uv.push_back(double(v)); }
  const size_t ncols = uv.size() / 2;
  for (int side = 0; side < 2; ++side) for (int u = 0; u < w; ++u) { uv.push_back(double(u)); uv.push_back(side ? double(h - 1) : 0.0); }
  const size_t n = uv.size() / 2;
  std::vector<double> xy(2 * n); std::vector<uint8_t> status(n);
  const int rc = oicc_camera_unproject(device, model, intr.data(), int32_t(intr.size()), int64_t(n), uv.data(), xy.data(), status.data(), nullptr);
  if (rc != OICC_OK) { *err = "oicc_camera_unproject failed (" + std::to_string(rc) + ")"; return false; }
  const double inf = INFINITY;
  double x_in = inf, y_in = inf, x_out = 0.0, y_out = 0.0;
  size_t cols = 0, rows = 0;
  for (size_t i = 0; i < n; ++i) {
    if (status[i] != 0) continue;
    const double ax = std::fabs(xy[2 * i]), ay = std::fabs(xy[2 * i + 1]);
    if (i < ncols) { x_in = std::min(x_in, ax); ++cols; } else { y_in = std::min(y_in, ay); ++rows; }
    x_out = std::max(x_out, ax); y_out = std::max(y_out, ay);
  }
  if (!cols || !rows) { *err = "the image border has no rays"; return false; }
  const double hw = (w - 1) / 2.0, hh = (h - 1) / 2.0;
  const double f0 = std::max(hw / x_in, hh / y_in), f1 = std::min(hw / x_out, hh / y_out);
  const double f = (1.0 - balance) * f0 + balance * f1;
  if (!std::isfinite(f) || f <= 0.0) { *err = "the image is too small for a rectified pinhole"; return false; }
  *out = {f, 1.0, 0.0, hw, hh, 0.0, 0.0};
  return true;
}

// f, aspect and principal point of the source, zero distortion except EXTENDED_UNIFIED (alpha, beta) = (0.5, 1) and DOUBLE_SPHERE
// (xi, alpha) = (0, 0.5)
inline std::vector<double> ConversionStart(int model, const std::vector<double>& intr, int dst_model) {
  const bool div = model == OICC_CAM_DIVISION_UNDISTORTION, ddiv = dst_model == OICC_CAM_DIVISION_UNDISTORTION;
  std::vector<double> out(size_t(core::NumIntrinsics(dst_model)), 0.0);
  out[0] = intr[0]; out[1] = intr[1];
  out[ddiv ? 2 : 3] = intr[div ? 2 : 3]; out[ddiv ? 3 : 4] = intr[div ? 3 : 4];
  if (dst_model == OICC_CAM_EXTENDED_UNIFIED) { out[5] = 0.5; out[6] = 1.0; }
  if (dst_model == OICC_CAM_DOUBLE_SPHERE) { out[5] = 0.0; out[6] = 0.5; }
  return out;
}

struct Conversion {
  std::vector<double> intrinsics;
  double fit_rms_px = 0.0, full_image_rms_px = 0.0, full_image_max_px = 0.0;
  int64_t valid_pixels = 0, grid_points = 0;
};

// The rays of the pixel grid u = 0, stride, ..., v = 0, stride, ... are the scene points (x, y, 1, 1) of a view bundle adjustment with
// identity, constant poses, one view per grid row; only the destination intrinsics (all but the skew) vary and huber_width lies
// beyond every residual: plain least squares.  Then the discrepancy over the full-resolution image.
inline bool ConvertCameraModel(int device, int model, const std::vector<double>& intr, int w, int h, int dst_model, int stride, Conversion* out,
                               std::string* err, int max_iterations = 200) {
  std::vector<double> uv;
  int nu = 0, nv = 0;
  for (int v = 0; v < h; v += stride) { ++nv; nu = 0; for (int u = 0; u < w; u += stride) { ++nu; uv.push_back(double(u)); uv.push_back(double(v)); } }
  const size_t n = uv.size() / 2;
  std::vector<double> xy(2 * n); std::vector<uint8_t> status(n);
  int rc = oicc_camera_unproject(device, model, intr.data(), int32_t(intr.size()), int64_t(n), uv.data(), xy.data(), status.data(), nullptr);
  if (rc != OICC_OK) { *err = "oicc_camera_unproject failed (" + std::to_string(rc) + ")"; return false; }
  std::vector<std::array<double, 4>> points;
  core::BaViews views;
  for (int r = 0; r < nv; ++r) {
    std::vector<std::array<double, 3>> obs;
    for (int c = 0; c < nu; ++c) {
      const size_t i = size_t(r) * size_t(nu) + size_t(c);
      if (status[i] != 0) continue;
      obs.push_back({double(points.size()), uv[2 * i], uv[2 * i + 1]});
      points.push_back({xy[2 * i], xy[2 * i + 1], 1.0, 1.0});
    }
    if (obs.empty()) continue;
    views.pose.push_back({0.0, 0.0, 0.0, 0.0, 0.0, 0.0}); views.t_s.push_back(double(r)); views.obs.push_back(obs);
  }
  if (points.size() < size_t(2 * core::NumIntrinsics(dst_model))) { *err = "too few pixels with a ray for the fit"; return false; }
  core::ViewBundleAdjuster ba(device);
  ba.SetOption("huber_width", 1e30);                 // beyond every residual: the loss is out of play
  ba.SetOption("function_tolerance", 1e-16);
  ba.SetOption("parameter_tolerance", 1e-14);
  ba.SetOption("gradient_tolerance", 1e-16);
  ba.Upload(dst_model, ConversionStart(model, intr, dst_model), points, views);
  const int all_but_skew = core::FOCAL_LENGTH | core::ASPECT_RATIO | core::PRINCIPAL_POINTS | core::RADIAL_DISTORTION | core::TANGENTIAL_DISTORTION;
  const oicc_summary s = ba.Optimize(max_iterations, 0, core::IntrinsicsMask(dst_model, all_but_skew));
  ba.Download(&out->intrinsics, &views);
  out->grid_points = int64_t(points.size());
  out->fit_rms_px = std::sqrt(2.0 * s.final_cost / double(points.size()));
  double stats[3] = {0.0, 0.0, 0.0};
  rc = oicc_camera_discrepancy(device, model, intr.data(), dst_model, out->intrinsics.data(), w, h, stats, nullptr);
  if (rc != OICC_OK) { *err = "oicc_camera_discrepancy failed (" + std::to_string(rc) + ")"; return false; }
  out->valid_pixels = int64_t(stats[0]); out->full_image_rms_px = stats[1]; out->full_image_max_px = stats[2];
  return true;
}

}  // namespace camera_maps
}  // namespace OpenICC
