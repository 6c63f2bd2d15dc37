// Host side of the stabilisation for stabilize_frames.cpp, the C++ twin of openimucameracalibrator_amd/stabilize_frames.py: the
// zoom mode by name, the frames in the order of their times, and the plan file (include/oicc_hip.h, "stabilisation"; DESIGN.md,
// "Stabilisation").  Nothing here touches the device.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

namespace OpenICC {
namespace stabilization {

// none / fixed / dynamic -> 0 / 1 / 2 (oicc_stab_options.zoom_mode)
inline bool ZoomModeFromName(const std::string& name, int* mode) {
  const char* const names[3] = {"none", "fixed", "dynamic"};
  for (int k = 0; k < 3; ++k)
    if (name == names[k]) { *mode = k; return true; }
  return false;
}

// the frames by time, equal times in the order given: file names sort as text, their times need not
inline std::vector<size_t> OrderByTime(const std::vector<double>& times) {
  std::vector<size_t> order(times.size());
  std::iota(order.begin(), order.end(), size_t(0));
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return times[a] < times[b]; });
  return order;
}

// a double as 17 significant digits, null where it is not finite
inline std::string JsonNumber(double v) {
  if (!std::isfinite(v)) return "null";
  char buf[40];
  std::snprintf(buf, sizeof(buf), "%.17g", v);
  return buf;
}

// what oicc_stab_plan_level returns on top of oicc_stab_plan, over the frames
struct LevelArrays {
  std::vector<double> level_q, up, roll, level_angle;      // [n][4], [n][3], [n], [n]
  std::vector<int32_t> gravity_samples, level_status;

  explicit LevelArrays(size_t n = 0) : level_q(4 * n), up(3 * n), roll(n), level_angle(n), gravity_samples(n), level_status(n) {}
};

// names without quotes or backslashes (they are <timestamp_ns>.png).  One line per frame.  level: the horizon lock is on, and
// every frame also gets level_q, up, roll, level_angle, gravity_samples and level_status.
inline std::string PlanJson(const std::vector<std::string>& names, const std::vector<int32_t>& status, const std::vector<double>& correction_q,
                            const std::vector<double>& required_zoom, const std::vector<double>& zoom, const std::vector<uint8_t>& zoom_clamped,
                            const LevelArrays* level = nullptr) {
  std::string s = "{\"frames\": [";
  for (size_t k = 0; k < names.size(); ++k) {
    s += k ? ",\n" : "\n";
    s += " {\"name\": \"" + names[k] + "\", \"status\": " + std::to_string(status[k]) + ", \"correction_q\": [";
    for (int c = 0; c < 4; ++c) s += (c ? ", " : "") + JsonNumber(correction_q[4 * k + size_t(c)]);
    s += "], \"required_zoom\": " + JsonNumber(required_zoom[k]) + ", \"zoom\": " + JsonNumber(zoom[k]) + ", \"zoom_clamped\": " +
         std::to_string(int(zoom_clamped[k]));
    if (level) {
      s += ", \"level_q\": [";
      for (int c = 0; c < 4; ++c) s += (c ? ", " : "") + JsonNumber(level->level_q[4 * k + size_t(c)]);
      s += "], \"up\": [";
      for (int c = 0; c < 3; ++c) s += (c ? ", " : "") + JsonNumber(level->up[3 * k + size_t(c)]);
      s += "], \"roll\": " + JsonNumber(level->roll[k]) + ", \"level_angle\": " + JsonNumber(level->level_angle[k]) + ", \"gravity_samples\": " +
           std::to_string(level->gravity_samples[k]) + ", \"level_status\": " + std::to_string(level->level_status[k]);
    }
    s += "}";
  }
  s += "\n]}\n";
  return s;
}

}  // namespace stabilization
}  // namespace OpenICC
