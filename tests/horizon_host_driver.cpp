// Stand-alone driver of the host preparation of the horizon lock in stabilize_frames (csrc/host/rolling_shutter.hpp: the corrected
// accelerometer; cli_common.hpp: the accelerometer part of the intrinsics and bias files; csrc/host/stabilization.hpp: the plan file
// with the level's keys), with no device call.  tests/test_horizon_restatement.py compiles it plain and with
// -fsanitize=address,undefined, runs it on files it wrote and compares what it prints with the Python twin.
//
//   horizon_host_driver <telemetry.json> <imu_intrinsics.json or -> <imu_bias.json or -> <n> then per frame
//     <name> <status> <w> <x> <y> <z> <required> <zoom> <clamped> <level w x y z> <up x y z> <roll> <angle> <samples> <level status>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "host/rolling_shutter.hpp"
#include "host/stabilization.hpp"

int main(int argc, char* argv[]) {
  using namespace oicc_cli;
  namespace rsh = OpenICC::rolling_shutter;
  namespace sth = OpenICC::stabilization;
  if (argc < 5) { std::fprintf(stderr, "usage: %s telemetry intrinsics bias n frames\n", argv[0]); return 2; }
  const auto path = [](const char* a) { return std::string(a) == "-" ? std::string() : std::string(a); };
  CameraTelemetryData telemetry;
  if (!ReadTelemetryJSON(argv[1], &telemetry)) { std::fprintf(stderr, "telemetry\n"); return 1; }
  ThreeAxisSensorCalibParams acc, gyr;
  if (!ReadIMUIntrinsics(path(argv[2]), path(argv[3]), &acc, &gyr)) { std::fprintf(stderr, "intrinsics\n"); return 1; }
  std::printf("intrinsics");
  for (int k = 0; k < 3; ++k) std::printf(" %s", sth::JsonNumber(acc.mis[k]).c_str());
  for (int k = 0; k < 3; ++k) std::printf(" %s", sth::JsonNumber(acc.scale[k]).c_str());
  std::printf("\nbias %s %s %s\n", sth::JsonNumber(acc.bias[0]).c_str(), sth::JsonNumber(acc.bias[1]).c_str(), sth::JsonNumber(acc.bias[2]).c_str());
  std::vector<double> t, a;
  rsh::CorrectedAccl(telemetry, acc, &t, &a);
  for (size_t i = 0; i < t.size(); ++i)
    std::printf("%s %s %s %s\n", sth::JsonNumber(t[i]).c_str(), sth::JsonNumber(a[3 * i]).c_str(), sth::JsonNumber(a[3 * i + 1]).c_str(),
                sth::JsonNumber(a[3 * i + 2]).c_str());
  const int n = std::atoi(argv[4]);
  const int per = 20;
  if (n < 0 || argc != 5 + per * n) { std::fprintf(stderr, "%d arguments for %d frames\n", argc, n); return 2; }
  std::vector<std::string> names; std::vector<int32_t> status; std::vector<double> q, required, zoom; std::vector<uint8_t> clamped;
  sth::LevelArrays level{size_t(n)};
  for (int k = 0; k < n; ++k) {
    char** f = argv + 5 + per * k;
    names.push_back(f[0]); status.push_back(std::atoi(f[1]));
    for (int c = 0; c < 4; ++c) q.push_back(std::strtod(f[2 + c], nullptr));
    required.push_back(std::strtod(f[6], nullptr)); zoom.push_back(std::strtod(f[7], nullptr)); clamped.push_back(uint8_t(std::atoi(f[8])));
    for (int c = 0; c < 4; ++c) level.level_q[size_t(4 * k + c)] = std::strtod(f[9 + c], nullptr);
    for (int c = 0; c < 3; ++c) level.up[size_t(3 * k + c)] = std::strtod(f[13 + c], nullptr);
    level.roll[size_t(k)] = std::strtod(f[16], nullptr); level.level_angle[size_t(k)] = std::strtod(f[17], nullptr);
    level.gravity_samples[size_t(k)] = std::atoi(f[18]); level.level_status[size_t(k)] = std::atoi(f[19]);
  }
  std::fputs(sth::PlanJson(names, status, q, required, zoom, clamped, &level).c_str(), stdout);
  return 0;
}
