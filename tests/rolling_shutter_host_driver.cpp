// Stand-alone driver of the host preparation of rectify_rolling_shutter (csrc/host/rolling_shutter.hpp): corrected gyroscope
// rates, frame times from file names and the reading of the result JSON, with no device call.  tests/
// test_rolling_shutter_restatement.py compiles it plain and with -fsanitize=address,undefined, runs it on files it wrote and
// compares the printed numbers with the Python twin.
//
//   rolling_shutter_host_driver <telemetry.json> <result.json> <imu_intrinsics.json or -> <imu_bias.json or -> <name.png>...
#include <cstdio>
#include <string>
#include <vector>

#include "host/rolling_shutter.hpp"

int main(int argc, char* argv[]) {
  using namespace oicc_cli;
  namespace rsh = OpenICC::rolling_shutter;
  if (argc < 5) { std::fprintf(stderr, "usage: %s telemetry result intrinsics bias [names]\n", argv[0]); return 2; }
  const auto path = [](const char* a) { return std::string(a) == "-" ? std::string() : std::string(a); };
  CameraTelemetryData telemetry;
  if (!ReadTelemetryJSON(argv[1], &telemetry)) { std::fprintf(stderr, "telemetry\n"); return 1; }
  std::string err;
  rsh::Scene scene;
  if (!rsh::ReadImuCameraResult(argv[2], &scene.calib, &err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
  rsh::ImuCameraResult missing;
  if (rsh::ReadImuCameraResult(argv[1], &missing, &err)) { std::fprintf(stderr, "the telemetry file passed as a result file\n"); return 1; }
  ThreeAxisSensorCalibParams acc, gyr;
  if (!ReadIMUIntrinsics(path(argv[3]), path(argv[4]), &acc, &gyr)) { std::fprintf(stderr, "intrinsics\n"); return 1; }
  rsh::CorrectedGyro(telemetry, gyr, &scene.gyro_t, &scene.gyro_rates);
  const double t_offset = telemetry.img_timestamps_s.empty() ? 0.0 : telemetry.img_timestamps_s[0];
  std::printf("result %.17g %.17g %.17g %.17g %.17g %.17g\n", scene.calib.q_i_c[0], scene.calib.q_i_c[1], scene.calib.q_i_c[2], scene.calib.q_i_c[3],
              scene.calib.time_offset_imu_to_cam_s, scene.calib.line_delay_s);
  for (size_t i = 0; i < scene.gyro_t.size(); ++i)
    std::printf("gyro %.17g %.17g %.17g %.17g\n", scene.gyro_t[i], scene.gyro_rates[3 * i], scene.gyro_rates[3 * i + 1], scene.gyro_rates[3 * i + 2]);
  for (int a = 5; a < argc; ++a) {
    double t = 0.0;
    if (rsh::FrameTimeFromName(argv[a], t_offset, &t)) { std::printf("frame %s %.17g\n", argv[a], t); scene.frame_t.push_back(t); }
    else std::printf("frame %s refused\n", argv[a]);
  }
  scene.src_intr = {1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0}; scene.dst_intr = scene.src_intr;
  const oicc_rs_scene c = scene.c();
  std::printf("scene %lld %d\n", (long long)c.num_gyro, int(c.num_frames));
  return c.gyro_t == scene.gyro_t.data() && c.frame_t == scene.frame_t.data() ? 0 : 1;
}
