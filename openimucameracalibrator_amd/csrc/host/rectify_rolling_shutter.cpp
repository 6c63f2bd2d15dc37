// rectify_rolling_shutter -- global-shutter-equivalent copies of a folder of rolling-shutter PNG frames, from the gyroscope.
//
//   rectify_rolling_shutter --input_path DIR --telemetry_json F --camera_calibration_json F --imu_camera_calibration_json F
//                           --output_path DIR [--line_delay_us X] [--time_offset_imu_to_cam_s X] [--imu_intrinsics F]
//                           [--imu_bias_file F] [--reference_row Y] [--undistort] [--balance 0] [--output_camera_json F] [--device 0]
//
// Every <timestamp_ns>.png of the input folder (8-bit gray or RGB, the size of the calibration) is exposed row by row:
// row y at t = timestamp_ns 1e-9 + img_timestamps_ns[0] 1e-9 + y line_delay.  --imu_camera_calibration_json is the result.json of
// continuous_time_imu_to_camera_calibration (q_i_c, time_offset_imu_to_cam_s, calib_line_delay_us); the two override flags replace
// its values.  The gyroscope rates of --telemetry_json are corrected with --imu_intrinsics / --imu_bias_file and integrated;
// oicc_rs_rectify_frames resamples every frame into the camera at its reference row's time (rolling_shutter.hpp, include/oicc_hip.h
// "rolling shutter": rotation only).  --undistort makes the destination the rectified pinhole (--balance) instead of the camera
// itself; --output_camera_json receives the destination camera.  Frames without gyro coverage are not written: they are listed on
// stderr with the reason.  The twin of openimucameracalibrator_amd/rectify_rolling_shutter.py: the PNGs decode to the same arrays.
// The reference has no such application.
#include <dirent.h>
#include <sys/stat.h>

#include <algorithm>
#include <exception>
#include <iostream>
#include <string>
#include <vector>

#include "ba_cli_common.hpp"
#include "camera_maps.hpp"
#include "png_reader.hpp"
#include "png_writer.hpp"
#include "rolling_shutter.hpp"

using namespace oicc_cli;
namespace rsh = OpenICC::rolling_shutter;

namespace {

constexpr int kBatch = 16;

struct Frame { int w = 0, h = 0, c = 0; std::vector<uint8_t> px; };

// gray and gray + alpha -> 1 channel, RGB and RGBA -> RGB
bool decode(const std::string& path, Frame* f, std::string* err) {
  oicc_png::Image im;
  if (!oicc_png::read_png(path, &im, err)) return false;
  f->w = im.width; f->h = im.height; f->c = im.channels <= 2 ? 1 : 3;
  const size_t n = size_t(im.width) * size_t(im.height);
  f->px.resize(n * size_t(f->c));
  for (size_t i = 0; i < n; ++i)
    for (int c = 0; c < f->c; ++c) f->px[i * size_t(f->c) + size_t(c)] = im.pixels[i * size_t(im.channels) + size_t(c)];
  return true;
}

bool is_dir(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode); }

}  // namespace

static int run_main(int argc, char* argv[]) {
  Flags F({{"input_path", ""}, {"telemetry_json", ""}, {"camera_calibration_json", ""}, {"imu_camera_calibration_json", ""}, {"line_delay_us", ""},
           {"time_offset_imu_to_cam_s", ""}, {"imu_intrinsics", ""}, {"imu_bias_file", ""}, {"reference_row", ""}, {"undistort", "false"},
           {"balance", "0"}, {"output_camera_json", ""}, {"output_path", ""}, {"device", "0"}});
  if (!F.parse(argc, argv)) return 2;
  const std::string input = F.str("input_path"), output = F.str("output_path"), calib_json = F.str("camera_calibration_json");
  const int device = std::stoi(F.str("device"));
  CHECK_MSG(!input.empty() && !output.empty() && !calib_json.empty() && !F.str("telemetry_json").empty() && !F.str("imu_camera_calibration_json").empty(),
            "--input_path, --telemetry_json, --camera_calibration_json, --imu_camera_calibration_json and --output_path are required");
  CalibDataset cam; double fps = 0.0;
  if (!read_camera_calibration(calib_json, &cam, &fps)) return 1;
  CHECK_MSG(OpenICC::camera_maps::ReadPinholeRadialTerms(calib_json, cam.camera_model, &cam.intrinsics), "Could not open: " << calib_json);
  std::string err;
  rsh::Scene scene;
  CHECK_MSG(rsh::ReadImuCameraResult(F.str("imu_camera_calibration_json"), &scene.calib, &err), err);
  if (!F.str("line_delay_us").empty()) scene.calib.line_delay_s = F.d("line_delay_us") * 1e-6;
  if (!F.str("time_offset_imu_to_cam_s").empty()) scene.calib.time_offset_imu_to_cam_s = F.d("time_offset_imu_to_cam_s");
  CameraTelemetryData telemetry;
  CHECK_MSG(ReadTelemetryJSON(F.str("telemetry_json"), &telemetry), "Could not read: " << F.str("telemetry_json"));
  const double t_offset_cam_s = telemetry.img_timestamps_s.empty() ? 0.0 : telemetry.img_timestamps_s[0];
  ThreeAxisSensorCalibParams acc_intr, gyr_intr;
  CHECK_MSG(ReadIMUIntrinsics(F.str("imu_intrinsics"), F.str("imu_bias_file"), &acc_intr, &gyr_intr), "Could not open " << F.str("imu_intrinsics"));
  rsh::CorrectedGyro(telemetry, gyr_intr, &scene.gyro_t, &scene.gyro_rates);
  CHECK_MSG(is_dir(input), "not a folder: " << input);
  const int w = cam.image_width, h = cam.image_height;
  scene.src_model = cam.camera_model; scene.src_intr = cam.intrinsics; scene.src_w = w; scene.src_h = h;
  scene.dst_model = cam.camera_model; scene.dst_intr = cam.intrinsics; scene.dst_w = w; scene.dst_h = h;
  if (F.b("undistort")) {
    scene.dst_model = OICC_CAM_PINHOLE;
    CHECK_MSG(OpenICC::camera_maps::RectifiedPinhole(device, cam.camera_model, cam.intrinsics, w, h, F.d("balance"), &scene.dst_intr, &err), err);
  }
  scene.reference_row = F.str("reference_row").empty() ? (h - 1) / 2.0 : F.d("reference_row");

  std::vector<std::string> names;
  if (DIR* d = opendir(input.c_str())) {
    while (dirent* e = readdir(d)) {
      const std::string n = e->d_name;
      if (n.size() > 4 && n.compare(n.size() - 4, 4, ".png") == 0) names.push_back(n);
    }
    closedir(d);
  }
  std::sort(names.begin(), names.end());
  std::vector<double> times(names.size());
  for (size_t i = 0; i < names.size(); ++i)
    CHECK_MSG(rsh::FrameTimeFromName(names[i], t_offset_cam_s, &times[i]), names[i] << ": the name is not <timestamp_ns>.png");
  mkdir(output.c_str(), 0777);
  CHECK_MSG(is_dir(output), "cannot create " << output);
  size_t k = 0, written = 0;
  Frame next; bool have_next = false;
  while (k < names.size()) {                    // runs of frames with the same colour layout travel as one call
    std::vector<Frame> frames;
    if (have_next) { frames.push_back(next); have_next = false; }
    while (k + frames.size() < names.size() && int(frames.size()) < kBatch) {
      Frame f;
      CHECK_MSG(decode(input + "/" + names[k + frames.size()], &f, &err), err);
      CHECK_MSG(f.w == w && f.h == h, names[k + frames.size()] << ": " << f.w << " x " << f.h << ", the calibration is for " << w << " x " << h);
      if (!frames.empty() && f.c != frames[0].c) { next = f; have_next = true; break; }
      frames.push_back(f);
    }
    const int n = int(frames.size()), ch = frames[0].c;
    const size_t frame_bytes = size_t(w) * size_t(h) * size_t(ch);
    std::vector<uint8_t> in(frame_bytes * size_t(n)), out(frame_bytes * size_t(n));
    for (int i = 0; i < n; ++i) std::copy(frames[size_t(i)].px.begin(), frames[size_t(i)].px.end(), in.begin() + long(frame_bytes) * i);
    scene.frame_t.assign(times.begin() + long(k), times.begin() + long(k) + n);
    std::vector<int32_t> status(size_t(n), 0);
    const oicc_rs_scene c = scene.c();
    const int rc = oicc_rs_rectify_frames(device, &c, ch, in.data(), 0, kBatch, out.data(), status.data(), nullptr);
    CHECK_MSG(rc == OICC_OK, "oicc_rs_rectify_frames failed (" << rc << ")");
    for (int i = 0; i < n; ++i) {
      const std::string& name = names[k + size_t(i)];
      if (status[size_t(i)] != 0) { std::cerr << "skipped " << name << ": " << rsh::FrameStatusText(status[size_t(i)]) << std::endl; continue; }
      CHECK_MSG(oicc_png::write_png(output + "/" + name, w, h, ch, out.data() + frame_bytes * size_t(i), &err), err);
      ++written;
    }
    k += size_t(n);
  }
  if (!F.str("output_camera_json").empty()) {
    oicc_json::Value src;
    CHECK_MSG(oicc_json::parse_file(calib_json, &src), "Could not open: " << calib_json);
    const std::string type = F.b("undistort") ? std::string("PINHOLE") : src.at("intrinsic_type").as_string();
    if (!write_camera_calibration(F.str("output_camera_json"), scene.dst_model, type, scene.dst_intr, w, h, fps, 0, 0.0)) return 1;
  }
  std::cout << "rectified " << written << " of " << names.size() << " frames, line delay " << scene.calib.line_delay_s * 1e6 << " us, time offset "
            << scene.calib.time_offset_imu_to_cam_s << " s, reference row " << scene.reference_row << std::endl;
  return 0;
}

int main(int argc, char* argv[]) {
  try {
    return run_main(argc, argv);
  } catch (const std::exception& e) {
    std::cerr << "rectify_rolling_shutter: " << e.what() << std::endl;
    return 1;
  }
}
