// stabilize_frames -- stabilised, global-shutter-equivalent copies of a folder of rolling-shutter PNG frames, from the gyroscope.
//
//   stabilize_frames --input_path DIR --telemetry_json F --camera_calibration_json F --imu_camera_calibration_json F
//                    --output_path DIR [--line_delay_us X] [--time_offset_imu_to_cam_s X] [--imu_intrinsics F] [--imu_bias_file F]
//                    [--reference_row Y] [--undistort] [--balance 0] [--output_camera_json F] [--device 0]
//                    [--smoothing_s 0.5] [--max_correction_deg 0] [--zoom_mode none|fixed|dynamic] [--zoom_window_s 1]
//                    [--max_zoom 4] [--output_plan_json F]
//                    [--horizon_lock 0] [--horizon_roll_deg 0] [--gravity_window_s 1] [--gravity_const 9.811104] [--accl_gate 0]
//
// The flags and files of rectify_rolling_shutter.  The destination is always the rectified pinhole of --balance (--undistort is
// accepted and changes nothing).  oicc_stab_plan sees the times of every <timestamp_ns>.png of the folder, in the order of their
// times: the orientation path, the smooth camera (--smoothing_s: sigma of the Gaussian window; --max_correction_deg: 0 = no bound)
// and the zoom (--zoom_mode, --zoom_window_s, --max_zoom).  Then the frames are read in chunks and oicc_stab_frames warps each
// chunk with its part of the plan (include/oicc_hip.h "stabilisation": rotation only).  --output_plan_json receives, per frame,
// name, status, correction quaternion, required and applied zoom.  --horizon_lock X in (0, 1] turns the horizon lock on
// (oicc_stab_plan_level): the accelerometer of the telemetry, corrected by the accelerometer part of --imu_intrinsics and
// --imu_bias_file, gives gravity over a Gaussian window of sigma --gravity_window_s, and the part X of the smooth camera's roll
// against --horizon_roll_deg is taken out (--accl_gate G: samples whose norm is further than G from --gravity_const are left out;
// 0 = no gate); the plan file then also holds level_q, up, roll, level_angle, gravity_samples and level_status per frame.  With
// --horizon_lock 0 the PNGs and the plan file are what they are without these flags.  Frames without gyro coverage are not written: they are listed
// on stderr with the reason.  The twin of openimucameracalibrator_amd/stabilize_frames.py: the same PNGs, the same plan file.
// The reference has no such application.
#include <dirent.h>
#include <sys/stat.h>

#include <algorithm>
#include <exception>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "ba_cli_common.hpp"
#include "camera_maps.hpp"
#include "png_reader.hpp"
#include "png_writer.hpp"
#include "rolling_shutter.hpp"
#include "stabilization.hpp"

using namespace oicc_cli;
namespace rsh = OpenICC::rolling_shutter;
namespace sth = OpenICC::stabilization;

namespace {

constexpr int kBatch = 16;
constexpr double kPi = 3.14159265358979323846;

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
           {"balance", "0"}, {"output_camera_json", ""}, {"output_path", ""}, {"device", "0"}, {"smoothing_s", "0.5"}, {"max_correction_deg", "0"},
           {"zoom_mode", "fixed"}, {"zoom_window_s", "1"}, {"max_zoom", "4"}, {"output_plan_json", ""}, {"horizon_lock", "0"}, {"horizon_roll_deg", "0"},
           {"gravity_window_s", "1"}, {"gravity_const", "9.811104"}, {"accl_gate", "0"}});
  if (!F.parse(argc, argv)) return 2;
  const std::string input = F.str("input_path"), output = F.str("output_path"), calib_json = F.str("camera_calibration_json");
  const int device = std::stoi(F.str("device"));
  CHECK_MSG(!input.empty() && !output.empty() && !calib_json.empty() && !F.str("telemetry_json").empty() && !F.str("imu_camera_calibration_json").empty(),
            "--input_path, --telemetry_json, --camera_calibration_json, --imu_camera_calibration_json and --output_path are required");
  oicc_stab_options opt;
  opt.smoothing_sigma_s = F.d("smoothing_s"); opt.max_correction_rad = F.d("max_correction_deg") * kPi / 180.0; opt.reserved = 0;
  opt.zoom_window_s = F.d("zoom_window_s"); opt.max_zoom = F.d("max_zoom");
  int mode = 0;
  CHECK_MSG(sth::ZoomModeFromName(F.str("zoom_mode"), &mode), "--zoom_mode is none, fixed or dynamic");
  opt.zoom_mode = mode;
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
  scene.dst_model = OICC_CAM_PINHOLE; scene.dst_w = w; scene.dst_h = h;
  CHECK_MSG(OpenICC::camera_maps::RectifiedPinhole(device, cam.camera_model, cam.intrinsics, w, h, F.d("balance"), &scene.dst_intr, &err), err);
  scene.reference_row = F.str("reference_row").empty() ? (h - 1) / 2.0 : F.d("reference_row");

  std::vector<std::string> listed;
  if (DIR* d = opendir(input.c_str())) {
    while (dirent* e = readdir(d)) {
      const std::string n = e->d_name;
      if (n.size() > 4 && n.compare(n.size() - 4, 4, ".png") == 0) listed.push_back(n);
    }
    closedir(d);
  }
  std::sort(listed.begin(), listed.end());
  std::vector<double> listed_t(listed.size());
  for (size_t i = 0; i < listed.size(); ++i)
    CHECK_MSG(rsh::FrameTimeFromName(listed[i], t_offset_cam_s, &listed_t[i]), listed[i] << ": the name is not <timestamp_ns>.png");
  CHECK_MSG(!listed.empty(), "no <timestamp_ns>.png in " << input);
  std::vector<std::string> names; std::vector<double> times;
  for (size_t i : sth::OrderByTime(listed_t)) { names.push_back(listed[i]); times.push_back(listed_t[i]); }
  const size_t total = names.size();

  // the plan, over the whole clip
  std::vector<double> path_q(4 * total), smooth_q(4 * total), correction_q(4 * total), required(total), zoom(total);
  std::vector<int32_t> iterations(total), plan_status(total);
  std::vector<uint8_t> clamped(total);
  scene.frame_t = times;
  const bool horizon = F.d("horizon_lock") != 0.0;            // off: the plan and its file as without the horizon lock
  sth::LevelArrays levelled(horizon ? total : 0);
  if (horizon) {
    std::vector<double> accl_t, accl;
    rsh::CorrectedAccl(telemetry, acc_intr, &accl_t, &accl);
    oicc_stab_level level;
    level.num_accl = int64_t(accl_t.size()); level.accl_t = accl_t.data(); level.accl = accl.data();
    level.gravity_sigma_s = F.d("gravity_window_s"); level.gravity_const = F.d("gravity_const"); level.accl_gate = F.d("accl_gate");
    level.lock = F.d("horizon_lock"); level.roll_rad = F.d("horizon_roll_deg") * kPi / 180.0;
    const oicc_rs_scene c = scene.c();
    const int rc = oicc_stab_plan_level(device, &c, &opt, &level, path_q.data(), smooth_q.data(), correction_q.data(), required.data(), zoom.data(),
                                        iterations.data(), plan_status.data(), clamped.data(), levelled.level_q.data(), levelled.up.data(),
                                        levelled.roll.data(), levelled.level_angle.data(), levelled.gravity_samples.data(),
                                        levelled.level_status.data(), nullptr);
    CHECK_MSG(rc == OICC_OK, "oicc_stab_plan_level failed (" << rc << ")");
  } else {
    const oicc_rs_scene c = scene.c();
    const int rc = oicc_stab_plan(device, &c, &opt, path_q.data(), smooth_q.data(), correction_q.data(), required.data(), zoom.data(), iterations.data(),
                                  plan_status.data(), clamped.data(), nullptr);
    CHECK_MSG(rc == OICC_OK, "oicc_stab_plan failed (" << rc << ")");
  }
  if (!F.str("output_plan_json").empty()) {
    std::ofstream f(F.str("output_plan_json"), std::ios::binary);
    f << sth::PlanJson(names, plan_status, correction_q, required, zoom, clamped, horizon ? &levelled : nullptr);
    CHECK_MSG(bool(f), "cannot write " << F.str("output_plan_json"));
  }
  mkdir(output.c_str(), 0777);
  CHECK_MSG(is_dir(output), "cannot create " << output);
  size_t k = 0, written = 0;
  Frame next; bool have_next = false;
  while (k < total) {                           // runs of frames with the same colour layout travel as one call
    std::vector<Frame> frames;
    if (have_next) { frames.push_back(next); have_next = false; }
    while (k + frames.size() < total && int(frames.size()) < kBatch) {
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
    const int rc = oicc_stab_frames(device, &c, correction_q.data() + 4 * k, zoom.data() + k, ch, in.data(), 0, kBatch, out.data(), status.data(), nullptr);
    CHECK_MSG(rc == OICC_OK, "oicc_stab_frames failed (" << rc << ")");
    for (int i = 0; i < n; ++i) {
      const std::string& name = names[k + size_t(i)];
      if (status[size_t(i)] != 0) { std::cerr << "skipped " << name << ": " << rsh::FrameStatusText(status[size_t(i)]) << std::endl; continue; }
      CHECK_MSG(oicc_png::write_png(output + "/" + name, w, h, ch, out.data() + frame_bytes * size_t(i), &err), err);
      ++written;
    }
    k += size_t(n);
  }
  if (!F.str("output_camera_json").empty())
    if (!write_camera_calibration(F.str("output_camera_json"), scene.dst_model, "PINHOLE", scene.dst_intr, w, h, fps, 0, 0.0)) return 1;
  std::cout << "stabilised " << written << " of " << total << " frames, smoothing " << opt.smoothing_sigma_s << " s, zoom mode " << F.str("zoom_mode")
            << ", line delay " << scene.calib.line_delay_s * 1e6 << " us, time offset " << scene.calib.time_offset_imu_to_cam_s << " s" << std::endl;
  return 0;
}

int main(int argc, char* argv[]) {
  try {
    return run_main(argc, argv);
  } catch (const std::exception& e) {
    std::cerr << "stabilize_frames: " << e.what() << std::endl;
    return 1;
  }
}
