// undistort_images -- undistorted copies of a folder of PNG frames.
//
//   undistort_images --input_path DIR --camera_calibration_json F --output_path DIR [--balance 0] [--output_camera_json F] [--device 0]
//
// Every <name>.png of the input folder (8-bit gray or RGB, read by png_reader.hpp; an alpha channel is dropped) is resampled
// through the map from the calibrated camera to its rectified pinhole (camera_maps.hpp RectifiedPinhole, oicc_camera_rectify_map,
// oicc_camera_remap) and written under the same name by png_writer.hpp; --output_camera_json receives the pinhole in the format
// of cam_calib.json.  The twin of openimucameracalibrator_amd/undistort_images.py: the PNGs decode to the same arrays.  The
// reference has no such application.
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

using namespace oicc_cli;

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
  Flags F({{"input_path", ""}, {"camera_calibration_json", ""}, {"output_path", ""}, {"balance", "0"}, {"output_camera_json", ""}, {"device", "0"}});
  if (!F.parse(argc, argv)) return 2;
  const std::string input = F.str("input_path"), output = F.str("output_path");
  const int device = std::stoi(F.str("device"));
  CHECK_MSG(!input.empty() && !output.empty() && !F.str("camera_calibration_json").empty(),
            "--input_path, --camera_calibration_json and --output_path are required");
  CalibDataset cam; double fps = 0.0;
  if (!read_camera_calibration(F.str("camera_calibration_json"), &cam, &fps)) return 1;
  CHECK_MSG(OpenICC::camera_maps::ReadPinholeRadialTerms(F.str("camera_calibration_json"), cam.camera_model, &cam.intrinsics),
            "Could not open: " << F.str("camera_calibration_json"));
  CHECK_MSG(is_dir(input), "not a folder: " << input);
  const int w = cam.image_width, h = cam.image_height;
  std::vector<double> dst; std::string err;
  CHECK_MSG(OpenICC::camera_maps::RectifiedPinhole(device, cam.camera_model, cam.intrinsics, w, h, F.d("balance"), &dst, &err), err);
  std::vector<float> map(size_t(w) * size_t(h) * 2); std::vector<uint8_t> valid(size_t(w) * size_t(h));
  int64_t num_valid = 0;
  int rc = oicc_camera_rectify_map(device, cam.camera_model, cam.intrinsics.data(), w, h, OICC_CAM_PINHOLE, dst.data(), w, h, nullptr, map.data(),
                                   valid.data(), &num_valid, nullptr);
  CHECK_MSG(rc == OICC_OK, "oicc_camera_rectify_map failed (" << rc << ")");
  std::vector<std::string> names;
  if (DIR* d = opendir(input.c_str())) {
    while (dirent* e = readdir(d)) {
      const std::string n = e->d_name;
      if (n.size() > 4 && n.compare(n.size() - 4, 4, ".png") == 0) names.push_back(n);
    }
    closedir(d);
  }
  std::sort(names.begin(), names.end());
  mkdir(output.c_str(), 0777);
  CHECK_MSG(is_dir(output), "cannot create " << output);
  size_t k = 0;
  Frame next; bool have_next = false;
  while (k < names.size()) {                    // runs of frames with the same colour layout travel as one batch
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
    rc = oicc_camera_remap(device, n, w, h, ch, in.data(), map.data(), w, h, 0, kBatch, out.data(), nullptr);
    CHECK_MSG(rc == OICC_OK, "oicc_camera_remap failed (" << rc << ")");
    for (int i = 0; i < n; ++i)
      CHECK_MSG(oicc_png::write_png(output + "/" + names[k + size_t(i)], w, h, ch, out.data() + frame_bytes * size_t(i), &err), err);
    k += size_t(n);
  }
  if (!F.str("output_camera_json").empty() &&
      !write_camera_calibration(F.str("output_camera_json"), OICC_CAM_PINHOLE, "PINHOLE", dst, w, h, fps, 0, 0.0)) return 1;
  std::cout << "undistorted " << names.size() << " frames, focal length " << dst[0] << ", valid pixels " << num_valid << " of " << int64_t(w) * h << std::endl;
  return 0;
}

int main(int argc, char* argv[]) {
  try {
    return run_main(argc, argv);
  } catch (const std::exception& e) {
    std::cerr << "undistort_images: " << e.what() << std::endl;
    return 1;
  }
}
