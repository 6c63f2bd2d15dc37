// convert_camera_model -- a calibrated camera re-expressed in another camera model.
//
//   convert_camera_model --camera_calibration_json F --camera_model_to_calibrate NAME --save_path_calib_dataset OUT [--grid_stride 8] [--device 0]
//
// Writes OUT.json with the keys of cam_calib.json for the fitted model plus an object "conversion" (source_intrinsic_type,
// fit_rms_px, full_image_rms_px, full_image_max_px, valid_pixels) and prints the same figures: what the new model costs in pixels
// over the FULL image, so that a bad fit is reported as bad.  The fit goes through the ViewBundleAdjuster facade
// (camera_maps.hpp ConvertCameraModel).  The twin of openimucameracalibrator_amd/convert_camera_model.py.  The reference has no
// such application.
#include <exception>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "ba_cli_common.hpp"
#include "camera_maps.hpp"

using namespace oicc_cli;

static const char* model_name(int model) {
  switch (model) {
    case OICC_CAM_PINHOLE: return "PINHOLE"; case OICC_CAM_PINHOLE_RADIAL_TANGENTIAL: return "PINHOLE_RADIAL_TANGENTIAL";
    case OICC_CAM_FISHEYE: return "FISHEYE"; case OICC_CAM_DIVISION_UNDISTORTION: return "DIVISION_UNDISTORTION";
    case OICC_CAM_DOUBLE_SPHERE: return "DOUBLE_SPHERE"; default: return "EXTENDED_UNIFIED";
  }
}

static int run_main(int argc, char* argv[]) {
  Flags F({{"camera_calibration_json", ""}, {"camera_model_to_calibrate", ""}, {"save_path_calib_dataset", ""}, {"grid_stride", "8"}, {"device", "0"}});
  if (!F.parse(argc, argv)) return 2;
  CHECK_MSG(!F.str("camera_calibration_json").empty() && !F.str("save_path_calib_dataset").empty(),
            "--camera_calibration_json and --save_path_calib_dataset are required");
  const int device = std::stoi(F.str("device")), stride = std::stoi(F.str("grid_stride"));
  const int dst_model = model_from_string(F.str("camera_model_to_calibrate"));
  CHECK_MSG(dst_model >= 0 && stride >= 1, "unknown camera model " << F.str("camera_model_to_calibrate") << " or a stride < 1");
  CalibDataset cam; double fps = 0.0;
  if (!read_camera_calibration(F.str("camera_calibration_json"), &cam, &fps)) return 1;
  Value src;
  CHECK_MSG(oicc_json::parse_file(F.str("camera_calibration_json"), &src), "Could not open: " << F.str("camera_calibration_json"));
  CHECK_MSG(OpenICC::camera_maps::ReadPinholeRadialTerms(F.str("camera_calibration_json"), cam.camera_model, &cam.intrinsics),
            "Could not open: " << F.str("camera_calibration_json"));
  OpenICC::camera_maps::Conversion res; std::string err;
  CHECK_MSG(OpenICC::camera_maps::ConvertCameraModel(device, cam.camera_model, cam.intrinsics, cam.image_width, cam.image_height, dst_model, stride,
                                                    &res, &err), err);
  Value conv;
  conv["source_intrinsic_type"] = Value(std::string(model_name(cam.camera_model)));
  conv["fit_rms_px"] = Value(res.fit_rms_px); conv["full_image_rms_px"] = Value(res.full_image_rms_px);
  conv["full_image_max_px"] = Value(res.full_image_max_px); conv["valid_pixels"] = Value(int64_t(res.valid_pixels));
  const std::string path = F.str("save_path_calib_dataset") + ".json";
  const int nr = src.contains("nr_calib_images") ? int(src.at("nr_calib_images").as_double()) : 0;
  const double reproj = src.contains("final_reproj_error") ? src.at("final_reproj_error").as_double() : 0.0;
  if (!write_camera_calibration(path, dst_model, model_name(dst_model), res.intrinsics, cam.image_width, cam.image_height, fps, nr, reproj)) return 1;
  Value obj;
  CHECK_MSG(oicc_json::parse_file(path, &obj), "Could not open: " << path);
  obj["conversion"] = conv;
  std::ofstream f(path);
  CHECK_MSG(f.is_open(), "Could not open: " << path);
  oicc_json::dump(obj, f, 2); f << std::endl;
  char line[512];
  std::snprintf(line, sizeof(line), "%s -> %s: fit_rms_px %.6g full_image_rms_px %.6g full_image_max_px %.6g valid_pixels %lld",
                model_name(cam.camera_model), model_name(dst_model), res.fit_rms_px, res.full_image_rms_px, res.full_image_max_px,
                (long long)res.valid_pixels);
  std::cout << line << std::endl;
  return f.good() ? 0 : 1;
}

int main(int argc, char* argv[]) {
  try {
    return run_main(argc, argv);
  } catch (const std::exception& e) {
    std::cerr << "convert_camera_model: " << e.what() << std::endl;
    return 1;
  }
}
