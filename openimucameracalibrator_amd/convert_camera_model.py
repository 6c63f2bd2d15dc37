"""python -m openimucameracalibrator_amd.convert_camera_model: a calibrated camera re-expressed in another camera model.

  --camera_calibration_json F --camera_model_to_calibrate NAME --save_path_calib_dataset OUT [--grid_stride 8] [--device 0]

Writes OUT.json with the keys of cam_calib.json for the fitted model plus an object `conversion` (source_intrinsic_type,
fit_rms_px, full_image_rms_px, full_image_max_px, valid_pixels) and prints the same figures: what the new model costs in pixels
over the FULL image, so that a bad fit is reported as bad.  camera_maps.convert_camera_model does the work; the twin of
csrc/host/convert_camera_model.cpp.  No reference counterpart."""
import argparse
import json
import os
import sys

from . import camera_calibrator as cc
from . import camera_maps
from . import io_files


def main(argv=None):
    ap = argparse.ArgumentParser(prog="convert_camera_model")
    ap.add_argument("--camera_calibration_json", required=True)
    ap.add_argument("--camera_model_to_calibrate", required=True)
    ap.add_argument("--save_path_calib_dataset", required=True)
    ap.add_argument("--grid_stride", type=int, default=8)
    ap.add_argument("--device", type=int, default=0)
    args = io_files.parse_reference_flags(ap, argv)
    if not os.path.isfile(args.camera_calibration_json):
        print("Could not open: %s" % args.camera_calibration_json, file=sys.stderr)
        return 1
    if args.camera_model_to_calibrate not in cc.MODEL_IDS or args.grid_stride < 1:
        print("unknown camera model %s or a stride < 1" % args.camera_model_to_calibrate, file=sys.stderr)
        return 1
    with open(args.camera_calibration_json) as f:
        src = json.load(f)
    model, intr, w, h, fps = io_files.read_camera_calibration(args.camera_calibration_json)
    dst_model = cc.MODEL_IDS[args.camera_model_to_calibrate]
    res = camera_maps.convert_camera_model(model, intr, w, h, dst_model, stride=args.grid_stride, device=args.device)
    path = args.save_path_calib_dataset + ".json"
    io_files.write_camera_calibration(path, dst_model, res["intrinsics"], w, h, fps, int(src.get("nr_calib_images", 0)),
                                      float(src.get("final_reproj_error", 0.0)))
    with open(path) as f:
        obj = json.load(f)
    obj["conversion"] = dict(source_intrinsic_type=io_files.MODEL_NAMES[model], fit_rms_px=res["fit_rms_px"],
                             full_image_rms_px=res["full_image_rms_px"], full_image_max_px=res["full_image_max_px"],
                             valid_pixels=res["valid_pixels"])
    with open(path, "w") as f:
        json.dump(obj, f, indent=2)
    print("%s -> %s: fit_rms_px %.6g full_image_rms_px %.6g full_image_max_px %.6g valid_pixels %d" % (
        io_files.MODEL_NAMES[model], args.camera_model_to_calibrate, res["fit_rms_px"], res["full_image_rms_px"], res["full_image_max_px"],
        res["valid_pixels"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
