"""python -m openimucameracalibrator_amd.undistort_images: undistorted copies of a folder of PNG frames.

  --input_path DIR --camera_calibration_json F --output_path DIR [--balance 0] [--output_camera_json F] [--device 0]

Every <name>.png of the input folder (8-bit gray or RGB, the size of the calibration) is resampled through the map from the
calibrated camera to its rectified pinhole (camera_maps.rectified_pinhole) and written under the same name; the pinhole goes to
--output_camera_json in the format of cam_calib.json.  The twin of csrc/host/undistort_images.cpp: the PNGs decode to the same
arrays.  No reference counterpart."""
import argparse
import os
import sys

import numpy as np

from . import camera_maps
from . import io_files
from . import synthetic as S

BATCH = 16


def read_frame(path):
    """8-bit gray (also gray + alpha) -> [h, w]; anything else -> RGB [h, w, 3] (alpha dropped)."""
    from PIL import Image
    img = Image.open(path)
    return np.asarray(img.convert("L" if img.mode in ("L", "LA") else "RGB"))


def main(argv=None):
    from PIL import Image
    ap = argparse.ArgumentParser(prog="undistort_images")
    ap.add_argument("--input_path", required=True)
    ap.add_argument("--camera_calibration_json", required=True)
    ap.add_argument("--output_path", required=True)
    ap.add_argument("--balance", type=float, default=0.0)
    ap.add_argument("--output_camera_json", default="")
    ap.add_argument("--device", type=int, default=0)
    args = io_files.parse_reference_flags(ap, argv)
    if not os.path.isfile(args.camera_calibration_json):
        print("Could not open: %s" % args.camera_calibration_json, file=sys.stderr)
        return 1
    if not os.path.isdir(args.input_path):
        print("not a folder: %s" % args.input_path, file=sys.stderr)
        return 1
    model, intr, w, h, fps = io_files.read_camera_calibration(args.camera_calibration_json)
    dst_intr = camera_maps.rectified_pinhole(model, intr, w, h, args.balance, device=args.device)
    mapxy, valid, num_valid = camera_maps.rectify_map(model, intr, w, h, S.CAM_PINHOLE, dst_intr, w, h, device=args.device)
    os.makedirs(args.output_path, exist_ok=True)
    names = sorted(n for n in os.listdir(args.input_path) if len(n) > 4 and n.endswith(".png"))
    k = 0
    while k < len(names):                      # runs of frames with the same colour layout travel as one batch
        frames = [read_frame(os.path.join(args.input_path, names[k]))]
        while k + len(frames) < len(names) and len(frames) < BATCH:
            f = read_frame(os.path.join(args.input_path, names[k + len(frames)]))
            if f.ndim != frames[0].ndim:
                break
            frames.append(f)
        for f, n in zip(frames, names[k:]):
            if f.shape[:2] != (h, w):
                print("%s: %d x %d, the calibration is for %d x %d" % (n, f.shape[1], f.shape[0], w, h), file=sys.stderr)
                return 1
        out = camera_maps.remap(np.stack(frames), mapxy, batch=BATCH, device=args.device)
        for o, n in zip(out, names[k:]):
            Image.fromarray(o).save(os.path.join(args.output_path, n))
        k += len(frames)
    if args.output_camera_json:
        io_files.write_camera_calibration(args.output_camera_json, S.CAM_PINHOLE, dst_intr, w, h, fps, 0, 0.0)
    print("undistorted %d frames, focal length %.6f, valid pixels %d of %d" % (len(names), dst_intr[0], num_valid, w * h))
    return 0


if __name__ == "__main__":
    sys.exit(main())
