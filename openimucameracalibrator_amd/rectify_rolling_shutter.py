"""python -m openimucameracalibrator_amd.rectify_rolling_shutter: global-shutter-equivalent copies of a folder of rolling-shutter
PNG frames, from the gyroscope.

  --input_path DIR --telemetry_json F --camera_calibration_json F --imu_camera_calibration_json F --output_path DIR
  [--line_delay_us X] [--time_offset_imu_to_cam_s X] [--imu_intrinsics F] [--imu_bias_file F] [--reference_row Y]
  [--undistort] [--balance 0] [--output_camera_json F] [--device 0]

Every <timestamp_ns>.png of the input folder (8-bit gray or RGB, the size of the calibration) is exposed row by row: row y at
t = timestamp_ns 1e-9 + img_timestamps_ns[0] 1e-9 + y line_delay.  --imu_camera_calibration_json is the result.json of the spline
calibration (q_i_c, time_offset_imu_to_cam_s, calib_line_delay_us); the two override flags replace its values.  The gyroscope rates
are corrected with --imu_intrinsics / --imu_bias_file and integrated; rolling_shutter.rs_rectify_frames resamples every frame into
the camera at its reference row's time (rotation only).  --undistort makes the destination the rectified pinhole (--balance)
instead of the camera itself; --output_camera_json receives the destination camera.  Frames without gyro coverage are not written:
they are listed on stderr with the reason.  The twin of csrc/host/rectify_rolling_shutter.cpp: the PNGs decode to the same arrays.
No reference counterpart."""
import argparse
import json
import os
import sys

import numpy as np

from . import camera_maps
from . import io_files
from . import rolling_shutter as rs
from . import synthetic as S
from .undistort_images import read_frame

BATCH = 16


def read_imu_camera_result(path):
    """(q_i_c (w, x, y, z), time_offset_imu_to_cam_s, line_delay_s) of the spline calibration's result.json."""
    obj = json.load(open(path))
    for key in ("q_i_c", "time_offset_imu_to_cam_s", "calib_line_delay_us"):
        if key not in obj:
            raise ValueError("%s has no %s" % (path, key))
    q = np.array([float(obj["q_i_c"][k]) for k in "wxyz"])
    return q, float(obj["time_offset_imu_to_cam_s"]), float(obj["calib_line_delay_us"]) * 1e-6


def read_gyro_intrinsics(path_intr, path_bias):
    """(gyro intrinsics [9]: six misalignments and three scales, gyro bias [3]) of the IMU intrinsics and bias files the spline
    calibration reads (misalignment matrix [[1, -yz, zy], [xz, 1, -zx], [-xy, yx, 1]]); identity and zero without a file."""
    intr = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0]); bias = np.zeros(3)
    if path_bias:
        try:
            b = json.load(open(path_bias))["gyro_bias"]
            bias = np.array([float(b[k]) for k in "xyz"])
        except (OSError, ValueError):
            print("Error loading IMU bias file: %s" % path_bias, file=sys.stderr)
    if path_intr:
        g = json.load(open(path_intr))["gyroscope"]
        M, Sc = g["misalignment_matrix"], g["scale_matrix"]
        intr = np.array([-M[0][1], M[0][2], -M[1][2], M[1][0], -M[2][0], M[2][1], Sc[0][0], Sc[1][1], Sc[2][2]], dtype=np.float64)
    return intr, bias


def read_accl_intrinsics(path_intr, path_bias):
    """(accelerometer intrinsics [6]: the three misalignments of the upper triangle and three scales, accl bias [3]) of the same two
    files; identity and zero without a file."""
    intr = np.array([0.0, 0.0, 0.0, 1.0, 1.0, 1.0]); bias = np.zeros(3)
    if path_bias:
        try:
            b = json.load(open(path_bias))["accl_bias"]
            bias = np.array([float(b[k]) for k in "xyz"])
        except (OSError, ValueError):
            print("Error loading IMU bias file: %s" % path_bias, file=sys.stderr)
    if path_intr:
        a = json.load(open(path_intr))["accelerometer"]
        M, Sc = a["misalignment_matrix"], a["scale_matrix"]
        intr = np.array([-M[0][1], M[0][2], -M[1][2], Sc[0][0], Sc[1][1], Sc[2][2]], dtype=np.float64)
    return intr, bias


def frame_time_from_name(name, t_offset_cam_s):
    """<timestamp_ns>.png -> timestamp_ns 1e-9 + t_offset_cam_s, the rule the calibration program applies to view keys; None for
    another name."""
    digits = name[:-4]
    if not name.endswith(".png") or not digits or len(digits) > 19 or any(c not in "0123456789" for c in digits):
        return None
    return float(int(digits)) * 1e-9 + t_offset_cam_s


def main(argv=None):
    from PIL import Image
    ap = argparse.ArgumentParser(prog="rectify_rolling_shutter")
    ap.add_argument("--input_path", required=True)
    ap.add_argument("--telemetry_json", required=True)
    ap.add_argument("--camera_calibration_json", required=True)
    ap.add_argument("--imu_camera_calibration_json", required=True)
    ap.add_argument("--output_path", required=True)
    ap.add_argument("--line_delay_us", type=float, default=None)
    ap.add_argument("--time_offset_imu_to_cam_s", type=float, default=None)
    ap.add_argument("--imu_intrinsics", default="")
    ap.add_argument("--imu_bias_file", default="")
    ap.add_argument("--reference_row", type=float, default=None)
    ap.add_argument("--undistort", action="store_true")
    ap.add_argument("--balance", type=float, default=0.0)
    ap.add_argument("--output_camera_json", default="")
    ap.add_argument("--device", type=int, default=0)
    args = io_files.parse_reference_flags(ap, argv)
    for path in (args.camera_calibration_json, args.imu_camera_calibration_json, args.telemetry_json) + ((args.imu_intrinsics,) if args.imu_intrinsics else ()):
        if not os.path.isfile(path):
            print("Could not open: %s" % path, file=sys.stderr)
            return 1
    if not os.path.isdir(args.input_path):
        print("not a folder: %s" % args.input_path, file=sys.stderr)
        return 1
    model, intr, w, h, fps = io_files.read_camera_calibration(args.camera_calibration_json)
    q_i_c, time_offset, line_delay = read_imu_camera_result(args.imu_camera_calibration_json)
    if args.line_delay_us is not None:
        line_delay = args.line_delay_us * 1e-6
    if args.time_offset_imu_to_cam_s is not None:
        time_offset = args.time_offset_imu_to_cam_s
    telemetry = json.load(open(args.telemetry_json))
    img_ts = telemetry.get("img_timestamps_ns", [])
    t_offset_cam_s = float(img_ts[0]) * 1e-9 if len(img_ts) else 0.0
    gyro_t, rates = rs.corrected_gyro(telemetry, *read_gyro_intrinsics(args.imu_intrinsics, args.imu_bias_file))
    dst = (model, intr, w, h)
    if args.undistort:
        dst = (S.CAM_PINHOLE, camera_maps.rectified_pinhole(model, intr, w, h, args.balance, device=args.device), w, h)
    reference_row = (h - 1) / 2.0 if args.reference_row is None else args.reference_row
    names = sorted(n for n in os.listdir(args.input_path) if len(n) > 4 and n.endswith(".png"))
    times = [frame_time_from_name(n, t_offset_cam_s) for n in names]
    for n, t in zip(names, times):
        if t is None:
            print("%s: the name is not <timestamp_ns>.png" % n, file=sys.stderr)
            return 1
    os.makedirs(args.output_path, exist_ok=True)
    k = written = 0
    while k < len(names):                      # runs of frames with the same colour layout travel as one call
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
        scene = rs.Scene((model, intr, w, h), dst, gyro_t, rates, times[k:k + len(frames)], line_delay, q_i_c=q_i_c,
                         time_offset_imu_to_cam=time_offset, reference_row=reference_row)
        out, status = rs.rs_rectify_frames(np.stack(frames), scene, batch=BATCH, device=args.device)
        for o, st, n in zip(out, status, names[k:]):
            if st != 0:
                print("skipped %s: %s" % (n, rs.FRAME_STATUS[int(st)]), file=sys.stderr)
                continue
            Image.fromarray(o).save(os.path.join(args.output_path, n))
            written += 1
        k += len(frames)
    if args.output_camera_json:
        io_files.write_camera_calibration(args.output_camera_json, dst[0], dst[1], w, h, fps, 0, 0.0)
    print("rectified %d of %d frames, line delay %g us, time offset %g s, reference row %g" % (written, len(names), line_delay * 1e6, time_offset,
                                                                                                 reference_row))
    return 0


if __name__ == "__main__":
    sys.exit(main())
