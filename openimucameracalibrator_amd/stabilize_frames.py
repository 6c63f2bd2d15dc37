"""python -m openimucameracalibrator_amd.stabilize_frames: stabilised, global-shutter-equivalent copies of a folder of
rolling-shutter PNG frames, from the gyroscope.

  --input_path DIR --telemetry_json F --camera_calibration_json F --imu_camera_calibration_json F --output_path DIR
  [--line_delay_us X] [--time_offset_imu_to_cam_s X] [--imu_intrinsics F] [--imu_bias_file F] [--reference_row Y]
  [--undistort] [--balance 0] [--output_camera_json F] [--device 0]
  [--smoothing_s 0.5] [--max_correction_deg 0] [--zoom_mode none|fixed|dynamic] [--zoom_window_s 1] [--max_zoom 4]
  [--output_plan_json F]
  [--horizon_lock 0] [--horizon_roll_deg 0] [--gravity_window_s 1] [--gravity_const 9.811104] [--accl_gate 0]

The flags and files of rectify_rolling_shutter.  The destination is always the rectified pinhole of --balance (--undistort is
accepted and changes nothing).  stabilization.stab_plan sees the times of every <timestamp_ns>.png of the folder, in the order of
their times: the orientation path, the smooth camera (--smoothing_s: sigma of the Gaussian window; --max_correction_deg: 0 = no
bound) and the zoom.  Then the frames are read in chunks and stabilization.stab_frames warps each chunk with its part of the plan
(rotation only).  --output_plan_json receives, per frame, name, status, correction quaternion, required and applied zoom.
--horizon_lock X in (0, 1] turns the horizon lock on: the accelerometer of the telemetry, corrected by the accelerometer part of
--imu_intrinsics and --imu_bias_file, gives gravity over a Gaussian window of sigma --gravity_window_s, and the part X of the
smooth camera's roll against --horizon_roll_deg is taken out (--accl_gate G: samples whose norm is further than G from
--gravity_const are left out; 0 = no gate); the plan file then also holds level_q, up, roll, level_angle, gravity_samples and
level_status per frame.  With --horizon_lock 0 the PNGs and the plan file are what they are without these flags.  Frames
without gyro coverage are not written: they are listed on stderr with the reason.  The twin of csrc/host/stabilize_frames.cpp: the
same PNGs, the same plan file.  No reference counterpart."""
import argparse
import json
import math
import os
import sys

import numpy as np

from . import camera_maps
from . import io_files
from . import rolling_shutter as rs
from . import stabilization as stab
from . import synthetic as S
from .rectify_rolling_shutter import frame_time_from_name, read_accl_intrinsics, read_gyro_intrinsics, read_imu_camera_result
from .undistort_images import read_frame

BATCH = 16


def order_by_time(times):
    """Indices of the frames by time, equal times in the order given: file names sort as text, their times need not."""
    return sorted(range(len(times)), key=lambda i: times[i])


def json_number(v):
    """A double as 17 significant digits, null where it is not finite."""
    return "%.17g" % v if math.isfinite(v) else "null"


def plan_json(names, status, correction_q, required_zoom, zoom, zoom_clamped, level=None):
    """The plan file's text, one line per frame; byte for byte what csrc/host/stabilization.hpp writes.  level: the plan itself or a
    dict with level_q, up, roll, level_angle, gravity_samples and level_status (the horizon lock is on), or None."""
    get = (lambda key: level[key]) if isinstance(level, dict) else (lambda key: getattr(level, key))
    s = "{\"frames\": ["
    for k, name in enumerate(names):
        s += ",\n" if k else "\n"
        s += " {\"name\": \"%s\", \"status\": %d, \"correction_q\": [%s], \"required_zoom\": %s, \"zoom\": %s, \"zoom_clamped\": %d" % (
            name, int(status[k]), ", ".join(json_number(float(c)) for c in correction_q[k]), json_number(float(required_zoom[k])),
            json_number(float(zoom[k])), int(zoom_clamped[k]))
        if level is not None:
            s += ", \"level_q\": [%s], \"up\": [%s], \"roll\": %s, \"level_angle\": %s, \"gravity_samples\": %d, \"level_status\": %d" % (
                ", ".join(json_number(float(c)) for c in get("level_q")[k]), ", ".join(json_number(float(c)) for c in get("up")[k]),
                json_number(float(get("roll")[k])), json_number(float(get("level_angle")[k])), int(get("gravity_samples")[k]), int(get("level_status")[k]))
        s += "}"
    return s + "\n]}\n"


def main(argv=None):
    from PIL import Image
    ap = argparse.ArgumentParser(prog="stabilize_frames")
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
    ap.add_argument("--smoothing_s", type=float, default=0.5)
    ap.add_argument("--max_correction_deg", type=float, default=0.0)
    ap.add_argument("--zoom_mode", default="fixed")
    ap.add_argument("--zoom_window_s", type=float, default=1.0)
    ap.add_argument("--max_zoom", type=float, default=4.0)
    ap.add_argument("--output_plan_json", default="")
    ap.add_argument("--horizon_lock", type=float, default=0.0)
    ap.add_argument("--horizon_roll_deg", type=float, default=0.0)
    ap.add_argument("--gravity_window_s", type=float, default=1.0)
    ap.add_argument("--gravity_const", type=float, default=9.811104)
    ap.add_argument("--accl_gate", type=float, default=0.0)
    args = io_files.parse_reference_flags(ap, argv)
    if args.zoom_mode not in stab.ZOOM_MODES:
        print("--zoom_mode is none, fixed or dynamic", file=sys.stderr)
        return 1
    for path in (args.camera_calibration_json, args.imu_camera_calibration_json, args.telemetry_json) + ((args.imu_intrinsics,) if args.imu_intrinsics else ()):
        if not os.path.isfile(path):
            print("Could not open: %s" % path, file=sys.stderr)
            return 1
    if not os.path.isdir(args.input_path):
        print("not a folder: %s" % args.input_path, file=sys.stderr)
        return 1
    options = stab.StabOptions(args.smoothing_s, args.max_correction_deg * math.pi / 180.0, args.zoom_mode, args.zoom_window_s, args.max_zoom)
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
    dst = (S.CAM_PINHOLE, camera_maps.rectified_pinhole(model, intr, w, h, args.balance, device=args.device), w, h)
    reference_row = (h - 1) / 2.0 if args.reference_row is None else args.reference_row
    listed = sorted(n for n in os.listdir(args.input_path) if len(n) > 4 and n.endswith(".png"))
    listed_t = [frame_time_from_name(n, t_offset_cam_s) for n in listed]
    for n, t in zip(listed, listed_t):
        if t is None:
            print("%s: the name is not <timestamp_ns>.png" % n, file=sys.stderr)
            return 1
    if not listed:
        print("no <timestamp_ns>.png in %s" % args.input_path, file=sys.stderr)
        return 1
    order = order_by_time(listed_t)
    names, times = [listed[i] for i in order], [listed_t[i] for i in order]

    def scene_of(t):
        return rs.Scene((model, intr, w, h), dst, gyro_t, rates, t, line_delay, q_i_c=q_i_c, time_offset_imu_to_cam=time_offset, reference_row=reference_row)

    level = None
    if args.horizon_lock != 0.0:               # off: the plan and its file as without the horizon lock
        accl_t, accl = rs.corrected_accl(telemetry, *read_accl_intrinsics(args.imu_intrinsics, args.imu_bias_file))
        level = stab.LevelOptions(accl_t, accl, args.gravity_window_s, args.gravity_const, args.accl_gate, args.horizon_lock,
                                  args.horizon_roll_deg * math.pi / 180.0)
    plan = stab.stab_plan(scene_of(times), options, device=args.device, level=level)          # over the whole clip
    if args.output_plan_json:
        with open(args.output_plan_json, "w", newline="") as f:
            f.write(plan_json(names, plan.frame_status, plan.correction_q, plan.required_zoom, plan.zoom, plan.zoom_clamped,
                              None if level is None else plan))
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
        m = len(frames)
        out, status = stab.stab_frames(np.stack(frames), scene_of(times[k:k + m]), plan.correction_q[k:k + m], plan.zoom[k:k + m], batch=BATCH,
                                       device=args.device)
        for o, st, n in zip(out, status, names[k:]):
            if st != 0:
                print("skipped %s: %s" % (n, rs.FRAME_STATUS[int(st)]), file=sys.stderr)
                continue
            Image.fromarray(o).save(os.path.join(args.output_path, n))
            written += 1
        k += m
    if args.output_camera_json:
        io_files.write_camera_calibration(args.output_camera_json, dst[0], dst[1], w, h, fps, 0, 0.0)
    print("stabilised %d of %d frames, smoothing %g s, zoom mode %s, line delay %g us, time offset %g s" % (written, len(names), args.smoothing_s,
                                                                                                          args.zoom_mode, line_delay * 1e6, time_offset))
    return 0


if __name__ == "__main__":
    sys.exit(main())
