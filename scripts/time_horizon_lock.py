#!/usr/bin/env python
"""Timings of the horizon lock on the GPU ("Horizon lock"): a clip of 1800 frames of 960 x 540 at 30 fps, gopro9_division
onto its rectified pinhole, a 200 Hz gyroscope with N(0, sigma) rad/s per axis and a 200 Hz accelerometer that reads a rolled up
vector with noise; smoothing sigma 0.5 s, dynamic zoom with T = 1 s, gravity sigma 1.0 s.

  python scripts/time_horizon_lock.py [--frames 1800] [--runs 3] [--repeats 5] [--rate_sigma 1.0] [--gravity_window_s 1.0]
                                      [--compare_lib OTHER/liboicc_hip.so] [--out FILE]

HIP events inside the library, warm: device_ms [5] of oicc_stab_plan_level (path, smoothing, zoom, accelerometer and level kernels)
and device_ms [3] of oicc_stab_plan without a level, alternating inside every repeat.  --compare_lib times oicc_stab_plan of another
build of the library (the parent commit's) in the same process and the same alternation.  Fails without a GPU."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openimucameracalibrator_amd import _abi                           # noqa: E402
from openimucameracalibrator_amd import camera_maps as cm              # noqa: E402
from openimucameracalibrator_amd import rolling_shutter as rs          # noqa: E402
from openimucameracalibrator_amd import stabilization as stab          # noqa: E402
from openimucameracalibrator_amd import synthetic as S                 # noqa: E402


def spread(v):
    return dict(min=float(np.min(v)), mean=float(np.mean(v)), max=float(np.max(v)))


def plain_plan_of(path):
    """oicc_stab_plan of another build of the library: scene, options -> StabPlan."""
    fn = C.CDLL(path).oicc_stab_plan
    fn.restype, fn.argtypes = _abi.STABILIZATION_SIGNATURES["plan"]

    def call(scene, options):
        o = options.c()
        p = stab.StabPlan(scene.num_frames)
        dp, i32 = (lambda a: a.ctypes.data_as(_abi.c_dp)), (lambda a: a.ctypes.data_as(_abi.c_i32p))
        rc = fn(0, scene.ref(), C.byref(o), dp(p.path_q), dp(p.smooth_q), dp(p.correction_q), dp(p.required_zoom), dp(p.zoom), i32(p.iterations),
                i32(p.frame_status), p.zoom_clamped.ctypes.data_as(_abi.c_u8p), dp(p.device_ms))
        if rc != 0:
            raise RuntimeError("oicc_stab_plan of %s failed with %d" % (path, rc))
        return p
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1800)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rate_sigma", type=float, default=1.0)
    ap.add_argument("--gravity_window_s", type=float, default=1.0)
    ap.add_argument("--compare_lib", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    model, intr, w, h = S.CAMERAS["gopro9_division"]
    rng = np.random.RandomState(1)
    dst = cm.rectified_pinhole(model, intr, w, h)
    frame_t = 100.0 + 0.05 + np.arange(args.frames) / 30.0
    n = int((frame_t[-1] - 100.0 + 0.1) * 200.0)
    gyro_t = 100.0 + np.arange(n) / 200.0 + rng.uniform(-2e-4, 2e-4, n)
    rates = rng.normal(0.0, args.rate_sigma, (n, 3))
    accl_t = 100.0 + np.arange(n) / 200.0 + rng.uniform(-2e-4, 2e-4, n)
    accl = np.array([np.sin(0.1), -np.cos(0.1), 0.05]) * 9.811104 + rng.normal(0.0, 0.5, (n, 3))
    options = stab.StabOptions(smoothing_sigma_s=0.5, zoom_mode="dynamic", zoom_window_s=1.0, max_zoom=100.0)
    level = stab.LevelOptions(accl_t, accl, gravity_sigma_s=args.gravity_window_s)
    scene = rs.Scene((model, intr, w, h), (S.CAM_PINHOLE, dst, w, h), gyro_t, rates, frame_t, 30e-6)
    other = plain_plan_of(args.compare_lib) if args.compare_lib else None
    p = stab.stab_plan(scene, options, level=level)                       # warm
    plain = stab.stab_plan(scene, options)
    assert np.all(p.frame_status == 0)
    result = dict(frames=args.frames, width=w, height=h, gyro_samples=n, accl_samples=n, runs=args.runs, repeats=args.repeats, rate_sigma=args.rate_sigma,
                  gravity_window_s=args.gravity_window_s, level_status_counts=[int((p.level_status == s).sum()) for s in (0, 1, 2)],
                  gravity_samples=spread(p.gravity_samples), level_angle_deg=spread(np.degrees(p.level_angle)),
                  zoom=spread(p.zoom), zoom_without_level=spread(plain.zoom))
    if other:
        q = other(scene, options)                                         # warm
        result["other_equals_plain"] = bool(all(np.array_equal(getattr(q, k), getattr(plain, k), equal_nan=True)
                                                for k in ("path_q", "smooth_q", "correction_q", "required_zoom", "zoom")))
    with_level, without, parent = [], [], []
    for _ in range(args.runs):
        acc = [np.zeros(5), np.zeros(3), np.zeros(3)]
        for _ in range(args.repeats):
            acc[0] += stab.stab_plan(scene, options, level=level).device_ms
            acc[1] += stab.stab_plan(scene, options).device_ms
            if other:
                acc[2] += other(scene, options).device_ms
        with_level.append(acc[0] / args.repeats); without.append(acc[1] / args.repeats); parent.append(acc[2] / args.repeats)
    with_level, without, parent = np.array(with_level), np.array(without), np.array(parent)
    names = ("path_kernels_ms", "smooth_kernel_ms", "zoom_kernels_ms", "accl_world_kernel_ms", "level_kernel_ms")
    result["with_level"] = {k: spread(with_level[:, i]) for i, k in enumerate(names)}
    result["without_level"] = {k: spread(without[:, i]) for i, k in enumerate(names[:3])}
    result["without_level"]["sum_ms"] = spread(without.sum(1))
    if other:
        result["other_library"] = {k: spread(parent[:, i]) for i, k in enumerate(names[:3])}
        result["other_library"]["sum_ms"] = spread(parent.sum(1))
        result["plan_without_level_over_other"] = float(without.sum(1).mean() / parent.sum(1).mean())
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
