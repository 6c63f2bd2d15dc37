#!/usr/bin/env python
"""Timings of the stabilisation on the GPU ("Stabilisation"): the scene of time_rolling_shutter.py, 64 frames of
960 x 540 at 30 fps, RGB and gray, gopro9_division onto its rectified pinhole, a 200 Hz gyroscope with N(0, sigma) rad/s per axis.

  python scripts/time_stabilization.py [--frames 64] [--runs 3] [--repeats 20] [--batch 16] [--rate_sigma 1.0 4.0]
                                       [--smoothing_s 0.5] [--out FILE]

HIP events inside the library: path, smoothing and zoom kernels of oicc_stab_plan, the record and map kernels of oicc_stab_map,
the fused kernel of oicc_stab_frames (summed over its batches) and next to it the fused kernel of oicc_rs_rectify_frames on the
same frames; warm; `runs` runs of `repeats` calls, the routes alternating inside every repeat.  Fails without a GPU: there is no
CPU path to time."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openimucameracalibrator_amd import camera_maps as cm              # noqa: E402
from openimucameracalibrator_amd import rolling_shutter as rs          # noqa: E402
from openimucameracalibrator_amd import stabilization as stab          # noqa: E402
from openimucameracalibrator_amd import synthetic as S                 # noqa: E402


def spread(v):
    return dict(min=float(np.min(v)), mean=float(np.mean(v)), max=float(np.max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rate_sigma", type=float, nargs="+", default=[1.0, 4.0])
    ap.add_argument("--smoothing_s", type=float, default=0.5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    model, intr, w, h = S.CAMERAS["gopro9_division"]
    rng = np.random.RandomState(1)
    frames = {3: rng.randint(0, 256, (args.frames, h, w, 3)).astype(np.uint8), 1: rng.randint(0, 256, (args.frames, h, w)).astype(np.uint8)}
    dst = cm.rectified_pinhole(model, intr, w, h)
    frame_t = 100.0 + 0.05 + np.arange(args.frames) / 30.0
    n_gyro = int((frame_t[-1] - 100.0 + 0.1) * 200.0)
    gyro_t = 100.0 + np.arange(n_gyro) / 200.0 + rng.uniform(-2e-4, 2e-4, n_gyro)
    unit = rng.normal(0.0, 1.0, (n_gyro, 3))
    options = stab.StabOptions(smoothing_sigma_s=args.smoothing_s, zoom_mode="dynamic", zoom_window_s=1.0, max_zoom=100.0)
    result = dict(frames=args.frames, width=w, height=h, batch=args.batch, runs=args.runs, repeats=args.repeats, line_delay_us=30.0,
                  smoothing_s=args.smoothing_s, by_rate_sigma={})
    for sigma in args.rate_sigma:
        scene = rs.Scene((model, intr, w, h), (S.CAM_PINHOLE, dst, w, h), gyro_t, unit * sigma, frame_t, 30e-6)
        plan = stab.stab_plan(scene, options)                                                      # warm
        assert np.all(plan.frame_status == 0)
        mapxy, valid, status, num_valid, evals, ms = stab.stab_map(scene, plan.correction_q, plan.zoom, return_evaluations=True, return_ms=True)
        out = dict(valid_fraction=float(valid.mean()), evaluations_mean=float(evals[valid == 1].mean()), evaluations_max=int(evals.max()),
                   correction_deg_max=float(np.degrees(2 * np.arccos(np.clip(plan.correction_q[:, 0], -1, 1))).max()),
                   required_zoom=spread(plan.required_zoom), zoom=spread(plan.zoom), mean_iterations_max=int(plan.iterations.max()),
                   zoom_clamped=int(plan.zoom_clamped.sum()))
        del mapxy, evals
        for c in (3, 1):
            stab.stab_frames(frames[c], scene, plan.correction_q, plan.zoom, batch=args.batch)
            rs.rs_rectify_frames(frames[c], scene, batch=args.batch)
        plan_ms, mapk = [], []
        fused = {3: [], 1: []}; rolled = {3: [], 1: []}
        for _ in range(args.runs):
            acc_p = np.zeros(3); acc_m = np.zeros(3); acc_f = {3: 0.0, 1: 0.0}; acc_r = {3: 0.0, 1: 0.0}
            for _ in range(args.repeats):
                for c in (3, 1):                                           # the routes alternate inside a repeat
                    rep = {}
                    stab.stab_frames(frames[c], scene, plan.correction_q, plan.zoom, batch=args.batch, report=rep)
                    acc_f[c] += rep["ms_kernel"]
                    rep = {}
                    rs.rs_rectify_frames(frames[c], scene, batch=args.batch, report=rep)
                    acc_r[c] += rep["ms_kernel"]
                acc_p += stab.stab_plan(scene, options).device_ms
                acc_m += stab.stab_map(scene, plan.correction_q, plan.zoom, return_ms=True)[4]
            plan_ms.append(acc_p / args.repeats); mapk.append(acc_m / args.repeats)
            for c in (3, 1):
                fused[c].append(acc_f[c] / args.repeats); rolled[c].append(acc_r[c] / args.repeats)
        plan_ms, mapk = np.array(plan_ms), np.array(mapk)
        out["path_kernels_ms"] = spread(plan_ms[:, 0])
        out["smooth_kernel_ms"] = spread(plan_ms[:, 1])
        out["zoom_kernels_ms"] = spread(plan_ms[:, 2])
        out["zoom_kernels_ms_per_frame"] = spread(plan_ms[:, 2] / args.frames)
        out["record_kernel_ms"] = spread(mapk[:, 1])
        out["map_kernel_ms_per_frame"] = spread(mapk[:, 2] / args.frames)
        for c, name in ((3, "rgb"), (1, "gray")):
            out["fused_kernel_ms_per_frame_" + name] = spread(np.array(fused[c]) / args.frames)
            out["rolling_shutter_fused_kernel_ms_per_frame_" + name] = spread(np.array(rolled[c]) / args.frames)
        out["map_kernel_ns_per_evaluation"] = float(np.mean(mapk[:, 2]) * 1e6 / (args.frames * w * h * out["evaluations_mean"] * out["valid_fraction"]))
        result["by_rate_sigma"]["%g" % sigma] = out
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
