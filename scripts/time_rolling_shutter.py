#!/usr/bin/env python
"""Timings of the rolling-shutter rectification on the GPU ("Rolling-shutter rectification"): 64 frames of 960 x 540 at
30 fps, RGB and gray, gopro9_division onto its rectified pinhole, a 200 Hz gyroscope with N(0, sigma) rad/s per axis.

  python scripts/time_rolling_shutter.py [--frames 64] [--runs 3] [--repeats 20] [--batch 16] [--rate_sigma 1.0 4.0] [--out FILE]

HIP events inside the library: table kernel, ray kernel and map kernel of oicc_rs_rectify_map, the fused kernel of
oicc_rs_rectify_frames (summed over its batches), and next to them the static remap kernel of oicc_camera_remap at the same size;
warm; `runs` runs of `repeats` calls, the routes alternating inside every repeat.  Evaluations per pixel come from the map entry.
Fails without a GPU: there is no CPU path to time."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openimucameracalibrator_amd import camera_maps as cm              # noqa: E402
from openimucameracalibrator_amd import rolling_shutter as rs          # noqa: E402
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
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    model, intr, w, h = S.CAMERAS["gopro9_division"]
    rng = np.random.RandomState(1)
    frames = {3: rng.randint(0, 256, (args.frames, h, w, 3)).astype(np.uint8), 1: rng.randint(0, 256, (args.frames, h, w)).astype(np.uint8)}
    dst = cm.rectified_pinhole(model, intr, w, h)
    static_map = cm.rectify_map(model, intr, w, h, S.CAM_PINHOLE, dst, w, h)[0]
    frame_t = 100.0 + 0.05 + np.arange(args.frames) / 30.0
    n_gyro = int((frame_t[-1] - 100.0 + 0.1) * 200.0)
    gyro_t = 100.0 + np.arange(n_gyro) / 200.0 + rng.uniform(-2e-4, 2e-4, n_gyro)
    unit = rng.normal(0.0, 1.0, (n_gyro, 3))
    result = dict(frames=args.frames, width=w, height=h, batch=args.batch, runs=args.runs, repeats=args.repeats, line_delay_us=30.0, by_rate_sigma={})
    for sigma in args.rate_sigma:
        scene = rs.Scene((model, intr, w, h), (S.CAM_PINHOLE, dst, w, h), gyro_t, unit * sigma, frame_t, 30e-6)
        mapxy, valid, status, num_valid, evals, ms = rs.rs_rectify_map(scene, return_evaluations=True, return_ms=True)      # warm
        assert np.all(status == 0)
        out = dict(valid_fraction=float(valid.mean()), evaluations_mean=float(evals[valid == 1].mean()), evaluations_max=int(evals.max()))
        del mapxy, evals
        for c in (3, 1):
            rs.rs_rectify_frames(frames[c], scene, batch=args.batch)
            cm.remap(frames[c], static_map, batch=args.batch)
        table, rays, mapk = [], [], []
        fused = {3: [], 1: []}; static = {3: [], 1: []}
        for _ in range(args.runs):
            acc = np.zeros(3); acc_f = {3: 0.0, 1: 0.0}; acc_s = {3: 0.0, 1: 0.0}
            for _ in range(args.repeats):
                for c in (3, 1):                                           # the routes alternate inside a repeat
                    rep = {}
                    rs.rs_rectify_frames(frames[c], scene, batch=args.batch, report=rep)
                    acc_f[c] += rep["ms_kernel"]
                    rep = {}
                    cm.remap(frames[c], static_map, batch=args.batch, report=rep)
                    acc_s[c] += rep["ms_kernel"]
                acc += rs.rs_rectify_map(scene, return_ms=True)[4]
            table.append(acc[0] / args.repeats); rays.append(acc[1] / args.repeats); mapk.append(acc[2] / args.repeats)
            for c in (3, 1):
                fused[c].append(acc_f[c] / args.repeats); static[c].append(acc_s[c] / args.repeats)
        out["table_kernel_ms"] = spread(table)
        out["ray_kernel_ms"] = spread(rays)
        out["map_kernel_ms_per_frame"] = spread(np.array(mapk) / args.frames)
        for c, name in ((3, "rgb"), (1, "gray")):
            out["fused_kernel_ms_per_frame_" + name] = spread(np.array(fused[c]) / args.frames)
            out["static_remap_kernel_ms_per_frame_" + name] = spread(np.array(static[c]) / args.frames)
        out["map_kernel_ns_per_evaluation"] = float(np.mean(mapk) * 1e6 / (args.frames * w * h * out["evaluations_mean"] * out["valid_fraction"]))
        result["by_rate_sigma"]["%g" % sigma] = out
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
