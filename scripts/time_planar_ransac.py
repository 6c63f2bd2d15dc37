"""Time the robust start poses (oicc_planar_ransac): 2000 views of 40 and of 126 corners, 15 % of them moved 10-60 px,
256 hypotheses per view, both modes.  Per case: the kernel by device events and the whole call by the wall clock (median
of --repeats after a warm-up), against (a) the host start values on the same views (numpy planar_init.initialize_view
per view: what this step costs without the option) and (b) the numpy restatement on one core (timed on 30 views, scaled
to 2000).  Prints one JSON line.
usage: python scripts/time_planar_ransac.py [--repeats 5] [--views 2000] [--no_cpu]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from openimucameracalibrator_amd import camera_calibrator as CC, planar_init, robust_init as RI, synthetic as S  # noqa: E402


def views_of(camera, nx, ny, calibrated, seed=3):
    """30 views of an nx x ny board under the poses of make_calibration_dataset: (points, [(ids, features)], threshold)."""
    ds = CC.make_calibration_dataset(camera, num_views=30, corners_per_view=40)
    gx, gy = np.meshgrid(np.linspace(0, 7 * 0.021, nx), np.linspace(0, 5 * 0.021, ny))
    pts = np.stack([gx.ravel(), gy.ravel(), np.zeros(nx * ny), np.ones(nx * ny)], -1)
    rng = np.random.default_rng(seed)
    w, h = ds["width"], ds["height"]
    views = []
    for pose in ds["pose_true"]:
        pc = (pts[:, :3] - pose[:3]) @ CC.angle_axis_to_rotation(pose[3:]).T
        px, _ = S.project(ds["model"], ds["intrinsics"], pc)
        px = px + rng.normal(0, 0.2, px.shape)
        o = rng.choice(len(px), int(0.15 * len(px)), replace=False)
        ang = rng.uniform(0, 2 * np.pi, len(o)); mag = rng.uniform(10, 60, len(o))
        px[o] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1)
        feat = planar_init.pixel_to_normalized(ds["model"], ds["intrinsics"], px) if calibrated else px - [w / 2.0, h / 2.0]
        views.append((np.arange(len(pts), dtype=np.int32), feat))
    thr = 0.004 * h / ds["intrinsics"][0] if calibrated else 0.003 * h
    return pts, views, thr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--views", type=int, default=2000)
    ap.add_argument("--hypotheses", type=int, default=256)
    ap.add_argument("--camera", default="gopro9_division")
    ap.add_argument("--no_cpu", action="store_true")
    args = ap.parse_args()
    hip = RI.HipBackend()
    out = {}
    for corners, (nx, ny) in ((40, (8, 5)), (126, (14, 9))):
        for calibrated in (False, True):
            pts, views30, thr = views_of(args.camera, nx, ny, calibrated)
            views = [views30[i % 30] for i in range(args.views)]
            off, ab, xy = RI.pack_views(pts, views)
            mode = RI.CALIBRATED if calibrated else RI.UNCALIBRATED
            hip.run(off[:31], ab[:off[30]], xy[:off[30]], mode, thr, args.hypotheses)        # warm-up: module load
            dev, wall = [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                inl, num, _, _, _ = hip.run(off, ab, xy, mode, thr, args.hypotheses)
                wall.append((time.perf_counter() - t0) * 1e3); dev.append(hip.device_ms)
            row = dict(views=args.views, corners=corners, hypotheses=args.hypotheses, kernel_ms=round(float(np.median(dev)), 3),
                       kernel_ms_min_max=[round(min(dev), 3), round(max(dev), 3)], call_ms=round(float(np.median(wall)), 3), inlier_share=round(float(inl.mean()), 4))
            if not args.no_cpu:
                t0 = time.perf_counter()
                for pid, feat in views:
                    planar_init.initialize_view(pts, pid, feat, focal=1.0 if calibrated else None)
                row["host_start_values_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                import planar_ransac_restatement as PR
                o30, a30, x30 = RI.pack_views(pts, views30)
                t0 = time.perf_counter()
                PR.run(o30, a30, x30, mode, thr, args.hypotheses)
                row["restatement_ms_1core"] = round((time.perf_counter() - t0) * 1e3 * args.views / 30.0, 1)
            out["%dx%d_%s" % (args.views, corners, "calibrated" if calibrated else "uncalibrated")] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
