#!/usr/bin/env python
"""Timings of the camera maps on the GPU: 64 frames of 960 x 540, RGB and gray, gopro9_division.

  python scripts/time_camera_maps.py [--frames 64] [--runs 3] [--repeats 20] [--batch 16] [--out FILE]

HIP events inside the library (map kernel, upload / kernel / download of oicc_camera_remap) and torch events around
oicc_camera_remap_device; warm; `runs` runs of `repeats` calls with the routes alternating inside every repeat.  The remap kernel's
rate is its algorithmic traffic -- the frames in, the frames out, the map once per batch -- over its device time.  Baseline: the
numpy restatement of tests/ on the CPU of the same machine (one frame, scaled).  Also: oicc_camera_unproject for every pixel of the
image per model against planar_init.pixel_to_normalized.  Fails without a GPU: there is no CPU path to time."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import camera_maps_restatement as R                                    # noqa: E402
from openimucameracalibrator_amd import camera_maps as cm              # noqa: E402
from openimucameracalibrator_amd import planar_init                    # noqa: E402
from openimucameracalibrator_amd import synthetic as S                 # noqa: E402


def spread(v):
    return dict(min=float(np.min(v)), mean=float(np.mean(v)), max=float(np.max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    model, intr, w, h = S.CAMERAS["gopro9_division"]
    rng = np.random.RandomState(1)
    frames = {3: rng.randint(0, 256, (args.frames, h, w, 3)).astype(np.uint8), 1: rng.randint(0, 256, (args.frames, h, w)).astype(np.uint8)}
    dst = cm.rectified_pinhole(model, intr, w, h)
    mapxy, valid, num_valid = cm.rectify_map(model, intr, w, h, S.CAM_PINHOLE, dst, w, h)
    tensors = {c: torch.from_numpy(f).cuda() for c, f in frames.items()}
    map_t = torch.from_numpy(mapxy).cuda()
    result = dict(frames=args.frames, width=w, height=h, batch=args.batch, runs=args.runs, repeats=args.repeats)

    # warm: every route once
    for c in (3, 1):
        cm.remap(frames[c], mapxy, batch=args.batch)
        cm.remap(tensors[c], map_t)
    torch.cuda.synchronize()

    host = {c: dict(ms_upload=[], ms_kernel=[], ms_download=[], ms_total=[], wall_ms=[]) for c in (3, 1)}
    dev = {c: [] for c in (3, 1)}
    map_ms = []
    for _ in range(args.runs):
        acc_host = {c: dict(ms_upload=0.0, ms_kernel=0.0, ms_download=0.0, ms_total=0.0, wall_ms=0.0) for c in (3, 1)}
        acc_dev = {3: 0.0, 1: 0.0}
        acc_map = 0.0
        for _ in range(args.repeats):
            for c in (3, 1):                                           # the routes alternate inside a repeat
                rep = {}
                t0 = time.perf_counter()
                cm.remap(frames[c], mapxy, batch=args.batch, report=rep)
                acc_host[c]["wall_ms"] += (time.perf_counter() - t0) * 1e3
                for k in ("ms_upload", "ms_kernel", "ms_download", "ms_total"):
                    acc_host[c][k] += rep[k]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                cm.remap(tensors[c], map_t)
                e1.record()
                e1.synchronize()
                acc_dev[c] += e0.elapsed_time(e1)
            acc_map += cm.rectify_map(model, intr, w, h, S.CAM_PINHOLE, dst, w, h, return_ms=True)[3]
        for c in (3, 1):
            for k in host[c]:
                host[c][k].append(acc_host[c][k] / args.repeats)
            dev[c].append(acc_dev[c] / args.repeats)
        map_ms.append(acc_map / args.repeats)

    result["map_kernel_ms"] = spread(map_ms)
    pixels = w * h
    for c, name in ((3, "rgb"), (1, "gray")):
        nbatches = -(-args.frames // args.batch)
        traffic = 2.0 * args.frames * pixels * c + nbatches * pixels * 8.0       # frames in + frames out + the map once per batch
        r = {k: spread(v) for k, v in host[c].items()}
        r["kernel_ms_per_frame"] = spread(np.array(host[c]["ms_kernel"]) / args.frames)
        r["kernel_algorithmic_bytes"] = traffic
        r["kernel_GBps"] = spread(traffic / (np.array(host[c]["ms_kernel"]) * 1e-3) / 1e9)
        r["device_entry_ms"] = spread(dev[c])
        r["device_entry_ms_per_frame"] = spread(np.array(dev[c]) / args.frames)
        r["device_entry_GBps"] = spread((2.0 * args.frames * pixels * c + pixels * 8.0) / (np.array(dev[c]) * 1e-3) / 1e9)
        t0 = time.perf_counter()
        R.remap(frames[c][:1], mapxy)
        r["numpy_restatement_ms_per_frame"] = (time.perf_counter() - t0) * 1e3
        result["remap_" + name] = r

    uv = R.pixel_grid(w, h)
    unp = {}
    for cam, (m, i, cw, ch) in S.CAMERAS.items():
        cm.unproject(m, i, uv)
        ms = [cm.unproject(m, i, uv, return_ms=True)[2] for _ in range(args.repeats)]
        walls = []
        for _ in range(3):
            t0 = time.perf_counter(); cm.unproject(m, i, uv); walls.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        planar_init.pixel_to_normalized(m, i, uv)
        unp[cam] = dict(kernel_ms=spread(ms), call_ms=spread(walls), pixel_to_normalized_ms=(time.perf_counter() - t0) * 1e3)
    result["unproject_960x540"] = unp
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
