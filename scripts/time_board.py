"""Time radon board extraction (oicc_board_radon_detect) for batches of 64 frames at 960x540 and 1920x1080: the device
time of every kernel, grid assembly and the marker decision on the host, host PNG decoding (Pillow, one core) and a
single-core CPU loop over the numpy restatement (tests/board_restatement.py).  There is no OpenCV on this project's
machines, so there is no findChessboardCornersSB baseline.  Prints one JSON line.
usage: python scripts/time_board.py [--repeats 3] [--frames 64] [--no_cpu]"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from openimucameracalibrator_amd import board_extractor as BE, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--no_cpu", action="store_true")
    args = ap.parse_args()
    from PIL import Image
    import torch
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    base = synthetic.render_radon_views("gopro9_division", 16, tilt_deg=25, noise_sigma=1.0, device=dev)["images"]
    out = {}
    for name, up in (("960x540", 1), ("1920x1080", 2)):
        frames = np.concatenate([base] * (args.frames // 16 + 1))[:args.frames]
        if up > 1:
            frames = frames.repeat(up, 1).repeat(up, 2)                  # the same boards at twice the size
        BE.radon_detect(frames[:2], 1.0, 14, 9)                          # warm-up: module load, allocations
        reps = []
        for _ in range(args.repeats):
            _, found, ncand, rep = BE.radon_detect(frames, 1.0, 14, 9)
            reps.append(rep)
        best = min(reps, key=lambda r: r["ms_total"])
        pngs = []
        for im in frames[:8]:
            b = io.BytesIO(); Image.fromarray(im).save(b, format="PNG"); pngs.append(b.getvalue())
        t0 = time.perf_counter()
        for p in pngs:
            np.asarray(Image.open(io.BytesIO(p)).convert("L"))
        ms_decode = (time.perf_counter() - t0) * 1e3 / len(pngs)
        row = {k: round(best[k], 3) for k in ("ms_resize", "ms_response", "ms_candidates", "ms_subpix", "ms_marker", "ms_assembly_host", "ms_total")}
        dev_ms = sum(best[k] for k in ("ms_resize", "ms_response", "ms_candidates", "ms_subpix", "ms_marker"))
        row.update(frames=len(frames), found=int(found.sum()), candidates_per_frame=float(np.mean(ncand)),
                   device_frames_per_s=round(len(frames) / (dev_ms * 1e-3), 1), call_frames_per_s=round(len(frames) / (best["ms_total"] * 1e-3), 1),
                   png_decode_ms_per_frame_1core=round(ms_decode, 2))
        if not args.no_cpu:
            import board_restatement as BR
            t0 = time.perf_counter()
            BR.detect(frames[:1], 1.0, 14, 9)
            row["restatement_s_per_frame_1core"] = round(time.perf_counter() - t0, 2)
        out[name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
