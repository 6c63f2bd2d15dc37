"""Covariance of the view bundle adjustment (GPU box): python scripts/time_ba_covariance.py [--runs 3] [--repeats 20]
Device time of one oicc_ba_estimate_covariance (HIP events on the library's stream: option covariance_timing,
oicc_ba_get_covariance_timing) for
  calib   45 views x 40 corners, poses + the intrinsics of the third stage of RunCalibration (d = 6, a = 6)
  poses   2000 views x 40 corners, poses only (d = 6, a = 0)
split into the assembly pass -- the device work of one oicc_ba_evaluate on the same problem, the yardstick -- and the covariance
kernels behind it, next to the whole call on the host clock (it ends in a device synchronise: launches + read-back).  Per case
`runs` times the median, minimum and maximum of `repeats` estimates after a warm-up."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from openimucameracalibrator_amd import camera_calibrator as CC

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--repeats", type=int, default=20)
a = ap.parse_args()
POSE = CC.BA_POSITION | CC.BA_ORIENTATION

for name, nv, bits in (("calib", 45, CC.PRINCIPAL_POINTS | CC.FOCAL_LENGTH | CC.ASPECT_RATIO | CC.RADIAL_DISTORTION), ("poses", 2000, 0)):
    ds = CC.make_calibration_dataset("pinhole", num_views=nv, corners_per_view=40)
    ba = CC.ViewBundleAdjuster()
    ba.SetCamera(ds["model"], ds["intrinsics"]); ba.SetScenePoints(ds["points"])
    ba.SetViews(ds["pose_init"], ds["corner_offset"], ds["uv"], ds["point_ids"])
    ba.SetOption("covariance_timing", 1)                    # HIP events around the two parts of every estimate
    mask = CC.intrinsics_mask(ds["model"], bits)
    for _ in range(5):                                      # warm-up: code objects, buffers
        info = ba.EstimateCovariance(POSE, mask)
    assert info["status"] == CC.COV_OK, info
    for run in range(a.runs):
        asm, cov, call = [], [], []
        for _ in range(a.repeats):
            t = time.perf_counter(); ba.EstimateCovariance(POSE, mask); call.append(1e3 * (time.perf_counter() - t))
            m = ba.CovarianceTiming(); asm.append(m[0]); cov.append(m[1])
        f = lambda x: "%.4f ms (min %.4f, max %.4f)" % (np.median(x), min(x), max(x))
        print("%s run %d: assembly pass %s; covariance kernels %s; ratio of the medians %.2f; whole call %s  [%d estimates; %d views, %d observations, P = %d]"
              % (name, run, f(asm), f(cov), np.median(cov) / np.median(asm), f(call), a.repeats, nv, len(ds["uv"]), info["P"]), flush=True)
