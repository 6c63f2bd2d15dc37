"""Time the Allan variance of six channels on the device (oicc_allan_variance's device_ms: scan + variance + reduction
launches) for 2 h and 4 h at 200 Hz, and a reference-shaped single-core C++ loop (scripts/allan_cpu_loop.cpp, the
reference's calcThetas + calcVariance) on channels of the same data.  Prints one JSON line.
usage: python scripts/time_allan.py [--repeats 5] [--cpu_channels 1] [--out DIR]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openimucameracalibrator_amd import allan as A, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu_channels", type=int, default=1, help="channels timed on the CPU (0: none); the six-channel CPU time is this x 6 / cpu_channels")
    ap.add_argument("--out", default=tempfile.mkdtemp())
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    exe = os.path.join(args.out, "allan_cpu_loop")
    if args.cpu_channels:
        subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "scripts", "allan_cpu_loop.cpp"), "-o", exe])
    scale = np.array([1.0, 1.0, 1.0, A.GYRO_SCALE, A.GYRO_SCALE, A.GYRO_SCALE])
    result = {}
    for hours in (2, 4):
        tel, _ = synthetic.make_stationary_imu(duration=hours * 3600.0, rate=200.0, seed=21)
        w = np.concatenate([tel["accelerometer"].T, tel["gyroscope"].T], axis=0)
        t = tel["timestamps_ns"] * 1e-9
        n = len(t)
        v = A.allan_variance(w, t, scale)                                  # warm-up
        ms = sorted(A.allan_variance(w, t, scale)["device_ms"] for _ in range(args.repeats))
        terms = 6 * int(np.sum(np.maximum(n - 2 * v["factors"].astype(np.int64), 0)))
        r = dict(n=n, channels=6, num_factors=int(len(v["factors"])), terms=terms, device_ms_median=ms[len(ms) // 2], device_ms_min=ms[0],
                 terms_per_ns=terms / (ms[len(ms) // 2] * 1e6))
        if args.cpu_channels:
            fac_path = os.path.join(args.out, "factors.i32")
            v["factors"].astype(np.int32).tofile(fac_path)
            cpu = []
            for c in range(6 - args.cpu_channels, 6):
                path = os.path.join(args.out, "w.f64")
                np.ascontiguousarray(w[c] * scale[c]).tofile(path)
                o = subprocess.run([exe, path, str(n), repr(v["freq"]), repr(v["period"]), fac_path, str(len(v["factors"]))],
                                   capture_output=True, text=True, check=True).stdout.split()
                cpu.append(float(o[0]))
                rel = abs(float(o[1]) - v["sigma2"][c, 0]) / v["sigma2"][c, 0]
                assert rel < 1e-8, rel
            r["cpu_s_per_channel"] = cpu
            r["cpu_s_six_channels_est"] = float(np.mean(cpu) * 6)
        result["%dh_200Hz" % hours] = r
    print(json.dumps(result))


if __name__ == "__main__":
    main()
