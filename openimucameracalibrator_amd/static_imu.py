"""Static multi-pose IMU intrinsics: host-side mirror of the reference's applications/static_imu_calibration.cc and
core::StaticImuCalibrator (src/core/static_imu_calibrator.cc, restated from imu_tk) over the C-ABI entries
oicc_static_imu_*.  Static-interval detection, the accelerometer fits of all thresholds and the gyroscope residuals run
on the MI355X; the sequential pieces run on the host inside the library.  There is no CPU fallback."""
import argparse
import ctypes as C
import json
import sys

import numpy as np

from . import _abi
from . import _lib
from . import io_files

THRESHOLDS = 10
ACC_IMPOSSIBLE = 1
TERMINATIONS = {-1: "SKIPPED", 0: "GRADIENT_TOLERANCE", 1: "FUNCTION_TOLERANCE", 2: "PARAMETER_TOLERANCE",
                3: "MAX_ITERATIONS", 4: "MIN_TRUST_REGION_RADIUS", 5: "INVALID_STEPS", 6: "EVALUATION_FAILED"}

_i32p = C.POINTER(C.c_int32)
_dp = C.POINTER(C.c_double)


def _p(a, t=_dp):
    return a.ctypes.data_as(t)


def _rows3(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1, 3))


def static_intervals(acc, thresholds, win_size=101, device=0, with_norms=False, backend=None):
    """StaticIntervalsDetector for every threshold in one pass.  Returns a list of int arrays [k][2] (start, end), and
    with with_norms also the norm series (NaN outside [h, n-h)) and the device time."""
    b = backend if backend is not None else _lib.load_static_imu()
    a = _rows3(acc)
    n = a.shape[0]
    th = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).ravel())
    cap = max(n // 2 + 2, 1)
    counts = np.zeros(len(th), dtype=np.int32)
    iv = np.zeros((len(th), cap, 2), dtype=np.int32)
    norms = np.zeros(n) if with_norms else None
    ms = C.c_double()
    rc = b.intervals(int(device), n, _p(a), len(th), _p(th), int(win_size), cap, _p(counts, _i32p), _p(iv, _i32p),
                     _p(norms) if with_norms else None, C.byref(ms))
    if rc != 0:
        raise RuntimeError("oicc_static_imu_intervals failed with status %d" % rc)
    out = [iv[t, :counts[t]].copy() for t in range(len(th))]
    return (out, norms, ms.value) if with_norms else out


def eval_acc(samples, params, g_mag, device=0, backend=None):
    """MultiPosAccResidual of every sample at params[9]: dict(r, J, cost, gram, gradient)."""
    b = backend if backend is not None else _lib.load_static_imu()
    s = _rows3(samples)
    p = np.ascontiguousarray(np.asarray(params, dtype=np.float64))
    n = s.shape[0]
    r, J, H, g, cost = np.zeros(n), np.zeros((n, 9)), np.zeros((9, 9)), np.zeros(9), C.c_double()
    rc = b.eval_acc(int(device), n, _p(s), float(g_mag), _p(p), _p(r), _p(J), C.byref(cost), _p(H), _p(g))
    if rc != 0:
        raise RuntimeError("oicc_static_imu_eval_acc failed with status %d" % rc)
    return dict(r=r, J=J, cost=cost.value, gram=H, gradient=g)


def eval_gyro(t_s, gyro, ranges, g_versors, params, optimize_bias=False, gyro_dt=-1.0, device=0, backend=None):
    """MultiPosGyroResidual of every block (ranges [b][2] inclusive sample indices of the bias-free gyro samples,
    g_versors [b][6] = g0, g1): dict(r [3b], J [3b][np], cost, gram, gradient, device_ms)."""
    b = backend if backend is not None else _lib.load_static_imu()
    t = np.ascontiguousarray(np.asarray(t_s, dtype=np.float64).ravel())
    w = _rows3(gyro)
    rg = np.ascontiguousarray(np.asarray(ranges, dtype=np.int32).reshape(-1, 2))
    gv = np.ascontiguousarray(np.asarray(g_versors, dtype=np.float64).reshape(-1, 6))
    p = np.zeros(12)
    p[:len(params)] = params
    nb, npar = rg.shape[0], 12 if optimize_bias else 9
    r, J, H, g, cost, ms = np.zeros(3 * nb), np.zeros((3 * nb, npar)), np.zeros((npar, npar)), np.zeros(npar), C.c_double(), C.c_double()
    rc = b.eval_gyro(int(device), len(t), _p(t), _p(w), nb, _p(rg, _i32p), _p(gv), int(bool(optimize_bias)), float(gyro_dt), _p(p),
                     _p(r), _p(J), C.byref(cost), _p(H), _p(g), C.byref(ms))
    if rc != 0:
        raise RuntimeError("oicc_static_imu_eval_gyro failed with status %d" % rc)
    return dict(r=r, J=J, cost=cost.value, gram=H, gradient=g, device_ms=ms.value)


def triad_matrices(params):
    """ThreeAxisSensorCalibParams(misYZ, misZY, misZX, misXZ, misXY, misYX, sX, sY, sZ, bX, bY, bZ) -> (T, K, b)."""
    p = np.asarray(params, dtype=np.float64)
    T = np.array([[1.0, -p[0], p[1]], [p[3], 1.0, -p[2]], [-p[4], p[5], 1.0]])
    return T, np.diag(p[6:9]), p[9:12].copy()


def acc_triad(acc_params):
    """The 12-vector of the accelerometer triad (lower misalignments 0)."""
    a = np.asarray(acc_params, dtype=np.float64)
    return np.r_[a[:3], 0.0, 0.0, 0.0, a[3:9]]


class StaticImuCalibrator:
    """core::StaticImuCalibrator with the reference's method names; defaults of its constructor (.cc:44-52)."""

    def __init__(self, device=0, backend=None):
        self.device = device
        self.backend = backend
        self.opt = _abi.StaticImuOptions(9.81, 30.0, -1.0, 100, 12, 101, 0, 0, 0)
        self.verbose = True
        self.acc_params = np.r_[0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0]
        self.gyro_params = np.r_[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0]
        self.report = None
        self.status = None

    def SetGravityMagnitude(self, g):
        self.opt.gravity_magnitude = float(g)

    def SetInitStaticIntervalDuration(self, duration_s):
        self.opt.init_interval_duration_s = float(duration_s)

    def SetIntarvalsNumSamples(self, num):
        self.opt.interval_n_samples = int(num)

    def EnableAccUseMeans(self, enabled):
        self.opt.acc_use_means = int(bool(enabled))

    def SetGyroDataPeriod(self, dt):
        self.opt.gyro_dt = float(dt)

    def EnableGyroBiasOptimization(self, enabled):
        self.opt.optimize_gyro_bias = int(bool(enabled))

    def EnableVerboseOutput(self, enabled):
        self.verbose = bool(enabled)

    def _run(self, t_s, acc, gyro):
        b = self.backend if self.backend is not None else _lib.load_static_imu()
        t = np.ascontiguousarray(np.asarray(t_s, dtype=np.float64).ravel())
        a, g = _rows3(acc), _rows3(gyro)
        if not (len(t) == a.shape[0] == g.shape[0]):
            raise ValueError("timestamps, accelerometer and gyroscope differ in length")
        ap, gp, rep = np.zeros(9), np.zeros(12), _abi.StaticImuReport()
        rc = b.calibrate(int(self.device), len(t), _p(t), _p(a), _p(g), C.byref(self.opt), _p(ap), _p(gp), C.byref(rep))
        if rc not in (0, ACC_IMPOSSIBLE):
            raise RuntimeError("oicc_static_imu_calibrate failed with status %d" % rc)
        self.status, self.report = rc, report_dict(rep)
        self.acc_params, self.gyro_params = ap, gp
        return rc == 0

    def CalibrateAcc(self, t_s, acc):
        """The accelerometer part; the gyroscope fit also runs (on the accelerometer samples as gyro input it is cheap and
        its result is discarded: getGyroCalib keeps the default triad, as after the reference's CalibrateAcc)."""
        ok = self._run(t_s, acc, np.zeros_like(_rows3(acc)))
        self.gyro_params = np.r_[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0]
        return ok

    def CalibrateAccGyro(self, t_s, acc, gyro):
        return self._run(t_s, acc, gyro)

    def getAccCalib(self):
        """(T, K, b) of the accelerometer triad."""
        return triad_matrices(acc_triad(self.acc_params))

    def getGyroCalib(self):
        """(T, K, b) of the gyroscope triad."""
        return triad_matrices(self.gyro_params)


def report_dict(rep):
    return dict(th_mult=rep.th_mult, num_intervals=list(rep.num_intervals), acc_iterations=list(rep.acc_iterations),
                acc_termination=list(rep.acc_termination), acc_final_cost=list(rep.acc_final_cost), norm_th=rep.norm_th,
                init_acc_bias=list(rep.init_acc_bias), gyro_init_bias=list(rep.gyro_init_bias), gyro_num_blocks=rep.gyro_num_blocks,
                gyro_iterations=rep.gyro_iterations, gyro_termination=rep.gyro_termination,
                gyro_initial_cost=rep.gyro_initial_cost, gyro_final_cost=rep.gyro_final_cost,
                ms_detector=rep.ms_detector, ms_acc=rep.ms_acc, ms_gyro=rep.ms_gyro)


def calibration_json(acc_params, gyro_params):
    """The output document of applications/static_imu_calibration.cc:55-85 (nlohmann's object: keys sorted)."""
    Ta, Ka, ba = triad_matrices(acc_triad(acc_params))
    Tg, Kg, bg = triad_matrices(gyro_params)
    f = float
    return {
        "accelerometer": {"bias": [f(ba[0]), f(ba[1]), f(ba[2])],
                          "misalignment_matrix": [[1.0, f(Ta[0, 1]), f(Ta[0, 2])], [0.0, 1.0, f(Ta[1, 2])], [0.0, 0.0, 1.0]],
                          "scale_matrix": [[f(Ka[0, 0]), 0.0, 0.0], [0.0, f(Ka[1, 1]), 0.0], [0.0, 0.0, f(Ka[2, 2])]]},
        "gyroscope": {"bias": [f(bg[0]), f(bg[1]), f(bg[2])],
                      "misalignment_matrix": [[1.0, f(Tg[0, 1]), f(Tg[0, 2])], [f(Tg[1, 0]), 1.0, f(Tg[1, 2])], [f(Tg[2, 0]), f(Tg[2, 1]), 1.0]],
                      "scale_matrix": [[f(Kg[0, 0]), 0.0, 0.0], [0.0, f(Kg[1, 1]), 0.0], [0.0, 0.0, f(Kg[2, 2])]]},
    }


def write_calibration_json(path, acc_params, gyro_params):
    with open(path, "w") as fh:
        json.dump(calibration_json(acc_params, gyro_params), fh, indent=4, sort_keys=True)
        fh.write("\n")


def main(argv=None):
    ap = argparse.ArgumentParser(description="Multi-pose accelerometer and gyroscope intrinsics (static_imu_calibration)")
    ap.add_argument("--telemetry_json", default="", help="Path to the telemetry json.")
    ap.add_argument("--gravity_magnitude", default=9.811107, type=float, help="Gravity magnitude.")
    ap.add_argument("--initial_static_interval_s", default=10.0, type=float,
                    help="Length of the initial static interval for bias estimation.")
    ap.add_argument("--output_calibration_path", default="", help="path to output calibration json")
    ap.add_argument("--verbose", action="store_true", help="If more stuff should be printed")
    ap.add_argument("--device", default=0, type=int)
    args = io_files.parse_reference_flags(ap, argv)
    with open(args.telemetry_json) as f:
        tel = json.load(f)
    t_s = np.asarray(tel["timestamps_ns"], dtype=np.float64) * 1e-9     # read_telemetry.cc: timestamp_s
    cal = StaticImuCalibrator(device=args.device)
    cal.SetGravityMagnitude(args.gravity_magnitude)
    cal.SetInitStaticIntervalDuration(args.initial_static_interval_s)
    cal.EnableVerboseOutput(args.verbose)
    if not cal.CalibrateAccGyro(t_s, tel["accelerometer"], tel["gyroscope"]):
        print("Failed to calibra accelerometer", file=sys.stderr)       # main ignores the failure (.cc:47-50)
    r = cal.report
    print("Accelerometers calibration: threshold multiplier %d, %s intervals; gyroscope residual %.6g (%d iterations)"
          % (r["th_mult"], r["num_intervals"], r["gyro_final_cost"], r["gyro_iterations"]))
    write_calibration_json(args.output_calibration_path, cal.acc_params, cal.gyro_params)


if __name__ == "__main__":
    main()
