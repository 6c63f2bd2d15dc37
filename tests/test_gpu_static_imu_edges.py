"""The static IMU calibration on the device at the edges of its own code (csrc/static_imu.hip), cases of static_imu_cases.py:
the detector's norms bit for bit and its interval lists exactly -- window sizes 11 ... 1025, tile tails, interval edges on lane 0,
63, 64, 255 and across workgroups, thresholds equal to a norm, a caller's capacity below the count; eval_gyro and eval_acc
against the 50-digit restatement (static_imu_reference.py) within DEVICE_FACTOR x the float64 yardstick of the case class
(YARDSTICK, measured on the host by test_static_imu_reference.py) -- step counts where the chunking of simu_gyro_kernel changes,
sample counts that leave lanes and waves of acc_normal_eq idle; and the whole calibration under the options no other test sets,
against the float64 restatement.  Every figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest

import static_imu_cases as K
import static_imu_reference as R
import static_imu_restatement as S
from openimucameracalibrator_amd import _lib, static_imu as SI, synthetic

pytestmark = pytest.mark.gpu

INVALID_ARG = -1          # OICC_ERR_INVALID_ARG (include/oicc_hip.h)
_i32p = C.POINTER(C.c_int32)
_dp = C.POINTER(C.c_double)


def check(figures, yardstick=True):
    """figures: (name, value, bound).  Prints all, then asserts all.  yardstick: the bounds are DEVICE_FACTOR x a yardstick."""
    ratio = lambda f: f[1] / f[2] if f[2] > 0 else (0.0 if f[1] == 0 else np.inf)
    for f in figures:
        print("%-28s %.3e  bound %.3e  ratio %.4f" % (f[0], f[1], f[2], ratio(f)) + ("  (%.2f x yardstick)" % (ratio(f) * R.DEVICE_FACTOR) if yardstick else ""))
    worst = max(figures, key=ratio)
    print("largest: %s %.3e = %.4f x its bound" % (worst[0], worst[1], ratio(worst)))
    bad = [f for f in figures if not f[1] <= f[2]]
    assert not bad, bad


# ---- detector --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.DETECTOR_NAMES)
def test_detector_case(name):
    case = K.detector_cases()[name]
    acc, win, th = case["acc"], case["win"], case["thresholds"]
    lists, norms, _ = SI.static_intervals(acc, th, win_size=win, with_norms=True)
    ref_norms = S.window_norms(acc, win)
    np.testing.assert_array_equal(norms, ref_norms)          # bitwise; NaN outside [h, n - h)
    h, n = case["h"], len(acc)
    assert np.all(np.isnan(norms[:h])) and np.all(np.isnan(norms[n - h:]))
    for k in range(len(th)):
        got = [tuple(int(v) for v in iv) for iv in lists[k]]
        print("%s threshold %d (%r): %d intervals" % (name, k, float(th[k]), len(got)))
        assert got == [tuple(int(v) for v in iv) for iv in S.intervals_from_norms(ref_norms, th[k], win)], (name, k)
        if case["expected"][k] is not None:
            assert got == [tuple(e) for e in case["expected"][k]], (name, k)
    lists2, norms2, _ = SI.static_intervals(acc, th, win_size=win, with_norms=True)
    assert norms.tobytes() == norms2.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(lists, lists2))


def _raw_intervals(acc, th, win, capacity, buffer_pairs, sentinel=-77):
    b = _lib.load_static_imu()
    a = np.ascontiguousarray(acc, dtype=np.float64)
    th = np.ascontiguousarray(th, dtype=np.float64)
    counts = np.full(len(th), sentinel, dtype=np.int32)
    iv = np.full(2 * buffer_pairs, sentinel, dtype=np.int32)
    rc = b.intervals(0, len(a), a.ctypes.data_as(_dp), len(th), th.ctypes.data_as(_dp), int(win), int(capacity),
                     counts.ctypes.data_as(_i32p), iv.ctypes.data_as(_i32p), None, None)
    return rc, counts, iv


@pytest.mark.parametrize("capacity", [1, 0])
def test_capacity_below_the_count(capacity):
    """Four intervals, room for `capacity`: the count in full, the first `capacity` pairs of every threshold at [t][capacity][2],
    the rest of the caller's buffer as it was."""
    case = K.detector_cases()["table"]
    th = np.array([K.STILL_TH, 1e9])
    runs = [(5, 5), (68, 132), (260, 261), (516, 517)]
    rc, counts, iv = _raw_intervals(case["acc"], th, 11, capacity, 16)
    assert rc == 0
    assert list(counts) == [4, 1]
    expected = np.full(32, -77, dtype=np.int32)
    for t, lst in enumerate((runs, [(5, 517)])):
        for k in range(min(capacity, len(lst))):
            expected[2 * (t * capacity + k):2 * (t * capacity + k) + 2] = lst[k]
    print("capacity %d: counts %s buffer %s" % (capacity, list(counts), list(iv[:8])))
    np.testing.assert_array_equal(iv, expected)


def test_window_above_the_cap_is_refused():
    case = K.detector_cases()["noisy_win1025_M257"]
    rc, counts, iv = _raw_intervals(case["acc"], case["thresholds"], 1027, 4, 64)
    assert rc == INVALID_ARG
    assert np.all(counts == -77) and np.all(iv == -77)
    rc, counts, iv = _raw_intervals(case["acc"], case["thresholds"], 1026, 4, 64)          # normalised to 1027
    assert rc == INVALID_ARG


# ---- eval_gyro -------------------------------------------------------------------------------------------------------------
_GYRO = {}


def device_gyro(config):
    if config not in _GYRO:
        t, w, ranges, gv, p, ob, dt, _ = K.gyro_inputs(config)
        _GYRO[config] = SI.eval_gyro(t, w, ranges, gv, p, optimize_bias=ob, gyro_dt=dt)
    return _GYRO[config]


@pytest.mark.parametrize("config,cls", K.gyro_case_list())
def test_eval_gyro_block(config, cls):
    """One block of a step class: residuals and Jacobian against the 50 digits of the reference's per-step-normalised RK4."""
    d = device_gyro(config)
    classes = K.GYRO_CONFIGS[config][4]
    b = classes.index(cls)
    r, J = d["r"][3 * b:3 * b + 3], d["J"][3 * b:3 * b + 3]
    assert J.shape == (3, 12 if K.GYRO_CONFIGS[config][2] else 9)
    er, ej = R.gyro_errors(r, J, config, cls)
    check([("%s/%s r" % (config, cls), er, R.DEVICE_FACTOR * R.yardstick("gyro/r/" + cls)),
           ("%s/%s J" % (config, cls), ej, R.DEVICE_FACTOR * R.yardstick("gyro/J/" + cls))])
    if K.gyro_steps(cls) == 0:          # no step: g0 - g1 to the bit, every derivative exactly zero
        g0, g1 = K.gyro_versors()[cls]
        np.testing.assert_array_equal(r, g0 - g1)
        assert not J.any()


@pytest.mark.parametrize("config", list(K.GYRO_CONFIGS))
def test_eval_gyro_sums_are_the_row_order_sums_of_its_rows(config):
    """cost, gradient and Gram of the entry are host sums of the device's own r and J in row order: a few ulp of d_i d_j (the
    long-double sum of the same rows is the reference; a sequential float64 sum of m terms is within m eps of it)."""
    d = device_gyro(config)
    r, J = d["r"].astype(R.LD), d["J"].astype(R.LD)
    m = len(r)
    cost, H, g = r @ r / 2, J.T @ J, J.T @ r
    bound = m * R.EPS
    check([("%s cost" % config, float(abs(R.LD(d["cost"]) - cost) / cost), bound),
           ("%s gram" % config, R.entrywise_error(d["gram"], H)[0], bound),
           ("%s gradient" % config, R.gradient_error(d["gradient"], g, H, cost)[0], bound)], yardstick=False)
    np.testing.assert_array_equal(d["gram"], d["gram"].T)


def test_eval_gyro_fixed_step_ignores_the_timestamps():
    """gyro_dt > 0 is what is integrated with: the jittered and the uniform timestamps give the same bits."""
    t, w, ranges, gv, p, ob, dt, _ = K.gyro_inputs("jitter_fixed_dt")
    a = device_gyro("jitter_fixed_dt")
    b = SI.eval_gyro(K.gyro_series()["uniform"][0], w, ranges, gv, p, optimize_bias=ob, gyro_dt=dt)
    np.testing.assert_array_equal(a["r"], b["r"])
    np.testing.assert_array_equal(a["J"], b["J"])
    c = device_gyro("jitter")
    assert np.abs(a["r"] - c["r"]).max() > 1e-6          # and the jitter does matter without it


# ---- eval_acc --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", K.ACC_COUNTS)
def test_eval_acc_count(count):
    """The first `count` samples: rows against the 50-digit rows, cost, gradient and Gram against the sums of the 50-digit rows."""
    figures = []
    for name, p in K.ACC_PARAMS.items():
        d = SI.eval_acc(K.acc_samples()[:count], p, K.G)
        er, ej = R.acc_row_errors(d["r"], d["J"], name)
        eh, eg, ec = R.acc_sum_errors(d["cost"], d["gram"], d["gradient"], name, count)
        figures += [("%s/%d r" % (name, count), er, R.DEVICE_FACTOR * R.yardstick("acc/r")),
                    ("%s/%d J" % (name, count), ej, R.DEVICE_FACTOR * R.yardstick("acc/J")),
                    ("%s/%d gram" % (name, count), eh, R.DEVICE_FACTOR * R.yardstick("acc/H/%d" % count)),
                    ("%s/%d gradient" % (name, count), eg, R.DEVICE_FACTOR * R.yardstick("acc/g/%d" % count)),
                    ("%s/%d cost" % (name, count), ec, R.DEVICE_FACTOR * R.yardstick("acc/cost/%d" % count))]
        np.testing.assert_array_equal(d["gram"], d["gram"].T)
    check(figures)


# ---- the calibration under its other options ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recording():
    tel, truth = synthetic.make_static_multipose_imu(**K.RECORDING)
    return tel["timestamps_ns"] * 1e-9, tel


@pytest.mark.parametrize("config", list(K.CALIBRATION_CONFIGS))
def test_calibration_options_match_restatement(recording, config):
    """What test_calibration_matches_restatement asserts, with its tolerances (both sides are the same float64 algorithm), under
    acc_use_means (fits of 14 samples: three idle waves), 7 samples per interval, a 41-sample window, a fixed gyro step with the
    bias optimised."""
    t, tel = recording
    calls, fields, kw = K.CALIBRATION_CONFIGS[config]
    cal = SI.StaticImuCalibrator()
    cal.SetGravityMagnitude(K.G)
    cal.SetInitStaticIntervalDuration(K.CALIBRATION_INIT_S)
    for name, v in calls:
        getattr(cal, name)(v)
    for name, v in fields.items():
        setattr(cal.opt, name, v)
    ok = cal.CalibrateAccGyro(t, tel["accelerometer"], tel["gyroscope"])
    ref = S.calibrate(t, tel["accelerometer"], tel["gyroscope"], g_mag=K.G, init_s=K.CALIBRATION_INIT_S, **kw)
    rep = cal.report
    print(config, "th_mult", rep["th_mult"], "intervals", rep["num_intervals"], "acc iterations", rep["acc_iterations"],
          "gyro iterations", rep["gyro_iterations"], "blocks", rep["gyro_num_blocks"])
    assert max(p["num"] for p in ref["per_threshold"]) >= 12, "the recording leaves fewer than 12 intervals at every threshold"
    assert ok and cal.status == 0 and ref["status"] == 0
    assert rep["th_mult"] == ref["th_mult"]
    assert rep["num_intervals"] == [p["num"] for p in ref["per_threshold"]]
    assert rep["acc_iterations"] == [p["iterations"] for p in ref["per_threshold"]]
    assert rep["acc_termination"] == [p["termination"] for p in ref["per_threshold"]]
    for k, p in enumerate(ref["per_threshold"]):
        if p["termination"] != S.TERM_SKIPPED:
            print("  threshold %d cost %.17g restatement %.17g" % (k + 1, rep["acc_final_cost"][k], p["cost"]))
            assert abs(rep["acc_final_cost"][k] - p["cost"]) <= 1e-9 * p["cost"]
    print("  acc params error", np.abs(cal.acc_params - ref["acc_params"]).max(), "gyro params error", np.abs(cal.gyro_params - ref["gyro_params"]).max())
    np.testing.assert_allclose(cal.acc_params, ref["acc_params"], rtol=1e-9, atol=1e-12)
    assert rep["gyro_iterations"] == ref["gyro_iterations"] and rep["gyro_termination"] == ref["gyro_termination"]
    assert rep["gyro_num_blocks"] == len(ref["gyro_ranges"])
    np.testing.assert_allclose(cal.gyro_params, ref["gyro_params"], rtol=1e-9, atol=1e-12)
    assert rep["norm_th"] == ref["norm_th"]
    np.testing.assert_array_equal(rep["init_acc_bias"], ref["init_acc_bias"])
