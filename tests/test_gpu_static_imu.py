"""GPU checks of the static multi-pose IMU calibration (static_imu_calibration) against the numpy restatement
(tests/static_imu_restatement.py): the detector's interval lists exactly, the residual evaluations to rounding, the
whole CalibrateAccGyro (threshold, interval counts, iteration counts, terminations, parameters), recovery of the
generator's truth, repeatability, and the application against the Python mirror."""
import json
import os
import subprocess

import numpy as np
import pytest

import static_imu_restatement as R
from static_imu_cases import plain_detector_loop
from openimucameracalibrator_amd import io_files, static_imu as SI, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "openimucameracalibrator_amd", "csrc", "static_imu_calibration")
G = 9.811107


def _recording(**kw):
    tel, truth = synthetic.make_static_multipose_imu(**kw)
    return tel["timestamps_ns"] * 1e-9, tel, truth


@pytest.fixture(scope="module")
def rec200():
    return _recording()


@pytest.fixture(scope="module")
def ref200(rec200):
    t, tel, _ = rec200
    return R.calibrate(t, tel["accelerometer"], tel["gyroscope"], g_mag=G, init_s=10.0)


def _thresholds(t, acc, init_s=10.0):
    s, e = R.initial_interval(t, init_s)
    nt = float(R.norm3(R.data_variance(acc, s, e)))
    return np.arange(1, 11) * nt


@pytest.mark.parametrize("rate,poses", [(200.0, 36), (1000.0, 14)])
def test_detector_lists_equal_restatement(rate, poses):
    t, tel, _ = _recording(rate=rate, num_poses=poses, seed=5)
    acc = tel["accelerometer"]
    th = _thresholds(t, acc)
    dev, norms, ms = SI.static_intervals(acc, th, with_norms=True)
    ref_norms = R.window_norms(acc)
    np.testing.assert_array_equal(norms, ref_norms)              # bitwise, NaN outside [h, n-h)
    for k in range(10):
        np.testing.assert_array_equal(dev[k], R.intervals_from_norms(ref_norms, th[k]))
    # the recording ends still: at th_mult 10 an interval is open at the end and closes at n-h-1
    assert dev[9][-1, 1] == len(acc) - 50 - 1
    assert ms > 0


def test_detector_plain_loop_and_short_series():
    rng = np.random.RandomState(3)
    acc = rng.standard_normal((1500, 3)) * 0.02 + np.array([0.0, 0.0, 9.8])
    acc[400:700] += rng.standard_normal((300, 3)) * 0.5
    acc[1100:1300] += rng.standard_normal((200, 3)) * 0.5
    th = np.array([0.5, 1.0, 2.0]) * 1e-3
    dev = SI.static_intervals(acc, th)
    for k in range(3):   # utils::StaticIntervalsDetector, literally
        assert [tuple(x) for x in dev[k]] == plain_detector_loop(acc, th[k])
    for n in (101, 60, 3):   # win_size >= n: no intervals
        lists, norms, _ = SI.static_intervals(acc[:n], th, with_norms=True)
        assert all(len(x) == 0 for x in lists) and np.all(np.isnan(norms))
    lists = SI.static_intervals(acc[:102], [1.0])   # two centres, the interval still open at the end
    assert [tuple(x) for x in lists[0]] == [(50, 51)]


def test_eval_acc_matches_restatement(rec200):
    t, tel, truth = rec200
    samples = tel["accelerometer"][::7][:3600]
    for p in (np.r_[0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.05, -0.02, 0.1], np.r_[truth["acc_params"]] * 1.01):
        d = SI.eval_acc(samples, p, G)
        r, J = R.acc_rows(samples, p, G)
        np.testing.assert_allclose(d["r"], r, rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(d["J"], J, rtol=1e-13, atol=1e-15)
        c, H, g = R.normal_eq(r, J)
        assert abs(d["cost"] - c) <= 1e-12 * c
        np.testing.assert_allclose(d["gradient"], g, rtol=1e-12, atol=1e-12 * np.abs(g).max())
        np.testing.assert_allclose(d["gram"], H, rtol=1e-12, atol=1e-12 * np.abs(H).max())


@pytest.mark.parametrize("optimize_bias", [False, True])
def test_eval_gyro_matches_restatement(ref200, rec200, optimize_bias):
    t, tel, truth = rec200
    ranges, gv, gw = ref200["gyro_ranges"], ref200["gyro_versors"], ref200["gyro_samples"]
    p = np.r_[1e-3, -2e-3, 5e-4, 1e-3, -1e-3, 2e-3, 0.99, 1.01, 1.005, 1e-3, -2e-3, 3e-3]
    d = SI.eval_gyro(t, gw, ranges, gv, p, optimize_bias=optimize_bias)
    r, J = R.gyro_blocks_eval(t, gw, ranges, gv, p, optimize_bias)
    assert J.shape == d["J"].shape == (3 * len(ranges), 12 if optimize_bias else 9)
    np.testing.assert_allclose(d["r"], r, rtol=0, atol=1e-11)
    np.testing.assert_allclose(d["J"], J, rtol=0, atol=1e-11)
    c, H, g = R.normal_eq(r, J)
    assert abs(d["cost"] - c) <= 1e-9 * c + 1e-15


def test_eval_gyro_long_blocks_1khz():
    t, tel, _ = _recording(rate=1000.0, num_poses=4, move_s=5.0, hold_s=2.0, seed=9)
    gw = tel["gyroscope"] - tel["gyroscope"][:100].mean(axis=0)
    ranges = [(14000, 14200), (14000, 19000), (21000, 23500), (100, 99), (5, 6)]
    rng = np.random.RandomState(1)
    gv = rng.standard_normal((len(ranges), 6))
    for p in (np.r_[0, 0, 0, 0, 0, 0, 1.0, 1.0, 1.0, 0, 0, 0], np.r_[2e-3, -1e-3, 1e-3, -2e-3, 1e-3, 2e-3, 0.99, 1.007, 1.012, 1e-3, 0, -1e-3]):
        for ob in (False, True):
            d = SI.eval_gyro(t, gw, ranges, gv, p, optimize_bias=ob)
            r, J = R.gyro_blocks_eval(t, gw, ranges, gv, p, ob)
            np.testing.assert_allclose(d["r"], r, rtol=0, atol=1e-11)
            np.testing.assert_allclose(d["J"], J, rtol=0, atol=1e-11)


def _calibrate(t, tel, **kw):
    cal = SI.StaticImuCalibrator()
    cal.SetGravityMagnitude(G)
    cal.SetInitStaticIntervalDuration(10.0)
    for k, v in kw.items():
        getattr(cal, k)(v)
    ok = cal.CalibrateAccGyro(t, tel["accelerometer"], tel["gyroscope"])
    return ok, cal


def test_calibration_matches_restatement(rec200, ref200):
    t, tel, truth = rec200
    ok, cal = _calibrate(t, tel)
    assert ok and cal.status == 0
    rep = cal.report
    assert rep["th_mult"] == ref200["th_mult"]
    assert rep["num_intervals"] == [p["num"] for p in ref200["per_threshold"]]
    assert rep["acc_iterations"] == [p["iterations"] for p in ref200["per_threshold"]]
    assert rep["acc_termination"] == [p["termination"] for p in ref200["per_threshold"]]
    for k, p in enumerate(ref200["per_threshold"]):
        if p["termination"] != R.TERM_SKIPPED:
            assert abs(rep["acc_final_cost"][k] - p["cost"]) <= 1e-9 * p["cost"]
    np.testing.assert_allclose(cal.acc_params, ref200["acc_params"], rtol=1e-9, atol=1e-12)
    assert rep["gyro_iterations"] == ref200["gyro_iterations"] and rep["gyro_termination"] == ref200["gyro_termination"]
    assert rep["gyro_num_blocks"] == len(ref200["gyro_ranges"])
    np.testing.assert_allclose(cal.gyro_params, ref200["gyro_params"], rtol=1e-9, atol=1e-12)
    assert rep["norm_th"] == ref200["norm_th"]
    np.testing.assert_array_equal(rep["init_acc_bias"], ref200["init_acc_bias"])


def test_truth_recovered_on_noisy_data(rec200):
    t, tel, truth = rec200
    ok, cal = _calibrate(t, tel, EnableGyroBiasOptimization=True)
    assert ok
    # Accelerometer: ~3600 samples of white noise sigma_a; nine parameters each carry ~sigma_a / sqrt(N / 9) per unit of
    # sensitivity (scales and misalignments relative to g), so 10x that bounds the error.
    n_used = 100 * cal.report["num_intervals"][cal.report["th_mult"] - 1]
    sa = truth["acc_noise"] / np.sqrt(n_used / 9.0)
    err = cal.acc_params - truth["acc_params"]
    assert np.all(np.abs(err[:6]) < 10 * sa / G) and np.all(np.abs(err[6:]) < 10 * sa * 3), err
    # Gyroscope: the gravity versors carry sigma_a / (g sqrt(n_hold)) each; the integrated rotation adds
    # sigma_g sqrt(move_s / rate) rad; the 36 blocks average both.  The bias term is bounded by the versor error over
    # the move time.
    sg = truth["acc_noise"] / (G * np.sqrt(truth["n_hold"])) + truth["gyro_noise"] * np.sqrt(truth["n_move"]) / truth["rate"]
    errg = cal.gyro_params - truth["gyro_params"]
    assert np.all(np.abs(errg[:9]) < 10 * sg), errg
    assert np.all(np.abs(errg[9:]) < 10 * sg / (truth["n_move"] / truth["rate"])), errg


def test_too_few_poses_fails_and_cli_writes_defaults(tmp_path):
    t, tel, _ = _recording(num_poses=8, seed=4)
    ok, cal = _calibrate(t, tel)
    assert not ok and cal.status == SI.ACC_IMPOSSIBLE and cal.report["th_mult"] == -1
    assert all(k < 12 for k in cal.report["num_intervals"])
    path = str(tmp_path / "tel.json")
    io_files.write_telemetry_json(path, tel["timestamps_ns"], tel["accelerometer"], tel["gyroscope"])
    out = str(tmp_path / "intr.json")
    r = subprocess.run([CLI, "--telemetry_json", path, "--output_calibration_path", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Failed to calibra accelerometer" in r.stderr
    d = json.load(open(out))
    assert d["accelerometer"]["misalignment_matrix"] == [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    assert d["gyroscope"]["scale_matrix"] == [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    assert d["accelerometer"]["bias"] == [0, 0, 0] and d["gyroscope"]["bias"] == [0, 0, 0]


def test_repeated_calls_bitwise_identical(rec200):
    t, tel, _ = rec200
    a = _calibrate(t, tel)[1]
    b = _calibrate(t, tel)[1]
    np.testing.assert_array_equal(a.acc_params, b.acc_params)
    np.testing.assert_array_equal(a.gyro_params, b.gyro_params)
    ra, rb = dict(a.report), dict(b.report)
    for k in ("ms_detector", "ms_acc", "ms_gyro"):
        ra.pop(k); rb.pop(k)
    assert json.dumps(ra) == json.dumps(rb)
    x = SI.static_intervals(tel["accelerometer"], np.arange(1, 11) * 1e-4, with_norms=True)
    y = SI.static_intervals(tel["accelerometer"], np.arange(1, 11) * 1e-4, with_norms=True)
    np.testing.assert_array_equal(x[1], y[1])
    assert all(np.array_equal(u, v) for u, v in zip(x[0], y[0]))


def test_cli_equals_python_mirror_and_feeds_the_main_solve(tmp_path, rec200):
    t, tel, _ = rec200
    path = str(tmp_path / "tel.json")
    io_files.write_telemetry_json(path, tel["timestamps_ns"], tel["accelerometer"], tel["gyroscope"])
    out_c, out_p = str(tmp_path / "c.json"), str(tmp_path / "p.json")
    r = subprocess.run([CLI, "--telemetry_json", path, "--output_calibration_path", out_c, "--verbose"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0].startswith("Accelerometers calibration: calibrating...Setting initial accelerometer bias: ")
    assert any(x.startswith("Gyroscopes calibration: residual ") for x in lines)
    assert "Accelerometer misalignment matrix: " in lines and "Gyroscope inverse scale factors: " in r.stdout
    SI.main(["--telemetry_json", path, "--output_calibration_path", out_p])
    assert json.load(open(out_c)) == json.load(open(out_p))
    ds = synthetic.make_config("tiny")
    files = io_files.write_dataset_files(ds, str(tmp_path / "ds"))
    main = os.path.join(ROOT, "openimucameracalibrator_amd", "csrc", "continuous_time_imu_to_camera_calibration")
    args = [main, "--dry_run", "--imu_intrinsics", out_c]
    for k, v in files.items():
        args += ["--" + k, v]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
