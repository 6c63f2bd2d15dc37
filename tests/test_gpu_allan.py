"""The Allan variance on the MI355X against the reference-shaped restatement (tests/allan_restatement.py), its
repeatability, the n - 2m <= 0 deviation, the physics of a synthetic still IMU, and the C++ application against the
Python mirror."""
import json
import os
import subprocess

import numpy as np
import pytest

import allan_restatement as R
from openimucameracalibrator_amd import allan as A, io_files, synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "openimucameracalibrator_amd", "csrc", "fit_allan_variance")
SCALE = np.array([1.0, 1.0, 1.0, A.GYRO_SCALE, A.GYRO_SCALE, A.GYRO_SCALE])


def channels(duration, rate, seed, **kw):
    # gravity left out: a 9.8 m/s^2 mean makes the restatement's own running sum too coarse for a 1e-8 comparison
    # (gravity, and larger means, are tested against the exact reference in tests/test_gpu_allan_edges.py)
    tel, truth = synthetic.make_stationary_imu(duration=duration, rate=rate, seed=seed, gravity=(0.0, 0.0, 0.0), **kw)
    w = np.concatenate([tel["accelerometer"].T, tel["gyroscope"].T], axis=0)
    return w, tel["timestamps_ns"] * 1e-9, truth


def restated(w, t, fac):
    freq, period = R.host_values(t)
    out = []
    for c in range(w.shape[0]):
        th = R.thetas(w[c] * SCALE[c], freq)
        assert R.rounding_bound(th, fac) < 1e-9
        out.append(R.variance(th, period, fac))
    return np.array(out), freq, period


def test_every_factor_matches_the_restatement():
    w, t, _ = channels(1000.0, 200.0, seed=5)                     # n = 200 000
    v = A.allan_variance(w, t, SCALE)
    fac = R.factors(len(t))
    np.testing.assert_array_equal(v["factors"], fac)
    ref, freq, period = restated(w, t, fac)
    assert v["freq"] == freq and v["period"] == period
    np.testing.assert_allclose(v["sigma2"], ref, rtol=1e-8, atol=0)


def test_two_hours_at_200_hz():
    w, t, _ = channels(7200.0, 200.0, seed=6)                     # n = 1 440 000
    v = A.allan_variance(w, t, SCALE)
    fac = R.factors(len(t))
    freq, period = R.host_values(t)
    np.testing.assert_array_equal(v["factors"], fac)
    np.testing.assert_array_equal(v["taus"], fac * period)
    assert v["freq"] == freq and v["period"] == period
    np.testing.assert_array_equal(v["mean"], [R.seq_mean(w[c] * SCALE[c]) for c in range(6)])
    pick = np.unique(np.linspace(0, len(fac) - 1, 100).round().astype(int))
    assert pick[0] == 0 and pick[-1] == len(fac) - 1
    for c in range(6):
        th = R.thetas(w[c] * SCALE[c], freq)
        assert R.rounding_bound(th, fac) < 1e-9
        np.testing.assert_allclose(v["sigma2"][c, pick], R.variance(th, period, fac[pick]), rtol=1e-8, atol=0)


def test_last_factor_without_terms_is_nan_and_the_fit_succeeds():
    tel, _ = synthetic.make_stationary_imu(duration=1048576 / 200.0, rate=200.0, seed=8)
    assert len(tel["timestamps_ns"]) == 1048576
    res = A.AllanVarianceFitter(tel).RunFit()
    assert res["factors"][-1] == 524288
    for name, ax in res["axes"].items():
        assert np.isnan(ax["sigma2"][-1]) and np.isfinite(ax["sigma2"][:-1]).all()
        assert ax["fit"]["num_used"] <= len(res["factors"]) - 1 and np.isfinite(ax["fit"]["white_noise"])


def test_repeated_calls_are_bitwise_identical():
    w, t, _ = channels(600.0, 200.0, seed=9)
    a = A.allan_variance(w, t, SCALE)["sigma2"]
    b = A.allan_variance(w, t, SCALE)["sigma2"]
    assert a.tobytes() == b.tobytes()


def test_white_rate_noise_and_random_walk_physics():
    # white rate noise only: sigma2(m) = sigma_w^2 / m, scatter ~ sqrt(m / n)
    w, t, truth = channels(7200.0, 200.0, seed=12, gyro_rrw=0.0, accel_rrw=0.0)
    v = A.allan_variance(w, t, SCALE)
    n = len(t)
    m = v["factors"].astype(np.float64)
    sel = m <= n / 100
    for c in range(6):
        white = truth["accel_white"] if c < 3 else truth["gyro_white"]
        sw2 = (white * np.sqrt(truth["rate"]) * SCALE[c]) ** 2        # per-sample variance
        dev = np.abs(v["sigma2"][c, sel] * m[sel] / sw2 - 1)
        assert (dev <= 4 * np.sqrt(m[sel] / n)).all(), (c, dev.max())
    # white noise + rate random walk: sigma2(tau) = D^2 / tau + K^2 tau / 3, the two cross at tau = sqrt(3) D / K ~ 12-17 s so
    # that 2 h of data determine K.  The fit is the reference's 50-iteration DOGLEG run: on some axes of other seeds it stalls
    # on Cauchy steps short of the optimum (seed 13, acc_y: cost 66.5 where the optimum is 21.2, white noise 12 % high;
    # DESIGN.md 3.x), so this seed pins the physics, not the solver's robustness
    tel, truth = synthetic.make_stationary_imu(duration=7200.0, rate=200.0, seed=14, gyro_rrw=2e-4, accel_rrw=3e-3)
    res = A.AllanVarianceFitter(tel).RunFit()
    for name, ax in res["axes"].items():
        gyro = name.startswith("gyr")
        sc = A.GYRO_SCALE if gyro else 1.0
        D = truth["gyro_white"] if gyro else truth["accel_white"]
        K = truth["gyro_rrw"] if gyro else truth["accel_rrw"]
        p = np.abs(ax["fit"]["params"])
        assert abs(p[1] / (D * sc) - 1) <= 0.05, (name, p)
        assert abs(p[3] / (K * sc / np.sqrt(3)) - 1) <= 0.30, (name, p)


def test_cli_matches_the_python_mirror(tmp_path):
    tel, _ = synthetic.make_stationary_imu(duration=1200.0, rate=100.0, seed=14)
    path = str(tmp_path / "telemetry.json")
    io_files.write_telemetry_json(path, tel["timestamps_ns"], tel["accelerometer"], tel["gyroscope"])
    out = str(tmp_path / "allan.json")
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-C", os.path.dirname(CLI), "-s"])
    r = subprocess.run([CLI, "--telemetry_json", path, "--result_output_json", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    res = A.AllanVarianceFitter(json.load(open(path))).RunFit()
    assert json.load(open(out)) == json.loads(json.dumps(A.result_json(res)))
    lines = r.stdout.splitlines()
    pos = [lines.index(l) for l in A.result_lines(res) if l != "-------------------"]
    assert pos == sorted(pos)
