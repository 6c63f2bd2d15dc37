"""CPU checks of the IMU noise characterisation (fit_allan_variance): the factor list against the reference-shaped
restatement, the noise-model fit (exact data, SciPy's optimum, the accelerometer's checkData, the findMin quirk), the
C-ABI surface without a device and the C++ application's command line."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import allan_restatement as R
from openimucameracalibrator_amd import _abi, _lib, allan as A, io_files, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "openimucameracalibrator_amd", "csrc", "fit_allan_variance")


@pytest.mark.parametrize("n", [1000, 20000, 16384, 131072, 1048576, 1440000, 2880000])
def test_factor_list_matches_the_restatement(n):
    got = A.allan_factors(n, 10000)
    np.testing.assert_array_equal(got, R.factors(n, 10000))


def test_factor_counts_and_last_factors():
    f = A.allan_factors(20000)
    assert len(f) == 3328 and f[-2:].tolist() == [8185, 8193]
    f = A.allan_factors(1440000)
    assert len(f) == 5723 and f[-2:].tolist() == [523598, 524288]
    assert len(A.allan_factors(2880000)) == 5974
    # the last factor can be maxStride + 1: no term is left for it within 2 of a power of two
    assert 16384 - 2 * A.allan_factors(16384)[-1] < 0
    assert 1048576 - 2 * A.allan_factors(1048576)[-1] == 0


TAUS = R.factors(1440000) * 0.005


@pytest.mark.parametrize("kind", [A.GYRO, A.ACC])
@pytest.mark.parametrize("p", [(0.3, 10.0, 2.0, 0.05, 0.001), (0.02, 0.9, 0.1, 3e-3, 2e-5)])
def test_fit_recovers_exact_parameters(kind, p):
    p = np.array(p)
    s2 = R.model_sigma2(p, TAUS)
    f = A.allan_fit(kind, TAUS, s2, 200.0)
    np.testing.assert_allclose(np.abs(f["params"]), p, rtol=1e-4)


def check_data(taus, s2):
    """FitAllanAcc::checkData (fitallan_acc.cc:120-139)."""
    keep, mx = [], 0.0
    for i, (t, s) in enumerate(zip(taus, s2)):
        if t < 1 and mx < s:
            mx = s
            continue
        keep.append(i)
    return np.array(keep)


@pytest.fixture(scope="module")
def stationary_sigma2():
    """n = 60 000 (300 s at 200 Hz) with a strong rate random walk, so that every term of the model is determined and the
    optimum is a proper minimum (with a weak one the 50-iteration DOGLEG run of the reference can stop short of it)."""
    out = {}
    for name, seed in (("gyr", 1), ("acc", 3)):
        tel, truth = synthetic.make_stationary_imu(duration=300.0, rate=200.0, gyro_rrw=2e-3, accel_rrw=3e-2, seed=seed)
        t = tel["timestamps_ns"] * 1e-9
        freq, period = R.host_values(t)
        fac = R.factors(len(t))
        w = tel["gyroscope"][:, 0] * A.GYRO_SCALE if name == "gyr" else tel["accelerometer"][:, 0]
        out[name] = (fac * period, R.variance(R.thetas(w, freq), period, fac), freq)
    return out


@pytest.mark.parametrize("name", ["gyr", "acc"])
def test_fit_matches_scipy_least_squares(stationary_sigma2, name):
    from scipy.optimize import least_squares
    taus, s2, freq = stationary_sigma2[name]
    kind = A.GYRO if name == "gyr" else A.ACC
    f = A.allan_fit(kind, taus, s2, freq)
    keep = check_data(taus, s2) if kind == A.ACC else np.arange(len(taus))
    assert f["num_used"] == len(keep)
    t, s = taus[keep], s2[keep]

    def res(p):
        return np.log(R.model_sigma2(p, t)) / np.log(10) - np.log(s) / np.log(10)

    x0 = np.abs(f["init"])
    ref = least_squares(res, x0, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=100000)
    cost_ref = 0.5 * np.dot(ref.fun, ref.fun)
    assert f["cost"] <= cost_ref * (1 + 1e-6), (f["cost"], cost_ref)
    unit = A.GYRO_SCALE if kind == A.GYRO else 1.0
    dev = np.sqrt(R.model_sigma2(ref.x, t))
    assert f["bias_instability"] == pytest.approx(min(1000.0, dev.min()) / unit, rel=1e-3)
    assert f["white_noise"] == pytest.approx(np.sqrt(freq) * np.sqrt(R.model_sigma2(ref.x, 1.0)) / unit, rel=1e-3)


def test_accelerometer_check_data_drops_rising_points_below_one_second():
    taus = np.concatenate([np.linspace(0.01, 0.9, 40), np.linspace(1.0, 500.0, 60)])
    p = np.array([0.01, 0.05, 0.002, 1e-4, 1e-6])
    s2 = R.model_sigma2(p, taus)
    s2[[3, 10, 11, 25]] *= [50.0, 80.0, 90.0, 200.0]      # spikes below 1 s raise the running maximum
    s2[70] *= 300.0                                        # above 1 s nothing is filtered
    keep = check_data(taus, s2)
    # the running maximum starts at 0 (the first point goes) and only the first spike exceeds it; later, smaller spikes stay
    assert sorted(set(range(len(taus))) - set(keep.tolist())) == [0, 3]
    acc = A.allan_fit(A.ACC, taus, s2, 100.0)
    gyr = A.allan_fit(A.GYRO, taus[keep], s2[keep], 100.0)   # the gyroscope fit filters nothing
    assert acc["num_used"] == len(keep) and gyr["num_used"] == len(keep)
    np.testing.assert_array_equal(acc["params"], gyr["params"])
    np.testing.assert_array_equal(acc["init"], gyr["init"])


def test_find_min_starts_at_1000():
    """findMinNum / findMinIndex start from 1000.0: a model deviation above 1000 everywhere reports 1000 at taus[0]."""
    p = np.array([0.0, 3000.0, 2000.0, 100.0, 0.5])
    taus = TAUS[:3000]
    for kind, unit in ((A.GYRO, A.GYRO_SCALE), (A.ACC, 1.0)):
        f = A.allan_fit(kind, taus, R.model_sigma2(p, taus), 200.0)
        assert f["bias_instability"] == 1000.0 / unit
        assert f["tau_at_min"] == (taus[0] if kind == A.GYRO else taus[1])   # checkData dropped the accelerometer's first point
    q = np.array([0.0, 30.0, 20.0, 1.0, 0.005])              # below 1000 the true minimum is found
    f = A.allan_fit(A.GYRO, taus, R.model_sigma2(q, taus), 200.0)
    dev = np.sqrt(R.model_sigma2(np.abs(f["params"]), taus))
    assert f["bias_instability"] == dev.min() / A.GYRO_SCALE and f["tau_at_min"] == taus[int(np.argmin(dev))]


def test_fit_leaves_out_points_without_terms():
    p = np.array([0.3, 10.0, 2.0, 0.05, 0.001])
    s2 = R.model_sigma2(p, TAUS)
    s2[-1] = np.nan
    f = A.allan_fit(A.GYRO, TAUS, s2, 200.0)
    assert f["num_used"] == len(TAUS) - 1
    np.testing.assert_allclose(np.abs(f["params"]), p, rtol=1e-4)


def _variance_call(b, n, t):
    w = np.zeros((6, n)); sc = np.ones(6)
    fac = np.zeros(100, dtype=np.int32); taus = np.zeros(100); s2 = np.zeros(600); mean = np.zeros(6)
    nf, fr, pe, ms = ctypes.c_int32(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    P = lambda a, t=ctypes.c_double: a.ctypes.data_as(ctypes.POINTER(t))
    return b.variance(0, 6, n, P(w), P(np.ascontiguousarray(t, dtype=np.float64)), P(sc), 100, ctypes.byref(nf), P(fac, ctypes.c_int32),
                      P(taus), P(s2), ctypes.byref(fr), ctypes.byref(pe), P(mean), ctypes.byref(ms))


def test_variance_argument_checks_and_no_cpu_fallback():
    b = _lib.load_allan()
    assert _variance_call(b, 4, np.arange(4.0)) == -1                    # n < 8
    assert _variance_call(b, 100, np.r_[np.arange(50.0), np.arange(50.0)]) == -1   # times not increasing
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert _variance_call(b, 100, np.arange(100.0) * 0.005) == -2        # OICC_ERR_NO_DEVICE
    with pytest.raises(RuntimeError):
        A.allan_variance(np.zeros((6, 100)), np.arange(100.0) * 0.005, np.ones(6))


def test_header_entries_exported_and_table_binds_declared_names():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "oicc_hip.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(oicc_[a-z0-9_A-Z]+)\s*\(", src))
    declared = sorted(n for n in names if n.startswith("oicc_allan_"))
    assert declared == sorted("oicc_allan_" + n for n in _abi.ALLAN_SIGNATURES)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, n) for n in declared)
    assert not set(_abi.ALLAN_SIGNATURES) & set(_abi.SIGNATURES)     # the oracle-bound table stays as it is
    _lib.load_allan()


def run_cli(*args):
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-C", os.path.dirname(CLI), "-s"])
    return subprocess.run([CLI] + list(args), capture_output=True, text=True)


def test_cli_dry_run_and_flags(tmp_path):
    tel, _ = synthetic.make_stationary_imu(duration=30.0, rate=100.0)
    path = str(tmp_path / "telemetry.json")
    io_files.write_telemetry_json(path, tel["timestamps_ns"], tel["accelerometer"], tel["gyroscope"])
    r = run_cli("--telemetry_json", path, "--dry_run")
    assert r.returncode == 0, r.stderr
    assert "Inputs: 3000 IMU samples" in r.stdout
    assert run_cli("--telemetry_json", path, "--dry_run", "--not_a_flag").returncode == 2
    r = run_cli("--telemetry_json", str(tmp_path / "missing.json"), "--dry_run")
    assert r.returncode == 1 and "Could not read" in r.stderr
    # the reference's gflags (applications/fit_allan_variance.cc) are all accepted
    src = open(os.path.join(ROOT, "openimucameracalibrator_amd", "csrc", "host", "fit_allan_variance.cpp")).read()
    table = src[src.index("Flags F("):src.index("});", src.index("Flags F("))]
    mine = set(re.findall(r'\{"(\w+)",\s*"', table))
    assert {"telemetry_json", "verbose"} <= mine
    assert mine - {"telemetry_json", "verbose"} == {"device", "dry_run", "result_output_json", "nr_clusters"}


def test_telemetry_writer_roundtrip(tmp_path):
    tel, truth = synthetic.make_stationary_imu(duration=10.0, rate=200.0, seed=3)
    path = str(tmp_path / "t.json")
    io_files.write_telemetry_json(path, tel["timestamps_ns"], tel["accelerometer"], tel["gyroscope"])
    d = json.load(open(path))
    assert d["timestamps_ns"][1] == 5000000 and len(d["gyroscope"]) == 2000
    np.testing.assert_array_equal(np.array(d["accelerometer"]), tel["accelerometer"])
    assert abs(np.mean(tel["gyroscope"][:, 1]) - truth["gyro_bias"][1]) < 5 * truth["gyro_white"] * np.sqrt(200.0) / np.sqrt(2000) + 1e-3
