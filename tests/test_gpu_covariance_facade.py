"""The C++ facade's covariance methods and the "covariance" object of a calibration result against the Python mirror.

tests/covariance_facade_driver.cpp is compiled against liboicc_hip into a shared library and called through ctypes on the mirror's
own problem handle (the facade wraps it), so both sides see the same parameters and measurements; with option accumulation = 1 the
Jacobian passes are bit-repeatable, so the two estimates agree far inside the 1e-9 the comparison asks.  The C++ calibration
program has no flag that writes the object (tests/test_cli.py fixes its flags); covariance_json is the code such a flag would call."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import normal_equations_cases as cases
from openimucameracalibrator_amd import synthetic, estimator as E, _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openimucameracalibrator_amd", "csrc")
_DRIVER = {}


def driver(tmp_path_factory):
    if "lib" not in _DRIVER:
        _lib.load()
        out = str(tmp_path_factory.mktemp("facade") / "libcovariance_facade_driver.so")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "covariance_facade_driver.cpp"),
                               "-L" + CSRC, "-loicc_hip", "-Wl,-rpath," + CSRC, "-o", out])
        lib = ctypes.CDLL(out)
        lib.covariance_facade_driver.restype = ctypes.c_int
        lib.covariance_facade_driver.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p]
        _DRIVER["lib"] = lib
    return _DRIVER["lib"]


def calibrator(**overrides):
    cal = E.ImuCameraCalibrator().BatchInitSpline(synthetic.make_config("tiny", **overrides))
    cal.trajectory_.SetOption("accumulation", 1)
    return cal


def close(a, b, rel=1e-9):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    return bool(np.all(np.abs(a[ok] - b[ok]) <= rel * np.abs(b[ok]).max())) if ok.any() else True


def nan(v):
    return np.array([np.nan if x is None else x for x in v], dtype=np.float64)


@pytest.mark.parametrize("flags", [cases.FLAGS1 | E.CAM_LINE_DELAY, cases.ALL], ids=["line_delay", "ALL"])
def test_facade_and_json_object_match_the_mirror(tmp_path, tmp_path_factory, flags):
    lib = driver(tmp_path_factory)
    cal = calibrator()
    tr = cal.trajectory_
    want = cal.CovarianceJson(flags)
    est = tr.EstimateCovariance(flags)
    path = str(tmp_path / "facade.json")
    assert lib.covariance_facade_driver(tr._h, int(flags), 1, path.encode()) == 0
    got = json.load(open(path))
    cv, e = got["covariance"], got["estimate"]
    # the JSON object: same keys in the same (sorted) order, same names, matrix and standard deviations to 1e-9
    assert list(cv) == sorted(want) and cv["status"] == want["status"] == "ok" and cv["scaled"] is True
    assert cv["tangent_order"] == want["tangent_order"] and all(cv["tangent_order"])
    assert close(cv["matrix"], want["matrix"])
    assert abs(cv["variance_factor"] - want["variance_factor"]) <= 1e-12 * want["variance_factor"]
    assert abs(cv["rcond"] - want["rcond"]) <= 1e-9 * want["rcond"]
    assert list(cv["std_devs"]) == sorted(want["std_devs"])
    for k, v in want["std_devs"].items():
        assert close(nan(cv["std_devs"][k]), nan(v)), k
    # the named standard deviations are sqrt(variance_factor * diagonal), in the order tangent_order names
    d = np.sqrt(cv["variance_factor"] * np.diag(np.asarray(cv["matrix"])))
    by_name = dict(zip(cv["tangent_order"], d))
    assert np.allclose(cv["std_devs"]["t_i_c_m"], [by_name["T_i_c[%d]" % k] for k in range(3)], rtol=1e-14, atol=0)
    assert np.allclose(cv["std_devs"]["q_i_c_rad"], [by_name["T_i_c[%d]" % k] for k in range(3, 6)], rtol=1e-14, atol=0)
    assert np.allclose(cv["std_devs"]["gravity"], [by_name["gravity[%d]" % k] for k in range(3)], rtol=1e-14, atol=0)
    assert np.allclose(cv["std_devs"]["line_delay_s"], [by_name["line_delay[0]"]], rtol=1e-14, atol=0)
    if flags == cases.ALL:
        assert np.allclose(cv["std_devs"]["gyro_intrinsics"], [by_name["gyro_intrinsics[%d]" % k] for k in range(9)], rtol=1e-14, atol=0)
        gb = nan(cv["std_devs"]["gyro_bias"]).reshape(-1, 3)
        for k, o in enumerate(est["layout"]["gyro_bias"]):
            assert (np.all(np.isnan(gb[k])) if o < 0 else np.allclose(gb[k], [by_name["gyro_bias[%d][%d]" % (k, c)] for c in range(3)], rtol=1e-14, atol=0))
    # EstimateCovariance of the facade: info, layout and blocks
    info, lay = est["info"], est["layout"]
    for k in ("status", "P", "Pb", "a", "hb", "num_residuals"):
        assert e[k] == info[k], k
    assert e["so3_offsets"] == list(lay["so3"]) and e["r3_offsets"] == list(lay["r3"]) and e["other_offsets"] == list(lay["other"])
    assert e["accl_bias_offsets"] == list(lay["accl_bias"]) and e["gyro_bias_offsets"] == list(lay["gyro_bias"])
    assert close(nan(e["arrow"]).reshape(info["a"], info["a"]), est["arrow"])
    assert close(nan(e["so3"]).reshape(-1, 3, 3), est["so3"]) and close(nan(e["r3"]).reshape(-1, 3, 3), est["r3"])


def test_rank_deficient_estimate_is_a_status_not_an_error(tmp_path, tmp_path_factory):
    lib = driver(tmp_path_factory)
    cal = calibrator(duration=0.3, num_views=3)
    want = cal.CovarianceJson(cases.FLAGS1)
    assert sorted(want) == ["rcond", "status"] and want["status"] == "rank_deficient" and want["rcond"] < 1e-12
    path = str(tmp_path / "facade.json")
    assert lib.covariance_facade_driver(cal.trajectory_._h, int(cases.FLAGS1), 1, path.encode()) == 0
    got = json.load(open(path))
    assert list(got["covariance"]) == ["rcond", "status"] and got["covariance"]["status"] == "rank_deficient"
    assert got["covariance"]["rcond"] < 1e-12 and got["estimate"]["status"] == 1 and got["estimate"]["arrow"] == []
