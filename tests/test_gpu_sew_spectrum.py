"""The device's spectral quantities of the spline-error-weighting pre-stage (csrc/sew.hip: hipFFT, sew_power_kernel,
sew_reduce_kernel) against the 50-digit restatement tests/sew_restatement.py, through the debug entry oicc_debug_sew_spectrum --
the same SewSpectrum object the calibration entry drives.  Bound: DEVICE_FACTOR (64) x the float64 yardstick of each class, on the
natural scale of each quantity (sew_restatement's docstring).  The end-to-end tests (tests/test_sew.py) see these kernels only
through Brent's root at 1e-9; here every bin and every sum is compared at the edges: the minimum length, odd / even Nyquist
multiplicity, bin counts on a block boundary, primes, DC leakage, the grid-stride loop (grid_cap 1 / 2), the plan cache's rebuild."""
import ctypes as C

import numpy as np
import pytest

import sew_restatement as S

DP = C.POINTER(C.c_double)


def device_spectrum(name, grid_cap=0):
    """pw [nh], sums [num_dt, 2] of a case from the device."""
    from openimucameracalibrator_amd import _lib
    fn = _lib.load().lib.oicc_debug_sew_spectrum
    fn.restype = C.c_int
    fn.argtypes = [C.c_int32, C.c_int32, C.c_int64, DP, C.c_double, C.c_int32, DP, C.c_int32, DP, DP]
    sig, rate, dts = S.CASES[name]
    sig = np.ascontiguousarray(np.atleast_2d(sig), dtype=np.float64)
    dims, n = sig.shape
    dl = np.array([dt for _, dt in dts], dtype=np.float64)
    pw = np.full(n // 2 + 1, np.nan); sums = np.full((len(dl), 2), np.nan)
    rc = fn(0, dims, n, sig.ctypes.data_as(DP), rate, len(dl), dl.ctypes.data_as(DP), grid_cap, pw.ctypes.data_as(DP), sums.ctypes.data_as(DP))
    assert rc == 0, rc
    return pw, sums


def check(name, grid_cap, capsys):
    pw, sums = device_spectrum(name, grid_cap)
    e = S.errors(name, pw, sums)
    ratios = {k: v / S.YARDSTICK[k] for k, v in e.items()}
    with capsys.disabled():
        print("\n  %s cap %d: " % (name, grid_cap) + ", ".join("%s %.2e (%.1f x)" % (k, e[k], ratios[k]) for k in sorted(e)))
    for k, r in ratios.items():
        assert r <= S.DEVICE_FACTOR, (name, grid_cap, k, e[k], S.YARDSTICK[k])
    return pw, sums


@pytest.mark.gpu
@pytest.mark.parametrize("name,grid_cap", [(n, 0) for n in sorted(S.CASES)] + [(n, c) for n in S.GRID_CAP_CASES for c in (1, 2)])
def test_spectrum_and_sums_against_the_restatement(name, grid_cap, capsys):
    check(name, grid_cap, capsys)


@pytest.mark.gpu
def test_plan_cache_is_rebuilt_between_shapes(capsys):
    """(512, 3) -> (513, 3) -> (512, 1) -> (512, 3) in one process: every call meets the restatement, the last equals the first."""
    got = [check(name, 0, capsys) for name in S.PLAN_SEQUENCE]
    assert np.array_equal(got[0][0], got[3][0])


@pytest.mark.gpu
def test_calibration_entry_runs_the_same_sums():
    """oicc_sew_knot_spacing_and_variance reports variance = removed(dt) / n / n at the spacing it found: the debug entry's raw sum
    at that spacing gives the same number bit for bit (one code path behind both doors)."""
    from openimucameracalibrator_amd import _lib, sew
    fn = _lib.load().lib.oicc_debug_sew_spectrum
    fn.restype = C.c_int
    fn.argtypes = [C.c_int32, C.c_int32, C.c_int64, DP, C.c_double, C.c_int32, DP, C.c_int32, DP, DP]
    for name in ("n513_d3", "n512_d1"):
        sig, rate, _ = S.CASES[name]
        sig = np.ascontiguousarray(np.atleast_2d(sig)); dims, n = sig.shape
        t = np.arange(n) / rate
        dt, var = sew.knot_spacing_and_variance(sig if dims > 1 else sig[0], t, 0.9)
        span = t[-1] - t[0]
        dl = np.array([dt]); pw = np.zeros(n // 2 + 1); sums = np.zeros(2)
        assert fn(0, dims, n, sig.ctypes.data_as(DP), float(n - 1) / span, 1, dl.ctypes.data_as(DP), 0, pw.ctypes.data_as(DP), sums.ctypes.data_as(DP)) == 0
        assert sums[1] / float(n) / float(n) == var, (name, sums[1] / n / n, var)
