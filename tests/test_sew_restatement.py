"""CPU tests of tests/sew_restatement.py: the 50-digit restatement against closed forms, the float64 yardsticks (a fresh measurement
within [1/8, 1] of every recorded figure), planted defects of the kind a reworked launch geometry produces, and the argument checks
of the debug entry oicc_debug_sew_spectrum (refused before any device call).  The device comparison is
tests/test_gpu_sew_spectrum.py."""
import ctypes as C

import mpmath as mp
import numpy as np
import pytest

import sew_restatement as S


def test_direct_dft_against_closed_forms():
    with mp.workdps(S.DPS):
        for n in (8, 9, 16):
            j = np.arange(n)
            # a cosine on bin m: |X[m]| = n A / 2, mirrored bin counted by the multiplicity; nothing elsewhere
            m = 3
            pw, P = S.spectrum(0.75 * np.cos(2 * np.pi * m * j / n + 0.3))
            want = 2 * (mp.mpf(n) * mp.mpf(0.75) / 2) ** 2
            assert abs(pw[m] - want) <= 1e-14 * want            # (the cosine itself is a float64 evaluation)
            assert all(abs(pw[k]) <= 1e-28 * want for k in range(len(pw)) if k != m) and P == pw[m]
            # Parseval on exact inputs: sum_k pw[k] + |X[0]|^2 = n sum x^2, to the working precision
            x = np.random.default_rng(n).standard_normal((2, n))
            pw, P = S.spectrum(x)
            dc = sum(mp.fsum(mp.mpf(float(v)) for v in row) ** 2 for row in x) / 2
            total = n * mp.fsum(mp.mpf(float(v)) ** 2 for v in x.ravel()) / 2
            assert abs(mp.fsum(pw) + dc - total) <= mp.mpf(10) ** -45 * total
        # the Nyquist bin of an even length appears once: x = (-1)^j has X[n/2] = n
        pw, _ = S.spectrum(np.array([1.0, -1.0] * 8))
        assert pw[8] == 256 and S.multiplicity(8, 16) == 1 and S.multiplicity(8, 17) == 2 and S.multiplicity(0, 9) == 1
        # response: unit DC gain, exact zeros at integer f dt, the known value at x = 1/2
        assert S.response(0, 512, 256.0, 0.25) == 1
        assert S.response(8, 512, 256.0, 0.25) == 0 and S.response(16, 512, 256.0, 0.25) == 0
        assert abs(S.response(4, 512, 256.0, 0.25) - 3 * (2 / mp.pi) ** 4) <= mp.mpf(10) ** -45


def test_cases_reach_the_edges():
    shapes = {name: np.atleast_2d(sig).shape for name, (sig, _, _) in S.CASES.items()}
    assert {n for _, n in shapes.values()} == {8, 9, 16, 510, 511, 512, 513, 521, 1031}
    assert {d for d, _ in shapes.values()} == {1, 3}
    assert sorted(shapes[c][1] // 2 + 1 for c in S.GRID_CAP_CASES) == [257, 257, 261, 261]
    assert [shapes[c] for c in S.PLAN_SEQUENCE] == [(3, 512), (3, 513), (1, 512), (3, 512)]
    sig, rate, dts = S.CASES["n512_d3"]
    assert ("integer", 0.25) in dts and all(float(k * (rate / 512) * 0.25) == k / 8 for k in range(257))
    assert abs(S.CASES["n521_d3_gravity"][0][1].mean() - 9.81) < 0.1
    for name, (sig, rate, dts) in S.CASES.items():
        n = shapes[name][1]
        assert [c for c, _ in dts][:3] == ["sample", "max", "fine"] and dts[0][1] == 1.0 / rate and dts[1][1] == (n / 4.0) / rate and dts[2][1] == 1e-4


def test_float64_yardsticks(capsys):
    worst = S.measure_yardsticks()
    with capsys.disabled():
        print("\nSEW float64 yardsticks (measured / recorded): " + ", ".join("%s %.2e / %.0e" % (k, v, S.YARDSTICK[k]) for k, v in sorted(worst.items())))
    assert set(worst) == set(S.YARDSTICK)
    for k, v in worst.items():
        assert S.YARDSTICK[k] / 8 <= v <= S.YARDSTICK[k], (k, v)


@pytest.mark.parametrize("name", ["n512_d3", "n521_d1", "n9_d3"])
def test_planted_defects_are_caught(name):
    """What a wrong power kernel or reduction would hand back, planted on the float64 evaluation: each exceeds the device bound."""
    sig, rate, dts = S.CASES[name]
    n = np.atleast_2d(sig).shape[1]
    dl = [dt for _, dt in dts]
    pw, sums = S.float64_evaluation(sig, rate, dl)

    def exceeds(e):
        return any(v > S.DEVICE_FACTOR * S.YARDSTICK[k] for k, v in e.items())
    assert not exceeds(S.errors(name, pw, sums))
    bad = pw.copy(); bad[-1] *= 2.0 if n % 2 == 0 else 0.5                    # the Nyquist bin counted twice / the last bin of an odd length once
    assert S.errors(name, bad, sums)["pw"] > 1e6 * S.DEVICE_FACTOR * S.YARDSTICK["pw"]
    fr = np.fft.rfftfreq(n, d=1.0 / rate)
    short = np.array([[np.sum(pw[:-1]), np.sum(pw[:-1] * (1.0 - S.sew_oracle.interpolation_response(fr[:-1], dt)) ** 2)] for dt in dl])
    assert exceeds(S.errors(name, pw, short))                                 # the last bin left out of the reduction
    first = np.array([[np.sum(pw[:256]), np.sum(pw[:256] * (1.0 - S.sew_oracle.interpolation_response(fr[:256], dt)) ** 2)] for dt in dl])
    if len(pw) > 256:
        assert exceeds(S.errors(name, pw, first))                             # only the first block's bins summed


def test_debug_entry_refuses_bad_arguments():
    """oicc_debug_sew_spectrum answers OICC_ERR_INVALID_ARG (-1) before it touches a device."""
    from openimucameracalibrator_amd import _lib
    fn = _lib.load().lib.oicc_debug_sew_spectrum
    dp = C.POINTER(C.c_double)
    fn.restype = C.c_int
    fn.argtypes = [C.c_int32, C.c_int32, C.c_int64, dp, C.c_double, C.c_int32, dp, C.c_int32, dp, dp]
    sig = np.zeros(16); dts = np.array([0.01]); pw = np.zeros(9); sums = np.zeros(2)

    def call(dims=1, n=16, signal=sig, rate=256.0, num_dt=1, dt=dts, cap=0, pw_out=pw, sums_out=sums):
        p = [None if a is None else a.ctypes.data_as(dp) for a in (signal, dt, pw_out, sums_out)]
        return fn(0, dims, n, p[0], rate, num_dt, p[1], cap, p[2], p[3])
    assert call(n=7) == -1 and call(dims=0) == -1 and call(signal=None) == -1 and call(pw_out=None) == -1
    assert call(rate=0.0) == -1 and call(rate=float("nan")) == -1 and call(rate=float("inf")) == -1
    assert call(num_dt=-1) == -1 and call(dt=None) == -1 and call(sums_out=None) == -1 and call(cap=-1) == -1
    assert call(dt=np.array([0.0])) == -1 and call(dt=np.array([-0.1])) == -1 and call(dt=np.array([float("nan")])) == -1
    assert call(n=2 ** 31) == -1
