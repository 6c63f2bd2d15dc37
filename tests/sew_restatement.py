"""50-digit restatement of the spectral quantities of the spline-error-weighting pre-stage (python/sew.py of the reference:
make_reference_spectrum :170-179, bspline_interp_freq_func / spline_interpolation_response :35-76, signal_energy :79-80), the
quantities the device forms in csrc/sew.hip before the scalar search sees them: the power of the half spectrum and, per trial knot
spacing, the two sums of the spectral reduction.  Written from the reference's text as a function of the exact float64 inputs:

    X_axis[k] = sum_j x_axis[j] exp(-2 pi i (j k mod n) / n)           a direct DFT, the index reduced in integers; no FFT
    pw[k]     = w_k / dims * sum_axes |X_axis[k]|^2,   k = 0 .. n/2    w_k = 1 for DC and the Nyquist bin of an even n, else 2
    pw[0]     = 0                                                      (DC removed, sew.py:177)
    H(x)      = 3 sinc(x)^4 / (2 + cos 2 pi x),  x = k (rate / n) dt   formed exactly (sinc(x) = sin(pi x) / (pi x))
    sums      = sum_k pw[k],  sum_k pw[k] (1 - H)^2                    (n x sew.py's signal_energy of Xhat and of (1 - H) Xhat)

Error measures (the natural scale of each quantity):
    pw[k]   |pw - ref| / sqrt(ref[k] P), P the largest w_k / dims sum |X|^2 over all bins, DC included before it is zeroed: the
            rounding error of a transform in one bin is relative to the whole signal, not to that bin (d|X|^2 = 2 |X| d|X|);
    sums    relative to the sum (every term is >= 0).

Yardsticks: the error of a plain float64 evaluation (numpy.fft.rfft and the formulas of oracle/sew_oracle.py) against the
restatement, the largest over the cases of a class, rounded up to one digit -- YARDSTICK below; tests/test_sew_restatement.py
asserts that a fresh measurement lies within [1/8, 1] of every figure.  The device is allowed DEVICE_FACTOR (64) x the figure.
Classes: 'pw'; 'energy' (sum pw); the removed-energy sum per kind of knot spacing -- 'sample' (1 / rate), 'integer' (f dt an
exact integer on every eighth bin), 'max' (the default max_dt = n / (4 rate)), 'fine' (1e-4: 1 - H cancels to ~x^4).

Measured float64 figures: pw 4.9e-16, energy 5.5e-16, sample 1.4e-14, integer 2.7e-16, max 4.6e-16, fine 2.1e-7 (YARDSTICK below).
Worst device error on an MI355X, as a multiple of the yardstick (allowed: 64): pw 1.3, energy 1.1, sample 1.2, integer 0.3, max 1.1,
fine 0.8 (DEVICE_OBSERVED below; hipFFT and the two kernels are as accurate as numpy's transform and a float64 sum).
"""
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import sew_oracle  # noqa: E402

DPS = 50
DEVICE_FACTOR = 64          # the project's factor (tests/normal_equations_reference.py)

# float64 evaluation against the restatement, largest over the cases of the class, rounded up to one digit
#   measured: pw 4.9e-16, energy 5.5e-16, sample 1.4e-14, integer 2.7e-16, max 4.6e-16, fine 2.1e-7
YARDSTICK = {"pw": 5e-16, "energy": 6e-16, "sample": 2e-14, "integer": 3e-16, "max": 5e-16, "fine": 3e-7}
# worst device error / yardstick seen on an MI355X (allowed: DEVICE_FACTOR)
DEVICE_OBSERVED = {"pw": 1.3, "energy": 1.1, "sample": 1.2, "integer": 0.3, "max": 1.1, "fine": 0.8}


def _signal(n, rate, seed, dims, mean=None):
    """Band-limited hand-held-like motion + white noise; `mean`: a constant added per axis (gravity on one axis: DC leakage)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    sig = np.zeros((dims, n))
    for a in range(dims):
        for _ in range(5):
            f = rng.uniform(0.02, 0.45) * rate * min(1.0, 64.0 / n)
            sig[a] += rng.uniform(0.1, 1.0) * np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi))
        sig[a] += 0.05 * rng.standard_normal(n)
        if mean is not None:
            sig[a] += mean[a]
    return sig


def _dts(n, rate, extra=()):
    """(class, dt) of a case: 1 / rate, the default max_dt, 1e-4, and the extras."""
    return [("sample", 1.0 / rate), ("max", (n / 4.0) / rate), ("fine", 1e-4)] + list(extra)


def _cases():
    """name -> (signal [dims, n], rate, [(class, dt)]).  The smallest lengths that reach the edges: the minimum n = 8, odd / even
    Nyquist multiplicity, bin counts on a block boundary (nh = 256 / 257), small primes, DC leakage."""
    out = {}
    for n, dims, rate, seed in ((8, 1, 256.0, 1), (9, 3, 256.0, 2), (16, 1, 200.0, 3), (510, 3, 256.0, 4), (511, 1, 200.0, 5),
                                (512, 3, 256.0, 6), (512, 1, 256.0, 7), (513, 3, 256.0, 8), (521, 1, 256.0, 9), (1031, 1, 200.0, 10)):
        extra = [("integer", 0.25)] if n == 512 else []          # f dt = k (256 / 512) 0.25 = k / 8
        out["n%d_d%d" % (n, dims)] = (_signal(n, rate, seed, dims), rate, _dts(n, rate, extra))
    out["n521_d3_gravity"] = (_signal(521, 256.0, 11, 3, mean=(0.0, 9.81, 0.0)), 256.0, _dts(521, 256.0))
    return out


CASES = _cases()
GRID_CAP_CASES = ("n512_d3", "n513_d3", "n521_d1", "n521_d3_gravity")     # nh = 257, 257, 261, 261
PLAN_SEQUENCE = ("n512_d3", "n513_d3", "n512_d1", "n512_d3")              # (n, dims) changes between the calls: the plan is rebuilt


def multiplicity(k, n):
    return 1 if k == 0 or 2 * k == n else 2


def spectrum(signal):
    """pw [n/2 + 1] (mpf) and P of a signal [dims, n] of float64."""
    sig = np.atleast_2d(np.asarray(signal, dtype=np.float64))
    dims, n = sig.shape
    nh = n // 2 + 1
    with mp.workdps(DPS):
        c = [mp.cospi(mp.mpf(2 * m) / n) for m in range(n)]
        s = [-mp.sinpi(mp.mpf(2 * m) / n) for m in range(n)]
        x = [[mp.mpf(float(v)) for v in sig[a]] for a in range(dims)]
        full = []
        for k in range(nh):
            idx = [(j * k) % n for j in range(n)]
            ck = [c[m] for m in idx]; sk = [s[m] for m in idx]
            tot = mp.mpf(0)
            for a in range(dims):
                re = mp.fdot(x[a], ck); im = mp.fdot(x[a], sk)
                tot += re * re + im * im
            full.append(multiplicity(k, n) * tot / dims)
        P = max(full)
        return [mp.mpf(0)] + full[1:], P


def response(k, n, rate, dt):
    """H at bin k: x = k (rate / n) dt from the exact float64 rate and dt."""
    with mp.workdps(DPS):
        x = k * (mp.mpf(float(rate)) / n) * mp.mpf(float(dt))
        sinc = mp.mpf(1) if x == 0 else mp.sinpi(x) / (mp.pi * x)
        return 3 * sinc ** 4 / (2 + mp.cospi(2 * x))


def sums(pw, n, rate, dt):
    with mp.workdps(DPS):
        e = mp.fsum(pw)
        r = mp.fsum(p * (1 - response(k, n, rate, dt)) ** 2 for k, p in enumerate(pw))
        return e, r


_CACHE = {}


def restated(name):
    """(pw, P, {dt: (sum pw, sum pw (1 - H)^2)}) of a case, computed once per process."""
    if name not in _CACHE:
        sig, rate, dts = CASES[name]
        n = np.atleast_2d(sig).shape[1]
        pw, P = spectrum(sig)
        _CACHE[name] = (pw, P, {dt: sums(pw, n, rate, dt) for _, dt in dts})
    return _CACHE[name]


def float64_evaluation(signal, rate, dts):
    """numpy.fft.rfft and the formulas of oracle/sew_oracle.py: pw [nh], sums [len(dts), 2]."""
    sig = np.atleast_2d(np.asarray(signal, dtype=np.float64))
    dims, n = sig.shape
    spec = np.fft.rfft(sig, axis=1)
    w = np.array([multiplicity(k, n) for k in range(n // 2 + 1)], dtype=np.float64)
    pw = w * np.sum(np.abs(spec) ** 2, axis=0) / dims
    pw[0] = 0.0
    freqs = np.fft.rfftfreq(n, d=1.0 / rate)
    out = np.array([[np.sum(pw), np.sum(pw * (1.0 - sew_oracle.interpolation_response(freqs, dt)) ** 2)] for dt in dts])
    return pw, out


def pw_error(pw, pw_ref, P):
    """max_k |pw[k] - ref[k]| / sqrt(ref[k] P) over k >= 1; pw[0] must be exactly 0."""
    assert pw[0] == 0.0, "the DC bin is removed exactly"
    with mp.workdps(DPS):
        worst = mp.mpf(0)
        for k in range(1, len(pw_ref)):
            assert pw_ref[k] > 0
            worst = max(worst, abs(mp.mpf(float(pw[k])) - pw_ref[k]) / mp.sqrt(pw_ref[k] * P))
        return float(worst)


def sum_error(value, ref):
    with mp.workdps(DPS):
        return float(abs(mp.mpf(float(value)) - ref) / ref)


def errors(name, pw, sums_):
    """{class: error} of an evaluation (pw [nh], sums [num_dt, 2] in the order of the case's knot spacings) of a case."""
    sig, rate, dts = CASES[name]
    pw_ref, P, s_ref = restated(name)
    out = {"pw": pw_error(pw, pw_ref, P), "energy": 0.0}
    for (cls, dt), (e, r) in zip(dts, np.asarray(sums_)):
        out["energy"] = max(out["energy"], sum_error(e, s_ref[dt][0]))
        out[cls] = max(out.get(cls, 0.0), sum_error(r, s_ref[dt][1]))
    return out


def measure_yardsticks():
    """{class: largest float64 error over the cases}."""
    worst = {}
    for name, (sig, rate, dts) in CASES.items():
        pw, s = float64_evaluation(sig, rate, [dt for _, dt in dts])
        for cls, e in errors(name, pw, s).items():
            worst[cls] = max(worst.get(cls, 0.0), e)
    return worst
