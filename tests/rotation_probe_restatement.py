"""50-digit restatement of one probe of the gyroscope-to-camera rotation search and of its host preparation
(src/core/imu_to_camera_rotation_estimator.cc of the reference: SolveClosedForm :39-114, EstimateCameraImuRotation :116-218;
src/utils/utils.cc: FindClosestTimestamp :194-212, InterpolateQuaternions :220-240, InterpolateVector3d :242-261; Eigen's
Quaternion::slerp).  Written from the reference's text as a function of the exact float64 inputs; the device path is
csrc/rotation_init.hip (rot_moments_kernel, rot_error_kernel, the host Kabsch step, prepare_rotation_series).

Probe (times ts [n], smoothed rates imu / vis [n, 3], offset td):
    shifted[j] = ts[j] - td;  k_i = the FIRST index at the minimum |ts[i] - shifted[j]|  (strict `<` in the scan: ties -> earlier)
    q_i = (1 - f) vis[k] + f vis[k + 1],  f = |ts[i] - shifted[k]| / (shifted[k + 1] - shifted[k])  -- towards k + 1 from the NEAREST
          sample, whichever side it lies on; at k + 1 == n the last sample is held (the documented deviation: the reference reads
          one element past the end there)
    moments: sum imu, sum q, sum imu q^T;  A = sum (imu - mean)(q - mean)^T = U S V^T (mp.svd_r);  R = V C U^T, C(2,2) = -1 when
          det(V U^T) < 0;  bias = mean q - R mean imu (or 0);  error = sum huber(|q_i - (R imu_i + bias)|^2), the switch on the
          SQUARED error: e > 1.345 ? 2 * 1.345 sqrt(e) - 1.345^2 : e.
Preparation: window [later start, LATER end], times zero based (that float64 subtraction is the reference's own: tI is compared
    exactly); view quaternions at the IMU times by the same nearest / towards k + 1 rule with Eigen's slerp (linear blend at
    |d| >= 1 - eps, sign flip on d < 0); rates -2 / dt vec((q_{i+1} - q_i) q_i^-1), the last difference repeated; a rate with a
    component over 2 pi takes the previous cleaned value for i > 1, otherwise zero; trailing 15-tap means.

Error measures: each moment relative to the sum of the absolute values of its terms; R and bias absolute; the error relative to the
error; sImu / sVis relative to the largest entry of the array.
Conditions (asserted per case, `check_conditions`; inputs are chosen so that they hold): restated-R cases have sigma_3 / sigma_1 >=
1e-3 (planar motion: sigma_2 / sigma_1 >= 1e-3 and sigma_3 == 0), per-axis mean^2 <= variance of both series, no squared error
within 1e-6 of the Huber threshold, a 'huber' series has 20 % .. 80 % of its samples above it (and some between 1.345 and 1.345^2);
apart from the deliberate exact ties no nearest-sample decision lies within BRANCH_MARGIN of a tie.
Where R is not unique (single-axis motion; every sample held or extrapolated from the first pair, which leaves the resampled
series constant or on one line) only the moments are restated and R is checked to be a rotation: `restate_R` False.

Yardsticks: the error of a plain float64 numpy evaluation (oracle/rotation_init_oracle.py: solve_closed_form, prepare) against
the restatement, the largest over the cases of a class, rounded up to one digit -- YARDSTICK / PREPARE_YARDSTICK below;
tests/test_rotation_probe_restatement.py asserts that a fresh measurement lies within [1/8, 1] of every figure.  The device is
allowed DEVICE_FACTOR (64) x the figure.  Classes: (series kind, edge the offset reaches).
Worst device error on an MI355X over all classes, as a multiple of the class's yardstick (allowed: 64): moments 0.7, R 1.4,
bias 0.9, error 1.6 (DEVICE_OBSERVED below); the library's host preparation: sImu 0.2, sVis 0.9.
"""
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import rotation_init_oracle as O  # noqa: E402

DPS = 50
DEVICE_FACTOR = 64          # the project's factor (tests/normal_equations_reference.py)
RATE = 256.0                # ts = i / 256: a dyadic grid, so that td = 1 / 512 ties exactly in float64 and in mpmath
HUBER_K = 1.345
BRANCH_MARGIN = 1e-9        # seconds; the float64 rounding of ts - td is ~1e-16
SIGMA_RATIO = 1e-3

# offset -> the edge it reaches
TDS = ((0.0, "generic"), (0.013, "generic"), (1.0 / 512.0, "tie"), (1.0, "held"), (-1.0, "extrapolated"), (-0.4, "shifted"))

# (series kind, edge) -> quantity -> float64 evaluation against the restatement, largest over the series of the kind (all n, bias
# estimated and not), rounded up to one digit.  Classes without R: R is not unique there (restate_R).
YARDSTICK = {
    ("rank3", "generic"): {"moments": 2e-15, "R": 3e-15, "bias": 2e-16, "err": 5e-15},        # measured 1.06e-15, 2.87e-15, 1.85e-16, 4.66e-15
    ("rank3", "tie"): {"moments": 2e-15, "R": 3e-15, "bias": 2e-16, "err": 4e-16},            # measured 1.32e-15, 2.20e-15, 1.19e-16, 3.32e-16
    ("rank3", "held"): {"moments": 7e-15, "R": 2e-15, "bias": 2e-15, "err": 2e-16},           # measured 6.89e-15, 1.36e-15, 1.21e-15, 1.05e-16
    ("rank3", "extrapolated"): {"moments": 5e-15, "R": 1e-15, "bias": 3e-15, "err": 1e-16},   # measured 4.09e-15, 9.46e-16, 2.46e-15, 9.31e-17
    ("rank3", "shifted"): {"moments": 2e-15, "R": 2e-15, "bias": 3e-15, "err": 5e-16},        # measured 1.72e-15, 1.89e-15, 2.00e-15, 4.39e-16
    ("huber", "generic"): {"moments": 2e-15, "R": 8e-16, "bias": 2e-16, "err": 6e-16},        # measured 1.23e-15, 7.52e-16, 1.17e-16, 5.14e-16
    ("huber", "tie"): {"moments": 5e-16, "R": 4e-16, "bias": 3e-17, "err": 2e-16},            # measured 4.50e-16, 3.90e-16, 2.73e-17, 1.14e-16
    ("planar", "generic"): {"moments": 4e-16, "R": 4e-16, "bias": 2e-16, "err": 9e-16},       # measured 3.88e-16, 3.92e-16, 1.08e-16, 8.96e-16
    ("planar", "tie"): {"moments": 2e-15, "R": 4e-16, "bias": 4e-17, "err": 3e-16},           # measured 1.13e-15, 3.37e-16, 3.49e-17, 2.36e-16
    ("planar", "held"): {"moments": 5e-15},                                                   # measured 4.08e-15
    ("planar", "extrapolated"): {"moments": 7e-16},                                           # measured 6.13e-16
    ("planar", "shifted"): {"moments": 1e-15, "R": 4e-16, "bias": 8e-16, "err": 3e-16},       # measured 9.63e-16, 3.13e-16, 7.19e-16, 2.12e-16
    ("axis", "generic"): {"moments": 8e-16},                                                  # measured 7.33e-16
    ("axis", "tie"): {"moments": 5e-16},                                                      # measured 4.96e-16
    ("axis", "held"): {"moments": 5e-15},                                                     # measured 4.84e-15
    ("axis", "extrapolated"): {"moments": 5e-16},                                             # measured 4.28e-16
    ("axis", "shifted"): {"moments": 5e-16},                                                  # measured 4.56e-16
}
# rotation_init_oracle.prepare against the restatement, relative to the largest entry of the array (measured 1.93e-15, 6.45e-15)
PREPARE_YARDSTICK = {"sImu": 2e-15, "sVis": 7e-15}
# worst device error / yardstick seen on an MI355X (allowed: DEVICE_FACTOR), per quantity
DEVICE_OBSERVED = {"moments": 0.7, "R": 1.4, "bias": 0.9, "err": 1.6}

Q_IC = np.array([-0.0060003, -0.70763572, 0.70653566, 0.00480024])
BIAS = np.array([0.01, -0.02, 0.015])


def _rot(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _rates(t, rng, fmin, fmax, amp):
    out = np.zeros((len(t), 3))
    for a in range(3):
        for _ in range(4):
            out[:, a] += rng.uniform(0.3, 1.0) * amp * np.sin(2 * np.pi * rng.uniform(fmin, fmax) * t + rng.uniform(0, 2 * np.pi))
    return out


def make_series(kind, n, seed):
    """ts, imu, vis of a seeded sum of sinusoids.  kind: 'rank3', 'huber' (visual series scaled by 3: the rotation cannot absorb
    it, the squared errors straddle the threshold), 'planar' (two-axis motion: rank 2), 'axis' (single-axis motion: rank 1)."""
    rng = np.random.default_rng(seed)
    ts = np.arange(n) / RATE
    fmin, fmax = (16.0, 60.0) if n <= 16 else (1.0, 6.0)          # n = 16 spans 62 ms: motion fast enough to be rank 3
    amp = 0.35 if kind == "huber" else 0.6
    imu = _rates(ts, rng, fmin, fmax, amp)
    lead = _rates(ts + 0.004, np.random.default_rng(seed), fmin, fmax, amp)      # the same motion seen 4 ms earlier
    if kind == "planar":
        imu[:, 2] = 0.0; lead[:, 2] = 0.0
    elif kind == "axis":
        u = np.array([0.36, -0.48, 0.8])
        imu = imu[:, :1] * u; lead = lead[:, :1] * u
    # (planar motion leaves one visual axis with noise only: no bias there, so that its mean stays below its spread)
    vis = lead @ _rot(Q_IC).T + (0.0 if kind == "planar" else BIAS) + 0.01 * rng.standard_normal((n, 3))
    if kind == "huber":
        vis = 3.0 * vis
    return ts, imu, vis


ALL_TDS = tuple(td for td, _ in TDS)
HUBER_TDS = (0.0, 0.013, 1.0 / 512.0)      # offsets at which the scaled series straddles the threshold (far offsets put every sample above it)
# name -> (kind, n, seed, offsets)
SERIES = {"rank3_n16": ("rank3", 16, 21, ALL_TDS), "rank3_n255": ("rank3", 255, 22, ALL_TDS), "rank3_n256": ("rank3", 256, 23, ALL_TDS),
          "rank3_n257": ("rank3", 257, 24, ALL_TDS), "rank3_n600": ("rank3", 600, 25, ALL_TDS), "huber_n257": ("huber", 257, 26, HUBER_TDS),
          "huber_n600": ("huber", 600, 27, HUBER_TDS), "planar_n256": ("planar", 256, 28, ALL_TDS), "axis_n255": ("axis", 255, 29, ALL_TDS)}


def restate_R(name, td):
    """Whether R is unique in exact arithmetic.  Not for single-axis motion, nor where every sample resamples from the same pair:
    td >= the last time (all held at the last sample: the cross-covariance is exactly zero), -td >= the last time (all extrapolated
    from the first pair: one line)."""
    kind, n = SERIES[name][:2]
    return kind != "axis" and abs(td) < (n - 1) / RATE


def _mpf(a):
    return [mp.mpf(float(v)) for v in np.asarray(a, dtype=np.float64).ravel()]


def nearest_first(grid, t, hint=None):
    """First index at the minimum |t - grid[j]| and that distance: the reference's linear scan (a strictly smaller distance moves
    the index).  `hint`: an index known to be within two of the answer on a sorted grid (the scan is then a window around it);
    returns also the gap to the runner-up (None at one candidate)."""
    lo, hi = (0, len(grid)) if hint is None else (max(0, hint - 2), min(len(grid), hint + 3))
    best, dist, second = lo, abs(t - grid[lo]), None
    for j in range(lo + 1, hi):
        d = abs(t - grid[j])
        if d < dist:
            second = dist; best, dist = j, d
        elif second is None or d < second:
            second = d
    return best, dist, (None if second is None else second - dist)


def resample(ts, vis, td, exact_ties=False):
    """q [n][3] (mpf), the nearest indices, the fractions, the number of held samples; asserts the branch margin."""
    n = len(ts)
    with mp.workdps(DPS):
        t = _mpf(ts); v = _mpf(vis); tdm = mp.mpf(float(td))
        shifted = [x - tdm for x in t]
        sf = np.asarray(ts, dtype=np.float64) - td
        q, ks, fs, held = [], [], [], 0
        for i in range(n):
            hint = int(np.clip(np.searchsorted(sf, ts[i]), 0, n - 1))
            k, dist, gap = nearest_first(shifted, t[i], hint)
            if gap is not None:
                if exact_ties and k + 1 < n:
                    assert gap == 0, "td = 1/512 on the dyadic grid: every interior decision is an exact tie"
                else:
                    assert gap >= BRANCH_MARGIN, ("nearest-sample decision within the margin of a tie", i, float(gap))
            if k + 1 < n:
                f = dist / (shifted[k + 1] - shifted[k])
                q.append([(1 - f) * v[3 * k + c] + f * v[3 * (k + 1) + c] for c in range(3)])
            else:
                f = mp.mpf(0); held += 1
                q.append([v[3 * k + c] for c in range(3)])
            ks.append(k); fs.append(f)
        return q, ks, fs, held


def probe(ts, imu, vis, td, exact_ties=False, want_R=True):
    """The restated probe: dict with moments / abs_moments (15), A, sigma, and for want_R: R (3x3 mp matrix), bias[estimate],
    err[estimate], errs[estimate] (per sample squared errors)."""
    n = len(ts)
    with mp.workdps(DPS):
        q, ks, fs, held = resample(ts, vis, td, exact_ties)
        p = [[mp.mpf(float(imu[i][c])) for c in range(3)] for i in range(n)]
        terms = [[p[i][c] for i in range(n)] for c in range(3)] + [[q[i][c] for i in range(n)] for c in range(3)] + \
                [[p[i][r] * q[i][c] for i in range(n)] for r in range(3) for c in range(3)]
        out = dict(moments=[mp.fsum(x) for x in terms], abs_moments=[mp.fsum(abs(y) for y in x) for x in terms], ks=ks, fs=fs, held=held, q=q)
        mi = [out["moments"][c] / n for c in range(3)]; mv = [out["moments"][3 + c] / n for c in range(3)]
        A = mp.matrix(3, 3)
        for r in range(3):
            for c in range(3):
                A[r, c] = mp.fsum((p[i][r] - mi[r]) * (q[i][c] - mv[c]) for i in range(n))
        out["A"] = A
        out["var_ok"] = all(mi[c] ** 2 <= mp.fsum((p[i][c] - mi[c]) ** 2 for i in range(n)) / n for c in range(3)) and \
            all(mv[c] ** 2 <= mp.fsum((q[i][c] - mv[c]) ** 2 for i in range(n)) / n for c in range(3))
        if not want_R:
            return out
        U, S, Vt = mp.svd_r(A)                      # A = U diag(S) Vt
        V = Vt.T
        C = mp.eye(3)
        if mp.det(V * U.T) < 0:
            C[2, 2] = -1
        R = V * C * U.T
        out["sigma"] = [S[k] for k in range(3)]; out["R"] = R
        K = mp.mpf(HUBER_K)
        for est in (True, False):
            b = [mv[r] - mp.fsum(R[r, c] * mi[c] for c in range(3)) for r in range(3)] if est else [mp.mpf(0)] * 3
            errs = [mp.fsum((q[i][r] - (mp.fsum(R[r, c] * p[i][c] for c in range(3)) + b[r])) ** 2 for r in range(3)) for i in range(n)]
            out[("bias", est)] = b; out[("errs", est)] = errs
            out[("err", est)] = mp.fsum(2 * K * mp.sqrt(e) - K * K if e > K else e for e in errs)
        return out


def check_conditions(name, td, ref):
    """The conditions of a restated-R case (module docstring)."""
    kind = SERIES[name][0]
    with mp.workdps(DPS):
        s = ref["sigma"]
        if kind == "planar":
            assert s[1] / s[0] >= SIGMA_RATIO and s[2] <= mp.mpf(10) ** (-40) * s[0], (name, td, [float(x) for x in s])
        else:
            assert s[2] / s[0] >= SIGMA_RATIO, (name, td, [float(x) for x in s])
        assert ref["var_ok"], (name, td, "per-axis mean^2 above the variance")
        K = mp.mpf(HUBER_K)
        for est in (True, False):
            errs = ref[("errs", est)]
            assert min(abs(e - K) for e in errs) >= mp.mpf("1e-6"), (name, td, est, "a squared error within 1e-6 of the Huber threshold")
            if kind == "huber":
                share = sum(1 for e in errs if e > K) / len(errs)
                assert 0.2 <= share <= 0.8, (name, td, est, share)
                assert any(K < e < K * K for e in errs), (name, td, est, "no sample between the threshold and its square")


_CACHE = {}
_SERIES_CACHE = {}


def series(name):
    if name not in _SERIES_CACHE:
        _SERIES_CACHE[name] = make_series(*SERIES[name][:3])
    return _SERIES_CACHE[name]


def restated(name, td):
    """The restated probe of a (series, offset), conditions checked, computed once per process."""
    key = (name, td)
    if key not in _CACHE:
        ts, imu, vis = series(name)
        cls = dict(TDS)[td]
        want = restate_R(name, td)
        ref = probe(ts, imu, vis, td, exact_ties=(cls == "tie"), want_R=want)
        if want:
            check_conditions(name, td, ref)
        _CACHE[key] = ref
    return _CACHE[key]


def moments_error(m, ref):
    """max over the 15 moments of |m - ref| / sum |terms|; a moment whose terms are all zero must be exactly zero."""
    worst = 0.0
    with mp.workdps(DPS):
        for k in range(15):
            if ref["abs_moments"][k] == 0:
                assert m[k] == 0.0, k
                continue
            worst = max(worst, float(abs(mp.mpf(float(m[k])) - ref["moments"][k]) / ref["abs_moments"][k]))
    return worst


def errors(ref, moments, R=None, b=None, err=None, estimate_bias=True):
    """{quantity: error} of an evaluation against a restated probe."""
    out = {"moments": moments_error(moments, ref)}
    if R is not None and "R" in ref:
        with mp.workdps(DPS):
            R = np.asarray(R, dtype=np.float64).reshape(3, 3)
            out["R"] = max(float(abs(mp.mpf(float(R[r, c])) - ref["R"][r, c])) for r in range(3) for c in range(3))
            out["bias"] = max(float(abs(mp.mpf(float(b[r])) - ref[("bias", estimate_bias)][r])) for r in range(3))
            e = ref[("err", estimate_bias)]
            out["err"] = float(abs(mp.mpf(float(err)) - e) / e)
    return out


def float64_moments(ts, imu, vis, td):
    """The 15 moments by plain numpy with the resampling lines of the oracle's solve_closed_form."""
    shifted = ts - td
    k, dist = O.nearest(shifted, ts)
    k1 = np.minimum(k + 1, len(ts) - 1)
    inner = k + 1 < len(ts)
    f = np.where(inner, dist / np.where(inner, shifted[k1] - shifted[k], 1.0), 0.0)[:, None]
    q = np.where(inner[:, None], (1.0 - f) * vis[k] + f * vis[k1], vis[k])
    return np.concatenate([imu.sum(axis=0), q.sum(axis=0), (imu.T @ q).ravel()])


def measure_yardsticks():
    """{(kind, edge): {quantity: largest float64 error over the cases of the class}}."""
    worst = {}
    for name, (kind, n, _, tds) in SERIES.items():
        ts, imu, vis = series(name)
        for td in tds:
            cls = dict(TDS)[td]
            ref = restated(name, td)
            w = worst.setdefault((kind, cls), {})
            m = float64_moments(ts, imu, vis, td)
            for est in (True, False):
                err, R, b = O.solve_closed_form(ts, vis, imu, td, est)
                for k, e in errors(ref, m, R, b, err, est).items():
                    w[k] = max(w.get(k, 0.0), e)
    return worst


# ---- the host preparation -------------------------------------------------------------------------------------------------------
def _slerp(a, t, b):
    """Eigen::Quaternion::slerp on mpf 4-lists (x, y, z, w); also whether the linear blend was taken."""
    d = mp.fsum(x * y for x, y in zip(a, b)); ad = abs(d)
    linear = ad >= 1 - mp.mpf(2) ** -52
    if linear:
        s0, s1 = 1 - t, t
    else:
        th = mp.acos(ad); st = mp.sin(th)
        s0, s1 = mp.sin((1 - t) * th) / st, mp.sin(t * th) / st
    if d < 0:
        s1 = -s1
    return [s0 * x + s1 * y for x, y in zip(a, b)], linear


def _qmul(a, b):
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
            aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz]


def prepare(t_vis, q_vis, t_imu, gyro, dt_imu):
    """tI (float64: the reference's own subtraction), sImu, sVis ([n][3] mpf), the indices where the over-2 pi rule held a value,
    the smallest distance of a rate component from 2 pi, and how often each branch was reached: exact nearest-frame ties, exact
    frame hits, linear blends of slerp, samples that take the last frame as it is."""
    t_vis = np.asarray(t_vis, dtype=np.float64); t_imu = np.asarray(t_imu, dtype=np.float64)
    t0 = max(t_vis[0], t_imu[0]); tend = max(t_vis[-1], t_imu[-1])
    mi = (t_imu >= t0) & (t_imu <= tend); mv = (t_vis >= t0) & (t_vis <= tend)
    tI = t_imu[mi] - t0; tV = t_vis[mv] - t0
    n = len(tI)
    with mp.workdps(DPS):
        gy = [[mp.mpf(float(x)) for x in row] for row in np.asarray(gyro, dtype=np.float64)[mi]]
        qV = [[mp.mpf(float(x)) for x in row] for row in np.asarray(q_vis, dtype=np.float64)[mv]]
        tIm = _mpf(tI); tVm = _mpf(tV)
        qi, ties, hits, linear, last_held = [], 0, 0, 0, 0
        for i in range(n):
            k, dist, gap = nearest_first(tVm, tIm[i])
            ties += gap is not None and gap == 0; hits += dist == 0
            if k + 1 < len(tVm):
                q, lin = _slerp(qV[k], dist / (tVm[k + 1] - tVm[k]), qV[k + 1])
                linear += bool(lin)
            else:
                q = qV[k]; last_held += 1
            qi.append(q)
        two_pi = 2 * mp.pi
        ang, held, margin = [], [], mp.inf
        for i in range(n):
            j = i if i + 1 < n else n - 2
            dq = [x - y for x, y in zip(qi[j + 1], qi[j])]
            nrm = mp.fsum(x * x for x in qi[i])
            inv = [-qi[i][0] / nrm, -qi[i][1] / nrm, -qi[i][2] / nrm, qi[i][3] / nrm]
            a = _qmul(dq, inv)
            v = [-2 / mp.mpf(float(dt_imu)) * a[c] for c in range(3)]
            margin = min(margin, min(abs(abs(x) - two_pi) for x in v))
            if any(abs(x) > two_pi for x in v):
                v = list(ang[i - 1]) if i > 1 else [mp.mpf(0)] * 3
                held.append(i)
            ang.append(v)

        def sma(x):
            return [[mp.fsum(x[j][c] for j in range(max(0, i - 14), i + 1)) / min(i + 1, 15) for c in range(3)] for i in range(n)]
        return dict(tI=tI, sImu=sma(gy), sVis=sma(ang), held=held, margin=float(margin), ties=int(ties), hits=int(hits), linear=linear, last_held=last_held, n_vis=len(tV))


def array_error(x, ref):
    """max |x - ref| / max |ref| of an [n, 3] array against [n][3] mpf."""
    x = np.asarray(x, dtype=np.float64)
    with mp.workdps(DPS):
        big = max(abs(v) for row in ref for v in row)
        return float(max(abs(mp.mpf(float(x[i, c])) - ref[i][c]) for i in range(len(ref)) for c in range(3)) / big)


def _exp_so3(phi):
    th = np.linalg.norm(phi, axis=1, keepdims=True)
    k = np.where(th > 1e-12, np.sin(th / 2) / np.where(th > 1e-12, th, 1.0), 0.5)
    return np.concatenate([k * phi, np.cos(th / 2)], axis=1)


def _views(t, seed, amp=0.5):
    rng = np.random.default_rng(seed)
    phi = np.stack([sum(amp * rng.uniform(0.3, 1.0) * np.sin(2 * np.pi * rng.uniform(0.3, 1.5) * t + rng.uniform(0, 2 * np.pi)) for _ in range(3))
                    for _ in range(3)], axis=1)
    return _exp_so3(phi)


def _prepare_cases():
    """name -> (t_vis, q_vis, t_imu, gyro, dt_imu).  IMU at 256 Hz."""
    out = {}
    rng = np.random.default_rng(40)
    dt = 1.0 / 256.0

    def gyro(n):
        return 0.5 * rng.standard_normal((n, 3)) + np.array([0.1, -0.2, 0.05])
    # camera (30 fps) starts and ends later than the IMU: the window opens at the first frame, the IMU tail is kept to the LATER end
    tv = 0.1037 + np.arange(40) / 30.0; ti = np.arange(330) / 256.0
    out["cam30_starts_later"] = (tv, _views(tv, 41), ti, gyro(len(ti)), dt)
    # IMU starts and ends later than the camera (10 fps): frames before the first IMU sample are cut, the IMU runs past the last frame
    tv = np.arange(15) / 10.0; ti = 0.2511 + np.arange(400) / 256.0
    out["cam10_imu_starts_later"] = (tv, _views(tv, 42), ti, gyro(len(ti)), dt)
    # dyadic frame times (32 fps) from the same start: IMU samples exactly on a frame time and exactly midway between two frames
    tv = np.arange(12) / 32.0; ti = np.arange(90) / 256.0
    out["cam32_ties_and_hits"] = (tv, _views(tv, 43, amp=0.2), ti, gyro(len(ti)), dt)
    # hemisphere flip (q -> -q from frame 5 on) on fast motion: the blend jumps a whole frame interval at every change of the nearest
    # frame, rates over 2 pi at i > 1; two early frames 3 / 256 apart put such a jump between IMU samples 1 and 2 (i <= 1: zero)
    tv = np.concatenate([[0.0, 3.0 / 256.0], 3.0 / 256.0 + np.arange(1, 12) / 30.0]); ti = np.arange(100) / 256.0
    qv = _views(tv * 1.0, 44, amp=1.2); qv[5:] *= -1.0
    out["flip_and_early_jump"] = (tv, qv, ti, gyro(len(ti)), dt)
    # identical consecutive quaternions: the linear-blend branch of slerp (|d| >= 1 - eps)
    tv = np.arange(10) / 30.0; ti = 0.01 + np.arange(70) / 256.0
    qv = _views(tv, 45, amp=0.3); qv[3:7] = qv[3]
    out["repeated_quaternions"] = (tv, qv, ti, gyro(len(ti)), dt)
    # the smallest window the estimator accepts: exactly 16 IMU samples
    tv = np.array([0.0, 0.03, 0.06]); ti = np.arange(16) / 256.0
    out["window_of_16"] = (tv, _views(tv, 46, amp=0.1), ti, gyro(16), dt)
    return out


PREPARE_CASES = _prepare_cases()
_PREP_CACHE = {}


def prepared(name):
    if name not in _PREP_CACHE:
        _PREP_CACHE[name] = prepare(*PREPARE_CASES[name])
    return _PREP_CACHE[name]


def measure_prepare_yardsticks():
    """{'sImu' / 'sVis': largest error of rotation_init_oracle.prepare over the cases}; tI must equal exactly."""
    worst = {"sImu": 0.0, "sVis": 0.0}
    for name, (tv, qv, ti, gy, dt) in PREPARE_CASES.items():
        ref = prepared(name)
        tI, sI, sV = O.prepare(tv, qv, ti, gy, dt)
        assert np.array_equal(tI, ref["tI"]), name
        worst["sImu"] = max(worst["sImu"], array_error(sI, ref["sImu"])); worst["sVis"] = max(worst["sVis"], array_error(sV, ref["sVis"]))
    return worst


def library_prepare(t_vis, q_vis, t_imu, gyro, dt_imu, cap=None):
    """The library's own host preparation (debug export oicc_debug_rotation_prepare, no device call): (status, n, tI, sImu, sVis)."""
    import ctypes as C
    from openimucameracalibrator_amd import _lib
    _DP = C.POINTER(C.c_double)
    fn = _lib.load().lib.oicc_debug_rotation_prepare
    fn.restype = C.c_int
    fn.argtypes = [C.c_int64, _DP, _DP, C.c_int64, _DP, _DP, C.c_double, C.c_int64, C.POINTER(C.c_int64), _DP, _DP, _DP]
    tv = np.ascontiguousarray(t_vis, dtype=np.float64); qv = np.ascontiguousarray(q_vis, dtype=np.float64)
    ti = np.ascontiguousarray(t_imu, dtype=np.float64); gy = np.ascontiguousarray(gyro, dtype=np.float64)
    cap = len(ti) if cap is None else cap
    tI = np.zeros(max(cap, 1)); sI = np.zeros((max(cap, 1), 3)); sV = np.zeros((max(cap, 1), 3)); n = C.c_int64(-1)
    rc = fn(len(tv), tv.ctypes.data_as(_DP), qv.ctypes.data_as(_DP), len(ti), ti.ctypes.data_as(_DP), gy.ctypes.data_as(_DP), dt_imu, cap,
            C.byref(n), tI.ctypes.data_as(_DP), sI.ctypes.data_as(_DP), sV.ctypes.data_as(_DP))
    return rc, n.value, tI[:max(n.value, 0)], sI[:max(n.value, 0)], sV[:max(n.value, 0)]
