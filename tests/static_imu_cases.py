"""Inputs of the static IMU calibration's edge tests (test_static_imu_reference.py on the host, test_gpu_static_imu_edges.py on
the device), deterministic: detector signals whose interval lists are known by construction, gyro blocks at the step counts where
simu_gyro_kernel's chunking changes, accelerometer sample sets at the counts where acc_normal_eq's lanes and waves fall idle.

Detector signals: the constant (0, 0, 9.75) with offsets in [0.5, 1) on every sample that is not within h of a centre meant to be
still.  A window of the constant alone has a norm of exactly 0 (the sums of 9.75 are exact); every other window is far above, so
any threshold between (STILL_TH) gives exactly the runs placed, and the interval edges land on chosen lanes: centre i is lane
(i - h) % 256 of workgroup (i - h) // 256."""
import functools

import numpy as np

import static_imu_restatement as S

STILL_TH = 1e-9
QUIET = np.array([0.0, 0.0, 9.75])
G = 9.811107


# ---- detector -------------------------------------------------------------------------------------------------------------
def plain_detector_loop(acc, th, win=101):
    """utils::StaticIntervalsDetector, literally: per sample, DataVariance of the window, the look-for-start state machine."""
    w = S.normalized_win(win)
    h, n = w // 2, len(acc)
    out, look, cur = [], True, None
    if w >= n:
        return out
    for i in range(h, n - h):
        nrm = float(S.norm3(S.data_variance(acc, i - h, i + h)))
        if look and nrm < th:
            cur, look = i, False
        elif not look and nrm >= th:
            out.append((cur, i - 1)); look = True
    if not look:
        out.append((cur, n - h - 1))
    return out


def spiked_series(n, h, runs, seed):
    """[n][3]: still exactly on the centres of `runs` (inclusive pairs, at least 2h + 2 apart), loud on every other centre."""
    rng = np.random.RandomState(seed)
    acc = QUIET + rng.uniform(0.5, 1.0, (n, 3))
    prev_end = None
    for a, b in runs:
        assert h <= a <= b <= n - h - 1 and (prev_end is None or a >= prev_end + 2 * h + 2), (a, b, prev_end)
        acc[a - h:b + h + 1] = QUIET
        prev_end = b
    return acc


def _thresholds(nt, acc, win, runs):
    """nt thresholds and per threshold the list the construction fixes (None: only the restatement says).  0.0 equals the still
    norms bit for bit and the comparison is strict: nothing is still.  The smallest loud norm as a threshold leaves that centre
    loud for the same reason; one ulp above it does not."""
    full = [(win // 2, len(acc) - win // 2 - 1)]
    if nt == 1:
        return [STILL_TH], [runs]
    if nt == 2:
        return [0.0, STILL_TH], [[], runs]
    norms = S.window_norms(acc, win)
    loud = norms[np.isfinite(norms) & (norms > 0)]
    m = float(loud.min()) if len(loud) else 1.0
    th = [STILL_TH, 0.0, 1e9, m, float(np.nextafter(m, np.inf)), float(np.median(loud)) if len(loud) else 2.0, 5e-324, 0.5 * m, 2e-9, 1e300]
    return th, [runs, [], full, runs, None, None, runs, runs, runs, full]


def _spiked_case(name, win, M, runs, nt, seed):
    w = S.normalized_win(win)
    h = w // 2
    n = M + 2 * h
    acc = spiked_series(n, h, runs, seed) if M > 1 else np.tile(QUIET, (n, 1))
    th, expected = _thresholds(nt, acc, w, [tuple(r) for r in runs])
    if M == 1:          # win_size >= n: the detector returns before it looks at a sample, however still the series is
        expected = [[] for _ in th]
    return dict(name=name, acc=acc, win=win, h=h, thresholds=np.array(th), expected=expected)


def _centre(h, group, lane):
    return h + 256 * group + lane


def _length_runs(h, M):
    """Runs for a series of M centres: from the first centre, at the last centre alone, and one across centre 255 | 256 if it fits."""
    first, last = h, h + M - 1
    if M <= 2:          # M = 1 never reaches the kernels (_spiked_case); M = 2: still at the first centre, loud at the last
        return [(first, first)] if M == 2 else []
    runs = [(first, first + 2)]
    a = h + 254
    if a >= runs[-1][1] + 2 * h + 2 and a + 3 + 2 * h + 2 <= last:
        runs.append((a, a + 3))
    if last >= runs[-1][1] + 2 * h + 2:
        runs.append((last, last))
    return runs


@functools.lru_cache(maxsize=None)
def detector_cases():
    """{name: case}; case: acc [n][3], win (as passed in), h, thresholds [nt], expected (per threshold a list of pairs, or None)."""
    c = _centre
    cases = [
        # rises at lanes 63, 255 (one centre: its fall is lane 0 of the next workgroup), 64, 0, 255 (ends in the next workgroup)
        _spiked_case("lanes", 11, 1024, [(c(5, 0, 63), c(5, 0, 63) + 1), (c(5, 0, 255), c(5, 0, 255)), (c(5, 1, 64), c(5, 1, 64) + 5),
                                           (c(5, 2, 0), c(5, 2, 0) + 13), (c(5, 2, 255), c(5, 2, 255) + 3)], 10, 1),
        # start in workgroup 0, end in workgroup 2; then starts whose index follows a run of several workgroups
        _spiked_case("span3", 11, 1024, [(200, 700), (c(5, 3, 0), c(5, 3, 0)), (c(5, 3, 63), c(5, 3, 64))], 2, 2),
        _spiked_case("span4_to_the_end", 11, 1100, [(c(5, 0, 255), 5 + 1099)], 1, 3),
        # the i > h guard, and rise && last in one lane (lane 0 of workgroup 2)
        _spiked_case("first_and_last", 11, 513, [(5, 20), (517, 517)], 2, 4),
        _spiked_case("first_centre_alone", 11, 300, [(5, 5), (40, 41)], 1, 5),
        _spiked_case("table", 11, 513, [(5, 5), (68, 132), (260, 261), (516, 517)], 10, 6),
        _spiked_case("all_still", 11, 513, [(5, 517)], 10, 7),
        _spiked_case("all_loud", 11, 513, [], 10, 8),
        # the densest alternation the construction allows: one still centre in every 2h + 2
        _spiked_case("dense", 11, 1030, [(i, i) for i in range(5, 5 + 1030, 12)], 2, 9),
    ]
    k = 0
    for win in (11, 12, 41):
        h = S.normalized_win(win) // 2
        for M in LENGTHS:
            cases.append(_spiked_case("len_win%d_M%d" % (win, M), win, M, _length_runs(h, M), (1, 2, 10)[k % 3], 20 + k))
            k += 1
    # the largest window: thresholds from the restatement's own norms, one of them a norm bit for bit
    for win in (1025, 1024):
        for M in LARGE_LENGTHS:
            rng = np.random.RandomState(40 + win + M)
            acc = QUIET + 0.02 * rng.standard_normal((M + 1024, 3))
            acc[300:500] += 0.3 * rng.standard_normal((200, 3))
            norms = S.window_norms(acc, win)[512:512 + M]
            if M == 1:
                th, expected = [1e-3, 1e9], [[], []]
            elif M == 2:
                th = [float(norms.max()), float(np.nextafter(norms.max(), np.inf))]
                k = int(np.argmin(norms))
                expected = [[(512 + k, 512 + k)], [(512, 513)]]
            else:
                q = np.sort(norms)
                th = [float(q[0]), float(q[1]), float(q[M // 10]), float(q[M // 4]), float(q[M // 2]), float(norms[100]),
                      float(q[3 * M // 4]), float(q[-1]), float(np.nextafter(q[-1], np.inf)), float(0.5 * (q[M // 2] + q[M // 2 + 1]))]
                expected = [[]] + [None] * 7 + [[(512, 512 + M - 1)], None]
            cases.append(dict(name="noisy_win%d_M%d" % (win, M), acc=acc, win=win, h=512, thresholds=np.array(th), expected=expected))
    # a noisy series at the smallest window: the median threshold alternates as fast as a signal can
    rng = np.random.RandomState(77)
    acc = QUIET + 0.02 * rng.standard_normal((5 + 600 + 5, 3))
    norms = S.window_norms(acc, 11)[5:605]
    q = np.sort(norms)
    th = [float(q[k]) for k in (0, 60, 150, 240, 300, 360, 450, 540, 599)] + [float(norms[255])]
    cases.append(dict(name="noisy_win11_M600", acc=acc, win=11, h=5, thresholds=np.array(th), expected=[[]] + [None] * 9))
    out = {k["name"]: k for k in cases}
    assert len(out) == len(cases)
    return out


LENGTHS = (1, 2, 255, 256, 257, 513)          # n - 2h; 1 is win_size = n, which the entry answers without a launch
LARGE_LENGTHS = (1, 2, 257)
DETECTOR_NAMES = ["lanes", "span3", "span4_to_the_end", "first_and_last", "first_centre_alone", "table", "all_still", "all_loud", "dense"] + \
    ["len_win%d_M%d" % (w, M) for w in (11, 12, 41) for M in LENGTHS] + \
    ["noisy_win%d_M%d" % (w, M) for w in (1025, 1024) for M in LARGE_LENGTHS] + ["noisy_win11_M600"]


# ---- gyro blocks ----------------------------------------------------------------------------------------------------------
GYRO_N = 1100
GYRO_I0 = 100
GYRO_STEPS = (1, 2, 255, 256, 257, 513)
GYRO_END_STEPS = 37
P_AWAY = np.r_[1e-3, -2e-3, 5e-4, 1e-3, -1e-3, 2e-3, 0.99, 1.01, 1.005, 1e-3, -2e-3, 3e-3]
P_START = np.r_[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0]

# class -> (i0, i1).  The step classes share their first sample, so that one 50-digit integration serves them all.
GYRO_RANGES = {"0a": (-1, 300), "0b": (GYRO_I0, GYRO_I0)}
GYRO_RANGES.update({str(s): (GYRO_I0, GYRO_I0 + s) for s in GYRO_STEPS})
GYRO_RANGES["end"] = (GYRO_N - 1 - GYRO_END_STEPS, GYRO_N - 1)
GYRO_CLASSES = list(GYRO_RANGES)


def gyro_steps(cls):
    i0, i1 = GYRO_RANGES[cls]
    return i1 - i0 if i0 >= 0 and i1 > i0 else 0


@functools.lru_cache(maxsize=None)
def gyro_series():
    """{'uniform' | 'jitter': (t [n], w [n][3])}: 200 Hz, smooth rates of order 1 rad/s plus noise; the jittered copy moves every
    timestamp by up to 30 % of the period (strictly increasing)."""
    rng = np.random.RandomState(21)
    t = np.arange(GYRO_N) / 200.0
    f = rng.uniform(0.3, 2.0, (3, 3))
    ph = rng.uniform(0, 2 * np.pi, (3, 3))
    a = rng.uniform(0.3, 0.8, (3, 3))
    w = np.stack([(a[c] * np.sin(2 * np.pi * f[c] * t[:, None] + ph[c])).sum(axis=1) for c in range(3)], axis=1)
    w = w + 1e-3 * rng.standard_normal(w.shape)
    tj = t + rng.uniform(-0.3, 0.3, GYRO_N) / 200.0
    assert np.all(np.diff(tj) > 0)
    return {"uniform": (t, w), "jitter": (tj, w)}


@functools.lru_cache(maxsize=None)
def gyro_versors():
    """{class: (g0, g1)} random unit vectors."""
    rng = np.random.RandomState(22)
    out = {}
    for cls in GYRO_CLASSES:
        g = rng.standard_normal((2, 3))
        g /= np.linalg.norm(g, axis=1)[:, None]
        out[cls] = (g[0], g[1])
    return out


# name -> (series, parameters, optimize_bias, gyro_dt, classes)
GYRO_CONFIGS = {
    "away": ("uniform", P_AWAY, True, -1.0, GYRO_CLASSES),
    "start": ("uniform", P_START, True, -1.0, GYRO_CLASSES),
    "jitter": ("jitter", P_AWAY, True, -1.0, GYRO_CLASSES),
    "jitter_fixed_dt": ("jitter", P_AWAY, True, 0.005, GYRO_CLASSES),     # the fixed step must be what is used
    "no_bias": ("uniform", P_AWAY, False, -1.0, ["257"]),
}


def gyro_case_list():
    """[(config, class)] of every gyro case."""
    return [(cfg, cls) for cfg, v in GYRO_CONFIGS.items() for cls in v[4]]


def gyro_inputs(config):
    """(t, w, ranges [b][2], versors [b][6], parameters, optimize_bias, gyro_dt, classes) of a configuration: what eval_gyro and
    gyro_blocks_eval take."""
    series, p, ob, dt, classes = GYRO_CONFIGS[config]
    t, w = gyro_series()[series]
    gv = gyro_versors()
    return (t, w, np.array([GYRO_RANGES[c] for c in classes], dtype=np.int32), np.array([np.r_[gv[c][0], gv[c][1]] for c in classes]),
            p, ob, dt, list(classes))


# ---- accelerometer --------------------------------------------------------------------------------------------------------
ACC_COUNTS = (1, 63, 64, 65, 255, 256, 257, 513)
ACC_BIAS = np.r_[0.05, -0.02, 0.1]
ACC_PARAMS = {"start": np.r_[0.0, 0.0, 0.0, 1.0, 1.0, 1.0, ACC_BIAS],
              "misaligned": np.r_[0.02, -0.02, 0.02, 1.02, 0.98, 1.02, ACC_BIAS]}


@functools.lru_cache(maxsize=None)
def acc_samples():
    """[513][3] near |x - b| = g; the sample sets are its leading rows.  Row 0 is generic (a count of one has no zero column);
    rows 1 ... 3 have components equal to the bias bit for bit (u = 0), and row 4 has |c| within 1e-12 of g at the start parameters."""
    rng = np.random.RandomState(31)
    d = rng.standard_normal((513, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    x = ACC_BIAS + G * d * (1.0 + 5e-3 * rng.standard_normal((513, 1))) + 2e-3 * rng.standard_normal((513, 3))
    x[1, 0] = ACC_BIAS[0]
    x[2, 1], x[2, 2] = ACC_BIAS[1], ACC_BIAS[2]
    x[3, 0], x[3, 1] = ACC_BIAS[0], ACC_BIAS[1]
    x[4] = ACC_BIAS + G * np.r_[2.0, 3.0, 6.0] / 7.0
    u = x[4] - ACC_BIAS
    assert abs(np.sqrt(u @ u) - G) <= 1e-12 * G
    return x


# ---- the calibrator under its other options --------------------------------------------------------------------------------
RECORDING = dict(num_poses=14, rate=100.0, init_s=6.0, hold_s=2.0, move_s=1.0)
CALIBRATION_INIT_S = 6.0
# name -> (setter calls on StaticImuCalibrator, fields of its options, keywords of static_imu_restatement.calibrate)
CALIBRATION_CONFIGS = {
    "acc_use_means": ([("EnableAccUseMeans", True)], {}, dict(acc_use_means=True)),
    "n_samples_7": ([("SetIntarvalsNumSamples", 7)], {}, dict(n_samps=7)),
    "win_41": ([], dict(win_size=41), dict(win=41)),
    "gyro_dt_and_bias": ([("SetGyroDataPeriod", 0.01), ("EnableGyroBiasOptimization", True)], {}, dict(gyro_dt=0.01, optimize_gyro_bias=True)),
}
