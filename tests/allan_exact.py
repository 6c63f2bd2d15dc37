"""Exact reference of the overlapping Allan variance, the yardstick of tests/test_allan_exact.py (CPU) and
tests/test_gpu_allan_edges.py (MI355X).

The float64 restatement (tests/allan_restatement.py) loses its own running sum under a 9.8 m/s^2 mean.  Here nothing is rounded
before the last step.  The samples are snapped to a binary grid, q = rint(w 2^b) (b = 20 for accelerometer channels, 30 for
gyroscope channels in rad/s) and w = q 2^-b is what is tested; P = cumsum(q) and e = P[k+2m] - 2 P[k+m] + P[k] are exact in
int64.  The second difference annihilates a constant, so the mean the device subtracts does not enter, and scale[c] and freq
factor out of the sum.  e = h 2^21 + l with 0 <= l < 2^21, the three int64 dot products h.h, h.l, l.l cannot overflow for
|e| < 2^42 and n <= 65 537, and S_m = (hh << 42) + (hl << 22) + ll is the exact sum of squares as a Python int.  Then
sigma2_m = S_m scale^2 2^-2b / (freq^2 2 (period m)^2 (n - 2m)) in mpmath at 50 digits, freq and period the host's doubles.

The bound.  u = 2^-53.  With x_i = w_i scale - mean (mean the double the entry returns) the device stores
th_k = fl(S_k / freq), S_k its blocked sum of x_0..x_k (csrc/allan.hip, allan_scan_kernel: 8 values per thread, Hillis-Steele over
the 64 lanes of a wave, the 16 wave totals added in wave order onto a carry that advances once per pass of 8192 samples).  Let
Theta = max_k |sum_{i<=k} x_i| / freq, taken exactly.  Every intermediate of that scan is a sum over a range of samples, so at
most 2 Theta freq in size, and a sum that starts at sample 0 at most Theta freq.  To first order a stored prefix carries one
relative rounding u per addition on its way: 8 in the thread, 6 shuffle steps, 16 wave totals, the carry once per pass, the final
add (the division, and the c - 2b of the second difference, are of the same kind and sit inside the slack of the first two
counts: the thread's and the block total's first addition are to 0.0 and exact, and a wave adds 15 totals at most).  That is
A = 32 + ceil(n / 8192) roundings of at most u Theta each.  A term e = th[k+2m] - 2 th[k+m] + th[k] takes three of them with
weights 1, 2, 1: |de| <= 4 A u Theta.  A square doubles a relative error, so every term, and with it the mean of the terms in
the root-mean-square sense, moves by at most 2 . 4 A u Theta / rms_m relative to rms_m^2, rms_m = sqrt(S_m / T_m) in theta units,
T_m = n - 2m.  The sum of T_m squares (a fused multiply-add per term and lane, a fixed tree over the lanes of a factor, the chunks
in order) adds at most T_m u, the normalisation 2 (period m)^2 T_m and the division at most 8 u:

    B_m = 8 A u Theta / rms_m + (T_m + 8) u.

What of this is proved and what is not.  From a bound D on the error of every term to the sum is Cauchy-Schwarz:
|sum (e + d)^2 - sum e^2| <= (2 D / rms_m + (D / rms_m)^2) sum e^2, which is the factor 2 above.  That D = 4 A u Theta is a model,
not a chain of inequalities.  It counts the roundings on the path of one stored prefix; the whole summation tree below th_k has
k - 1 additions, and the worst case over it would put k where A stands.  The samples round as well: fl(w scale) by up to
|w scale| u on a gyroscope channel, and fl(. - mean) drops the same low bits of the mean at every sample of one binade, so that
the stored prefix of the emulation drifts from the exact one by up to 128 u Theta (measured over CASES, A <= 39) -- a drift
that is linear in k over long stretches and that the second difference removes like the mean itself.  So B_m is the size a
correct kernel must stay well inside, and tests/test_allan_exact.py measures by how much: the float64 emulation of the scan order
below (blocked_scan, then the second difference and a dot product as numpy takes them) reaches at most 0.044 B_m over every
factor, channel and case of CASES (at the one-term factor 16384 of n = 32 769; 0.027 or less elsewhere), and the largest B_m
there is 2.6e-11 (asserted <= 1e-10).  A dropped or misplaced term moves a factor by about 1 / T_m >= 2e-5, a million times B_m.
"""
import functools
import math

import mpmath as mp
import numpy as np

import allan_restatement as R

DPS = 50
ACC_BITS, GYRO_BITS = 20, 30
BITS = (ACC_BITS,) * 3 + (GYRO_BITS,) * 3
U = 2.0 ** -53
SCAN_PASS, TILE, CHUNK, SPAN, MAX_GROUP = 8192, 1024, 16384, 1024, 256
E_LIMIT = 1 << 42
SPLIT = 21

# name -> (n, num_clusters, seed, gravity, timestamp jitter).  What each reaches is asserted in tests/test_allan_exact.py.
CASES = {
    "n8": (8, 10000, 31, (0.0, 0.0, 9.81), False),
    "n9_c2": (9, 2, 32, (3.0, -4.0, 8.0), False),
    "n8191": (8191, 10000, 33, (0.0, 0.0, 9.81), False),
    "n8193": (8193, 10000, 34, (3.0, -4.0, 8.0), False),
    "n16385": (16385, 10000, 35, (0.0, 0.0, 9.81), True),
    "n32769": (32769, 10000, 36, (3.0, -4.0, 8.0), False),
    "n32770": (32770, 10000, 37, (0.0, 0.0, 9.81), False),
    "n49153": (49153, 10000, 38, (3.0, -4.0, 8.0), False),
    "n32769_c64": (32769, 64, 39, (0.0, 0.0, 9.81), False),
    "n40000_c300": (40000, 300, 40, (3.0, -4.0, 8.0), False),
}
REPEAT_CASES = ("n16385", "n49153")
GYRO_BIAS_CHANNEL, GYRO_BIAS = 4, 0.5          # gyr_y, rad/s
ACC_OFFSET_CHANNEL, ACC_OFFSET = 0, 150.0      # acc_x, m/s^2


def snap(w, bits):
    """q = rint(w 2^b) as int64 and the tested input q 2^-b, per channel."""
    w = np.atleast_2d(np.asarray(w, dtype=np.float64))
    q = np.stack([np.rint(w[c] * 2.0 ** bits[c]).astype(np.int64) for c in range(w.shape[0])])
    return q, np.stack([q[c] * 2.0 ** -bits[c] for c in range(w.shape[0])])


def plan(n, num_clusters=10000, fac=None):
    """The host's grouping rule (oicc_allan_variance): a group opens at factor f and takes members while cnt < 256 and
    factors[f + cnt] - factors[f] <= 1024; ceil((n - 2 factors[f]) / 16384) chunks, or 0.  [(m_first, count, span, chunks)]."""
    fac = R.factors(n, num_clusters).tolist() if fac is None else list(fac)
    out, f = [], 0
    while f < len(fac):
        cnt = 1
        while f + cnt < len(fac) and cnt < MAX_GROUP and fac[f + cnt] - fac[f] <= SPAN:
            cnt += 1
        kend1 = n - 2 * fac[f]
        out.append((fac[f], cnt, fac[f + cnt - 1] - fac[f], -(-kend1 // CHUNK) if kend1 > 0 else 0))
        f += cnt
    return out


def exact_sums(q, fac):
    """S[c][f] = sum_k (P[k+2m] - 2 P[k+m] + P[k])^2 as Python ints, None where n - 2m <= 0.  q int64 [channels][n]."""
    q = np.atleast_2d(q)
    ch, n = q.shape
    assert n <= 65537
    P = np.cumsum(q, axis=1, dtype=np.int64)
    out = [[None] * len(fac) for _ in range(ch)]
    e_buf, h_buf, l_buf = (np.empty(n, dtype=np.int64) for _ in range(3))
    for c in range(ch):
        p = P[c]
        for f, m in enumerate(np.asarray(fac).tolist()):
            T = n - 2 * m
            if T <= 0:
                continue
            e, h, l = e_buf[:T], h_buf[:T], l_buf[:T]
            np.subtract(p[2 * m:], p[m:n - m], out=e)
            e -= p[m:n - m]
            e += p[:T]
            np.right_shift(e, SPLIT, out=h)                         # floor: e = h 2^21 + l also for e < 0
            np.bitwise_and(e, (1 << SPLIT) - 1, out=l)
            assert -(E_LIMIT >> SPLIT) <= h.min() and h.max() < (E_LIMIT >> SPLIT)      # -2^42 <= e < 2^42
            out[c][f] = (int(np.dot(h, h)) << 2 * SPLIT) + (int(np.dot(h, l)) << (SPLIT + 1)) + int(np.dot(l, l))
    return out


def exact_sigma2(S, n, fac, scale, bits, freq, period):
    """sigma2 of one channel from its exact sums, [mpf], NaN where n - 2m <= 0."""
    with mp.workdps(DPS):
        k = mp.mpf(scale) ** 2 * mp.mpf(2) ** (-2 * bits) / mp.mpf(freq) ** 2
        return [mp.nan if s is None else s * k / (2 * (mp.mpf(period) * m) ** 2 * (n - 2 * m)) for s, m in zip(S, np.asarray(fac).tolist())]


def theta_max(q, bits, scale, mean, freq):
    """Theta = max_k |sum_{i<=k} (w_i scale - mean)| / freq, exactly: scale and mean are dyadic, so the prefixes are integers over
    one power of two."""
    sn, sd = float(scale).as_integer_ratio()
    mn, md = float(mean).as_integer_ratio()
    P = np.cumsum(np.asarray(q, dtype=np.int64)).astype(object)
    k1 = np.arange(1, len(P) + 1).astype(object)
    num = P * (sn * md) - k1 * (mn * sd << bits)
    with mp.workdps(DPS):
        return mp.mpf(int(np.abs(num).max())) / (sd * md << bits) / mp.mpf(freq)


def additions(n):
    return 32 + -(-n // SCAN_PASS)


def bound(S, n, fac, scale, bits, freq, theta):
    """B_m of one channel for every factor (module docstring), float64 [num_factors]; NaN where the factor has no term."""
    out = np.full(len(fac), np.nan)
    with mp.workdps(DPS):
        unit = mp.mpf(scale) * mp.mpf(2) ** -bits / mp.mpf(freq)
        for f, (s, m) in enumerate(zip(S, np.asarray(fac).tolist())):
            if s is None:
                continue
            T = n - 2 * m
            rms = mp.sqrt(mp.mpf(s) / T) * unit
            out[f] = float(8 * additions(n) * U * theta / rms + (T + 8) * U) if rms > 0 else np.inf
    return out


def blocked_scan(x, freq):
    """float64 emulation of allan_scan_kernel's order on x = w scale - mean: 8 values per thread in sequence, a Hillis-Steele scan
    of the thread totals over the 64 lanes of each wave, the wave totals added in wave order onto the carry, one carry step per
    pass of 8192 samples, and th = (excl + v) / freq."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    out = np.empty(n)
    carry = 0.0
    for base in range(0, n, SCAN_PASS):
        blk = np.zeros(SCAN_PASS)
        seg = x[base:base + SCAN_PASS]
        blk[:len(seg)] = seg
        v = np.cumsum(blk.reshape(1024, 8), axis=1)                  # sequential in the thread
        run = v[:, 7].reshape(16, 64)
        s = run.copy()
        d = 1
        while d < 64:
            y = s.copy()
            s[:, d:] = y[:, d:] + y[:, :-d]
            d <<= 1
        tot = s[:, 63]
        before = np.cumsum(np.concatenate([[carry], tot]))[:16]      # carry + tot[0] + ... + tot[wave - 1], in order
        excl = before[:, None] + (s - run)
        th = (excl.reshape(1024, 1) + v) / freq
        out[base:base + len(seg)] = th.reshape(-1)[:len(seg)]
        carry = carry + np.cumsum(tot)[-1]
    return out


def dot_variance(theta, period, n, num_clusters, fac, defect=None):
    """The partial and reduce kernels' arithmetic as numpy takes it (second difference (c - 2b) + a, one dot product), with the
    tile and group geometry of `plan` so that a defect can be planted:
      "tile_last"   the last term (i = 1023) of the first tile of every factor is dropped
      "middle_1024" element 1024 of the staged middle segment of the first tile reads 0
      "kend"        terms k < n - 2m - 1
      "group_d"     the last member of every group of two or more reads with d + 1 (zero fill past n, as the staging has it)"""
    theta = np.asarray(theta, dtype=np.float64)
    fac = np.asarray(fac).tolist()
    out = np.full(len(fac), np.nan)
    f = 0
    for m1, cnt, span, chunks in plan(n, num_clusters, fac):
        for g in range(cnt):
            m = fac[f + g]
            T = n - 2 * m
            if T <= 0:
                continue
            a, b, c = theta[:T], theta[m:m + T].copy(), theta[2 * m:2 * m + T]
            if defect == "group_d" and cnt > 1 and g == cnt - 1:
                pad = np.concatenate([theta, np.zeros(2 * m + 2)])
                b, c = pad[m + 1:m + 1 + T], pad[2 * m + 2:2 * m + 2 + T]
            if defect == "middle_1024" and 1 <= m - m1 <= TILE and TILE - (m - m1) < T:
                b[TILE - (m - m1)] = 0.0                              # i + d = 1024 in the tile k0 = 0
            e = (c - 2.0 * b) + a
            if defect == "tile_last" and T >= TILE:
                e = np.delete(e, TILE - 1)
            if defect == "kend":
                e = e[:-1]
            out[f + g] = np.dot(e, e) / (2.0 * ((period * m) * (period * m)) * T)
        f += cnt
    return out


SCALE = np.array([1.0, 1.0, 1.0, 57.3 * 3600, 57.3 * 3600, 57.3 * 3600])


def case_inputs(name):
    """w [6][n] (snapped), q, t_s of a case: synthetic.make_stationary_imu at 200 Hz with gravity, 150 m/s^2 added to acc_x and
    0.5 rad/s to gyr_y; with jitter, the timestamps move by up to 3 microseconds."""
    from openimucameracalibrator_amd import synthetic
    n, _, seed, gravity, jitter = CASES[name]
    tel, _ = synthetic.make_stationary_imu(duration=n / 200.0, rate=200.0, seed=seed, gravity=gravity)
    w = np.concatenate([tel["accelerometer"].T, tel["gyroscope"].T], axis=0)
    assert w.shape == (6, n)
    w[ACC_OFFSET_CHANNEL] += ACC_OFFSET
    w[GYRO_BIAS_CHANNEL] += GYRO_BIAS
    q, w = snap(w, BITS)
    t_ns = tel["timestamps_ns"].copy()
    if jitter:
        t_ns += (np.arange(n, dtype=np.int64) * 7919) % 6001 - 3000
        assert (np.diff(t_ns) > 0).all()
    return w, q, t_ns * 1e-9


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """Everything a test needs of a case, computed once per process and left unchanged: inputs, the restatement's host values,
    the exact sigma2 [6][num_factors] (mpf), Theta and B_m [6][num_factors]."""
    n, clusters = CASES[name][:2]
    w, q, t = case_inputs(name)
    fac = R.factors(n, clusters)
    freq, period = R.host_values(t)
    mean = [R.seq_mean(w[c] * SCALE[c]) for c in range(6)]
    S = exact_sums(q, fac)
    theta = [theta_max(q[c], BITS[c], SCALE[c], mean[c], freq) for c in range(6)]
    sigma2 = [exact_sigma2(S[c], n, fac, SCALE[c], BITS[c], freq, period) for c in range(6)]
    B = np.stack([bound(S[c], n, fac, SCALE[c], BITS[c], freq, theta[c]) for c in range(6)])
    for a in (w, q, t, fac, B):
        a.setflags(write=False)
    return dict(n=n, clusters=clusters, w=w, q=q, t=t, fac=fac, freq=freq, period=period, mean=mean, S=S, theta=theta,
                sigma2=sigma2, B=B)


def ratios(sigma2, ref, channel_map=None):
    """|sigma2 - exact| / (B_m exact) for every channel and factor that has a term, float64 [channels][num_factors] (NaN where
    the factor has none).  channel_map[c] names the reference channel of row c."""
    sigma2 = np.atleast_2d(sigma2)
    cm = range(sigma2.shape[0]) if channel_map is None else channel_map
    out = np.full(sigma2.shape, np.nan)
    with mp.workdps(DPS):
        for row, c in enumerate(cm):
            for f, ex in enumerate(ref["sigma2"][c]):
                if mp.isnan(ex):
                    continue
                got = float(sigma2[row, f])
                out[row, f] = float(abs(mp.mpf(got) - ex) / (ex * ref["B"][c, f])) if math.isfinite(got) else np.inf
    return out
