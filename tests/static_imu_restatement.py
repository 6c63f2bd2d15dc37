"""numpy restatement of core::StaticImuCalibrator::CalibrateAccGyro (src/core/static_imu_calibrator.cc), operation for
operation, written from the reference's sources and independent of the HIP unit:
  - StaticIntervalsDetector (imu_data_interval.cc:111-149): vectorised over the window centre, sequential over the
    offsets, so every norm is the per-sample loop's bit for bit (numpy does not contract to FMA);
  - MultiPosAccResidual / MultiPosGyroResidual (static_imu_calibrator.h): the gyro residual integrates with the
    per-step-normalised RK4 of gyro_integration.h on dual numbers (Jets), one derivative column per parameter;
  - the minimiser: Ceres 2.1 TrustRegionMinimizer + LevenbergMarquardtStrategy with default Solver::Options, the
    damped step by Cholesky of the normal equations."""
import numpy as np

OPTS = dict(ftol=1e-6, ptol=1e-8, gtol=1e-10, radius=1e4, max_radius=1e16, min_radius=1e-32, min_rel=1e-3, min_diag=1e-6,
            max_diag=1e32, max_invalid=5, max_iters=50)
TERM_GRADIENT, TERM_FUNCTION, TERM_PARAMETER, TERM_MAX_ITERATIONS, TERM_MIN_RADIUS, TERM_INVALID, TERM_EVAL = range(7)
TERM_SKIPPED = -1


# ---- DataInterval / DataMean / DataVariance (imu_data_interval.h, .cc:35-61) --------------------------------------
def time_to_index(t, ts):
    i0, i1 = 0, len(t) - 1
    while i1 - i0 > 1:
        m = (i1 + i0) // 2
        if ts > t[m]:
            i0 = m
        else:
            i1 = m
    return i0 if ts - t[i0] < t[i1] - ts else i1


def initial_interval(t, duration):
    end_ts = t[0] + duration
    return (0, len(t) - 1) if end_ts >= t[-1] else (0, time_to_index(t, end_ts))


def seq_sum(x):
    """Sequential sum over axis 0 (np.sum is pairwise; the cumulative sum adds in order)."""
    return np.cumsum(x, axis=0)[-1]


def data_mean(x, s, e):
    return seq_sum(x[s:e + 1]) / float(e - s + 1)


def data_variance(x, s, e):
    d = x[s:e + 1] - data_mean(x, s, e)
    return seq_sum(d * d) / float(e - s)


def norm3(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def normalized_win(w):
    w = max(w, 11)
    return w + 1 if w % 2 == 0 else w


def window_norms(acc, win=101):
    """norm[i] for i in [h, n-h) (NaN elsewhere)."""
    w = normalized_win(win)
    h, n = w // 2, len(acc)
    out = np.full(n, np.nan)
    if w >= n:
        return out
    M = n - 2 * h
    m = np.zeros((M, 3))
    for k in range(w):
        m = m + acc[k:k + M]
    m = m / float(w)
    v = np.zeros((M, 3))
    for k in range(w):
        d = acc[k:k + M] - m
        v = v + d * d
    v = v / float(w - 1)
    out[h:n - h] = norm3(v)
    return out


def intervals_from_norms(norms, th, win=101):
    """The detector's state machine on precomputed norms (vectorised: starts at rising, ends before falling edges)."""
    w = normalized_win(win)
    h, n = w // 2, len(norms)
    if w >= n:
        return np.zeros((0, 2), dtype=np.int64)
    f = norms[h:n - h] < th
    prev = np.r_[False, f[:-1]]
    starts = np.nonzero(f & ~prev)[0] + h
    ends = np.nonzero(~f & prev)[0] + h - 1
    if f[-1]:
        ends = np.r_[ends, n - h - 1]
    return np.stack([starts, ends], axis=1).astype(np.int64)


def extract(intervals, n_samps):
    return [tuple(iv) for iv in intervals if iv[1] - iv[0] + 1 >= n_samps]


# ---- residuals ----------------------------------------------------------------------------------------------------
def acc_rows(x, p, g_mag):
    """r [n] and J [n][9] of MultiPosAccResidual; ms = T K, c = ms (x - b) summed in column order."""
    m0, m1, m2, sx, sy, sz = p[:6]
    u0, u1, u2 = x[:, 0] - p[6], x[:, 1] - p[7], x[:, 2] - p[8]
    ms01, ms02, ms12 = -m0 * sy, m1 * sz, -m2 * sz
    c0 = (sx * u0 + ms01 * u1) + ms02 * u2
    c1 = sy * u1 + ms12 * u2
    c2 = sz * u2
    nrm = np.sqrt((c0 * c0 + c1 * c1) + c2 * c2)
    e0, e1, e2 = c0 / nrm, c1 / nrm, c2 / nrm
    J = np.stack([e0 * (sy * u1), -e0 * (sz * u2), e1 * (sz * u2), -e0 * u0, -(e0 * (-m0 * u1) + e1 * u1),
                  -((e0 * (m1 * u2) + e1 * (-m2 * u2)) + e2 * u2), e0 * sx, -(e0 * (m0 * sy) - e1 * sy),
                  -((e0 * (-m1 * sz) + e1 * (m2 * sz)) - e2 * sz)], axis=1)
    return g_mag - nrm, J


def acc_residual_plain(x, p, g_mag):
    """g - |T K (x - b)| for one sample in plain Python floats (the Jacobian tests difference this)."""
    T = [[1, -p[0], p[1]], [0, 1, -p[2]], [0, 0, 1]]
    u = [x[i] - p[6 + i] for i in range(3)]
    c = [sum(T[i][j] * p[3 + j] * u[j] for j in range(3)) for i in range(3)]
    return g_mag - (c[0] ** 2 + c[1] ** 2 + c[2] ** 2) ** 0.5


# Jets: arrays [..., 1 + np], value first
def jmul(a, b):
    out = a[..., :1] * b
    out[..., 1:] += a[..., 1:] * b[..., :1]
    return out


def jconst(v, np_):
    v = np.asarray(v, dtype=np.float64)
    out = np.zeros(v.shape + (1 + np_,))
    out[..., 0] = v
    return out


def gyro_ms_bias(p, optimize_bias):
    """Jet T K and bias from the 12 parameters (derivative columns 9 or 12)."""
    np_ = 12 if optimize_bias else 9
    th = np.zeros((12, 1 + np_))
    th[:, 0] = p
    for k in range(np_):
        th[k, 1 + k] = 1.0
    one, zero = jconst(1.0, np_), jconst(0.0, np_)
    T = [[one, -th[0], th[1]], [th[3], one, -th[2]], [-th[4], th[5], one]]
    ms = [[jmul(T[i][j], th[6 + j]) for j in range(3)] for i in range(3)]
    b = [th[9 + k] if optimize_bias else zero for k in range(3)]
    return ms, b, np_


def gyro_omega(ms, b, x):
    """UnbiasNormalize of samples x [m][3] -> Jet omega [m][3][1+np]."""
    np1 = ms[0][0].shape[-1]
    u = [jconst(x[:, k], np1 - 1) - b[k] for k in range(3)]
    return np.stack([(jmul(ms[i][0][None], u[0]) + jmul(ms[i][1][None], u[1])) + jmul(ms[i][2][None], u[2]) for i in range(3)], axis=1)


def half_skew(w, q):
    """0.5 * Omega(w) q (ComputeOmegaSkew), Jets [..., 3|4, 1+np]."""
    w0, w1, w2 = w[..., 0, :], w[..., 1, :], w[..., 2, :]
    q0, q1, q2, q3 = q[..., 0, :], q[..., 1, :], q[..., 2, :], q[..., 3, :]
    return 0.5 * np.stack([(jmul(-w0, q1) - jmul(w1, q2)) - jmul(w2, q3), (jmul(w0, q0) + jmul(w2, q2)) - jmul(w1, q3),
                           (jmul(w1, q0) - jmul(w2, q1)) + jmul(w0, q3), (jmul(w2, q0) + jmul(w1, q1)) - jmul(w0, q2)], axis=-2)


def rk4_step(q, w0, w1, dt):
    """QuatIntegrationStepRK4 without the normalisation; dt broadcast as a plain factor."""
    w01 = 0.5 * (w0 + w1)
    k1 = half_skew(w0, q)
    k2 = half_skew(w01, q + (0.5 * dt) * k1)
    k3 = half_skew(w01, q + (0.5 * dt) * k2)
    k4 = half_skew(w1, q + dt * k3)
    m1, m2 = 1.0 / 6.0, 1.0 / 3.0
    return q + dt * (((m1 * k1 + m2 * k2) + m2 * k3) + m1 * k4)


def jnormalize(q):
    n2 = ((jmul(q[..., 0, :], q[..., 0, :]) + jmul(q[..., 1, :], q[..., 1, :])) + jmul(q[..., 2, :], q[..., 2, :])) + jmul(q[..., 3, :], q[..., 3, :])
    s = np.sqrt(n2[..., 0])
    inv = np.zeros_like(n2)
    inv[..., 0] = 1.0 / s
    inv[..., 1:] = -n2[..., 1:] / (2.0 * s[..., None] ** 3)
    return jmul(q, inv[..., None, :])


def quat_to_rotation(q):
    """ceres::QuaternionToRotation on Jets [..., 4, 1+np] -> [..., 3, 3, 1+np]."""
    a, b, c, d = q[..., 0, :], q[..., 1, :], q[..., 2, :], q[..., 3, :]
    aa, ab, ac, ad, bb, bc, bd, cc, cd, dd = (jmul(a, a), jmul(a, b), jmul(a, c), jmul(a, d), jmul(b, b), jmul(b, c), jmul(b, d),
                                              jmul(c, c), jmul(c, d), jmul(d, d))
    R = np.stack([np.stack([((aa + bb) - cc) - dd, 2.0 * (bc - ad), 2.0 * (ac + bd)], -2),
                  np.stack([2.0 * (ad + bc), ((aa - bb) + cc) - dd, 2.0 * (cd - ab)], -2),
                  np.stack([2.0 * (bd - ac), 2.0 * (ab + cd), ((aa - bb) - cc) + dd], -2)], -3)
    n2 = ((aa + bb) + cc) + dd
    inv = np.zeros_like(n2)
    inv[..., 0] = 1.0 / n2[..., 0]
    inv[..., 1:] = -n2[..., 1:] / (n2[..., :1] * n2[..., :1])
    return jmul(R, inv[..., None, None, :])


def gyro_blocks_eval(t, gyro, ranges, gv, p, optimize_bias=False, gyro_dt=-1.0, product_form=False):
    """r [3 nb], J [3 nb][np] of MultiPosGyroResidual for every block, all blocks stepped together.  product_form:
    integrate without the per-step normalisation (what the device evaluates)."""
    ms, b, np_ = gyro_ms_bias(np.asarray(p, dtype=np.float64), optimize_bias)
    nb = len(ranges)
    steps = np.array([max(i1 - i0, 0) if i0 >= 0 else 0 for i0, i1 in ranges])
    q = np.zeros((nb, 4, 1 + np_))
    q[:, 0, 0] = 1.0
    i0s = np.array([max(r[0], 0) for r in ranges])
    for k in range(int(steps.max(initial=0))):
        act = np.nonzero(steps > k)[0]
        s = i0s[act] + k
        w0 = gyro_omega(ms, b, gyro[s])
        w1 = gyro_omega(ms, b, gyro[s + 1])
        dt = np.full(len(act), gyro_dt) if gyro_dt > 0 else t[s + 1] - t[s]
        qn = rk4_step(q[act], w0, w1, dt[:, None, None])
        q[act] = qn if product_form else jnormalize(qn)
    R = quat_to_rotation(q)
    g0 = jconst(np.asarray(gv)[:, :3], np_)
    g1 = jconst(np.asarray(gv)[:, 3:], np_)
    res = np.stack([(jmul(g0[:, 0], R[:, 0, i]) + jmul(g0[:, 1], R[:, 1, i])) + jmul(g0[:, 2], R[:, 2, i]) for i in range(3)], axis=1) - g1
    return res[..., 0].reshape(-1), res[..., 1:].reshape(-1, np_)


def normal_eq(r, J):
    # einsum, not BLAS: rows in order on every machine (static_imu_reference.YARDSTICK is measured from these sums)
    return 0.5 * seq_sum(r * r), np.einsum("ri,rj->ij", J, J), np.einsum("ri,r->i", J, r)


# ---- minimiser ----------------------------------------------------------------------------------------------------
def chol_solve(A, rhs):
    n = len(rhs)
    L = np.zeros((n, n))
    for j in range(n):
        t = A[j, j] - sum(L[j, k] * L[j, k] for k in range(j))
        if not t > 0.0:
            return None
        L[j, j] = np.sqrt(t)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - sum(L[i, k] * L[j, k] for k in range(j))) / L[j, j]
    y = np.zeros(n)
    for i in range(n):
        y[i] = (rhs[i] - sum(L[i, k] * y[k] for k in range(i))) / L[i, i]
    x = np.zeros(n)
    for i in reversed(range(n)):
        x[i] = (y[i] - sum(L[k, i] * x[k] for k in range(i + 1, n))) / L[i, i]
    return x if np.all(np.isfinite(x)) else None


def lm(evaluate, x0, o=OPTS):
    """Ceres 2.1 LM, default options.  evaluate(x) -> (cost, H, g) or None.  Returns x, cost, iterations, termination."""
    x = np.array(x0, dtype=np.float64)
    ev = evaluate(x)
    if ev is None:
        return x, np.nan, 0, TERM_EVAL
    cost, H, g = ev
    scale = 1.0 / (1.0 + np.sqrt(np.diag(H)))
    radius, dec, reuse, invalid, it = o["radius"], 2.0, False, 0, 0
    x_norm = np.sqrt(seq_sum(x * x))
    if np.max(np.abs(g)) <= o["gtol"]:
        return x, cost, 0, TERM_GRADIENT
    diag = None
    while True:
        if it >= o["max_iters"]:
            return x, cost, it, TERM_MAX_ITERATIONS
        if radius <= o["min_radius"]:
            return x, cost, it, TERM_MIN_RADIUS
        it += 1
        if not reuse:
            diag = np.minimum(np.maximum(np.diag(H) * scale * scale, o["min_diag"]), o["max_diag"])
        D2 = diag / radius
        A = H * scale[:, None] * scale[None, :] + np.diag(D2)
        step = chol_solve(A, -g * scale)
        model = 0.0
        if step is not None:
            model = seq_sum(0.5 * step * (D2 * step - g * scale))
        if step is None or not model > 0.0:
            invalid += 1
            if invalid >= o["max_invalid"]:
                return x, cost, it, TERM_INVALID
            radius /= dec; dec *= 2.0; reuse = True
            continue
        invalid = 0
        cand = x + step * scale
        ec = evaluate(cand)
        cc = ec[0] if ec is not None and np.isfinite(ec[0]) else np.finfo(np.float64).max
        step_norm = np.sqrt(seq_sum((cand - x) ** 2))
        change = cost - cc
        rel = change / model
        if step_norm <= o["ptol"] * (x_norm + o["ptol"]):
            return x, cost, it, TERM_PARAMETER
        if abs(change) <= o["ftol"] * cost:
            return x, cost, it, TERM_FUNCTION
        if rel > o["min_rel"]:
            x = cand
            x_norm = np.sqrt(seq_sum(x * x))
            cost, H, g = ec
            q = 2.0 * rel - 1.0
            radius = min(o["max_radius"], radius / max(1.0 / 3.0, 1.0 - q * q * q))
            dec, reuse = 2.0, False
            if np.max(np.abs(g)) <= o["gtol"]:
                return x, cost, it, TERM_GRADIENT
        else:
            radius /= dec; dec *= 2.0; reuse = True


# ---- CalibrateAccGyro ---------------------------------------------------------------------------------------------
def calibrate(t, acc, gyro, g_mag=9.81, init_s=30.0, n_samps=100, min_intervals=12, win=101, acc_use_means=False,
              gyro_dt=-1.0, optimize_gyro_bias=False):
    t = np.asarray(t, dtype=np.float64); acc = np.asarray(acc, dtype=np.float64); gyro = np.asarray(gyro, dtype=np.float64)
    s, e = initial_interval(t, init_s)
    mean = data_mean(acc, s, e)
    imax = int(np.argmax(mean))                # maxCoeff: the first largest
    bias0 = mean.copy(); bias0[imax] -= g_mag
    norm_th = float(norm3(data_variance(acc, s, e)))
    norms = window_norms(acc, win)
    x0 = np.r_[0.0, 0.0, 0.0, 1.0, 1.0, 1.0, bias0]
    per = []
    best, min_cost = -1, np.finfo(np.float64).max
    for th_mult in range(1, 11):
        ivs = intervals_from_norms(norms, th_mult * norm_th, win)
        valid = extract(ivs, n_samps)
        rec = dict(th_mult=th_mult, intervals=ivs, valid=valid, num=len(valid), cost=np.nan, iterations=0, termination=TERM_SKIPPED)
        per.append(rec)
        if len(valid) < min_intervals or not valid:
            continue
        if acc_use_means:
            samples = np.array([data_mean(acc, a, b) for a, b in valid])
        else:
            samples = np.concatenate([acc[a:a + n_samps] for a, b in valid])

        def ev(p, samples=samples):
            r, J = acc_rows(samples, p, g_mag)
            c, H, g = normal_eq(r, J)
            return (c, H, g) if np.isfinite(c) else None
        x, c, it, term = lm(ev, x0)
        rec.update(params=x, cost=c, iterations=it, termination=term)
        if c < min_cost:
            min_cost, best = c, th_mult - 1
    out = dict(per_threshold=per, norm_th=norm_th, init_acc_bias=bias0, norms=norms)
    if best < 0:
        out.update(status=1, th_mult=-1, acc_params=np.r_[0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0],
                   gyro_params=np.r_[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0])
        return out
    pa = per[best]["params"]
    valid = per[best]["valid"]
    # static means of the calibrated accelerometer (only_means), normalised
    ms01, ms02, ms12 = -pa[0] * pa[4], pa[1] * pa[5], -pa[2] * pa[5]
    gv = []
    for a, b in valid:
        u = acc[a:b + 1] - pa[6:9]
        c = np.stack([(pa[3] * u[:, 0] + ms01 * u[:, 1]) + ms02 * u[:, 2], pa[4] * u[:, 1] + ms12 * u[:, 2], pa[5] * u[:, 2]], axis=1)
        m = seq_sum(c) / float(b - a + 1)
        gv.append(m / norm3(m))
    gs, ge = initial_interval(t, init_s)
    gb = data_mean(gyro, gs, ge)
    gw = gyro - gb
    ranges, t_idx = [], 0
    for k in range(len(valid) - 1):
        ts0, ts1 = t[valid[k][1]], t[valid[k + 1][0]]
        i0 = i1 = -1
        while t_idx < len(t):
            if i0 < 0:
                if t[t_idx] >= ts0:
                    i0 = t_idx
            elif t[t_idx] >= ts1:
                i1 = t_idx - 1
                break
            t_idx += 1
        ranges.append((i0, i1))
    gvs = np.array([np.r_[gv[k], gv[k + 1]] for k in range(len(valid) - 1)])
    npar = 12 if optimize_gyro_bias else 9

    def evg(p):
        full = np.zeros(12); full[6:9] = 1.0; full[:npar] = p
        r, J = gyro_blocks_eval(t, gw, ranges, gvs, full, optimize_gyro_bias, gyro_dt)
        c, H, g = normal_eq(r, J)
        return (c, H, g) if np.isfinite(c) else None
    x0g = np.r_[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0][:npar]
    xg, cg, itg, termg = lm(evg, x0g)
    gp = np.r_[xg[:9], gb + (xg[9:12] if optimize_gyro_bias else 0.0)]
    out.update(status=0, th_mult=best + 1, acc_params=pa, gyro_params=gp, gyro_ranges=ranges, gyro_versors=gvs, gyro_bias0=gb,
               gyro_samples=gw, gyro_cost=cg, gyro_iterations=itg, gyro_termination=termg)
    return out
