"""50-digit restatement of the static IMU calibration's residuals (core/static_imu_calibrator.h, utils/gyro_integration.h of the
reference), written from those sources and independent of the HIP unit and of static_imu_restatement.py:
  - MultiPosAccResidual g - |T K (x - b)| and its nine derivatives in closed form (checked against 50-digit central differences by
    test_static_imu_reference.py);
  - MultiPosGyroResidual on mpmath dual numbers (9 or 12 derivative columns), integrated in the REFERENCE's form -- RK4 with the
    quaternion normalised after every step -- not in the device's product form, so DESIGN.md 3.y deviation (2) is tested;
  - cost, gradient and Gram of the accelerometer problem as sums of the 50-digit rows.
A chain of RK4 steps is integrated once per (configuration, first sample) and extended on demand, so a test pays for its own
blocks only; the step classes of static_imu_cases.py share their first sample.

YARDSTICK: per case class the error of the float64 numpy restatement (static_imu_restatement.py: gyro_blocks_eval with
product_form=False; acc_rows and normal_eq) against the 50 digits -- the largest figure over the class, rounded up to one digit
and floored at one float64 epsilon.  Measured on the host by test_static_imu_reference.py, which asserts that a fresh measurement
lies within [1/4, 1] of the table.  The device is held to DEVICE_FACTOR x the table (test_gpu_static_imu_edges.py).

Figures:
  gyro/r   largest absolute error of a block's three residuals (differences of unit vectors)
  gyro/J   per block and column the largest absolute error over the three rows / the largest 50-digit magnitude of that column
           in that block; the largest over the columns.  A column that is zero at 50 digits must be zero (else: inf)
  acc/r    largest absolute residual error;  acc/J  per row, relative to the row's largest entry
  acc/H, acc/g, acc/cost   entrywise_error, gradient_error (normal_equations_reference.py) and the relative cost error"""
import functools

import mpmath as mp
import numpy as np

import static_imu_cases as K
from normal_equations_reference import DEVICE_FACTOR, LD, entrywise_error, gradient_error   # noqa: F401 (DEVICE_FACTOR: re-exported)

DPS = 50
EPS = float(np.finfo(np.float64).eps)


def at_dps(fn):
    """Run fn at DPS digits whatever the global precision is (other tests of the suite set their own)."""
    @functools.wraps(fn)
    def wrapped(*a, **kw):
        with mp.workdps(DPS):
            return fn(*a, **kw)
    return wrapped


YARDSTICK = {   # measured: the figure behind each entry
    "gyro/r/0a": 3e-16,      # 1.110e-16 (floored)
    "gyro/J/0a": 3e-16,      # 0
    "gyro/r/0b": 3e-16,      # 4.163e-17
    "gyro/J/0b": 3e-16,      # 0
    "gyro/r/1": 3e-16,       # 1.930e-16
    "gyro/J/1": 5e-16,       # 4.684e-16
    "gyro/r/2": 3e-16,       # 1.214e-16
    "gyro/J/2": 5e-16,       # 4.246e-16
    "gyro/r/255": 6e-16,     # 5.778e-16
    "gyro/J/255": 2e-13,     # 1.522e-13
    "gyro/r/256": 2e-15,     # 1.317e-15
    "gyro/J/256": 2e-14,     # 1.052e-14
    "gyro/r/257": 1e-15,     # 9.697e-16
    "gyro/J/257": 2e-14,     # 1.271e-14
    "gyro/r/513": 9e-16,     # 8.811e-16
    "gyro/J/513": 6e-15,     # 5.596e-15
    "gyro/r/end": 3e-16,     # 1.798e-16
    "gyro/J/end": 2e-15,     # 1.397e-15
    "acc/r": 4e-15,          # 3.250e-15
    "acc/J": 5e-16,          # 4.055e-16
    "acc/H/1": 9e-16, "acc/g/1": 2e-13, "acc/cost/1": 3e-13,          # 8.186e-16, 1.051e-13, 2.096e-13 (one residual of 1e-2 carries eps g)
    "acc/H/63": 4e-16, "acc/g/63": 3e-16, "acc/cost/63": 3e-16,       # 3.518e-16, 1.771e-16, 1.689e-16
    "acc/H/64": 4e-16, "acc/g/64": 3e-16, "acc/cost/64": 3e-16,       # 3.962e-16, 1.786e-16, 1.899e-16
    "acc/H/65": 5e-16, "acc/g/65": 3e-16, "acc/cost/65": 3e-16,       # 4.328e-16, 1.830e-16, 2.106e-16
    "acc/H/255": 7e-16, "acc/g/255": 5e-16, "acc/cost/255": 6e-16,    # 6.880e-16, 4.483e-16, 5.247e-16
    "acc/H/256": 8e-16, "acc/g/256": 5e-16, "acc/cost/256": 6e-16,    # 7.162e-16, 4.500e-16, 5.286e-16
    "acc/H/257": 8e-16, "acc/g/257": 5e-16, "acc/cost/257": 5e-16,    # 7.521e-16, 4.491e-16, 4.995e-16
    "acc/H/513": 1e-15, "acc/g/513": 7e-16, "acc/cost/513": 5e-16,    # 9.387e-16, 6.125e-16, 4.254e-16
}


def yardstick(key):
    return YARDSTICK[key]


def round_up(x):
    """x rounded up to one digit, floored at one float64 epsilon."""
    x = max(float(x), EPS)
    e = int(np.floor(np.log10(x)))
    m = int(np.ceil(x / 10.0 ** e - 1e-9))
    return float("%de%d" % (m, e)) if m < 10 else float("1e%d" % (e + 1))


def mpf(x):
    """A float64 exactly; an mpf as it is (the difference quotients of the tests pass p +- 1e-20)."""
    return x if isinstance(x, mp.mpf) else mp.mpf(float(x))


@at_dps
def to_ld(a):
    """mpf array -> np.longdouble (two float64 pieces: exact to 2^-106, rounded once to the 64-bit significand)."""
    a = np.asarray(a, dtype=object)
    hi = np.array([float(v) for v in a.ravel()])
    lo = np.array([float(v - mp.mpf(h)) for v, h in zip(a.ravel(), hi)])
    return (hi.astype(LD) + lo.astype(LD)).reshape(a.shape)


@at_dps
def abs_err(x, ref):
    """|x - ref| entry by entry, formed at 50 digits, as float64."""
    x = np.asarray(x, dtype=np.float64)
    ref = np.asarray(ref, dtype=object)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    return np.array([float(abs(mp.mpf(float(a)) - b)) for a, b in zip(x.ravel(), ref.ravel())]).reshape(x.shape)


# ---- accelerometer --------------------------------------------------------------------------------------------------------
@at_dps
def acc_residual(x, p, g_mag):
    """MultiPosAccResidual at 50 digits: g - |T K (x - b)|, T = [[1, -p0, p1], [0, 1, -p2], [0, 0, 1]], K = diag(p3..5), b = p6..8."""
    T = [[1, -p[0], p[1]], [0, 1, -p[2]], [0, 0, 1]]
    u = [x[k] - p[6 + k] for k in range(3)]
    c = [sum(T[i][j] * p[3 + j] * u[j] for j in range(3)) for i in range(3)]
    return g_mag - mp.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])


@at_dps
def acc_row(x, p, g_mag):
    """(r, [dr/dp0 .. dr/dp8]) at 50 digits, closed form: dr = -(c . dc) / |c|."""
    x, p, g_mag = [mpf(v) for v in x], [mpf(v) for v in p], mpf(g_mag)
    m0, m1, m2, sx, sy, sz = p[:6]
    u0, u1, u2 = x[0] - p[6], x[1] - p[7], x[2] - p[8]
    c = [sx * u0 - m0 * sy * u1 + m1 * sz * u2, sy * u1 - m2 * sz * u2, sz * u2]
    nrm = mp.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
    z = mp.mpf(0)
    dc = [[-sy * u1, z, z], [sz * u2, z, z], [z, -sz * u2, z], [u0, z, z], [-m0 * u1, u1, z], [m1 * u2, -m2 * u2, u2],
          [-sx, z, z], [m0 * sy, -sy, z], [-m1 * sz, m2 * sz, -sz]]
    return g_mag - nrm, [-(c[0] * d[0] + c[1] * d[1] + c[2] * d[2]) / nrm for d in dc]


@functools.lru_cache(maxsize=None)
@at_dps
def acc_reference(params_name):
    """(r [513], J [513][9]) object arrays of mpf for every sample of static_imu_cases.acc_samples()."""
    rows = [acc_row(x, K.ACC_PARAMS[params_name], K.G) for x in K.acc_samples()]
    return np.array([r for r, _ in rows], dtype=object), np.array([J for _, J in rows], dtype=object)


@functools.lru_cache(maxsize=None)
@at_dps
def acc_sums(params_name, count):
    """(cost, H [9][9], g [9]) of the first `count` samples: sums of the 50-digit rows, as np.longdouble."""
    r, J = acc_reference(params_name)
    r, J = r[:count], J[:count]
    cost = sum((v * v for v in r), mp.mpf(0)) / 2
    g = [sum((J[i, a] * r[i] for i in range(count)), mp.mpf(0)) for a in range(9)]
    H = [[sum((J[i, a] * J[i, b] for i in range(count)), mp.mpf(0)) for b in range(9)] for a in range(9)]
    return to_ld([cost])[0], to_ld(H), to_ld(g)


@at_dps
def acc_row_errors(r, J, params_name):
    """(acc/r, acc/J) of float64 rows of the leading samples."""
    ref_r, ref_J = acc_reference(params_name)
    n = len(r)
    er = abs_err(r, ref_r[:n])
    dj = abs_err(J, ref_J[:n])
    scale = np.array([[float(abs(v)) for v in row] for row in ref_J[:n]])
    zero = scale == 0
    assert not dj[zero].any(), "an entry that is zero at 50 digits is not zero"
    return float(er.max()), float((dj.max(axis=1) / scale.max(axis=1)).max())


@at_dps
def acc_sum_errors(cost, H, g, params_name, count):
    """(acc/H, acc/g, acc/cost)."""
    c_ref, H_ref, g_ref = acc_sums(params_name, count)
    return (entrywise_error(np.asarray(H), H_ref)[0], gradient_error(np.asarray(g), g_ref, H_ref, c_ref)[0],
            float(abs(LD(cost) - c_ref) / c_ref))


# ---- gyroscope: dual numbers [value, d/dp0, ...] as lists of mpf ------------------------------------------------------------
def jadd(a, b):
    return [x + y for x, y in zip(a, b)]


def jsub(a, b):
    return [x - y for x, y in zip(a, b)]


def jneg(a):
    return [-x for x in a]


def jscale(s, a):
    return [s * x for x in a]


def jmul(a, b):
    a0, b0 = a[0], b[0]
    return [a0 * b0] + [a0 * y + x * b0 for x, y in zip(a[1:], b[1:])]


def jconst(v, ncols):
    return [mp.mpf(v)] + [mp.mpf(0)] * ncols


@at_dps
def triad(p, ncols, optimize_bias):
    """(T K as 3 x 3 dual numbers, bias [3]) of ThreeAxisSensorCalibParams(p0 .. p11); derivative column k belongs to p[k]."""
    th = [jconst(mpf(p[k]), ncols) for k in range(12)]
    for k in range(ncols):
        th[k][1 + k] = mp.mpf(1)
    one, zero = jconst(1, ncols), jconst(0, ncols)
    # mis_mat << 1, -mis_yz, mis_zy, mis_xz, 1, -mis_zx, -mis_xy, mis_yx, 1 with (yz, zy, zx, xz, xy, yx) = p0 .. p5
    T = [[one, jneg(th[0]), th[1]], [th[3], one, jneg(th[2])], [jneg(th[4]), th[5], one]]
    ms = [[jmul(T[i][j], th[6 + j]) for j in range(3)] for i in range(3)]
    b = [th[9 + k] if optimize_bias else zero for k in range(3)]
    return ms, b


@at_dps
def unbias_normalize(ms, b, x, ncols):
    u = [jsub(jconst(mpf(x[k]), ncols), b[k]) for k in range(3)]
    return [jadd(jadd(jmul(ms[i][0], u[0]), jmul(ms[i][1], u[1])), jmul(ms[i][2], u[2])) for i in range(3)]


def half_omega_q(w, q):
    """0.5 * ComputeOmegaSkew(w) * q."""
    h = mp.mpf(0.5)
    return [jscale(h, jsub(jsub(jneg(jmul(w[0], q[1])), jmul(w[1], q[2])), jmul(w[2], q[3]))),
            jscale(h, jsub(jadd(jmul(w[0], q[0]), jmul(w[2], q[2])), jmul(w[1], q[3]))),
            jscale(h, jadd(jsub(jmul(w[1], q[0]), jmul(w[2], q[1])), jmul(w[0], q[3]))),
            jscale(h, jsub(jadd(jmul(w[2], q[0]), jmul(w[1], q[1])), jmul(w[0], q[2])))]


@at_dps
def rk4_step_normalised(q, w0, w1, dt):
    """QuatIntegrationStepRK4, NormalizeQuaternion included."""
    w01 = [jscale(mp.mpf(0.5), jadd(a, b)) for a, b in zip(w0, w1)]
    k1 = half_omega_q(w0, q)
    k2 = half_omega_q(w01, [jadd(a, jscale(dt / 2, k)) for a, k in zip(q, k1)])
    k3 = half_omega_q(w01, [jadd(a, jscale(dt / 2, k)) for a, k in zip(q, k2)])
    k4 = half_omega_q(w1, [jadd(a, jscale(dt, k)) for a, k in zip(q, k3)])
    m1, m2 = mp.mpf(1) / 6, mp.mpf(1) / 3
    qn = [jadd(a, jscale(dt, jadd(jadd(jscale(m1, x1), jscale(m2, x2)), jadd(jscale(m2, x3), jscale(m1, x4)))))
          for a, x1, x2, x3, x4 in zip(q, k1, k2, k3, k4)]
    n2 = jadd(jadd(jmul(qn[0], qn[0]), jmul(qn[1], qn[1])), jadd(jmul(qn[2], qn[2]), jmul(qn[3], qn[3])))
    s = mp.sqrt(n2[0])
    inv = [1 / s] + [-d / (2 * s * n2[0]) for d in n2[1:]]          # d (n2^-1/2) = -dn2 / (2 n2^3/2)
    return [jmul(a, inv) for a in qn]


@at_dps
def residual_of_quaternion(q, g0, g1, ncols):
    """rot^T g0 - g1 with rot = ceres::QuaternionToRotation(q) (scaled by 1 / |q|^2)."""
    a, b, c, d = q
    aa, ab, ac, ad, bb, bc, bd, cc, cd, dd = (jmul(a, a), jmul(a, b), jmul(a, c), jmul(a, d), jmul(b, b), jmul(b, c), jmul(b, d),
                                              jmul(c, c), jmul(c, d), jmul(d, d))
    two = mp.mpf(2)
    R = [[jsub(jsub(jadd(aa, bb), cc), dd), jscale(two, jsub(bc, ad)), jscale(two, jadd(ac, bd))],
         [jscale(two, jadd(ad, bc)), jsub(jadd(jsub(aa, bb), cc), dd), jscale(two, jsub(cd, ab))],
         [jscale(two, jsub(bd, ac)), jscale(two, jadd(ab, cd)), jadd(jsub(jsub(aa, bb), cc), dd)]]
    n2 = jadd(jadd(aa, bb), jadd(cc, dd))
    inv = [1 / n2[0]] + [-x / (n2[0] * n2[0]) for x in n2[1:]]
    out = []
    for i in range(3):
        v = jconst(0, ncols)
        for j in range(3):
            v = jadd(v, jscale(mpf(g0[j]), jmul(R[j][i], inv)))
        out.append(jsub(v, jconst(mpf(g1[i]), ncols)))
    return out


class Chain:
    """The quaternion after k steps from sample i0, k = 0, 1, ...: extended on demand, snapshots kept where asked for."""

    @at_dps
    def __init__(self, t, w, i0, p, optimize_bias, gyro_dt, ncols):
        self.t, self.w, self.i0, self.ncols, self.gyro_dt = t, w, i0, ncols, gyro_dt
        self.ms, self.b = triad(p, ncols, optimize_bias)
        self.q = [jconst(1, ncols), jconst(0, ncols), jconst(0, ncols), jconst(0, ncols)]
        self.k = 0
        self.omega = unbias_normalize(self.ms, self.b, w[i0], ncols) if i0 >= 0 else None
        self.kept = {0: self.q}

    @at_dps
    def after(self, steps, keep=()):
        assert steps in self.kept or steps >= self.k, "step %d was not kept" % steps
        while self.k < steps:
            s = self.i0 + self.k
            w1 = unbias_normalize(self.ms, self.b, self.w[s + 1], self.ncols)
            dt = mp.mpf(self.gyro_dt) if self.gyro_dt > 0 else mpf(self.t[s + 1]) - mpf(self.t[s])
            self.q = rk4_step_normalised(self.q, self.omega, w1, dt)
            self.omega = w1
            self.k += 1
            if self.k in keep or self.k == steps:
                self.kept[self.k] = self.q
        return self.kept[steps]


@at_dps
def gyro_block(t, w, i0, i1, g0, g1, p, optimize_bias=False, gyro_dt=-1.0, ncols=None):
    """(r [3], J [3][ncols]) of one MultiPosGyroResidual at 50 digits, from scratch (ncols 0: the residual alone)."""
    ncols = (12 if optimize_bias else 9) if ncols is None else ncols
    steps = i1 - i0 if i0 >= 0 and i1 > i0 else 0
    q = Chain(t, w, i0, p, optimize_bias, gyro_dt, ncols).after(steps)
    res = residual_of_quaternion(q, g0, g1, ncols)
    return [v[0] for v in res], [v[1:] for v in res]


_CHAINS = {}


@at_dps
def gyro_reference(config, cls):
    """(r [3], J [3][np]) object arrays of mpf for one case of static_imu_cases (cached; the chain is shared by the classes that
    start at the same sample)."""
    key = (config, cls)
    if key not in _CHAINS:
        series, p, ob, dt, classes = K.GYRO_CONFIGS[config]
        assert cls in classes
        t, w = K.gyro_series()[series]
        i0, i1 = K.GYRO_RANGES[cls]
        steps = K.gyro_steps(cls)
        ncols = 12 if ob else 9
        ck = ("chain", config, i0 if steps else -2)
        if ck not in _CHAINS:
            _CHAINS[ck] = Chain(t, w, i0 if steps else -1, p, ob, dt, ncols)
        keep = {K.gyro_steps(c) for c in classes if K.GYRO_RANGES[c][0] == i0}
        q = _CHAINS[ck].after(steps, keep)
        g0, g1 = K.gyro_versors()[cls]
        res = residual_of_quaternion(q, g0, g1, ncols)
        _CHAINS[key] = (np.array([v[0] for v in res], dtype=object), np.array([v[1:] for v in res], dtype=object))
    return _CHAINS[key]


@at_dps
def gyro_errors(r, J, config, cls):
    """(gyro/r, gyro/J) of one block's float64 residuals [3] and Jacobian [3][np]."""
    ref_r, ref_J = gyro_reference(config, cls)
    er = float(abs_err(r, ref_r).max())
    dj = abs_err(J, ref_J).max(axis=0)
    scale = np.array([max(float(abs(v)) for v in ref_J[:, c]) for c in range(ref_J.shape[1])])
    ej = 0.0
    for c in range(len(scale)):
        if scale[c] == 0:
            ej = max(ej, np.inf if dj[c] > 0 or np.asarray(J)[:, c].any() else 0.0)
        else:
            ej = max(ej, dj[c] / scale[c])
    return er, float(ej)


def gyro_config_errors(r, J, config):
    """{class: (gyro/r, gyro/J)} of an evaluation of all blocks of a configuration (r [3 b], J [3 b][np], the blocks in the order
    of static_imu_cases.gyro_inputs)."""
    classes = K.GYRO_CONFIGS[config][4]
    r = np.asarray(r).reshape(len(classes), 3)
    J = np.asarray(J).reshape(len(classes), 3, -1)
    return {cls: gyro_errors(r[b], J[b], config, cls) for b, cls in enumerate(classes)}
