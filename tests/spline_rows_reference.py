"""50-digit restatement of the spline calibration's residual rows (no GPU): what the right rows of a view corner, an accelerometer
sample and a gyroscope sample are.

Only the FORWARD model is restated, from the model definitions (the header comments of spline_math.h, spline_seg.h and block_items.h,
DESIGN.md section 4):

    blending matrices       the reference's closed formula (binomial sums), as exact fractions -- not kM6 / kMc6 / kM3
    u                       the exact rational ((t - start) mod dt) / dt of the integer times in ns; window = (t - start) // dt
    R(u), omega(u)          cumulative SO(3) B-spline of order 6:  R = R_0 prod_i exp(k_{i+1}(u) d_i),  d_i = log(R_i^-1 R_{i+1}),
                            omega_i = exp(k_{i+1} d_i)^-1 omega_{i-1} + k'_{i+1}(u) / dt  d_i        (body rate)
    p(u), p''(u)            R^3 B-spline of order 6 (value for views, second derivative for the accelerometer); order 3 for the biases
    view                    r = S (pi(R_ic^T (R_wi^T (X / X.w - t_wi) - t_ic)) - uv),  S = diag(1 / sqrt(cov))
                            quirk Q1: a rolling-shutter corner is evaluated at u + obs_v ld sh, sh = 1 or 1 / dt [1 / s] (option
                            rs_time_in_seconds), the window stays that of the view;  quirk Q2: a global-shutter view without
                            gs_unit_loss has zero residuals and rows;  a failed projection: residuals 1e10, zero rows
    accelerometer           r = w (R_wi^T (p''(u) + g) - MS (m - bias)),   MS = Mis Scale of imu_ms_matrix
    gyroscope               r = w (omega(u) - MS (m - bias))
    pi                      ba_rows_reference.project

and every Jacobian entry is a central difference of that model with step 1e-20, the quotient at 80 digits (STEP / STENCIL_DPS of
ba_rows_reference.py), along the tangent the library documents: SO(3) knots R_j <- R_j exp(eps); T_i_c <- T_i_c Exp([upsilon, omega])
(lm_retract.h: translation first; to first order d p_c = [-I | [p_c]x]); everything else additive, in the ABI column order of
oicc_evaluate_blocks (view 43, accelerometer 54, gyroscope 36; inactive columns zero).  No derivation is shared with the closed
forms under test.

Rotations: exp and log are the exact functions, the log's angle in (-pi, pi] (a function of the rotation, not of the quaternion's
sign).  The small-angle series of the code (squared_n < 1e-20 in the log, theta^2 < 1e-4 in the coefficient of Jr^-1, the axis of
identical knots) are numerical devices and are NOT restated.  One branch changes the function and is restated, for the VALUE:
Sophus' |w| < 1e-10 -> theta = +-pi.  Inside that sliver the constant-f branch has another derivative than the smooth log that the
device's closed form differentiates, so cases inside it compare RESIDUALS ONLY (spline_rows_cases: `residuals_only`).
`assert_clear_of_branches`: no function-changing decision -- the log's cut at pi (sign of w), the sliver, the camera models' own
branches, the failed projection -- flips when a parameter moves by 1e-12.

A problem is a dict (spline_rows_cases.make_problem): float64 / integer values, taken exactly.
"""
import math
from fractions import Fraction

import mpmath as mp
import numpy as np

import ba_rows_reference as B
from ba_rows_reference import LD, EPS, STEP, STENCIL_DPS, BRANCH_MARGIN, round_up_one_digit, _to_ld   # noqa: F401
from normal_equations_reference import DEVICE_FACTOR   # noqa: F401  (the device's allowance over a yardstick: the project's own)
from openimucameracalibrator_amd import estimator as E

NCOLS = {0: 43, 1: 54, 2: 36}
NROWS = {0: 2, 1: 3, 2: 3}
KIND_NAMES = {0: "view", 1: "accel", 2: "gyro"}
ROW_FLOOR = 1e-3            # a column below ROW_FLOOR x the largest column of its family in the item is scaled by that (a condition)
FLOOR_CAP = 0.25            # at most this share of the (item, column) pairs of the whole case table may sit on the floor
COST_BOUND = 1e-14
# column families of the three ABI layouts: name -> slice
FAMILIES = {0: {"so3": slice(0, 18), "r3": slice(18, 36), "tic_t": slice(36, 39), "tic_r": slice(39, 42), "ld": slice(42, 43)},
            1: {"so3": slice(0, 18), "r3": slice(18, 36), "gravity": slice(36, 39), "bias": slice(39, 48), "intr": slice(48, 54)},
            2: {"so3": slice(0, 18), "bias": slice(18, 27), "intr": slice(27, 36)}}


# ---- blending matrices: the reference's closed formula in exact fractions ---------------------------------------------------
def blending_matrix(n, cumulative):
    """M[i][k]: coefficient of u^k in the weight of control point i (order n), m(j, i) = C(n-1, n-1-i) sum_{s>=j} (-1)^(s-j)
    C(n, s-j) (n-s-1)^(n-1-i), rows summed from below for the cumulative form, over (n-1)!."""
    m = [[Fraction(0)] * n for _ in range(n)]
    for i in range(n):
        for j in range(n):
            s_ = sum(Fraction((-1) ** (s - j) * math.comb(n, s - j) * (n - s - 1) ** (n - 1 - i)) for s in range(j, n))
            m[j][i] = math.comb(n - 1, n - 1 - i) * s_
    if cumulative:
        for i in range(n):
            for j in range(i + 1, n):
                m[i] = [a + b for a, b in zip(m[i], m[j])]
    f = math.factorial(n - 1)
    return [[v / f for v in row] for row in m]


M6, MC6, M3 = blending_matrix(6, False), blending_matrix(6, True), blending_matrix(3, False)


def _coeffs(ctx, M, u, deriv, inv_dt):
    """sum_k M[i][k] d^deriv/du^deriv u^k * inv_dt^deriv"""
    n = len(M)
    out = []
    for i in range(n):
        s = 0
        for k in range(deriv, n):
            if M[i][k] == 0:
                continue
            f = math.perm(k, deriv)
            s = s + (ctx.mpf(M[i][k].numerator) / M[i][k].denominator) * f * u ** (k - deriv)
        out.append(s * inv_dt ** deriv)
    return out


# ---- quaternions (x, y, z, w); `ctx` is mpmath.mp (50 / 80 digits) or mpmath.fp (float64: placing cases, branch margins) --------
def qmul(a, b):
    return [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
            a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
            a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
            a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]


def qconj(q):
    return [-q[0], -q[1], -q[2], q[3]]


def qunit(ctx, q):
    n = ctx.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [v / n for v in q]


def qexp(ctx, v):
    t2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    if t2 == 0:
        return [0, 0, 0, 1]
    t = ctx.sqrt(t2)
    s = ctx.sin(t / 2) / t
    return [s * v[0], s * v[1], s * v[2], ctx.cos(t / 2)]


def qlog(ctx, q, branches=None):
    """The rotation vector of the unit quaternion q, angle in (-pi, pi]; |w| < 1e-10: Sophus' +-pi (module docstring)."""
    x, y, z, w = q
    n2 = x * x + y * y + z * z
    sliver = bool(abs(w) < 1e-10)
    if branches is not None:
        branches.append((bool(w > 0), sliver))
    if n2 == 0:
        return [0, 0, 0]
    n = ctx.sqrt(n2)
    if sliver:
        th = ctx.pi if w > 0 else -ctx.pi
    else:
        th = 2 * ctx.atan(n / w)
    f = th / n
    return [f * x, f * y, f * z]


def qmatrix(q):
    x, y, z, w = q
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]


def mat_tvec(R, v):
    return [R[0][i] * v[0] + R[1][i] * v[1] + R[2][i] * v[2] for i in range(3)]


def mat_vec(R, v):
    return [R[i][0] * v[0] + R[i][1] * v[1] + R[i][2] * v[2] for i in range(3)]


_seg_cache = {}
_rot_cache = {}


def _segment(ctx, q0, q1, branches):
    if ctx is not mp.mp or branches is not None:
        return qlog(ctx, qunit(ctx, qmul(qconj(q0), q1)), branches)
    key = (mp.mp.prec, q0, q1)
    d = _seg_cache.get(key)
    if d is None:
        if len(_seg_cache) > 20000:
            _seg_cache.clear()
        d = _seg_cache[key] = qlog(ctx, qunit(ctx, qmul(qconj(q0), q1)))
    return d


def so3_spline(ctx, knots, u, inv_dt, branches=None):
    """(unit quaternion R(u), body rate omega(u)) of the window of six knots (tuples x, y, z, w)."""
    key = None
    if ctx is mp.mp and branches is None:
        key = (mp.mp.prec, knots, u, inv_dt)
        hit = _rot_cache.get(key)
        if hit is not None:
            return hit
    k = _coeffs(ctx, MC6, u, 0, 1)
    dk = _coeffs(ctx, MC6, u, 1, inv_dt)
    q = qunit(ctx, list(knots[0]))
    w = [0, 0, 0]
    for i in range(5):
        d = _segment(ctx, knots[i], knots[i + 1], branches)
        e = qexp(ctx, [k[i + 1] * d[0], k[i + 1] * d[1], k[i + 1] * d[2]])
        q = qmul(q, e)
        w = mat_tvec(qmatrix(e), w)
        w = [w[c] + d[c] * dk[i + 1] for c in range(3)]
    out = (qunit(ctx, q), w)
    if key is not None:
        if len(_rot_cache) > 20000:
            _rot_cache.clear()
        _rot_cache[key] = out
    return out


def r3_spline(ctx, knots, u, deriv, inv_dt):
    c = _coeffs(ctx, M6, u, deriv, inv_dt)
    return [sum(c[j] * knots[j][e] for j in range(6)) for e in range(3)]


def imu_ms(intr, kind):
    """Mis Scale (imu_ms_matrix): accelerometer [yz zy zx | sx sy sz] (lower triangle zero), gyroscope [yz zy zx xz xy yx | sx sy sz]."""
    mis = list(intr[:3]) + [0, 0, 0] if kind == 1 else list(intr[:6])
    sc = intr[3:6] if kind == 1 else intr[6:9]
    return [[sc[0], -mis[0] * sc[1], mis[1] * sc[2]], [mis[3] * sc[0], sc[1], -mis[2] * sc[2]], [-mis[4] * sc[0], mis[5] * sc[1], sc[2]]]


# ---- state: the parameters of a problem as context numbers ----------------------------------------------------------------------
def _num(ctx, a):
    return tuple(ctx.mpf(float(v)) for v in a)


def state_of(ctx, P):
    return dict(so3=tuple(_num(ctx, q) for q in P["so3"]), r3=tuple(_num(ctx, p) for p in P["r3"]),
                tic_q=_num(ctx, P["T_i_c"][:4]), tic_t=_num(ctx, P["T_i_c"][4:]), g=_num(ctx, P["g"]), ld=ctx.mpf(float(P["ld"])),
                acc_intr=_num(ctx, P["acc_intr"]), gyr_intr=_num(ctx, P["gyr_intr"]), intr=_num(ctx, P["intr"]),
                ab=tuple(_num(ctx, P["ab"]) for _ in range(P["n_bias"])), gb=tuple(_num(ctx, P["gb"]) for _ in range(P["n_bias"])),
                points=tuple(_num(ctx, X) for X in P["points"]))


def _replace(t, i, v):
    return t[:i] + (v,) + t[i + 1:]


def bumped(ctx, S, name, i, c, h):
    """The state with one tangent coordinate moved by h: name in so3 / tic_r (right increments), tic_t (t + R upsilon), the rest additive."""
    S = dict(S)
    e = [h if k == c else 0 for k in range(3)]
    if name == "so3":
        S["so3"] = _replace(S["so3"], i, tuple(qmul(S["so3"][i], qexp(ctx, e))))
    elif name == "tic_r":
        S["tic_q"] = tuple(qmul(S["tic_q"], qexp(ctx, e)))
    elif name == "tic_t":
        d = mat_vec(qmatrix(qunit(ctx, list(S["tic_q"]))), e)
        S["tic_t"] = tuple(S["tic_t"][k] + d[k] for k in range(3))
    elif name == "ld":
        S["ld"] = S["ld"] + h
    elif name in ("r3", "ab", "gb"):
        S[name] = _replace(S[name], i, _replace(S[name][i], c, S[name][i][c] + h))
    else:
        S[name] = _replace(S[name], c, S[name][c] + h)
    return S


def window(P, t_ns, dt_ns):
    """(first knot, exact u as a fraction) of time t."""
    st = int(t_ns) - int(P["start_ns"])
    assert st >= 0
    return st // int(dt_ns), Fraction(st % int(dt_ns), int(dt_ns))


def _frac(ctx, f):
    return ctx.mpf(f.numerator) / f.denominator


class FailedProjection(Exception):
    pass


def view_residual(ctx, P, S, v, c, branches=None):
    """The two residuals of corner c of view v (unweighted views: zeros; raises FailedProjection)."""
    view = P["views"][v]
    if not (view["rs"] or P["options"].get("gs_unit_loss", 0)):
        return [ctx.mpf(0), ctx.mpf(0)]
    s_s, u_s = window(P, view["t_ns"], P["dt_so3_ns"])
    s_r, u_r = window(P, view["t_ns"], P["dt_r3_ns"])
    inv_s, inv_r = ctx.mpf(10 ** 9) / int(P["dt_so3_ns"]), ctx.mpf(10 ** 9) / int(P["dt_r3_ns"])
    uv = _num(ctx, view["uv"][c])
    tau = uv[1] * S["ld"] if view["rs"] else 0
    secs = bool(P["options"].get("rs_time_in_seconds", 0))
    us = _frac(ctx, u_s) + tau * (inv_s if secs else 1)
    ur = _frac(ctx, u_r) + tau * (inv_r if secs else 1)
    q, _ = so3_spline(ctx, S["so3"][s_s:s_s + 6], us, inv_s, branches)
    t = r3_spline(ctx, S["r3"][s_r:s_r + 6], ur, 0, inv_r)
    X = S["points"][int(view["point_ids"][c])]
    a = [X[k] / X[3] - t[k] for k in range(3)]
    b = mat_tvec(qmatrix(q), a)
    b = [b[k] - S["tic_t"][k] for k in range(3)]
    p = mat_tvec(qmatrix(qunit(ctx, list(S["tic_q"]))), b)
    try:
        px = B.project(ctx, int(P["cam_model"]), list(S["intr"]), p, branches)
    except B.OutsideDomain:
        raise FailedProjection()
    cov = _num(ctx, view["cov"][c])
    return [(px[0] - uv[0]) / ctx.sqrt(cov[0]), (px[1] - uv[1]) / ctx.sqrt(cov[1])]


def imu_parts(ctx, P, S, kind, i, branches=None):
    """(prediction, MS (m - bias)) of sample i: kind 1 accelerometer, 2 gyroscope."""
    samples = P["acc"] if kind == 1 else P["gyr"]
    t_ns = samples["t_ns"][i]
    s_s, u_s = window(P, t_ns, P["dt_so3_ns"])
    inv_s, inv_r = ctx.mpf(10 ** 9) / int(P["dt_so3_ns"]), ctx.mpf(10 ** 9) / int(P["dt_r3_ns"])
    q, om = so3_spline(ctx, S["so3"][s_s:s_s + 6], _frac(ctx, u_s), inv_s, branches)
    if kind == 1:
        s_r, u_r = window(P, t_ns, P["dt_r3_ns"])
        a = r3_spline(ctx, S["r3"][s_r:s_r + 6], _frac(ctx, u_r), 2, inv_r)
        pred = mat_tvec(qmatrix(q), [a[k] + S["g"][k] for k in range(3)])
    else:
        pred = om
    s_b, u_b = window(P, t_ns, P["dt_bias_ns"])
    cb = _coeffs(ctx, M3, _frac(ctx, u_b), 0, 1)
    knots = S["ab" if kind == 1 else "gb"]
    m = _num(ctx, samples["meas"][i])
    d = [m[e] - sum(cb[k] * knots[s_b + k][e] for k in range(3)) for e in range(3)]
    return pred, mat_vec(imu_ms(S["acc_intr" if kind == 1 else "gyr_intr"], kind), d)


def imu_residual(ctx, P, S, kind, i, branches=None):
    pred, un = imu_parts(ctx, P, S, kind, i, branches)
    w = ctx.mpf(float(P["w_acc" if kind == 1 else "w_gyr"]))
    return [w * (pred[k] - un[k]) for k in range(3)]


# ---- items and their columns -------------------------------------------------------------------------------------------------------
def items(P, kind):
    """[(view, corner)] in dump order, or the sample indices."""
    if kind == 0:
        return [(v, c) for v, view in enumerate(P["views"]) for c in range(len(view["uv"]))]
    return list(range(len((P["acc"] if kind == 1 else P["gyr"])["t_ns"])))


def _item_time(P, kind, it):
    return P["views"][it[0]]["t_ns"] if kind == 0 else (P["acc"] if kind == 1 else P["gyr"])["t_ns"][it]


def column_parameters(P, kind, it):
    """The parameter (name, index, component) of every ABI column of the item."""
    t = _item_time(P, kind, it)
    s_s = window(P, t, P["dt_so3_ns"])[0]
    cols = [("so3", s_s + j, c) for j in range(6) for c in range(3)]
    if kind != 2:
        s_r = window(P, t, P["dt_r3_ns"])[0]
        cols += [("r3", s_r + j, c) for j in range(6) for c in range(3)]
    if kind == 0:
        cols += [("tic_t", 0, c) for c in range(3)] + [("tic_r", 0, c) for c in range(3)] + [("ld", 0, 0)]
    else:
        s_b = window(P, t, P["dt_bias_ns"])[0]
        if kind == 1:
            cols += [("g", 0, c) for c in range(3)]
        cols += [("ab" if kind == 1 else "gb", s_b + k, c) for k in range(3) for c in range(3)]
        cols += [("acc_intr", 0, c) for c in range(6)] if kind == 1 else [("gyr_intr", 0, c) for c in range(9)]
    assert len(cols) == NCOLS[kind]
    return cols


def active_columns(P, kind, flags):
    """Boolean [NCOLS]: SetFixedParams as the library implements it (a line delay of exactly 0 stays variable whatever the flag)."""
    act = np.zeros(NCOLS[kind], bool)
    spline = bool(flags & E.SPLINE)
    act[0:18] = spline
    if kind == 0:
        act[18:36] = spline
        act[36:42] = bool(flags & E.T_I_C)
        has_rs = any(v["rs"] for v in P["views"])
        act[42] = has_rs and (bool(flags & E.CAM_LINE_DELAY) if float(P["ld"]) != 0.0 else True)
    elif kind == 1:
        act[18:36] = spline
        act[36:39] = bool(flags & E.GRAVITY_DIR)
        act[39:48] = bool(flags & (E.ACC_BIAS | E.IMU_BIASES))
        act[48:54] = bool(flags & E.IMU_INTRINSICS)
    else:
        act[18:27] = bool(flags & (E.GYR_BIAS | E.IMU_BIASES))
        act[27:36] = bool(flags & E.IMU_INTRINSICS)
    return act


def _residual(ctx, P, S, kind, it, branches=None):
    return view_residual(ctx, P, S, it[0], it[1], branches) if kind == 0 else imu_residual(ctx, P, S, kind, it, branches)


_rows_cache = {}


def full_rows(P, kind):
    """(r, J) of every item with every column differentiated (long double); failed / unweighted corners: zero rows."""
    key = (P["name"], kind)
    if key in _rows_cache:
        return _rows_cache[key]
    with mp.workdps(STENCIL_DPS):
        S = state_of(mp.mp, P)
        res, jac = [], []
        for it in items(P, kind):
            nr = NROWS[kind]
            weighted = kind != 0 or P["views"][it[0]]["rs"] or bool(P["options"].get("gs_unit_loss", 0))
            try:
                r0 = _residual(mp.mp, P, S, kind, it)
            except FailedProjection:
                r0, weighted = [mp.mpf(10) ** 10] * nr, False
            cols = []
            for name, i, c in column_parameters(P, kind, it):
                if not weighted or (name == "ld" and not P["views"][it[0]]["rs"]):
                    cols.append([mp.mpf(0)] * nr)
                    continue
                a = _residual(mp.mp, P, bumped(mp.mp, S, name, i, c, STEP), kind, it)
                b = _residual(mp.mp, P, bumped(mp.mp, S, name, i, c, -STEP), kind, it)
                cols.append([(a[e] - b[e]) / (2 * STEP) for e in range(nr)])
            for e in range(nr):
                res.append(_to_ld(r0[e]))
                jac.append([_to_ld(col[e]) for col in cols])
    out = (np.array(res, dtype=LD), np.array(jac, dtype=LD).reshape(len(res), NCOLS[kind]))
    _rows_cache[key] = out
    return out


def rows(P, kind, flags):
    """(r, J) in np.longdouble in the ABI layout of oicc_evaluate_blocks; inactive columns zero."""
    r, J = full_rows(P, kind)
    J = J.copy()
    J[:, ~active_columns(P, kind, flags)] = 0
    return r.copy(), J


class RowsBackend:
    """What normal_equations_reference.assemble needs of a `rows_backend`: the 50-digit rows behind EvaluateBlocks."""

    def __init__(self, P):
        self.P = P
        self.trajectory_ = self
        self.num_corners = sum(len(v["uv"]) for v in P["views"])

    def EvaluateBlocks(self, flags, kind, n_rows):
        r, J = rows(self.P, kind, flags)
        assert n_rows == len(r)
        return r, J


def residual_scales(P, kind):
    """Per residual row, in float64: S (|pi| + |uv|) for views, w (|prediction| + |MS (m - bias)|) for the IMU families (what the
    residual's rounding is relative to); 1e10 for a failed projection and 1 for an unweighted view (the residual is exact there)."""
    S = state_of(mp.fp, P)
    out = []
    for it in items(P, kind):
        if kind == 0:
            view = P["views"][it[0]]
            uv, cov = view["uv"][it[1]], view["cov"][it[1]]
            try:
                r = view_residual(mp.fp, P, S, it[0], it[1])
            except FailedProjection:
                out += [1e10, 1e10]
                continue
            if not (view["rs"] or P["options"].get("gs_unit_loss", 0)):
                out += [1.0, 1.0]
                continue
            for e in range(2):
                isd = 1.0 / math.sqrt(cov[e])
                out.append(abs(r[e] + isd * uv[e]) + isd * abs(uv[e]))
        else:
            pred, un = imu_parts(mp.fp, P, S, kind, it)
            w = float(P["w_acc" if kind == 1 else "w_gyr"])
            out += [w * (abs(pred[e]) + abs(un[e])) for e in range(3)]
    return np.array(out, dtype=np.float64)


# ---- branches ------------------------------------------------------------------------------------------------------------------------
def _signature(P, S):
    sig = []
    for kind in (0, 1, 2):
        for it in items(P, kind):
            b = []
            try:
                _residual(mp.fp, P, S, kind, it, b)
                b.append("ok")
            except FailedProjection:
                b.append("failed")
            sig.append(tuple(b))
    return sig


def assert_clear_of_branches(P):
    """No function-changing decision of any item -- sign of w and the sliver of every segment log of its window, the camera model's
    branches, the failed projection -- within BRANCH_MARGIN of the case along any parameter that is differentiated."""
    S = state_of(mp.fp, P)
    base = _signature(P, S)
    params = set()
    for kind in (0, 1, 2):
        for it in items(P, kind):
            params.update(p for p in column_parameters(P, kind, it) if p[0] in ("so3", "r3", "tic_t", "tic_r", "ld"))
    for name, i, c in sorted(params):
        for h in (BRANCH_MARGIN, -BRANCH_MARGIN):
            assert _signature(P, bumped(mp.fp, S, name, i, c, h)) == base, "%s: within %g of a branch along %s %d [%d]" % (P["name"], BRANCH_MARGIN, name, i, c)


# ---- the measure ----------------------------------------------------------------------------------------------------------------------
def row_figures(P, kind, r, J, r_ref, J_ref, want_jacobian=True):
    """dict(residual, family, column): the largest of the three figures over the items of the kind (module docstring of
    spline_rows_cases / DESIGN.md section 6), and the number of (item, column) pairs (on the floor, in all)."""
    nr = NROWS[kind]
    scale = residual_scales(P, kind)
    fig = dict(residual=float((np.abs(np.asarray(r).astype(LD) - r_ref).astype(np.float64) / scale).max()) if len(r_ref) else 0.0,
               family=0.0, column=0.0)
    on_floor = pairs = 0
    if not want_jacobian:
        return fig, (0, 0)
    for k in range(len(r_ref) // nr):
        Jk, Rk = np.asarray(J)[nr * k:nr * k + nr].astype(LD), J_ref[nr * k:nr * k + nr]
        diff = np.abs(Jk - Rk).astype(np.float64)
        norms = np.sqrt((Rk.astype(np.float64) ** 2).sum(axis=0))
        for name, sl in FAMILIES[kind].items():
            F = float(norms[sl].max())
            if F == 0.0:
                assert not Jk[:, sl].any(), "%s %s item %d: nonzero entries in the inactive family %s" % (P["name"], KIND_NAMES[kind], k, name)
                continue
            fig["family"] = max(fig["family"], float(diff[:, sl].max()) / F)
            den = np.maximum(norms[sl], ROW_FLOOR * F)
            fig["column"] = max(fig["column"], float((diff[:, sl].max(axis=0) / den).max()))
            on_floor += int((norms[sl] < ROW_FLOOR * F).sum())
            pairs += len(norms[sl])
    return fig, (on_floor, pairs)


def cost_at(P, so3=None, r3=None, others=None):
    """50-digit cost 1/2 sum r^2 of the problem, optionally at other knots / parameters (dict of problem fields)."""
    Q = dict(P)
    if so3 is not None:
        Q["so3"] = so3
    if r3 is not None:
        Q["r3"] = r3
    Q.update(others or {})
    S = state_of(mp.mp, Q)
    total = mp.mpf(0)
    for kind in (0, 1, 2):
        for it in items(Q, kind):
            try:
                r = _residual(mp.mp, Q, S, kind, it)
            except FailedProjection:
                r = [mp.mpf(10) ** 10] * 2
            total += sum(v * v for v in r) / 2
    return _to_ld(total)


# Figures of the Jet oracle's float64 rows against the 50-digit rows per case, kind and figure -- residual, family-relative,
# column-relative (row_figures) -- and "ne": the entry-wise error (the larger of H's and g's, every entry by its own d_i d_j) of a
# float64 assembly of the Jet oracle's rows against the long-double assembly of the 50-digit rows, blocks shuffled, the largest of
# three seeds.  Each rounded up to one digit behind the measured figure; test_spline_rows_reference.py asserts that a fresh measurement
# lies within [1/8, 1] of it.  Every case carries its own figure: the Jets lose no digits at any of these edges (over the whole table
# residuals 1.3e-16 ... 3.4e-15, family-relative 3e-16 ... 2e-15 and 1.3e-14 for the division model's literal quotient,
# column-relative -- set by the columns on the floor -- 1e-15 ... 1e-12, "ne" 7e-16 ... 9e-13), so none is borrowed.  An entry of 0
# is a kind without an active column under the case's flags: exactly zero rows.  The device and the host compile of its closed
# forms are allowed DEVICE_FACTOR x the figure.
YARDSTICK = {
    "generic/view/residual": 3e-16,    # 2.17e-16
    "generic/view/family": 2e-15,    # 1.06e-15
    "generic/view/column": 7e-13,    # 6.41e-13
    "generic/accel/residual": 2e-16,    # 1.48e-16
    "generic/accel/family": 6e-16,    # 5.52e-16
    "generic/accel/column": 4e-13,    # 3.98e-13
    "generic/gyro/residual": 3e-16,    # 2.61e-16
    "generic/gyro/family": 8e-16,    # 7.52e-16
    "generic/gyro/column": 7e-14,    # 6.20e-14
    "generic/ne": 7e-13,    # 6.42e-13
    "generic_division/view/residual": 4e-15,    # 3.01e-15
    "generic_division/view/family": 2e-14,    # 1.25e-14
    "generic_division/view/column": 7e-13,    # 6.91e-13
    "generic_division/accel/residual": 2e-16,    # 1.48e-16
    "generic_division/accel/family": 6e-16,    # 5.52e-16
    "generic_division/accel/column": 4e-13,    # 3.98e-13
    "generic_division/gyro/residual": 3e-16,    # 2.61e-16
    "generic_division/gyro/family": 8e-16,    # 7.52e-16
    "generic_division/gyro/column": 7e-14,    # 6.20e-14
    "generic_division/ne": 8e-13,    # 7.07e-13
    "theta0/view/residual": 4e-16,    # 3.45e-16
    "theta0/view/family": 9e-16,    # 8.75e-16
    "theta0/view/column": 7e-13,    # 6.35e-13
    "theta0/accel/residual": 3e-16,    # 2.52e-16
    "theta0/accel/family": 7e-16,    # 6.54e-16
    "theta0/accel/column": 4e-13,    # 3.24e-13
    "theta0/gyro/residual": 6e-16,    # 5.50e-16
    "theta0/gyro/family": 4e-16,    # 3.37e-16
    "theta0/gyro/column": 7e-14,    # 6.23e-14
    "theta0/ne": 7e-13,    # 6.43e-13
    "static/view/residual": 2e-16,    # 1.77e-16
    "static/view/family": 7e-16,    # 6.77e-16
    "static/view/column": 4e-13,    # 3.61e-13
    "static/accel/residual": 4e-16,    # 3.69e-16
    "static/accel/family": 8e-16,    # 7.55e-16
    "static/accel/column": 3e-13,    # 2.23e-13
    "static/gyro/residual": 2e-16,    # 2.00e-16
    "static/gyro/family": 4e-16,    # 3.02e-16
    "static/gyro/column": 7e-14,    # 6.35e-14
    "static/ne": 3e-13,    # 2.25e-13
    "t1e-12/view/residual": 3e-16,    # 2.48e-16
    "t1e-12/view/family": 2e-15,    # 1.13e-15
    "t1e-12/view/column": 7e-13,    # 6.79e-13
    "t1e-12/accel/residual": 4e-16,    # 3.37e-16
    "t1e-12/accel/family": 1e-15,    # 9.94e-16
    "t1e-12/accel/column": 4e-13,    # 3.28e-13
    "t1e-12/gyro/residual": 4e-16,    # 3.77e-16
    "t1e-12/gyro/family": 7e-16,    # 6.99e-16
    "t1e-12/gyro/column": 7e-14,    # 6.23e-14
    "t1e-12/ne": 7e-13,    # 6.43e-13
    "t1.9e-10/view/residual": 5e-16,    # 4.23e-16
    "t1.9e-10/view/family": 9e-16,    # 8.75e-16
    "t1.9e-10/view/column": 7e-13,    # 6.34e-13
    "t1.9e-10/accel/residual": 5e-16,    # 4.45e-16
    "t1.9e-10/accel/family": 9e-16,    # 8.87e-16
    "t1.9e-10/accel/column": 3e-13,    # 2.74e-13
    "t1.9e-10/gyro/residual": 3e-16,    # 2.54e-16
    "t1.9e-10/gyro/family": 6e-16,    # 5.91e-16
    "t1.9e-10/gyro/column": 7e-14,    # 6.23e-14
    "t1.9e-10/ne": 7e-13,    # 6.43e-13
    "t2.1e-10/view/residual": 3e-16,    # 2.53e-16
    "t2.1e-10/view/family": 2e-15,    # 1.25e-15
    "t2.1e-10/view/column": 7e-13,    # 6.35e-13
    "t2.1e-10/accel/residual": 5e-16,    # 4.51e-16
    "t2.1e-10/accel/family": 9e-16,    # 8.89e-16
    "t2.1e-10/accel/column": 3e-13,    # 2.70e-13
    "t2.1e-10/gyro/residual": 3e-16,    # 2.95e-16
    "t2.1e-10/gyro/family": 5e-16,    # 4.51e-16
    "t2.1e-10/gyro/column": 7e-14,    # 6.23e-14
    "t2.1e-10/ne": 7e-13,    # 6.44e-13
    "t1e-6/view/residual": 3e-16,    # 2.27e-16
    "t1e-6/view/family": 2e-15,    # 1.28e-15
    "t1e-6/view/column": 7e-13,    # 6.35e-13
    "t1e-6/accel/residual": 4e-16,    # 3.51e-16
    "t1e-6/accel/family": 2e-15,    # 1.03e-15
    "t1e-6/accel/column": 3e-13,    # 2.70e-13
    "t1e-6/gyro/residual": 4e-16,    # 3.74e-16
    "t1e-6/gyro/family": 7e-16,    # 6.41e-16
    "t1e-6/gyro/column": 7e-14,    # 6.23e-14
    "t1e-6/ne": 7e-13,    # 6.43e-13
    "t0.0099/view/residual": 6e-16,    # 5.06e-16
    "t0.0099/view/family": 2e-15,    # 1.27e-15
    "t0.0099/view/column": 7e-13,    # 6.34e-13
    "t0.0099/accel/residual": 3e-16,    # 2.07e-16
    "t0.0099/accel/family": 2e-15,    # 1.04e-15
    "t0.0099/accel/column": 3e-13,    # 2.79e-13
    "t0.0099/gyro/residual": 4e-16,    # 3.54e-16
    "t0.0099/gyro/family": 7e-16,    # 6.03e-16
    "t0.0099/gyro/column": 7e-14,    # 6.23e-14
    "t0.0099/ne": 7e-13,    # 6.43e-13
    "t0.0101/view/residual": 4e-16,    # 3.89e-16
    "t0.0101/view/family": 1e-15,    # 9.93e-16
    "t0.0101/view/column": 7e-13,    # 6.35e-13
    "t0.0101/accel/residual": 5e-16,    # 4.01e-16
    "t0.0101/accel/family": 1e-15,    # 9.99e-16
    "t0.0101/accel/column": 3e-13,    # 2.71e-13
    "t0.0101/gyro/residual": 3e-16,    # 2.18e-16
    "t0.0101/gyro/family": 9e-16,    # 8.28e-16
    "t0.0101/gyro/column": 7e-14,    # 6.23e-14
    "t0.0101/ne": 7e-13,    # 6.43e-13
    "pi-1e-6/view/residual": 2e-15,    # 1.13e-15
    "pi-1e-6/view/family": 1e-15,    # 9.37e-16
    "pi-1e-6/view/column": 6e-13,    # 5.95e-13
    "pi-1e-6/accel/residual": 9e-16,    # 8.56e-16
    "pi-1e-6/accel/family": 9e-16,    # 8.45e-16
    "pi-1e-6/accel/column": 4e-13,    # 3.31e-13
    "pi-1e-6/gyro/residual": 4e-16,    # 3.49e-16
    "pi-1e-6/gyro/family": 6e-16,    # 5.43e-16
    "pi-1e-6/gyro/column": 4e-14,    # 3.71e-14
    "pi-1e-6/ne": 6e-13,    # 5.61e-13
    "pi+1e-6/view/residual": 2e-15,    # 1.05e-15
    "pi+1e-6/view/family": 2e-15,    # 1.47e-15
    "pi+1e-6/view/column": 8e-13,    # 7.14e-13
    "pi+1e-6/accel/residual": 2e-15,    # 1.88e-15
    "pi+1e-6/accel/family": 1e-15,    # 9.60e-16
    "pi+1e-6/accel/column": 4e-13,    # 3.98e-13
    "pi+1e-6/gyro/residual": 3e-16,    # 2.13e-16
    "pi+1e-6/gyro/family": 4e-16,    # 3.20e-16
    "pi+1e-6/gyro/column": 4e-14,    # 3.37e-14
    "pi+1e-6/ne": 6e-13,    # 5.71e-13
    "pi-1e-11/view/residual": 2e-15,    # 1.80e-15
    "pi-1e-11/accel/residual": 2e-15,    # 1.01e-15
    "pi-1e-11/gyro/residual": 4e-16,    # 3.10e-16
    "t0.7_negated/view/residual": 6e-16,    # 5.12e-16
    "t0.7_negated/view/family": 1e-15,    # 9.50e-16
    "t0.7_negated/view/column": 7e-13,    # 6.16e-13
    "t0.7_negated/accel/residual": 5e-16,    # 4.30e-16
    "t0.7_negated/accel/family": 2e-15,    # 1.11e-15
    "t0.7_negated/accel/column": 3e-13,    # 2.49e-13
    "t0.7_negated/gyro/residual": 5e-16,    # 4.24e-16
    "t0.7_negated/gyro/family": 8e-16,    # 7.21e-16
    "t0.7_negated/gyro/column": 6e-14,    # 5.95e-14
    "t0.7_negated/ne": 7e-13,    # 6.38e-13
    "generic/knot_times/view/residual": 2e-16,    # 1.64e-16
    "generic/knot_times/view/family": 2e-15,    # 1.54e-15
    "generic/knot_times/view/column": 1e-12,    # 9.65e-13
    "generic/knot_times/accel/residual": 2e-15,    # 1.36e-15
    "generic/knot_times/accel/family": 3e-15,    # 2.03e-15
    "generic/knot_times/accel/column": 5e-13,    # 4.11e-13
    "generic/knot_times/gyro/residual": 3e-16,    # 2.68e-16
    "generic/knot_times/gyro/family": 7e-16,    # 6.96e-16
    "generic/knot_times/gyro/column": 3e-14,    # 2.63e-14
    "generic/knot_times/ne": 5e-15,    # 4.48e-15
    "static/knot_times/view/residual": 2e-16,    # 1.26e-16
    "static/knot_times/view/family": 3e-15,    # 2.02e-15
    "static/knot_times/view/column": 4e-13,    # 3.38e-13
    "static/knot_times/accel/residual": 4e-15,    # 3.43e-15
    "static/knot_times/accel/family": 2e-15,    # 1.95e-15
    "static/knot_times/accel/column": 2e-13,    # 1.37e-13
    "static/knot_times/gyro/residual": 2e-16,    # 2.00e-16
    "static/knot_times/gyro/family": 5e-16,    # 4.04e-16
    "static/knot_times/gyro/column": 3e-13,    # 2.52e-13
    "static/knot_times/ne": 3e-15,    # 2.72e-15
    "generic/56_128/view/residual": 3e-16,    # 2.25e-16
    "generic/56_128/view/family": 2e-15,    # 1.02e-15
    "generic/56_128/view/column": 2e-12,    # 1.02e-12
    "generic/56_128/accel/residual": 5e-16,    # 4.37e-16
    "generic/56_128/accel/family": 8e-16,    # 7.34e-16
    "generic/56_128/accel/column": 5e-13,    # 4.37e-13
    "generic/56_128/gyro/residual": 7e-16,    # 6.58e-16
    "generic/56_128/gyro/family": 8e-16,    # 7.02e-16
    "generic/56_128/gyro/column": 8e-14,    # 7.74e-14
    "generic/56_128/ne": 3e-13,    # 2.64e-13
    "static/56_128/view/residual": 2e-16,    # 1.38e-16
    "static/56_128/view/family": 9e-16,    # 8.67e-16
    "static/56_128/view/column": 6e-13,    # 5.72e-13
    "static/56_128/accel/residual": 4e-16,    # 3.06e-16
    "static/56_128/accel/family": 2e-15,    # 1.04e-15
    "static/56_128/accel/column": 2e-13,    # 1.22e-13
    "static/56_128/gyro/residual": 2e-16,    # 2.00e-16
    "static/56_128/gyro/family": 6e-16,    # 5.78e-16
    "static/56_128/gyro/column": 8e-14,    # 7.83e-14
    "static/56_128/ne": 2e-13,    # 1.58e-13
    "rs/past_1/view/residual": 2e-16,    # 1.40e-16
    "rs/past_1/view/family": 3e-15,    # 2.01e-15
    "rs/past_1/view/column": 9e-13,    # 8.18e-13
    "rs/past_1/accel/residual": 2e-16,    # 1.48e-16
    "rs/past_1/accel/family": 6e-16,    # 5.52e-16
    "rs/past_1/accel/column": 4e-13,    # 3.98e-13
    "rs/past_1/gyro/residual": 3e-16,    # 2.61e-16
    "rs/past_1/gyro/family": 8e-16,    # 7.52e-16
    "rs/past_1/gyro/column": 7e-14,    # 6.20e-14
    "rs/past_1/ne": 6e-13,    # 5.60e-13
    "rs/below_0/view/residual": 2e-16,    # 1.72e-16
    "rs/below_0/view/family": 2e-15,    # 1.29e-15
    "rs/below_0/view/column": 7e-14,    # 6.54e-14
    "rs/below_0/accel/residual": 2e-16,    # 1.48e-16
    "rs/below_0/accel/family": 6e-16,    # 5.52e-16
    "rs/below_0/accel/column": 4e-13,    # 3.98e-13
    "rs/below_0/gyro/residual": 3e-16,    # 2.61e-16
    "rs/below_0/gyro/family": 8e-16,    # 7.52e-16
    "rs/below_0/gyro/column": 7e-14,    # 6.20e-14
    "rs/below_0/ne": 9e-15,    # 8.86e-15
    "rs/ld0/view/residual": 6e-16,    # 5.38e-16
    "rs/ld0/view/family": 2e-15,    # 1.50e-15
    "rs/ld0/view/column": 4e-13,    # 3.94e-13
    "rs/ld0/accel/residual": 2e-16,    # 1.48e-16
    "rs/ld0/accel/family": 6e-16,    # 5.52e-16
    "rs/ld0/accel/column": 4e-13,    # 3.98e-13
    "rs/ld0/gyro/residual": 3e-16,    # 2.61e-16
    "rs/ld0/gyro/family": 8e-16,    # 7.52e-16
    "rs/ld0/gyro/column": 7e-14,    # 6.20e-14
    "rs/ld0/ne": 8e-13,    # 7.25e-13
    "rs/v0/view/residual": 4e-16,    # 3.74e-16
    "rs/v0/view/family": 2e-15,    # 1.06e-15
    "rs/v0/view/column": 7e-13,    # 6.41e-13
    "rs/v0/accel/residual": 2e-16,    # 1.48e-16
    "rs/v0/accel/family": 6e-16,    # 5.52e-16
    "rs/v0/accel/column": 4e-13,    # 3.98e-13
    "rs/v0/gyro/residual": 3e-16,    # 2.61e-16
    "rs/v0/gyro/family": 8e-16,    # 7.52e-16
    "rs/v0/gyro/column": 7e-14,    # 6.20e-14
    "rs/v0/ne": 9e-13,    # 8.89e-13
    "rs/seconds/view/residual": 3e-16,    # 2.17e-16
    "rs/seconds/view/family": 1e-15,    # 9.18e-16
    "rs/seconds/view/column": 7e-13,    # 6.41e-13
    "rs/seconds/accel/residual": 2e-16,    # 1.48e-16
    "rs/seconds/accel/family": 6e-16,    # 5.52e-16
    "rs/seconds/accel/column": 4e-13,    # 3.98e-13
    "rs/seconds/gyro/residual": 3e-16,    # 2.61e-16
    "rs/seconds/gyro/family": 8e-16,    # 7.52e-16
    "rs/seconds/gyro/column": 7e-14,    # 6.20e-14
    "rs/seconds/ne": 7e-13,    # 6.42e-13
    "rs/seconds_past_1/view/residual": 6e-16,    # 5.33e-16
    "rs/seconds_past_1/view/family": 2e-15,    # 1.20e-15
    "rs/seconds_past_1/view/column": 7e-13,    # 6.96e-13
    "rs/seconds_past_1/accel/residual": 5e-16,    # 4.37e-16
    "rs/seconds_past_1/accel/family": 8e-16,    # 7.34e-16
    "rs/seconds_past_1/accel/column": 5e-13,    # 4.37e-13
    "rs/seconds_past_1/gyro/residual": 7e-16,    # 6.58e-16
    "rs/seconds_past_1/gyro/family": 8e-16,    # 7.02e-16
    "rs/seconds_past_1/gyro/column": 8e-14,    # 7.74e-14
    "rs/seconds_past_1/ne": 4e-13,    # 3.88e-13
    "failed_projection/view/residual": 8e-16,    # 7.93e-16
    "failed_projection/view/family": 7e-16,    # 6.54e-16
    "failed_projection/view/column": 5e-13,    # 4.47e-13
    "failed_projection/accel/residual": 2e-16,    # 1.48e-16
    "failed_projection/accel/family": 6e-16,    # 5.52e-16
    "failed_projection/accel/column": 4e-13,    # 3.98e-13
    "failed_projection/gyro/residual": 3e-16,    # 2.61e-16
    "failed_projection/gyro/family": 8e-16,    # 7.52e-16
    "failed_projection/gyro/column": 7e-14,    # 6.20e-14
    "failed_projection/ne": 8e-13,    # 7.03e-13
    "gs_view/view/residual": 3e-16,    # 2.17e-16
    "gs_view/view/family": 2e-15,    # 1.06e-15
    "gs_view/view/column": 7e-13,    # 6.30e-13
    "gs_view/accel/residual": 2e-16,    # 1.48e-16
    "gs_view/accel/family": 6e-16,    # 5.52e-16
    "gs_view/accel/column": 4e-13,    # 3.98e-13
    "gs_view/gyro/residual": 3e-16,    # 2.61e-16
    "gs_view/gyro/family": 8e-16,    # 7.52e-16
    "gs_view/gyro/column": 7e-14,    # 6.20e-14
    "gs_view/ne": 3e-14,    # 2.21e-14
    "gs_view_unit_loss/view/residual": 3e-16,    # 2.17e-16
    "gs_view_unit_loss/view/family": 2e-15,    # 1.24e-15
    "gs_view_unit_loss/view/column": 7e-13,    # 6.30e-13
    "gs_view_unit_loss/accel/residual": 2e-16,    # 1.48e-16
    "gs_view_unit_loss/accel/family": 6e-16,    # 5.52e-16
    "gs_view_unit_loss/accel/column": 4e-13,    # 3.98e-13
    "gs_view_unit_loss/gyro/residual": 3e-16,    # 2.61e-16
    "gs_view_unit_loss/gyro/family": 8e-16,    # 7.52e-16
    "gs_view_unit_loss/gyro/column": 7e-14,    # 6.20e-14
    "gs_view_unit_loss/ne": 8e-13,    # 7.25e-13
    "flags/FLAGS1/view/residual": 3e-16,    # 2.17e-16
    "flags/FLAGS1/view/family": 1e-15,    # 9.05e-16
    "flags/FLAGS1/view/column": 7e-13,    # 6.41e-13
    "flags/FLAGS1/accel/residual": 2e-16,    # 1.48e-16
    "flags/FLAGS1/accel/family": 6e-16,    # 5.52e-16
    "flags/FLAGS1/accel/column": 4e-13,    # 3.98e-13
    "flags/FLAGS1/gyro/residual": 3e-16,    # 2.61e-16
    "flags/FLAGS1/gyro/family": 8e-16,    # 7.52e-16
    "flags/FLAGS1/gyro/column": 7e-14,    # 6.20e-14
    "flags/FLAGS1/ne": 7e-13,    # 6.42e-13
    "flags/LINE_DELAY/view/residual": 3e-16,    # 2.17e-16
    "flags/LINE_DELAY/view/family": 2e-15,    # 1.06e-15
    "flags/LINE_DELAY/view/column": 2e-15,    # 1.06e-15
    "flags/LINE_DELAY/accel/residual": 2e-16,    # 1.48e-16
    "flags/LINE_DELAY/accel/family": 0,    # 0.00e+00
    "flags/LINE_DELAY/accel/column": 0,    # 0.00e+00
    "flags/LINE_DELAY/gyro/residual": 3e-16,    # 2.61e-16
    "flags/LINE_DELAY/gyro/family": 0,    # 0.00e+00
    "flags/LINE_DELAY/gyro/column": 0,    # 0.00e+00
    "flags/LINE_DELAY/ne": 7e-16,    # 6.83e-16
}


def yardstick(key):
    return YARDSTICK[key]
