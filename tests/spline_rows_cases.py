"""Small spline-calibration problems placed on the branches and degenerate values of the row code (block_items.h, spline_seg.h,
spline_math.h), for tests/spline_rows_reference.py: shared by the host tests and the GPU tests.

A problem is a dict built by `make_problem` and handed to an estimator through the public setters (`build`): 9 SO(3) and 9 R^3 knots
(the 56 / 128 ms case: 9 and 7), at most 3 views of 2 corners, 4 accelerometer and 4 gyroscope samples; weights isx != isy,
w_acc != w_gyr != 1, all IMU misalignments distinct and non-zero, non-zero bias knots, T_i_c away from the identity, board points with
homogeneous scales other than 1.  Every corner's point is placed in front of the camera at the view's own pose, so the geometry stays
ordinary whatever the knots do.  Observations lie some 100 px off the projection, accelerometer and gyroscope measurements 3 m/s^2
and 0.5 rad/s off the model: a residual of float64 carries a few eps of the terms it is the difference of (|pi| + |uv| ~ 900 px,
|R^T (a + g)| + |MS (m - bias)| ~ 20 m/s^2), so the cost 1/2 sum r^2 can be held to COST_BOUND = 1e-14 = 45 eps only where the
residuals are a tenth or more of those terms; where the body rate is exactly 0 (static windows) a smaller gyroscope residual would
also be measured against nothing but the rounding of the knots' quaternions (1e-17 rad per segment, times 1 / dt).

The edge of a case is a segment angle theta of TWO knot pairs, (2, 3) and (4, 5), with different axes: the default samples sit in the
windows 0 and 2, which see the pairs as segments (2, 4) and (0, 2) -- the first, an interior and the last position of the backward
chain.  Every other segment has a generic angle of 0.1 ... 0.3 rad.
"""
import mpmath as mp
import numpy as np

import ba_rows_reference as B
import spline_rows_reference as R
from openimucameracalibrator_amd import estimator as E

FLAGS1 = E.SPLINE | E.T_I_C | E.GRAVITY_DIR
ALL = FLAGS1 | E.CAM_LINE_DELAY | E.IMU_BIASES | E.IMU_INTRINSICS
LD_ONLY = E.CAM_LINE_DELAY

DT = 100_000_000
START = 5_000_000_007
PINHOLE_INTR = [600.0, 1.02, 0.5, 320.0, 240.0, -0.05, 0.01]
DIVISION_INTR = [600.0, 1.02, 320.0, 240.0, -2e-7]
DOUBLE_SPHERE_INTR = [600.0, 1.02, 0.5, 320.0, 240.0, -0.2, 0.55]
AXIS_A = np.array([0.36, -0.48, 0.8])
AXIS_B = np.array([-0.6, 0.64, 0.48])
CORNERS = [(0.3, 0.2, 1.5), (-0.25, -0.15, 1.3), (0.1, -0.2, 1.7), (-0.3, 0.1, 1.4)]
OFFSETS = [(70.0, -40.0), (-50.0, 90.0), (30.0, 60.0), (-80.0, -20.0)]
SCALES = [1.0, 2.0, 0.5, 1.0]


def _qmul_exp(q, v):
    """float64 q * exp(v), the product taken in 50 digits (the placed angle is accurate to the rounding of the stored knot)."""
    qm = [mp.mpf(float(x)) for x in q]
    r = R.qunit(mp.mp, R.qmul(qm, R.qexp(mp.mp, [mp.mpf(float(x)) for x in v])))
    return np.array([float(x) for x in r])


def make_problem(name, theta=None, static=False, negate=False, dt_so3=DT, dt_r3=DT, duration=4 * DT - 1, dt_bias=2 * DT,
                 view_times=(0.37, 2.81), acc_times=(0.21, 0.66, 2.13, 2.58), gyr_times=(0.45, 0.9, 2.3, 2.77), gs=(), ld=1e-4,
                 camera=(B.PINHOLE, PINHOLE_INTR), options=None, flags=ALL, zero_v=None, behind=None, residuals_only=False,
                 corners_per_view=2, offset_scale=1.0):
    """times: in units of DT from the start (floats are rounded to ns; integers of ns are given as ("ns", t))."""
    rng = np.random.default_rng(20240611)
    n_so3, n_r3 = duration // dt_so3 + 6, duration // dt_r3 + 6
    q = [np.array([0.05, -0.08, 0.03, 1.0]) / np.linalg.norm([0.05, -0.08, 0.03, 1.0])]
    for j in range(n_so3 - 1):
        v = rng.normal(size=3); v *= (0.1 + 0.2 * rng.random()) / np.linalg.norm(v)
        if static:
            v = np.zeros(3)
        elif theta is not None and j in (2, 4):
            v = theta * (AXIS_A if j == 2 else AXIS_B)
        nxt = q[-1].copy() if not v.any() else _qmul_exp(q[-1], v)
        q.append(nxt)
    if negate:
        q[3] = -q[3]; q[5] = -q[5]
    r3 = np.array([0.1, -0.05, 0.2]) + 0.05 * rng.normal(size=(n_r3, 3)) + 0.02 * np.arange(n_r3)[:, None]
    ns = lambda t: int(t[1]) if isinstance(t, tuple) else int(round(t * DT))
    P = dict(name=name, dt_so3_ns=int(dt_so3), dt_r3_ns=int(dt_r3), start_ns=START, end_ns=START + int(duration), so3=np.array(q), r3=r3,
             T_i_c=np.concatenate([np.array([0.05, -0.03, 0.02, 1.0]) / np.linalg.norm([0.05, -0.03, 0.02, 1.0]), [0.03, -0.02, 0.05]]),
             g=np.array([0.3, -0.2, 9.79]), ld=float(ld), acc_intr=np.array([0.011, -0.007, 0.004, 1.02, 0.97, 1.01]),
             gyr_intr=np.array([0.006, -0.009, 0.003, 0.008, -0.005, 0.002, 0.99, 1.03, 1.01]), cam_model=int(camera[0]),
             intr=np.array(camera[1], dtype=np.float64), ab=np.array([0.12, -0.08, 0.05]), gb=np.array([0.004, -0.006, 0.003]),
             dt_bias_ns=int(dt_bias), n_bias=int(duration // dt_bias + 3), w_acc=3.7, w_gyr=11.3, options=dict(options or {}), flags=int(flags),
             residuals_only=bool(residuals_only), views=[], points=[])
    for v, t in enumerate(view_times):
        view = dict(t_ns=START + ns(t), rs=v not in gs, uv=np.zeros((corners_per_view, 2)), point_ids=[],
                    cov=np.array([[0.25 + 0.01 * c, 0.64 - 0.02 * c] for c in range(corners_per_view)]))
        P["views"].append(view)
        for c in range(corners_per_view):
            k = (2 * v + c) % 4
            # the pose of the view's own time (float64): the point in front of that camera, the pixel near its projection
            s_s, u_s = R.window(P, view["t_ns"], dt_so3); s_r, u_r = R.window(P, view["t_ns"], dt_r3)
            qw, _ = R.so3_spline(mp.fp, tuple(tuple(float(x) for x in a) for a in P["so3"][s_s:s_s + 6]), float(u_s), 1e9 / dt_so3)
            tw = R.r3_spline(mp.fp, [[float(x) for x in a] for a in r3[s_r:s_r + 6]], float(u_r), 0, 1e9 / dt_r3)
            xc = np.array(CORNERS[k]) * (np.array([1, 1, -1]) if behind == (v, c) else 1)
            Ric, Rwi = np.array(R.qmatrix(list(P["T_i_c"][:4]))), np.array(R.qmatrix(qw))
            X = Rwi @ (Ric @ xc + P["T_i_c"][4:]) + np.array(tw)
            view["point_ids"].append(len(P["points"]))
            P["points"].append(np.concatenate([X * SCALES[k], [SCALES[k]]]))
            px = B.project(mp.fp, P["cam_model"], [float(x) for x in P["intr"]], [float(x) for x in CORNERS[k]])
            view["uv"][c] = [px[0] + offset_scale * OFFSETS[k][0], px[1] + offset_scale * OFFSETS[k][1]]
            if zero_v == (v, c):
                view["uv"][c, 1] = 0.0
    P["points"] = np.array(P["points"])
    S = R.state_of(mp.fp, P)
    for kind, key, times in ((1, "acc", acc_times), (2, "gyr", gyr_times)):
        P[key] = dict(t_ns=[START + ns(t) for t in times], meas=np.zeros((len(times), 3)))
        bias = P["ab" if kind == 1 else "gb"]
        MS = np.array(R.imu_ms([float(x) for x in P["acc_intr" if kind == 1 else "gyr_intr"]], kind))
        for i in range(len(times)):
            pred, _ = R.imu_parts(mp.fp, P, S, kind, i)
            off = offset_scale * (3.0 if kind == 1 else 0.5) * np.array([1.0, -0.6, 0.8]) * (1 + 0.3 * i)
            P[key]["meas"][i] = bias + np.linalg.solve(MS, np.array([float(x) for x in pred])) + off
    return P


def build(backend, P, options=None):
    """The problem on an estimator (backend None: the device) through the public setters."""
    tr = E.SplineTrajectoryEstimator(backend=backend)
    for k, v in dict(P["options"], **(options or {})).items():
        tr.SetOption(k, v)
    tr.SetTimes(P["dt_so3_ns"], P["dt_r3_ns"], P["start_ns"], P["end_ns"])
    assert tr.GetNumSO3Knots() == len(P["so3"]) and tr.GetNumR3Knots() == len(P["r3"])
    tr.SetKnots(P["so3"], P["r3"])
    tr.SetT_i_c(P["T_i_c"][:4], P["T_i_c"][4:]); tr.SetGravity(P["g"]); tr.SetCameraLineDelay(P["ld"])
    tr.SetIMUIntrinsics(P["acc_intr"], P["gyr_intr"]); tr.SetCamera(P["cam_model"], P["intr"])
    tr.InitBiasSplines(P["ab"], P["gb"], P["dt_bias_ns"], P["dt_bias_ns"], 10.0, 10.0)
    tr.SetImageData([], P["points"])
    for view in P["views"]:
        add = tr.AddRSCameraMeasurements if view["rs"] else tr.AddGSCameraMeasurements
        assert add([view["t_ns"]], [0, len(view["uv"])], view["uv"], view["point_ids"], view["cov"]).all()
    assert tr.AddAccelerometerMeasurements(P["acc"]["meas"], P["acc"]["t_ns"], P["w_acc"]).all()
    assert tr.AddGyroscopeMeasurements(P["gyr"]["meas"], P["gyr"]["t_ns"], P["w_gyr"]).all()
    return tr


class _Calibrator:
    """The attributes of ImuCameraCalibrator that normal_equations_reference.assemble reads, for a bare estimator."""

    def __init__(self, P, tr):
        self.trajectory_ = tr
        self.num_corners = sum(len(v["uv"]) for v in P["views"])
        self.views_accepted = np.ones(len(P["views"]), bool)
        ta, tg = np.array(P["acc"]["t_ns"], np.int64), np.array(P["gyr"]["t_ns"], np.int64)
        self.imu_t_ns = np.concatenate([ta, tg])
        self.accl_accepted = np.concatenate([np.ones(len(ta), bool), np.zeros(len(tg), bool)])
        self.gyro_accepted = ~self.accl_accepted


class _DataSet:
    def __init__(self, P):
        t = np.array([v["t_ns"] for v in P["views"]], np.int64)
        s = t / E.S_TO_NS
        s = np.where((s * E.S_TO_NS).astype(np.int64) < t, np.nextafter(s, np.inf), s)
        assert np.array_equal((s * E.S_TO_NS).astype(np.int64), t)           # block_times converts them back
        self.view_t_s = s
        self.corner_offset = np.concatenate([[0], np.cumsum([len(v["uv"]) for v in P["views"]])]).astype(np.int64)


def unweighted_rows(P):
    """Boolean per view residual row: the rows of global-shutter views that carry no weight (quirk Q2)."""
    off = bool(P["options"].get("gs_unit_loss", 0))
    return np.concatenate([np.full(2 * len(v["uv"]), not (v["rs"] or off)) for v in P["views"]])


class EstimatorRows:
    """EvaluateBlocks of an estimator as a `rows_backend` of assemble.  jets=True: quirk Q2 applied to the Jet oracle's dump, which holds
    the rows of an unweighted global-shutter view BEFORE the loss (its Evaluate drops those views; the device and the host compile
    of the closed forms leave zeros in the dump already)."""

    def __init__(self, P, tr, jets=False):
        self.P, self.tr, self.jets, self.trajectory_ = P, tr, jets, self
        self.num_corners = sum(len(v["uv"]) for v in P["views"])

    def EvaluateBlocks(self, flags, kind, n_rows):
        r, J = self.tr.EvaluateBlocks(flags, kind, n_rows)
        if kind == 0 and self.jets:
            r[unweighted_rows(self.P)] = 0.0; J[unweighted_rows(self.P)] = 0.0
        return r, J


def assemble(P, tr, flags, rows_of=None, dtype=R.LD, shuffle_seed=None):
    """cost, H, g of normal_equations_reference.assemble for the problem on estimator `tr` (which supplies the tangent layout);
    rows_of: whose rows are summed -- EstimatorRows(P, estimator) or the 50-digit RowsBackend(P)."""
    import normal_equations_reference as NE
    return NE.assemble(_Calibrator(P, tr), _DataSet(P), flags, rows_backend=rows_of, dtype=dtype, shuffle_seed=shuffle_seed,
                       bias_dt_ns=(P["dt_bias_ns"], P["dt_bias_ns"]))


def stepped_cost(P, tr):
    """50-digit cost of the problem at the parameters the estimator holds now (knots, T_i_c, gravity, line delay, IMU intrinsics;
    the bias knots must not have moved)."""
    so3, r3 = tr.GetKnots()
    ab, gb = tr.GetBiasKnots()
    assert np.array_equal(ab, np.tile(P["ab"], (len(ab), 1))) and np.array_equal(gb, np.tile(P["gb"], (len(gb), 1)))
    acc_intr, gyr_intr = tr.GetIMUIntrinsics()
    return R.cost_at(P, so3, r3, dict(T_i_c=tr.GetT_i_c(), g=tr.GetGravity(), ld=tr.GetRSLineDelay(), acc_intr=acc_intr, gyr_intr=gyr_intr))


NS = lambda t: ("ns", t)
# sample times on the knot times: u = 0 exactly, 1 ns behind a knot time, 1 ns in front of the next; the first ns of the first window
# and the last ns of the last window of the 9-knot trajectory; bias splines (dt 200 ms) at u_b = 0 and u_b = 1 - 1 ns / dt
KNOT_TIMES = dict(view_times=(NS(2 * DT), NS(3 * DT - 1), NS(DT + 1)), acc_times=(NS(0), NS(2 * DT), NS(2 * DT - 1), NS(4 * DT - 1)),
                  gyr_times=(NS(0), NS(2 * DT + 1), NS(2 * DT - 1), NS(4 * DT - 1)))
SPACING = dict(dt_so3=56_000_000, dt_r3=128_000_000, duration=223_999_999, dt_bias=112_000_000, view_times=(0.3, 1.5),
               acc_times=(0.1, 0.7, 1.3, 2.1), gyr_times=(0.2, 0.9, 1.6, 2.2))

_SPECS = {
    # ---- the segment angle of the pairs (2, 3) and (4, 5) ----
    "generic": dict(),
    "generic_division": dict(camera=(B.DIVISION, DIVISION_INTR)),
    "theta0": dict(theta=0.0),
    "static": dict(static=True),
    "t1e-12": dict(theta=1e-12),
    "t1.9e-10": dict(theta=1.9e-10),
    "t2.1e-10": dict(theta=2.1e-10),
    "t1e-6": dict(theta=1e-6),
    "t0.0099": dict(theta=0.0099),
    "t0.0101": dict(theta=0.0101),
    "pi-1e-6": dict(theta=np.pi - 1e-6),
    "pi+1e-6": dict(theta=np.pi + 1e-6),
    "pi-1e-11": dict(theta=np.pi - 1e-11, residuals_only=True),
    "t0.7_negated": dict(theta=0.7, negate=True),
    # ---- sample times ----
    "generic/knot_times": dict(KNOT_TIMES),
    "static/knot_times": dict(KNOT_TIMES, static=True),
    "generic/56_128": dict(SPACING),
    "static/56_128": dict(SPACING, static=True),
    # ---- rolling shutter ----
    "rs/past_1": dict(ld=1.5e-3),
    "rs/below_0": dict(ld=-3e-3),
    "rs/ld0": dict(ld=0.0),
    "rs/v0": dict(zero_v=(0, 1)),
    "rs/seconds": dict(ld=1e-5, options={"rs_time_in_seconds": 1}),
    "rs/seconds_past_1": dict(ld=1.5e-4, options={"rs_time_in_seconds": 1}, **SPACING),
    # ---- blocks ----
    "failed_projection": dict(camera=(B.DOUBLE_SPHERE, DOUBLE_SPHERE_INTR), behind=(1, 0)),
    "gs_view": dict(gs=(0,)),
    "gs_view_unit_loss": dict(gs=(0,), options={"gs_unit_loss": 1}),
    "flags/FLAGS1": dict(flags=FLAGS1),
    "flags/LINE_DELAY": dict(flags=LD_ONLY),
}
# the static window a tenth as far from its measurements, so that the first LM step (FLAGS1) is one the trust region accepts
LM_CASE = dict(static=True, offset_scale=0.1, flags=FLAGS1)
CASES = list(_SPECS)
# the cases that also run at assembly = 2 and with wide_cells = 0 on the device
ASSEMBLY_SUBSET = ["generic", "static", "generic/knot_times", "rs/past_1", "gs_view"]
_problems = {}


def problem(name):
    if name not in _problems:
        _problems[name] = make_problem(name, **(LM_CASE if name == "static/lm" else _SPECS[name]))
    return _problems[name]


def check_first_lm_step(P, tr):
    """One LM iteration (FLAGS1) on estimator `tr`: finite, accepted, and the reported cost is the 50-digit cost at the stepped
    parameters to 1e-12 relative.  Returns (reported cost, 50-digit cost)."""
    s = tr.Optimize(1, FLAGS1)
    it = tr.GetIterations()[-1]
    so3, r3 = tr.GetKnots()
    assert s["num_iterations"] == 1 and np.isfinite(s["final_cost"]) and np.isfinite(so3).all() and np.isfinite(r3).all()
    assert np.isfinite(tr.GetT_i_c()).all() and np.isfinite(tr.GetGravity()).all()
    assert it["step_is_successful"] == 1 and it["relative_decrease"] >= 0.1 + 1e-3, it
    assert not np.array_equal(so3, P["so3"]) and not np.array_equal(r3, P["r3"]), "the step was not taken"
    ref = float(stepped_cost(P, tr))
    print("cost after the first LM step %.17g, 50 digits %.17g, relative difference %.3e" % (s["final_cost"], ref, abs(s["final_cost"] - ref) / ref))
    assert abs(s["final_cost"] - ref) <= 1e-12 * ref, (s["final_cost"], ref)
    return s["final_cost"], ref
