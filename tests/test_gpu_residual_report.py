"""Residual report and corner gating of the spline problem (oicc_residual_report, oicc_gate_corners; csrc/kernels_report.hip,
csrc/oicc_report.hip) against the CPU oracle.  The oracle has no report of its own: its per-block residual dump
(EvaluateBlocks, forward-mode Jets or the analytic rows, weighted) is the reference every figure is restated from with numpy.

Tolerances: corner errors and IMU residuals 1e-12 (1 + |r|), the bound the parity suite applies to block residuals (fp64, two
independent evaluation orders); per-view and whole-problem figures are norms, medians and maxima of those values (1-Lipschitz in
each of them), so the same bound holds for them.  The gated solve is held to the tolerances tests/test_gpu_parity.py applies to
plain Levenberg-Marquardt results: cost 1e-8 relative, T_i_c 1e-7, gravity 1e-6.
"""
import numpy as np
import pytest

import oracle_backend
from openimucameracalibrator_amd import synthetic, estimator as E

pytestmark = pytest.mark.gpu

FLAGS1 = E.SPLINE | E.T_I_C | E.GRAVITY_DIR
RAYLEIGH = 1.17741
ACC_BIAS0, GYR_BIAS0 = np.array([0.11, -0.07, 0.05]), np.array([0.012, -0.02, 0.007])
ACCL6, GYRO9 = (0.01, -0.02, 0.015, 1.02, 0.99, 1.01), (0.005, -0.01, 0.02, -0.015, 0.01, 0.004, 0.98, 1.01, 1.03)


def calibrator(ds, backend=None, cov_diag=None, live_imu=False):
    """BatchInitSpline(ds) with, optionally, a per-corner covariance and non-trivial bias splines / IMU intrinsics."""
    c = E.ImuCameraCalibrator(backend=backend)
    tr = c.trajectory_
    if cov_diag is not None:
        for name in ("AddRSCameraMeasurements", "AddGSCameraMeasurements"):
            setattr(tr, name, (lambda f: lambda t, off, uv, pt: f(t, off, uv, pt, cov_diag))(getattr(tr, name)))
    if live_imu:
        init, intr = tr.InitBiasSplines, tr.SetIMUIntrinsics
        tr.InitBiasSplines = lambda a, g, *rest: init(ACC_BIAS0, GYR_BIAS0, *rest)
        tr.SetIMUIntrinsics = lambda: intr(ACCL6, GYRO9)
    return c.BatchInitSpline(ds)


def pair(ds, **kw):
    return calibrator(ds, **kw), calibrator(ds, backend=oracle_backend.load(), **kw)


def oracle_corner_residuals(cpu, flags=FLAGS1):
    return cpu.trajectory_.EvaluateBlocks(flags, 0, 2 * cpu.num_corners, False)[0].reshape(-1, 2)


def close(a, b, ref_err=0.0):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) <= 1e-12 * (1 + np.abs(b)) + ref_err))


def literal_division_error(ds, rc):
    """[n, 1] what the ORACLE's pixel of a division-model corner carries: it keeps the reference's quotient
    sc = (1 - sqrt(1 - 4 m)) / (2 m), m = k u^2, whose numerator is of size 2 |m| with an absolute rounding of eps, so the pixel offset
    u sc is off by up to eps / (|k| u) -- 1.5e-11 px ten pixels from the principal point, 8e-13 at 200.  The product computes
    2 / (1 + sqrt(1 - 4 m)), which tests/test_gpu_ba_edges.py holds to a 50-digit restatement."""
    q = np.asarray(ds.intrinsics, dtype=np.float64)
    u = np.linalg.norm(ds.corner_uv + rc - q[2:4], axis=1)
    return (np.finfo(np.float64).eps / (abs(q[4]) * u))[:, None]


def check_corners(gpu, rc, scale=None, ref_err=0.0):
    """Report of `gpu` against the oracle's corner residuals rc [n, 2] (times `scale` where the oracle's are weighted)."""
    info = gpu.trajectory_.ResidualReport()
    e, st = gpu.trajectory_.GetCornerErrors()
    ref = rc if scale is None else rc * scale
    print("corner errors: max |e - ref| %.3e over %d corners" % (np.abs(e - ref).max(), len(e)))
    assert e.shape == ref.shape and close(e, ref, ref_err)
    assert not st.any() and info["num_used"] == info["num_corners"] == len(e) and info["num_failed"] == info["num_gated"] == 0
    return info, e


@pytest.mark.parametrize("camera", ["gopro9_division", "gopro6_fisheye", "gopro6_double_sphere"])
def test_corner_errors_equal_the_oracle_residuals(camera):
    gpu, cpu = pair(synthetic.make_config("tiny", camera=camera))
    check_corners(gpu, oracle_corner_residuals(cpu))


def test_corner_errors_of_global_shutter_views():
    """GS functor, no quirk Q2 zeroing in the report: the oracle shows those residuals with gs_unit_loss = 1."""
    ds = synthetic.make_config("tiny", rolling_shutter=False)
    gpu, cpu = pair(ds)
    cpu.trajectory_.SetOption("gs_unit_loss", 1)
    rc = oracle_corner_residuals(cpu)
    assert np.abs(rc).max() > 1e-3
    check_corners(gpu, rc)   # (the device problem keeps gs_unit_loss = 0: its solve gives these views no weight, the report does not care)


def test_corner_errors_are_unweighted():
    ds = synthetic.make_config("tiny")
    cov = np.random.RandomState(3).uniform(0.25, 9.0, (ds.num_corners, 2))
    gpu, cpu = pair(ds, cov_diag=cov)
    rc = oracle_corner_residuals(cpu)
    plain = oracle_corner_residuals(calibrator(ds, backend=oracle_backend.load()))
    assert np.abs(rc - plain).max() > 1e-2          # the weights are live on the oracle's side
    check_corners(gpu, rc, scale=np.sqrt(cov))


def test_getters_keep_the_callers_order():
    """Views handed over in the string order of the corner file's keys: the library sorts them by time, the getters do not show it."""
    ds = synthetic.make_config("tiny")
    order = ds.file_key_order()
    assert not np.array_equal(order, np.arange(ds.num_views))
    d2 = ds.with_view_order(order)
    d2.imu_t_s = d2.imu_t_s[::-1].copy(); d2.accel = d2.accel[::-1].copy(); d2.gyro = d2.gyro[::-1].copy()
    gpu, cpu = pair(d2)
    rc = oracle_corner_residuals(cpu)
    info, e = check_corners(gpu, rc)
    v = gpu.trajectory_.GetViewErrors()
    mag = np.linalg.norm(rc, axis=1)
    off = d2.corner_offset
    assert np.array_equal(v["n_used"], np.diff(off))
    assert close(v["rms_px"], [np.sqrt(np.mean(mag[a:b] ** 2)) for a, b in zip(off[:-1], off[1:])])
    assert close(v["max_px"], [mag[a:b].max() for a, b in zip(off[:-1], off[1:])])
    # ... and the time-ordered problem reports the same numbers at the permuted places
    ref = calibrator(ds)
    ref.trajectory_.ResidualReport()
    e_ref, _ = ref.trajectory_.GetCornerErrors()
    e_perm = np.concatenate([e_ref[ds.corner_offset[k]:ds.corner_offset[k + 1]] for k in order])
    assert np.array_equal(e, e_perm)
    for kind, n, w in ((1, int(gpu.accl_accepted.sum()), 1.0 / d2.std_r3), (2, int(gpu.gyro_accepted.sum()), 1.0 / d2.std_so3)):
        r = gpu.trajectory_.GetImuResiduals(kind)
        assert close(r, cpu.trajectory_.EvaluateBlocks(FLAGS1, kind, 3 * n, False)[0].reshape(-1, 3) / w)


def test_views_at_the_wave_edges():
    """Views of 1, 63, 64, 65 and 80 corners and one left whole: lanes without a corner, a full wave, a second round of one lane.
    The 10 x 8 board has a corner 10 px from the principal point, where the oracle's own pixel is 4e-12 off (literal_division_error);
    the per-view and whole-problem figures are restated from the corner errors the report itself hands out, checked first."""
    ds = synthetic.make_config("tiny", board=(10, 8), corners_per_view=80, num_views=6)
    assert np.array_equal(np.diff(ds.corner_offset), [80] * 6)
    want = [1, 63, 64, 65, 80, 80]
    keep = np.zeros(ds.num_corners, bool)
    for v, n in enumerate(want):
        keep[ds.corner_offset[v]:ds.corner_offset[v] + n] = True
    ds.corner_uv = ds.corner_uv[keep]; ds.corner_point = ds.corner_point[keep]
    ds.corner_offset = np.concatenate([[0], np.cumsum(want)]).astype(np.int64)
    gpu, cpu = pair(ds)
    rc = oracle_corner_residuals(cpu)
    assert ds.camera_model == synthetic.CAM_DIVISION_UNDISTORTION
    info, e = check_corners(gpu, rc, ref_err=literal_division_error(ds, rc))
    mag = np.linalg.norm(e, axis=1)
    v = gpu.trajectory_.GetViewErrors()
    off = ds.corner_offset
    assert np.array_equal(v["n_used"], want)
    assert close(v["rms_px"], [np.sqrt(np.mean(mag[a:b] ** 2)) for a, b in zip(off[:-1], off[1:])])
    assert close(v["max_px"], [mag[a:b].max() for a, b in zip(off[:-1], off[1:])])
    assert close(info["median_px"], np.median(mag)) and close(info["sigma_px"], np.median(mag) / RAYLEIGH)
    assert close(info["mean_px"], mag.mean()) and close(info["rms_px"], np.sqrt(np.mean(mag ** 2))) and close(info["max_px"], mag.max())
    assert info["num_views"] == 6


def test_failed_projections_have_status_1_and_stay_out_of_the_statistics():
    ds = synthetic.make_config("tiny", camera="gopro6_double_sphere")
    ds.points = ds.points.copy(); ds.points[0] = [0.0, 0.0, 5.0, 1.0]      # behind the camera that looks down -z at the board
    gpu, cpu = pair(ds)
    rc = oracle_corner_residuals(cpu)
    bad = np.all(rc == 1e10, axis=1)
    assert 1 <= bad.sum() < len(rc)
    info = gpu.trajectory_.ResidualReport()
    e, st = gpu.trajectory_.GetCornerErrors()
    assert np.array_equal(st == E.SplineTrajectoryEstimator.CORNER_PROJECTION_FAILED, bad) and np.array_equal(st != 0, bad)
    assert np.all(e[bad] == 1e10) and close(e[~bad], rc[~bad])
    assert info["num_failed"] == bad.sum() and info["num_used"] == (~bad).sum() and info["num_gated"] == 0
    mag = np.linalg.norm(rc[~bad], axis=1)
    assert close(info["median_px"], np.median(mag)) and close(info["sigma_px"], np.median(mag) / RAYLEIGH)
    assert close(info["mean_px"], mag.mean()) and close(info["rms_px"], np.sqrt(np.mean(mag ** 2))) and close(info["max_px"], mag.max())
    v = gpu.trajectory_.GetViewErrors()
    off = ds.corner_offset
    ok = ~bad
    assert np.array_equal(v["n_used"], [ok[a:b].sum() for a, b in zip(off[:-1], off[1:])])
    full = np.linalg.norm(rc, axis=1)
    assert close(v["rms_px"], [np.sqrt(np.mean(full[a:b][ok[a:b]] ** 2)) for a, b in zip(off[:-1], off[1:])])
    assert close(v["max_px"], [full[a:b][ok[a:b]].max() for a, b in zip(off[:-1], off[1:])])
    # a gate never takes a failed corner: its status stays 1
    gpu.trajectory_.GateCorners(1e-3)
    gpu.trajectory_.ResidualReport()
    assert np.array_equal(gpu.trajectory_.GetCornerErrors()[1] == 1, bad)


def test_imu_residuals_equal_the_oracle_residuals_over_the_weight():
    """Bias splines away from zero and a non-trivial triad model, so that b and MS of the residuals are live."""
    ds = synthetic.make_config("tiny")
    gpu, cpu = pair(ds, live_imu=True)
    flags = FLAGS1 | E.IMU_BIASES | E.IMU_INTRINSICS
    info = gpu.trajectory_.ResidualReport()
    plain = calibrator(ds)
    plain.trajectory_.ResidualReport()
    for kind, n, w, key in ((1, int(gpu.accl_accepted.sum()), 1.0 / ds.std_r3, "accl"), (2, int(gpu.gyro_accepted.sum()), 1.0 / ds.std_so3, "gyro")):
        rc = cpu.trajectory_.EvaluateBlocks(flags, kind, 3 * n, False)[0].reshape(-1, 3) / w
        r = gpu.trajectory_.GetImuResiduals(kind)
        print("kind %d: max |r - ref| %.3e over %d samples" % (kind, np.abs(r - rc).max(), n))
        assert r.shape == rc.shape and close(r, rc)
        assert np.abs(r - plain.trajectory_.GetImuResiduals(kind)).max() > 1e-3      # bias and triad terms are live
        assert close(info[key + "_rms"], np.sqrt(np.mean(rc ** 2, axis=0)))
        assert close(info[key + "_rms_weighted"], w * np.sqrt(np.mean(rc ** 2, axis=0)))
        assert info["num_" + key] == n


def test_report_and_lifted_gate_leave_the_solve_alone():
    """Bitwise comparisons: option accumulation = 1 (every sum of a Jacobian pass in one order) makes two runs of one problem
    bit-identical in the first place (tests/test_gpu_parity.py test_deterministic_accumulation_is_bit_identical); the default agrees
    to rounding.  The cost is therefore read from a Jacobian pass (Evaluate), with the gradient: the cost-only pass adds one atomic
    per chain of tiles in arrival order."""
    ds = synthetic.make_config("tiny")
    traces = []
    for with_report in (False, True):
        c = calibrator(ds)
        c.trajectory_.SetOption("accumulation", 1)
        if with_report:
            c.trajectory_.ResidualReport()
            assert c.trajectory_.GateCorners(0.0) == 0
        c.trajectory_.Optimize(50, FLAGS1)
        traces.append([(i["cost"], i["step_is_successful"]) for i in c.trajectory_.GetIterations()])
    assert len(traces[0]) >= 3 and traces[0] == traces[1]
    # gate, lift: the weights of the first report are back
    c = calibrator(ds)
    c.trajectory_.SetOption("accumulation", 1)
    info = c.trajectory_.ResidualReport()
    def cost_and_gradient():
        cost, _, g = c.trajectory_.Evaluate(FLAGS1, want_H=False)
        return cost, g.tobytes()
    cost0 = cost_and_gradient()
    n = c.trajectory_.GateCorners(info["median_px"])
    assert n == c.num_corners // 2 and c.trajectory_.GetCornerGate(c.num_corners).sum() == n
    cost_gated = cost_and_gradient()
    assert cost_gated[0] < cost0[0]
    info2 = c.trajectory_.ResidualReport()
    assert info2["num_gated"] == n and info2["num_used"] == c.num_corners - n
    e, st = c.trajectory_.GetCornerErrors()
    assert np.array_equal(st == 2, c.trajectory_.GetCornerGate(c.num_corners)) and np.all(np.linalg.norm(e[st == 2], axis=1) > info["median_px"])
    assert c.trajectory_.GateCorners(-1.0) == 0 and not c.trajectory_.GetCornerGate(c.num_corners).any()
    assert cost_and_gradient() == cost0
    # gating twice at one threshold is gating once (the original weight is kept next to the effective one)
    c.trajectory_.ResidualReport(); c.trajectory_.GateCorners(info["median_px"])
    c.trajectory_.ResidualReport(); assert c.trajectory_.GateCorners(info["median_px"]) == n
    assert cost_and_gradient() == cost_gated


def rotation_error_deg(q, q_true):
    d = abs(float(np.dot(q, q_true))) / (np.linalg.norm(q) * np.linalg.norm(q_true))
    return 2 * np.degrees(np.arccos(min(1.0, d)))


def test_gating_end_to_end_with_planted_outliers():
    """C1, gopro9_division, plain LM: 48 corners (4 %) displaced by 8-40 px.  One report, one 5 sigma gate, a second solve; the
    oracle is driven through the same steps (numpy gate over its residuals, cov_diag = inf on the gated corners, second solve from
    its stage-1 point)."""
    ds = synthetic.make_config("C1", camera="gopro9_division")
    n = ds.num_corners
    rng = np.random.RandomState(1)
    bad = rng.permutation(n)[:48]
    mag = rng.uniform(8, 40, 48)
    th = rng.uniform(0, 2 * np.pi, 48)
    ds.corner_uv = ds.corner_uv.copy()
    ds.corner_uv[bad] += mag[:, None] * np.stack([np.cos(th), np.sin(th)], -1)
    planted = np.zeros(n, bool); planted[bad] = True
    q_true = np.asarray(ds.truth["q_i_c"])

    ungated = calibrator(ds)
    ungated.Optimize(50, FLAGS1)
    err_ungated = rotation_error_deg(ungated.trajectory_.GetT_i_c()[:4], q_true)

    gpu = calibrator(ds)
    gpu.OptimizeGated(50, FLAGS1)
    gate = gpu.trajectory_.GetCornerGate(n)
    err_gated = rotation_error_deg(gpu.trajectory_.GetT_i_c()[:4], q_true)
    print("rotation error of T_i_c: ungated %.3f deg, gated %.3f deg; gate holds %d planted + %d clean corners at %.3f px"
          % (err_ungated, err_gated, (gate & planted).sum(), (gate & ~planted).sum(), gpu.gate_threshold_px))
    assert gpu.gated_corners == gate.sum()
    assert np.all(gate[planted])
    assert (gate & ~planted).sum() <= 0.01 * (n - 48)
    assert err_gated < 0.5 * err_ungated

    # the oracle through the same steps
    backend = oracle_backend.load()
    cpu1 = calibrator(ds, backend=backend)
    cpu1.Optimize(50, FLAGS1)
    rc = oracle_corner_residuals(cpu1)
    m = np.linalg.norm(rc, axis=1)
    sigma = np.median(m) / RAYLEIGH
    gate_cpu = m > 5.0 * sigma
    assert abs(gpu.gate_report["sigma_px"] - sigma) <= 1e-6 * sigma
    assert np.array_equal(np.nonzero(gate)[0], np.nonzero(gate_cpu)[0])
    cov = np.ones((n, 2)); cov[gate_cpu] = np.inf
    cpu2 = calibrator(ds, backend=backend, cov_diag=cov)
    cpu2.trajectory_.SetKnots(*cpu1.trajectory_.GetKnots())
    T = cpu1.trajectory_.GetT_i_c()
    cpu2.trajectory_.SetT_i_c(T[:4], T[4:]); cpu2.trajectory_.SetGravity(cpu1.trajectory_.GetGravity())
    cpu2.Optimize(50, FLAGS1)
    sg, sc = gpu.summary, cpu2.summary
    print("second solve: cost %.9g (device) %.9g (oracle), %d / %d iterations" % (sg["final_cost"], sc["final_cost"], sg["num_iterations"], sc["num_iterations"]))
    assert abs(sg["final_cost"] - sc["final_cost"]) <= 1e-8 * sc["final_cost"]
    assert np.abs(gpu.trajectory_.GetT_i_c() - cpu2.trajectory_.GetT_i_c()).max() < 1e-7
    assert np.abs(gpu.trajectory_.GetGravity() - cpu2.trajectory_.GetGravity()).max() < 1e-6


def test_error_paths():
    ds = synthetic.make_config("tiny")
    c = calibrator(ds)
    tr = c.trajectory_
    b, h = tr._b, tr._h
    n = c.num_corners
    e = np.zeros((n, 2)); st = np.zeros(n, np.uint8)
    dp, u8 = e.ctypes.data_as(E._abi.c_dp), st.ctypes.data_as(E._abi.c_u8p)
    OICC_ERR_STATE, OICC_ERR_UNSUPPORTED = -4, -5
    # no report yet
    assert b.get_corner_errors(h, dp, u8, n) == OICC_ERR_STATE
    assert b.get_view_errors(h, None, None, None, ds.num_views) == OICC_ERR_STATE
    assert b.get_imu_residuals(h, 1, dp, 0) == OICC_ERR_STATE
    assert b.gate_corners(h, 1.0, None) == OICC_ERR_STATE
    assert b.gate_corners(h, 0.0, None) == 0            # lifting needs none
    tr.ResidualReport()
    assert b.get_corner_errors(h, dp, u8, n) == 0
    assert b.get_corner_errors(h, dp, u8, n + 1) == -1
    # a report belongs to the parameters and measurements it was made at
    tr.SetGravity(tr.GetGravity())
    assert b.get_corner_errors(h, dp, u8, n) == OICC_ERR_STATE
    tr.ResidualReport(); tr.Optimize(1, FLAGS1)
    assert b.get_corner_errors(h, dp, u8, n) == OICC_ERR_STATE
    tr.ResidualReport()
    assert tr.GateCorners(1e-9) > 0                       # a gate that changes a weight changes the measurements
    assert b.get_corner_errors(h, dp, u8, n) == OICC_ERR_STATE
    # time shards
    tr.GateCorners(0.0); tr.ResidualReport()
    tr.SetShard(2, 0)
    assert b.gate_corners(h, 1.0, None) == OICC_ERR_UNSUPPORTED
    info = E._abi.ResidualInfo()
    import ctypes
    assert b.residual_report(h, ctypes.byref(info)) == OICC_ERR_UNSUPPORTED
