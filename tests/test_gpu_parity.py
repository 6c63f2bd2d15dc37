"""GPU parity: the HIP path (through the C-ABI, liboicc_hip.so) against the CPU
oracle on the same seeded inputs.  Run on an MI355X with `-m gpu`.

Tolerances (fp64): residuals 1e-12 abs+rel, tangent Jacobians
1e-8 rel-to-row-scale (analytic vs forward-mode autodiff), J^T J / J^T r 1e-10
rel-to-scale as SURVEY proposes (round 6: tightened from 1e-9; measured <= 4e-14, scripts/dbg_ne_margins.py),
LM iterates: cost 1e-8 rel, final parameters 1e-7 (the reference-option solves of the application's
flag set: 1e-9 / 1e-9, profiles/r06l_parity_margins.log).
The assembly tests assert J^T J / J^T r entry by entry as well (entry_err: every entry on its own scale d_i d_j; one global scale
leaves the small blocks unchecked); tests/test_gpu_normal_equations_reference.py holds the full entry-wise comparison.
"""
import numpy as np
import pytest

import oracle_backend
import normal_equations_reference as NER
from openimucameracalibrator_amd import synthetic, estimator as E

pytestmark = pytest.mark.gpu

FLAGS1 = E.SPLINE | E.T_I_C | E.GRAVITY_DIR


def build_pair(cfg="tiny", **kw):
    ds = synthetic.make_config(cfg, **kw)
    gpu = E.ImuCameraCalibrator().BatchInitSpline(ds)
    cpu = E.ImuCameraCalibrator(backend=oracle_backend.load()).BatchInitSpline(ds)
    return ds, gpu, cpu


def rel_err(a, b, scale=None):
    s = np.abs(b).max() if scale is None else scale
    return np.abs(a - b).max() / max(s, 1e-300)


def entry_err(tr, flags, Ha, Hb, ga, gb, cost):
    """Entry-wise errors of (Ha, ga) against (Hb, gb): max |dH_ij| / (d_i d_j) and max |dg_i| / (d_i sqrt(2 cost)), d = sqrt(diag Hb)
    (tests/normal_equations_reference.py) -- every entry on its own scale, where rel_err has one scale for the whole matrix."""
    kinds = NER.column_kinds(tr.GetTangentLayout(flags))
    eh, eg = NER.entrywise_error(Ha, Hb, kinds)[0], NER.gradient_error(ga, gb, Hb, cost, kinds)[0]
    print("entry-wise: H %.2e g %.2e" % (eh, eg))
    return eh, eg


@pytest.fixture(scope="module")
def tiny():
    return build_pair("tiny")


def test_layout_matches(tiny):
    _, gpu, cpu = tiny
    for flags in (FLAGS1, E.CAM_LINE_DELAY, FLAGS1 | E.IMU_BIASES | E.CAM_LINE_DELAY | E.IMU_INTRINSICS):
        lg, lc = gpu.trajectory_.GetTangentLayout(flags), cpu.trajectory_.GetTangentLayout(flags)
        assert lg["P"] == lc["P"]
        for k in ("so3", "r3", "accl_bias", "gyro_bias", "other"):
            assert np.array_equal(lg[k], lc[k]), k


@pytest.mark.parametrize("flags", [FLAGS1, FLAGS1 | E.CAM_LINE_DELAY, FLAGS1 | E.IMU_BIASES | E.IMU_INTRINSICS, E.CAM_LINE_DELAY])
def test_block_residuals_and_jacobians(tiny, flags):
    ds, gpu, cpu = tiny
    nrows = {0: 2 * gpu.num_corners, 1: 3 * int(gpu.accl_accepted.sum()), 2: 3 * int(gpu.gyro_accepted.sum())}
    for kind in (0, 1, 2):
        rg, Jg = gpu.trajectory_.EvaluateBlocks(flags, kind, nrows[kind])
        rc, Jc = cpu.trajectory_.EvaluateBlocks(flags, kind, nrows[kind])
        assert np.abs(rg - rc).max() <= 1e-12 * (1 + np.abs(rc).max()), (kind, np.abs(rg - rc).max())
        # row scale with a floor: rows whose true derivative is ~0 (constant knots past the last view) hold rounding noise
        scale = np.abs(Jc).max(axis=1, keepdims=True) + 1e-6 * np.abs(Jc).max() + 1e-30
        err = np.abs(Jg - Jc) / scale
        assert err.max() < 1e-8, (kind, err.max(), np.unravel_index(err.argmax(), err.shape))


@pytest.mark.parametrize("flags", [FLAGS1, FLAGS1 | E.CAM_LINE_DELAY | E.IMU_BIASES, E.CAM_LINE_DELAY])
def test_normal_equations(tiny, flags):
    _, gpu, cpu = tiny
    cg, Hg, gg = gpu.trajectory_.Evaluate(flags)
    cc, Hc, gc = cpu.trajectory_.Evaluate(flags)
    assert abs(cg - cc) <= 1e-11 * cc
    assert rel_err(gg, gc) < 1e-10
    assert rel_err(Hg, Hc) < 1e-10
    eh, eg = entry_err(gpu.trajectory_, flags, Hg, Hc, gg, gc, cc)
    assert eh < 1e-10 and eg < 1e-10, (eh, eg)
    assert np.abs(Hg - Hg.T).max() <= 1e-13 * np.abs(Hg).max()   # arrow corner: two atomics per off-diagonal pair
    assert NER.symmetry_error(Hg, Hc) <= 1e-13
    assert abs(gpu.trajectory_.EvaluateCost(flags) - cc) <= 1e-11 * cc


@pytest.mark.parametrize("camera", ["pinhole", "pinhole_radtan", "gopro6_fisheye", "gopro6_double_sphere", "gopro9_eucm"])
def test_all_camera_models(camera):
    ds, gpu, cpu = build_pair("tiny", camera=camera)
    n = 2 * gpu.num_corners
    flags = FLAGS1 | E.CAM_LINE_DELAY
    rg, Jg = gpu.trajectory_.EvaluateBlocks(flags, 0, n)
    rc, Jc = cpu.trajectory_.EvaluateBlocks(flags, 0, n)
    assert np.abs(rg - rc).max() <= 1e-11 * (1 + np.abs(rc).max())
    scale = np.abs(Jc).max(axis=1, keepdims=True) + 1e-6 * np.abs(Jc).max() + 1e-30
    assert (np.abs(Jg - Jc) / scale).max() < 1e-8


def test_lm_iterates_and_final_parameters(tiny):
    ds, _, _ = tiny
    _, gpu, cpu = build_pair("tiny")
    sg = gpu.trajectory_.Optimize(50, FLAGS1)
    sc = cpu.trajectory_.Optimize(50, FLAGS1)
    ig, ic = gpu.trajectory_.GetIterations(), cpu.trajectory_.GetIterations()
    assert sg["termination"] == sc["termination"] and sg["num_iterations"] == sc["num_iterations"], (sg, sc)
    for a, b in zip(ig, ic):
        assert a["step_is_successful"] == b["step_is_successful"]
        assert abs(a["cost"] - b["cost"]) <= 1e-8 * b["cost"]
    assert np.abs(gpu.trajectory_.GetT_i_c() - cpu.trajectory_.GetT_i_c()).max() < 1e-7
    assert np.abs(gpu.trajectory_.GetGravity() - cpu.trajectory_.GetGravity()).max() < 1e-6
    kg, kc = gpu.trajectory_.GetKnots(), cpu.trajectory_.GetKnots()
    assert np.abs(kg[0] - kc[0]).max() < 1e-7 and np.abs(kg[1] - kc[1]).max() < 1e-7
    assert abs(gpu.trajectory_.GetMeanReprojectionError() - cpu.trajectory_.GetMeanReprojectionError()) < 1e-7
    # stage 2: line delay only (continuous_time_imu_to_camera_calibration.cc:217-221)
    s2g = gpu.trajectory_.Optimize(10, E.CAM_LINE_DELAY)
    s2c = cpu.trajectory_.Optimize(10, E.CAM_LINE_DELAY)
    assert s2g["num_parameters_tangent"] == 1 == s2c["num_parameters_tangent"]
    assert abs(gpu.trajectory_.GetRSLineDelay() - cpu.trajectory_.GetRSLineDelay()) < 1e-9 * max(1.0, abs(cpu.trajectory_.GetRSLineDelay()) * 1e6)


def test_trajectory_getters(tiny):
    ds, gpu, cpu = tiny
    t = np.concatenate([[gpu.trajectory_.GetMinTimeNs() - 5, gpu.trajectory_.GetMaxTimeNs() + 10 ** 9], gpu.imu_t_ns[::7]]).astype(np.int64)
    og, oc = gpu.trajectory_.GetTrajectory(t), cpu.trajectory_.GetTrajectory(t)
    assert np.array_equal(og["valid"], oc["valid"]) and not og["valid"][0] and not og["valid"][1]
    for k in ("pose", "gyro", "accel", "gyro_bias", "accl_bias"):
        assert np.abs(og[k] - oc[k]).max() < 1e-11 * (1 + np.abs(oc[k]).max()), k


def test_c2_full_size_properties():
    """BASELINE config C2 at full size: parity on cost/gradient against the oracle
    plus size-independent properties (H symmetric PSD-diagonal, g = J^T r sign
    via descent: LM reduces the cost; gradient linear in residual scale)."""
    ds, gpu, cpu = build_pair("C2")
    cg, _, gg = gpu.trajectory_.Evaluate(FLAGS1, want_H=False)
    cc, _, gc = cpu.trajectory_.Evaluate(FLAGS1, want_H=False)
    assert abs(cg - cc) <= 1e-10 * cc and rel_err(gg, gc) < 1e-10
    s = gpu.trajectory_.Optimize(50, FLAGS1)
    assert s["termination"] == 0 and s["final_cost"] < 0.05 * s["initial_cost"]
    assert gpu.trajectory_.GetMeanReprojectionError() < 1.0
    q = gpu.trajectory_.GetT_i_c()[:4]
    qt = ds.truth["q_i_c"]
    ang = 2 * np.arccos(min(1.0, abs(float(q @ qt))))
    assert ang < np.deg2rad(0.5)


def test_c2_lm_iterates_match_the_jet_oracle():
    """BASELINE config C2 at full size, plain LM, stage 1 and stage 2: every iterate of the HIP path against the oracle's forward-mode
    Jets (analytic_jacobians = 0: none of the product's closed forms on the checker's side) -- accept / reject sequence, costs,
    step norms, gradient norms, final extrinsics, gravity, knots, line delay and mean reprojection error."""
    ds, gpu, cpu = build_pair("C2")
    cpu.trajectory_.SetOption("analytic_jacobians", 0)
    sg = gpu.trajectory_.Optimize(50, FLAGS1); sc = cpu.trajectory_.Optimize(50, FLAGS1)
    ig, ic = gpu.trajectory_.GetIterations(), cpu.trajectory_.GetIterations()
    assert sg["termination"] == sc["termination"] and sg["num_iterations"] == sc["num_iterations"] >= 3, (sg, sc)
    for a, b in zip(ig, ic):
        assert a["step_is_successful"] == b["step_is_successful"]
        assert abs(a["cost"] - b["cost"]) <= 1e-8 * b["cost"], (a, b)
        assert abs(a["step_norm"] - b["step_norm"]) <= 1e-6 * max(b["step_norm"], 1e-12), (a, b)
        assert abs(a["gradient_max_norm"] - b["gradient_max_norm"]) <= 1e-6 * max(b["gradient_max_norm"], 1e-9), (a, b)
    assert np.abs(gpu.trajectory_.GetT_i_c() - cpu.trajectory_.GetT_i_c()).max() < 1e-7
    assert np.abs(gpu.trajectory_.GetGravity() - cpu.trajectory_.GetGravity()).max() < 1e-6
    kg, kc = gpu.trajectory_.GetKnots(), cpu.trajectory_.GetKnots()
    assert np.abs(kg[0] - kc[0]).max() < 1e-7 and np.abs(kg[1] - kc[1]).max() < 1e-7
    assert abs(gpu.trajectory_.GetMeanReprojectionError() - cpu.trajectory_.GetMeanReprojectionError()) < 1e-7
    s2g = gpu.trajectory_.Optimize(10, E.CAM_LINE_DELAY); s2c = cpu.trajectory_.Optimize(10, E.CAM_LINE_DELAY)
    assert s2g["num_iterations"] == s2c["num_iterations"] and abs(s2g["final_cost"] - s2c["final_cost"]) <= 1e-8 * s2c["final_cost"]
    assert abs(gpu.trajectory_.GetRSLineDelay() - cpu.trajectory_.GetRSLineDelay()) < 1e-3 * 1e-6      # 1e-3 us


def test_c2_reestimate_biases_mode_matches_the_jet_oracle():
    """The application's other mode at BASELINE config C2, full size: --reestimate_biases adds IMU_BIASES to the stage-1 flags
    (continuous_time_imu_to_camera_calibration.cc:201-204), so the program is bounds constrained and Ceres runs, besides the inner
    iterations of impl.h:266, its bounds line search and reports the projected gradient norm (UseReferenceSolverOptions).  Every
    outer iterate, the sweep count, the final extrinsics / gravity / bias splines and stage 2 against the oracle with forward-mode
    Jets (analytic_jacobians = 0)."""
    ds, gpu, cpu = build_pair("C2")
    flags = FLAGS1 | E.IMU_BIASES
    for c in (gpu, cpu):
        c.trajectory_.UseReferenceSolverOptions()
    cpu.trajectory_.SetOption("analytic_jacobians", 0)
    sg = gpu.trajectory_.Optimize(50, flags); sc = cpu.trajectory_.Optimize(50, flags)
    ig, ic = gpu.trajectory_.GetIterations(), cpu.trajectory_.GetIterations()
    assert sg["termination"] == sc["termination"] and sg["num_iterations"] == sc["num_iterations"] >= 3, ([i["cost"] for i in ig], [i["cost"] for i in ic])
    assert sg["inner_sweeps"] == sc["inner_sweeps"] >= 1 and sg["line_search_steps"] == sc["line_search_steps"]
    for a, b in zip(ig, ic):
        assert a["step_is_successful"] == b["step_is_successful"] and abs(a["cost"] - b["cost"]) <= 1e-7 * b["cost"], (a, b)
        assert abs(a["gradient_max_norm"] - b["gradient_max_norm"]) <= 1e-5 * max(b["gradient_max_norm"], 1e-9), (a, b)
    assert np.abs(gpu.trajectory_.GetT_i_c() - cpu.trajectory_.GetT_i_c()).max() < 1e-6
    assert np.abs(gpu.trajectory_.GetGravity() - cpu.trajectory_.GetGravity()).max() < 1e-5
    t_ns = (np.linspace(ds.view_t_s.min() + 0.5, ds.view_t_s.max() - 0.5, 17) * 1e9).astype(np.int64)
    for t in t_ns:
        assert np.abs(np.asarray(gpu.trajectory_.GetAcclBias(int(t))) - np.asarray(cpu.trajectory_.GetAcclBias(int(t)))).max() < 1e-6
        assert np.abs(np.asarray(gpu.trajectory_.GetGyroBias(int(t))) - np.asarray(cpu.trajectory_.GetGyroBias(int(t)))).max() < 1e-7
    s2g = gpu.trajectory_.Optimize(10, E.CAM_LINE_DELAY); s2c = cpu.trajectory_.Optimize(10, E.CAM_LINE_DELAY)
    assert s2g["num_iterations"] == s2c["num_iterations"] and abs(s2g["final_cost"] - s2c["final_cost"]) <= 1e-7 * s2c["final_cost"]
    assert abs(gpu.trajectory_.GetRSLineDelay() - cpu.trajectory_.GetRSLineDelay()) < 1e-3 * 1e-6      # 1e-3 us
    assert abs(gpu.trajectory_.GetMeanReprojectionError() - cpu.trajectory_.GetMeanReprojectionError()) < 1e-6


@pytest.mark.parametrize("algo,parts", [(1, 2), (1, 3), (1, 5), (4, 0), (0, 0)])
def test_parallel_solvers_match_sequential(algo, parts):
    """The time-partitioned band+arrow Cholesky (algorithm 1: p interior sweeps + reduced
    separator system), the block cyclic reduction through the pivot inverses (algorithm 4 = the automatic choice 0: log-depth nested
    dissection in time; the factor-based formulations 2 and 3 of rounds 1-3 left the library in round 4:
    no back substitution levels) and the automatic choice must reproduce the single-workgroup
    sequential sweep: same LM iterates on C2."""
    ds = synthetic.make_config("C2")
    ref = E.ImuCameraCalibrator().BatchInitSpline(ds)
    ref.trajectory_.SetOption("solver_algorithm", 1)
    ref.trajectory_.SetOption("solver_partitions", 1)
    s1 = ref.trajectory_.Optimize(50, FLAGS1)
    par = E.ImuCameraCalibrator().BatchInitSpline(ds)
    par.trajectory_.SetOption("solver_algorithm", algo)
    par.trajectory_.SetOption("solver_partitions", parts)
    s2 = par.trajectory_.Optimize(50, FLAGS1)
    assert s1["num_iterations"] == s2["num_iterations"] and s1["termination"] == s2["termination"]
    c1 = [i["cost"] for i in ref.trajectory_.GetIterations()]
    c2 = [i["cost"] for i in par.trajectory_.GetIterations()]
    assert np.allclose(c1, c2, rtol=1e-9, atol=0)
    assert np.abs(ref.trajectory_.GetT_i_c() - par.trajectory_.GetT_i_c()).max() < 1e-9
    k1, k2 = ref.trajectory_.GetKnots(), par.trajectory_.GetKnots()
    assert np.abs(k1[0] - k2[0]).max() < 1e-9 and (np.abs(k1[1] - k2[1]) / (1 + np.abs(k1[1]))).max() < 1e-9


@pytest.mark.parametrize("algo,intrinsics", [(1, 1), (4, 0), (4, 1), (0, 1)])
def test_bias_and_intrinsics_active_lm_matches_oracle(algo, intrinsics):
    """IMU_BIASES | IMU_INTRINSICS: 27+15 arrow columns, box-bounded bias knots, through the band sweep (1), the block cyclic
    reduction (2: three border tiles; IMU_BIASES alone: two) and the automatic choice (0 = BCR)."""
    ds = synthetic.make_config("tiny")
    flags = FLAGS1 | E.IMU_BIASES | (E.IMU_INTRINSICS if intrinsics else 0)
    gpu = E.ImuCameraCalibrator().BatchInitSpline(ds)
    gpu.trajectory_.SetOption("solver_algorithm", algo)
    cpu = E.ImuCameraCalibrator(backend=oracle_backend.load()).BatchInitSpline(ds)
    cg, Hg, gg = gpu.trajectory_.Evaluate(flags)
    cc, Hc, gc = cpu.trajectory_.Evaluate(flags)
    assert rel_err(Hg, Hc) < 1e-10 and rel_err(gg, gc) < 1e-10
    sg = gpu.trajectory_.Optimize(15, flags); sc = cpu.trajectory_.Optimize(15, flags)
    assert sg["num_iterations"] == sc["num_iterations"] and sg["arrow_dim"] == sc["arrow_dim"] > 16
    assert abs(sg["final_cost"] - sc["final_cost"]) <= 1e-7 * sc["final_cost"]
    ag, gg2 = gpu.trajectory_.GetBiasKnots(); ac, gc2 = cpu.trajectory_.GetBiasKnots()
    assert np.abs(ag - ac).max() < 1e-6 and np.abs(gg2 - gc2).max() < 1e-6
    assert np.abs(ag).max() <= 1.0 and np.abs(gg2).max() <= 0.1          # impl.h:213-218,235-240 bounds
    ig, ic = gpu.trajectory_.GetIMUIntrinsics(), cpu.trajectory_.GetIMUIntrinsics()
    assert np.abs(ig[0] - ic[0]).max() < 1e-6 and np.abs(ig[1] - ic[1]).max() < 1e-6


@pytest.mark.parametrize("cfg", ["tiny", "C1"])
def test_bcr_wide_borders_and_the_panel_hazard(cfg):
    """Block cyclic reduction with three and four 16-row border tiles (biases + IMU intrinsics: > 31 arrow columns), LDS poisoned
    before every pass and solve, over accepted and rejected steps: the iterates of the band sweep, also when the panel waves other
    than wave 0 start every panel late (debug_bcr_delay: they read the panel's diagonal block from the copy `dg` the trailing update
    leaves for them, kernels_bcr.hip -- the in-place read of round 2's kernel, the cause of its sporadic NaN pivots, left the library
    with that kernel in round 4)."""
    ds = synthetic.make_config(cfg)
    flags = FLAGS1 | E.IMU_BIASES | E.IMU_INTRINSICS

    def run(algo, **opts):
        c = E.ImuCameraCalibrator().BatchInitSpline(ds)
        c.trajectory_.SetOption("solver_algorithm", algo); c.trajectory_.SetOption("bcr_max_border", 64); c.trajectory_.SetOption("debug_poison_lds", 1)
        for k, v in opts.items():
            c.trajectory_.SetOption(k, v)
        s_ = c.trajectory_.Optimize(12, flags)
        return s_, c.trajectory_.GetIterations()

    s_ref, it_ref = run(1)
    assert 31 < s_ref["arrow_dim"] < 64 and s_ref["num_unsuccessful_steps"] + s_ref["num_successful_steps"] >= 4

    def same(it):
        return len(it) == len(it_ref) and all(a["step_is_successful"] == b["step_is_successful"] and abs(a["cost"] - b["cost"]) <= 1e-9 * b["cost"] for a, b in zip(it, it_ref))
    for opts in ({}, {"debug_bcr_delay": 3}, {"debug_bcr_delay": 9}):
        s_, it = run(4, **opts)
        assert s_["termination"] == s_ref["termination"] and same(it), (opts, [i["cost"] for i in it], [i["cost"] for i in it_ref])


@pytest.mark.parametrize("unit_loss", [0, 1])
def test_global_shutter_views_quirk_q2(unit_loss):
    """--global_shutter: GS functor with HuberLoss(0.0) leaves the views without weight
    (impl.h:532); option gs_unit_loss gives them a trivial loss instead."""
    ds = synthetic.make_config("tiny", rolling_shutter=False)
    assert ds.line_delay_init == 0.0
    gpu = E.ImuCameraCalibrator().BatchInitSpline(ds)
    cpu = E.ImuCameraCalibrator(backend=oracle_backend.load()).BatchInitSpline(ds)
    for c in (gpu, cpu):
        c.trajectory_.SetOption("gs_unit_loss", unit_loss)
    cg, Hg, gg = gpu.trajectory_.Evaluate(FLAGS1)
    cc, Hc, gc = cpu.trajectory_.Evaluate(FLAGS1)
    assert abs(cg - cc) <= 1e-11 * cc and rel_err(Hg, Hc) < 1e-10 and rel_err(gg, gc) < 1e-10
    if unit_loss == 0:   # only IMU blocks carry cost
        ca = gpu.trajectory_.EvaluateBlocks(FLAGS1, 1, 3 * int(gpu.accl_accepted.sum()), False)[0]
        cy = gpu.trajectory_.EvaluateBlocks(FLAGS1, 2, 3 * int(gpu.gyro_accepted.sum()), False)[0]
        assert abs(0.5 * (ca @ ca + cy @ cy) - cg) <= 1e-10 * cg
    # the mean reprojection error always uses the RS functor (impl.h:1017)
    assert abs(gpu.trajectory_.GetMeanReprojectionError() - cpu.trajectory_.GetMeanReprojectionError()) < 1e-9


def test_rs_time_in_seconds_option():
    ds = synthetic.make_config("tiny")
    gpu = E.ImuCameraCalibrator().BatchInitSpline(ds)
    cpu = E.ImuCameraCalibrator(backend=oracle_backend.load()).BatchInitSpline(ds)
    for c in (gpu, cpu):
        c.trajectory_.SetOption("rs_time_in_seconds", 1)
    flags = FLAGS1 | E.CAM_LINE_DELAY
    n = 2 * gpu.num_corners
    rg, Jg = gpu.trajectory_.EvaluateBlocks(flags, 0, n)
    rc, Jc = cpu.trajectory_.EvaluateBlocks(flags, 0, n)
    assert np.abs(rg - rc).max() <= 1e-11 * (1 + np.abs(rc).max())
    scale = np.abs(Jc).max(axis=1, keepdims=True) + 1e-6 * np.abs(Jc).max() + 1e-30
    assert (np.abs(Jg - Jc) / scale).max() < 1e-8
    # the fixed model shifts rows by ~20x more than the quirky one: residuals must differ
    gpu.trajectory_.SetOption("rs_time_in_seconds", 0)
    r0, _ = gpu.trajectory_.EvaluateBlocks(flags, 0, n, False)
    assert np.abs(r0 - rg).max() > 1e-3


def test_other_knot_spacings_change_bandwidth():
    """dt_so3/dt_r3 = 0.056/0.128 (Readme.md:45): different half bandwidth, same parity."""
    ds = synthetic.make_config("tiny", dt_so3=0.056, dt_r3=0.128, duration=2.4, num_views=24)
    gpu = E.ImuCameraCalibrator().BatchInitSpline(ds)
    cpu = E.ImuCameraCalibrator(backend=oracle_backend.load()).BatchInitSpline(ds)
    cg, Hg, gg = gpu.trajectory_.Evaluate(FLAGS1); cc, Hc, gc = cpu.trajectory_.Evaluate(FLAGS1)
    assert rel_err(Hg, Hc) < 1e-12 and rel_err(gg, gc) < 1e-11
    sg = gpu.trajectory_.Optimize(30, FLAGS1); sc = cpu.trajectory_.Optimize(30, FLAGS1)
    assert sg["half_bandwidth"] == sc["half_bandwidth"] == 56
    # With more rotation knots than views the valley floor is flat (cond(H) ~ 1e13): the
    # first iterates agree tightly, later ones only in cost.
    ig, ic = gpu.trajectory_.GetIterations(), cpu.trajectory_.GetIterations()
    for a, b in list(zip(ig, ic))[:3]:
        assert abs(a["cost"] - b["cost"]) <= 1e-8 * b["cost"]
    assert abs(sg["final_cost"] - sc["final_cost"]) <= 2e-3 * sc["final_cost"]


def test_block_cyclic_reduction_deep_tree_c4():
    """C4 (2000 views, ~18 k band columns -> ~290 blocks, 9 reduction levels): the first LM
    iterations with the block cyclic reduction equal those of the partitioned band sweep."""
    ds = synthetic.make_config("C4")
    costs = []
    for algo in (1, 0, 4):     # (0 = 4: the cyclic reduction through the inverses of the pivots)
        cal = E.ImuCameraCalibrator().BatchInitSpline(ds)
        cal.trajectory_.SetOption("solver_algorithm", algo)
        cal.trajectory_.Optimize(3, FLAGS1)
        costs.append([i["cost"] for i in cal.trajectory_.GetIterations()])
        steps = [i["step_norm"] for i in cal.trajectory_.GetIterations()]
        assert all(np.isfinite(steps))
    assert len(costs[0]) == len(costs[1]) == len(costs[2]) >= 3
    assert all(np.allclose(costs[0], c, rtol=1e-9, atol=0) for c in costs[1:])


@pytest.mark.parametrize("cfg", ["C2", "C4", "C5"])
def test_linear_solvers_leave_a_small_residual_at_full_size(cfg):
    """A size-independent check of the linear solvers, at the full size of BASELINE's configurations (C5: 90 k band columns, 1406
    blocks, 11 reduction levels): one damped solve, then ||M d - rhs|| / ||rhs|| with H and g from the packed normal equations but
    the scale and the damping D2 the route's own build wrote -- so a wrong damping term in a build passes here; the damping and the
    step against a host-built M: tests/test_gpu_linear_solve_reference.py.  The Cholesky-based solvers (band sweep, factor-based cyclic reduction) are backward stable: ~5e-16.  The cyclic
    reduction through the explicit inverses of the pivot blocks (the automatic choice) and the parallel cyclic reduction pay a
    factor of 10-150, still 1e-14 -- five orders below the tolerance of the LM iterate comparisons."""
    ds = synthetic.make_config(cfg)
    for algo, bound in ((1, 2e-14), (0, 1e-12), (4, 1e-12)):
        cal = E.ImuCameraCalibrator().BatchInitSpline(ds)
        cal.trajectory_.SetOption("solver_algorithm", algo)
        for radius in (1e4, 1e16):       # Ceres' initial radius; (almost) no damping: the normal equations as they are
            res, rhs_norm, failed = cal.trajectory_.SolveResidual(FLAGS1, radius)
            assert not failed and rhs_norm > 0 and res < bound, (cfg, algo, radius, res)


@pytest.mark.parametrize("cfg,ranks", [("C1", (2, 3, 5)), ("C2", (2, 3, 5, 8, 29)), ("C3", (4, 7)), ("C4", (8,)), ("C5", (2, 7, 8, 64))])
def test_distributed_cyclic_reduction_leaves_a_small_residual_at_full_size(cfg, ranks):
    """The distributed cyclic reduction (round 6) as ONE process runs it for N ranks on the unsharded problem (oicc_debug_dist_solve_
    emulated: every rank's forward part into its slot, every rank's top system + back substitution, the gathered step): the step
    against the packed normal equations (with the scale and D2 the ranks' builds wrote), ||M d - rhs|| / ||rhs|| < 1e-12 like the one-GPU cyclic reduction (undamped: within 100 x of it) -- block ranges
    of unequal length (7 ranks on 1407 blocks), one block per rank (29 ranks on C2's 29 blocks: no local level at all), ranges whose
    active block counts are odd at some level (the coupling to the ghost block carried on), 64 ranks (six levels of the top system);
    with Ceres' initial radius and (almost) undamped."""
    ds = synthetic.make_config(cfg)
    cal = E.ImuCameraCalibrator().BatchInitSpline(ds)
    for radius in (1e4, 1e16):
        one, _, failed1 = cal.trajectory_.SolveResidual(FLAGS1, radius)     # the one-GPU cyclic reduction on the same system
        assert not failed1
        for n in ranks:
            res, failed, fwd, mid = cal.trajectory_.DistributedSolveEmulated(FLAGS1, n, radius, repeats=1)
            # 1e-12 with Ceres' radius (measured: 3e-15 for 2-3 ranks, growing with the number of ranks to 3e-14 at 8 and 5e-13 at 29:
            # every rank solves the top system itself, its fp64 atomics arrive in its own order, and the step is a patchwork of N
            # solutions that each solve a slightly different nearby system -- the pieces differ by the FORWARD error, cond x eps);
            # undamped, where the small configurations' knots beyond the last measurement are barely determined, 1e-8 (measured
            # <= 6e-10; one GPU 3e-14)
            assert not failed and res < (1e-12 if radius == 1e4 else 1e-8), (cfg, n, radius, res, one)
            assert len(fwd) == n and (fwd > 0).all() and (mid > 0).all()


def test_cyclic_reduction_on_c3_through_rejected_steps():
    """C3 (606 + 306 knots: 43 blocks, 6 levels of the cyclic reduction through the pivot inverses) against the partitioned band sweep,
    with LDS poisoned before every solve and through rejected steps (a start far from the valley)."""
    ds = synthetic.make_config("C3")
    costs = []
    for algo in (1, 4):
        cal = E.ImuCameraCalibrator().BatchInitSpline(ds)
        cal.trajectory_.SetOption("solver_algorithm", algo); cal.trajectory_.SetOption("debug_poison_lds", 1)
        cal.trajectory_.SetOption("initial_trust_region_radius", 1e9)      # the first steps overshoot: rejected steps, reused diagonals
        s_ = cal.trajectory_.Optimize(8, FLAGS1)
        costs.append([(i["cost"], i["step_is_successful"]) for i in cal.trajectory_.GetIterations()])
    assert len(costs[0]) == len(costs[1]) >= 4
    for other in costs[1:]:
        assert all(a[1] == b[1] and abs(a[0] - b[0]) <= 1e-9 * b[0] for a, b in zip(costs[0], other))


@pytest.mark.parametrize("algo", [1, 4])
@pytest.mark.parametrize("duration,views", [(0.3, 3), (0.75, 8)])
def test_very_short_trajectories_single_and_two_block_band(algo, duration, views):
    """Band of <= 64 columns (one block: only the last elimination runs) and of two blocks."""
    ds = synthetic.make_config("tiny", duration=duration, num_views=views)
    gpu = E.ImuCameraCalibrator().BatchInitSpline(ds)
    cpu = E.ImuCameraCalibrator(backend=oracle_backend.load()).BatchInitSpline(ds)
    gpu.trajectory_.SetOption("solver_algorithm", algo)
    sg = gpu.trajectory_.Optimize(8, FLAGS1); sc = cpu.trajectory_.Optimize(8, FLAGS1)
    assert sg["band_dim"] == sc["band_dim"] and sg["band_dim"] <= (64 if views == 3 else 128)
    ig, ic = gpu.trajectory_.GetIterations(), cpu.trajectory_.GetIterations()
    for a, b in list(zip(ig, ic))[:3]:
        assert abs(a["cost"] - b["cost"]) <= 1e-8 * b["cost"] and a["step_is_successful"] == b["step_is_successful"]


def test_native_rccl_reduction_single_rank():
    """oicc_rccl_init with a one-rank communicator: ncclAllReduce in place on the library's stream must leave the
    normal equations and the LM iterates unchanged (the N > 1 logic is covered by tests/test_distributed_gloo.py)."""
    ds = synthetic.make_config("tiny")
    ref = E.ImuCameraCalibrator().BatchInitSpline(ds)
    par = E.ImuCameraCalibrator().BatchInitSpline(ds)
    par.trajectory_.EnableRccl(1, 0, par.trajectory_.RcclUniqueId())
    c0, H0, g0 = ref.trajectory_.Evaluate(FLAGS1); c1, H1, g1 = par.trajectory_.Evaluate(FLAGS1)
    assert abs(c0 - c1) <= 1e-12 * c0 and rel_err(H1, H0) < 1e-12 and rel_err(g1, g0) < 1e-12
    s0 = ref.trajectory_.Optimize(20, FLAGS1); s1 = par.trajectory_.Optimize(20, FLAGS1)
    assert s0["num_iterations"] == s1["num_iterations"] and abs(s0["final_cost"] - s1["final_cost"]) <= 1e-9 * s0["final_cost"]


def _recovery_errors(ds, tr):
    T = tr.GetT_i_c()
    ang = 2 * np.arccos(min(1.0, abs(float(T[:4] @ ds.truth["q_i_c"]))))
    return ang, np.abs(T[4:] - ds.truth["t_i_c"]).max(), np.abs(tr.GetGravity() - ds.truth["gravity"]).max()


def test_c3_fisheye_full_calibration():
    """BASELINE config 3 (GoPro6 FISHEYE, 900 views x 40 corners, 6000 IMU samples, 606 SO3 / 306 R3 knots):
    cost / gradient parity with the oracle at full size, EVERY LM iterate up to convergence equals the Jet oracle's, and the
    full calibration recovers the planted T_i_c / gravity (tolerances of SURVEY 8c: noisy data, CRLB scale)."""
    ds, gpu, cpu = build_pair("C3")
    cg, _, gg = gpu.trajectory_.Evaluate(FLAGS1, want_H=False)
    cc, _, gc = cpu.trajectory_.Evaluate(FLAGS1, want_H=False)
    assert abs(cg - cc) <= 1e-10 * cc and rel_err(gg, gc) < 1e-10
    cpu.trajectory_.SetOption("analytic_jacobians", 0)   # Jets on the checker's side, every iterate up to convergence
    sc = cpu.trajectory_.Optimize(50, FLAGS1)
    sg = gpu.trajectory_.Optimize(50, FLAGS1)
    ig, ic = gpu.trajectory_.GetIterations(), cpu.trajectory_.GetIterations()
    assert sg["termination"] == sc["termination"] == 0 and sg["num_iterations"] == sc["num_iterations"] >= 4 and len(ig) == len(ic)
    for a, b in zip(ig, ic):
        assert abs(a["cost"] - b["cost"]) <= 1e-8 * b["cost"] and a["step_is_successful"] == b["step_is_successful"]
        assert abs(a["step_norm"] - b["step_norm"]) <= 1e-6 * max(b["step_norm"], 1e-12), (a, b)
    assert np.abs(gpu.trajectory_.GetT_i_c() - cpu.trajectory_.GetT_i_c()).max() < 1e-7
    assert sg["final_cost"] < 0.05 * sg["initial_cost"]
    ang, dt, dg = _recovery_errors(ds, gpu.trajectory_)
    assert ang < np.deg2rad(0.5) and dt < 5e-3 and dg < 0.05      # same 0.5 deg as the C2 test: the quirk-Q1 row-time model is not the one that generated the data
    assert gpu.trajectory_.GetMeanReprojectionError() < 1.0


def test_c4_double_sphere_line_delay_calibration():
    """BASELINE config 4 (DOUBLE_SPHERE, 2000 views x 40 rolling-shutter corners): stage 1, then stage 2 with the line
    delay as the only variable (continuous_time_imu_to_camera_calibration.cc:226-239).  Default (quirk Q1) mode: cost
    parity with the oracle, both stages descend.  With the documented fix rs_time_in_seconds the synthetic data
    (generated with row times in seconds) lets a JOINT spline + T_i_c + line-delay solve recover the planted line delay
    from a 40 % wrong start (stage 2 alone cannot: the stage-1 spline has absorbed the wrong row times)."""
    ds = synthetic.make_config("C4")
    gpu = E.ImuCameraCalibrator().BatchInitSpline(ds)
    cpu = E.ImuCameraCalibrator(backend=oracle_backend.load()).BatchInitSpline(ds)
    cc, _, gc = cpu.trajectory_.Evaluate(FLAGS1, want_H=False)                  # forward-mode Jets over 80 000 corners + 16 000 IMU blocks
    cg, _, gg = gpu.trajectory_.Evaluate(FLAGS1, want_H=False)
    assert abs(cg - cc) <= 1e-10 * cc and rel_err(gg, gc) < 1e-10
    assert abs(gpu.trajectory_.EvaluateCost(FLAGS1) - cc) <= 1e-10 * cc
    s1 = gpu.trajectory_.Optimize(50, FLAGS1)
    assert s1["termination"] == 0 and s1["final_cost"] < 0.05 * s1["initial_cost"]
    s2 = gpu.trajectory_.Optimize(10, E.CAM_LINE_DELAY)
    assert s2["num_parameters_tangent"] == 1 and s2["final_cost"] <= s2["initial_cost"]
    ang, dt, _ = _recovery_errors(ds, gpu.trajectory_)
    assert ang < np.deg2rad(0.5) and dt < 5e-3
    # physical row-time model
    true_ld = ds.truth["line_delay"]
    ds.line_delay_init = 0.6 * true_ld
    fix = E.ImuCameraCalibrator()
    fix.trajectory_.SetOption("rs_time_in_seconds", 1)
    fix.BatchInitSpline(ds)
    fix.trajectory_.SetOption("function_tolerance", 1e-9)
    f2 = fix.trajectory_.Optimize(50, FLAGS1 | E.CAM_LINE_DELAY)
    assert f2["final_cost"] < 0.05 * f2["initial_cost"] and abs(fix.trajectory_.GetRSLineDelay() - true_ld) < 0.1 * true_ld


def test_c5_time_shards_sum_to_the_whole():
    """BASELINE config 5 (10 k views x 50 corners + 200 k IMU samples, P ~ 90 k) at full size on ONE GPU: the
    multi-GPU decomposition is a sum -- cost and gradient of the four time shards (each built exactly as
    rank r of 4 would, remote measurements declared) add up to those of the whole problem, and one LM iteration on the
    whole problem (12 reduction levels of the block cyclic reduction) descends."""
    ds = synthetic.make_config("C5")
    whole = E.ImuCameraCalibrator().BatchInitSpline(ds)
    c_all, _, g_all = whole.trajectory_.Evaluate(FLAGS1, want_H=False)
    c_sum, g_sum, blocks = 0.0, np.zeros_like(g_all), 0
    for r in range(4):
        part = E.ImuCameraCalibrator().BatchInitSpline(ds, shard=(r, 4))
        c, _, g = part.trajectory_.Evaluate(FLAGS1, want_H=False)
        assert g.shape == g_all.shape          # identical tangent layout on every rank
        c_sum += c; g_sum += g; blocks += part.num_blocks
    assert blocks == whole.num_blocks
    assert abs(c_sum - c_all) <= 1e-11 * c_all and rel_err(g_sum, g_all) < 1e-10
    idx = np.arange(len(g_all))
    diag = whole.trajectory_.EvaluateEntries(FLAGS1, idx, idx)
    d = np.sqrt(diag)                       # every gradient entry on its own scale d_i sqrt(2 cost)
    ok = (d > 0) & ~NER.weak_from_diagonal(diag, NER.column_kinds(whole.trajectory_.GetTangentLayout(FLAGS1)))
    assert not g_sum[d == 0].any() and not g_all[d == 0].any()
    eg = (np.abs(g_sum - g_all)[ok] / (d[ok] * np.sqrt(2 * c_all))).max()
    print("entry-wise: g %.2e" % eg)
    assert eg < 1e-10, eg
    # ... and the whole against the CPU oracle (forward-mode Jets, 410 000 residual blocks, P ~ 90 k): cost and gradient
    cpu = E.ImuCameraCalibrator(backend=oracle_backend.load()).BatchInitSpline(ds)
    c_cpu, _, g_cpu = cpu.trajectory_.Evaluate(FLAGS1, want_H=False)
    assert g_cpu.shape == g_all.shape and abs(c_all - c_cpu) <= 1e-10 * c_cpu and rel_err(g_all, g_cpu) < 1e-10
    eg = (np.abs(g_all - g_cpu)[ok] / (d[ok] * np.sqrt(2 * c_cpu))).max()
    print("entry-wise: g %.2e" % eg)
    assert eg < 1e-10, eg
    s = whole.trajectory_.Optimize(1, FLAGS1)
    assert s["num_successful_steps"] == 1 and s["final_cost"] < 0.5 * s["initial_cost"] and s["band_dim"] > 85000
    # at this size the segment tables come once per parameter vector (written by the retraction kernel for the candidate);
    # the same iteration with every tile computing its own gives the same candidate cost
    alt = E.ImuCameraCalibrator().BatchInitSpline(ds)
    alt.trajectory_.SetOption("debug_seg_precompute", 2)
    s2 = alt.trajectory_.Optimize(1, FLAGS1)
    assert abs(s2["final_cost"] - s["final_cost"]) <= 1e-10 * s["final_cost"]


def test_wide_band_falls_back_to_the_global_memory_solver():
    """dt_r3 << dt_so3 (what the spline error weighting picks for noisy accelerometer data): half bandwidth > 200, beyond
    both LDS solvers; the global-memory band Cholesky takes over and the LM iterates still equal the oracle's."""
    ds = synthetic.make_config("tiny", dt_so3=0.2, dt_r3=0.017, duration=2.0, num_views=20)
    gpu = E.ImuCameraCalibrator().BatchInitSpline(ds)
    cpu = E.ImuCameraCalibrator(backend=oracle_backend.load()).BatchInitSpline(ds)
    sg = gpu.trajectory_.Optimize(6, FLAGS1); sc = cpu.trajectory_.Optimize(6, FLAGS1)
    assert sg["half_bandwidth"] == sc["half_bandwidth"] > 128
    ig, ic = gpu.trajectory_.GetIterations(), cpu.trajectory_.GetIterations()
    assert len(ig) == len(ic) >= 3
    for a, b in list(zip(ig, ic))[:4]:
        assert abs(a["cost"] - b["cost"]) <= 1e-8 * b["cost"] and a["step_is_successful"] == b["step_is_successful"]


@pytest.mark.parametrize("camera", ["gopro6_double_sphere", "gopro9_eucm"])
def test_failed_projection_gives_1e10_residual_and_zero_jacobian(camera):
    """ceres_calib_split_residuals.h:391-393: a corner whose projection fails (here: a board point moved behind the
    camera of a model with a validity cone) contributes the residual (1e10, 1e10) and no derivative."""
    if camera not in synthetic.CAMERAS:
        pytest.skip("camera preset not defined")
    ds = synthetic.make_config("tiny", camera=camera)
    ds.points = ds.points.copy(); ds.points[0] = [0.0, 0.0, 5.0, 1.0]          # behind the camera that looks down -z at the board
    gpu = E.ImuCameraCalibrator().BatchInitSpline(ds)
    cpu = E.ImuCameraCalibrator(backend=oracle_backend.load()).BatchInitSpline(ds)
    n = 2 * gpu.num_corners
    rg, Jg = gpu.trajectory_.EvaluateBlocks(FLAGS1, 0, n)
    rc, Jc = cpu.trajectory_.EvaluateBlocks(FLAGS1, 0, n)
    bad = np.abs(rc) >= 1e10
    assert bad.sum() >= 2 and np.array_equal(np.abs(rg) >= 1e10, bad)
    assert np.all(rg[bad] == 1e10) and np.all(Jg[bad] == 0.0) and np.all(Jc[bad] == 0.0)
    ok = ~bad
    assert np.abs(rg[ok] - rc[ok]).max() <= 1e-11 * (1 + np.abs(rc[ok]).max())
    scale = np.abs(Jc[ok]).max(axis=1, keepdims=True) + 1e-6 * np.abs(Jc[ok]).max() + 1e-30
    assert (np.abs(Jg[ok] - Jc[ok]) / scale).max() < 1e-8
    cg = gpu.trajectory_.EvaluateCost(FLAGS1); cc = cpu.trajectory_.EvaluateCost(FLAGS1)
    assert abs(cg - cc) <= 1e-12 * cc and cc > 1e19


def test_ragged_views_empty_view_and_views_above_64_corners():
    """Views with 80 corners (split into two work-list chunks of 64 + 16), a view with half of its corners and a view
    with none: normal equations and LM iterates equal the oracle's; the empty view triggers quirk Q6
    (GetMeanReprojectionError returns 0.0, impl.h:1002-1004)."""
    ds = synthetic.make_config("tiny", board=(10, 8), corners_per_view=80)
    assert ds.num_corners == 80 * ds.num_views
    keep = np.ones(ds.num_corners, dtype=bool)
    a3, b3 = ds.corner_offset[3], ds.corner_offset[4]; keep[a3:b3] = False                 # view 3: empty
    a5, b5 = ds.corner_offset[5], ds.corner_offset[6]; keep[a5 + 40:b5] = False            # view 5: 40 corners
    counts = np.array([keep[ds.corner_offset[v]:ds.corner_offset[v + 1]].sum() for v in range(ds.num_views)])
    ds.corner_uv = ds.corner_uv[keep]; ds.corner_point = ds.corner_point[keep]
    ds.corner_offset = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    gpu = E.ImuCameraCalibrator().BatchInitSpline(ds)
    cpu = E.ImuCameraCalibrator(backend=oracle_backend.load()).BatchInitSpline(ds)
    cg, Hg, gg = gpu.trajectory_.Evaluate(FLAGS1); cc, Hc, gc = cpu.trajectory_.Evaluate(FLAGS1)
    assert abs(cg - cc) <= 1e-11 * cc and rel_err(Hg, Hc) < 1e-10 and rel_err(gg, gc) < 1e-10
    sg = gpu.trajectory_.Optimize(10, FLAGS1); sc = cpu.trajectory_.Optimize(10, FLAGS1)
    assert sg["num_iterations"] == sc["num_iterations"] and abs(sg["final_cost"] - sc["final_cost"]) <= 1e-8 * sc["final_cost"]
    assert gpu.trajectory_.GetMeanReprojectionError() == 0.0 == cpu.trajectory_.GetMeanReprojectionError()


# ---- time-tile assembly (kernels_tiles.hip): LDS accumulators + slab merge vs direct atomics ----
@pytest.mark.parametrize("wide", [1, 0])
@pytest.mark.parametrize("mode,tile_windows", [(0, 0), (0, 1), (0, 3), (0, 7), (0, 64), (2, 0), (2, 5)])
def test_assembly_modes_match_the_oracle(tiny, mode, tile_windows, wide):
    """Every way the normal equations can be assembled gives the oracle's J^T J / J^T r / cost: tiles of 1 ... all windows
    (halo rows summed by the merge kernel), tiles in direct mode (fp64 atomics)."""
    ds, _, cpu = tiny
    gpu = E.ImuCameraCalibrator().BatchInitSpline(ds)
    gpu.trajectory_.SetOption("assembly", mode); gpu.trajectory_.SetOption("tile_windows", tile_windows); gpu.trajectory_.SetOption("wide_cells", wide)
    for flags in (FLAGS1, FLAGS1 | E.IMU_BIASES, FLAGS1 | E.CAM_LINE_DELAY | E.IMU_BIASES | E.IMU_INTRINSICS, E.CAM_LINE_DELAY):
        cg, Hg, gg = gpu.trajectory_.Evaluate(flags); cc, Hc, gc = cpu.trajectory_.Evaluate(flags)
        assert abs(cg - cc) <= 1e-11 * cc, (flags, cg, cc)
        assert rel_err(Hg, Hc) < 1e-10 and rel_err(gg, gc) < 1e-10, (flags, rel_err(Hg, Hc), rel_err(gg, gc))
        eh, eg = entry_err(gpu.trajectory_, flags, Hg, Hc, gg, gc, cc)
        assert eh < 1e-10 and eg < 1e-10, (flags, eh, eg)
        assert np.abs(Hg - Hg.T).max() <= 1e-13 * np.abs(Hg).max()
        assert NER.symmetry_error(Hg, Hc) <= 1e-13
        assert abs(gpu.trajectory_.EvaluateCost(flags) - cc) <= 1e-11 * cc


def test_tiles_are_run_to_run_reproducible_up_to_lds_order():
    """Two passes over the same problem: the slab merge sums tiles in a fixed order, so the only freedom left is the order of
    the LDS additions inside a tile (a few ulp)."""
    ds = synthetic.make_config("C2")
    gpu = E.ImuCameraCalibrator().BatchInitSpline(ds)
    c0, H0, g0 = gpu.trajectory_.Evaluate(FLAGS1)
    c1, H1, g1 = gpu.trajectory_.Evaluate(FLAGS1)
    assert abs(c0 - c1) <= 1e-14 * c0 and rel_err(H1, H0) < 1e-14 and rel_err(g1, g0) < 1e-13
    eh, eg = entry_err(gpu.trajectory_, FLAGS1, H1, H0, g1, g0, c0)
    assert eh < 1e-14 and eg < 1e-13, (eh, eg)


@pytest.mark.parametrize("cfg,flags,chain", [("C2", FLAGS1, 0), ("C2", FLAGS1 | E.IMU_BIASES, 4), ("C3", FLAGS1, 3)])
def test_deterministic_accumulation_is_bit_identical(cfg, flags, chain):
    """Option accumulation = 1: one wave per chain takes the units in their fixed order, the merge sums the chains in a fixed order --
    every sum of the Jacobian pass has ONE order.  Two passes of one problem and a pass of a second problem object give the same
    BITS (cost, gradient, every entry of J^T J), so a parity failure can be bisected bit for bit; the default (four waves, LDS
    additions in arrival order) agrees to rounding."""
    ds = synthetic.make_config(cfg)
    out = []
    for rep in range(2):
        c = E.ImuCameraCalibrator().BatchInitSpline(ds)
        c.trajectory_.SetOption("accumulation", 1); c.trajectory_.SetOption("chain_tiles", chain)
        out.append(c.trajectory_.Evaluate(flags))
        if rep == 0: out.append(c.trajectory_.Evaluate(flags))
    (c0, H0, g0) = out[0]
    for (c1, H1, g1) in out[1:]:
        assert c0 == c1 and np.array_equal(H0, H1) and np.array_equal(g0, g1)
    d = E.ImuCameraCalibrator().BatchInitSpline(ds)
    cd, Hd, gd = d.trajectory_.Evaluate(flags)
    assert abs(cd - c0) <= 1e-13 * c0 and rel_err(Hd, H0) < 1e-13 and rel_err(gd, g0) < 1e-12
    eh, eg = entry_err(d.trajectory_, flags, Hd, H0, gd, g0, c0)
    assert eh < 1e-13 and eg < 1e-12, (eh, eg)


@pytest.mark.parametrize("cfg,chain,tile_windows", [("C2", 3, 0), ("C2", 7, 4), ("C3", 2, 0), ("C3", 25, 0), ("C1", 100, 2)])
def test_chains_of_tiles_equal_single_tiles(cfg, chain, tile_windows):
    """Round 4: a workgroup walks a CHAIN of consecutive tiles with a ring accumulator (a knot's rows stay in LDS from the first to the
    last tile that touches it and are stored once; only the rows at the two ends of a chain go through slabs).  Any chain length --
    including one chain for the whole problem -- gives the sums of one-tile chains (option chain_tiles) and of the direct-atomics mode."""
    ds = synthetic.make_config(cfg)
    a = E.ImuCameraCalibrator().BatchInitSpline(ds); b = E.ImuCameraCalibrator().BatchInitSpline(ds); c = E.ImuCameraCalibrator().BatchInitSpline(ds)
    for x in (a, b):
        x.trajectory_.SetOption("tile_windows", tile_windows)
    a.trajectory_.SetOption("chain_tiles", chain); b.trajectory_.SetOption("chain_tiles", 1); c.trajectory_.SetOption("assembly", 2)
    a.trajectory_.SetOption("debug_poison_lds", 1)
    ca, Ha, ga = a.trajectory_.Evaluate(FLAGS1); cb, Hb, gb = b.trajectory_.Evaluate(FLAGS1); cc, Hc, gc = c.trajectory_.Evaluate(FLAGS1)
    assert abs(ca - cb) <= 1e-13 * cb and rel_err(Ha, Hb) < 1e-13 and rel_err(ga, gb) < 1e-12
    assert abs(ca - cc) <= 1e-12 * cc and rel_err(Ha, Hc) < 1e-12 and rel_err(ga, gc) < 1e-11
    eh, eg = entry_err(a.trajectory_, FLAGS1, Ha, Hb, ga, gb, cb)
    assert eh < 1e-13 and eg < 1e-12, (eh, eg)
    eh, eg = entry_err(a.trajectory_, FLAGS1, Ha, Hc, ga, gc, cc)
    assert eh < 1e-12 and eg < 1e-11, (eh, eg)
    assert abs(a.trajectory_.EvaluateCost(FLAGS1) - ca) <= 1e-13 * ca      # the cost-only pass walks the same chains
    sa = a.trajectory_.Optimize(8, FLAGS1); sb = b.trajectory_.Optimize(8, FLAGS1)
    assert sa["num_iterations"] == sb["num_iterations"] and abs(sa["final_cost"] - sb["final_cost"]) <= 1e-9 * sb["final_cost"]


@pytest.mark.parametrize("cfg,tile_windows", [("C2", 0), ("C2", 2), ("C3", 0)])
def test_tiles_on_baseline_configs_match_direct_atomics(cfg, tile_windows):
    """Full-size BASELINE configurations: tiled assembly against the direct-atomics mode of the same kernel (independent
    accumulation paths: LDS + slabs + merge vs global fp64 atomics)."""
    ds = synthetic.make_config(cfg)
    a = E.ImuCameraCalibrator().BatchInitSpline(ds); b = E.ImuCameraCalibrator().BatchInitSpline(ds)
    a.trajectory_.SetOption("tile_windows", tile_windows)
    b.trajectory_.SetOption("assembly", 2)
    ca, _, ga = a.trajectory_.Evaluate(FLAGS1, want_H=False); cb, _, gb = b.trajectory_.Evaluate(FLAGS1, want_H=False)
    assert abs(ca - cb) <= 1e-12 * cb and rel_err(ga, gb) < 1e-11
    sa = a.trajectory_.Optimize(8, FLAGS1); sb = b.trajectory_.Optimize(8, FLAGS1)
    assert sa["num_iterations"] == sb["num_iterations"] and abs(sa["final_cost"] - sb["final_cost"]) <= 1e-9 * sb["final_cost"]


@pytest.mark.parametrize("cfg,tile_windows,flags", [("C2", 8, FLAGS1), ("C2", 16, FLAGS1 | E.IMU_BIASES), ("C3", 0, FLAGS1)])
def test_interior_rows_stored_by_the_tile_equal_the_slab_route(cfg, tile_windows, flags):
    """Accumulator rows that belong to one tile only are written into the packed normal equations by the tile kernel itself,
    the halo rows go through the slabs and the merge kernel.  Routing every row through the slabs (debug_no_direct_rows) must
    give the same matrix (bit for bit on the interior rows; the LDS addition order of a tile varies from launch to launch by a few ulp) and both must match the oracle."""
    ds = synthetic.make_config(cfg)
    a = E.ImuCameraCalibrator().BatchInitSpline(ds); b = E.ImuCameraCalibrator().BatchInitSpline(ds)
    for c in (a, b):
        c.trajectory_.SetOption("tile_windows", tile_windows)
    b.trajectory_.SetOption("debug_no_direct_rows", 1)
    ca, Ha, ga = a.trajectory_.Evaluate(flags); cb, Hb, gb = b.trajectory_.Evaluate(flags)
    assert abs(ca - cb) <= 1e-14 * cb and rel_err(Ha, Hb) < 1e-13 and rel_err(ga, gb) < 1e-12
    eh, eg = entry_err(a.trajectory_, flags, Ha, Hb, ga, gb, cb)
    assert eh < 1e-13 and eg < 1e-12, (eh, eg)
    assert np.abs(Ha - Ha.T).max() <= 1e-13 * np.abs(Ha).max()
    cpu = E.ImuCameraCalibrator(backend=oracle_backend.load()).BatchInitSpline(ds)
    cpu.trajectory_.SetOption("analytic_jacobians", 0)   # forward-mode Jets: none of the product's closed forms on the checker's side
    cc, Hc, gc = cpu.trajectory_.Evaluate(flags)
    assert abs(ca - cc) <= 1e-11 * cc and rel_err(Ha, Hc) < 1e-10 and rel_err(ga, gc) < 1e-10
    eh, eg = entry_err(a.trajectory_, flags, Ha, Hc, ga, gc, cc)
    assert eh < 1e-10 and eg < 1e-10 and NER.symmetry_error(Ha, Hc) <= 1e-13, (eh, eg)
    sa = a.trajectory_.Optimize(6, flags); sb = b.trajectory_.Optimize(6, flags)
    assert sa["num_iterations"] == sb["num_iterations"] and abs(sa["final_cost"] - sb["final_cost"]) <= 1e-9 * sb["final_cost"]


@pytest.mark.parametrize("cfg,flags,inner", [("C2", FLAGS1, 0), ("tiny", FLAGS1 | E.IMU_BIASES, 1), ("C1", FLAGS1 | E.ACC_BIAS, 0)])   # (C1 with the line delay free is chaotic from run to run within ONE mode: scripts/dbg_segdiff.py)
def test_segment_tables_per_parameter_vector_equal_per_tile(cfg, flags, inner):
    """The per-knot-pair segment tables (log of the relative rotation, J_r^-1) are either computed by every tile for its own
    knots (small problems) or once per parameter vector -- by the retraction kernel for the candidate, by a small kernel
    otherwise -- and kept valid across accepted steps, inner sweeps and line-search trials.  Both routes run the same code
    on the same knots: identical solves."""
    ds = synthetic.make_config(cfg)
    a = E.ImuCameraCalibrator().BatchInitSpline(ds); b = E.ImuCameraCalibrator().BatchInitSpline(ds)
    a.trajectory_.SetOption("debug_seg_precompute", 1); b.trajectory_.SetOption("debug_seg_precompute", 2)
    for c in (a, b):
        c.trajectory_.SetOption("inner_iterations", inner); c.trajectory_.SetOption("bounds_line_search", 1)
    ca, Ha, ga = a.trajectory_.Evaluate(flags); cb, Hb, gb = b.trajectory_.Evaluate(flags)
    assert abs(ca - cb) <= 1e-14 * cb and rel_err(Ha, Hb) < 1e-13 and rel_err(ga, gb) < 1e-12
    # (ten iterations: the candidate's tables come from a second inlined copy of the retraction arithmetic, whose FMA contraction
    # may differ in the last bit; the inner-iteration solves amplify that over dozens of iterations)
    sa = a.trajectory_.Optimize(10, flags); sb = b.trajectory_.Optimize(10, flags)
    ia, ib = a.trajectory_.GetIterations(), b.trajectory_.GetIterations()
    assert sa["num_iterations"] == sb["num_iterations"], ([i["cost"] for i in ia], [i["cost"] for i in ib])
    for x, y in zip(ia, ib):
        assert x["step_is_successful"] == y["step_is_successful"] and abs(x["cost"] - y["cost"]) <= 1e-8 * y["cost"], (x, y)
    assert np.abs(a.trajectory_.GetT_i_c() - b.trajectory_.GetT_i_c()).max() < 1e-7
    # a second solve from the accepted point (tables of the swapped buffers still valid) and a host-side parameter change
    for c in (a, b):
        c.trajectory_.SetGravity(np.array([0.05, -0.03, 9.79]))
    assert abs(a.trajectory_.EvaluateCost(flags) - b.trajectory_.EvaluateCost(flags)) <= 1e-7 * b.trajectory_.EvaluateCost(flags)   # (the iterates agree to 1e-8; a stale table would be a gross error)


# ---- Ceres' inner iterations (reference impl.h:266), device sweep (inner_iterations.hip) against oracle/ceres_inner.hpp ----
@pytest.mark.parametrize("cfg,flags", [("tiny", FLAGS1), ("tiny", FLAGS1 | E.IMU_BIASES), ("tiny", FLAGS1 | E.CAM_LINE_DELAY), ("C2", FLAGS1), ("C3", FLAGS1), ("C4", FLAGS1)])
def test_inner_iterations_match_the_oracle(cfg, flags):
    """use_inner_iterations = true: after every candidate one block coordinate descent sweep over the independent sets of the
    parameter blocks.  Same outer iterate sequence (costs to 1e-7: hundreds of small LM loops whose accept / reject decisions
    see the summation order) and final extrinsics as the CPU restatement with forward-mode Jets (analytic_jacobians = 0), at the
    full size of BASELINE configs 2-4, followed by the application's stage 2 (line delay only) with the same options."""
    ds = synthetic.make_config(cfg)
    gpu = E.ImuCameraCalibrator().BatchInitSpline(ds)
    cpu = E.ImuCameraCalibrator(backend=oracle_backend.load()).BatchInitSpline(ds)
    for c in (gpu, cpu):
        c.trajectory_.SetOption("inner_iterations", 1)
    cpu.trajectory_.SetOption("analytic_jacobians", 0)
    sg = gpu.trajectory_.Optimize(50, flags); sc = cpu.trajectory_.Optimize(50, flags)
    ig, ic = gpu.trajectory_.GetIterations(), cpu.trajectory_.GetIterations()
    assert sg["num_iterations"] == sc["num_iterations"], ([i["cost"] for i in ig], [i["cost"] for i in ic])
    assert sg["inner_sweeps"] == sc["inner_sweeps"] >= 1
    # Round 6: with the application's flag set the tolerances are SURVEY 8(c)'s or tighter -- cost 1e-9 (8c: 1e-8), T_i_c / gravity 1e-9
    # (8c: 1e-7), identical totals of per-block LM iterations -- two orders above what scripts/dbg_c5_margins.py measures
    # (profiles/r06l_parity_margins.log: costs <= 2e-12, T_i_c <= 5e-13, gravity <= 2e-12, the totals identical at every configuration);
    # the other flag sets of the tiny problem keep the round-3 tolerances (bias knots at their bounds: not measured)
    tight = flags == FLAGS1
    for a, b in zip(ig, ic):
        assert a["step_is_successful"] == b["step_is_successful"] and abs(a["cost"] - b["cost"]) <= (1e-9 if tight else 1e-7) * b["cost"], (a, b)
    assert np.abs(gpu.trajectory_.GetT_i_c() - cpu.trajectory_.GetT_i_c()).max() < (1e-9 if tight else 1e-6)
    assert np.abs(gpu.trajectory_.GetGravity() - cpu.trajectory_.GetGravity()).max() < (1e-9 if tight else 1e-5)
    if tight:
        assert abs(sg["inner_lm_iterations"] - sc["inner_lm_iterations"]) <= 1e-3 * sc["inner_lm_iterations"] + 1, (sg["inner_lm_iterations"], sc["inner_lm_iterations"])
        for a, b in zip(gpu.trajectory_.GetKnots(), cpu.trajectory_.GetKnots()):
            assert (np.abs(a - b) / (1 + np.abs(b))).max() < 1e-8
    if cfg != "tiny":   # stage 2 of the application (continuous_time_imu_to_camera_calibration.cc:217-221): one parameter block -> Ceres disables the sweep
        s2g = gpu.trajectory_.Optimize(10, E.CAM_LINE_DELAY); s2c = cpu.trajectory_.Optimize(10, E.CAM_LINE_DELAY)
        assert s2g["num_iterations"] == s2c["num_iterations"] and s2g["inner_sweeps"] == s2c["inner_sweeps"] == 0
        assert abs(s2g["final_cost"] - s2c["final_cost"]) <= 1e-10 * s2c["final_cost"]
        assert abs(gpu.trajectory_.GetRSLineDelay() - cpu.trajectory_.GetRSLineDelay()) < 1e-12
        assert abs(gpu.trajectory_.GetMeanReprojectionError() - cpu.trajectory_.GetMeanReprojectionError()) < 1e-10
    # and the sweep changes the trajectory of the solve (it is not a no-op)
    plain = E.ImuCameraCalibrator().BatchInitSpline(ds)
    sp = plain.trajectory_.Optimize(50, flags)
    assert abs(sp["final_cost"] - sg["final_cost"]) > 1e-9 * sg["final_cost"]


def _with_measurement_gap(ds, t0, t1):
    """The data set without the views and IMU samples of [t0, t1) s (relative to the first view)."""
    import dataclasses
    base = ds.view_t_s.min()
    keep_v = np.where(~((ds.view_t_s - base >= t0) & (ds.view_t_s - base < t1)))[0]
    keep_i = ~((ds.imu_t_s - base >= t0) & (ds.imu_t_s - base < t1))
    off, uv, pt = [0], [], []
    for v in keep_v:
        a, b = ds.corner_offset[v], ds.corner_offset[v + 1]
        uv.append(ds.corner_uv[a:b]); pt.append(ds.corner_point[a:b]); off.append(off[-1] + (b - a))
    return dataclasses.replace(ds, view_t_s=ds.view_t_s[keep_v], view_q_wc=ds.view_q_wc[keep_v], view_p_wc=ds.view_p_wc[keep_v],
                               corner_offset=np.asarray(off, np.int64), corner_uv=np.concatenate(uv), corner_point=np.concatenate(pt).astype(np.int32),
                               imu_t_s=ds.imu_t_s[keep_i], accel=ds.accel[keep_i], gyro=ds.gyro[keep_i])


def test_inner_iterations_across_a_measurement_gap():
    """A pause of 1.1 s without views or IMU samples (longer than the support of a knot in either spline): the first SO(3) knot
    behind the gap is the FIRST knot of all its items' windows, so the knot pair in front of it is not part of the block's staged
    neighbourhood (round-3 advisor finding: the LDS mirror of that pair's segment table was written out of bounds).  Sweeps and
    outer iterates as the Jet oracle, also under LDS poison."""
    ds = _with_measurement_gap(synthetic.make_config("C1"), 1.0, 2.1)
    gpu = E.ImuCameraCalibrator().BatchInitSpline(ds)
    cpu = E.ImuCameraCalibrator(backend=oracle_backend.load()).BatchInitSpline(ds)
    for c in (gpu, cpu):
        c.trajectory_.SetOption("inner_iterations", 1)
    gpu.trajectory_.SetOption("debug_poison_lds", 1)
    cpu.trajectory_.SetOption("analytic_jacobians", 0)
    sg = gpu.trajectory_.Optimize(50, FLAGS1); sc = cpu.trajectory_.Optimize(50, FLAGS1)
    ig, ic = gpu.trajectory_.GetIterations(), cpu.trajectory_.GetIterations()
    assert sg["num_parameters_tangent"] == sc["num_parameters_tangent"] < 3 * (gpu.trajectory_.GetNumSO3Knots() + gpu.trajectory_.GetNumR3Knots())   # knots inside the gap are not in the problem
    assert sg["num_iterations"] == sc["num_iterations"] and sg["inner_sweeps"] == sc["inner_sweeps"] >= 1, ([i["cost"] for i in ig], [i["cost"] for i in ic])
    for a, b in zip(ig, ic):
        assert a["step_is_successful"] == b["step_is_successful"] and abs(a["cost"] - b["cost"]) <= 1e-7 * b["cost"], (a, b)
    assert np.abs(gpu.trajectory_.GetT_i_c() - cpu.trajectory_.GetT_i_c()).max() < 1e-6


def test_both_builds_of_the_inner_kernel_give_the_same_sweeps():
    """Sets that hold nothing but R^3 knots run on the 8-wave build of inner_set_kernel (forward pass only, all items of a knot in
    one round); option debug_inner_general_kernel sends them through the general 4-wave build: same iterates (the per-wave partial
    sums are grouped differently: 1e-9)."""
    ds = synthetic.make_config("C2")
    out = []
    for general in (0, 1):
        c = E.ImuCameraCalibrator().BatchInitSpline(ds)
        c.trajectory_.SetOption("inner_iterations", 1); c.trajectory_.SetOption("debug_inner_general_kernel", general)
        s_ = c.trajectory_.Optimize(50, FLAGS1)
        out.append((s_, c.trajectory_.GetIterations(), c.trajectory_.GetT_i_c()))
    (s0, i0, t0), (s1, i1, t1) = out
    assert s0["num_iterations"] == s1["num_iterations"] and s0["inner_sweeps"] == s1["inner_sweeps"] >= 1 and s0["inner_lm_iterations"] == s1["inner_lm_iterations"]
    assert all(a["step_is_successful"] == b["step_is_successful"] and abs(a["cost"] - b["cost"]) <= 1e-9 * b["cost"] for a, b in zip(i0, i1))
    assert np.abs(t0 - t1).max() < 1e-8


@pytest.mark.parametrize("cfg,flags", [("tiny", FLAGS1), ("C2", FLAGS1), ("C2", FLAGS1 | E.IMU_BIASES), ("C3", FLAGS1), ("C4", FLAGS1)])
def test_one_wave_per_block_gives_the_sweeps_of_one_workgroup_per_block(cfg, flags):
    """Round 5: large sets of knot blocks (>= 4 x compute units: BASELINE config 5) are minimised with ONE WAVE per block
    (inner_wave_kernel: a workgroup is one wave, items read as per-item records in rounds of 64, no workgroup
    barrier) instead of one workgroup per block.  Option inner_wave_blocks = 1 sends every eligible set of the smaller configurations
    through it: the sweeps of the workgroup kernel (= 2: never), hence of the oracle -- same outer iterates, sweep counts, per-block LM
    iteration totals, extrinsics; with the bias knots free (shared blocks stay on the workgroup kernel), on C3 / C4
    (R^3 knots with up to 17 views per window), and against the oracle on tiny and C2."""
    ds = synthetic.make_config(cfg)
    out = []
    for mode in (1, 2):
        c = E.ImuCameraCalibrator().BatchInitSpline(ds)
        c.trajectory_.UseReferenceSolverOptions(); c.trajectory_.SetOption("inner_wave_blocks", mode)
        s_ = c.trajectory_.Optimize(50, flags)
        out.append((s_, c.trajectory_.GetIterations(), c.trajectory_.GetT_i_c(), c.trajectory_.GetKnots()))
    (s0, i0, t0, k0), (s1, i1, t1, k1) = out
    assert s0["num_iterations"] == s1["num_iterations"] and s0["inner_sweeps"] == s1["inner_sweeps"] >= 1, (s0, s1)
    assert abs(s0["inner_lm_iterations"] - s1["inner_lm_iterations"]) <= 0.002 * s1["inner_lm_iterations"] + 1, (s0["inner_lm_iterations"], s1["inner_lm_iterations"])
    assert all(a["step_is_successful"] == b["step_is_successful"] and abs(a["cost"] - b["cost"]) <= 1e-9 * b["cost"] for a, b in zip(i0, i1)), (i0, i1)
    assert np.abs(t0 - t1).max() < 1e-8 and np.abs(k0[0][:-1] - k1[0][:-1]).max() < 1e-7 and np.abs(k0[0][-1] - k1[0][-1]).max() < 1e-5 and (np.abs(k0[1] - k1[1]) <= 1e-7 * (1 + np.abs(k1[1]))).all()   # (the last knots, past the last view, are held by a few IMU samples only)
    if cfg in ("tiny", "C2") and flags == FLAGS1:
        cpu = E.ImuCameraCalibrator(backend=oracle_backend.load()).BatchInitSpline(ds)
        cpu.trajectory_.UseReferenceSolverOptions()
        sc = cpu.trajectory_.Optimize(50, flags)
        assert sc["num_iterations"] == s0["num_iterations"] and sc["inner_sweeps"] == s0["inner_sweeps"]
        for a, b in zip(i0, cpu.trajectory_.GetIterations()):
            assert a["step_is_successful"] == b["step_is_successful"] and abs(a["cost"] - b["cost"]) <= 1e-7 * b["cost"], (a, b)
        assert np.abs(t0 - cpu.trajectory_.GetT_i_c()).max() < 1e-6


@pytest.mark.parametrize("cfg,flags", [("tiny", FLAGS1), ("tiny", FLAGS1 | E.IMU_BIASES | E.IMU_INTRINSICS), ("C2", FLAGS1), ("C2", FLAGS1 | E.IMU_INTRINSICS), ("C3", FLAGS1)])
def test_shared_blocks_by_a_sequence_of_launches_give_the_sweeps_of_resident_workgroups(cfg, flags):
    """Round 5: a block every view / sample depends on (T_i_c, gravity, IMU intrinsics, bias knots) above a size threshold
    (option inner_shared_launch_slots, default 65536 item slots: BASELINE config 5) is minimised by a SEQUENCE OF LAUNCHES over the
    whole device -- inner_shared_eval_kernel leaves one row of partial sums per part, inner_shared_advance_kernel adds the rows in
    order and advances the loop, whose state lives in global memory -- instead of resident workgroups that wait for each other.
    Threshold 1 sends every shared block of the smaller configurations through it: the sweeps of the resident workgroups (0: never),
    hence of the oracle -- same outer iterates, sweep counts, per-block LM iteration totals, extrinsics."""
    ds = synthetic.make_config(cfg)
    out = []
    for slots in (1, 0):
        c = E.ImuCameraCalibrator().BatchInitSpline(ds)
        c.trajectory_.UseReferenceSolverOptions(); c.trajectory_.SetOption("inner_shared_launch_slots", slots)
        s_ = c.trajectory_.Optimize(50, flags)
        out.append((s_, c.trajectory_.GetIterations(), c.trajectory_.GetT_i_c(), c.trajectory_.GetKnots()))
    (s0, i0, t0, k0), (s1, i1, t1, k1) = out
    assert s0["num_iterations"] == s1["num_iterations"] and s0["inner_sweeps"] == s1["inner_sweeps"] >= 1, (s0, s1)
    assert abs(s0["inner_lm_iterations"] - s1["inner_lm_iterations"]) <= 0.002 * s1["inner_lm_iterations"] + 1, (s0["inner_lm_iterations"], s1["inner_lm_iterations"])
    assert all(a["step_is_successful"] == b["step_is_successful"] and abs(a["cost"] - b["cost"]) <= 1e-9 * b["cost"] for a, b in zip(i0, i1)), (i0, i1)
    assert np.abs(t0 - t1).max() < 1e-8 and np.abs(k0[0][:-1] - k1[0][:-1]).max() < 1e-7 and np.abs(k0[0][-1] - k1[0][-1]).max() < 1e-5 and (np.abs(k0[1] - k1[1]) <= 1e-7 * (1 + np.abs(k1[1]))).all()   # (relative: the last R^3 knots, held by a few accelerometer samples only, run away to 1e4 and more)
    if cfg == "tiny":
        cpu = E.ImuCameraCalibrator(backend=oracle_backend.load()).BatchInitSpline(ds)
        cpu.trajectory_.UseReferenceSolverOptions()
        sc = cpu.trajectory_.Optimize(50, flags)
        assert sc["num_iterations"] == s0["num_iterations"] and sc["inner_sweeps"] == s0["inner_sweeps"]
        for a, b in zip(i0, cpu.trajectory_.GetIterations()):
            assert a["step_is_successful"] == b["step_is_successful"] and abs(a["cost"] - b["cost"]) <= 1e-7 * b["cost"], (a, b)
        assert np.abs(t0 - cpu.trajectory_.GetT_i_c()).max() < 1e-6


# ---- Ceres' bounds line search (box-bounded bias knots, impl.h:206-240): host-driven Armijo search of oicc_optimize ----
@pytest.mark.parametrize("cfg,flags,inner", [("C1", FLAGS1 | E.ACC_BIAS, 0), ("C1", FLAGS1 | E.ACC_BIAS, 1), ("tiny", FLAGS1 | E.IMU_BIASES, 1)])
def test_bounds_line_search_matches_the_oracle(cfg, flags, inner):
    """With bias knots among the variables Ceres runs an Armijo search along the projected path (cubic interpolation on value
    and slope samples) before it judges the candidate; a step that plain LM would reject is shortened instead.  Same iterate
    sequence as oracle/oicc_oracle.cpp with the option on, and a different one than without it."""
    ds = synthetic.make_config(cfg)
    gpu = E.ImuCameraCalibrator().BatchInitSpline(ds)
    cpu = E.ImuCameraCalibrator(backend=oracle_backend.load()).BatchInitSpline(ds)
    for c in (gpu, cpu):
        c.trajectory_.SetOption("inner_iterations", inner); c.trajectory_.SetOption("bounds_line_search", 1)
    cpu.trajectory_.SetOption("analytic_jacobians", 0)   # Jets on the checker's side
    sg = gpu.trajectory_.Optimize(50, flags); sc = cpu.trajectory_.Optimize(50, flags)
    ig, ic = gpu.trajectory_.GetIterations(), cpu.trajectory_.GetIterations()
    assert sg["num_iterations"] == sc["num_iterations"], ([i["cost"] for i in ig], [i["cost"] for i in ic])
    for a, b in zip(ig, ic):
        assert a["step_is_successful"] == b["step_is_successful"] and abs(a["cost"] - b["cost"]) <= 1e-7 * b["cost"], (a, b)
    assert np.abs(gpu.trajectory_.GetT_i_c() - cpu.trajectory_.GetT_i_c()).max() < 1e-6
    plain = E.ImuCameraCalibrator().BatchInitSpline(ds)
    plain.trajectory_.SetOption("inner_iterations", inner)
    sp = plain.trajectory_.Optimize(50, flags)
    assert sp["num_iterations"] != sg["num_iterations"] or abs(sp["final_cost"] - sg["final_cost"]) > 1e-9 * sg["final_cost"]


def test_projected_gradient_norm_of_the_bounded_problem_matches_the_oracle():
    """With bias knots among the variables the program is bounds constrained and Ceres reports (and tests against its gradient
    tolerance) the max norm of Plus(x, -g) - x in the ambient space instead of max |g|: a quaternion block contributes at most 2,
    a bias entry at most its distance to the bound.  Same numbers from the device kernel and the oracle, different from max |g|."""
    ds = synthetic.make_config("tiny")
    flags = FLAGS1 | E.IMU_BIASES
    gpu = E.ImuCameraCalibrator().BatchInitSpline(ds); cpu = E.ImuCameraCalibrator(backend=oracle_backend.load()).BatchInitSpline(ds)
    plain = E.ImuCameraCalibrator().BatchInitSpline(ds)
    for c in (gpu, cpu):
        c.trajectory_.SetOption("projected_gradient_norm", 1)
    sg = gpu.trajectory_.Optimize(6, flags); sc = cpu.trajectory_.Optimize(6, flags); plain.trajectory_.Optimize(6, flags)
    ig, ic, ip = gpu.trajectory_.GetIterations(), cpu.trajectory_.GetIterations(), plain.trajectory_.GetIterations()
    assert len(ig) == len(ic) == len(ip) >= 4
    for a, b, c in zip(ig, ic, ip):
        assert abs(a["cost"] - b["cost"]) <= 1e-8 * b["cost"] and abs(a["cost"] - c["cost"]) <= 1e-10 * c["cost"]   # the iterates do not depend on it
        assert abs(a["gradient_max_norm"] - b["gradient_max_norm"]) <= 1e-6 * b["gradient_max_norm"], (a, b)
    assert ig[0]["gradient_max_norm"] < 0.5 * ip[0]["gradient_max_norm"]


# ---- two processes, one GPU: the product's all-reduce hook inside oicc_optimize ---------------------------------------------
@pytest.mark.parametrize("cfg,flags,ls,inner,owner", [("C1", FLAGS1, 0, 0, 0), ("tiny", FLAGS1 | E.ACC_BIAS, 1, 0, 0), ("C1", FLAGS1, 0, 1, 0), ("tiny", FLAGS1 | E.IMU_BIASES, 1, 1, 0),
                                                     ("C1", FLAGS1, 0, 0, 1), ("C2", FLAGS1, 0, 0, 1), ("tiny", FLAGS1 | E.IMU_BIASES, 1, 1, 1), ("C1", FLAGS1, 0, 1, 1),
                                                     ("C1", FLAGS1 | E.POINTS, 0, 0, 0), ("C1", FLAGS1 | E.POINTS, 0, 0, 1), ("tiny", FLAGS1 | E.POINTS, 0, 1, 1)])   # (the last: board points under owner-computes sweeps -- replicated blocks behind the IMU intrinsics, broadcast from rank 0: advisor, round 5)   # (C1 with the line delay free is chaotic from run to run within ONE process: not a test case)
def test_two_processes_on_one_gpu_reduce_through_the_hook(cfg, flags, ls, inner, owner, tmp_path):
    """Two time shards in two processes on one GPU take the steps of one process (see _sharded_processes_take_the_steps_of_one)."""
    _sharded_processes_take_the_steps_of_one(cfg, flags, ls, inner, owner, tmp_path, 2)


@pytest.mark.parametrize("cfg,flags,owner,nproc,inner", [("C2", FLAGS1, 1, 4, 0), ("C1", FLAGS1, 0, 4, 0), ("C1", FLAGS1 | E.POINTS, 1, 4, 0), ("C2", FLAGS1, 1, 8, 0), ("C2", FLAGS1, 1, 4, 1)])
def test_four_and_eight_processes_on_one_gpu_with_owned_ranges_in_the_middle(cfg, flags, owner, nproc, inner, tmp_path):
    """Four / eight time shards: the ranks in the middle own a range with a neighbour on either side (two cuts, halo rows to and from
    both, a gather from every owner) -- the geometry of every rank but the first and last of an 8-GPU run, which two shards never
    produce."""
    _sharded_processes_take_the_steps_of_one(cfg, flags, 0, inner, owner, tmp_path, nproc)


def test_owner_computes_sweeps_with_the_shared_blocks_as_a_sequence_of_launches(tmp_path, monkeypatch):
    """Round 5: on sharded ranks with owner-computes sweeps the blocks every view / sample depends on are replicated -- every rank
    minimises them, rank 0's count of LM iterations is the one that is reported, the non-knot tail of the parameter vector is
    broadcast from rank 0 after the set.  With the threshold at 1 slot those blocks take the sequence-of-launches path
    (inner_shared_eval_kernel / inner_shared_advance_kernel) on every rank: two processes still take the steps of one."""
    monkeypatch.setenv("OICC_TEST_SHARED_LAUNCH_SLOTS", "1")
    _sharded_processes_take_the_steps_of_one("C1", FLAGS1, 0, 1, 1, tmp_path, 2)


@pytest.mark.parametrize("cfg,nproc,iters", [("C1", 2, 6), ("C1", 4, 6), ("C2", 2, 6), ("C2", 4, 6), ("C2", 8, 6), ("C3", 4, 4), ("C5", 2, 1), ("C5", 4, 1)])
def test_distributed_cyclic_reduction_takes_the_steps_of_one_process(cfg, nproc, iters, tmp_path):
    """Round 6, SURVEY 8(e) "v2 ... Solve": with the owner-computes exchange agreed on, every rank eliminates the 64-column blocks of
    ITS band range (kernels_bcr.hip: launch_bcr_dist_*; the last pivots of a range have the next rank's first block as a ghost
    neighbour), the ranks' separator blocks (+ ghost blocks, final couplings, corner parts: 0.11 MB per rank) are gathered, every rank
    solves the N-block top system, back-substitutes its own range, and the step is gathered -- the band itself is NEVER gathered:
    besides its own rows a rank only receives the halo rows of its own range, two doubles per foreign row (diagonal, gradient) and
    the solution.  2 / 4 / 8 processes on one GPU through the transport hooks take the steps of ONE process (costs 1e-8, T_i_c 1e-7);
    every solve of every rank ran distributed; no broadcast as large as a rank's band range happened; and with distributed_solve = 0
    the same shards fall back to the gathered band (the larger messages come back)."""
    parts, whole = _sharded_processes_take_the_steps_of_one(cfg, FLAGS1, 0, 0, 1, tmp_path, nproc, iters=iters)
    nit = len(whole["iterations"])
    assert all(p_["dist_ranks"] == nproc and p_["dist_solves"] >= nit - 1 and p_["dist_blocks"] >= 1 for p_ in parts), [(p_["dist_ranks"], p_["dist_solves"], p_["dist_blocks"]) for p_ in parts]
    # every rank retracts the same gathered step: no candidate is broadcast (only the step's scalars travel), and the ranks end BIT-identical
    assert all(p_["T_i_c"] == parts[0]["T_i_c"] and p_["final_cost"] == parts[0]["final_cost"] for p_ in parts[1:])
    assert sum(p_["dist_blocks"] for p_ in parts) == (whole["band_dim"] + 63) // 64 and [p_["dist_first_block"] for p_ in parts] == sorted(p_["dist_first_block"] for p_ in parts)
    # the largest message any rank received: one of the three gathers (top-system slot, solution slot, diagonal + gradient), never a band range
    a1 = parts[0]["P"] - whole["band_dim"] + 1
    most = max(p_["dist_blocks"] for p_ in parts)
    limit = max(3 * 4096 + 128 * a1 + a1 * a1 + 8, 64 * most + a1 + 8, 2 * 64 * most)
    assert all(p_["exchange"]["max_broadcast"] <= limit for p_ in parts), ([p_["exchange"]["max_broadcast"] for p_ in parts], limit)
    rows = whole["band_dim"] // nproc
    if cfg not in ("C1",) and not (cfg == "C2" and nproc == 8):   # (C1, and C2 on eight ranks -- 228 rows each: a rank's band range is no larger than a top-system slot)
        assert limit < 0.5 * rows * parts[0]["band_row_doubles"]      # (... which would be this large)
    if cfg == "C2" and nproc == 2:
        import os
        os.environ["OICC_TEST_DISTRIBUTED_SOLVE"] = "0"
        try:
            parts0, _ = _sharded_processes_take_the_steps_of_one(cfg, FLAGS1, 0, 0, 1, tmp_path, nproc, iters=iters)
        finally:
            del os.environ["OICC_TEST_DISTRIBUTED_SOLVE"]
        assert all(p_["dist_solves"] == 0 and p_["exchange"]["max_broadcast"] > 0.5 * rows * p_["band_row_doubles"] > limit for p_ in parts0)


@pytest.mark.parametrize("extra", [0, E.IMU_INTRINSICS])
def test_distributed_cyclic_reduction_through_rejected_steps(tmp_path, monkeypatch, extra):
    """The tiny problem with the bias knots free, on two ranks, from a trust-region radius of 1e9 (the case of
    test_device_side_lm_control_takes_the_steps_of_the_host_loop: iterations 2-5 and 11 are REJECTED): the distributed solve runs with
    reused diagonals and shrinking radii (every rank rebuilds its blocks from the kept diagonal) and a wider arrow (bias knots) --
    the same accept / reject sequence and costs as one process."""
    monkeypatch.setenv("OICC_TEST_RADIUS", "1e9")
    parts, whole = _sharded_processes_take_the_steps_of_one("tiny", FLAGS1 | E.IMU_BIASES | extra, 0, 0, 1, tmp_path, 2, iters=12)   # (with the IMU intrinsics: 31 border rows, two arrow strips)
    assert whole["rejected"] >= (3 if extra == 0 else 0) and all(p_["rejected"] == whole["rejected"] and p_["dist_ranks"] == 2 and p_["dist_solves"] >= 12 for p_ in parts), (whole["rejected"], [(p_["rejected"], p_["dist_ranks"], p_["dist_solves"]) for p_ in parts])


def test_more_ranks_than_blocks_fall_back_to_the_gathered_band(tmp_path):
    """Degenerate sharding: C1 (five 64-column blocks) on EIGHT time shards -- the cuts, rounded to block boundaries, leave ranks that
    own no block, so the distributed solve does not apply: every rank gathers the band (owned ranges of zero rows included) and solves
    the whole system, and the eight ranks still take the steps of one."""
    parts, whole = _sharded_processes_take_the_steps_of_one("C1", FLAGS1, 0, 0, 1, tmp_path, 8)
    assert all(p_["dist_ranks"] == 0 and p_["dist_solves"] == 0 for p_ in parts)


MAX_WORKER_PROCESSES = 4     # (with this test process: no more than five processes have the GPU open at once)


def _sharded_processes_take_the_steps_of_one(cfg, flags, ls, inner, owner, tmp_path, nproc, iters=6, exchange_agreed=True):
    """Rank r of `nproc` ranks holds the r-th time shard (remote measurements declared) and runs `oicc_optimize` with the
    all-reduce hook (`oicc_set_allreduce`): packed normal equations after every Jacobian pass, the candidate cost (accumulated in
    LmState) after every cost pass, slopes of the bounds line search.  RCCL refuses two ranks on one device, so the hook stages
    through host memory and gloo -- the product side of the hook is what is tested.  Both ranks must take the same steps as ONE
    process holding the whole problem.
    owner = 1 (round 4): the owner-computes exchange instead of the all-reduce of the whole buffer -- every band row has one owning
    rank; the ranks send the partial rows they hold of the other's range (oicc_set_exchange: send / receive), gather the owned
    ranges (broadcast per owner) and all-reduce only the arrow corner, the arrow gradient and the cost: the whole buffer is never
    summed, the steps are those of ONE process.
    Every rank runs in a process of its own up to MAX_WORKER_PROCESSES ranks; with more, each worker process hosts several ranks, one
    thread, problem, stream and gloo group per rank (tests/mp_shard_worker.py).
    exchange_agreed = False: the ranks are set up so that they must NOT agree on the owner-computes exchange -- every rank falls
    back to the all-reduce of the whole packed buffer, as without owner."""
    import os, subprocess, sys as _sys, json as _json, socket
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mp_shard_worker.py")

    def run(world):
        # at most MAX_WORKER_PROCESSES processes hold the GPU besides this one: more ranks share a process (a thread per rank)
        nprocs = min(world, MAX_WORKER_PROCESSES)
        procs, outs = [], [str(tmp_path / ("w%d_r%d.json" % (world, r))) for r in range(world)]
        sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()   # (a port found free for THIS run: port + world was never checked)
        for k in range(nprocs):
            ranks = ",".join(str(r) for r in range(world) if r % nprocs == k)
            env = dict(os.environ, RANKS=ranks, WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK="0")
            out = str(tmp_path / ("w%d_r{rank}.json" % world))
            procs.append(subprocess.Popen([_sys.executable, worker, cfg, str(int(flags)), str(iters), str(ls), out, str(inner), str(owner)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
        for p_ in procs:
            o, _ = p_.communicate(timeout=400)
            assert p_.returncode == 0, o.decode()[-2000:]
        return [_json.load(open(o)) for o in outs]

    whole = run(1)[0]
    parts = run(nproc)
    assert sum(p_["blocks"] for p_ in parts) == whole["blocks"] and all(p_["hook_calls"] >= 2 * (len(whole["iterations"]) - 1) for p_ in parts)
    if owner and exchange_agreed:   # halo rows travelled, owned ranges were gathered, and no all-reduce was larger than the arrow corner + a rank-consistency pack
        assert all(p_["exchange"]["sendrecv"] >= len(whole["iterations"]) and p_["exchange"]["broadcast"] >= 2 * len(whole["iterations"]) for p_ in parts)
        if not flags & E.POINTS and (parts[0]["P"] - parts[0]["band_dim"]) ** 2 < 5 * parts[0]["P"]:   # (with the board points -- or bias knots + IMU intrinsics on the tiny problem -- in the arrow the corner alone is as large as the packed buffer)
            assert all(p_["hook_max_doubles"] < 10 * p_["P"] for p_ in parts)       # (the packed buffer is ~50 P doubles: it was never all-reduced)
    else:
        assert all(p_["hook_max_doubles"] > 10 * p_["P"] for p_ in parts)
    if inner:   # the reference's solver configuration on time-sharded ranks: the sweeps run over the whole problem's measurements
        assert whole["inner_sweeps"] >= 1 and all(p_["inner_sweeps"] == whole["inner_sweeps"] for p_ in parts)
        if owner:   # round 5, owner-computes sweeps: a rank minimises only the knot blocks it owns, after every independent set the owners
                    # broadcast what the set changed (>= 2 pieces per set: the replicated tail, a knot range) -- and the ranks' counts of
                    # per-block LM iterations add up to one process's (a block is minimised exactly once per sweep)
            assert all(p_["exchange"]["broadcast"] >= 2 * len(whole["iterations"]) + 10 * whole["inner_sweeps"] for p_ in parts)
            assert all(abs(p_["inner_lm_iterations"] - whole["inner_lm_iterations"]) <= 0.03 * whole["inner_lm_iterations"] + 2 for p_ in parts), (whole["inner_lm_iterations"], [p_["inner_lm_iterations"] for p_ in parts])
    for p_ in parts:
        assert len(p_["iterations"]) == len(whole["iterations"])
        for a, b in zip(p_["iterations"], whole["iterations"]):
            assert a["ok"] == b["ok"] and abs(a["cost"] - b["cost"]) <= (1e-7 if inner else 1e-8) * b["cost"], (a, b)
        assert np.abs(np.array(p_["T_i_c"]) - np.array(whole["T_i_c"])).max() < (1e-6 if inner else 1e-7)
    assert all(np.abs(np.array(parts[0]["T_i_c"]) - np.array(p_["T_i_c"])).max() < 1e-9 for p_ in parts[1:])
    return parts, whole



# ---- SplineOptimFlags::POINTS (impl.h:136-153): the board points as variables ------------------------------------------
POINT_CASES = [("tiny", FLAGS1 | E.POINTS), ("tiny", E.T_I_C | E.POINTS), ("tiny", FLAGS1 | E.CAM_LINE_DELAY | E.IMU_BIASES | E.POINTS),
               ("C1", FLAGS1 | E.POINTS)]


@pytest.mark.parametrize("cfg,flags", POINT_CASES)
def test_points_flag_layout_and_normal_equations(cfg, flags):
    """Tangent layout (the point columns behind every other block, 3 per observed point), cost, gradient and J^T J with the
    board points variable, against the Jet oracle (HomogeneousVectorParameterization::ComputeJacobian behind the ambient
    4-vector columns); the time tiles and the direct-atomics route of the tile pass give the same system."""
    _, gpu, cpu = build_pair(cfg)
    tg, tc = gpu.trajectory_, cpu.trajectory_
    lg, lc = tg.GetTangentLayout(flags), tc.GetTangentLayout(flags)
    assert lg["P"] == lc["P"]
    for k in ("so3", "r3", "accl_bias", "gyro_bias", "other"):
        assert np.array_equal(lg[k], lc[k]), k
    og, oc = tg.GetScenePointOffsets(flags), tc.GetScenePointOffsets(flags)
    assert np.array_equal(og, oc) and (og >= 0).any()
    assert (tg.GetScenePointOffsets(flags & ~E.POINTS) == -1).all()
    cc, Hc, gc = tc.Evaluate(flags)
    for assembly in (0, 2):
        tg.SetOption("assembly", assembly)
        cg, Hg, gg = tg.Evaluate(flags)
        assert abs(cg - cc) <= 1e-11 * cc
        assert rel_err(gg, gc) < 1e-10, (assembly, rel_err(gg, gc))
        assert rel_err(Hg, Hc) < 1e-10, (assembly, rel_err(Hg, Hc))
        p0 = og[og >= 0].min()
        assert rel_err(Hg[p0:, :], Hc[p0:, :]) < 1e-10 and rel_err(gg[p0:], gc[p0:]) < 1e-10      # the point rows on their own scale
        assert np.abs(Hg - Hg.T).max() <= 1e-13 * np.abs(Hg).max()
    tg.SetOption("assembly", 0)
    # the flag off again: the system of the other blocks is what it was (the layout cache keys on the flags)
    c0, H0, g0 = tg.Evaluate(flags & ~E.POINTS)
    c1, H1, g1 = tc.Evaluate(flags & ~E.POINTS)
    assert H0.shape == H1.shape and rel_err(H0, H1) < 1e-10 and rel_err(g0, g1) < 1e-10


def test_points_flag_with_the_bounds_line_search_and_the_projected_gradient_norm():
    """POINTS next to box-bounded bias knots: Ceres' Armijo search along the projected path re-retracts the points with its step
    sizes (HomogeneousVectorParameterization::Plus of alpha * delta) and reports the ambient max norm of Plus(x, -g) - x, points
    included.  Same iterates and gradient norms as the oracle."""
    flags = FLAGS1 | E.IMU_BIASES | E.POINTS
    _, gpu, cpu = build_pair("tiny")
    for c in (gpu, cpu):
        c.trajectory_.SetOption("bounds_line_search", 1); c.trajectory_.SetOption("projected_gradient_norm", 1)
    sg, sc = gpu.trajectory_.Optimize(8, flags), cpu.trajectory_.Optimize(8, flags)
    ig, ic = gpu.trajectory_.GetIterations(), cpu.trajectory_.GetIterations()
    assert sg["num_iterations"] == sc["num_iterations"] and sg["line_search_steps"] == sc["line_search_steps"] >= 1, (sg, sc)
    for a, b in zip(ig, ic):
        assert a["step_is_successful"] == b["step_is_successful"] and abs(a["cost"] - b["cost"]) <= 1e-8 * b["cost"]
        assert abs(a["gradient_max_norm"] - b["gradient_max_norm"]) <= 1e-6 * max(b["gradient_max_norm"], 1e-12), (a, b)
    assert np.abs(gpu.trajectory_.GetScenePoints() - cpu.trajectory_.GetScenePoints()).max() < 1e-7


@pytest.mark.parametrize("cfg,flags", [POINT_CASES[0], POINT_CASES[3]])
def test_points_flag_lm_iterates_and_refined_points(cfg, flags):
    """oicc_optimize with POINTS: the iterates of the oracle's trust-region loop (same accept / reject sequence, costs),
    the refined points (HomogeneousVectorParameterization::Plus keeps |x|), T_i_c and the knots."""
    _, gpu, cpu = build_pair(cfg)
    tg, tc = gpu.trajectory_, cpu.trajectory_
    p0 = tg.GetScenePoints()
    assert np.array_equal(p0, tc.GetScenePoints())
    sg, sc = tg.Optimize(30, flags), tc.Optimize(30, flags)
    ig, ic = tg.GetIterations(), tc.GetIterations()
    assert sg["termination"] == sc["termination"] and sg["num_iterations"] == sc["num_iterations"], (sg, sc)
    assert sg["arrow_dim"] == sc["arrow_dim"] and sg["num_parameters_tangent"] == sc["num_parameters_tangent"]
    for a, b in zip(ig, ic):
        assert a["step_is_successful"] == b["step_is_successful"]
        assert abs(a["cost"] - b["cost"]) <= 1e-8 * b["cost"]
        assert abs(a["step_norm"] - b["step_norm"]) <= 1e-6 * max(b["step_norm"], 1e-12)
    pg, pc = tg.GetScenePoints(), tc.GetScenePoints()
    seen = tg.GetScenePointOffsets(flags) >= 0
    assert np.abs(pg - pc).max() < 1e-7 and np.abs(pg[seen] - p0[seen]).max() > 1e-6
    assert np.allclose(np.linalg.norm(pg, axis=1), np.linalg.norm(p0, axis=1), rtol=1e-12)
    assert np.abs(tg.GetT_i_c() - tc.GetT_i_c()).max() < 1e-7
    kg, kc = tg.GetKnots(), tc.GetKnots()
    assert np.abs(kg[0] - kc[0]).max() < 1e-7 and np.abs(kg[1] - kc[1]).max() < 1e-7
    assert abs(tg.GetMeanReprojectionError() - tc.GetMeanReprojectionError()) < 1e-7
    # a second solve without the flag starts from the refined points on both sides
    s2g, s2c = tg.Optimize(5, flags & ~E.POINTS), tc.Optimize(5, flags & ~E.POINTS)
    assert abs(s2g["initial_cost"] - s2c["initial_cost"]) <= 1e-8 * s2c["initial_cost"]
    assert abs(s2g["initial_cost"] - sg["final_cost"]) <= 1e-8 * sg["final_cost"]


@pytest.mark.parametrize("cfg,flags,iters", [("tiny", FLAGS1 | E.POINTS, 8), ("tiny", FLAGS1 | E.POINTS | E.CAM_LINE_DELAY | E.IMU_BIASES, 5), ("tiny", E.T_I_C | E.POINTS, 6)])
def test_points_flag_with_the_reference_solver_options(cfg, flags, iters):
    """Round 5: SplineOptimFlags::POINTS under the configuration the reference's Optimize always runs with (use_inner_iterations =
    true, impl.h:266; round 4 refused the combination).  A board point is one more parameter block of the sweep: it depends on
    every view that sees it -- a view is ONE residual block over all its corners, so all those corners count in the block's cost
    and the points of a view are neighbours in the Hessian graph (they end up in sets of their own, one point each) -- and moves
    under HomogeneousVectorParameterization::Plus.  Outer iterates, sweep count, per-block LM iterations, refined points, extrinsics
    and knots against the oracle's restatement (ceres_inner.hpp with PB_PT blocks; Jets)."""
    _, gpu, cpu = build_pair(cfg)
    tg, tc = gpu.trajectory_, cpu.trajectory_
    tg.UseReferenceSolverOptions(); tc.UseReferenceSolverOptions()
    p0 = tg.GetScenePoints()
    sg, sc = tg.Optimize(iters, flags), tc.Optimize(iters, flags)
    assert sg["num_iterations"] == sc["num_iterations"] and sg["inner_sweeps"] == sc["inner_sweeps"] >= 1, (sg, sc)
    assert abs(sg["inner_lm_iterations"] - sc["inner_lm_iterations"]) <= 0.02 * sc["inner_lm_iterations"] + 2, (sg["inner_lm_iterations"], sc["inner_lm_iterations"])
    for a, b in zip(tg.GetIterations(), tc.GetIterations()):
        assert a["step_is_successful"] == b["step_is_successful"] and abs(a["cost"] - b["cost"]) <= 1e-7 * b["cost"], (a, b)
    pg, pc = tg.GetScenePoints(), tc.GetScenePoints()
    seen = tg.GetScenePointOffsets(flags) >= 0
    assert np.abs(pg - pc).max() < 1e-6 and np.abs(pg[seen] - p0[seen]).max() > 1e-6
    assert np.allclose(np.linalg.norm(pg, axis=1), np.linalg.norm(p0, axis=1), rtol=1e-12)
    assert np.abs(tg.GetT_i_c() - tc.GetT_i_c()).max() < 1e-6
    kg, kc = tg.GetKnots(), tc.GetKnots()
    assert np.abs(kg[0] - kc[0]).max() < 1e-6 and np.abs(kg[1] - kc[1]).max() < 1e-6


# ---- a sweep over small problems of varied geometry (round 4): knot spacing ratios, IMU rates, view counts, shutters, cameras, flags ----
def _random_cases():
    rng = np.random.RandomState(424242)
    cams = ["pinhole", "pinhole_radtan", "gopro9_division", "gopro6_fisheye", "gopro6_double_sphere", "gopro9_eucm"]
    spacing = [(0.05, 0.1), (0.1, 0.1), (0.04, 0.12), (0.1, 0.05), (0.03, 0.09), (0.07, 0.11)]
    flag_sets = [FLAGS1, FLAGS1 | E.CAM_LINE_DELAY, FLAGS1 | E.IMU_BIASES, FLAGS1 | E.IMU_INTRINSICS | E.ACC_BIAS, E.T_I_C | E.GRAVITY_DIR,
                 FLAGS1 | E.POINTS, E.SPLINE, FLAGS1 | E.GYR_BIAS | E.CAM_LINE_DELAY | E.POINTS]
    cases = []
    for k in range(12):
        dt_so3, dt_r3 = spacing[k % len(spacing)]
        cases.append(dict(num_views=int(rng.randint(6, 40)), corners_per_view=int(rng.randint(4, 20)), duration=float(rng.uniform(0.9, 3.5)),
                          camera=cams[k % len(cams)], imu_rate=float(rng.choice([100.0, 200.0, 400.0])), dt_so3=dt_so3, dt_r3=dt_r3,
                          rolling_shutter=bool(k % 4 != 3), seed=1000 + k, flags=flag_sets[k % len(flag_sets)]))
    return cases


@pytest.mark.parametrize("case", _random_cases(), ids=lambda c: "seed%d" % c["seed"])
def test_small_problems_of_varied_geometry_match_the_oracle(case):
    """Twelve seeded small problems -- knot spacing ratios from 1:3 to 2:1, IMU rates 100-400 Hz, 6-40 views of 4-20 corners, rolling and
    global shutter, six camera models, eight flag sets (POINTS among them): tangent layout, cost, gradient and J^T J against the Jet
    oracle through the time tiles and through the direct-atomics route, and the first LM iterates."""
    kw = dict(case); flags = kw.pop("flags")
    _, gpu, cpu = build_pair("tiny", board=(6, 5), **kw)
    tg, tc = gpu.trajectory_, cpu.trajectory_
    lg, lc = tg.GetTangentLayout(flags), tc.GetTangentLayout(flags)
    assert lg["P"] == lc["P"]
    for k in ("so3", "r3", "accl_bias", "gyro_bias", "other"):
        assert np.array_equal(lg[k], lc[k]), k
    cc, Hc, gc = tc.Evaluate(flags)
    for assembly in (0, 2):
        tg.SetOption("assembly", assembly)
        cg, Hg, gg = tg.Evaluate(flags)
        assert abs(cg - cc) <= 1e-11 * max(cc, 1e-300), (assembly, cg, cc)
        assert rel_err(gg, gc) < 1e-10 and rel_err(Hg, Hc) < 1e-10, (assembly, rel_err(gg, gc), rel_err(Hg, Hc))
    tg.SetOption("assembly", 0)
    sg, sc = tg.Optimize(4, flags), tc.Optimize(4, flags)
    ig, ic = tg.GetIterations(), tc.GetIterations()
    assert len(ig) == len(ic)
    for a, b in zip(ig, ic):
        assert a["step_is_successful"] == b["step_is_successful"] and abs(a["cost"] - b["cost"]) <= 1e-7 * max(b["cost"], 1e-300), (a, b)


@pytest.mark.parametrize("k,flags", [(3, FLAGS1), (5, FLAGS1 | E.CAM_LINE_DELAY), (9, FLAGS1 | E.IMU_BIASES), (10, FLAGS1)])
def test_reference_solver_options_on_small_problems_of_varied_geometry(k, flags):
    """The reference's solver configuration (inner iterations, bounds line search, projected gradient norm) on four of the seeded small
    problems above -- knot spacings 2:1 and 1:3, 100-400 Hz -- against the Jet oracle: the inner-iteration plan (blocks, independent sets,
    the items of every block) on geometries the BASELINE configurations do not have."""
    kw = dict(_random_cases()[k]); kw.pop("flags")
    ds = synthetic.make_config("tiny", board=(6, 5), **kw)
    gpu = E.ImuCameraCalibrator().BatchInitSpline(ds)
    cpu = E.ImuCameraCalibrator(backend=oracle_backend.load()).BatchInitSpline(ds)
    for c in (gpu, cpu):
        c.trajectory_.UseReferenceSolverOptions()
    sg, sc = gpu.trajectory_.Optimize(6, flags), cpu.trajectory_.Optimize(6, flags)
    ig, ic = gpu.trajectory_.GetIterations(), cpu.trajectory_.GetIterations()
    assert len(ig) == len(ic) and sg["inner_sweeps"] == sc["inner_sweeps"] >= 1, (sg, sc)
    for a, b in zip(ig, ic):
        assert a["step_is_successful"] == b["step_is_successful"] and abs(a["cost"] - b["cost"]) <= 1e-7 * max(b["cost"], 1e-300), (a, b)
    assert np.abs(gpu.trajectory_.GetT_i_c() - cpu.trajectory_.GetT_i_c()).max() < 1e-6


@pytest.mark.parametrize("cfg,radius,iters,flags", [("tiny", 1e4, 50, FLAGS1), ("C2", 1e4, 50, FLAGS1), ("C3", 1e9, 50, FLAGS1), ("C2", 1e4, 2, FLAGS1), ("tiny", 1e-30, 50, FLAGS1),
                                                    ("tiny", 1e9, 12, FLAGS1 | E.IMU_BIASES)])
def test_device_side_lm_control_takes_the_steps_of_the_host_loop(cfg, radius, iters, flags):
    """Round 5: plain LM takes its trust-region decisions on the device (LmCtl / lm_decide_kernel; option device_lm, default on) and
    evaluates a candidate with ONE Jacobian pass (cost + gradient + normal equations) instead of a cost pass followed by a Jacobian
    pass.  Same accept / reject sequence, termination, iteration records and final parameters as the host-driven loop (the
    candidate's cost is summed in another order: 1e-12), stage 1 and stage 2, with rejected steps and reused diagonals (the bias
    knots free from a radius of 1e9: iterations 2-5 and 11 are rejected with rho between -15 and -0.08, far from the threshold),
    an iteration limit inside the run, and a tiny start radius."""
    ds = synthetic.make_config(cfg)
    runs = []
    for dev in (1, 0):
        tr = E.ImuCameraCalibrator().BatchInitSpline(ds).trajectory_
        tr.SetOption("device_lm", dev); tr.SetOption("initial_trust_region_radius", radius)
        s1 = tr.Optimize(iters, flags); it1 = tr.GetIterations()
        s2 = tr.Optimize(10, E.CAM_LINE_DELAY); it2 = tr.GetIterations()
        runs.append((s1, it1, s2, it2, tr.GetT_i_c(), tr.GetKnots(), tr.GetRSLineDelay(), tr.GetGravity()))
    d, h = runs
    for k in (0, 2):
        for key in ("termination", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "message"):
            assert d[k][key] == h[k][key], (k, key, d[k], h[k])
        assert abs(d[k]["final_cost"] - h[k]["final_cost"]) <= 1e-12 * h[k]["initial_cost"] + 1e-11 * h[k]["final_cost"]
        assert abs(d[k]["final_radius"] - h[k]["final_radius"]) <= 1e-6 * h[k]["final_radius"]
    for k in (1, 3):
        assert len(d[k]) == len(h[k])
        for a, b in zip(d[k], h[k]):
            assert a["iteration"] == b["iteration"] and a["step_is_successful"] == b["step_is_successful"], (a, b)
            assert abs(a["cost"] - b["cost"]) <= 1e-12 * h[1][0]["cost"] + 1e-11 * b["cost"], (a, b)   # (the two solves differ in the last bits of the step: relative to the cost the step started from)
            assert abs(a["step_norm"] - b["step_norm"]) <= 1e-7 * max(b["step_norm"], 1e-12), (a, b)
            assert abs(a["gradient_max_norm"] - b["gradient_max_norm"]) <= 1e-7 * max(b["gradient_max_norm"], 1e-9), (a, b)
            assert abs(a["trust_region_radius"] - b["trust_region_radius"]) <= 1e-6 * b["trust_region_radius"], (a, b)
    assert np.abs(d[4] - h[4]).max() < 1e-9 and np.abs(d[7] - h[7]).max() < 1e-8
    assert np.abs(d[5][0] - h[5][0]).max() < 1e-9 and np.abs(d[5][1] - h[5][1]).max() < 1e-9
    assert abs(d[6] - h[6]) < 1e-12
    if flags & E.IMU_BIASES:
        assert d[0]["num_unsuccessful_steps"] >= 4 and d[0]["num_successful_steps"] >= 5


def test_c5_sampled_normal_equations_and_first_lm_iterate_match_the_jet_oracle():
    """BASELINE config 5 at full size (P ~ 90 k: the dense matrix does not fit) beyond cost and gradient: 30 000 sampled entries of
    J^T J -- band (every offset up to the half bandwidth), arrow rows, the arrow corner -- through oicc_evaluate_entries against
    the oracle's forward-mode Jets, each to 1e-9 of sqrt(H_ii H_jj); and the first Levenberg-Marquardt iterate of the chained tile
    pass + 12-level cyclic reduction against the oracle's band Cholesky: candidate cost 1e-9, step norm and rho 1e-6, the radius
    update, the gradient norm at the accepted point."""
    ds = synthetic.make_config("C5")
    gpu = E.ImuCameraCalibrator().BatchInitSpline(ds)
    cpu = E.ImuCameraCalibrator(backend=oracle_backend.load()).BatchInitSpline(ds)
    lay = gpu.trajectory_.GetTangentLayout(FLAGS1)
    P = lay["P"]; Pb = 3 * int((lay["so3"] >= 0).sum() + (lay["r3"] >= 0).sum()); a = P - Pb
    hb = gpu.trajectory_.Optimize(0, FLAGS1)["half_bandwidth"]
    assert Pb > 85000 and a == 9 and 40 <= hb <= 64
    rng = np.random.default_rng(7)
    nb = 24000
    i = rng.integers(0, Pb, nb); k = rng.integers(0, hb + 1, nb); j = np.minimum(i + k, Pb - 1)
    ia = rng.integers(0, Pb, 5000); ja = Pb + rng.integers(0, a, 5000)
    ic, jc = np.divmod(np.arange(a * a), a)
    rows = np.concatenate([i, ia, Pb + ic, np.arange(0, Pb, 97)]); cols = np.concatenate([j, ja, Pb + jc, np.arange(0, Pb, 97)])
    vg = gpu.trajectory_.EvaluateEntries(FLAGS1, rows, cols)
    vc = cpu.trajectory_.EvaluateEntries(FLAGS1, rows, cols)
    dg = gpu.trajectory_.EvaluateEntries(FLAGS1, np.concatenate([rows, cols]), np.concatenate([rows, cols]))     # the diagonal entries of the sampled rows and columns
    scale = np.sqrt(np.abs(dg[:len(rows)] * dg[len(rows):])) + 1e-30
    assert np.count_nonzero(vc) > 0.6 * len(vc)          # (inside the band a third of the offsets couple SO(3) / R^3 knots that share no window)
    err = np.abs(vg - vc) / scale
    assert err.max() < 1e-10, (err.max(), rows[err.argmax()], cols[err.argmax()])
    sg = gpu.trajectory_.Optimize(1, FLAGS1); sc = cpu.trajectory_.Optimize(1, FLAGS1)
    ig, ic_ = gpu.trajectory_.GetIterations(), cpu.trajectory_.GetIterations()
    assert len(ig) == len(ic_) == 2 and ig[1]["step_is_successful"] == ic_[1]["step_is_successful"] == 1
    assert abs(ig[1]["cost"] - ic_[1]["cost"]) <= 1e-9 * ic_[1]["cost"], (ig[1], ic_[1])
    assert abs(ig[1]["step_norm"] - ic_[1]["step_norm"]) <= 1e-6 * ic_[1]["step_norm"], (ig[1], ic_[1])
    assert abs(ig[1]["relative_decrease"] - ic_[1]["relative_decrease"]) <= 1e-6, (ig[1], ic_[1])
    assert abs(ig[1]["trust_region_radius"] - ic_[1]["trust_region_radius"]) <= 1e-5 * ic_[1]["trust_region_radius"]
    assert abs(ig[1]["gradient_max_norm"] - ic_[1]["gradient_max_norm"]) <= 1e-6 * ic_[1]["gradient_max_norm"], (ig[1], ic_[1])
    assert sg["termination"] == sc["termination"]


def test_measurements_added_out_of_time_order():
    """Views in the string order of the corner file's keys (what the reference's application produces) and IMU samples reversed:
    the library sorts them (sync_groups) and every result is that of the time-ordered problem -- per-block residuals and Jacobians
    come back in the CALLER's order (oicc_evaluate_blocks), normal equations and the reference-option solve (inner iterations:
    plan, tiles and chains all walk the measurements in time order) against the oracle fed in the same shuffled order."""
    ds = synthetic.make_config("C1")
    d2 = ds.with_view_order(ds.file_key_order())
    d2.imu_t_s = d2.imu_t_s[::-1].copy(); d2.accel = d2.accel[::-1].copy(); d2.gyro = d2.gyro[::-1].copy()
    gpu = E.ImuCameraCalibrator().BatchInitSpline(d2)
    cpu = E.ImuCameraCalibrator(backend=oracle_backend.load()).BatchInitSpline(d2)
    flags = FLAGS1 | E.CAM_LINE_DELAY
    nrows = {0: 2 * gpu.num_corners, 1: 3 * int(gpu.accl_accepted.sum()), 2: 3 * int(gpu.gyro_accepted.sum())}
    for kind in (0, 1, 2):
        rg, Jg = gpu.trajectory_.EvaluateBlocks(flags, kind, nrows[kind]); rc, Jc = cpu.trajectory_.EvaluateBlocks(flags, kind, nrows[kind])
        assert np.abs(rg - rc).max() <= 1e-12 * (1 + np.abs(rc).max()), kind
        scale = np.abs(Jc).max(axis=1, keepdims=True) + 1e-6 * np.abs(Jc).max() + 1e-30
        assert (np.abs(Jg - Jc) / scale).max() < 1e-8, kind
    cg, Hg, gg = gpu.trajectory_.Evaluate(FLAGS1); cc, Hc, gc = cpu.trajectory_.Evaluate(FLAGS1)
    assert abs(cg - cc) <= 1e-11 * cc and rel_err(gg, gc) < 1e-10 and rel_err(Hg, Hc) < 1e-10
    eh, eg = entry_err(gpu.trajectory_, FLAGS1, Hg, Hc, gg, gc, cc)
    assert eh < 1e-10 and eg < 1e-10, (eh, eg)
    # ... and equal to the time-ordered problem's
    ref = E.ImuCameraCalibrator().BatchInitSpline(ds)
    cr, Hr, gr = ref.trajectory_.Evaluate(FLAGS1)
    assert abs(cg - cr) <= 1e-12 * cr and rel_err(Hg, Hr) < 1e-12
    eh, eg = entry_err(gpu.trajectory_, FLAGS1, Hg, Hr, gg, gr, cr)
    assert eh < 1e-12 and eg < 1e-12, (eh, eg)
    for c in (gpu, cpu, ref):
        c.trajectory_.UseReferenceSolverOptions()
    sg = gpu.trajectory_.Optimize(50, FLAGS1); sc = cpu.trajectory_.Optimize(50, FLAGS1); sr = ref.trajectory_.Optimize(50, FLAGS1)
    assert sg["num_iterations"] == sc["num_iterations"] == sr["num_iterations"] and sg["inner_sweeps"] == sc["inner_sweeps"] >= 1
    for a, b in zip(gpu.trajectory_.GetIterations(), cpu.trajectory_.GetIterations()):
        assert a["step_is_successful"] == b["step_is_successful"] and abs(a["cost"] - b["cost"]) <= 1e-7 * b["cost"], (a, b)
    assert np.abs(gpu.trajectory_.GetT_i_c() - cpu.trajectory_.GetT_i_c()).max() < 1e-6
    assert np.abs(gpu.trajectory_.GetT_i_c() - ref.trajectory_.GetT_i_c()).max() < 1e-6
