"""Every route of the damped LM linear solve against an extended-precision host solve of the system Ceres defines.

oicc_debug_lm_step (estimator.DebugLmStep) runs ONE damped solve at the current point and hands back the packed normal equations it
read with the device's scale, clamped diagonal, D2 and step.  tests/lm_step_reference.py rebuilds M = S H S + clamp(h_ii s_i^2) /
radius and rhs = -S g from the packed arrays alone and solves it in float64 with longdouble refinement.  Every case
  - asserts the geometry (Pb, hb, a, n) and the route the library reports, so that no case drifts onto another solver;
  - runs with the LDS poisoned (debug_poison_lds);
  - checks (a) the device's scale and D2 against the host's within 4 ulp -- this holds each of the three copies of the damping
    (lm_build_kernel, bcr_build_body, the fused inversion of level 0) to Ceres' formula; (b) the normwise backward error
    ||M d - rhs||_inf / (||M||_inf ||d||_inf + ||rhs||_inf) of the device step against the HOST-built M, in longdouble; (c) the
    forward error ||d - d*||_inf / ||d*||_inf <= c kappa_1(M) eps.

Geometry notes (the spline layout, oicc_layout.hip):
  - the half bandwidth is 3 c - 1 (c knots in a window), so the edges are taken by the nearest reachable pairs: 56 / 59 (sweep window
    64 -> 128 and partition eligibility), 62 / 65 (the cyclic reduction's hb <= 64);
  - the arrow is 9 (T_i_c, gravity) or 10 (+ line delay) plus multiples of 3, never 2 mod 3: the border-tile edges are taken by
    a = 15 / 16 (one / two 16-row tiles), 31 / 33 (two / three), 46 / 48 (three / four), 63 (four, the bcr_max_border limit);
  - with a = 9 the LDS window of 128 columns no longer fits above hb = 108, so hb 119 runs on the global-memory solver through the
    sweep's LDS check and hb 122 through hb + 8 > 128.
"""
import numpy as np
import pytest

import lm_step_reference as R
from openimucameracalibrator_amd import synthetic, estimator as E

pytestmark = pytest.mark.gpu

F = E.SPLINE | E.T_I_C | E.GRAVITY_DIR
EPS = R.EPS
MIN_DIAG, MAX_DIAG = 1e-6, 1e32          # Ceres' defaults (the library's too)

# Backward-error bounds and forward-error constants c per route, >= 10 x the largest value measured on an MI355X over these cases:
# backward 1.1e-16 (Cholesky routes), 9.0e-15 (cyclic reduction: the one-block band; 1e-15 elsewhere), 1.3e-14 (distributed);
# forward error / (kappa_1 eps) 0.10 (Cholesky), 5.8 (cyclic reduction, the one-block band), 8e-8 (distributed).
BACKWARD = dict(bcr_fused=1e-13, bcr_unfused=1e-13, sweep64=2e-15, sweep128=2e-15, partitioned=2e-15, global_=2e-15, distributed=2e-13)
FORWARD_C = dict(bcr_fused=100.0, bcr_unfused=100.0, sweep64=1.0, sweep128=1.0, partitioned=1.0, global_=1.0, distributed=1.0)


def _key(route):
    return "global_" if route == "global" else route


_DATA = {}


def dataset(duration=1.2, **kw):
    key = (duration, tuple(sorted(kw.items())))
    if key not in _DATA:
        _DATA[key] = synthetic.make_config("tiny", duration=duration, num_views=max(3, int(10 * duration)), **kw)
    return _DATA[key]


def calibrator(ds, **opts):
    cal = E.ImuCameraCalibrator().BatchInitSpline(ds)
    cal.trajectory_.SetOption("debug_poison_lds", 1)
    for k, v in opts.items():
        cal.trajectory_.SetOption(k, v)
    return cal


def check_step(out, radius, min_diag=MIN_DIAG, max_diag=MAX_DIAG, jacobi=True, previous_diag=None, label=""):
    """(a), (b), (c) for one read-out; returns the host diag and the measured numbers."""
    scale, diag, S = R.from_step(out, radius, min_diag, max_diag, jacobi, previous_diag)
    ulp = lambda v: np.spacing(np.abs(v))
    assert np.all(np.abs(out["scale"] - scale) <= 4 * ulp(scale)), (label, "scale")
    assert np.all(np.abs(out["D2"] - S.D2) <= 4 * ulp(S.D2)), (label, "D2", np.abs(out["D2"] - S.D2).max())
    assert not out["chol_failed"], label
    d = out["step_s"]
    assert np.all(np.isfinite(d)), label
    be = S.backward_error(d)
    xs = S.solve()
    kappa = S.cond1()
    fe = np.abs(d - xs).max() / np.abs(xs).max()
    ratio = fe / (kappa * EPS)
    key = _key(out["route"])
    print("MARGIN %-12s %-40s radius %.0e  backward %.3e (bound %.0e)  forward %.3e  kappa1 %.3e  fe/(kappa eps) %.3e"
          % (out["route"], label, radius, be, BACKWARD[key], fe, kappa, ratio))
    assert be <= BACKWARD[key], (label, out["route"], be)
    assert fe <= FORWARD_C[key] * kappa * EPS, (label, out["route"], fe, kappa)
    return diag


def run_case(ds, flags, expect, radii=(1e4, 1e16), nranks=0, **opts):
    cal = calibrator(ds, **opts)
    tr = cal.trajectory_
    geo = tr.DebugLmStep(flags, radii[0], nranks=nranks, solve=False)
    for k, v in expect.items():
        assert geo[k] == v, (k, geo[k], v, geo)
    for radius in radii:
        out = tr.DebugLmStep(flags, radius, nranks=nranks)
        assert all(out[k] == geo[k] for k in ("Pb", "hb", "a", "n", "route", "p"))
        check_step(out, radius, min_diag=opts.get("min_lm_diagonal", MIN_DIAG), max_diag=opts.get("max_lm_diagonal", MAX_DIAG),
                   jacobi=opts.get("jacobi_scaling", 1) != 0, label="%s %s" % (expect, opts))
    return tr


# ---- the block cyclic reduction: border tiles ---------------------------------------------------------------------------------
ARROWS = [   # (a, flags, dataset overrides): tiny, 129 band columns (3 blocks), hb 50
    (15, E.SPLINE | E.T_I_C | E.ACC_BIAS, {}),
    (16, E.SPLINE | E.T_I_C | E.ACC_BIAS | E.CAM_LINE_DELAY, {}),
    (31, E.SPLINE | E.T_I_C | E.CAM_LINE_DELAY | E.IMU_INTRINSICS | E.ACC_BIAS, {}),
    (33, F | E.IMU_INTRINSICS | E.ACC_BIAS, {}),
    (46, F | E.CAM_LINE_DELAY | E.POINTS, dict(board=(4, 3), corners_per_view=12)),
    (48, F | E.IMU_INTRINSICS | E.POINTS, dict(board=(4, 2), corners_per_view=12)),
    (63, F | E.POINTS, dict(board=(6, 3), corners_per_view=18)),
]
# (the board points leave the undamped system singular up to the gauge -- kappa_1 ~ 1e18 at radius 1e16 -- so the cases with POINTS
# solve at Ceres' initial radius only)


@pytest.mark.parametrize("a,flags,kw", ARROWS, ids=["a%d" % c[0] for c in ARROWS])
def test_bcr_border_tiles(a, flags, kw):
    run_case(dataset(**kw), flags, dict(Pb=129, hb=50, a=a, n=3, route="bcr_fused"), radii=(1e4,) if flags & E.POINTS else (1e4, 1e16))


@pytest.mark.parametrize("a,flags,kw,max_border", [
    (64, F | E.CAM_LINE_DELAY | E.POINTS, dict(board=(6, 3), corners_per_view=18), 64),
    (63, F | E.POINTS, dict(board=(6, 3), corners_per_view=18), 48)], ids=["a64", "a63_border48"])
def test_wide_arrow_falls_back_to_the_sweep(a, flags, kw, max_border):
    run_case(dataset(**kw), flags, dict(Pb=129, hb=50, a=a, n=3, route="sweep64"), radii=(1e4,), bcr_max_border=max_border)


def test_large_arrow_goes_to_the_global_solver():
    """POINTS on a 6 x 5 board: 99 arrow columns, the sweep's LDS (and wave) check sends the system to the global-memory solver."""
    run_case(dataset(board=(6, 5), corners_per_view=30), F | E.POINTS, dict(Pb=129, hb=50, a=99, n=3, route="global"), radii=(1e4,), solver_algorithm=1)


# ---- the block cyclic reduction: block counts ---------------------------------------------------------------------------------
BLOCKS = [   # (duration, Pb, n, route): FLAGS, hb 50 (44 on the one-block band)
    (0.3, 48, 1, "bcr_unfused"), (0.75, 90, 2, "bcr_fused"), (1.2, 129, 3, "bcr_fused"), (1.87, 192, 3, "bcr_fused"),
    (2.5, 252, 4, "bcr_fused"), (3.0, 297, 5, "bcr_fused"), (5.0, 477, 8, "bcr_fused"), (6.0, 567, 9, "bcr_fused"),
    (6.15, 576, 9, "bcr_fused"), (11.5, 1062, 17, "bcr_fused"),
]


@pytest.mark.parametrize("duration,Pb,n,route", BLOCKS, ids=["n%d_Pb%d" % (c[2], c[1]) for c in BLOCKS])
def test_bcr_block_counts(duration, Pb, n, route):
    run_case(dataset(duration), F, dict(Pb=Pb, n=n, a=9, route=route))


def test_bcr_unfused_build_above_512_blocks():
    """A 370 s trajectory with few views: 32778 band columns, 513 blocks -- the build runs apart from the inversions of level 0."""
    ds = synthetic.make_config("tiny", duration=370.0, num_views=60)
    run_case(ds, F, dict(Pb=32778, hb=50, a=9, n=513, route="bcr_unfused"))


# ---- half-bandwidth edges -----------------------------------------------------------------------------------------------------
HB = [   # (dt_so3, dt_r3, Pb, hb, algorithm, route)
    (0.056, 0.128, 117, 56, 0, "bcr_fused"), (0.056, 0.128, 117, 56, 1, "sweep64"),
    (0.1, 0.039, 150, 59, 0, "bcr_fused"), (0.1, 0.039, 150, 59, 1, "sweep128"),
    (0.1, 0.036, 156, 62, 0, "bcr_fused"), (0.1, 0.033, 165, 65, 0, "sweep128"),
    (0.12, 0.018, 246, 119, 0, "global"), (0.15, 0.022, 204, 122, 0, "global"),
]


@pytest.mark.parametrize("so3,r3,Pb,hb,algo,route", HB, ids=["hb%d_algo%d" % (c[3], c[4]) for c in HB])
def test_half_bandwidth_edges(so3, r3, Pb, hb, algo, route):
    run_case(dataset(dt_so3=so3, dt_r3=r3), F, dict(Pb=Pb, hb=hb, a=9, route=route), solver_algorithm=algo)


# ---- the time-partitioned sweep -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("duration,Pb,force,p", [(5.0, 477, 0, 3), (5.0, 477, 2, 2), (12.0, 1107, 3, 3), (12.0, 1107, 5, 5)],
                         ids=["Pb477_auto", "Pb477_p2", "Pb1107_p3", "Pb1107_p5"])
def test_partitioned_sweep(duration, Pb, force, p):
    """Pb = 477 lies just above 8 (hb + 8) = 464, where the heuristic starts to partition."""
    run_case(dataset(duration), F, dict(Pb=Pb, hb=50, route="partitioned", p=p), solver_algorithm=1, solver_partitions=force)


# ---- damping --------------------------------------------------------------------------------------------------------------------
DAMP_ROUTES = [   # (dataset overrides, options, route)
    ({}, dict(solver_algorithm=0), "bcr_fused"),
    ({}, dict(solver_algorithm=1), "sweep64"),
    (dict(dt_so3=0.15, dt_r3=0.022), {}, "global"),
]


@pytest.mark.parametrize("kw,opts,route", DAMP_ROUTES, ids=[c[2] for c in DAMP_ROUTES])
def test_reused_diagonal_at_half_the_radius(kw, opts, route):
    """A rejected step: the second call reuses the first call's clamped diagonal at half the radius -- under clamps changed in
    between, which a recomputed diagonal would follow."""
    tr = calibrator(dataset(**kw), **opts).trajectory_
    first = tr.DebugLmStep(F, 1e4)
    assert first["route"] == route
    diag1 = check_step(first, 1e4, label=route + " first")
    assert np.all(np.abs(first["diag"] - diag1) <= 4 * np.spacing(diag1))
    tr.SetOption("min_lm_diagonal", float(np.median(diag1)))
    second = tr.DebugLmStep(F, 0.5e4, reuse_diagonal=1)
    assert second["route"] == route
    assert np.array_equal(second["diag"], first["diag"])
    check_step(second, 0.5e4, previous_diag=diag1, label=route + " reused")


@pytest.mark.parametrize("kw,opts,route", DAMP_ROUTES, ids=[c[2] for c in DAMP_ROUTES])
def test_both_clamps_engage(kw, opts, route):
    ds = dataset(**kw)
    probe = calibrator(ds, **opts).trajectory_.DebugLmStep(F, 1e4)
    scale = R.jacobi_scale(probe["band"], probe["C"])
    v = np.sort(R.hdiag(probe["band"], probe["C"]) * scale * scale)
    lo, hi = float(v[len(v) // 4]), float(v[3 * len(v) // 4])
    tr = calibrator(ds, min_lm_diagonal=lo, max_lm_diagonal=hi, **opts).trajectory_
    for radius in (1e4, 1e16):
        out = tr.DebugLmStep(F, radius)
        assert out["route"] == route
        diag = check_step(out, radius, min_diag=lo, max_diag=hi, label=route + " clamped")
        assert (diag == lo).sum() >= len(v) // 8 and (diag == hi).sum() >= len(v) // 8   # both clamps engage on many rows


@pytest.mark.parametrize("algo,route", [(0, "bcr_fused"), (1, "sweep64")])
def test_without_jacobi_scaling(algo, route):
    run_case(dataset(), F, dict(route=route), solver_algorithm=algo, jacobi_scaling=0)


# ---- the distributed cyclic reduction (one process emulates the ranks) --------------------------------------------------------
DIST = [   # (duration, flags, dataset overrides, a, n, ranks)
    (6.0, F, {}, 9, 9, (2, 3, 7, 9)),
    (11.5, F, {}, 9, 17, (7, 17)),
    (6.0, E.SPLINE | E.T_I_C | E.ACC_BIAS, {}, 15, 9, (3, 7)),
    (6.0, E.SPLINE | E.T_I_C | E.ACC_BIAS | E.CAM_LINE_DELAY, {}, 16, 9, (2, 9)),
    (6.0, F | E.POINTS, dict(board=(6, 3), corners_per_view=18), 63, 9, (3, 7)),
]


@pytest.mark.parametrize("duration,flags,kw,a,n,ranks", DIST, ids=["n%d_a%d" % (c[4], c[3]) for c in DIST])
def test_distributed_cyclic_reduction(duration, flags, kw, a, n, ranks):
    ds = dataset(duration, **kw)
    for N in ranks:
        run_case(ds, flags, dict(a=a, n=n, route="distributed"), radii=(1e4,) if flags & E.POINTS else (1e4, 1e16), nranks=N)


# ---- failure ------------------------------------------------------------------------------------------------------------------
FAIL_ROUTES = [   # (duration, dataset overrides, options, nranks, route)
    (1.2, {}, dict(solver_algorithm=0), 0, "bcr_fused"),
    (0.3, {}, dict(solver_algorithm=0), 0, "bcr_unfused"),
    (3.0, {}, dict(solver_algorithm=0), 0, "bcr_fused"),
    (1.2, {}, dict(solver_algorithm=1), 0, "sweep64"),
    (1.2, dict(dt_so3=0.1, dt_r3=0.039), dict(solver_algorithm=1), 0, "sweep128"),
    (5.0, {}, dict(solver_algorithm=1), 0, "partitioned"),
    (1.2, dict(dt_so3=0.15, dt_r3=0.022), {}, 0, "global"),
    (6.0, {}, {}, 3, "distributed"),
]


@pytest.mark.parametrize("duration,kw,opts,nranks,route", FAIL_ROUTES, ids=["%s_%g" % (c[4], c[0]) for c in FAIL_ROUTES])
def test_indefinite_system_is_reported(duration, kw, opts, nranks, route):
    """A clamped diagonal of -1 at radius 1e-3 makes M negative definite (every pivot negative): every route must raise the
    failure flag -- a finite step without it would be accepted by the LM control."""
    tr = calibrator(dataset(duration, **kw), min_lm_diagonal=-1.0, max_lm_diagonal=-1.0, **opts).trajectory_
    out = tr.DebugLmStep(F, 1e-3, nranks=nranks)
    assert out["route"] == route
    _, diag, S = R.from_step(out, 1e-3, -1.0, -1.0)
    assert np.all(S.Mb[:, 0] < 0) and np.all(np.diag(S.Mc) < 0)
    assert out["chol_failed"], route


def test_read_out_is_the_public_normal_equations():
    """The hook's packed band, arrow rows, corner and gradient are the public Evaluate's H and g."""
    tr = calibrator(dataset()).trajectory_
    out = tr.DebugLmStep(F, 1e4)
    _, H, g = tr.Evaluate(F)
    Pb = out["Pb"]
    scale = np.abs(H).max()
    for k in range(out["W"]):
        j = np.arange(Pb - k)
        assert np.abs(out["band"][j, k] - H[j + k, j]).max() <= 1e-12 * scale
    assert np.abs(out["Et"] - H[Pb:, :Pb]).max() <= 1e-12 * scale and np.abs(out["C"] - H[Pb:, Pb:]).max() <= 1e-12 * scale
    assert np.abs(out["g"] - g).max() <= 1e-12 * np.abs(g).max()
    assert np.all(np.abs(H[:Pb, :Pb][np.abs(np.subtract.outer(np.arange(Pb), np.arange(Pb))) > out["hb"]]) == 0)
