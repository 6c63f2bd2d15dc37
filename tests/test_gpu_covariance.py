"""oicc_estimate_covariance (the selected inverse of the band + arrow normal equations on the device) against the extended-precision
inverse of tests/covariance_reference.py.

Every case asserts its geometry (P, Pb, a, hb) first, runs with the LDS poisoned (debug_poison_lds) and compares IN THE SCALED
SPACE (Zs = (S H S)^-1, s_i = H_ii^-1/2; the device's unscaled blocks are divided by s_i s_j again) the whole arrow block, the
3 x 3 block of every knot and the knot-arrow cross blocks of the first, middle and last active knot of each spline:

    max |Zs_device - Zs| / max |Zs|  <=  100 kappa_1(Hs) eps

the forward bound of a Cholesky solve with the largest constant tests/test_gpu_linear_solve_reference.py allows (FORWARD_C).  H is
the dense J^T J of Evaluate(flags) on the same estimator.  Also: the arrow block symmetric to 4 ulp, every diagonal entry > 0,
lambda_min / 2 <= rcond <= 2 P lambda_min, variance_factor = 2 cost / (m - P) to 1e-14.

Every case prints a MARGIN line with its error / (kappa_1 eps).
"""
import ctypes as C

import numpy as np
import pytest

import covariance_reference as CR
import normal_equations_cases as cases
from openimucameracalibrator_amd import synthetic, estimator as E

pytestmark = pytest.mark.gpu

FLAGS1, ALL = cases.FLAGS1, cases.ALL
EPS = CR.EPS
BOUND_C = 100.0
# (the largest measured error / (kappa_1 eps) belongs here and in DESIGN.md section 3.v once recorded from the MARGIN lines)
CASES = {   # name -> (make_config overrides, flags, Optimize iterations before the estimate, expected geometry)
    "tiny_FLAGS1": ({}, FLAGS1, 0, dict(P=138, Pb=129, a=9, hb=50)),
    "tiny_FLAGS1_optimized": ({}, FLAGS1, 10, dict(P=138, Pb=129, a=9, hb=50)),
    "tiny_line_delay": ({}, FLAGS1 | E.CAM_LINE_DELAY, 0, dict(P=139, Pb=129, a=10, hb=50)),
    "tiny_imu_biases": ({}, FLAGS1 | E.IMU_BIASES, 0, dict(P=156, Pb=129, a=27, hb=50)),
    "tiny_ALL": ({}, ALL, 0, dict(P=172, Pb=129, a=43, hb=50)),
    "tiny_3s_ALL": (dict(duration=3.0, num_views=30), ALL, 0, dict(P=340, Pb=297, a=43, hb=50)),
    "tiny_hb77": (dict(dt_so3=0.12, dt_r3=0.03, duration=1.5, num_views=15), FLAGS1 | E.CAM_LINE_DELAY, 0, dict(P=217, Pb=207, a=10, hb=77)),
    "tiny_hb77_ALL": (dict(dt_so3=0.12, dt_r3=0.03, duration=1.5, num_views=15), ALL, 0, dict(P=250, Pb=207, a=43, hb=77)),   # the window of 128 and 44 border rows exceed the LDS: the forward factor runs on the global-memory route
    "short_0.75s": (dict(duration=0.75, num_views=8), FLAGS1, 0, dict(P=102, a=9)),
}


def calibrator(overrides):
    cal = E.ImuCameraCalibrator().BatchInitSpline(synthetic.make_config("tiny", **overrides))
    cal.trajectory_.SetOption("debug_poison_lds", 1)
    return cal


def num_residuals(cal):
    return 2 * cal.num_corners + 3 * int(cal.accl_accepted.sum()) + 3 * int(cal.gyro_accepted.sum())


@pytest.mark.parametrize("name", list(CASES))
def test_covariance_against_extended_precision_inverse(name):
    overrides, flags, iters, geometry = CASES[name]
    cal = calibrator(overrides)
    tr = cal.trajectory_
    if iters:
        tr.Optimize(iters, flags)
    cov = tr.EstimateCovariance(flags)
    info = cov["info"]
    for k, v in geometry.items():
        assert info[k] == v, (name, k, info[k], v)
    assert info["status"] == tr.COV_OK, (name, cov["status_name"], cov["message"])
    P, Pb, a = info["P"], info["Pb"], info["a"]
    cost, H, _ = tr.Evaluate(flags)
    ref = CR.invert(H)
    assert ref.residual < 1e-17 * ref.kappa1, (name, ref.residual, ref.kappa1)
    s = ref.s.astype(np.float64)
    Zs = ref.Zs.astype(np.float64)
    zmax = float(np.abs(Zs).max())
    lay = cov["layout"]

    # arrow block
    sa = s[Pb:]
    arrow_s = cov["arrow"] / np.outer(sa, sa)
    err = float(np.abs(arrow_s - Zs[Pb:, Pb:]).max())
    ulp = np.spacing(np.abs(cov["arrow"]))
    assert np.all(np.abs(cov["arrow"] - cov["arrow"].T) <= 4 * ulp), name
    assert np.all(np.diag(cov["arrow"]) > 0), name
    # knot blocks and cross blocks
    n_blocks = 0
    for kind, key in ((0, "so3"), (1, "r3")):
        offs = np.asarray(lay[key])
        active = np.flatnonzero(offs >= 0)
        assert len(active), (name, key)
        assert np.all(np.isnan(cov[key][offs < 0])), (name, key, "knots outside the active set must be NaN")
        for k in active:
            o = int(offs[k])
            blk = cov[key][k] / np.outer(s[o:o + 3], s[o:o + 3])
            assert np.all(np.diag(cov[key][k]) > 0), (name, key, k)
            assert np.array_equal(cov[key][k], cov[key][k].T), (name, key, k)
            err = max(err, float(np.abs(blk - Zs[o:o + 3, o:o + 3]).max()))
            n_blocks += 1
        for k in (active[0], active[len(active) // 2], active[-1]):
            o = int(offs[k])
            cross = tr.GetCovarianceKnotArrow(kind, int(k)) / np.outer(s[o:o + 3], sa)
            err = max(err, float(np.abs(cross - Zs[o:o + 3, Pb:]).max()))
        inactive = np.flatnonzero(offs < 0)
        if len(inactive):
            assert np.all(np.isnan(tr.GetCovarianceKnotArrow(kind, int(inactive[0]))))
    assert 3 * n_blocks == Pb, (name, n_blocks, Pb)
    rel = err / zmax
    ratio = rel / (ref.kappa1 * EPS)
    print("MARGIN %-24s P %d Pb %d a %d hb %d  error %.3e  kappa1 %.3e  error/(kappa eps) %.3e (bound %g)  lambda_min %.3e rcond %.3e (reference %.3e)"
          % (name, P, Pb, a, info["hb"], rel, ref.kappa1, ratio, BOUND_C, ref.lambda_min, info["rcond"], ref.rcond))
    assert rel <= BOUND_C * ref.kappa1 * EPS, (name, rel, ref.kappa1)
    assert ref.lambda_min / 2 <= info["rcond"] <= 2 * P * ref.lambda_min, (name, info["rcond"], ref.lambda_min)
    m = num_residuals(cal)
    assert info["num_residuals"] == m
    vf = 2 * cost / (m - P)
    assert abs(info["variance_factor"] - vf) <= 1e-14 * vf, (name, info["variance_factor"], vf)
    assert abs(info["cost"] - cost) <= 1e-14 * cost


def _getter_status(tr):
    buf = np.zeros(64 * 64)
    return tr._b.get_covariance_arrow(tr._h, buf.ctypes.data_as(C.POINTER(C.c_double)), 64)


def test_rank_deficient_recording_is_reported_not_inverted():
    """short_0.3s: three views; lambda_min(Hs) = 5e-16, the float64 rcond 1e-15 lies three decades under covariance_min_rcond while the
    smallest pivot (4e-12) is still positive: rcond is the criterion."""
    cal = calibrator(dict(duration=0.3, num_views=3))
    tr = cal.trajectory_
    lay = tr.GetTangentLayout(FLAGS1)
    assert lay["P"] == 57 and int(lay["other"][0]) == 48, lay
    cov = tr.EstimateCovariance(FLAGS1)
    print("MARGIN short_0.3s rcond %.3e status %s" % (cov["info"]["rcond"], cov["status_name"]))
    assert cov["info"]["status"] == tr.COV_RANK_DEFICIENT, cov
    assert cov["info"]["rcond"] < 1e-12
    assert cov["arrow"] is None
    assert _getter_status(tr) == -4   # OICC_ERR_STATE
    with pytest.raises(E.OiccError):
        tr.GetCovarianceKnotArrow(0, 0)


def test_unsupported_geometries_are_refused():
    ds_name, build, _ = cases.SHAPES["knot_spacing_200_17"]
    cal = E.ImuCameraCalibrator().BatchInitSpline(build())
    tr = cal.trajectory_
    geo = tr.DebugLmStep(FLAGS1, solve=False)
    assert geo["hb"] == 197, geo
    with pytest.raises(E.OiccError, match=r"half bandwidth 197.*status -5"):
        tr.EstimateCovariance(FLAGS1)
    tiny = calibrator({}).trajectory_
    with pytest.raises(E.OiccError, match=r"OICC_POINTS.*status -5"):
        tiny.EstimateCovariance(FLAGS1 | E.POINTS)
    assert _getter_status(tiny) == -4


def test_setters_invalidate_the_estimate():
    tr = calibrator({}).trajectory_
    assert _getter_status(tr) == -4
    assert tr.EstimateCovariance(FLAGS1)["info"]["status"] == tr.COV_OK
    assert _getter_status(tr) == 0
    T = tr.GetT_i_c()
    tr.SetT_i_c(T[:4], T[4:])
    assert _getter_status(tr) == -4
    assert tr.EstimateCovariance(FLAGS1)["info"]["status"] == tr.COV_OK
    tr.Optimize(1, FLAGS1)
    assert _getter_status(tr) == -4


def test_calibration_standard_deviations_are_the_scaled_arrow_diagonal():
    cal = calibrator({})
    flags = FLAGS1 | E.CAM_LINE_DELAY
    sd = cal.GetCalibrationStdDevs(flags, scaled=True)
    raw = cal.GetCalibrationStdDevs(flags, scaled=False)
    assert sd["status"] == "ok" and len(sd["tangent_order"]) == 10
    assert sd["tangent_order"][:7] == ["T_i_c[0]", "T_i_c[1]", "T_i_c[2]", "T_i_c[3]", "T_i_c[4]", "T_i_c[5]", "gravity[0]"]
    d = np.sqrt(sd["variance_factor"] * np.diag(sd["covariance"]))
    got = np.concatenate([sd["t_i_c"], sd["q_i_c"], sd["gravity"], [sd["line_delay"]]])
    assert np.allclose(got, d, rtol=1e-14, atol=0)
    # scaled=False: the same quantities without the variance factor.  `raw` is an estimate of its own -- a second Jacobian pass, whose
    # sums are not bit-repeatable, through an inverse that amplifies the difference by kappa -- so it is checked against its own matrix
    d_raw = np.sqrt(np.diag(raw["covariance"]))
    got_raw = np.concatenate([raw["t_i_c"], raw["q_i_c"], raw["gravity"], [raw["line_delay"]]])
    assert raw["status"] == "ok" and raw["scaled"] is False and sd["scaled"] is True
    assert np.allclose(got_raw, d_raw, rtol=1e-14, atol=0)
    assert np.allclose(got_raw * np.sqrt(sd["variance_factor"]), got, rtol=1e-6, atol=0)   # kappa_1 eps = 2e-9 for this case (MARGIN tiny_line_delay)
    assert sd["accl_bias"] is None and sd["accl_intrinsics"] is None
