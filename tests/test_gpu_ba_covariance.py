"""oicc_ba_estimate_covariance on the device: the covariance of the intrinsics and the view poses, variable together, against the
50-digit inverse (tests/ba_covariance_reference.py) of the J^T J that oicc_ba_evaluate returns for the same flags and mask.

Every comparison is made in scaled form, Zs_ij = cov_ij / (s_i s_j) with s_i = H_ii^-1/2, and the bound is 100 kappa_1(S H S) eps
relative to max |Zs| (the constant of tests/test_gpu_ba_point_covariances.py); kappa_1 comes from the reference's float64 inverse,
never from the code under test."""
import contextlib
import functools
import io
import json

import numpy as np
import pytest

import ba_covariance_reference as R
from openimucameracalibrator_amd import camera_calibrator as CC, synthetic as S

pytestmark = pytest.mark.gpu

EPS = R.EPS
POSE = CC.BA_POSITION | CC.BA_ORIENTATION
CAMERAS = ["pinhole", "pinhole_radtan", "gopro6_fisheye", "gopro9_division", "gopro6_double_sphere", "gopro9_eucm"]   # tests/test_ba_oracle.py
ERR_STATE, ERR_INVALID_ARG = -4, -1
CHI2_0999 = {4: 18.4668, 6: 22.4577}   # 0.999 quantiles of chi^2 with 4 and 6 degrees of freedom


def stage3_mask(ds):
    """The intrinsics of the third BundleAdjustViews of CameraCalibrator.RunCalibration."""
    opt = CC.PRINCIPAL_POINTS | CC.FOCAL_LENGTH | CC.ASPECT_RATIO
    if ds["model_name"] == "PINHOLE":
        opt |= CC.RADIAL_DISTORTION
    elif ds["model_name"] == "PINHOLE_RADIAL_TANGENTIAL":
        opt |= CC.TANGENTIAL_DISTORTION
    return CC.intrinsics_mask(ds["model"], opt)


@functools.lru_cache(maxsize=None)
def dataset(camera, num_views, noise_px=0.2):
    return CC.make_calibration_dataset(camera, num_views=num_views, corners_per_view=40, noise_px=noise_px)


def adjuster(ds, pose=None, **opts):
    ba = CC.ViewBundleAdjuster()
    for k, v in opts.items():
        ba.SetOption(k, v)
    ba.SetCamera(ds["model"], ds["intrinsics"]); ba.SetScenePoints(ds["points"])
    ba.SetViews(ds["pose_init"] if pose is None else pose, ds["corner_offset"], ds["uv"], ds["point_ids"])
    return ba


def raw_getters(ba, nv=None):
    """Return codes of the three getters of the C interface."""
    nv = ba.nv if nv is None else nv
    buf = np.zeros(max(1, nv * 36 + nv * 60 + 100))
    return (ba.b.get_covariance_intrinsics(ba.h, CC._dp(buf), 10), ba.b.get_covariance_poses(ba.h, CC._dp(buf), nv),
            ba.b.get_covariance_pose_intrinsics(ba.h, CC._dp(buf), nv))


def check_block_inverses(cov, H, d):
    """Every d x d block of cov against the 50-digit inverse of the matching diagonal block of H, in scaled form."""
    for v in range(len(cov)):
        blk = H[d * v:d * v + d, d * v:d * v + d]
        s = R.scale_factors(blk)
        ref = R.dense_inverse(blk)
        err = np.abs(cov[v] / np.outer(s, s) - R.to_float(ref)).max() / float(R.max_abs([ref]))
        assert err <= 100 * R.kappa1(blk) * EPS, (v, err)


def check(ba, flags, mask, label, dense, n_obs, columns_identity=False):
    """Estimate, then every handed-out entry against the 50-digit reference of Evaluate's J^T J.  Returns the info dict."""
    cost, H, _ = ba.Evaluate(flags, mask)
    info = ba.EstimateCovariance(flags, mask)
    assert info["status"] == CC.COV_OK, info
    nv = ba.nv
    d = 3 * bool(flags & CC.BA_POSITION) + 3 * bool(flags & CC.BA_ORIENTATION)
    a = H.shape[0] - nv * d
    Hr, used = R.reduce(H, nv, d, a)
    nu = len(used)
    n_with_obs = nu if d else nv        # (with the poses constant J^T J does not show which views have observations: the callers' views all do)
    assert (info["pose_dim"], info["a"], info["views_used"], info["P"], info["first_bad"]) == (d, a, n_with_obs, d * nu + a, -1)
    assert info["num_residuals"] == 2 * n_obs
    s = R.scale_factors(Hr)
    s_th = s[nu * d:]
    if dense:
        theta, poses, cross = R.handed_out_from_dense(R.dense_inverse(Hr), nu, d, a)
    else:
        theta, poses, cross = R.schur_inverse(Hr, nu, d, a)
    kappa = R.kappa1(Hr)
    zmax = float(R.max_abs([theta] + poses))            # the largest entry of an SPD matrix lies on its diagonal
    bound = 100 * kappa * EPS
    th, po, cr = ba.CovarianceIntrinsics(), ba.CovariancePoses(), ba.CovariancePoseIntrinsics()
    assert th.shape == (a, a) and po.shape == (nv, d, d) and cr.shape == (nv, d, a)
    worst = 0.0
    if a:
        worst = max(worst, np.abs(th / np.outer(s_th, s_th) - R.to_float(theta)).max())
        assert np.array_equal(th, th.T) and np.all(np.diag(th) > 0)
    for v in range(nv):
        if v not in used:
            assert np.all(np.isnan(po[v])) and np.all(np.isnan(cr[v])), v
    zs_diag = [np.diag(th) / (s_th * s_th)] if a else []
    for i, v in enumerate(used):
        sv = s[i * d:(i + 1) * d]
        worst = max(worst, np.abs(po[v] / np.outer(sv, sv) - R.to_float(poses[i])).max())
        assert np.array_equal(po[v], po[v].T) and np.all(np.diag(po[v]) > 0), v
        zs_diag.append(np.diag(po[v]) / (sv * sv))
        if a:
            worst = max(worst, np.abs(cr[v] / np.outer(sv, s_th) - R.to_float(cross[i])).max())
    err = worst / zmax
    print("MARGIN %s: P %d kappa %.3e rcond %.3e largest error / (kappa eps) %.3e (bound 100)" % (label, info["P"], kappa, info["rcond"], err / (kappa * EPS)))
    assert err <= bound, (label, err, bound)
    rc_ref = R.rcond_of(theta, poses)
    assert abs(1.0 / info["rcond"] - 1.0 / rc_ref) <= bound * zmax, (info["rcond"], rc_ref)
    assert abs(1.0 / info["rcond"] - np.concatenate(zs_diag).max()) <= 16 * EPS / info["rcond"]   # ... and it is the maximum of what was handed out (a few roundings of the unscaling and back)
    assert abs(info["cost"] - cost) <= 1e-13 * cost
    vf = 2 * info["cost"] / (2 * n_obs - info["P"])
    assert abs(info["variance_factor"] - vf) <= 1e-14 * vf
    if columns_identity and a:
        # the intrinsics columns X = [cross; theta] of the scaled inverse satisfy (S H S) X = [0; I], however they were computed
        X = np.zeros((nu * d + a, a), dtype=np.longdouble)
        for i, v in enumerate(used):
            X[i * d:(i + 1) * d] = cr[v] / np.outer(s[i * d:(i + 1) * d], s_th)
        X[nu * d:] = th / np.outer(s_th, s_th)
        Rs = R.scaled_longdouble(Hr) @ X
        Rs[nu * d:] -= np.eye(a)
        res = float(np.abs(Rs).max()) / zmax
        print("MARGIN %s: identity residual / (kappa eps) %.3e (bound 100)" % (label, res / (kappa * EPS)))
        assert res <= bound, (label, res, bound)
    return info


def test_dense_case_every_entry():
    """9 views x 40 corners, pinhole_radtan, all 10 intrinsics, d = 6, P = 64: every handed-out entry against the dense inverse."""
    ds = dataset("pinhole_radtan", 9)
    ba = adjuster(ds)
    info = check(ba, POSE, CC.intrinsics_mask(ds["model"], CC.ALL), "dense 9 views", True, len(ds["uv"]))
    assert info["P"] == 64


@pytest.mark.parametrize("camera", CAMERAS)
def test_six_camera_models_67_views(camera):
    """67 views (not a multiple of 16 or 64), stage-3 intrinsics: pose and cross blocks against the Schur restatement, the
    intrinsics columns through the identity (S H S) X = [0; I]."""
    ds = dataset(camera, 67)
    assert len(ds["pose_init"]) == 67
    ba = adjuster(ds)
    check(ba, POSE, stage3_mask(ds), "67 views " + camera, False, len(ds["uv"]), columns_identity=True)


@pytest.mark.parametrize("name,flags,bits", [("position only", CC.BA_POSITION, CC.FOCAL_LENGTH | CC.PRINCIPAL_POINTS),
                                             ("orientation only", CC.BA_ORIENTATION, CC.FOCAL_LENGTH | CC.PRINCIPAL_POINTS),
                                             ("a = 0", POSE, 0), ("d = 0, a = 2", 0, CC.PRINCIPAL_POINTS), ("a = 1", POSE, CC.FOCAL_LENGTH)])
def test_active_sets(name, flags, bits):
    ds = dataset("pinhole", 9)
    ba = adjuster(ds)
    info = check(ba, flags, CC.intrinsics_mask(ds["model"], bits), name, True, len(ds["uv"]))
    if name == "a = 0":
        _, H, _ = ba.Evaluate(flags, 0)
        check_block_inverses(ba.CovariancePoses(), H, 6)      # the blocks are the inverses of the 6 x 6 blocks
        assert info["a"] == 0 and ba.CovariancePoseIntrinsics().shape == (9, 6, 0) and ba.CovarianceIntrinsics().shape == (0, 0)
        assert raw_getters(ba) == (0, 0, 0)
    if name == "d = 0, a = 2":
        assert info["pose_dim"] == 0 and info["P"] == 2 and ba.CovariancePoses().shape == (9, 0, 0)


def test_one_view_only():
    ds = dataset("pinhole", 1)
    ba = adjuster(ds)
    check(ba, POSE, CC.intrinsics_mask(ds["model"], CC.FOCAL_LENGTH), "one view", True, len(ds["uv"]))


def test_empty_view_and_view_with_more_than_64_observations():
    """Ragged views as tests/test_gpu_ba.py builds them: the 48-point board seen twice in view 0 (96 observations: two chunks of the
    assembly), a view without observations (NaN outputs, not counted in P, views_used or the variance factor; check() compares
    the neighbours with the reference of the system WITHOUT that view), two ordinary views."""
    ds = CC.make_calibration_dataset("pinhole", num_views=4, corners_per_view=48)
    off = ds["corner_offset"]
    n0 = off[1]
    uv = np.concatenate([ds["uv"][:n0], ds["uv"][:n0] + 0.1, ds["uv"][off[1]:off[2]], ds["uv"][off[3]:off[4]]])
    pid = np.concatenate([ds["point_ids"][:n0], ds["point_ids"][:n0], ds["point_ids"][off[1]:off[2]], ds["point_ids"][off[3]:off[4]]])
    n1, n3 = off[2] - off[1], off[4] - off[3]
    o = np.array([0, 2 * n0, 2 * n0 + n1, 2 * n0 + n1, 2 * n0 + n1 + n3], dtype=np.int64)
    assert 2 * n0 > 64
    ba = adjuster(dict(ds, uv=uv, point_ids=pid.astype(np.int32), corner_offset=o))
    info = check(ba, POSE, CC.intrinsics_mask(ds["model"], CC.FOCAL_LENGTH | CC.RADIAL_DISTORTION), "ragged views", True, len(uv))
    assert info["views_used"] == 3 and info["P"] == 18 + 3
    assert np.all(np.isnan(ba.CovariancePoses()[2])) and np.all(np.isfinite(ba.CovariancePoses()[[0, 1, 3]]))


@pytest.mark.parametrize("bits", [CC.FOCAL_LENGTH | CC.RADIAL_DISTORTION, 0])
def test_views_with_three_and_more_chunks(bits):
    """More than 128 observations in a view: the assembly adds the view's block and arrow rows from three or more waves with atomics,
    so the estimate sums them again in chunk order.  View 0 sees the 48-point board three times (144 observations, 3 chunks), view 1
    five times (240, 4 chunks), the others once; every entry against the reference, and repeated estimates return the same bits."""
    ds = CC.make_calibration_dataset("pinhole", num_views=5, corners_per_view=48)
    off = ds["corner_offset"]
    uv, pid, o = [], [], [0]
    for v, shifts in enumerate([(0.0, 0.1, -0.1), (0.0, 0.1, -0.1, 0.2, -0.2), (0.0,), (0.0,), (0.0,)]):
        for sh in shifts:
            uv.append(ds["uv"][off[v]:off[v + 1]] + sh); pid.append(ds["point_ids"][off[v]:off[v + 1]])
        o.append(o[-1] + len(shifts) * (off[v + 1] - off[v]))
    assert o[1] - o[0] > 128 and o[2] - o[1] > 192
    ba = adjuster(dict(ds, uv=np.concatenate(uv), point_ids=np.concatenate(pid).astype(np.int32), corner_offset=np.asarray(o, dtype=np.int64)))
    mask = CC.intrinsics_mask(ds["model"], bits)
    check(ba, POSE, mask, "views of 3 and 4 chunks, a = %d" % bin(mask).count("1"), True, o[-1])
    runs = []
    for _ in range(4):
        info = ba.EstimateCovariance(POSE, mask)
        runs.append((info["rcond"], ba.CovarianceIntrinsics().tobytes(), ba.CovariancePoses().tobytes(), ba.CovariancePoseIntrinsics().tobytes()))
    assert all(r == runs[0] for r in runs[1:])


def fronto_parallel(camera_intrinsics):
    """Three views with R = I at 0.30 / 0.36 / 0.42 m above the centre of the 8 x 6 board, exact projections."""
    ds = dataset("pinhole", 9)
    pts = ds["points"]
    centre = np.array([3.5 * 0.021, 2.5 * 0.021, 0.0])
    pose = np.zeros((3, 6))
    uv, pid, off = [], [], [0]
    for v, dist in enumerate((0.30, 0.36, 0.42)):
        pose[v, :3] = centre + [0.0, 0.0, -dist]
        px, ok = S.project(S.CAM_PINHOLE, camera_intrinsics, pts[:, :3] - pose[v, :3])
        assert np.all(ok)
        uv.append(px); pid.append(np.arange(len(pts))); off.append(off[-1] + len(pts))
    return dict(ds, intrinsics=np.asarray(camera_intrinsics, dtype=np.float64), pose_init=pose, pose_true=pose, uv=np.concatenate(uv),
                point_ids=np.concatenate(pid).astype(np.int32), corner_offset=np.asarray(off, dtype=np.int64))


def test_rank_deficiency_is_reported_and_nothing_handed_out():
    """Distortion-free pinhole, focal length and positions variable: focal length and depth are exactly exchangeable."""
    ds = fronto_parallel([450.0, 1.0, 0.0, 480.0, 270.0, 0.0, 0.0])
    ba = adjuster(ds)
    info = ba.EstimateCovariance(CC.BA_POSITION, CC.intrinsics_mask(ds["model"], CC.FOCAL_LENGTH))
    print("rank deficient case: status %d rcond %.3e first_bad %d" % (info["status"], info["rcond"], info["first_bad"]))
    assert info["status"] == CC.COV_RANK_DEFICIENT and info["rcond"] < 1e-12
    assert raw_getters(ba) == (ERR_STATE, ERR_STATE, ERR_STATE)
    with pytest.raises(RuntimeError):
        ba.CovarianceIntrinsics()
    # the synthetic pinhole camera's distortion breaks the symmetry
    ds = fronto_parallel(S.CAMERAS["pinhole"][1])
    ba = adjuster(ds)
    info = check(ba, CC.BA_POSITION, CC.intrinsics_mask(ds["model"], CC.FOCAL_LENGTH), "fronto-parallel, distorted", True, len(ds["uv"]))
    assert 1e-7 < info["rcond"] < 1e-4


def test_state_and_determinism():
    ds = dataset("pinhole", 9)
    ba = adjuster(ds)
    mask = CC.intrinsics_mask(ds["model"], CC.FOCAL_LENGTH | CC.PRINCIPAL_POINTS)
    assert raw_getters(ba) == (ERR_STATE,) * 3                 # nothing estimated yet
    with pytest.raises(RuntimeError):
        ba.CovariancePoses()

    def estimate():
        assert ba.EstimateCovariance(POSE, mask)["status"] == CC.COV_OK
        assert raw_getters(ba) == (0, 0, 0)
        return [x.tobytes() for x in (ba.CovarianceIntrinsics(), ba.CovariancePoses(), ba.CovariancePoseIntrinsics())]

    first = estimate()
    assert estimate() == first                                   # two estimates in a row: the same bits
    ba.SetPoses(ds["pose_init"])
    assert raw_getters(ba) == (ERR_STATE,) * 3
    assert estimate() == first
    ba.SetCamera(ds["model"], ds["intrinsics"])
    assert raw_getters(ba) == (ERR_STATE,) * 3
    estimate()
    ba.SetOption("huber_width", 1.345)
    assert raw_getters(ba) == (ERR_STATE,) * 3
    estimate()
    ba.Optimize(1, POSE, mask)
    assert raw_getters(ba) == (ERR_STATE,) * 3
    moved = estimate()
    with pytest.raises(RuntimeError):                            # timing is recorded only on request
        ba.CovarianceTiming()
    ba.SetOption("covariance_timing", 1)
    assert estimate() == moved                                   # the events change nothing
    assert all(0.0 < ms < 50.0 for ms in ba.CovarianceTiming())
    info = CC._abi.BaCovarianceInfo()
    assert ba.b.estimate_covariance(ba.h, CC.BA_POINTS, 0, info) == ERR_INVALID_ARG
    assert raw_getters(ba) == (ERR_STATE,) * 3                 # a refused estimate leaves none behind


@pytest.mark.parametrize("camera", CAMERAS)
def test_meaning_against_truth(camera):
    """0.2 px noise, no robust loss, poses + stage-3 intrinsics optimised: with Sigma = variance_factor cov the errors against the
    truth stay below the 0.999 chi^2 quantile and the variance factor is the noise variance."""
    ds = dataset(camera, 45)
    ba = adjuster(ds, huber_width=0.0)
    mask = stage3_mask(ds)
    s = ba.Optimize(100, POSE, mask)
    assert s["termination"] == 0
    info = ba.EstimateCovariance(POSE, mask)
    assert info["status"] == CC.COV_OK
    vf = info["variance_factor"]
    idx = [k for k in range(CC.NUM_INTRINSICS[ds["model"]]) if (mask >> k) & 1]
    e = ba.GetCamera()[idx] - ds["intrinsics"][idx]
    m_intr = float(e @ np.linalg.solve(vf * ba.CovarianceIntrinsics(), e))
    po = ba.CovariancePoses()
    ep = ba.GetPoses() - ds["pose_true"]
    m_pose = max(float(ep[v] @ np.linalg.solve(vf * po[v], ep[v])) for v in range(45))
    print("MEANING %s: intrinsics Mahalanobis^2 %.2f (quantile %.1f), worst pose %.2f (22.5), variance factor %.4f" % (camera, m_intr, CHI2_0999[len(idx)], m_pose, vf))
    assert m_intr < CHI2_0999[len(idx)]
    assert m_pose < CHI2_0999[6]
    assert abs(vf - 0.04) <= 0.1 * 0.04


def test_calibrator_mirror_and_application(tmp_path):
    import test_ba_applications as T
    from openimucameracalibrator_amd import calibrate_camera as APP, io_files
    ds = dataset("gopro9_division", 45)
    sc = T.scene_of(ds)
    cal = APP.calibrate_camera_from_json(sc, ds["model_name"], grid_size=0.02)
    assert cal is not None
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        cal.PrintResult()
    assert "+-" not in buf.getvalue()                              # unchanged without an estimate
    info = cal.EstimateCovariance()
    assert info["status"] == CC.COV_OK
    # the adjuster-level result on the same views
    pose, off, uv, pid = cal.views.flat()
    ba = CC.ViewBundleAdjuster()
    ba.SetCamera(cal.model, cal.intr); ba.SetScenePoints(cal.points); ba.SetViews(pose, off, uv, pid)
    mask = stage3_mask(ds)
    info2 = ba.EstimateCovariance(POSE, mask)
    for k in info:      # the cost comes from the assembly pass, which sums it with atomics: last bits may differ between two passes
        assert info2[k] == info[k] or (k in ("cost", "variance_factor") and abs(info2[k] - info[k]) <= 1e-13 * info[k]), k
    assert np.array_equal(ba.CovarianceIntrinsics(), cal.covariance_["intrinsics"]) and np.array_equal(ba.CovariancePoses(), cal.covariance_["poses"])
    sd = cal.GetIntrinsicsStdDevs()
    assert list(sd) == ["focal_length", "aspect_ratio", "principal_pt_x", "principal_pt_y"]
    assert np.allclose([sd[k] for k in sd], np.sqrt(info["variance_factor"] * np.diag(ba.CovarianceIntrinsics())), rtol=4 * EPS, atol=0)
    names, corr = cal.GetIntrinsicsCorrelation()
    assert np.allclose(np.diag(corr), 1.0) and np.abs(corr).max() <= 1.0 + 1e-12
    assert cal.GetPoseStdDevs().shape == (cal.NumViews(), 6)
    with contextlib.redirect_stdout(buf):
        cal.PrintResult()
    assert "+-" in buf.getvalue()
    # the Python application, with and without the flag
    corners = str(tmp_path / "corners.uson")
    open(corners, "wb").write(io_files.ubjson_encode(sc))
    out0, out1 = str(tmp_path / "plain"), str(tmp_path / "cov")
    args = ["--input_corners=" + corners, "--camera_model_to_calibrate=" + ds["model_name"], "--grid_size=0.02"]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert APP.main(args + ["--save_path_calib_dataset=" + out0]) == 0
        plain_stdout = buf.getvalue()
        assert APP.main(args + ["--save_path_calib_dataset=" + out1, "--estimate_covariance"]) == 0
    assert "Largest correlation" not in plain_stdout and "Largest correlation" in buf.getvalue() and "focal_length: " in buf.getvalue()
    obj = json.load(open(out1 + ".json"))
    cov = obj.pop("intrinsics_covariance")
    assert sorted(cov) == ["correlation", "parameters", "rcond", "std_dev", "variance_factor"]
    # (a calibration run twice ends at parameters that agree to the LM tolerances, not to the bit: its assembly sums with atomics)
    assert cov["parameters"] == list(sd) and abs(cov["rcond"] - info["rcond"]) <= 1e-6 * info["rcond"]
    assert np.allclose(cov["std_dev"], [sd[k] for k in sd], rtol=1e-6, atol=0) and np.allclose(cov["correlation"], corr, rtol=0, atol=1e-6)
    # without the flag: the file as it always was -- same keys in the same order and the writer's formatting (its bytes for given
    # numbers are pinned in tests/test_ba_covariance_reference.py); the numbers of two runs agree to the LM tolerances
    plain_text = open(out0 + ".json").read()
    plain = json.loads(plain_text)
    assert "intrinsics_covariance" not in plain_text and json.dumps(plain, indent=2) == plain_text
    assert list(plain) == list(obj) and list(plain["intrinsics"]) == list(obj["intrinsics"])
    assert np.allclose(list(plain["intrinsics"].values()), list(obj["intrinsics"].values()), rtol=1e-6, atol=1e-9)
    # the written object against the calibrator that wrote it: std_dev = sqrt(variance_factor diag), to the bit
    out2 = str(tmp_path / "cov2")
    cal2 = APP.calibrate_camera_from_json(sc, ds["model_name"], grid_size=0.02, output_path=out2, estimate_covariance=True)
    cov2 = json.load(open(out2 + ".json"))["intrinsics_covariance"]
    c2 = cal2.covariance_
    assert cov2["variance_factor"] == c2["info"]["variance_factor"] and cov2["rcond"] == c2["info"]["rcond"]
    assert cov2["std_dev"] == [float(x) for x in np.sqrt(c2["info"]["variance_factor"] * np.diag(c2["intrinsics"]))]


def test_pose_estimator_covariances_and_application(tmp_path):
    import test_ba_applications as T
    from openimucameracalibrator_amd import estimate_camera_poses_from_checkerboard as APP2, io_files
    ds = dataset("gopro9_division", 45)
    sc = T.scene_of(ds)
    res = APP2.estimate_poses_from_json(sc, ds["model"], ds["intrinsics"], ds["height"], estimate_covariance=True)
    t_s, pose, points, err, sd = res
    assert sd.shape == (len(t_s), 6) and np.all(sd > 0) and np.all(np.isfinite(sd))
    # EstimatePoseCovariances is the a = 0 case: the inverse of every frame's 6 x 6 block
    pe = CC.PoseEstimator()
    pe.EstimatePosesFromJson(sc, ds["model"], ds["intrinsics"], ds["height"])
    cov = pe.EstimatePoseCovariances()
    assert cov.shape == (len(pe.views.pose), 6, 6) and pe.pose_covariance_info_["a"] == 0
    _, H, _ = pe.ba.Evaluate(POSE, 0)
    check_block_inverses(cov, H, 6)
    p0, p1 = str(tmp_path / "p0.json"), str(tmp_path / "p1.json")
    io_files.write_pose_dataset(p0, t_s, pose, points)
    io_files.write_pose_dataset(p1, t_s, pose, points, pose_std_dev=sd)
    obj = json.load(open(p1))
    for v in obj["views"].values():
        assert len(v.pop("position_std_dev")) == 3 and len(v.pop("angle_axis_std_dev")) == 3
    assert json.dumps(obj) == open(p0).read()


def test_cpp_programs_take_the_flag(tmp_path):
    """The C++ applications with --estimate_covariance: the same object as the Python application writes (the intrinsics agree to
    the tolerance of tests/test_cli.py, so the standard deviations are compared to 1e-4 relative), and the per-view standard
    deviations in the pose data set; without the flag neither appears."""
    import os
    import subprocess
    import test_ba_applications as T
    from openimucameracalibrator_amd import calibrate_camera as APP, io_files
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "openimucameracalibrator_amd", "csrc")
    ds = dataset("gopro9_division", 45)
    sc = T.scene_of(ds)
    corners = str(tmp_path / "corners.uson")
    open(corners, "wb").write(io_files.ubjson_encode(sc))
    out = str(tmp_path / "cpp")
    r = subprocess.run([os.path.join(csrc, "calibrate_camera"), "--input_corners=" + corners, "--camera_model_to_calibrate=" + ds["model_name"],
                        "--grid_size=0.02", "--save_path_calib_dataset=" + out, "--estimate_covariance"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "focal_length: " in r.stdout and " +- " in r.stdout and "Largest correlation: " in r.stdout
    cov = json.load(open(out + ".json"))["intrinsics_covariance"]
    cal = APP.calibrate_camera_from_json(sc, ds["model_name"], grid_size=0.02, estimate_covariance=True)
    ref = cal.GetIntrinsicsCovarianceObject()
    assert cov["parameters"] == ref["parameters"]
    assert np.allclose(cov["std_dev"], ref["std_dev"], rtol=1e-4, atol=0) and np.allclose(cov["correlation"], ref["correlation"], rtol=0, atol=1e-4)
    assert abs(cov["variance_factor"] - ref["variance_factor"]) <= 1e-4 * ref["variance_factor"]
    calib = out + ".json"
    poses = []
    for flag in ([], ["--estimate_covariance"]):
        p = str(tmp_path / ("poses%d.json" % len(flag)))
        r = subprocess.run([os.path.join(csrc, "estimate_camera_poses_from_checkerboard"), "--input_corners=" + corners, "--camera_calibration_json=" + calib,
                            "--output_pose_dataset=" + p] + flag, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr + r.stdout
        poses.append(json.load(open(p)))
    assert all("position_std_dev" not in v for v in poses[0]["views"].values())
    assert len(poses[1]["views"]) == len(poses[0]["views"]) > 40
    for v in poses[1]["views"].values():
        sd = np.array(v["position_std_dev"] + v["angle_axis_std_dev"])
        assert sd.shape == (6,) and np.all(sd > 0) and np.all(sd < 0.05)      # sub-millimetre to millimetres, milliradians
