"""oicc_ba_point_covariances: the covariances of the refined board points (ceres::Covariance after theia::BundleAdjustTracks,
pose_estimator.cc:193-223) against the inverse of the 3 x 3 diagonal blocks of oicc_ba_evaluate's J^T J."""
import contextlib
import io
import os
import subprocess

import numpy as np
import pytest

from openimucameracalibrator_amd import camera_calibrator as CC, io_files

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)


def _adjuster(variable=None):
    ds = CC.make_calibration_dataset("pinhole", num_views=45, corners_per_view=40, noise_px=0.05)
    ba = CC.ViewBundleAdjuster()
    ba.SetCamera(ds["model"], ds["intrinsics"]); ba.SetScenePoints(ds["points"])
    ba.SetViews(ds["pose_init"], ds["corner_offset"], ds["uv"], ds["point_ids"])
    if variable is not None:
        ba.SetVariablePoints(variable)
    return ds, ba


def test_point_covariances_are_the_inverse_diagonal_blocks():
    ds, ba = _adjuster()
    n = len(ds["points"])
    variable = np.ones(n, np.uint8); variable[[1, 7, n - 1]] = 0      # constant points at the start, inside and at the end
    ba.SetVariablePoints(variable)
    ba.Optimize(5, CC.BA_POINTS, 0)
    cost, H, _ = ba.Evaluate(CC.BA_POINTS, 0)
    cov, vf = ba.PointCovariances()
    assert cov.shape == (n, 3, 3) and H.shape == (3 * (n - 3), 3 * (n - 3))
    t, worst = 0, 0.0
    for i in range(n):
        if not variable[i]:
            assert np.all(np.isnan(cov[i])), i
            continue
        blk = H[t:t + 3, t:t + 3].astype(np.longdouble); t += 3
        # the 3 x 3 inverse in longdouble by the adjugate
        c = np.array([[blk[(r + 1) % 3, (q + 1) % 3] * blk[(r + 2) % 3, (q + 2) % 3] - blk[(r + 1) % 3, (q + 2) % 3] * blk[(r + 2) % 3, (q + 1) % 3]
                       for r in range(3)] for q in range(3)], dtype=np.longdouble)
        inv = c / (blk[0] @ c[:, 0])
        kappa = float(np.abs(blk).sum(axis=0).max() * np.abs(inv).sum(axis=0).max())
        err = float(np.abs(cov[i] - inv).max() / np.abs(inv).max())
        worst = max(worst, err / (kappa * EPS))
        assert err <= 100 * kappa * EPS, (i, err, kappa)
        assert np.array_equal(cov[i], cov[i].T) and np.all(np.diag(cov[i]) > 0)
    print("MARGIN board point covariances: largest error / (kappa eps) %.3e (bound 100)" % worst)
    m = 2 * len(ds["uv"])
    assert abs(vf - 2 * cost / (m - 3 * (n - 3))) <= 1e-14 * vf


def test_pose_estimation_program_prints_the_reference_lines(tmp_path):
    """estimate_camera_poses_from_checkerboard --optimize_board_points: the three kinds of line of pose_estimator.cc:212-223, from
    the Python program and from the C++ one."""
    import test_ba_applications as T
    from openimucameracalibrator_amd import estimate_camera_poses_from_checkerboard as APP2
    ds = CC.make_calibration_dataset("pinhole", num_views=45, corners_per_view=40, noise_px=0.05)
    sc = T.scene_of(ds)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        APP2.estimate_poses_from_json(sc, ds["model"], ds["intrinsics"], ds["height"], optimize_board_points=True)
    out = buf.getvalue()
    assert "Empirical variance factor after board point optimization: " in out
    assert "Mean board point standard deviation after optimization: " in out and " mm" in out
    assert out.count("Track Id: ") >= 1
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "openimucameracalibrator_amd", "csrc")
    corners = str(tmp_path / "corners.uson")
    open(corners, "wb").write(io_files.ubjson_encode(sc))
    calib = str(tmp_path / "calib.json")
    io_files.write_camera_calibration(calib, ds["model"], ds["intrinsics"], ds["width"], ds["height"], 30.0, len(ds["pose_true"]), 0.1)
    r = subprocess.run([os.path.join(csrc, "estimate_camera_poses_from_checkerboard"), "--input_corners=" + corners, "--camera_calibration_json=" + calib,
                        "--output_pose_dataset=" + str(tmp_path / "poses.json"), "--optimize_board_points"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "Empirical variance factor after board point optimization: " in r.stdout
    assert "Mean board point standard deviation after optimization: " in r.stdout
    assert r.stdout.count("Track Id: ") == out.count("Track Id: ")
