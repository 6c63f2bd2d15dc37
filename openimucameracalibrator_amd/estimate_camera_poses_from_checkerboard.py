"""Twin of the reference application `estimate_camera_poses_from_checkerboard`
(applications/estimate_camera_poses_from_checkerboard.cc:33-78 + PoseEstimator::EstimatePosesFromJson,
src/core/pose_estimator.cc:92-190, FilterBadPoses :238-261): camera poses of every frame of a corner file for a
calibrated camera -- the pose data set continuous_time_imu_to_camera_calibration reads.

    python -m openimucameracalibrator_amd.estimate_camera_poses_from_checkerboard --input_corners=corners.uson \
        --camera_calibration_json=cam_calib.json --output_pose_dataset=out/pose_dataset.json

As in the reference the corners are taken to the normalised image plane and a PINHOLE camera with f = 1, c = 0 is
adjusted (pose_estimator.cc:130-150).  The per-view start pose comes from planar_init.py instead of Theia's RANSAC PnP
[EXT] -- over every corner by default; with --robust_init over the inliers of the RANSAC of robust_init.py (all frames in
one launch on the device, --ransac_hypotheses per frame), which alone become observations as in the reference; the per-view bundle adjustment (BundleAdjustView, Huber 1.345) of ALL views is one kernel launch on the device
(oicc_ba_optimize_views).  Output: the JSON twin of the Theia archive + `<out>.ply`."""
import argparse
import sys

import numpy as np

from . import camera_calibrator as CC
from . import io_files


def estimate_poses_from_json(scene, model, intrinsics, image_height, device=0, backend=None, min_num_points=8, optimize_board_points=False,
                             robust_init=False, ransac_backend=None, ransac_hypotheses=256, estimate_covariance=False):
    """applications/estimate_camera_poses_from_checkerboard.cc:55-70: EstimatePosesFromJson, optionally OptimizeBoardPoints +
    OptimizeAllPoses, FilterBadPoses, GetPoseDataset.  Returns (t_s, pose6, points, per-view mean reprojection error [px]);
    with estimate_covariance a fifth entry, the [n, 6] standard deviations of the kept poses (position | angle axis; None
    when the estimate is rank deficient, which is reported and fails nothing)."""
    pe = CC.PoseEstimator(device=device, backend=backend)
    pe.EstimatePosesFromJson(scene, model, intrinsics, image_height, min_num_points=min_num_points, robust_init=robust_init,
                             ransac_backend=ransac_backend, ransac_hypotheses=ransac_hypotheses)
    if optimize_board_points and pe.views.pose:
        pe.OptimizeBoardPoints()
        if hasattr(pe.ba.b, "point_covariances"):
            pe.PrintBoardPointCovariances()   # pose_estimator.cc:212-223
        else:   # a backend other than liboicc_hip (the test suite's CPU checker) has no such entry
            print("Board point covariances: not available from this backend, not printed")
        pe.OptimizeAllPoses()
    err = pe.FilterBadPoses()
    t_s, pose, points = pe.GetPoseDataset()
    if estimate_covariance:
        sd = pe.GetPoseStdDevs() if pe.views.pose else None
        info = getattr(pe, "pose_covariance_info_", None)
        if sd is None and info is not None:
            print("Pose covariance estimate: %s (rcond %.3e), no standard deviations written" % (CC.COV_STATUS_NAMES.get(info["status"], info["status"]), info["rcond"]))
        return t_s, pose, points, err, sd
    return t_s, pose, points, err


def make_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--input_corners", required=True)
    ap.add_argument("--camera_calibration_json", required=True)
    ap.add_argument("--output_pose_dataset", required=True)
    ap.add_argument("--optimize_board_points", nargs="?", const="true", default="false")
    ap.add_argument("--robust_init", nargs="?", const="true", default="false")
    ap.add_argument("--ransac_hypotheses", type=int, default=256)
    ap.add_argument("--estimate_covariance", nargs="?", const="true", default="false")
    return ap


def main(argv=None):
    a = io_files.parse_reference_flags(make_parser(), argv)
    scene = io_files.read_scene_bson(a.input_corners)
    model, intr, w, h, _ = io_files.read_camera_calibration(a.camera_calibration_json)
    want_cov = str(a.estimate_covariance).lower() in ("1", "true", "yes", "")
    res = estimate_poses_from_json(scene, model, intr, h,
                                   optimize_board_points=str(a.optimize_board_points).lower() in ("1", "true", "yes", ""),
                                   robust_init=str(a.robust_init).lower() in ("1", "true", "yes", ""),
                                   ransac_hypotheses=a.ransac_hypotheses, estimate_covariance=want_cov)
    t_s, pose, points, err = res[:4]
    sd = res[4] if want_cov else None
    print("Estimated %d camera poses, mean reprojection error %.4f px" % (len(t_s), float(np.mean(err)) if len(err) else float("nan")))
    io_files.write_pose_dataset(a.output_pose_dataset, t_s, pose, points, sorted(io_files.scene_points(scene)), pose_std_dev=sd)
    io_files.write_ply_cameras(a.output_pose_dataset + ".ply", pose, points)
    return 0


if __name__ == "__main__":
    sys.exit(main())
