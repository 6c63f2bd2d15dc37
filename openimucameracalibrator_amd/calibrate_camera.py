"""Twin of the reference application `calibrate_camera` (applications/calibrate_camera.cc:27-63 +
CameraCalibrator::CalibrateCameraFromJson, src/core/camera_calibrator.cc:221-377): camera intrinsics from a corner file.

    python -m openimucameracalibrator_amd.calibrate_camera --input_corners=corners.uson \
        --camera_model_to_calibrate=DIVISION_UNDISTORTION --save_path_calib_dataset=out/cam_calib [--grid_size=0.04] [--verbose] [--estimate_covariance]

Same flags, same input (the UBJSON corner file of extract_board_to_json) and the same calibration JSON keys
(src/io/write_camera_calibration.cc).  Differences, all outside the bundle adjustment: the per-view start values come
from planar_init.py (closed forms for a planar board) instead of Theia's RANSAC solvers [EXT] -- over every corner by
default, with --robust_init over the inliers of the RANSAC of robust_init.py (all views in one launch on the device;
--ransac_hypotheses per view), which alone become observations; the start focal length is the median over the views; `<out>.calibdata` is written as the JSON twin of the Theia archive.  The three
BundleAdjustViews stages and the view filters of RunCalibration run on the device (oicc_ba_*)."""
import argparse
import sys

from . import camera_calibrator as CC
from . import io_files


def str2bool(v):
    return str(v).lower() in ("1", "true", "yes", "on", "")


def calibrate_camera_from_json(scene, camera_model, grid_size=0.04, output_path="", verbose=False, device=0, backend=None,
                               optimize_board_points=False, robust_init=False, ransac_backend=None, ransac_hypotheses=256,
                               estimate_covariance=False):
    """applications/calibrate_camera.cc:50-59: CameraCalibrator(model, optimize_board_points), SetGridSize, SetVerbose,
    CalibrateCameraFromJson.  Returns the CameraCalibrator (or None on failure).  robust_init: see
    CameraCalibrator.CalibrateCameraFromJson; ransac_backend None = the HIP library.  estimate_covariance: one line per
    variable intrinsic (value +- sigma), the largest correlation, and the `intrinsics_covariance` object in the calibration JSON."""
    cal = CC.CameraCalibrator(camera_model, optimize_board_pts=optimize_board_points, device=device, backend=backend)
    cal.SetGridSize(grid_size)
    if verbose:
        cal.SetVerbose()
    ok = cal.CalibrateCameraFromJson(scene, output_path, robust_init=robust_init, ransac_backend=ransac_backend,
                                     ransac_hypotheses=ransac_hypotheses, estimate_covariance=estimate_covariance)
    return cal if ok else None


def make_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--input_corners", required=True)
    ap.add_argument("--camera_model_to_calibrate", default="DOUBLE_SPHERE")
    ap.add_argument("--save_path_calib_dataset", default="")
    ap.add_argument("--grid_size", type=float, default=0.04)
    ap.add_argument("--optimize_board_points", type=str2bool, nargs="?", const=True, default=False)
    ap.add_argument("--verbose", type=str2bool, nargs="?", const=True, default=False)
    ap.add_argument("--robust_init", type=str2bool, nargs="?", const=True, default=False)
    ap.add_argument("--ransac_hypotheses", type=int, default=256)
    ap.add_argument("--estimate_covariance", type=str2bool, nargs="?", const=True, default=False)
    return ap


def main(argv=None):
    a = io_files.parse_reference_flags(make_parser(), argv)
    scene = io_files.read_scene_bson(a.input_corners)
    cal = calibrate_camera_from_json(scene, a.camera_model_to_calibrate, a.grid_size, a.save_path_calib_dataset, a.verbose,
                                     optimize_board_points=a.optimize_board_points, robust_init=a.robust_init,
                                     ransac_hypotheses=a.ransac_hypotheses, estimate_covariance=a.estimate_covariance)
    if cal is None:
        return 1
    cal.PrintResult()
    return 0


if __name__ == "__main__":
    sys.exit(main())
