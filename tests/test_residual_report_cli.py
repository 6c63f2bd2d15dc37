"""continuous_time_imu_to_camera_calibration --gate_corners_sigmas / --residual_report_json (csrc/host): parsed without a GPU under
--dry_run; on the GPU the report file, the two extra keys of the result and, without the flags, the result of today."""
import json
import os
import subprocess

import numpy as np
import pytest

from openimucameracalibrator_amd import synthetic, io_files, estimator as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "openimucameracalibrator_amd", "csrc", "continuous_time_imu_to_camera_calibration")


def run_cli(flags, *extra):
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-C", os.path.dirname(CLI), "-s"])
    return subprocess.run([CLI] + ["--%s=%s" % kv for kv in flags.items()] + list(extra), capture_output=True, text=True)


def test_the_two_flags_are_parsed(tmp_path):
    ds = synthetic.make_config("tiny")
    flags = io_files.write_dataset_files(ds, str(tmp_path))
    r = run_cli(flags, "--dry_run", "--gate_corners_sigmas=5", "--residual_report_json=" + str(tmp_path / "report.json"))
    assert r.returncode == 0, r.stderr
    assert not (tmp_path / "report.json").exists()       # a dry run solves and reports nothing
    r = run_cli(flags, "--dry_run", "--gate_corners_sigmas", "4.5", "--residual_report_json", str(tmp_path / "report.json"))
    assert r.returncode == 0, r.stderr
    assert run_cli(flags, "--dry_run", "--gate_corners_sigmas=5", "--not_a_flag").returncode == 2
    assert run_cli(flags, "--dry_run", "--gate_corner_sigmas=5").returncode == 2


@pytest.mark.gpu
def test_gated_calibration_writes_the_report_and_the_two_keys(tmp_path):
    ds = synthetic.make_config("C1", camera="gopro9_division")
    rng = np.random.RandomState(7)
    bad = rng.permutation(ds.num_corners)[:12]
    ds.corner_uv = ds.corner_uv.copy(); ds.corner_uv[bad] += 25.0 * np.array([0.6, -0.8])
    flags = io_files.write_dataset_files(ds, str(tmp_path))
    report = str(tmp_path / "report.json")
    r = run_cli(flags, "--known_grav_dir_axis=UNKNOWN", "--gate_corners_sigmas=5", "--residual_report_json=" + report)
    assert r.returncode == 0, r.stderr + r.stdout
    out = json.load(open(flags["result_output_json"]))
    rep = json.load(open(report))
    # the Python mirror through the same steps
    cal = E.ImuCameraCalibrator().BatchInitSpline(ds)
    cal.trajectory_.UseReferenceSolverOptions()
    cal.OptimizeGated(50, E.SPLINE | E.T_I_C | E.GRAVITY_DIR, 5.0)
    info = cal.trajectory_.ResidualReport()
    views = cal.trajectory_.GetViewErrors()
    assert len(rep["views"]) == int(cal.views_accepted.sum()) == len(views["n_used"])
    assert set(rep["views"][0]) == {"timestamp", "n_used", "rms_px", "max_px"}
    # the application adds the views in the string order of the corner file's keys; the report lists them in that order
    order = ds.file_key_order()
    assert np.allclose([v["timestamp"] for v in rep["views"]], ds.view_t_s[order], atol=2e-6)
    assert [v["n_used"] for v in rep["views"]] == [int(x) for x in views["n_used"][order]]
    assert sum(v["n_used"] for v in rep["views"]) == rep["corners"]["used"] == ds.num_corners - out["gated_corners"]
    assert np.abs(np.array([v["rms_px"] for v in rep["views"]]) - views["rms_px"][order]).max() < 1e-2
    assert 12 <= out["gated_corners"] == rep["corners"]["gated"] <= 12 + 0.01 * ds.num_corners
    assert out["gated_corners"] == cal.gated_corners
    assert abs(out["corner_sigma_px"] - cal.gate_report["sigma_px"]) < 1e-2
    for key in ("accl_rms", "accl_rms_weighted", "gyro_rms", "gyro_rms_weighted"):
        assert np.abs(np.array([rep["imu"][key][c] for c in "xyz"]) - np.array(info[key])).max() < 1e-2 * max(info[key])
    T = cal.trajectory_.GetT_i_c()
    q = np.array([out["q_i_c"][c] for c in "xyzw"])
    assert min(np.abs(q - T[:4]).max(), np.abs(q + T[:4]).max()) < 1e-4


@pytest.mark.gpu
def test_without_the_flags_the_result_is_todays(tmp_path):
    ds = synthetic.make_config("C1", camera="gopro9_division")
    flags = io_files.write_dataset_files(ds, str(tmp_path))
    r = run_cli(flags, "--known_grav_dir_axis=UNKNOWN")
    assert r.returncode == 0, r.stderr + r.stdout
    out = json.load(open(flags["result_output_json"]))
    assert set(out) == {"q_i_c", "t_i_c", "final_reproj_error", "r3_dt", "so3_dt", "init_line_delay_us", "calib_line_delay_us", "time_offset_imu_to_cam_s", "trajectory"}
    cal = E.ImuCameraCalibrator().BatchInitSpline(ds)
    cal.trajectory_.UseReferenceSolverOptions()
    cal.Optimize(50, E.SPLINE | E.T_I_C | E.GRAVITY_DIR)
    T = cal.trajectory_.GetT_i_c()
    q = np.array([out["q_i_c"][c] for c in "xyzw"]); t = np.array([out["t_i_c"][c] for c in "xyz"])
    assert min(np.abs(q - T[:4]).max(), np.abs(q + T[:4]).max()) < 1e-4
    assert np.abs(t - T[4:]).max() < 1e-3
    assert abs(out["final_reproj_error"] - cal.trajectory_.GetMeanReprojectionError()) < 1e-2
    assert len(out["trajectory"]) == int(cal.gyro_accepted.sum())
