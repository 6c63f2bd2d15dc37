"""The two stabilize_frames programs (csrc/host/stabilize_frames.cpp and python -m openimucameracalibrator_amd.stabilize_frames) on
the files of the rectify_rolling_shutter program test: identical PNGs and plan files, equal to the library called from Python."""
import json
import os
import sys

import numpy as np
import pytest

import rolling_shutter_cases as K
import test_gpu_rolling_shutter as T
from openimucameracalibrator_amd import camera_maps as cm
from openimucameracalibrator_amd import rolling_shutter as rs
from openimucameracalibrator_amd import stabilization as stab
from openimucameracalibrator_amd import synthetic as S

pytestmark = pytest.mark.gpu

PROGRAMS = (("cpp", [os.path.join(T.CSRC, "stabilize_frames")]), ("py", [sys.executable, "-m", "openimucameracalibrator_amd.stabilize_frames"]))
NAMES = ["990000000.png", "1040000000.png", "1100000000.png", "1900000000.png"]        # by time; as text the first one sorts last


@pytest.mark.parametrize("mode", ("fixed", "dynamic"))
def test_stabilize_frames_programs_write_identical_pngs_and_plans(tmp_path, mode):
    from PIL import Image
    from openimucameracalibrator_amd import stabilize_frames as prog
    flags, views = T._program_inputs(tmp_path)
    Image.fromarray(views["images"][1]).save(os.path.join(flags[1], NAMES[0]))           # 2.99 s: before the telemetry
    extra = ["--balance", "0.25", "--smoothing_s", "0.08", "--max_correction_deg", "2.5", "--zoom_mode", mode, "--zoom_window_s", "0.05", "--max_zoom", "3"]
    outs, plans = {}, {}
    for tag, cmd in PROGRAMS:
        out = tmp_path / ("out_" + tag)
        plan = str(tmp_path / ("plan_%s.json" % tag))
        r = T._run(cmd + flags + extra + ["--output_path", str(out), "--output_plan_json", plan])
        assert r.returncode == 0, r.stdout + r.stderr
        assert sorted(os.listdir(str(out))) == ["1040000000.png", "1100000000.png"]                  # the uncovered frames are not written
        assert "skipped 1900000000.png: no gyro coverage" in r.stderr and "skipped 990000000.png: no gyro coverage" in r.stderr
        assert "stabilised 2 of 4 frames" in r.stdout
        outs[tag] = {n: np.asarray(Image.open(str(out / n))) for n in NAMES[1:3]}
        plans[tag] = open(plan).read()
    assert plans["cpp"] == plans["py"]
    for n in NAMES[1:3]:
        assert outs["cpp"][n].shape == outs["py"][n].shape and np.array_equal(outs["cpp"][n], outs["py"][n]), n
    assert outs["cpp"][NAMES[1]].ndim == 2 and outs["cpp"][NAMES[2]].shape[2] == 3
    doc = json.loads(plans["py"])["frames"]
    assert [f["name"] for f in doc] == NAMES and [f["status"] for f in doc] == [1, 0, 0, 1]
    # the plan and the first covered frame through the library, from the same files
    model, intr, w, h = S.CAMERAS["gopro9_division"]
    telemetry = json.load(open(flags[3]))
    gyro_t, rates = rs.corrected_gyro(telemetry, *prog.read_gyro_intrinsics(flags[9], flags[11]))
    dst = (S.CAM_PINHOLE, cm.rectified_pinhole(model, intr, w, h, 0.25), w, h)
    times = [prog.frame_time_from_name(n, 2000000000.0 * 1e-9) for n in NAMES]
    scene = lambda t: rs.Scene((model, intr, w, h), dst, gyro_t, rates, t, 30.0 * 1e-6, q_i_c=K.Q_I_C, time_offset_imu_to_cam=0.004)
    p = stab.stab_plan(scene(times), stab.StabOptions(0.08, 2.5 * np.pi / 180.0, mode, 0.05, 3.0))
    assert prog.plan_json(NAMES, p.frame_status, p.correction_q, p.required_zoom, p.zoom, p.zoom_clamped) == plans["py"]
    assert np.abs(p.correction_q[1:3, 1:]).max() > 1e-4                                 # the two covered frames are corrected
    expect, status = stab.stab_frames(views["images"][:1], scene(times[1:2]), p.correction_q[1:2], p.zoom[1:2])
    assert list(status) == [0]
    assert np.array_equal(outs["py"][NAMES[1]], expect[0])
    assert not np.array_equal(expect[0], views["images"][0])


def test_stabilize_frames_programs_reject_an_unknown_zoom_mode_and_flag(tmp_path):
    flags, _ = T._program_inputs(tmp_path)
    good = flags + ["--output_path", str(tmp_path / "o")]
    for tag, cmd in PROGRAMS:
        assert T._run(cmd + good + ["--zoom_mode", "sometimes"]).returncode != 0
        assert T._run(cmd + good + ["--no_such_flag", "1"]).returncode != 0
        assert T._run(cmd + good + ["--max_zoom", "0.5"]).returncode != 0
        assert not os.path.exists(str(tmp_path / "o")) or not os.listdir(str(tmp_path / "o"))
