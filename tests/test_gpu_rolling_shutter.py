"""The rolling-shutter rectification on the device (csrc/rolling_shutter.hip) against its numpy specification
tests/rolling_shutter_restatement.py.

The yardstick of a case is the distance of the float64 restatement from its numpy.longdouble run; the device may be ten times that
away from the float64 restatement.  Map coordinates are float32: one float32 ulp is added.  Both figures are printed (DESIGN.md,
"Rolling-shutter rectification", holds the measured ones).  Frames are byte-identical to remapping through the device's own maps:
the same fixed point, the same float32 rounding, the same bilinear tap."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import camera_maps_restatement as R
import rolling_shutter_cases as K
import rolling_shutter_restatement as RS
from openimucameracalibrator_amd import camera_maps as cm
from openimucameracalibrator_amd import rolling_shutter as rs
from openimucameracalibrator_amd import synthetic as S

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- rotations and frame status
def _rotation_queries(sc, n, seed=2):
    rng = np.random.RandomState(seed)
    frames = rng.randint(0, len(sc.frame_t), n)
    rows = np.concatenate([[0.0, sc.src[3] - 1.0, sc.reference_row, 100.0], rng.uniform(0, sc.src[3] - 1, 61)])[:n]
    if n > len(rows):
        rows = np.concatenate([rows, rng.uniform(0, sc.src[3] - 1, n - len(rows))])
    return frames.astype(np.int32), rows


ROTATION_CASES = [("plain", n) for n in (1, 63, 64, 65)] + [(k, 65) for k in ("inside-one-interval", "row-on-a-sample", "negative-delay",
                                                                               "zero-delay", "window-256", "window-257", "uncovered")]


@pytest.mark.parametrize("kind,n", ROTATION_CASES, ids=lambda v: str(v))
def test_row_rotations_and_frame_status_against_restatement(kind, n):
    kw = K.rotation_scene_args(kind)
    sc = RS.Scene(**kw)
    frames, rows = _rotation_queries(sc, n)
    ref, ref_status, ref_frames = RS.row_rotations(sc, frames, rows)
    ext = RS.row_rotations(sc, frames, rows, dtype=np.longdouble)[0]
    q, status, frame_status = rs.rs_row_rotations(rs.Scene(**kw), frames, rows)
    assert np.array_equal(frame_status, ref_frames)
    assert np.array_equal(status, ref_status)
    expected = {"uncovered": [1, 0, 1], "window-256": [0], "window-257": [2]}.get(kind)
    if expected is not None:
        assert list(frame_status) == expected
    good = status == 0
    assert np.all(np.isnan(q[~good]))
    if not good.any():
        return
    yardstick = float(K.quaternion_angle(ref[good], ext[good]).max())
    distance = float(K.quaternion_angle(ref[good], q[good]).max())
    print("rotations %s n=%d: yardstick (float64 vs longdouble) %.3e rad, device vs float64 %.3e rad" % (kind, n, yardstick, distance))
    assert distance <= 10.0 * yardstick
    assert np.abs(np.linalg.norm(q[good], axis=1) - 1.0).max() <= 1e-13


# ---------------------------------------------------------------- maps
@pytest.mark.parametrize("frames", (1, 3))
@pytest.mark.parametrize("size", K.MAP_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("case", K.MAP_CASES)
def test_map_against_restatement(case, size, frames):
    ref_map, ref_valid, ref_status, _, raw, _ = [a[:frames] for a in K.map_reference(case, size)]
    kw = K.scene_args(case, size, frames=frames)
    sw, sh = kw["src"][2:]
    dw, dh = size
    mapxy, valid, status, num_valid, evals = rs.rs_rectify_map(rs.Scene(**kw), return_evaluations=True)
    assert mapxy.shape == (frames, dh, dw, 2) and mapxy.dtype == np.float32 and valid.shape == (frames, dh, dw)
    assert np.array_equal(status, ref_status) and np.all(status == 0)
    assert np.array_equal(num_valid, valid.reshape(frames, -1).sum(1))
    flagged = K.near_border(raw, sw, sh)
    assert flagged.sum() <= 1e-3 * flagged.size
    assert np.array_equal(valid[~flagged], ref_valid[~flagged])
    assert np.all(np.isnan(mapxy[valid == 0]))
    assert evals.max() <= 20
    both = (valid == 1) & (ref_valid == 1)
    assert both.any()
    yardstick = K.map_yardstick(case, size)["px"]
    diff = np.abs(mapxy[both].astype(np.float64) - ref_map[both].astype(np.float64))
    ulp = np.spacing(np.abs(ref_map[both])).astype(np.float64)
    print("map %s %dx%d x %d: valid %s, worst |device - restatement| %.3e px, double yardstick %.3e px, evaluations mean %.2f max %d" % (
        case, dw, dh, frames, list(num_valid), diff.max(), yardstick, evals[valid == 1].mean(), evals.max()))
    assert np.all(diff <= ulp + 10.0 * yardstick)


@pytest.mark.parametrize("case", K.MAP_CASES)
def test_zero_rates_give_the_static_map_bit_for_bit(case):
    for size in ((67, 5), (960, 540)):
        kw = K.scene_args(case, size, rates_scale=0.0)
        (sm, si, sw, sh), (dm, di, dw, dh) = kw["src"], kw["dst"]
        mapxy, valid, status, num_valid = rs.rs_rectify_map(rs.Scene(**kw))
        static_map, static_valid, static_num = cm.rectify_map(sm, si, sw, sh, dm, di, dw, dh)
        assert np.all(status == 0)
        for k in range(3):
            assert np.array_equal(mapxy[k].view(np.uint32), static_map.view(np.uint32)), (size, k)
            assert np.array_equal(valid[k], static_valid) and num_valid[k] == static_num


# ---------------------------------------------------------------- frames
def _frames_scene(num_frames, size=(67, 5)):
    """The pinhole case with `num_frames` frames; with five, the second lies before the telemetry (status 1): at batch 2 it sits
    inside the first batch, behind a covered frame."""
    kw = K.scene_args("pinhole", size)
    times = [K.FRAME_TIMES[0], -0.5, K.FRAME_TIMES[1], K.FRAME_TIMES[2], 0.1][:num_frames]
    kw["frame_t"] = K.T_BASE + np.array(times)
    return kw


def _random_frames(num_frames, channels, seed=0):
    rng = np.random.RandomState(seed + 10 * num_frames + channels)
    return rng.randint(0, 256, (num_frames, 540, 960) if channels == 1 else (num_frames, 540, 960, channels)).astype(np.uint8)


# (frames, batch) beside the five frames at batch 2: both slots recycled more than once; no short batch; one slot alone, the
# batch as long as the frames and longer.  The first `frames` of the five frames, held to the batch-2 result byte for byte.
OTHER_BATCHES = ((3, 1), (4, 2), (5, 5), (5, 8))


def _check_report(rep):
    parts = [rep[k] for k in ("ms_table", "ms_rays", "ms_upload", "ms_kernel", "ms_download")]
    assert all(np.isfinite(v) and v >= 0 for v in parts + [rep["ms_total"]]), rep
    assert all(rep["ms_total"] >= v for v in parts), rep


@pytest.mark.parametrize("border", (0, 255))
@pytest.mark.parametrize("num_frames", (1, 5))
@pytest.mark.parametrize("channels", (1, 3))
def test_frames_are_byte_identical_to_remapping_through_the_maps(channels, num_frames, border):
    for size in ((67, 5), (240, 135)):
        kw = _frames_scene(num_frames, size)
        scene = rs.Scene(**kw)
        F = _random_frames(num_frames, channels)
        rep = {}
        out, status = rs.rs_rectify_frames(F, scene, border_value=border, batch=2, report=rep)     # 5 frames: three batches, the last one short
        mapxy, valid, map_status, _ = rs.rs_rectify_map(scene)
        assert np.array_equal(status, map_status)
        assert list(status) == [0, 1, 0, 0, 0][:num_frames]
        assert out.dtype == np.uint8 and out.shape == (num_frames, size[1], size[0]) + (() if channels == 1 else (3,))
        for k in range(num_frames):
            expect = cm.remap(F[k:k + 1], mapxy[k], border_value=border)[0]
            assert np.array_equal(out[k], expect), (size, k)
            if status[k] != 0:
                assert np.all(out[k] == border) and not valid[k].any()
        assert valid[0].any() and (out[0] != border).any()
        assert rep["ms_total"] > 0 and rep["ms_kernel"] > 0 and rep["ms_table"] > 0
        _check_report(rep)
        for frames, batch in OTHER_BATCHES if num_frames == 5 else ():
            rep = {}
            again, again_status = rs.rs_rectify_frames(F[:frames], rs.Scene(**_frames_scene(frames, size)), border_value=border, batch=batch, report=rep)
            assert np.array_equal(again, out[:frames]) and np.array_equal(again_status, status[:frames]), (size, frames, batch)
            _check_report(rep)


def test_frames_on_a_cuda_tensor_equal_the_host_route():
    import torch
    for channels in (1, 3):
        kw = _frames_scene(5)
        scene = rs.Scene(**kw)
        F = _random_frames(5, channels)
        host, host_status = rs.rs_rectify_frames(F, scene, border_value=17, batch=2)
        t = torch.from_numpy(F).cuda()
        out, status = rs.rs_rectify_frames(t, scene, border_value=17)
        assert isinstance(out, torch.Tensor) and out.is_cuda and out.device == t.device and out.dtype == torch.uint8
        assert np.array_equal(out.cpu().numpy(), host)
        assert np.array_equal(status, host_status)


def test_frames_device_rejects_arrays_that_are_not_on_the_device():
    import ctypes as C
    import torch
    from openimucameracalibrator_amd import _abi
    b = rs._bound()
    scene = rs.Scene(**K.small_scene())
    F = np.zeros((2, 540, 960), np.uint8); out = np.zeros((2, 3, 4), np.uint8); st = np.zeros(2, np.int32)
    t = torch.zeros((2, 540, 960), dtype=torch.uint8, device="cuda"); o = torch.zeros((2, 3, 4), dtype=torch.uint8, device="cuda")
    u8 = lambda x: C.cast(x.data_ptr(), _abi.c_u8p)
    i32 = st.ctypes.data_as(_abi.c_i32p)
    assert b.rectify_frames_device(None, scene.ref(), 1, u8(t), 0, u8(o), i32) == 0
    torch.cuda.synchronize()
    assert b.rectify_frames_device(None, scene.ref(), 1, F.ctypes.data_as(_abi.c_u8p), 0, u8(o), i32) == -1
    assert b.rectify_frames_device(None, scene.ref(), 1, u8(t), 0, out.ctypes.data_as(_abi.c_u8p), i32) == -1


# ---------------------------------------------------------------- points
@pytest.mark.parametrize("n", (1, 64, 257))
@pytest.mark.parametrize("case", K.MAP_CASES)
def test_points_against_restatement(case, n):
    kw = K.scene_args(case, (960, 540))
    sc = RS.Scene(**kw)
    rng = np.random.RandomState(7)
    frames = rng.randint(0, 3, n).astype(np.int32)
    xy = np.concatenate([[[479.5, 269.5], [np.nan, 10.0], [0.0, 0.0], [959.0, 539.0]], rng.uniform([0, 0], [959, 539], (n, 2))])[:n]
    ref, ref_status, _ = RS.rectify_points(sc, frames, xy)
    ext, ext_status, _ = RS.rectify_points(sc, frames, xy, dtype=np.longdouble)
    out, status, frame_status = rs.rs_rectify_points(rs.Scene(**kw), frames, xy)
    assert np.all(frame_status == 0)
    assert np.array_equal(status, ref_status) and np.array_equal(ext_status, ref_status)
    good = status == 0
    assert np.all(np.isnan(out[~good]))
    if n > 1:
        assert status[1] == 1
    yardstick = float(np.abs(np.asarray(ext[good] - ref[good], dtype=np.float64)).max())
    distance = float(np.abs(out[good] - ref[good]).max())
    print("points %s n=%d: yardstick (float64 vs longdouble) %.3e px, device vs float64 %.3e px" % (case, n, yardstick, distance))
    assert distance <= 10.0 * yardstick


@pytest.mark.parametrize("case", K.MAP_CASES)
def test_points_of_the_map_are_the_destination_pixels(case):
    """The map's float32 coordinates fed back: a float32 ulp of 3.1e-5 px below 1024, times a magnification below 3 for these
    cameras, with a factor of ten: 1e-3 px."""
    kw = K.scene_args(case, (960, 540))
    scene = rs.Scene(**kw)
    mapxy, valid, status, _ = rs.rs_rectify_map(scene)
    own = R.pixel_grid(960, 540).reshape(540, 960, 2)
    worst = 0.0
    for k in range(3):
        sel = valid[k] == 1
        back, st, _ = rs.rs_rectify_points(scene, np.full(int(sel.sum()), k, np.int32), mapxy[k][sel].astype(np.float64))
        assert np.all(st == 0)
        worst = max(worst, float(np.abs(back - own[sel]).max()))
    print("points(map) %s: worst distance from the destination pixel %.3e px" % (case, worst))
    assert worst <= 1e-3


def test_points_of_an_uncovered_frame_have_status_2():
    kw = _frames_scene(5)
    out, status, frame_status = rs.rs_rectify_points(rs.Scene(**kw), [0, 1, 4], [[100.0, 100.0]] * 3)
    assert list(frame_status) == [0, 1, 0, 0, 0] and list(status) == [0, 2, 0]
    assert np.all(np.isnan(out[1])) and np.all(np.isfinite(out[[0, 2]]))


# ---------------------------------------------------------------- bad arguments
@pytest.mark.parametrize("name", list(K.BAD_SCENES))
def test_bad_scenes_are_refused(name):
    assert K.call_every_entry(K.bad_scene(name)) == [-1] * 5


def test_bad_frames_and_queries_are_refused():
    scene = rs.Scene(**K.small_scene())
    F = np.zeros((2, 540, 960), np.uint8)
    with pytest.raises(ValueError):
        rs.rs_rectify_frames(F, scene, batch=0)
    with pytest.raises(ValueError):
        rs.rs_rectify_frames(F, scene, border_value=256)
    with pytest.raises(ValueError):
        rs.rs_rectify_frames(np.zeros((2, 540, 960, 2), np.uint8), scene)
    with pytest.raises(ValueError):
        rs.rs_rectify_frames(F[:1], scene)
    with pytest.raises(ValueError):
        rs.rs_rectify_points(scene, [2], [[1.0, 1.0]])             # two frames: index 2 is out of range
    with pytest.raises(ValueError):
        rs.rs_row_rotations(scene, [-1], [1.0])
    with pytest.raises(ValueError):
        rs.rs_row_rotations(scene, [0], [np.nan])
    out, status = rs.rs_rectify_frames(F, scene)
    assert out.shape == (2, 3, 4) and list(status) == [0, 0]


# ---------------------------------------------------------------- programs
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openimucameracalibrator_amd", "csrc")
PROGRAMS = (("cpp", [os.path.join(CSRC, "rectify_rolling_shutter")]), ("py", [sys.executable, "-m", "openimucameracalibrator_amd.rectify_rolling_shutter"]))


def _run(cmd):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600, env=env, cwd=ROOT)


def _program_inputs(tmp_path):
    """Two rendered radon views (gray and RGB) inside the telemetry and one frame behind it; returns the common flags."""
    import camera_maps_cases as CK
    from PIL import Image
    from openimucameracalibrator_amd import io_files
    views = CK.rendered_views()
    src = tmp_path / "in"; src.mkdir()
    rgb = np.stack([views["images"][1], views["images"][1][::-1], 255 - views["images"][1]], -1)
    Image.fromarray(views["images"][0]).save(str(src / "1040000000.png"))
    Image.fromarray(np.ascontiguousarray(rgb)).save(str(src / "1100000000.png"))
    Image.fromarray(views["images"][0]).save(str(src / "1900000000.png"))              # behind the telemetry
    rng = np.random.RandomState(8)
    t_ns = 3000000000 + np.arange(60) * 5000000 + rng.randint(-200000, 200000, 60)      # 3.0 .. 3.3 s, IMU clock
    io_files.write_telemetry_json(str(tmp_path / "telemetry.json"), t_ns, rng.normal(0, 1.0, (60, 3)), rng.normal(0, 3.0, (60, 3)),
                                  img_timestamps_ns=[2000000000])                       # frames at 3.04, 3.10 and 3.90 s, camera clock
    q = K.Q_I_C
    json.dump(dict(q_i_c=dict(w=q[0], x=q[1], y=q[2], z=q[3]), calib_line_delay_us=30.0, time_offset_imu_to_cam_s=0.004),
              open(str(tmp_path / "result.json"), "w"))
    json.dump(dict(accelerometer=dict(misalignment_matrix=[[1, 0, 0], [0, 1, 0], [0, 0, 1]], scale_matrix=[[1, 0, 0], [0, 1, 0], [0, 0, 1]]),
                   gyroscope=dict(misalignment_matrix=[[1, -0.011, 0.012], [0.013, 1, -0.014], [-0.015, 0.016, 1]],
                                  scale_matrix=[[1.001, 0, 0], [0, 0.998, 0], [0, 0, 1.003]])), open(str(tmp_path / "imu_intrinsics.json"), "w"))
    json.dump(dict(accl_bias=dict(x=0.0, y=0.0, z=0.0), gyro_bias=dict(x=0.01, y=-0.02, z=0.03)), open(str(tmp_path / "imu_bias.json"), "w"))
    calib = str(tmp_path / "cam_calib.json")
    model, intr, w, h = S.CAMERAS["gopro9_division"]
    io_files.write_camera_calibration(calib, model, intr, w, h, 60.0, 10, 0.1)
    return ["--input_path", str(src), "--telemetry_json", str(tmp_path / "telemetry.json"), "--camera_calibration_json", calib,
            "--imu_camera_calibration_json", str(tmp_path / "result.json"), "--imu_intrinsics", str(tmp_path / "imu_intrinsics.json"),
            "--imu_bias_file", str(tmp_path / "imu_bias.json")], views


@pytest.mark.parametrize("undistort", (False, True), ids=("same-camera", "undistort"))
def test_rectify_rolling_shutter_programs_write_identical_pngs(tmp_path, undistort):
    from PIL import Image
    from openimucameracalibrator_amd import io_files
    from openimucameracalibrator_amd import rectify_rolling_shutter as prog
    flags, views = _program_inputs(tmp_path)
    extra = ["--undistort", "--balance", "0.25", "--line_delay_us", "28.5"] if undistort else []
    outs = {}
    for tag, cmd in PROGRAMS:
        out = tmp_path / ("out_" + tag)
        cam = str(tmp_path / ("destination_%s.json" % tag))
        r = _run(cmd + flags + extra + ["--output_path", str(out), "--output_camera_json", cam])
        assert r.returncode == 0, r.stdout + r.stderr
        assert sorted(os.listdir(str(out))) == ["1040000000.png", "1100000000.png"]                  # the uncovered frame is not written
        assert "skipped 1900000000.png: no gyro coverage" in r.stderr
        assert "rectified 2 of 3 frames" in r.stdout
        outs[tag] = {n: np.asarray(Image.open(str(out / n))) for n in ("1040000000.png", "1100000000.png")}
        outs[tag + "_cam"] = io_files.read_camera_calibration(cam)
    for n in ("1040000000.png", "1100000000.png"):
        assert outs["cpp"][n].shape == outs["py"][n].shape
        assert np.array_equal(outs["cpp"][n], outs["py"][n]), n
    assert outs["cpp"]["1040000000.png"].ndim == 2 and outs["cpp"]["1100000000.png"].shape[2] == 3
    assert outs["cpp_cam"][0] == outs["py_cam"][0] == (S.CAM_PINHOLE if undistort else S.CAMERAS["gopro9_division"][0])
    assert np.allclose(outs["cpp_cam"][1], outs["py_cam"][1], rtol=1e-12, atol=0)
    # the first frame through the library, from the same files
    model, intr, w, h = S.CAMERAS["gopro9_division"]
    telemetry = json.load(open(flags[3]))
    gyro_t, rates = rs.corrected_gyro(telemetry, *prog.read_gyro_intrinsics(flags[9], flags[11]))
    dst = (S.CAM_PINHOLE, cm.rectified_pinhole(model, intr, w, h, 0.25), w, h) if undistort else (model, intr, w, h)
    scene = rs.Scene((model, intr, w, h), dst, gyro_t, rates, [prog.frame_time_from_name("1040000000.png", 2000000000.0 * 1e-9)], (28.5 if undistort else 30.0) * 1e-6, q_i_c=K.Q_I_C, time_offset_imu_to_cam=0.004)
    expect, status = rs.rs_rectify_frames(views["images"][:1], scene)
    assert list(status) == [0]
    assert np.array_equal(outs["py"]["1040000000.png"], expect[0])
    assert not np.array_equal(expect[0], views["images"][0])


def test_rectify_rolling_shutter_programs_reject_unknown_flags_and_missing_files(tmp_path):
    flags, _ = _program_inputs(tmp_path)
    good = flags + ["--output_path", str(tmp_path / "o")]
    for tag, cmd in PROGRAMS:
        assert _run(cmd + good + ["--no_such_flag", "1"]).returncode != 0
        for k in (3, 5, 7):                      # telemetry, camera calibration, result JSON
            missing = list(good); missing[k] = str(tmp_path / "nothing.json")
            assert _run(cmd + missing).returncode != 0, (tag, k)
        assert not os.path.exists(str(tmp_path / "o")) or not os.listdir(str(tmp_path / "o"))
