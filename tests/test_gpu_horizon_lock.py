"""The horizon lock on the device (csrc/stabilization.hip: stab_accl_world_kernel, stab_level_kernel) against its numpy
specification tests/horizon_restatement.py.

The yardstick of a case is the distance of the float64 restatement from its numpy.longdouble run; the device may be ten times that
away from the float64 restatement ("Horizon lock", holds the measured ratios).  Counts, frames and statuses are held
exactly; without a level, at lock 0 and wherever the angle is 0 the plan is oicc_stab_plan's bit for bit."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import horizon_cases as HC
import horizon_restatement as HR
import rolling_shutter_cases as K
import stabilization_cases as SC
import stabilization_restatement as SR
import test_gpu_rolling_shutter as T
from openimucameracalibrator_amd import _abi
from openimucameracalibrator_amd import rolling_shutter as rs
from openimucameracalibrator_amd import stabilization as stab

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
COMMON = ("path_q", "smooth_q", "correction_q", "required_zoom", "zoom", "iterations", "frame_status", "zoom_clamped")


def _same(a, b):
    """Bit for bit, NaN included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- G1
@pytest.mark.parametrize("kind", ("clip", "mixed"))
@pytest.mark.parametrize("na", HC.SAMPLE_COUNTS)
def test_accl_world_against_restatement(na, kind):
    kw, at, a, _ = HC.sample_case(na, kind)
    ref = HC.sample_reference(na, kind)
    world, frame_of = stab.accl_world(rs.Scene(**kw), stab.LevelOptions(at, a))
    assert np.array_equal(frame_of, ref["frame_of"])
    used = frame_of >= 0
    assert np.all(np.isnan(world[~used])) and np.all(np.isfinite(world[used]))
    distance = float(np.abs(world[used] - ref["world"][used]).max()) if used.any() else 0.0
    print("accl world %d %s: %d used, yardstick %.3e m/s^2, device vs float64 %.3e m/s^2" % (na, kind, used.sum(), ref["yardstick"], distance))
    assert distance <= 10.0 * ref["yardstick"]


# ---------------------------------------------------------------- G2
def _check_against(p, ref, what):
    y = HC.yardsticks(ref)
    on = ~np.isnan(ref["path_q"][:, 0])
    ok = ref["level_status"] != 2
    assert np.array_equal(p.gravity_samples, ref["gravity_samples"]) and np.array_equal(p.level_status, ref["level_status"])
    assert np.array_equal(np.isnan(p.up), np.isnan(ref["up"])) and np.array_equal(np.isnan(p.roll), np.isnan(ref["roll"]))
    assert np.array_equal(np.isnan(p.level_q[:, 0]), ~on)
    d = dict(level_q=float(K.quaternion_angle(ref["level_q"][on], p.level_q[on]).max()),
             correction_q=float(K.quaternion_angle(ref["correction_q"], p.correction_q).max()),
             up=float(np.abs(p.up[ok] - ref["up"][ok]).max()) if ok.any() else 0.0,
             roll=float(np.abs(p.roll[ok] - ref["roll"][ok]).max()) if ok.any() else 0.0,
             level_angle=float(np.abs(p.level_angle - ref["level_angle"]).max()))
    for key in sorted(d):
        print("%s %s: yardstick %.3e, device vs float64 %.3e" % (what, key, y[key], d[key]))
    for key in d:
        assert d[key] <= 10.0 * y[key], key
    assert np.all(p.correction_q[:, 0] > 0)
    assert np.all(p.level_angle[ref["level_status"] != 0] == 0)


@pytest.mark.parametrize("name", list(HC.LEVEL_CASES))
def test_levelled_camera_against_restatement(name):
    ref = HC.level_reference(name)
    at, a, opts = HC.level_of(name)
    scene = rs.Scene(**HC.level_args())
    options = stab.StabOptions(smoothing_sigma_s=HC.LEVEL_SMOOTHING, zoom_mode="none")
    p = stab.stab_plan(scene, options, level=stab.LevelOptions(at, a, **opts))
    plain = stab.stab_plan(scene, options)
    _check_against(p, ref, "level " + name)
    assert _same(p.path_q, plain.path_q) and _same(p.smooth_q, plain.smooth_q) and _same(p.iterations, plain.iterations)      # smooth_q stays the mean
    still = p.level_angle == 0
    assert _same(p.correction_q[still], plain.correction_q[still]) and _same(p.level_q[still], plain.smooth_q[still])
    if name in ("200", "63-65", "clip"):
        assert not still.any() and np.abs(p.level_angle).min() > 0.1
    if name == "gated out":
        assert still.all()


# ---------------------------------------------------------------- closed form
def _still_plan(alpha, tilt=0.0, smoothing=0.0, **opts):
    kw, at, a = HC.still_level(alpha, tilt)
    scene = rs.Scene(**kw)
    options = stab.StabOptions(smoothing_sigma_s=smoothing, zoom_mode="fixed")
    return scene, options, stab.stab_plan(scene, options, level=stab.LevelOptions(at, a, **opts))


@pytest.mark.parametrize("alpha", (0.02, 0.1, -0.25))
def test_a_still_rolled_camera_is_the_closed_form(alpha):
    """Zero rates and up = (sin alpha, -cos alpha, 0) in the camera: roll = alpha and C = (cos alpha/2, 0, 0, sin alpha/2), the roll of
    a centred pinhole whose required zoom test_gpu_stabilization.py bounds from both sides."""
    w, h = 96, 54
    _, _, p = _still_plan(alpha)
    want = np.array([np.cos(alpha / 2), 0.0, 0.0, np.sin(alpha / 2)])
    print("still %.2f: roll %s, correction %s, required zoom %s" % (alpha, p.roll, p.correction_q[0], p.required_zoom))
    assert np.all(p.level_status == 0) and np.all(p.frame_status == 0) and np.all(p.gravity_samples > 50)
    assert np.abs(p.roll - alpha).max() <= 4 * EPS and np.abs(p.level_angle - alpha).max() <= 4 * EPS
    assert np.abs(p.correction_q - want).max() <= 4 * EPS and np.abs(p.level_q - want).max() <= 4 * EPS
    assert np.abs(p.up - [np.sin(alpha), -np.cos(alpha), 0.0]).max() <= 4 * EPS
    a = abs(alpha)
    z = np.cos(a) + max((w - 1.0) / (h - 1.0), (h - 1.0) / (w - 1.0)) * np.sin(a)
    assert np.all(p.required_zoom >= z * (1.0 - 1e-12))
    assert np.all(p.required_zoom <= z * (1.0 + 2.0 ** -16 / 32.0) + 1e-12)
    assert np.array_equal(p.zoom, np.full(3, p.required_zoom.max()))
    # the wanted roll is the camera's own: nothing to do
    _, _, same = _still_plan(alpha, roll_rad=alpha)
    assert np.abs(same.level_angle).max() <= 4 * EPS and np.abs(same.correction_q - [1.0, 0.0, 0.0, 0.0]).max() <= 4 * EPS
    assert np.abs(same.roll - alpha).max() <= 4 * EPS
    # half the lock: half the angle
    _, _, half = _still_plan(alpha, lock=0.5)
    assert np.abs(half.level_angle - alpha / 2).max() <= 4 * EPS
    assert np.abs(half.correction_q - [np.cos(alpha / 4), 0.0, 0.0, np.sin(alpha / 4)]).max() <= 4 * EPS
    # and with a smoothing window over the three frames the smooth camera is still the identity
    _, _, smoothed = _still_plan(alpha, smoothing=0.05)
    assert np.abs(smoothed.correction_q - want).max() <= 4 * EPS


def _still_reference(alpha, tilt):
    kw, at, a = HC.still_level(alpha, tilt)
    sc = SC.restatement_scene(kw)
    lv = HR.Level(at, a)
    p = HR.plan(sc, lv, kw["q_i_c"], 0.0, zoom=False)
    p["ld"] = HR.plan(sc, lv, kw["q_i_c"], 0.0, zoom=False, dtype=np.longdouble)
    return p


def test_the_lock_fades_out_towards_the_vertical():
    alpha = 0.3
    # h = 0.25, between sin 10 deg and sin 20 deg: a scaled angle
    tilt = float(np.arccos(0.25))
    ref = _still_reference(alpha, tilt)
    _, _, p = _still_plan(alpha, tilt)
    fade = (0.25 - HR.SIN10) / (HR.SIN20 - HR.SIN10)
    assert 0.4 < fade < 0.5 and np.all(ref["level_status"] == 0)
    assert np.abs(ref["level_angle"] - fade * alpha).max() <= 64 * EPS
    _check_against(p, ref, "fade")
    # h = 0.1 < sin 10 deg: the camera looks along gravity
    tilt = float(np.arccos(0.1))
    scene, options, p = _still_plan(alpha, tilt)
    plain = stab.stab_plan(scene, options)
    assert np.all(p.level_status == 1) and np.all(p.level_angle == 0) and np.all(np.isfinite(p.roll))
    for key in COMMON:
        assert _same(getattr(p, key), getattr(plain, key)), key
    assert _same(p.level_q, plain.smooth_q)


# ---------------------------------------------------------------- lock 0 and no level
def _plan_without_level(scene, options):
    """oicc_stab_plan_level with level = NULL."""
    b = stab._bound()
    p = stab.StabPlan(scene.num_frames, True)
    o = options.c()
    dp, i32 = (lambda x: x.ctypes.data_as(_abi.c_dp)), (lambda x: x.ctypes.data_as(_abi.c_i32p))
    rc = b.plan_level(0, scene.ref(), C.byref(o), None, dp(p.path_q), dp(p.smooth_q), dp(p.correction_q), dp(p.required_zoom), dp(p.zoom), i32(p.iterations),
                      i32(p.frame_status), p.zoom_clamped.ctypes.data_as(_abi.c_u8p), dp(p.level_q), dp(p.up), dp(p.roll), dp(p.level_angle),
                      i32(p.gravity_samples), i32(p.level_status), dp(p.device_ms))
    assert rc == 0
    return p


def test_lock_zero_and_no_level_are_the_plan_bit_for_bit():
    kw = SC.clip_args(257)
    scene = rs.Scene(**kw)
    options = stab.StabOptions(smoothing_sigma_s=SC.SIGMAS["65"], zoom_mode="dynamic", zoom_window_s=0.1, max_zoom=100.0)
    plain = stab.stab_plan(scene, options)
    assert SR.correction_angle(plain.correction_q).max() > 1e-3
    at, a, opts = HC.level_of("200", lock=0.0)
    locked_off = stab.stab_plan(scene, options, level=stab.LevelOptions(at, a, **opts))
    none = _plan_without_level(scene, options)
    for p in (locked_off, none):
        for key in COMMON:
            assert _same(getattr(p, key), getattr(plain, key)), key
        assert _same(p.level_q, plain.smooth_q) and np.all(p.level_angle == 0) and not np.signbit(p.level_angle).any()
    assert np.all(locked_off.level_status == 0) and np.all(np.isfinite(locked_off.roll)) and np.all(locked_off.gravity_samples > 0)      # measured, not applied
    assert np.all(np.isnan(none.up)) and np.all(np.isnan(none.roll)) and np.all(none.gravity_samples == 0) and np.all(none.level_status == 0)


# ---------------------------------------------------------------- clamp
def test_levelled_correction_clamp_just_below_and_just_above():
    free_ref = HC.level_reference("200")
    angles = SR.correction_angle(free_ref["correction_q"])
    k = int(np.argsort(angles)[len(angles) // 2])            # a frame in the middle of the angles
    at, a, opts = HC.level_of("200")
    scene = rs.Scene(**HC.level_args())
    level = stab.LevelOptions(at, a, **opts)
    free = stab.stab_plan(scene, stab.StabOptions(smoothing_sigma_s=HC.LEVEL_SMOOTHING, zoom_mode="none"), level=level)
    for factor, clamped in ((1.0 + 1e-9, False), (1.0 - 1e-9, True)):
        bound = float(angles[k]) * factor
        p = stab.stab_plan(scene, stab.StabOptions(smoothing_sigma_s=HC.LEVEL_SMOOTHING, max_correction_rad=bound, zoom_mode="none"), level=level)
        ref = HC.level_reference("200", bound)
        got = SR.correction_angle(p.correction_q)
        below = angles < bound * (1.0 - 1e-6); above = angles > bound * (1.0 + 1e-6)
        assert below.sum() >= 3 and above.sum() >= 3
        assert _same(p.correction_q[below], free.correction_q[below])                    # untouched
        assert _same(p.level_q, free.level_q) and _same(p.smooth_q, free.smooth_q)       # the levelled camera itself is not clamped
        assert np.abs(got[above] - bound).max() <= 4 * EPS
        assert np.array_equal(p.correction_q[k], free.correction_q[k]) != clamped
        _check_against(p, ref, "clamp %s" % ("above" if clamped else "below"))
        axis = lambda q: q[:, 1:] / np.linalg.norm(q[:, 1:], axis=1, keepdims=True)
        assert np.abs(axis(p.correction_q[above]) - axis(free.correction_q[above])).max() <= 1e-12


# ---------------------------------------------------------------- the shaky clip
def test_the_levelled_shaky_clip_leaves_no_invalid_pixel():
    """The plan's path, smooth and levelled cameras against the restatement; the zoom is the plan's own kernels on the new
    correction (the closed-form test bounds it), held here by what it is for: no invalid pixel at the applied zoom."""
    ref = HC.shaky_reference()
    at, a = HC.shaky_level()
    scene = rs.Scene(**SC.shaky_args((96, 54), 40))
    p = stab.stab_plan(scene, stab.StabOptions(smoothing_sigma_s=SC.SHAKY_SIGMA, zoom_mode="fixed", max_zoom=100.0), level=stab.LevelOptions(at, a, **HC.SHAKY_LEVEL))
    _check_against(p, ref, "shaky")
    assert np.all(p.frame_status == 0) and not p.zoom_clamped.any() and np.all(p.zoom >= p.required_zoom)
    plain = stab.stab_plan(scene, stab.StabOptions(smoothing_sigma_s=SC.SHAKY_SIGMA, zoom_mode="fixed", max_zoom=100.0))
    print("shaky: zoom %.4f levelled, %.4f without; device ms %s" % (p.zoom[0], plain.zoom[0], p.device_ms))
    assert p.zoom[0] > plain.zoom[0]                                                      # 0.12 rad of roll cost field of view
    mapxy, valid, status, num_valid = stab.stab_map(scene, p.correction_q, p.zoom)
    assert np.all(num_valid == 96 * 54)
    assert (stab.stab_map(scene, p.correction_q, np.ones(40))[3] < 96 * 54).any()


# ---------------------------------------------------------------- programs
PROGRAMS = (("cpp", [os.path.join(T.CSRC, "stabilize_frames")]), ("py", [sys.executable, "-m", "openimucameracalibrator_amd.stabilize_frames"]))
NAMES = ["1040000000.png", "1100000000.png", "1900000000.png"]


def _inputs_with_gravity(tmp_path):
    """The files of the rectify_rolling_shutter program test, the accelerometer replaced by a rolled up vector with noise."""
    flags, views = T._program_inputs(tmp_path)
    telemetry = json.load(open(flags[3]))
    rng = np.random.RandomState(9)
    n = len(telemetry["timestamps_ns"])
    up = np.array([np.sin(0.15), -np.cos(0.15), 0.1]) * HC.G + rng.normal(0.0, 0.5, (n, 3))
    telemetry["accelerometer"] = [[float(v) for v in row] for row in HC.imu_from_camera(up)]
    json.dump(telemetry, open(flags[3], "w"))
    json.dump(dict(accl_bias=dict(x=0.05, y=-0.04, z=0.03), gyro_bias=dict(x=0.01, y=-0.02, z=0.03)), open(flags[11], "w"))
    return flags, views


def _same_frames(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def _run_programs(tmp_path, flags, extra, tag_suffix):
    from PIL import Image
    outs, plans = {}, {}
    for tag, cmd in PROGRAMS:
        out = tmp_path / ("out_%s_%s" % (tag, tag_suffix))
        plan = str(tmp_path / ("plan_%s_%s.json" % (tag, tag_suffix)))
        r = T._run(cmd + flags + extra + ["--output_path", str(out), "--output_plan_json", plan])
        assert r.returncode == 0, r.stdout + r.stderr
        assert sorted(os.listdir(str(out))) == NAMES[:2]
        outs[tag] = [np.asarray(Image.open(str(out / n))) for n in NAMES[:2]]
        plans[tag] = open(plan).read()
    return outs, plans


def test_stabilize_frames_programs_with_the_horizon_lock(tmp_path):
    from openimucameracalibrator_amd import camera_maps as cm
    from openimucameracalibrator_amd import stabilize_frames as prog
    from openimucameracalibrator_amd import synthetic as S
    flags, views = _inputs_with_gravity(tmp_path)
    common = ["--balance", "0.25", "--smoothing_s", "0.08", "--zoom_mode", "fixed", "--max_zoom", "3"]
    horizon = ["--horizon_lock", "1", "--horizon_roll_deg", "2", "--gravity_window_s", "0.05", "--accl_gate", "4"]
    outs, plans = _run_programs(tmp_path, flags, common + horizon, "on")
    assert plans["cpp"] == plans["py"] and _same_frames(outs["cpp"], outs["py"])
    doc = json.loads(plans["py"])["frames"]
    assert [f["name"] for f in doc] == NAMES and [f["status"] for f in doc] == [0, 0, 1] and [f["level_status"] for f in doc] == [0, 0, 2]
    assert all(abs(f["level_angle"] - (0.15 - np.radians(2.0))) < 0.05 and f["gravity_samples"] > 5 for f in doc[:2])
    assert doc[2]["up"] == [None] * 3 and doc[2]["roll"] is None and doc[2]["level_angle"] == 0
    # the same plan through the library, from the same files
    model, intr, w, h = S.CAMERAS["gopro9_division"]
    telemetry = json.load(open(flags[3]))
    gyro_t, rates = rs.corrected_gyro(telemetry, *prog.read_gyro_intrinsics(flags[9], flags[11]))
    accl_t, accl = rs.corrected_accl(telemetry, *prog.read_accl_intrinsics(flags[9], flags[11]))
    dst = (S.CAM_PINHOLE, cm.rectified_pinhole(model, intr, w, h, 0.25), w, h)
    times = [prog.frame_time_from_name(n, 2000000000.0 * 1e-9) for n in NAMES]
    scene = rs.Scene((model, intr, w, h), dst, gyro_t, rates, times, 30.0 * 1e-6, q_i_c=K.Q_I_C, time_offset_imu_to_cam=0.004)
    p = stab.stab_plan(scene, stab.StabOptions(0.08, 0.0, "fixed", 1.0, 3.0), level=stab.LevelOptions(accl_t, accl, 0.05, 9.811104, 4.0, 1.0, np.radians(2.0)))
    assert prog.plan_json(NAMES, p.frame_status, p.correction_q, p.required_zoom, p.zoom, p.zoom_clamped, p) == plans["py"]
    # off: the files of the programs without the horizon flags, whatever the other horizon flags say
    bare_outs, bare_plans = _run_programs(tmp_path, flags, common, "bare")
    off_outs, off_plans = _run_programs(tmp_path, flags, common + ["--horizon_lock", "0", "--horizon_roll_deg", "7", "--gravity_window_s", "0.3"], "off")
    assert bare_plans["cpp"] == bare_plans["py"] == off_plans["cpp"] == off_plans["py"] and "level_q" not in bare_plans["py"]
    assert all(_same_frames(bare_outs["py"], o) for o in (bare_outs["cpp"], off_outs["cpp"], off_outs["py"]))
    assert not _same_frames(bare_outs["py"], outs["py"])
    plain = stab.stab_plan(scene, stab.StabOptions(0.08, 0.0, "fixed", 1.0, 3.0))
    assert prog.plan_json(NAMES, plain.frame_status, plain.correction_q, plain.required_zoom, plain.zoom, plain.zoom_clamped) == bare_plans["py"]
    for tag, cmd in PROGRAMS:
        assert T._run(cmd + flags + common + ["--horizon_lock", "1.5", "--output_path", str(tmp_path / "o")]).returncode != 0
