"""The numpy specification of the horizon lock (tests/horizon_restatement.py) against independent arithmetic, a recovery scene
with a known camera, the premises of the GPU cases, what the new entries answer without a device, and the host code of the
programs against its Python twin.

Yardstick: max |float64 - numpy.longdouble| of the restatement on the case at hand, measured here and printed; a reference may be
ten times that away, plus the reference's own rounding where it has one (stated at the test)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

import horizon_cases as HC
import horizon_restatement as HR
import rolling_shutter_cases as K
import rolling_shutter_restatement as RS
import stabilization_cases as SC
import stabilization_restatement as SR
from openimucameracalibrator_amd import _abi
from openimucameracalibrator_amd import rolling_shutter as rs
from openimucameracalibrator_amd import stabilization as stab

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float64).eps)


class Orientation:
    """scipy's orientation of a camera whose rate is linear inside every gyro interval: Q(x) at x seconds behind the first sample."""

    def __init__(self, t, om):
        self.t, self.om = t, om
        self.Q = [Rot.identity()]
        for j in range(len(t) - 1):
            self.Q.append(self.Q[-1] * Rot.from_rotvec(0.5 * (om[j] + om[j + 1]) * (t[j + 1] - t[j])))

    def __call__(self, x):
        t, om = self.t, self.om
        j = int(np.clip(np.searchsorted(t, x, side="right") - 1, 0, len(t) - 2))
        s, dt = x - t[j], t[j + 1] - t[j]
        return self.Q[j] * Rot.from_rotvec(om[j] * s + (om[j + 1] - om[j]) * s * s / (2 * dt))


def _behind_first_sample(sc, lv):
    """(gyro times, reference times, sample times) in seconds behind the first gyro sample, camera clock."""
    t = sc.gyro_t - sc.gyro_t[0]
    tref = ((sc.frame_t - SC.T_BASE) + sc.reference_row * sc.line_delay) - ((sc.gyro_t[0] - SC.T_BASE) + sc.offset)
    return t, tref, lv.accl_t - sc.gyro_t[0]


# ---------------------------------------------------------------- G1
@pytest.mark.parametrize("kind", ("mixed", "clip"))
def test_accl_world_against_scipy_rotation_products(kind):
    """scipy chains one product per gyro interval from the first sample on, a few eps each: 8 eps per interval times the length of
    the vector is granted to it."""
    kw, at, a, _ = HC.sample_case(65, kind)
    ref = HC.sample_reference(65, kind)
    sc = SC.restatement_scene(kw)
    lv = HR.Level(at, a)
    t, tref, x = _behind_first_sample(sc, lv)
    Q = Orientation(t, sc.rates)
    first = SR.on_path(sc)[0]
    Q0 = Q(tref[first]).inv()
    cam = HR.camera_vectors(a, K.Q_I_C)
    used = np.where(ref["frame_of"] >= 0)[0]
    assert 20 < len(used) < 65
    worst = max(float(np.abs((Q0 * Q(x[j])).apply(cam[j]) - ref["world"][j]).max()) for j in used)
    print("accl world %s: yardstick %.3e m/s^2, restatement - scipy %.3e m/s^2" % (kind, ref["yardstick"], worst))
    assert worst <= 10.0 * ref["yardstick"] + 8 * EPS * len(t) * 12.0
    assert np.all(np.isnan(ref["world"][ref["frame_of"] < 0]))


# ---------------------------------------------------------------- G2
def test_gravity_about_a_fixed_axis_is_the_closed_form_weighted_mean():
    """A camera that turns about a fixed axis n by phi(t) and an accelerometer that reads the constant c: the sample in the path's
    frame is c turned about n by phi_j - phi(t_ref,first), and the mean is c_par + (sum w cos / sum w) c_perp + (sum w sin / sum w) n x c."""
    kw = SC.clip_args(9)
    j = np.arange(len(kw["gyro_t"]))
    axis = np.array([0.36, -0.48, 0.8])
    rate = 3.0 * np.sin(2 * np.pi * 2.0 * j * SC.STEP) + 1.0
    kw["gyro_rates"] = rate[:, None] * axis[None]
    n = RS.camera_rates(axis[None], K.Q_I_C)[0].astype(np.longdouble)
    c = np.array([0.25, -0.95, 0.1]) * HC.G
    rng = np.random.RandomState(3)
    x = np.sort(rng.uniform(0.0, 0.68, 200))
    at, a = HC.accl_times(x), HC.imu_from_camera(np.tile(c, (200, 1)))
    sc = SC.restatement_scene(kw)
    sigma = 0.04
    lv = HR.Level(at, a, gravity_sigma_s=sigma)
    p, pl = HR.plan(sc, lv, K.Q_I_C, 0.05, zoom=False), HR.plan(sc, lv, K.Q_I_C, 0.05, zoom=False, dtype=np.longdouble)
    yardstick = float(np.abs(p["gravity"] - pl["gravity"]).max())
    # phi at any time, the trapezoid of the linear rate, in extended precision
    r = rate.astype(np.longdouble); step = np.longdouble(SC.STEP)
    Phi = np.concatenate([[0], np.cumsum(0.5 * (r[:-1] + r[1:]) * step)])

    def phi(xs):
        i = np.clip(np.floor(xs / step).astype(int), 0, len(r) - 2)
        s = xs - i * step
        return Phi[i] + r[i] * s + (r[i + 1] - r[i]) * s * s / (2 * step)

    _, tref, xs = _behind_first_sample(sc, lv)
    tref, xs = tref.astype(np.longdouble), xs.astype(np.longdouble)
    cl = HR.camera_vectors(a[:1], K.Q_I_C, np.longdouble)[0]
    par = (cl @ n) * n; perp = cl - par; cross = np.cross(n, cl)
    lo, hi = HR.windows(sc, lv)
    assert (p["level_status"] == 0).all() and (hi - lo).min() > 20
    worst = 0.0
    for k in range(9):
        m = np.arange(lo[k], hi[k] + 1)
        s = xs[m] - tref[k]
        w = np.exp(-(s * s) / (2 * np.longdouble(sigma) ** 2))
        d = phi(xs[m]) - phi(tref[:1])[0]
        mean = par + ((w * np.cos(d)).sum() / w.sum()) * perp + ((w * np.sin(d)).sum() / w.sum()) * cross
        worst = max(worst, float(np.abs(mean - p["gravity"][k]).max()))
    print("fixed axis: yardstick %.3e m/s^2, restatement - closed form %.3e m/s^2" % (yardstick, worst))
    assert worst <= 10.0 * yardstick + 16 * EPS * HC.G           # the times behind the first sample are float64 differences


def test_the_levelled_camera_sees_up_straight_above():
    """Rz(theta)^T nu has x = 0 and y < 0 at full lock, full fade and no wanted roll."""
    p = HC.level_reference("200")
    ok = p["level_status"] == 0
    assert ok.all()
    nu, th = p["up"], p["level_angle"]
    assert np.array_equal(th, p["roll"]) and np.abs(th).min() > 0.2        # fade 1, lock 1: the whole roll
    x = np.cos(th) * nu[:, 0] + np.sin(th) * nu[:, 1]
    y = -np.sin(th) * nu[:, 0] + np.cos(th) * nu[:, 1]
    print("levelling identity: |x| max %.3e, y max %.6f" % (np.abs(x).max(), y.max()))
    assert np.abs(x).max() <= 4 * EPS and y.max() < 0
    # and through the quaternions: up in the levelled camera
    for k in range(len(th)):
        g = p["gravity"][k] / np.linalg.norm(p["gravity"][k])
        v = RS.qmat(p["level_q"][k]).T @ g
        assert abs(v[0]) <= 16 * EPS and v[1] < 0


# ---------------------------------------------------------------- recovery
def test_recovery_of_the_true_horizon():
    """A camera with a known orientation R_wc(t) (world z up): sway plus noise as dense_telemetry at half the rates, started 0.2 rad rolled and
    0.1 rad pitched; the accelerometer reads R_wc^T (0, 0, g) plus a 3 Hz linear acceleration of 1 m/s^2.  The levelled camera's
    roll against the true gravity stays within 0.2 degrees wherever the gravity window is not cut by the clip's ends."""
    n, frames, sigma_g = 5400, 150, 0.5
    rng = np.random.RandomState(21)
    j = np.arange(n)
    t = (SC.T_BASE - SC.OFFSET) + j * SC.STEP
    om = 0.5 * (rng.normal(0.0, 2.0, (n, 3)) + 1.5 * np.sin(2 * np.pi * 3.0 * j[:, None] * SC.STEP + np.array([0.0, 1.0, 2.0])[None]))
    kw = SC.clip_args(2)
    kw.update(gyro_t=t, gyro_rates=om, frame_t=SC.frame_times_for_reference(0.1 + np.arange(frames) / 30.0))
    sc = SC.restatement_scene(kw)
    Q = Orientation(t - t[0], sc.rates)
    level_camera = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])          # columns: camera x, y (down), z in the world
    R0 = Rot.from_matrix(level_camera) * Rot.from_euler("zx", [0.2, 0.1])
    x = np.arange(40, 5300, 5) * SC.STEP + 1e-4                                            # 205 Hz, off the gyro grid
    lin = np.stack([np.sin(2 * np.pi * 3.0 * x), np.cos(2 * np.pi * 3.0 * x), np.sin(2 * np.pi * 3.0 * x + 1.0)], -1) / np.sqrt(1.5)
    up_cam = np.stack([(R0 * Q(xj)).inv().apply([0.0, 0.0, HC.G]) for xj in x]) + lin
    lv = HR.Level(HC.accl_times(x), HC.imu_from_camera(up_cam), gravity_sigma_s=sigma_g)
    p = HR.plan(sc, lv, K.Q_I_C, 0.3, zoom=False)
    assert (p["frame_status"] == 0).all() and (p["level_status"] == 0).all()
    _, tref, _ = _behind_first_sample(sc, lv)
    world_of_path = R0 * Q(tref[0])                                                       # the path's frame is the first frame's camera
    whole = (tref - x[0] >= 3 * sigma_g) & (x[-1] - tref >= 3 * sigma_g)
    assert whole.sum() > 40
    residual = np.zeros(frames); before = np.zeros(frames)
    for k in range(frames):
        for q, out in ((p["level_q"][k], residual), (p["smooth_q"][k], before)):
            v = (world_of_path * Rot.from_quat(np.concatenate([q[1:], q[:1]]))).inv().apply([0.0, 0.0, 1.0])
            out[k] = np.degrees(np.arctan2(v[0], -v[1]))
    print("recovery: roll of the smooth camera %.2f .. %.2f deg, of the levelled camera |.| <= %.4f deg on %d whole windows, <= %.4f deg on all" % (
        before.min(), before.max(), np.abs(residual[whole]).max(), whole.sum(), np.abs(residual).max()))
    assert np.abs(before[whole]).min() > 5 * 0.2                    # the smooth camera is far from level: the bound below is the lock's doing
    assert np.abs(residual[whole]).max() <= 0.2


# ---------------------------------------------------------------- premises of the GPU cases
@pytest.mark.parametrize("kind", ("clip", "mixed"))
@pytest.mark.parametrize("na", HC.SAMPLE_COUNTS)
def test_premises_of_the_gpu_sample_cases(na, kind):
    kw, at, a, order = HC.sample_case(na, kind)
    ref = HC.sample_reference(na, kind)
    sc = SC.restatement_scene(kw)
    used = ref["frame_of"] >= 0
    print("premises samples %d %s: %d used, yardstick %.3e m/s^2" % (na, kind, used.sum(), ref["yardstick"]))
    assert ref["yardstick"] <= 1e-12
    assert np.array_equal(np.isnan(ref["world"][:, 0]), ~used) and np.array_equal(np.isnan(np.asarray(ref["world_ld"][:, 0], dtype=np.float64)), ~used)
    if kind == "mixed":
        special = np.argsort(order)[:min(na, len(HC.MIXED_SPECIAL))]                      # where the special samples went
        assert list(ref["frame_of"][special]) == HC.MIXED_FRAME_OF[:na]
        lv = HR.Level(at, a)
        assert HR.sample_times(sc, lv, 3)[special[0]] == 0.0                              # exactly on frame 3's reference time
        assert at[special[0]] == sc.gyro_t[12]                                            # which is gyro sample 12
        if na > 1:
            assert at[special[1]] == sc.gyro_t[14]
        if na > 8:
            _, interval = HR.sample_frames(sc, lv)
            on = SR.on_path(sc)[2]
            assert [int(interval[special[i]] - on[6]) for i in (2, 3, 4, 5)] == [0, 1, 2, 300]   # gyro samples between frame 6 and its samples
    else:
        assert na == 1 or (used.any() and (~used[:3]).any() and (~used[-3:]).any())      # before the first and behind the last reference time


@pytest.mark.parametrize("name", list(HC.LEVEL_CASES))
def test_premises_of_the_gpu_level_cases(name):
    p = HC.level_reference(name)
    at, a, opts = HC.level_of(name)
    sc = SC.restatement_scene(HC.level_args())
    lv = HR.Level(at, a, **opts)
    # window membership and gate in both precisions
    first, count, _ = SR.on_path(sc)
    assert (first, count) == (0, HC.LEVEL_FRAMES)
    used = HR.sample_frames(sc, lv)[0] >= 0
    for k in range(count):
        s64 = HR.sample_times(sc, lv, k)
        sld = ((at.astype(np.longdouble) - np.longdouble(sc.frame_t[k])) + np.longdouble(sc.offset)) - np.longdouble(sc.reference_row) * np.longdouble(sc.line_delay)
        assert np.array_equal(np.abs(s64) <= 3.0 * lv.sigma, np.abs(sld) <= 3 * np.longdouble(lv.sigma))
        assert (used & (np.abs(s64) <= 3.0 * lv.sigma)).sum() == p["members"][k]
    assert np.array_equal(HR.gate(lv), HR.gate(lv, np.longdouble))
    assert np.array_equal(p["gravity_samples"], p["ld"]["gravity_samples"]) and np.array_equal(p["level_status"], p["ld"]["level_status"])
    members = set(int(m) for m in p["members"])
    y = HC.yardsticks(p)
    print("premises level %s: windows %s, status %s, yardsticks %s" % (name, sorted(members), list(p["level_status"]), y))
    sigma = HC.LEVEL_CASES[name]["sigma"]
    if sigma == "0-1":
        assert members == {0, 1} and list(np.where(p["members"] == 1)[0]) == [2, 5]
        assert np.all(p["level_status"][p["members"] == 0] == 2) and np.all(p["level_status"][p["members"] == 1] == 0)
    elif sigma == "63-65":
        assert {63, 64, 65} <= members
    elif sigma == "200":
        assert any(190 <= m <= 210 for m in members)
    else:
        assert members == {int(used.sum())} and used.sum() > 200
    if name == "gated out":
        assert np.all(p["gravity_samples"] == 0) and np.all(p["level_status"] == 2) and np.all(p["level_angle"] == 0)
        assert np.array_equal(p["correction_q"], SR.smooth(sc, SR.path(sc), HC.LEVEL_SMOOTHING)[1])
    elif name == "gate edge":
        g = HR.gate(lv)
        assert g[0::2].all() and not g[1::2].any()                                        # on the edge: kept; a ulp outside: dropped
        lo = np.array([HR.windows(sc, lv)[0][k] for k in range(count)]); hi = HR.windows(sc, lv)[1]
        assert np.array_equal(p["gravity_samples"], [len(np.arange(l, h + 1)[np.arange(l, h + 1) % 2 == 0]) for l, h in zip(lo, hi)])
    elif name == "half lock":
        full = HC.level_reference("200")
        assert np.abs(p["level_angle"] - 0.5 * (full["roll"] - 0.1)).max() <= 4 * EPS
    assert max(y["level_q"], y["correction_q"]) <= 1e-13


def test_premises_of_the_shaky_level_case():
    p = HC.shaky_reference()
    y = HC.yardsticks(p)
    print("premises shaky level: status %s, angle %.4f .. %.4f rad, yardsticks %s" % (sorted(set(p["level_status"])), p["level_angle"].min(), p["level_angle"].max(), y))
    assert np.all(p["level_status"] == 0) and np.all(p["frame_status"] == 0) and np.abs(p["level_angle"]).min() > 0.05
    assert np.array_equal(p["gravity_samples"], p["ld"]["gravity_samples"])


# ---------------------------------------------------------------- the new entries without a device
def _call(scene, t, a, opts, options=None, null=None):
    """The return codes of oicc_stab_plan_level and oicc_debug_stab_accl_world; null: the name of an array that is left out."""
    b = stab._bound()
    dp, i32 = (lambda x: x.ctypes.data_as(_abi.c_dp)), (lambda x: x.ctypes.data_as(_abi.c_i32p))
    lv = stab.LevelOptions.__new__(stab.LevelOptions)
    lv.accl_t, lv.accl = np.ascontiguousarray(t, dtype=np.float64), np.ascontiguousarray(a, dtype=np.float64)
    c = _abi.StabLevel(len(lv.accl_t), dp(lv.accl_t), dp(lv.accl), *[float(dict(dict(gravity_sigma_s=1.0, gravity_const=HC.G, accl_gate=0.0, lock=1.0, roll_rad=0.0), **opts)[k])
                                                                    for k in ("gravity_sigma_s", "gravity_const", "accl_gate", "lock", "roll_rad")])
    if null == "accl_t":
        c.accl_t = None
    if null == "accl":
        c.accl = None
    if null == "num_accl":
        c.num_accl = 0
    n = max(scene.num_frames, 1)
    o = (stab.StabOptions() if options is None else options).c()
    p = stab.StabPlan(n, True)
    outs = dict(level_q=dp(p.level_q), up=dp(p.up), roll=dp(p.roll), level_angle=dp(p.level_angle), gravity_samples=i32(p.gravity_samples),
                level_status=i32(p.level_status))
    if null in outs:
        outs[null] = None
    world = np.zeros((max(len(lv.accl_t), 1), 3)); frame_of = np.zeros(max(len(lv.accl_t), 1), np.int32)
    return [b.plan_level(0, scene.ref(), C.byref(o), C.byref(c), dp(p.path_q), dp(p.smooth_q), dp(p.correction_q), dp(p.required_zoom), dp(p.zoom),
                         i32(p.iterations), i32(p.frame_status), p.zoom_clamped.ctypes.data_as(_abi.c_u8p), outs["level_q"], outs["up"], outs["roll"],
                         outs["level_angle"], outs["gravity_samples"], outs["level_status"], None),
            b.debug_accl_world(0, scene.ref(), C.byref(c), None if null == "world" else dp(world), None if null == "frame_of" else i32(frame_of))]


def test_the_new_entries_are_exported_and_bound():
    b = stab._bound()
    assert "plan_level" in _abi.STABILIZATION_SIGNATURES and "accl_world" in _abi.STABILIZATION_DEBUG_SIGNATURES
    assert b.plan_level is not None and b.debug_accl_world is not None
    assert C.sizeof(_abi.StabLevel) == 64
    lib = C.CDLL(b.lib._name)
    assert hasattr(lib, "oicc_stab_plan_level") and hasattr(lib, "oicc_debug_stab_accl_world")


@pytest.mark.parametrize("name", list(HC.BAD_LEVELS))
def test_bad_levels_are_refused_before_the_device_is_looked_for(name):
    scene = rs.Scene(**SC.small_args())
    assert _call(scene, *HC.BAD_LEVELS[name](*HC.small_level())) == [-1, -1]


def test_null_arrays_and_what_the_plan_refuses_are_refused():
    scene = rs.Scene(**SC.small_args())
    t, a, o = HC.small_level()
    for null in ("accl_t", "accl", "num_accl"):
        assert _call(scene, t, a, o, null=null) == [-1, -1]
    for null in ("level_q", "up", "roll", "level_angle", "gravity_samples", "level_status"):
        assert _call(scene, t, a, o, null=null)[0] == -1
    for null in ("world", "frame_of"):
        assert _call(scene, t, a, o, null=null)[1] == -1
    for bad in SC.BAD_SCENES:
        kw = SC.small_args()
        SC.BAD_SCENES[bad](kw)
        assert _call(rs.Scene(**kw), t, a, o) == [-1, -1], bad
    for bad in SC.BAD_OPTIONS:
        assert _call(scene, t, a, o, options=stab.StabOptions(**SC.BAD_OPTIONS[bad]))[0] == -1, bad
    with pytest.raises(ValueError):
        stab.stab_plan(scene, level=stab.LevelOptions(t, a, lock=2.0))
    with pytest.raises(ValueError):
        stab.LevelOptions(t[:4], a)


def test_the_new_entries_without_a_device():
    import torch
    if torch.cuda.is_available():
        return                      # what a machine without a device answers
    scene = rs.Scene(**SC.small_args())
    t, a, o = HC.small_level()
    assert _call(scene, t, a, o) == [-2, -2]                                  # OICC_ERR_NO_DEVICE
    assert _call(scene, t, a, dict(lock=0.0)) == [-2, -2]
    for call in (lambda: stab.stab_plan(scene, level=stab.LevelOptions(t, a)), lambda: stab.accl_world(scene, stab.LevelOptions(t, a))):
        with pytest.raises(RuntimeError):
            call()


# ---------------------------------------------------------------- host code of the programs, also under sanitizers
@pytest.mark.parametrize("sanitize", (False, True), ids=("plain", "address-undefined"))
def test_host_accelerometer_preparation_equals_the_python_twin(tmp_path, sanitize):
    from openimucameracalibrator_amd import io_files
    from openimucameracalibrator_amd import rectify_rolling_shutter as rrs
    from openimucameracalibrator_amd import stabilize_frames as prog
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    exe = str(tmp_path / "horizon_host_driver")
    csrc = os.path.join(ROOT, "openimucameracalibrator_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I", csrc] + extra + [os.path.join(ROOT, "tests", "horizon_host_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stdout
    rng = np.random.RandomState(4)
    n = 23
    t_ns = 3000000000 + np.arange(n) * 5000000 + rng.randint(-200000, 200000, n)
    io_files.write_telemetry_json(str(tmp_path / "telemetry.json"), t_ns, rng.normal(0, 4.0, (n, 3)) + [0.3, -9.7, 0.8], rng.normal(0, 3.0, (n, 3)))
    json.dump(dict(accelerometer=dict(misalignment_matrix=[[1, -0.021, 0.022], [0, 1, -0.023], [0, 0, 1]], scale_matrix=[[1.004, 0, 0], [0, 0.997, 0], [0, 0, 1.002]]),
                   gyroscope=dict(misalignment_matrix=[[1, -0.011, 0.012], [0.013, 1, -0.014], [-0.015, 0.016, 1]],
                                  scale_matrix=[[1.001, 0, 0], [0, 0.998, 0], [0, 0, 1.003]])), open(str(tmp_path / "intr.json"), "w"))
    json.dump(dict(accl_bias=dict(x=0.11, y=-0.07, z=0.05), gyro_bias=dict(x=0.01, y=-0.02, z=0.03)), open(str(tmp_path / "bias.json"), "w"))
    frames = 3
    q = rng.normal(0, 1, (frames, 4)); up = rng.normal(0, 1, (frames, 3)); up[1] = np.nan
    lq = rng.normal(0, 1, (frames, 4)); lq[2] = np.nan
    roll = rng.normal(0, 1, frames); roll[1] = np.nan; angle = rng.normal(0, 1, frames); angle[1] = 0.0
    samples = rng.randint(0, 300, frames); lstatus = np.array([0, 2, 1]); status = np.array([0, 0, 1])
    required = 1.0 + rng.rand(frames); zoom = 1.0 + rng.rand(frames); clamped = rng.randint(0, 2, frames)
    names = ["%d.png" % rng.randint(0, 2 ** 40) for _ in range(frames)]
    for intr, bias in ((str(tmp_path / "intr.json"), str(tmp_path / "bias.json")), ("", "")):
        args = [str(tmp_path / "telemetry.json"), intr or "-", bias or "-", str(frames)]
        for k in range(frames):
            args += [names[k], str(status[k])] + [repr(float(v)) for v in q[k]] + [repr(float(required[k])), repr(float(zoom[k])), str(clamped[k])]
            args += [repr(float(v)) for v in lq[k]] + [repr(float(v)) for v in up[k]] + [repr(float(roll[k])), repr(float(angle[k])), str(samples[k]), str(lstatus[k])]
        r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        a_intr, a_bias = rrs.read_accl_intrinsics(intr, bias)
        t, a = rs.corrected_accl(json.load(open(str(tmp_path / "telemetry.json"))), a_intr, a_bias)
        expect = "intrinsics" + "".join(" %s" % prog.json_number(float(v)) for v in a_intr) + "\n"
        expect += "bias" + "".join(" %s" % prog.json_number(float(v)) for v in a_bias) + "\n"
        for tj, aj in zip(t, a):
            expect += "%s %s %s %s\n" % tuple(prog.json_number(float(v)) for v in (tj,) + tuple(aj))
        level = dict(level_q=lq, up=up, roll=roll, level_angle=angle, gravity_samples=samples, level_status=lstatus)
        expect += prog.plan_json(names, status, q, required, zoom, clamped, level)
        assert r.stdout == expect
        doc = json.loads(prog.plan_json(names, status, q, required, zoom, clamped, level))["frames"]
        assert doc[0]["level_q"] == list(lq[0]) and doc[1]["up"] == [None] * 3 and doc[1]["roll"] is None and doc[2]["level_status"] == 1
        assert doc[0]["gravity_samples"] == samples[0] and doc[0]["level_angle"] == angle[0]
    assert "level_q" not in prog.plan_json(names, status, q, required, zoom, clamped)
