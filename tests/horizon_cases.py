"""Cases shared by the CPU and GPU tests of the horizon lock: accelerometer samples on stabilization_cases' telemetry (the
1 / 1024 s grid, base 9876.5 s), their float64 restatement and longdouble yardstick.  Everything here is computed once per process
(lru_cache) and must be left unchanged by the tests."""
import functools

import numpy as np

import horizon_restatement as HR
import rolling_shutter_cases as K
import rolling_shutter_restatement as RS
import stabilization_cases as SC

G = 9.811104
STEP = SC.STEP
SAMPLE_COUNTS = (1, 63, 64, 65, 257)
# the mixed frame times, in gyro steps behind the first gyro sample: exactly on frame 3's reference time and on gyro sample 12; on
# gyro sample 14; none, one, two and 300 gyro samples behind frame 6 (15.6); before the first on-path reference time (10.2) and
# behind the last (316.3); inside interval 10 with frame 1
MIXED_SPECIAL = np.array([12.0, 14.0, 15.7, 16.5, 17.5, 315.2, 5.0, 400.0, 10.5])
MIXED_FRAME_OF = [3, 5, 6, 6, 6, 6, -1, -1, 1]


def imu_from_camera(v):
    """Vectors in the camera frame -> the IMU frame: R(q_i_c) v."""
    return np.asarray(v, dtype=np.float64) @ RS.qmat(K.Q_I_C).T


def accl_times(x):
    """IMU-clock times of samples x seconds behind the first gyro sample."""
    return (SC.T_BASE - SC.OFFSET) + np.asarray(x, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def sample_case(na, kind):
    """(scene arguments, accl_t [na], accl [na, 3]) for G1: kind "clip" (65 frames, samples from 20 ms before the first gyro sample
    to 700 ms behind it: some before the first reference time, some behind the last) or "mixed" (the special samples first)."""
    rng = np.random.RandomState(100 + na)
    if kind == "mixed":
        kw = SC.mixed_args()
        x = MIXED_SPECIAL[:na] * STEP
        if na > len(x):
            x = np.concatenate([x, rng.uniform(2.0, 420.0, na - len(x)) * STEP])
    else:
        kw = SC.clip_args(65)
        x = rng.uniform(-0.02, 0.70, na) if na > 1 else np.array([0.3])
    order = np.argsort(x)
    x = x[order]
    assert np.all(np.diff(x) > 0)
    up = np.array([0.25, -0.95, 0.1]) * G + rng.normal(0.0, 1.0, (na, 3))
    t, a = accl_times(x), imu_from_camera(up)
    t.setflags(write=False); a.setflags(write=False)
    return kw, t, a, order


@functools.lru_cache(maxsize=None)
def sample_reference(na, kind):
    """dict(world, frame_of, world_ld, yardstick [m/s^2]) of a sample case."""
    kw, t, a, _ = sample_case(na, kind)
    sc = SC.restatement_scene(kw)
    lv = HR.Level(t, a)
    w, f, _ = HR.accl_world(sc, lv, K.Q_I_C)
    wl, fl, _ = HR.accl_world(sc, lv, K.Q_I_C, dtype=np.longdouble)
    used = f >= 0
    y = float(np.abs(w[used] - wl[used]).max()) if used.any() else 0.0
    return SC._freeze(dict(world=w, frame_of=f, world_ld=wl, yardstick=y))


# ---- G2: 17 frames, 257 samples; the window sizes by sigma_g
LEVEL_FRAMES = 17
LEVEL_SMOOTHING = 0.05
GRAVITY_SIGMAS = {"0-1": 2e-5, "63-65": 0.029, "200": 0.0934, "clip": 1.0}


@functools.lru_cache(maxsize=None)
def level_samples(values="tilted"):
    """(accl_t [257], accl [257, 3]): jittered samples over the clip, two of them 10 us behind the reference times of frames 2 and 5."""
    rng = np.random.RandomState(7)
    ref = 0.0101 + (0.65 / (LEVEL_FRAMES - 1)) * np.arange(LEVEL_FRAMES)
    x = np.sort(np.concatenate([rng.uniform(-0.02, 0.70, 255), ref[[2, 5]] + 1e-5]))
    assert np.all(np.diff(x) > 0)
    if values == "tilted":                  # up about 15 degrees of roll, a little forward, with noise
        up = np.array([0.25, -0.95, 0.1]) * G + rng.normal(0.0, 1.0, (257, 3))
    elif values == "gate":                  # dyadic: even samples exactly on the gate's edge, odd ones a ulp outside
        up = np.tile([0.0, -8.5, 0.0], (257, 1))
        up[1::2, 1] = -np.nextafter(8.5, 9.0)
        t = accl_times(x)
        t.setflags(write=False); up.setflags(write=False)
        return t, up                        # in the IMU frame as they are: the gate sees these numbers
    t, a = accl_times(x), imu_from_camera(up)
    t.setflags(write=False); a.setflags(write=False)
    return t, a


def level_args():
    return SC.clip_args(LEVEL_FRAMES)


LEVEL_CASES = {
    "0-1": dict(sigma="0-1"), "63-65": dict(sigma="63-65"), "200": dict(sigma="200"), "clip": dict(sigma="clip"),
    "half lock": dict(sigma="200", lock=0.5, roll_rad=0.1),
    "gated out": dict(sigma="200", accl_gate=1e-3, gravity_const=3.0),
    "gate edge": dict(sigma="200", values="gate", accl_gate=0.5, gravity_const=8.0),
}


def level_of(name, **more):
    """(accl_t, accl, keyword arguments of HR.Level / stabilization.LevelOptions behind the samples)."""
    c = dict(LEVEL_CASES[name]); c.update(more)
    t, a = level_samples(c.pop("values", "tilted"))
    opts = dict(gravity_sigma_s=GRAVITY_SIGMAS[c.pop("sigma")], gravity_const=c.pop("gravity_const", G), accl_gate=c.pop("accl_gate", 0.0),
                lock=c.pop("lock", 1.0), roll_rad=c.pop("roll_rad", 0.0))
    assert not c
    return t, a, opts


def _plan_pair(kw, t, a, opts, smoothing, max_correction=0.0, zoom=False, zoom_mode=1):
    sc = SC.restatement_scene(kw)
    lv = HR.Level(t, a, **opts)
    p = HR.plan(sc, lv, K.Q_I_C, smoothing, max_correction, zoom_mode, zoom=zoom)
    pl = HR.plan(sc, lv, K.Q_I_C, smoothing, max_correction, zoom_mode, dtype=np.longdouble, zoom=zoom)
    lo, hi = HR.windows(sc, lv)
    p["members"] = hi - lo + 1
    p["ld"] = pl
    return SC._freeze(p)


@functools.lru_cache(maxsize=None)
def level_reference(name, max_correction=0.0):
    """The float64 plan of a level case (no zoom) with its longdouble run under "ld" and the window sizes under "members"."""
    t, a, opts = level_of(name)
    return _plan_pair(level_args(), t, a, opts, LEVEL_SMOOTHING, max_correction)


def yardsticks(p):
    """dict of max |float64 - longdouble| of a plan pair: quaternion angles in rad, up (unit vector), roll and level_angle in rad."""
    l = p["ld"]
    on = ~np.isnan(p["path_q"][:, 0])
    ok = p["level_status"] != 2
    return dict(level_q=float(K.quaternion_angle(p["level_q"][on], l["level_q"][on]).max()),
                correction_q=float(K.quaternion_angle(p["correction_q"], l["correction_q"]).max()),
                up=float(np.abs(p["up"][ok] - l["up"][ok]).max()) if ok.any() else 0.0,
                roll=float(np.abs(p["roll"][ok] - l["roll"][ok]).max()) if ok.any() else 0.0,
                level_angle=float(np.abs(p["level_angle"] - l["level_angle"]).max()))


# ---- closed form: zero rates, a constant accelerometer
def still_level(alpha, tilt=0.0, **opts):
    """(scene arguments of SC.still_args at 96 x 54, accl_t, accl): up = (sin alpha cos tilt, -cos alpha cos tilt, sin tilt) in the
    camera at every sample, 64 samples over the clip's 60 ms."""
    kw = SC.still_args((96, 54))
    kw["q_i_c"] = (1.0, 0.0, 0.0, 0.0)
    x = (0.1 - SC.OFFSET) + (kw["reference_row"] * SC.LINE_DELAY - 0.001) + 0.001 * np.arange(64)
    up = G * np.array([np.sin(alpha) * np.cos(tilt), -np.cos(alpha) * np.cos(tilt), np.sin(tilt)])
    return kw, SC.T_BASE + x, np.tile(up, (64, 1))


# ---- the shaky clip with a level
@functools.lru_cache(maxsize=None)
def shaky_level():
    """(accl_t [300], accl [300, 3]) over the 40-frame shaky clip: up rolled by 0.12 rad, noise 0.3 m/s^2."""
    rng = np.random.RandomState(11)
    x = np.sort(rng.uniform(0.0, 0.68, 300))
    up = np.array([np.sin(0.12), -np.cos(0.12), 0.05]) * G + rng.normal(0.0, 0.3, (300, 3))
    t, a = accl_times(x), imu_from_camera(up)
    t.setflags(write=False); a.setflags(write=False)
    return t, a


SHAKY_LEVEL = dict(gravity_sigma_s=0.2, gravity_const=G, accl_gate=0.0, lock=1.0, roll_rad=0.0)


@functools.lru_cache(maxsize=None)
def shaky_reference():
    t, a = shaky_level()
    return _plan_pair(SC.shaky_args((96, 54), 40), t, a, SHAKY_LEVEL, SC.SHAKY_SIGMA)


# ---- what the entries refuse
def small_level(**opts):
    t = accl_times(0.02 + 0.01 * np.arange(5))
    a = np.tile([0.0, -G, 0.0], (5, 1))
    return t, a, opts


BAD_LEVELS = {
    "times repeat": lambda t, a, o: (t[[0, 1, 1, 2, 3]], a, o),
    "times decrease": lambda t, a, o: (t[::-1].copy(), a, o),
    "nan sample": lambda t, a, o: (t, np.where(np.arange(15).reshape(5, 3) == 7, np.nan, a), o),
    "infinite time": lambda t, a, o: (np.concatenate([t[:4], [np.inf]]), a, o),
    "zero sigma": lambda t, a, o: (t, a, dict(o, gravity_sigma_s=0.0)),
    "nan sigma": lambda t, a, o: (t, a, dict(o, gravity_sigma_s=np.nan)),
    "zero gravity": lambda t, a, o: (t, a, dict(o, gravity_const=0.0)),
    "negative gate": lambda t, a, o: (t, a, dict(o, accl_gate=-1.0)),
    "lock above 1": lambda t, a, o: (t, a, dict(o, lock=1.0 + 2.0 ** -52)),
    "negative lock": lambda t, a, o: (t, a, dict(o, lock=-0.1)),
    "nan lock": lambda t, a, o: (t, a, dict(o, lock=np.nan)),
    "infinite roll": lambda t, a, o: (t, a, dict(o, roll_rad=np.inf)),
}
