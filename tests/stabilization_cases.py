"""Cases shared by the CPU and GPU tests of the stabilisation: telemetry, scenes, their float64 restatement and longdouble
yardstick.  Everything here is computed once per process (lru_cache) and must be left unchanged by the tests.  Times carry the base
of 9876.5 s of rolling_shutter_cases; the dense telemetry lies on a dyadic grid (1 / 1024 s), so that a reference time can sit on a
sample exactly."""
import functools

import numpy as np

import rolling_shutter_cases as K
import rolling_shutter_restatement as RS
import stabilization_restatement as SR
from openimucameracalibrator_amd import synthetic as S

T_BASE = K.T_BASE
STEP = 1.0 / 1024.0
OFFSET = 0.25
LINE_DELAY = 2.0 ** -15           # 30.5 us; with reference row 256 the reference delay is 2^-7 s exactly
REFERENCE_ROW = 256.0
REF_DELAY = REFERENCE_ROW * LINE_DELAY
PATH_COUNTS = (1, 2, 63, 64, 65, 66, 257)        # 66: not a multiple of the scan's run of 4
ZOOM_SIZES = ((1, 1), (67, 5), (96, 54))


@functools.lru_cache(maxsize=None)
def dense_telemetry(n=700, sigma=2.0):
    """(t [n] IMU clock on the grid T_BASE - OFFSET + j / 1024, rates [n, 3] IMU frame): white noise plus a 3 Hz sway."""
    rng = np.random.RandomState(21)
    j = np.arange(n)
    t = (T_BASE - OFFSET) + j * STEP
    sway = 1.5 * np.sin(2 * np.pi * 3.0 * j[:, None] * STEP + np.array([0.0, 1.0, 2.0])[None])
    om = rng.normal(0.0, sigma, (n, 3)) + sway
    t.setflags(write=False); om.setflags(write=False)
    return t, om


def frame_times_for_reference(ref):
    """frame_t such that t_ref = T_BASE + ref (seconds behind the first gyro sample, camera clock)."""
    return (T_BASE + np.asarray(ref, dtype=np.float64)) - REF_DELAY


def pinhole_destination(size, f=None):
    dw, dh = size
    f = 450.0 * dw / 960.0 * 1.6 if f is None else f          # narrower than the source: room to move
    return (S.CAM_PINHOLE, np.array([f, 1.0, 0.0, (dw - 1) / 2.0, (dh - 1) / 2.0, 0.0, 0.0]), dw, dh)


def clip_args(count, size=(67, 5), source="pinhole", rates_scale=1.0):
    """`count` frames with reference times from 10 ms to 660 ms behind the first sample (two to three gyro samples apart at 257)."""
    t, om = dense_telemetry()
    ref = np.array([0.0101]) if count == 1 else 0.0101 + (0.65 / (count - 1)) * np.arange(count)
    return dict(src=S.CAMERAS[source], dst=pinhole_destination(size), gyro_t=t, gyro_rates=om * rates_scale, frame_t=frame_times_for_reference(ref),
                line_delay_s=LINE_DELAY, q_i_c=K.Q_I_C, time_offset_imu_to_cam=OFFSET, reference_row=REFERENCE_ROW)


MIXED_REFERENCE = np.array([-0.5, 10.2, 10.7, 12.0, 12.5, 13.5, 15.6, 316.3, 900.0]) * STEP
MIXED_STATUS = [1, 0, 0, 0, 0, 0, 0, 0, 1]


def mixed_args(size=(67, 5)):
    """Reference times in units of the gyro step: before the telemetry; two inside interval 10; exactly on sample 12; none, one, two
    and 300 samples up to the next; behind the telemetry."""
    kw = clip_args(2, size)
    kw["frame_t"] = frame_times_for_reference(MIXED_REFERENCE)
    return kw


def restatement_scene(kw):
    kw = dict(kw)
    if "R" in kw:
        kw["Rm"] = kw.pop("R")
    return RS.Scene(**kw)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def path_reference(kind):
    """(float64 path, longdouble path, yardstick rad) of clip `kind` (a frame count, or "mixed")."""
    sc = restatement_scene(mixed_args() if kind == "mixed" else clip_args(kind))
    a, b = SR.path(sc), SR.path(sc, np.longdouble)
    on = ~np.isnan(a[:, 0])
    y = float(K.quaternion_angle(a[on], b[on]).max()) if on.any() else 0.0
    a.setflags(write=False)
    return a, b, y


SIGMAS = {"none": 0.0, "65": 32.2 * (0.65 / 256) / 3.0, "201": 100.2 * (0.65 / 256) / 3.0, "clip": 1.0}


@functools.lru_cache(maxsize=None)
def smooth_reference(name, max_correction=0.0):
    """dict(S, C, iterations, S_ld, C_ld, iterations_ld, members [frames]) of the 257-frame clip at SIGMAS[name]."""
    sc = restatement_scene(clip_args(257))
    sigma = SIGMAS[name]
    P, Pl = SR.path(sc), SR.path(sc, np.longdouble)
    S_, C, it = SR.smooth(sc, P, sigma, max_correction)
    Sl, Cl, itl = SR.smooth(sc, Pl, sigma, max_correction, np.longdouble)
    lo, hi = SR.windows(sc, sigma)
    return _freeze(dict(S=S_, C=C, iterations=it, S_ld=Sl, C_ld=Cl, iterations_ld=itl, members=hi - lo + 1))


# ---- zoom and warp: a shaky clip over a wide source, 40 frames
def shaky_args(size=(96, 54), frames=40, source="gopro9_division"):
    kw = clip_args(frames, size, source, rates_scale=1.0)
    dw, dh = size
    sm, si, sw, sh = S.CAMERAS[source]
    di = np.array(K.destination(source, size)[1], dtype=np.float64)
    kw["dst"] = (S.CAM_PINHOLE, di, dw, dh)
    return kw


SHAKY_SIGMA = 0.05


@functools.lru_cache(maxsize=None)
def shaky_plan(size=(96, 54), frames=40, dtype_name="float64", zoom_mode=1):
    dtype = np.float64 if dtype_name == "float64" else np.longdouble
    return _freeze(SR.plan(restatement_scene(shaky_args(size, frames)), SHAKY_SIGMA, 0.0, zoom_mode, 0.1, np.inf, dtype))


def roll_matrix(alpha):
    c, s = np.cos(alpha), np.sin(alpha)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def still_args(size=(96, 54), R=None):
    """Zero rates, the same centred plain pinhole (f = 64: every ray and its projection are exact) as source and destination."""
    dw, dh = size
    cam = (S.CAM_PINHOLE, np.array([64.0, 1.0, 0.0, (dw - 1) / 2.0, (dh - 1) / 2.0, 0.0, 0.0]), dw, dh)
    kw = clip_args(3, size, rates_scale=0.0)
    kw.update(src=cam, dst=cam, reference_row=(dh - 1) / 2.0)
    kw["frame_t"] = (T_BASE + 0.1 + 0.03 * np.arange(3))
    if R is not None:
        kw["R"] = R
    return kw


# ---- what the entries refuse, and one call of every entry (the library is imported here only)
def _library():
    from openimucameracalibrator_amd import stabilization
    return stabilization


BAD_SCENES = {
    "frame times repeat": lambda kw: kw.update(frame_t=kw["frame_t"][[0, 1, 1, 2]]),
    "frame times decrease": lambda kw: kw.update(frame_t=kw["frame_t"][::-1].copy()),
    "distorted destination": lambda kw: kw.update(dst=(S.CAM_PINHOLE, [40.0, 1.0, 0.0, 1.5, 1.0, -0.05, 0.0], 4, 3)),
    "fisheye destination": lambda kw: kw.update(dst=(S.CAMERAS["gopro6_fisheye"][0], S.CAMERAS["gopro6_fisheye"][1], 4, 3)),
    "one gyro sample": lambda kw: kw.update(gyro_t=kw["gyro_t"][:1], gyro_rates=kw["gyro_rates"][:1]),
}
BAD_OPTIONS = {
    "negative sigma": dict(smoothing_sigma_s=-0.1),
    "nan sigma": dict(smoothing_sigma_s=np.nan),
    "unknown zoom mode": dict(zoom_mode=3),
    "negative zoom mode": dict(zoom_mode=-1),
    "max zoom below 1": dict(max_zoom=0.99),
    "negative correction bound": dict(max_correction_rad=-1.0),
    "negative zoom window": dict(zoom_window_s=-1.0),
}


def small_args():
    return clip_args(4, (4, 3))


def call_every_entry(scene, options=None, correction=None, zoom=None, channels=1, border=0, batch=1):
    """The return codes of oicc_stab_plan, _map, _frames, _frames_device on a scene (host frames)."""
    L = _library()
    b, A = L._bound(), L._abi
    import ctypes as C
    u8, dp, i32 = (lambda a: a.ctypes.data_as(A.c_u8p)), (lambda a: a.ctypes.data_as(A.c_dp)), (lambda a: a.ctypes.data_as(A.c_i32p))
    n = max(scene.num_frames, 1)
    (sw, sh), (dw, dh) = scene.src_size, scene.dst_size
    o = (L.StabOptions() if options is None else options).c()
    q = np.tile([1.0, 0.0, 0.0, 0.0], (n, 1)) if correction is None else np.ascontiguousarray(correction, dtype=np.float64)
    z = np.ones(n) if zoom is None else np.ascontiguousarray(zoom, dtype=np.float64)
    p = L.StabPlan(n)
    m = np.zeros((n, dh, dw, 2), np.float32); v = np.zeros((n, dh, dw), np.uint8); st = np.zeros(n, np.int32)
    F = np.zeros((n, sh, sw, channels), np.uint8); out = np.zeros((n, dh, dw, channels), np.uint8)
    return [b.plan(0, scene.ref(), C.byref(o), dp(p.path_q), dp(p.smooth_q), dp(p.correction_q), dp(p.required_zoom), dp(p.zoom), i32(p.iterations),
                   i32(p.frame_status), u8(p.zoom_clamped), None),
            b.map(0, scene.ref(), dp(q), dp(z), m.ctypes.data_as(A.c_fp), u8(v), None, i32(st), None, None),
            b.frames(0, scene.ref(), dp(q), dp(z), channels, u8(F), border, batch, u8(out), i32(st), None),
            b.frames_device(None, scene.ref(), dp(q), dp(z), channels, u8(F), border, u8(out), i32(st))]
