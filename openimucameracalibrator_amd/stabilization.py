"""Gyro video stabilisation on the GPU (csrc/stabilization.hip, the oicc_stab_* entries of include/oicc_hip.h; DESIGN.md,
"Stabilisation").

On top of the rolling-shutter rectification: stab_plan integrates the orientation path of a whole clip, smooths it on SO(3) and
finds the zoom that keeps every stabilised frame inside its source image; stab_map and stab_frames then warp chunks of frames with
the plan's per-frame correction and zoom, the rolling shutter taken out in the same pass.  With a LevelOptions the plan also levels
the smooth camera by gravity from the accelerometer (horizon lock).  The scene is rolling_shutter.Scene with
strictly increasing frame times and a plain PINHOLE destination.  Rotation only; there is no CPU path: every function raises
without the HIP library or a device."""
import ctypes as C

import numpy as np

from . import _abi
from .rolling_shutter import DEFAULT_BATCH, Scene, _check, _dp, _is_cuda_tensor, corrected_accl      # noqa: F401  (Scene, corrected_accl: part of this interface)

ZOOM_MODES = {"none": 0, "fixed": 1, "dynamic": 2}


def _bound():
    from . import _lib
    return _lib.load_stabilization()       # raises without the HIP library


class StabOptions:
    """smoothing_sigma_s: sigma of the Gaussian window over the reference times (0: no smoothing); max_correction_rad: the largest
    correction angle (0: none); zoom_mode: "none" / 0, "fixed" / 1, "dynamic" / 2; zoom_window_s: T of the dynamic zoom;
    max_zoom: applied zooms above it are clamped and flagged."""

    def __init__(self, smoothing_sigma_s=0.5, max_correction_rad=0.0, zoom_mode="fixed", zoom_window_s=1.0, max_zoom=4.0):
        self.smoothing_sigma_s, self.max_correction_rad = float(smoothing_sigma_s), float(max_correction_rad)
        self.zoom_mode = ZOOM_MODES[zoom_mode] if isinstance(zoom_mode, str) else int(zoom_mode)
        self.zoom_window_s, self.max_zoom = float(zoom_window_s), float(max_zoom)

    def c(self):
        return _abi.StabOptions(self.smoothing_sigma_s, self.max_correction_rad, self.zoom_mode, 0, self.zoom_window_s, self.max_zoom)


class LevelOptions:
    """The horizon lock (oicc_stab_level): accl_t [na] seconds in the IMU clock, strictly increasing, and accl [na, 3], the corrected
    specific force in the IMU frame in m/s^2 (corrected_accl: up at rest); gravity_sigma_s: sigma of the Gaussian window of the
    gravity mean; gravity_const; accl_gate: samples whose norm is further from gravity_const are left out (0: no gate); lock in
    [0, 1]: the part of the roll that is taken out; roll_rad: the roll that is wanted."""

    def __init__(self, accl_t, accl, gravity_sigma_s=1.0, gravity_const=9.811104, accl_gate=0.0, lock=1.0, roll_rad=0.0):
        self.accl_t = np.ascontiguousarray(accl_t, dtype=np.float64).ravel()
        self.accl = np.ascontiguousarray(accl, dtype=np.float64).reshape(-1, 3)
        if len(self.accl_t) != len(self.accl):
            raise ValueError("%d accelerometer times for %d samples" % (len(self.accl_t), len(self.accl)))
        self.gravity_sigma_s, self.gravity_const, self.accl_gate = float(gravity_sigma_s), float(gravity_const), float(accl_gate)
        self.lock, self.roll_rad = float(lock), float(roll_rad)

    def c(self):
        """The struct; this object keeps its arrays alive."""
        return _abi.StabLevel(len(self.accl_t), _dp(self.accl_t), _dp(self.accl), self.gravity_sigma_s, self.gravity_const, self.accl_gate, self.lock,
                              self.roll_rad)


class StabPlan:
    """What stab_plan returns, arrays over the scene's frames: path_q, smooth_q, correction_q [frames, 4] (w, x, y, z; NaN path and
    smooth off the path), required_zoom, zoom [frames], iterations, frame_status [frames] int32, zoom_clamped [frames] uint8,
    device_ms [3] (path, smoothing, zoom kernels).  With a level also level_q [frames, 4], up [frames, 3] (up in the smooth camera),
    roll, level_angle [frames], gravity_samples, level_status [frames] int32 (0 levelled, 1 the camera looks along gravity, 2 no
    gravity), and device_ms [5] (then the two kernels of the horizon lock)."""

    def __init__(self, n, level=False):
        self.path_q, self.smooth_q, self.correction_q = np.zeros((n, 4)), np.zeros((n, 4)), np.zeros((n, 4))
        self.required_zoom, self.zoom = np.zeros(n), np.zeros(n)
        self.iterations, self.frame_status = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.zoom_clamped = np.zeros(n, np.uint8)
        self.device_ms = np.zeros(5 if level else 3)
        if level:
            self.level_q, self.up, self.roll, self.level_angle = np.zeros((n, 4)), np.zeros((n, 3)), np.zeros(n), np.zeros(n)
            self.gravity_samples, self.level_status = np.zeros(n, np.int32), np.zeros(n, np.int32)


def stab_plan(scene, options=None, device=0, level=None):
    """The plan of a clip: scene.frame_t holds every frame's time.  level: LevelOptions, the horizon lock."""
    o = (StabOptions() if options is None else options).c()
    p = StabPlan(max(scene.num_frames, 1), level is not None)
    i32 = lambda a: a.ctypes.data_as(_abi.c_i32p)
    if level is None:
        _check(_bound().plan(int(device), scene.ref(), C.byref(o), _dp(p.path_q), _dp(p.smooth_q), _dp(p.correction_q), _dp(p.required_zoom), _dp(p.zoom),
                             i32(p.iterations), i32(p.frame_status), p.zoom_clamped.ctypes.data_as(_abi.c_u8p), _dp(p.device_ms)), "oicc_stab_plan")
        return p
    lv = level.c()
    _check(_bound().plan_level(int(device), scene.ref(), C.byref(o), C.byref(lv), _dp(p.path_q), _dp(p.smooth_q), _dp(p.correction_q), _dp(p.required_zoom),
                               _dp(p.zoom), i32(p.iterations), i32(p.frame_status), p.zoom_clamped.ctypes.data_as(_abi.c_u8p), _dp(p.level_q), _dp(p.up),
                               _dp(p.roll), _dp(p.level_angle), i32(p.gravity_samples), i32(p.level_status), _dp(p.device_ms)), "oicc_stab_plan_level")
    return p


def accl_world(scene, level, device=0):
    """Step G1 of the horizon lock alone: (world [na, 3], every accelerometer sample in the frame of the path, NaN for the samples
    before the first on-path frame's reference time or behind the last one's; frame_of [na] int32, the sample's frame or -1)."""
    lv = level.c()
    na = max(len(level.accl_t), 1)
    world = np.zeros((na, 3)); frame_of = np.zeros(na, np.int32)
    _check(_bound().debug_accl_world(int(device), scene.ref(), C.byref(lv), _dp(world), frame_of.ctypes.data_as(_abi.c_i32p)),
           "oicc_debug_stab_accl_world")
    return world, frame_of


def applied_zoom(frame_t, required_zoom, frame_status, options):
    """Step 4 of the model alone, on the host (needs no device): (zoom [frames], zoom_clamped [frames] uint8)."""
    t = np.ascontiguousarray(frame_t, dtype=np.float64).ravel()
    z = np.ascontiguousarray(required_zoom, dtype=np.float64).ravel()
    st = np.ascontiguousarray(frame_status, dtype=np.int32).ravel()
    if not (len(t) == len(z) == len(st)):
        raise ValueError("frame_t, required_zoom and frame_status differ in length")
    Z = np.zeros(max(len(t), 1)); cl = np.zeros(max(len(t), 1), np.uint8)
    o = options.c()
    _check(_bound().debug_zoom(len(t), _dp(t), _dp(z), st.ctypes.data_as(_abi.c_i32p), C.byref(o), _dp(Z), cl.ctypes.data_as(_abi.c_u8p)),
           "oicc_debug_stab_zoom")
    return Z, cl


def _plan_arrays(scene, correction_q, zoom):
    q = np.ascontiguousarray(correction_q, dtype=np.float64).reshape(-1, 4)
    z = np.ascontiguousarray(zoom, dtype=np.float64).ravel()
    if len(q) != scene.num_frames or len(z) != scene.num_frames:
        raise ValueError("%d corrections and %d zooms for %d frames" % (len(q), len(z), scene.num_frames))
    return q, z


def stab_map(scene, correction_q, zoom, device=0, return_evaluations=False, return_ms=False):
    """Per-frame stabilised maps for the frames of this scene, as rolling_shutter.rs_rectify_map: (map [frames, dst_h, dst_w, 2]
    float32, valid [frames, dst_h, dst_w] uint8, frame_status [frames], valid counts [frames]); then evaluations and (table, record,
    map kernel) milliseconds where asked for."""
    q, z = _plan_arrays(scene, correction_q, zoom)
    dw, dh = scene.dst_size
    shape = (max(scene.num_frames, 1), max(dh, 1), max(dw, 1))
    mapxy = np.zeros(shape + (2,), np.float32)
    valid = np.zeros(shape, np.uint8)
    evals = np.zeros(shape, np.uint8) if return_evaluations else None
    status = np.zeros(shape[0], np.int32); num = np.zeros(shape[0], np.int64); ms = np.zeros(3)
    _check(_bound().map(int(device), scene.ref(), _dp(q), _dp(z), mapxy.ctypes.data_as(_abi.c_fp), valid.ctypes.data_as(_abi.c_u8p),
                        None if evals is None else evals.ctypes.data_as(_abi.c_u8p), status.ctypes.data_as(_abi.c_i32p),
                        num.ctypes.data_as(_abi.c_i64p), _dp(ms)), "oicc_stab_map")
    out = (mapxy, valid, status, num)
    if return_evaluations:
        out += (evals,)
    if return_ms:
        out += (ms,)
    return out


def stab_frames(frames, scene, correction_q, zoom, border_value=0, batch=DEFAULT_BATCH, device=0, report=None):
    """Stabilised u8 frames [n, h, w] or [n, h, w, c] (c 1 or 3), one per scene.frame_t, and frame_status [n].  numpy in -> numpy out
    (pinned staging, two batches in flight); a CUDA torch.uint8 tensor in -> a CUDA tensor out, the work on torch's current stream.
    Frames whose status is not 0 come back as border_value.  report: a dict that receives the milliseconds of the host route."""
    q, z = _plan_arrays(scene, correction_q, zoom)
    if _is_cuda_tensor(frames):
        return _frames_tensor(frames, scene, q, z, border_value)
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim not in (3, 4):
        raise ValueError("frames must be uint8 [n, h, w] or [n, h, w, c]")
    F = np.ascontiguousarray(frames)
    n, h, w = F.shape[:3]
    c = 1 if F.ndim == 3 else F.shape[3]
    if n != scene.num_frames or (w, h) != scene.src_size:
        raise ValueError("frames %r do not match the scene (%d frames of %d x %d)" % ((F.shape, scene.num_frames) + scene.src_size))
    dw, dh = scene.dst_size
    out = np.zeros((n, dh, dw) + (() if F.ndim == 3 else (c,)), np.uint8)
    status = np.zeros(n, np.int32)
    rep = _abi.RsFramesReport()
    _check(_bound().frames(int(device), scene.ref(), _dp(q), _dp(z), int(c), F.ctypes.data_as(_abi.c_u8p), int(border_value), int(batch),
                           out.ctypes.data_as(_abi.c_u8p), status.ctypes.data_as(_abi.c_i32p), C.byref(rep)), "oicc_stab_frames")
    if report is not None:
        report.update(rep.as_dict())
    return out, status


def _frames_tensor(frames, scene, q, z, border_value):
    import torch
    if not frames.is_cuda or frames.dtype != torch.uint8 or frames.dim() not in (3, 4):
        raise ValueError("frames must be a CUDA uint8 tensor [n, h, w] or [n, h, w, c]")
    F = frames.contiguous()
    n, h, w = int(F.shape[0]), int(F.shape[1]), int(F.shape[2])
    c = 1 if F.dim() == 3 else int(F.shape[3])
    if n != scene.num_frames or (w, h) != scene.src_size:
        raise ValueError("frames %r do not match the scene (%d frames of %d x %d)" % ((tuple(F.shape), scene.num_frames) + scene.src_size))
    dw, dh = scene.dst_size
    out = torch.empty((n, dh, dw) + (() if F.dim() == 3 else (c,)), dtype=torch.uint8, device=F.device)
    status = np.zeros(n, np.int32)
    with torch.cuda.device(F.device):
        stream = torch.cuda.current_stream(F.device).cuda_stream
        _check(_bound().frames_device(C.c_void_p(stream), scene.ref(), _dp(q), _dp(z), c, C.cast(F.data_ptr(), _abi.c_u8p), int(border_value),
                                      C.cast(out.data_ptr(), _abi.c_u8p), status.ctypes.data_as(_abi.c_i32p)), "oicc_stab_frames_device")
    return out, status
