"""Rolling-shutter rectification from gyroscope rates on the GPU (csrc/rolling_shutter.hip, the oicc_rs_* entries of
include/oicc_hip.h; DESIGN.md, "Rolling-shutter rectification").

The spline calibration ends in q_i_c, time_offset_imu_to_cam_s and calib_line_delay_us.  This module uses them for what they are
calibrated for: every destination pixel of a frame looks up the source row it was exposed on and is rotated by the gyro-integrated
orientation between that row's time and the frame's reference time.  Rotation only: translation during the readout (parallax) is
out of scope, and so are fields of view of 180 degrees and more; smoothing between frames is stabilization.py's.  There is no CPU
path: every function raises without the HIP library or a device."""
import ctypes as C

import numpy as np

from . import _abi
from . import camera_calibrator as cc

DEFAULT_BATCH = 16
FRAME_STATUS = {0: "ok", 1: "no gyro coverage", 2: "more than 256 gyro samples in the frame's window"}


def _bound():
    from . import _lib
    return _lib.load_rolling_shutter()       # raises without the HIP library


def _check(rc, name):
    if rc == -1:
        raise ValueError("%s: invalid argument" % name)
    if rc != 0:
        raise RuntimeError("%s failed with %d (no usable HIP device?)" % (name, rc))


def _dp(a):
    return a.ctypes.data_as(_abi.c_dp)


def gyro_ms_matrix(gyro_intrinsics):
    """MS_g of the nine gyroscope intrinsics (six misalignments, three scales), as the device's imu_ms_matrix."""
    g = np.asarray(gyro_intrinsics, dtype=np.float64).ravel()
    if len(g) != 9:
        raise ValueError("gyro_intrinsics holds 9 values (6 misalignments, 3 scales)")
    m, s = g[:6], g[6:]
    return np.array([[s[0], -m[0] * s[1], m[1] * s[2]], [m[3] * s[0], s[1], -m[2] * s[2]], [-m[4] * s[0], m[5] * s[1], s[2]]])


def corrected_gyro(telemetry, gyro_intrinsics=None, gyro_bias=None):
    """(t [n] seconds in the IMU clock, rates [n, 3] = MS_g (omega_m - b) in the IMU frame) of a telemetry dict (timestamps_ns,
    gyroscope), the correction of the gyroscope residual.  None: identity intrinsics, zero bias."""
    t = np.asarray(telemetry["timestamps_ns"], dtype=np.float64) * 1e-9
    w = np.asarray(telemetry["gyroscope"], dtype=np.float64).reshape(-1, 3)
    if len(t) != len(w):
        raise ValueError("telemetry: %d timestamps for %d gyroscope samples" % (len(t), len(w)))
    b = np.zeros(3) if gyro_bias is None else np.asarray(gyro_bias, dtype=np.float64).reshape(3)
    MS = np.eye(3) if gyro_intrinsics is None else gyro_ms_matrix(gyro_intrinsics)
    d = w - b
    return t, np.stack([(MS[r, 0] * d[:, 0] + MS[r, 1] * d[:, 1]) + MS[r, 2] * d[:, 2] for r in range(3)], -1)


def accl_ms_matrix(accl_intrinsics):
    """MS_a of the six accelerometer intrinsics (three misalignments: the upper triangle, three scales), as the device's
    imu_ms_matrix with the lower misalignments 0."""
    a = np.asarray(accl_intrinsics, dtype=np.float64).ravel()
    if len(a) != 6:
        raise ValueError("accl_intrinsics holds 6 values (3 misalignments, 3 scales)")
    return gyro_ms_matrix(np.concatenate([a[:3], np.zeros(3), a[3:]]))


def corrected_accl(telemetry, accl_intrinsics=None, accl_bias=None):
    """(t [n] seconds in the IMU clock, accl [n, 3] = MS_a (a_m - b_a) in the IMU frame, m/s^2: up at rest) of a telemetry dict
    (timestamps_ns, accelerometer), the correction of the accelerometer residual, in corrected_gyro's order.  None: identity
    intrinsics, zero bias."""
    t = np.asarray(telemetry["timestamps_ns"], dtype=np.float64) * 1e-9
    a = np.asarray(telemetry["accelerometer"], dtype=np.float64).reshape(-1, 3)
    if len(t) != len(a):
        raise ValueError("telemetry: %d timestamps for %d accelerometer samples" % (len(t), len(a)))
    b = np.zeros(3) if accl_bias is None else np.asarray(accl_bias, dtype=np.float64).reshape(3)
    MS = np.eye(3) if accl_intrinsics is None else accl_ms_matrix(accl_intrinsics)
    d = a - b
    return t, np.stack([(MS[r, 0] * d[:, 0] + MS[r, 1] * d[:, 1]) + MS[r, 2] * d[:, 2] for r in range(3)], -1)


class Scene:
    """Everything the entries share: source and destination camera (model, intrinsics, w, h), R (row-major 3 x 3, destination
    camera -> source camera), gyro times [n] (IMU clock) and corrected rates [n, 3] (IMU frame), q_i_c (w, x, y, z),
    time_offset_imu_to_cam, frame_t [frames] (camera clock, row 0), line_delay_s and reference_row (None: (src_h - 1) / 2)."""

    def __init__(self, src, dst, gyro_t, gyro_rates, frame_t, line_delay_s, q_i_c=(1.0, 0.0, 0.0, 0.0), time_offset_imu_to_cam=0.0,
                 reference_row=None, R=None):
        (sm, si, sw, sh), (dm, di, dw, dh) = src, dst
        self.src_intr, self.dst_intr = self._intr(sm, si), self._intr(dm, di)
        self.R9 = None if R is None else np.ascontiguousarray(R, dtype=np.float64).reshape(9)
        self.gyro_t = np.ascontiguousarray(gyro_t, dtype=np.float64).ravel()
        self.gyro_rates = np.ascontiguousarray(gyro_rates, dtype=np.float64).reshape(-1, 3)
        if len(self.gyro_t) != len(self.gyro_rates):
            raise ValueError("%d gyro times for %d rates" % (len(self.gyro_t), len(self.gyro_rates)))
        self.frame_t = np.ascontiguousarray(frame_t, dtype=np.float64).ravel()
        self.num_frames = len(self.frame_t)
        self.src_size, self.dst_size = (int(sw), int(sh)), (int(dw), int(dh))
        self.reference_row = (int(sh) - 1) / 2.0 if reference_row is None else float(reference_row)
        s = _abi.RsScene()
        s.src_model, s.src_w, s.src_h, s.dst_model, s.dst_w, s.dst_h = int(sm), int(sw), int(sh), int(dm), int(dw), int(dh)
        s.src_intr, s.dst_intr = _dp(self.src_intr), _dp(self.dst_intr)
        s.R9 = None if self.R9 is None else _dp(self.R9)
        s.num_gyro, s.gyro_t, s.gyro_rates = len(self.gyro_t), _dp(self.gyro_t), _dp(self.gyro_rates)
        s.q_i_c = (C.c_double * 4)(*[float(x) for x in np.asarray(q_i_c, dtype=np.float64).ravel()])
        s.time_offset_imu_to_cam = float(time_offset_imu_to_cam)
        s.num_frames, s.frame_t = self.num_frames, _dp(self.frame_t)
        s.line_delay_s, s.reference_row = float(line_delay_s), self.reference_row
        self.c = s                       # the arrays above keep its pointers alive

    @staticmethod
    def _intr(model, intr):
        intr = np.ascontiguousarray(intr, dtype=np.float64).ravel()
        if model not in cc.NUM_INTRINSICS or len(intr) != cc.NUM_INTRINSICS[model]:
            raise ValueError("camera model %r does not take %d intrinsics" % (model, len(intr)))
        return intr

    def ref(self):
        return C.byref(self.c)


def rs_rectify_map(scene, device=0, return_evaluations=False, return_ms=False):
    """Per-frame maps: (map [frames, dst_h, dst_w, 2] float32 source coordinates, valid [frames, dst_h, dst_w] uint8, frame_status
    [frames] int32, valid counts [frames]); then evaluations [frames, dst_h, dst_w] uint8 and (table, ray, map kernel) milliseconds
    where asked for."""
    dw, dh = scene.dst_size
    shape = (max(scene.num_frames, 1), max(dh, 1), max(dw, 1))
    mapxy = np.zeros(shape + (2,), np.float32)
    valid = np.zeros(shape, np.uint8)
    evals = np.zeros(shape, np.uint8) if return_evaluations else None
    status = np.zeros(shape[0], np.int32); num = np.zeros(shape[0], np.int64); ms = np.zeros(3)
    _check(_bound().rectify_map(int(device), scene.ref(), mapxy.ctypes.data_as(_abi.c_fp), valid.ctypes.data_as(_abi.c_u8p),
                                None if evals is None else evals.ctypes.data_as(_abi.c_u8p), status.ctypes.data_as(_abi.c_i32p),
                                num.ctypes.data_as(_abi.c_i64p), _dp(ms)), "oicc_rs_rectify_map")
    out = (mapxy, valid, status, num)
    if return_evaluations:
        out += (evals,)
    if return_ms:
        out += (ms,)
    return out


def _is_cuda_tensor(x):
    return type(x).__module__.startswith("torch") and hasattr(x, "is_cuda")


def rs_rectify_frames(frames, scene, border_value=0, batch=DEFAULT_BATCH, device=0, report=None):
    """Rectified u8 frames [n, h, w] or [n, h, w, c] (c 1 or 3), one per scene.frame_t, and frame_status [n].  numpy in -> numpy out
    (pinned staging, two batches in flight); a CUDA torch.uint8 tensor in -> a CUDA tensor out, the work on torch's current stream,
    without copies of the frames.  Frames whose status is not 0 come back as border_value.  report: a dict that receives the
    milliseconds of the host route."""
    if _is_cuda_tensor(frames):
        return _rectify_tensor(frames, scene, border_value)
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
    _check(_bound().rectify_frames(int(device), scene.ref(), int(c), F.ctypes.data_as(_abi.c_u8p), int(border_value), int(batch),
                                   out.ctypes.data_as(_abi.c_u8p), status.ctypes.data_as(_abi.c_i32p), C.byref(rep)), "oicc_rs_rectify_frames")
    if report is not None:
        report.update(rep.as_dict())
    return out, status


def _rectify_tensor(frames, scene, border_value):
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
        _check(_bound().rectify_frames_device(C.c_void_p(stream), scene.ref(), c, C.cast(F.data_ptr(), _abi.c_u8p), int(border_value),
                                              C.cast(out.data_ptr(), _abi.c_u8p), status.ctypes.data_as(_abi.c_i32p)),
               "oicc_rs_rectify_frames_device")
    return out, status


def _queries(entry, name, scene, frame_index, values, width_in, width_out, device):
    frame_index = np.ascontiguousarray(frame_index, dtype=np.int32).ravel()
    values = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, width_in)
    n = len(frame_index)
    if len(values) != n:
        raise ValueError("%d frame indices for %d queries" % (n, len(values)))
    out = np.zeros((n, width_out)); status = np.zeros(n, np.uint8); frame_status = np.zeros(max(scene.num_frames, 1), np.int32)
    ms = C.c_double(0.0)
    if n:
        _check(entry(int(device), scene.ref(), n, frame_index.ctypes.data_as(_abi.c_i32p), _dp(values), _dp(out),
                     status.ctypes.data_as(_abi.c_u8p), frame_status.ctypes.data_as(_abi.c_i32p), C.byref(ms)), name)
    return out, status, frame_status


def rs_rectify_points(scene, frame_index, xy, device=0):
    """Observed pixels xy [n, 2] of frames frame_index [n] as the global-shutter destination camera sees them: (xy [n, 2] float64,
    status [n] uint8: 0 a point, 1 none, 2 the frame's status is not 0 -- NaN for both --, frame_status [frames])."""
    return _queries(_bound().rectify_points, "oicc_rs_rectify_points", scene, frame_index, xy, 2, 2, device)


def rs_row_rotations(scene, frame_index, rows, device=0):
    """R_rel at (frame, row) as quaternions (w, x, y, z): (q [n, 4], status [n] uint8: 0, or 2 with NaN, frame_status [frames])."""
    return _queries(_bound().row_rotations, "oicc_rs_row_rotations", scene, frame_index, rows, 1, 4, device)
