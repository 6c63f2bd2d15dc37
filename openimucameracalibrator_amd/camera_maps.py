"""Camera maps: pixel -> ray, rectification maps, image resampling and model conversion on the GPU (csrc/camera_maps.hip, the
oicc_camera_* entries of include/oicc_hip.h; DESIGN.md, "Camera maps").

The chain of this package ends in cam_calib.json, one of six camera models.  This module turns that camera into what the next
tool accepts: undistorted frames (undistort_frames) and the same camera in another model with the pixels that costs
(convert_camera_model).  There is no CPU path: every function raises without the HIP library or a device.  Rays are (x, y, 1),
so fields of view of 180 degrees and more are out of scope."""
import ctypes as C

import numpy as np

from . import _abi
from . import camera_calibrator as cc
from . import synthetic as S

DEFAULT_BATCH = 16
INTRINSICS_WITHOUT_SKEW = cc.ALL & ~cc.SKEW


def _bound():
    from . import _lib
    return _lib.load_camera_maps()       # raises without the HIP library


def _check(rc, name):
    if rc == -1:
        raise ValueError("%s: invalid argument" % name)
    if rc != 0:
        raise RuntimeError("%s failed with %d (no usable HIP device?)" % (name, rc))


def _intr(model, intr):
    intr = np.ascontiguousarray(intr, dtype=np.float64).ravel()
    if model not in cc.NUM_INTRINSICS or len(intr) != cc.NUM_INTRINSICS[model]:
        raise ValueError("camera model %r does not take %d intrinsics" % (model, len(intr)))
    return intr


def _dp(a):
    return a.ctypes.data_as(_abi.c_dp)


def unproject(model, intr, uv, device=0, return_ms=False):
    """Rays (x, y, 1) of the pixels uv [n, 2]: (xy [n, 2], status [n] uint8; 0 a ray, 1 none on the principal branch, xy NaN)."""
    intr = _intr(model, intr)
    uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
    n = len(uv)
    xy = np.zeros((n, 2)); status = np.zeros(n, np.uint8)
    ms = C.c_double(0.0)
    if n:
        _check(_bound().unproject(int(device), int(model), _dp(intr), len(intr), n, _dp(uv), _dp(xy), status.ctypes.data_as(_abi.c_u8p),
                                  C.byref(ms)), "oicc_camera_unproject")
    return (xy, status, ms.value) if return_ms else (xy, status)


def rectify_map(src_model, src_intr, src_w, src_h, dst_model, dst_intr, dst_w, dst_h, R=None, device=0, return_ms=False):
    """(map [dst_h, dst_w, 2] float32 source coordinates (x, y), valid [dst_h, dst_w] uint8, number of valid pixels).  R: row-major
    3 x 3, destination camera -> source camera."""
    src_intr, dst_intr = _intr(src_model, src_intr), _intr(dst_model, dst_intr)
    R9 = None if R is None else np.ascontiguousarray(R, dtype=np.float64).reshape(9)
    mapxy = np.zeros((max(int(dst_h), 1), max(int(dst_w), 1), 2), np.float32)
    valid = np.zeros(mapxy.shape[:2], np.uint8)
    num = C.c_int64(0); ms = C.c_double(0.0)
    _check(_bound().rectify_map(int(device), int(src_model), _dp(src_intr), int(src_w), int(src_h), int(dst_model), _dp(dst_intr),
                                int(dst_w), int(dst_h), None if R9 is None else _dp(R9), mapxy.ctypes.data_as(_abi.c_fp),
                                valid.ctypes.data_as(_abi.c_u8p), C.byref(num), C.byref(ms)), "oicc_camera_rectify_map")
    return (mapxy, valid, num.value, ms.value) if return_ms else (mapxy, valid, num.value)


def discrepancy(model_a, intr_a, model_b, intr_b, w, h, device=0):
    """Every pixel of a w x h image through camera A to a ray and through camera B back: dict(count, rms, max) of the distance."""
    intr_a, intr_b = _intr(model_a, intr_a), _intr(model_b, intr_b)
    stats = np.zeros(3)
    _check(_bound().discrepancy(int(device), int(model_a), _dp(intr_a), int(model_b), _dp(intr_b), int(w), int(h), _dp(stats), None),
           "oicc_camera_discrepancy")
    return dict(count=int(stats[0]), rms=float(stats[1]), max=float(stats[2]))


def _is_cuda_tensor(x):
    return type(x).__module__.startswith("torch") and hasattr(x, "is_cuda")


def remap(frames, mapxy, border_value=0, batch=DEFAULT_BATCH, device=0, report=None):
    """Bilinear resampling of u8 frames [n, h, w] or [n, h, w, c] (c 1 or 3) through one map [dh, dw, 2] float32.  numpy in ->
    numpy out (pinned staging, two batches in flight); a CUDA torch.uint8 tensor in -> a CUDA tensor out on torch's current
    stream, without copies (the map may be a tensor on the same device or an array).  report: a dict that receives ms_upload,
    ms_kernel, ms_download and ms_total of the host route."""
    if _is_cuda_tensor(frames):
        return _remap_tensor(frames, mapxy, border_value)
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim not in (3, 4):
        raise ValueError("frames must be uint8 [n, h, w] or [n, h, w, c]")
    F = np.ascontiguousarray(frames)
    n, h, w = F.shape[:3]
    c = 1 if F.ndim == 3 else F.shape[3]
    m = np.ascontiguousarray(mapxy, dtype=np.float32)
    if m.ndim != 3 or m.shape[2] != 2:
        raise ValueError("map must be [dst_h, dst_w, 2]")
    dh, dw = m.shape[:2]
    out = np.zeros((n, dh, dw) + (() if F.ndim == 3 else (c,)), np.uint8)
    rep = _abi.CameraRemapReport()
    _check(_bound().remap(int(device), n, w, h, c, F.ctypes.data_as(_abi.c_u8p), m.ctypes.data_as(_abi.c_fp), dw, dh,
                          int(border_value), int(batch), out.ctypes.data_as(_abi.c_u8p), C.byref(rep)), "oicc_camera_remap")
    if report is not None:
        report.update(rep.as_dict())
    return out


def _remap_tensor(frames, mapxy, border_value):
    import torch
    if not frames.is_cuda or frames.dtype != torch.uint8 or frames.dim() not in (3, 4):
        raise ValueError("frames must be a CUDA uint8 tensor [n, h, w] or [n, h, w, c]")
    F = frames.contiguous()
    n, h, w = F.shape[:3]
    c = 1 if F.dim() == 3 else F.shape[3]
    if _is_cuda_tensor(mapxy):
        m = mapxy.to(device=F.device, dtype=torch.float32).contiguous()
    else:
        m = torch.from_numpy(np.ascontiguousarray(mapxy, dtype=np.float32)).to(F.device)
    if m.dim() != 3 or m.shape[2] != 2:
        raise ValueError("map must be [dst_h, dst_w, 2]")
    dh, dw = int(m.shape[0]), int(m.shape[1])
    out = torch.empty((n, dh, dw) + (() if F.dim() == 3 else (c,)), dtype=torch.uint8, device=F.device)
    with torch.cuda.device(F.device):
        stream = torch.cuda.current_stream(F.device).cuda_stream
        _check(_bound().remap_device(C.c_void_p(stream), int(n), int(w), int(h), int(c), C.cast(F.data_ptr(), _abi.c_u8p),
                                     C.cast(m.data_ptr(), _abi.c_fp), dw, dh, int(border_value),
                                     C.cast(out.data_ptr(), _abi.c_u8p)), "oicc_camera_remap_device")
    return out


def border_pixels(w, h):
    """(left and right columns, top and bottom rows) of a w x h image as pixel lists."""
    v = np.arange(h, dtype=np.float64); u = np.arange(w, dtype=np.float64)
    cols = np.concatenate([np.stack([np.zeros(h), v], -1), np.stack([np.full(h, w - 1.0), v], -1)])
    rows = np.concatenate([np.stack([u, np.zeros(w)], -1), np.stack([u, np.full(w, h - 1.0)], -1)])
    return cols, rows


def rectified_pinhole(model, intr, w, h, balance=0.0, device=0):
    """Intrinsics of a distortion-free PINHOLE of the same size with its principal point at ((w - 1) / 2, (h - 1) / 2).

    The rays of the four border lines of the source image are unprojected on the device (pixels without a ray are ignored).
    With hw = (w - 1) / 2, hh = (h - 1) / 2:  f0 = max(hw / x_in, hh / y_in), f1 = min(hw / x_out, hh / y_out), where x_in is the
    smallest |x| over the left and right columns, y_in the smallest |y| over the top and bottom rows, x_out and y_out the
    largest |x| and |y| over the whole border;  f = (1 - balance) f0 + balance f1.  balance = 0 makes every destination pixel
    valid for barrel-type cameras (the six presets of synthetic.CAMERAS); it is no promise for pincushion or folding lenses.
    balance = 1 keeps the whole source border and leaves destination pixels without a source.  rectify_map always returns
    the valid count."""
    cols, rows = border_pixels(w, h)
    xy, status = unproject(model, intr, np.concatenate([cols, rows]), device=device)
    xc, sc, xr, sr = xy[:len(cols)], status[:len(cols)], xy[len(cols):], status[len(cols):]
    xc, xr = xc[sc == 0], xr[sr == 0]
    if not len(xc) or not len(xr):
        raise ValueError("the image border has no rays")
    hw, hh = (w - 1) / 2.0, (h - 1) / 2.0
    x_in, y_in = np.abs(xc[:, 0]).min(), np.abs(xr[:, 1]).min()
    both = np.concatenate([xc, xr])
    x_out, y_out = np.abs(both[:, 0]).max(), np.abs(both[:, 1]).max()
    with np.errstate(divide="ignore"):
        f0 = max(hw / x_in, hh / y_in)
        f1 = min(hw / x_out, hh / y_out)
    f = (1.0 - balance) * f0 + balance * f1
    if not np.isfinite(f) or f <= 0:
        raise ValueError("the image is too small for a rectified pinhole (%d x %d)" % (w, h))
    return np.array([f, 1.0, 0.0, hw, hh, 0.0, 0.0])


def undistort_frames(frames, model, intr, dst=None, balance=0.0, R=None, border_value=0, batch=DEFAULT_BATCH, device=0):
    """The map once, then remap: (frames, (dst_model, dst_intr, dst_w, dst_h), valid mask [dst_h, dst_w] bool).  dst: a destination
    camera (model, intrinsics, w, h); None = rectified_pinhole(model, intr, w, h, balance)."""
    h, w = int(frames.shape[1]), int(frames.shape[2])
    if dst is None:
        dst = (S.CAM_PINHOLE, rectified_pinhole(model, intr, w, h, balance, device=device), w, h)
    dst_model, dst_intr, dst_w, dst_h = dst
    mapxy, valid, _ = rectify_map(model, intr, w, h, dst_model, dst_intr, dst_w, dst_h, R=R, device=device)
    out = remap(frames, mapxy, border_value=border_value, batch=batch, device=device)
    return out, (dst_model, np.asarray(dst_intr, dtype=np.float64), int(dst_w), int(dst_h)), valid.astype(bool)


def conversion_start(model, intr, dst_model):
    """Start values of the fit: f, aspect and principal point of the source, zero distortion except EXTENDED_UNIFIED (alpha, beta) =
    (0.5, 1) and DOUBLE_SPHERE (xi, alpha) = (0, 0.5)."""
    intr = np.asarray(intr, dtype=np.float64)
    cx, cy = (intr[2], intr[3]) if model == S.CAM_DIVISION_UNDISTORTION else (intr[3], intr[4])
    out = np.zeros(cc.NUM_INTRINSICS[dst_model])
    out[0], out[1] = intr[0], intr[1]
    if dst_model == S.CAM_DIVISION_UNDISTORTION:
        out[2], out[3] = cx, cy
    else:
        out[3], out[4] = cx, cy
    if dst_model == S.CAM_EXTENDED_UNIFIED:
        out[5], out[6] = 0.5, 1.0
    elif dst_model == S.CAM_DOUBLE_SPHERE:
        out[5], out[6] = 0.0, 0.5
    return out


def conversion_grid(w, h, stride):
    """(uv [rows * columns, 2] row by row, columns, rows): the pixels u = 0, stride, ..., v = 0, stride, ...; a grid row is a view."""
    us = np.arange(0, w, stride, dtype=np.float64); vs = np.arange(0, h, stride, dtype=np.float64)
    uu, vv = np.meshgrid(us, vs)
    return np.stack([uu.ravel(), vv.ravel()], -1), len(us), len(vs)


def convert_camera_model(model, intr, w, h, dst_model, stride=8, intrinsics_to_optimize=INTRINSICS_WITHOUT_SKEW, max_iterations=200,
                         device=0):
    """The same camera in another model: the rays of a pixel grid (unprojected on the device) are the scene points (x, y, 1, 1) of
    a view bundle adjustment with identity, constant poses -- one view per grid row --, whose only variables are the destination
    model's intrinsics; huber_width lies beyond every residual, so the fit is plain least squares.  Then the discrepancy over the
    FULL-resolution image.  Returns dict(model, intrinsics, fit_rms_px, full_image_rms_px, full_image_max_px, valid_pixels,
    grid_points)."""
    intr = _intr(model, intr)
    uv, nu, nv = conversion_grid(w, h, stride)
    xy, status = unproject(model, intr, uv, device=device)
    keep = status == 0
    if keep.sum() < 2 * cc.NUM_INTRINSICS[dst_model]:
        raise ValueError("too few pixels with a ray for the fit (%d)" % keep.sum())
    row = np.repeat(np.arange(nv), nu)[keep]
    rows_used = np.unique(row)
    off = np.concatenate([[0], np.cumsum([np.sum(row == r) for r in rows_used])]).astype(np.int64)
    pts = np.concatenate([xy[keep], np.ones((int(keep.sum()), 2))], 1)
    ba = cc.ViewBundleAdjuster(device=device)
    ba.SetOption("huber_width", 1e30)                 # beyond every residual: the loss is out of play
    ba.SetOption("function_tolerance", 1e-16)
    ba.SetOption("parameter_tolerance", 1e-14)
    ba.SetOption("gradient_tolerance", 1e-16)
    ba.SetCamera(dst_model, conversion_start(model, intr, dst_model))
    ba.SetScenePoints(pts)
    ba.SetViews(np.zeros((len(rows_used), 6)), off, uv[keep], np.arange(len(pts), dtype=np.int32))
    summary = ba.Optimize(int(max_iterations), 0, cc.intrinsics_mask(dst_model, intrinsics_to_optimize))
    out = ba.GetCamera()
    fit_rms = float(np.sqrt(2.0 * summary["final_cost"] / len(pts)))
    d = discrepancy(model, intr, dst_model, out, w, h, device=device)
    return dict(model=dst_model, intrinsics=out, fit_rms_px=fit_rms, full_image_rms_px=d["rms"], full_image_max_px=d["max"],
                valid_pixels=d["count"], grid_points=int(len(pts)), summary=summary)
