"""numpy specification of the camera maps (csrc/camera_maps.hip, include/oicc_hip.h "camera maps"): pixel -> ray by Newton with
the analytic Jacobian and the principal-branch test, the rectification map, the discrepancy of two models, the bilinear remap in
its fixed order, and the rectified pinhole.  Forward models: synthetic.project.  Jacobians: closed forms of this file.  It does
not import the library.  `dtype` numpy.longdouble runs the same steps in extended precision (the yardstick of the GPU tests)."""
import numpy as np

from openimucameracalibrator_amd import synthetic as S

NEWTON_STEPS = 20
STEP_TOL = 1e-13
REPROJECTION_TOL = 1e-9

FOLDING_CAMERA = (S.CAM_PINHOLE_RADIAL_TANGENTIAL, [450.0, 1.0, 0.0, 480.0, 270.0, -0.3, 0.0, 0.0, 0.0, 0.0], 960, 540)
FOLD_RADIUS_PX = 450.0 * np.sqrt(1.0 / 0.9) * (1.0 - 0.3 / 0.9)       # 316.2278: r* = sqrt(1 / (3 * 0.3)), f r* (1 - 0.3 r*^2)


def _centre(model, intr):
    return (intr[2], intr[3]) if model == S.CAM_DIVISION_UNDISTORTION else (intr[3], intr[4])


def jacobian_xy(model, intr, x, y):
    """A = d project(x, y, 1) / d(x, y) as (A00, A01, A10, A11), closed forms."""
    intr = np.asarray(intr, dtype=np.float64)
    one = np.ones_like(x)
    if model == S.CAM_DIVISION_UNDISTORTION:
        f, a, _, _, k = intr[:5]
        fy = f * a
        ux, uy = f * x, fy * y
        r2 = ux * ux + uy * uy
        inner = 1.0 - 4.0 * k * r2
        ident = (np.abs(2.0 * k * r2) < np.finfo(np.float64).eps) | (inner < 0)
        sq = np.sqrt(np.where(ident, one, inner))
        sp = 1.0 + sq
        sc = np.where(ident, one, 2.0 / sp)
        dsc = np.where(ident, 0.0 * one, 4.0 * k / (sq * sp * sp))
        a00, a01, a11 = sc + 2.0 * dsc * ux * ux, 2.0 * dsc * ux * uy, sc + 2.0 * dsc * uy * uy
        return a00 * f, a01 * fy, a01 * f, a11 * fy
    f, a, skew = intr[0], intr[1], intr[2]
    r2 = x * x + y * y
    if model in (S.CAM_PINHOLE, S.CAM_PINHOLE_RADIAL_TANGENTIAL):
        if model == S.CAM_PINHOLE:
            k1, k2, k3, t1, t2 = intr[5], intr[6], 0.0, 0.0, 0.0
        else:
            k1, k2, k3, t1, t2 = intr[5:10]
        d = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        dd = k1 + r2 * (2.0 * k2 + 3.0 * k3 * r2)
        dxx = d + 2.0 * x * x * dd + 2.0 * t1 * y + 6.0 * t2 * x
        dxy = 2.0 * x * y * dd + 2.0 * t1 * x + 2.0 * t2 * y
        dyx = dxy
        dyy = d + 2.0 * y * y * dd + 2.0 * t2 * x + 6.0 * t1 * y
    elif model == S.CAM_FISHEYE:
        small = r2 < 1e-8
        r2s = np.where(small, one, r2)
        r = np.sqrt(r2s)
        th = np.arctan2(r, one)
        t2 = th * th
        thd = th * (1 + intr[5] * t2 + intr[6] * t2**2 + intr[7] * t2**3 + intr[8] * t2**4)
        dthd = 1 + 3 * intr[5] * t2 + 5 * intr[6] * t2**2 + 7 * intr[7] * t2**3 + 9 * intr[8] * t2**4
        s = thd / r
        g = (dthd * r / (1.0 + r2s) - thd) / (r2s * r)          # (ds/dr) / r
        dxx = np.where(small, one, s + g * x * x)
        dxy = np.where(small, 0.0 * one, g * x * y)
        dyx = dxy
        dyy = np.where(small, one, s + g * y * y)
    elif model == S.CAM_DOUBLE_SPHERE:
        xi, al = intr[5], intr[6]
        d1 = np.sqrt(r2 + 1.0)
        kk = xi * d1 + 1.0
        d2 = np.sqrt(r2 + kk * kk)
        nrm = al * d2 + (1 - al) * kk
        kx, ky = xi * x / d1, xi * y / d1
        nx = al * (x + kk * kx) / d2 + (1 - al) * kx
        ny = al * (y + kk * ky) / d2 + (1 - al) * ky
        dxx, dxy = 1.0 / nrm - x * nx / nrm**2, -x * ny / nrm**2
        dyx, dyy = -y * nx / nrm**2, 1.0 / nrm - y * ny / nrm**2
    elif model == S.CAM_EXTENDED_UNIFIED:
        al, be = intr[5], intr[6]
        rho = np.sqrt(be * r2 + 1.0)
        nrm = al * rho + (1 - al)
        nx, ny = al * be * x / rho, al * be * y / rho
        dxx, dxy = 1.0 / nrm - x * nx / nrm**2, -x * ny / nrm**2
        dyx, dyy = -y * nx / nrm**2, 1.0 / nrm - y * ny / nrm**2
    else:
        raise ValueError("unknown camera model %r" % (model,))
    fa = f * a
    return f * dxx + skew * dyx, f * dxy + skew * dyy, fa * dyx, fa * dyy


def _project_xy(model, intr, x, y):
    p = np.stack([x, y, np.ones_like(x)], -1)
    with np.errstate(all="ignore"):
        px, ok = S.project(model, intr, p)
    return px[..., 0], px[..., 1], np.asarray(ok, dtype=bool)


def unproject(model, intr, uv, dtype=np.float64):
    """(xy [n, 2], status [n] uint8): the Newton of camera_unproject_kernel, every pixel stopping on its own."""
    intr = np.asarray(intr, dtype=np.float64)
    uv = np.asarray(uv, dtype=dtype).reshape(-1, 2)
    u, v = uv[:, 0].copy(), uv[:, 1].copy()
    f, fa = dtype(intr[0]), dtype(intr[0]) * dtype(intr[1])
    cx, cy = _centre(model, intr)
    with np.errstate(all="ignore"):
        x, y = (u - dtype(cx)) / f, (v - dtype(cy)) / fa
        active = np.ones(len(u), dtype=bool)
        failed = np.zeros(len(u), dtype=bool)
        for _ in range(NEWTON_STEPS):
            if not active.any():
                break
            px, py, ok = _project_xy(model, intr, x, y)
            failed |= active & ~ok
            active &= ok
            a00, a01, a10, a11 = jacobian_xy(model, intr, x, y)
            ex, ey = px - u, py - v
            det = a00 * a11 - a01 * a10
            dx = (a11 * ex - a01 * ey) / det
            dy = (a00 * ey - a10 * ex) / det
            x = np.where(active, x - dx, x)
            y = np.where(active, y - dy, y)
            step = np.maximum(np.abs(dx), np.abs(dy))
            active &= step > STEP_TOL * (1.0 + np.maximum(np.abs(x), np.abs(y)))
        px, py, ok = _project_xy(model, intr, x, y)
        a00, a01, a10, a11 = jacobian_xy(model, intr, x, y)
        err = np.maximum(np.abs(px - u), np.abs(py - v))
        det = a00 * a11 - a01 * a10
        tr = a00 / f + a11 / fa
        good = (~failed & ok & np.isfinite(x) & np.isfinite(y) & np.isfinite(err) & np.isfinite(det) & np.isfinite(tr)
                & (err <= REPROJECTION_TOL * (1.0 + np.maximum(np.abs(u), np.abs(v)))) & (det > 0) & (tr > 0))
    xy = np.stack([np.where(good, x, np.nan), np.where(good, y, np.nan)], -1)
    return xy, (~good).astype(np.uint8)


def pixel_grid(w, h, stride=1, dtype=np.float64):
    uu, vv = np.meshgrid(np.arange(0, w, stride, dtype=dtype), np.arange(0, h, stride, dtype=dtype))
    return np.stack([uu.ravel(), vv.ravel()], -1)


def is_plain_pinhole(model, intr):
    return model == S.CAM_PINHOLE and intr[5] == 0.0 and intr[6] == 0.0


def rectify_map(src_model, src_intr, src_w, src_h, dst_model, dst_intr, dst_w, dst_h, R=None, dtype=np.float64):
    """(map [dst_h, dst_w, 2] float32, valid [dst_h, dst_w] uint8, coordinates [dst_h, dst_w, 2] before the rounding to float32,
    the projections [dst_h, dst_w, 2] before the validity test: what a pixel near the image border is judged by)."""
    dst_intr = np.asarray(dst_intr, dtype=np.float64)
    uv = pixel_grid(dst_w, dst_h, dtype=dtype)
    if is_plain_pinhole(dst_model, dst_intr):
        y = (uv[:, 1] - dtype(dst_intr[4])) / (dtype(dst_intr[0]) * dtype(dst_intr[1]))
        x = (uv[:, 0] - dtype(dst_intr[3]) - dtype(dst_intr[2]) * y) / dtype(dst_intr[0])
        ok = np.ones(len(x), dtype=bool)
    else:
        xy, status = unproject(dst_model, dst_intr, uv, dtype=dtype)
        x, y, ok = xy[:, 0], xy[:, 1], status == 0
    Rm = np.eye(3) if R is None else np.asarray(R, dtype=np.float64).reshape(3, 3)
    Rm = Rm.astype(dtype)
    with np.errstate(all="ignore"):
        p = np.stack([(Rm[k, 0] * x + Rm[k, 1] * y) + Rm[k, 2] for k in range(3)], -1)
        ok = ok & (p[:, 2] > 0)
        px, pok = S.project(src_model, src_intr, np.where(ok[:, None], p, dtype(1.0)))
        ok = ok & np.asarray(pok, dtype=bool)
        ok = ok & (px[:, 0] >= 0) & (px[:, 0] <= src_w - 1) & (px[:, 1] >= 0) & (px[:, 1] <= src_h - 1)
    coords = np.where(ok[:, None], px, np.nan)
    return (coords.astype(np.float32).reshape(dst_h, dst_w, 2), ok.astype(np.uint8).reshape(dst_h, dst_w),
            coords.reshape(dst_h, dst_w, 2), np.array(px).reshape(dst_h, dst_w, 2))


def remap_values(frames, mapxy, border_value=0):
    """The bilinear sum before rounding (float64), frames [n, h, w] or [n, h, w, c] u8, map [dh, dw, 2] float32."""
    frames = np.asarray(frames)
    squeeze = frames.ndim == 3
    F = (frames[..., None] if squeeze else frames).astype(np.float64)
    n, h, w, c = F.shape
    m = np.asarray(mapxy, dtype=np.float32)
    mx, my = m[..., 0], m[..., 1]
    with np.errstate(invalid="ignore"):
        inside = (mx >= 0) & (mx <= np.float32(w - 1)) & (my >= 0) & (my <= np.float32(h - 1))
    xf = np.where(inside, mx, 0).astype(np.float64)
    yf = np.where(inside, my, 0).astype(np.float64)
    x0, y0 = np.floor(xf), np.floor(yf)
    a, b = (xf - x0)[None, ..., None], (yf - y0)[None, ..., None]
    ix, iy = x0.astype(np.int64), y0.astype(np.int64)
    ix1 = np.where(xf - x0 != 0, ix + 1, ix)           # a neighbour of weight 0 is not read
    iy1 = np.where(yf - y0 != 0, iy + 1, iy)
    p00, p01, p10, p11 = F[:, iy, ix], F[:, iy, ix1], F[:, iy1, ix], F[:, iy1, ix1]
    val = ((1.0 - a) * (1.0 - b) * p00 + a * (1.0 - b) * p01) + ((1.0 - a) * b * p10 + a * b * p11)
    val = np.where(inside[None, ..., None], val, float(border_value) - 0.0)
    return val[..., 0] if squeeze else val


def remap(frames, mapxy, border_value=0):
    return np.clip(np.floor(remap_values(frames, mapxy, border_value) + 0.5), 0, 255).astype(np.uint8)


def discrepancy(model_a, intr_a, model_b, intr_b, w, h, dtype=np.float64):
    """(count, rms, max) of |project_B(unproject_A(px)) - px| over the pixels of a w x h image."""
    uv = pixel_grid(w, h, dtype=dtype)
    xy, status = unproject(model_a, intr_a, uv, dtype=dtype)
    ok = status == 0
    p = np.concatenate([np.where(ok[:, None], xy, 0.0), np.ones((len(xy), 1), dtype=dtype)], 1)
    with np.errstate(all="ignore"):
        px, pok = S.project(model_b, intr_b, p)
        d2 = ((px - uv) ** 2).sum(-1)
    ok = ok & np.asarray(pok, dtype=bool) & np.isfinite(d2)
    if not ok.any():
        return 0, 0.0, 0.0
    d2 = d2[ok]
    return int(ok.sum()), float(np.sqrt(d2.sum() / len(d2))), float(np.sqrt(d2.max()))


def border_pixels(w, h):
    """(left and right columns, top and bottom rows) of a w x h image as pixel lists."""
    v = np.arange(h, dtype=np.float64); u = np.arange(w, dtype=np.float64)
    cols = np.concatenate([np.stack([np.zeros(h), v], -1), np.stack([np.full(h, w - 1.0), v], -1)])
    rows = np.concatenate([np.stack([u, np.zeros(w)], -1), np.stack([u, np.full(w, h - 1.0)], -1)])
    return cols, rows


def rectified_pinhole(model, intr, w, h, balance=0.0):
    """Intrinsics of the distortion-free PINHOLE of the same size: f between 'every destination pixel sees the source'
    (balance 0) and 'every source border pixel is kept' (balance 1)."""
    cols, rows = border_pixels(w, h)
    xc, sc = unproject(model, intr, cols)
    xr, sr = unproject(model, intr, rows)
    xc, xr = xc[sc == 0], xr[sr == 0]
    hw, hh = (w - 1) / 2.0, (h - 1) / 2.0
    x_in, y_in = np.abs(xc[:, 0]).min(), np.abs(xr[:, 1]).min()
    both = np.concatenate([xc, xr])
    x_out, y_out = np.abs(both[:, 0]).max(), np.abs(both[:, 1]).max()
    f0 = max(hw / x_in, hh / y_in)
    f1 = min(hw / x_out, hh / y_out)
    f = (1.0 - balance) * f0 + balance * f1
    return np.array([f, 1.0, 0.0, hw, hh, 0.0, 0.0])
