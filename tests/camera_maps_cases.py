"""Cases shared by the CPU and GPU tests of the camera maps: pixel sets, map cases, remap inputs and the scipy reference of the
model conversion.  Everything here is computed once per process (lru_cache) and must be left unchanged by the tests."""
import functools

import numpy as np

import camera_maps_restatement as R
from openimucameracalibrator_amd import synthetic as S

PRESETS = tuple(S.CAMERAS)
UNPROJECT_SIZES = (1, 63, 64, 65, 257)
MAP_SIZES = ((1, 1), (67, 5), (960, 540))
CONVERSION_PAIRS = (("gopro9_division", S.CAM_EXTENDED_UNIFIED), ("gopro9_division", S.CAM_FISHEYE),
                    ("gopro9_division", S.CAM_PINHOLE_RADIAL_TANGENTIAL), ("gopro6_double_sphere", S.CAM_FISHEYE))
NUM_INTRINSICS = {S.CAM_PINHOLE: 7, S.CAM_PINHOLE_RADIAL_TANGENTIAL: 10, S.CAM_FISHEYE: 9, S.CAM_DIVISION_UNDISTORTION: 5,
                  S.CAM_DOUBLE_SPHERE: 7, S.CAM_EXTENDED_UNIFIED: 7}


def camera(name):
    return R.FOLDING_CAMERA if name == "folding" else S.CAMERAS[name]


def centre(model, intr):
    return (intr[2], intr[3]) if model == S.CAM_DIVISION_UNDISTORTION else (intr[3], intr[4])


@functools.lru_cache(maxsize=None)
def unproject_pixels(name):
    """257 pixels: the principal point, a NaN pixel, the four corners, then random positions in the image."""
    model, intr, w, h = camera(name)
    rng = np.random.RandomState(20241115)
    cx, cy = centre(model, intr)
    head = [[cx, cy], [np.nan, 100.0], [0.0, 0.0], [w - 1.0, 0.0], [0.0, h - 1.0], [w - 1.0, h - 1.0]]
    rest = rng.uniform([0, 0], [w - 1, h - 1], (257 - len(head), 2))
    uv = np.concatenate([np.array(head), rest])
    uv.setflags(write=False)
    return uv


def rotation_y(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


def shifted(model, intr, d):
    out = np.array(intr, dtype=np.float64)
    k = 2 if model == S.CAM_DIVISION_UNDISTORTION else 3
    out[k] += d; out[k + 1] += d
    return out


def map_cases():
    """name -> (src camera, dst model, dst intrinsics, R, all_valid): the destination size comes from MAP_SIZES."""
    cases = {}
    for name in PRESETS:
        model, intr, w, h = S.CAMERAS[name]
        # the same camera on both sides; the source image carries a margin of one pixel (principal point moved by (1, 1)), so that
        # no coordinate sits on the image border, where the last bit of the Newton decides the validity: the map is (u + 1, v + 1)
        cases["identity-" + name] = ((model, shifted(model, intr, 1.0), w + 2, h + 2), model, np.asarray(intr, dtype=np.float64), None, True)
        for balance in (0.0, 1.0):
            cases["rectified%d-%s" % (balance, name)] = ((model, intr, w, h), S.CAM_PINHOLE, R.rectified_pinhole(model, intr, w, h, balance),
                                                         None, balance == 0.0)
    model, intr, w, h = S.CAMERAS["gopro9_division"]
    cases["rotated"] = ((model, intr, w, h), S.CAM_PINHOLE, R.rectified_pinhole(model, intr, w, h, 0.0), rotation_y(5.0), False)
    fm, fi, _, _ = S.CAMERAS["gopro6_fisheye"]
    cases["fisheye-destination"] = ((model, intr, w, h), fm, np.asarray(fi, dtype=np.float64), None, False)
    return cases


MAP_CASES = map_cases()


@functools.lru_cache(maxsize=None)
def map_reference(case, size):
    (sm, si, sw, sh), dm, di, Rm, _ = MAP_CASES[case]
    dw, dh = size
    if case.startswith("identity"):
        sw, sh = dw + 2, dh + 2
    out = R.rectify_map(sm, si, sw, sh, dm, di, dw, dh, R=Rm) + ((sw, sh),)
    for a in out[:4]:
        a.setflags(write=False)
    return out


def near_border(raw, sw, sh, tol=1e-6):
    """Pixels whose (unmasked) restatement coordinate lies within tol of the image border: validity may differ there."""
    x, y = raw[..., 0], raw[..., 1]
    with np.errstate(invalid="ignore"):
        return (np.abs(x) < tol) | (np.abs(x - (sw - 1)) < tol) | (np.abs(y) < tol) | (np.abs(y - (sh - 1)) < tol)


def remap_maps():
    """name -> (source size (w, h), map [dh, dw, 2] float32)."""
    rng = np.random.RandomState(7)
    maps = {}
    maps["1x1"] = ((1, 1), np.zeros((1, 1, 2), np.float32))
    w = h = 2
    xs = np.array([0.0, w - 1.0, w - 1.0 + 1e-3, -1e-3, np.nan, 0.5], np.float32)
    ys = np.array([0.0, h - 1.0, h - 1.0 + 1e-3, -1e-3, np.nan, 0.25], np.float32)
    maps["2x2-edges"] = ((2, 2), np.stack(np.meshgrid(xs, ys), -1).astype(np.float32))
    m = rng.uniform([-1.0, -1.0], [67.0, 5.0], (9, 13, 2)).astype(np.float32)
    m[0, 0] = (66.0, 4.0); m[0, 1] = (66.0, 1.5); m[0, 2] = (12.25, 4.0); m[0, 3] = (0.0, 0.0); m[0, 4] = (np.nan, 1.0)
    maps["67x5-to-13x9"] = ((67, 5), m)
    uu, vv = np.meshgrid(np.arange(12, dtype=np.float32), np.arange(7, dtype=np.float32))
    maps["half-pixel-shift"] = ((13, 8), np.stack([uu + 0.5, vv + 0.5], -1).astype(np.float32))
    return maps


REMAP_MAPS = remap_maps()


def remap_frames(name, num_frames, channels):
    """Random u8 frames; the half-pixel case gets a checker of 0 / 255 (exact .5 ties: 127.5)."""
    (w, h), _ = REMAP_MAPS[name]
    rng = np.random.RandomState(100 * num_frames + channels)
    shape = (num_frames, h, w) if channels == 1 else (num_frames, h, w, channels)
    F = rng.randint(0, 256, shape).astype(np.uint8)
    if name == "half-pixel-shift":
        yy, xx = np.mgrid[0:h, 0:w]
        checker = (((xx + yy) % 2) * 255).astype(np.uint8)
        F[0] = checker if channels == 1 else checker[..., None]
    return F


@functools.lru_cache(maxsize=None)
def rendered_views():
    """Two rendered radon views of the gopro9_division preset (images [2, 540, 960] u8)."""
    views = S.render_radon_views("gopro9_division", 2)
    views["images"] = np.ascontiguousarray(views["images"], dtype=np.uint8)
    views["images"].setflags(write=False)
    return views


def conversion_start(model, intr, dst_model):
    intr = np.asarray(intr, dtype=np.float64)
    cx, cy = centre(model, intr)
    out = np.zeros(NUM_INTRINSICS[dst_model])
    out[0], out[1] = intr[0], intr[1]
    if dst_model == S.CAM_DIVISION_UNDISTORTION:
        out[2], out[3] = cx, cy
    else:
        out[3], out[4] = cx, cy
    if dst_model == S.CAM_EXTENDED_UNIFIED:
        out[5], out[6] = 0.5, 1.0
    if dst_model == S.CAM_DOUBLE_SPHERE:
        out[5], out[6] = 0.0, 0.5
    return out


@functools.lru_cache(maxsize=None)
def conversion_reference(src_name, dst_model, stride=8):
    """scipy.optimize.least_squares(method='lm') on the stride-8 grid, every intrinsic but the skew free: dict(intrinsics, rms,
    max) with rms and max over the grid points in px."""
    from scipy.optimize import least_squares
    model, intr, w, h = S.CAMERAS[src_name]
    uv = R.pixel_grid(w, h, stride)
    xy, status = R.unproject(model, intr, uv)
    keep = status == 0
    p = np.concatenate([xy[keep], np.ones((int(keep.sum()), 1))], 1)
    uvk = uv[keep]
    x0 = conversion_start(model, intr, dst_model)
    free = [k for k in range(len(x0)) if not (dst_model != S.CAM_DIVISION_UNDISTORTION and k == 2)]

    def full(x):
        q = x0.copy(); q[free] = x
        return q

    def res(x):
        with np.errstate(all="ignore"):
            px, ok = S.project(dst_model, full(x), p)
        r = (px - uvk)
        r[~np.asarray(ok, dtype=bool)] = 1e6
        return r.ravel()

    sol = least_squares(res, x0[free], method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale="jac", max_nfev=4000)
    r = res(sol.x).reshape(-1, 2)
    d = np.hypot(r[:, 0], r[:, 1])
    out = dict(intrinsics=full(sol.x), rms=float(np.sqrt((d ** 2).mean())), max=float(d.max()), points=int(len(d)))
    out["intrinsics"].setflags(write=False)
    return out


def grid_rms(src_name, dst_model, dst_intr, stride=8):
    """rms over the stride grid of |project_dst(ray) - pixel| for given destination intrinsics (numpy, float64)."""
    model, intr, w, h = S.CAMERAS[src_name]
    uv = R.pixel_grid(w, h, stride)
    xy, status = R.unproject(model, intr, uv)
    keep = status == 0
    p = np.concatenate([xy[keep], np.ones((int(keep.sum()), 1))], 1)
    px, _ = S.project(dst_model, np.asarray(dst_intr, dtype=np.float64), p)
    return float(np.sqrt(((px - uv[keep]) ** 2).sum(-1).mean()))
