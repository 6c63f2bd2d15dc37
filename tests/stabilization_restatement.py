"""numpy specification of the stabilisation (csrc/stabilization.hip, include/oicc_hip.h "stabilisation"): the orientation path of
a clip, the smooth camera on SO(3), the required and the applied zoom, the stabilised maps.  Quaternions, the interval exponential,
frame windows, tables and the fixed point on the source row are rolling_shutter_restatement's (imported, not copied).  It does not
import the library.  `dtype` numpy.longdouble runs the same steps in extended precision (the yardstick of the tests); what the host
of the library decides by time comparisons (who is on the path, the windows) is decided in float64 either way."""
import copy

import numpy as np

import rolling_shutter_restatement as RS

MEAN_ITERATIONS = 16
MEAN_TOL = 1e-12
MARCH = 32
BISECTIONS = 16
MIN_RUN = 4
SCAN_LANES = 256


def qnormalized(q):
    n = np.sqrt(((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3])
    return q / n[..., None]


def qlog(q):
    """Log of quaternions of any norm as rotation vectors, the shorter way round."""
    q = np.where(q[..., :1] < 0, -q, q)
    v = q[..., 1:]
    n = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    small = n < 1e-8
    k = np.where(small, 2 / q[..., 0], 2 * np.arctan2(n, q[..., 0]) / np.where(small, 1, n))
    return k[..., None] * v


def qexp(v):
    th = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    half = th / 2
    small = th < 1e-8
    k = np.where(small, 0.5 - th * th / 48, np.sin(half) / np.where(small, 1, th))
    return np.concatenate([np.cos(half)[..., None], k[..., None] * v], -1)


def check_scene(sc):
    dm, di = sc.dst[0], np.asarray(sc.dst[1], dtype=np.float64)
    assert RS.R.is_plain_pinhole(dm, di), "the destination is a plain PINHOLE"
    assert np.all(np.diff(sc.frame_t) > 0), "frame times strictly increase"


# ---------------------------------------------------------------- 1. path
def on_path(sc):
    """(first, count, interval [frames]) by time comparisons in float64: tau_j = ((t_j - t_k) + offset) - reference delay."""
    refd = sc.reference_row * sc.line_delay
    n = len(sc.gyro_t)
    flags = np.zeros(len(sc.frame_t), bool); interval = np.zeros(len(sc.frame_t), np.int64)
    for k, tk in enumerate(sc.frame_t):
        tau = ((sc.gyro_t - tk) + sc.offset) - refd
        if tau[0] > 0 or tau[-1] < 0:
            continue
        flags[k] = True
        interval[k] = min(int(np.searchsorted(tau, 0, side="right")) - 1, n - 2)
    idx = np.where(flags)[0]
    if not len(idx):
        return 0, 0, interval
    assert np.array_equal(idx, np.arange(idx[0], idx[-1] + 1))
    return int(idx[0]), len(idx), interval


def deltas(sc, dtype=np.float64):
    """D_k [count - 1, 4] = Q(t_ref,k)^-1 Q(t_ref,k+1) for the consecutive on-path frames, chained from the left."""
    first, count, interval = on_path(sc)
    t = sc.gyro_t.astype(dtype); om = sc.rates.astype(dtype); ft = sc.frame_t.astype(dtype)
    off, refd = dtype(sc.offset), dtype(sc.reference_row) * dtype(sc.line_delay)
    out = np.zeros((max(count - 1, 0), 4), dtype)
    for i in range(count - 1):
        k = first + i
        ja, jb = int(interval[k]), int(max(interval[k + 1], interval[k]))
        sa = dtype(0) - (((t[ja] - ft[k]) + off) - refd)
        sb = dtype(0) - (((t[jb] - ft[k + 1]) + off) - refd)
        dta = t[ja + 1] - t[ja]
        q = RS.qconj(RS.interval_exp(om[ja], om[ja + 1], dta, sa))
        if ja == jb:
            q = RS.qmul(q, RS.interval_exp(om[ja], om[ja + 1], dta, sb))
        else:
            q = RS.qmul(q, RS.interval_exp(om[ja], om[ja + 1], dta, dta))
            for j in range(ja + 1, jb):
                dt = t[j + 1] - t[j]
                q = RS.qmul(q, RS.interval_exp(om[j], om[j + 1], dt, dt))
            q = RS.qmul(q, RS.interval_exp(om[jb], om[jb + 1], t[jb + 1] - t[jb], sb))
        out[i] = q
    return out


def path(sc, dtype=np.float64):
    """path_q [frames, 4]: the left-to-right product over the on-path frames, each normalised once at the end; NaN off the path."""
    first, count, _ = on_path(sc)
    D = deltas(sc, dtype)
    out = np.full((len(sc.frame_t), 4), np.nan, dtype)
    q = np.array([1, 0, 0, 0], dtype)
    for i in range(count):
        if i:
            q = RS.qmul(q, D[i - 1])
        out[first + i] = qnormalized(q)
    return out


def scan_run(count):
    """Frames per lane of the device's scan (stab_path_scan_kernel)."""
    return max(MIN_RUN, -(-count // SCAN_LANES))


# ---------------------------------------------------------------- 2. smooth camera
def windows(sc, sigma):
    """(lo [frames], hi [frames]) frame indices, both included, of the on-path frames m with |frame_t[m] - frame_t[k]| <= 3 sigma."""
    first, count, _ = on_path(sc)
    t = sc.frame_t
    lo = np.zeros(len(t), np.int32); hi = np.zeros(len(t), np.int32)
    for k in range(first, first + count):
        m = np.arange(first, first + count)
        inside = m[np.abs(t[m] - t[k]) <= 3.0 * sigma]
        lo[k], hi[k] = inside[0], inside[-1]
    return lo, hi


def _wave_sum(a):
    """The device's butterfly over 64 lanes (lane l adds lane l ^ d, d = 32 .. 1); a [64, ...] -> the total every lane ends with."""
    idx = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        a = a + a[idx ^ d]
    return a[0]


def _lane_sums(values):
    """values [members, ...] -> [64, ...]: lane l sums the members l, l + 64, ... in that order."""
    out = np.zeros((64,) + values.shape[1:], values.dtype)
    for b in range(0, len(values), 64):
        chunk = values[b:b + 64]
        out[:len(chunk)] = out[:len(chunk)] + chunk
    return out


def smooth(sc, path_q, sigma, max_correction=0.0, dtype=np.float64):
    """(smooth_q [frames, 4], correction_q [frames, 4], iterations [frames]); off the path NaN, the identity, 0."""
    first, count, _ = on_path(sc)
    lo, hi = windows(sc, sigma)
    F = len(sc.frame_t)
    S_out = np.full((F, 4), np.nan, dtype); C_out = np.zeros((F, 4), dtype); C_out[:, 0] = 1
    its = np.zeros(F, np.int32)
    ft = sc.frame_t.astype(dtype)
    for k in range(first, first + count):
        qk = path_q[k]
        S_out[k] = qk
        if not (sigma > 0 and hi[k] > lo[k]):
            continue
        m = np.arange(lo[k], hi[k] + 1)
        dt = ft[m] - ft[k]
        w = np.exp(-(dt * dt) / (dtype(2) * (dtype(sigma) * dtype(sigma))))
        sw = _wave_sum(_lane_sums(w))
        S = qk
        it = 0
        while it < MEAN_ITERATIONS:
            v = qlog(RS.qmul(RS.qconj(S)[None], path_q[m]))
            mean = _wave_sum(_lane_sums(w[:, None] * v)) / sw
            S = RS.qmul(S, qexp(mean))
            it += 1
            if np.sqrt((mean[0] * mean[0] + mean[1] * mean[1]) + mean[2] * mean[2]) <= MEAN_TOL:
                break
        S = qnormalized(S)
        C = qnormalized(RS.qmul(RS.qconj(qk), S))
        if C[0] < 0:
            C = -C
        n = np.sqrt((C[1] * C[1] + C[2] * C[2]) + C[3] * C[3])
        if max_correction > 0 and 2 * np.arctan2(n, C[0]) > max_correction:
            h = dtype(max_correction) / 2
            C = np.concatenate([[np.cos(h)], (np.sin(h) / n) * C[1:]]).astype(dtype)
        S_out[k], C_out[k], its[k] = S, C, it
    return S_out, C_out, its


def correction_angle(C):
    C = np.asarray(C)
    return 2 * np.arctan2(np.sqrt((C[..., 1:] ** 2).sum(-1)), np.abs(C[..., 0]))


# ---------------------------------------------------------------- records and per-frame scenes
def frame_matrix(sc, c, dtype=np.float64):
    """M_k = R(C_k) R9 in the kernel's order."""
    Cm = RS.qmat(np.asarray(c, dtype=dtype))
    Rm = sc.Rm.astype(dtype)
    return np.array([[(Cm[i, 0] * Rm[0, j] + Cm[i, 1] * Rm[1, j]) + Cm[i, 2] * Rm[2, j] for j in range(3)] for i in range(3)], dtype)


def frame_scene(sc, k, c, zoom, dtype=np.float64):
    """The one-frame rolling-shutter scene whose map is frame k's stabilised map: R9 = M_k, the destination's focal length and skew
    times the zoom (float64 products: one rounding each)."""
    one = copy.copy(sc)
    dm, di, dw, dh = sc.dst
    di = np.array(di, dtype=np.float64)
    di[0] = di[0] * float(zoom); di[2] = di[2] * float(zoom)
    one.dst = (dm, di, dw, dh)
    one.frame_t = sc.frame_t[k:k + 1]
    one.Rm = frame_matrix(sc, c, dtype)
    return one


def stab_pixels(sc, correction_q, zoom, dtype=np.float64, frames=None):
    """Per frame what rolling_shutter_restatement.rectify_pixels gives for frame_scene: (coordinates [frames, pixels, 2] before the
    rounding to float32, valid [frames, pixels] uint8, frame_status [frames], raw projections)."""
    check_scene(sc)
    F = len(sc.frame_t)
    n = sc.dst[2] * sc.dst[3]
    coords = np.full((F, n, 2), np.nan, dtype); valid = np.zeros((F, n), np.uint8); status = np.zeros(F, np.int32); raw = np.zeros((F, n, 2), dtype)
    for k in (range(F) if frames is None else frames):
        c, v, fs, r, _ = RS.rectify_pixels(frame_scene(sc, k, correction_q[k], zoom[k], dtype), dtype)
        coords[k], valid[k], status[k], raw[k] = c[0], v[0], fs[0], r[0]
    if frames is not None:
        status = RS.frame_windows(sc)[0]
    return coords, valid, status, raw


def stab_map(sc, correction_q, zoom, dtype=np.float64):
    """(map [frames, dst_h, dst_w, 2] float32, valid [frames, dst_h, dst_w] uint8, frame_status)."""
    dw, dh = sc.dst[2], sc.dst[3]
    coords, valid, status, _ = stab_pixels(sc, correction_q, zoom, dtype)
    return coords.astype(np.float32).reshape(len(status), dh, dw, 2), valid.reshape(len(status), dh, dw), status


# ---------------------------------------------------------------- 3. required zoom
def border_pixels(w, h):
    """(u, v) of the border points in the kernel's order: top row, bottom row, left and right column between them."""
    if w == 1 or h == 1:
        i = np.arange(w * h)
        return np.stack([i % w, i // w], -1).astype(np.float64)
    top = np.stack([np.arange(w), np.zeros(w)], -1); bottom = np.stack([np.arange(w), np.full(w, h - 1)], -1)
    left = np.stack([np.zeros(h - 2), np.arange(1, h - 1)], -1); right = np.stack([np.full(h - 2, w - 1), np.arange(1, h - 1)], -1)
    return np.concatenate([top, bottom, left, right]).astype(np.float64)


def required_zoom(sc, correction_q, dtype=np.float64):
    """(z [frames]: 1 / min s, +inf for an invalid centre, NaN without a table; s [frames, points]; marched [frames, points, 33]:
    the validity of the centre and of s = j / 32, j = 1 .. 32, at every border point, whether the march got there or not)."""
    check_scene(sc)
    dm, di, dw, dh = sc.dst
    di = np.asarray(di, dtype=np.float64)
    uv = border_pixels(dw, dh).astype(dtype)
    y = (uv[:, 1] - dtype(di[4])) / (dtype(di[0] * 1.0) * dtype(di[1]))
    x = (uv[:, 0] - dtype(di[3]) - dtype(di[2] * 1.0) * y) / dtype(di[0] * 1.0)
    status, tabs = RS.tables(sc, dtype)
    F, n = len(status), len(uv)
    z = np.full(F, np.nan); s_out = np.full((F, n), np.nan); marched = np.zeros((F, n, MARCH + 1), bool)
    for k in range(F):
        if tabs[k] is None:
            continue
        M = frame_matrix(sc, correction_q[k], dtype)

        def valid_at(s, sel):
            xs, ys = s * x[sel], s * y[sel]
            with np.errstate(all="ignore"):
                p = np.stack([(M[r, 0] * xs + M[r, 1] * ys) + M[r, 2] for r in range(3)], -1)
                return RS.solve_rows(sc, tabs[k], p, p[:, 2] > 0, dtype)[1]

        everyone = np.arange(n)
        marched[k, :, 0] = valid_at(np.zeros(n, dtype), everyone)
        for j in range(1, MARCH + 1):
            marched[k, :, j] = valid_at(np.full(n, dtype(j) / dtype(MARCH)), everyone)
        s = np.zeros(n, dtype)
        centre = marched[k, :, 0]
        first_bad = np.where(marched[k, :, 1:].all(1), MARCH + 1, np.argmin(marched[k, :, 1:], axis=1) + 1)      # j of the first invalid sample
        s[centre & (first_bad > MARCH)] = 1
        sel = np.where(centre & (first_bad <= MARCH))[0]
        if len(sel):
            lo = (first_bad[sel] - 1).astype(dtype) / dtype(MARCH); hi = first_bad[sel].astype(dtype) / dtype(MARCH)
            for _ in range(BISECTIONS):
                mid = dtype(0.5) * (lo + hi)
                ok = valid_at(mid, sel)
                lo = np.where(ok, mid, lo); hi = np.where(ok, hi, mid)
            s[sel] = lo
        s_out[k] = s
        with np.errstate(divide="ignore"):
            z[k] = float(1 / s.min())
    return z, s_out, marched


# ---------------------------------------------------------------- 4. applied zoom (float64, the host's order)
def applied_zoom(frame_t, z, status, zoom_mode, zoom_window_s=1.0, max_zoom=np.inf):
    t = np.asarray(frame_t, dtype=np.float64); z = np.asarray(z, dtype=np.float64); ok = np.asarray(status) == 0
    F = len(t)
    Z = np.ones(F)
    if zoom_mode == 1:
        if ok.any():
            Z[:] = z[ok].max()
    elif zoom_mode == 2:
        T, sg = float(zoom_window_s), float(zoom_window_s) / 2.0
        win = [np.where(np.abs(t - t[k]) <= T)[0] for k in range(F)]
        Y = np.array([z[w[ok[w]]].max() if ok[w].any() else 1.0 for w in win])
        for k, w in enumerate(win):
            ymin, ymax = Y[w].min(), Y[w].max()
            if ymin == ymax:
                Z[k] = ymin
                continue
            num = den = 0.0
            for j in w:
                dt = t[j] - t[k]
                g = np.exp(-(dt * dt) / (2.0 * (sg * sg))) if sg > 0 else 1.0
                num += g * Y[j]; den += g
            mean = num / den
            Z[k] = ymax if np.isnan(mean) else min(max(mean, ymin), ymax)
    clamped = (Z > max_zoom).astype(np.uint8)
    return np.where(clamped == 1, max_zoom, Z), clamped


def plan(sc, sigma, max_correction=0.0, zoom_mode=1, zoom_window_s=1.0, max_zoom=np.inf, dtype=np.float64):
    """dict of everything oicc_stab_plan returns (the zoom in float64 from this run's required zoom)."""
    check_scene(sc)
    P = path(sc, dtype)
    S, C, its = smooth(sc, P, sigma, max_correction, dtype)
    z, s, marched = required_zoom(sc, C, dtype)
    status = RS.frame_windows(sc)[0]
    Z, clamped = applied_zoom(sc.frame_t, z, status, zoom_mode, zoom_window_s, max_zoom)
    return dict(path_q=P, smooth_q=S, correction_q=C, iterations=its, required_zoom=z, s=s, marched=marched, frame_status=status, zoom=Z,
                zoom_clamped=clamped)
