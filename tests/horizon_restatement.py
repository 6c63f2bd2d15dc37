"""numpy specification of the horizon lock (csrc/stabilization.hip: stab_accl_world_kernel, stab_level_kernel; include/oicc_hip.h
"stabilisation", steps G1 to G3; DESIGN.md, "Horizon lock").  Path, smooth camera, zoom and quaternions are
stabilization_restatement's (imported, not copied).  It does not import the library.  `dtype` numpy.longdouble runs the same steps
in extended precision (the yardstick of the tests); what the host of the library decides by time comparisons (the frame and the
gyro interval of a sample, the gravity windows) is decided in float64 either way.  The gate is the device's: decided in `dtype`."""
import math

import numpy as np

import rolling_shutter_restatement as RS
import stabilization_restatement as SR

SIN10 = 0.17364817766693033          # the float64 next to sin(10 deg) and sin(20 deg): the constants of the kernel
SIN20 = 0.3420201433256687
PI = 3.141592653589793
TWO_PI = 6.283185307179586


class Level:
    """oicc_stab_level: accelerometer times [na] (IMU clock), corrected specific force [na, 3] (IMU frame, m/s^2, up at rest)."""

    def __init__(self, accl_t, accl, gravity_sigma_s=1.0, gravity_const=9.811104, accl_gate=0.0, lock=1.0, roll_rad=0.0):
        self.accl_t = np.asarray(accl_t, dtype=np.float64)
        self.accl = np.asarray(accl, dtype=np.float64).reshape(-1, 3)
        self.sigma, self.g, self.gate, self.lock, self.roll = float(gravity_sigma_s), float(gravity_const), float(accl_gate), float(lock), float(roll_rad)


def sample_times(sc, lv, k):
    """s_jk [na] = ((accl_t[j] - frame_t[k]) + offset) - reference delay, float64."""
    return ((lv.accl_t - sc.frame_t[k]) + sc.offset) - sc.reference_row * sc.line_delay


def sample_frames(sc, lv):
    """(frame_of [na]: the last on-path frame with s_jk >= 0, -1 for a sample before the first on-path reference time or behind the
    last one; interval [na]: the last gyro interval i <= n - 2 with tau_i(k) <= s_jk) by time comparisons in float64."""
    first, count, _ = SR.on_path(sc)
    na, n = len(lv.accl_t), len(sc.gyro_t)
    frame_of = np.full(na, -1, np.int32); interval = np.zeros(na, np.int64)
    if count == 0:
        return frame_of, interval
    refd = sc.reference_row * sc.line_delay
    S = np.stack([sample_times(sc, lv, k) for k in range(first, first + count)])           # [count, na]
    inside = (S[0] >= 0) & ~(S[-1] > 0)
    for j in np.where(inside)[0]:
        k = first + int(np.where(S[:, j] >= 0)[0][-1])
        tau = ((sc.gyro_t - sc.frame_t[k]) + sc.offset) - refd
        frame_of[j] = k
        interval[j] = min(int(np.searchsorted(tau, S[k - first, j], side="right")) - 1, n - 2)
    return frame_of, interval


def camera_vectors(v, q_i_c, dtype=np.float64):
    """R(q_i_c)^T v in the order of the kernel, q_i_c normalised first in float64 (as the host does for the rates)."""
    q = np.asarray(q_i_c, dtype=np.float64)
    q = q / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    M = RS.qmat(q).astype(dtype)
    v = np.asarray(v).astype(dtype)
    return np.stack([(M[0, c] * v[:, 0] + M[1, c] * v[:, 1]) + M[2, c] * v[:, 2] for c in range(3)], -1)


def rotate(q, v):
    """R(q) v, rows summed from the left."""
    M = RS.qmat(q)
    return np.stack([(M[..., r, 0] * v[..., 0] + M[..., r, 1] * v[..., 1]) + M[..., r, 2] * v[..., 2] for r in range(3)], -1)


def gate(lv, dtype=np.float64):
    """g_j [na] bool: | |a_j| - gravity_const | <= accl_gate, or no gate."""
    a = lv.accl.astype(dtype)
    norm = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
    if lv.gate == 0:
        return np.ones(len(a), bool)
    return np.abs(norm - dtype(lv.g)) <= dtype(lv.gate)


def accl_world(sc, lv, q_i_c, path_q=None, dtype=np.float64):
    """G1: (world [na, 3], frame_of [na], q [na, 4] the orientation at the sample): NaN and -1 for the unused samples."""
    first, count, frame_interval = SR.on_path(sc)
    P = SR.path(sc, dtype) if path_q is None else path_q
    frame_of, interval = sample_frames(sc, lv)
    t = sc.gyro_t.astype(dtype); om = sc.rates.astype(dtype); ft = sc.frame_t.astype(dtype); at = lv.accl_t.astype(dtype)
    off, refd = dtype(sc.offset), dtype(sc.reference_row) * dtype(sc.line_delay)
    cam = camera_vectors(lv.accl, q_i_c, dtype)
    na = len(at)
    world = np.full((na, 3), np.nan, dtype); Q = np.full((na, 4), np.nan, dtype)
    for j in range(na):
        k = int(frame_of[j])
        if k < 0:
            continue
        ja, jb = int(frame_interval[k]), int(max(interval[j], frame_interval[k]))
        s = ((at[j] - ft[k]) + off) - refd
        sa = dtype(0) - (((t[ja] - ft[k]) + off) - refd)
        sb = s - (((t[jb] - ft[k]) + off) - refd)
        dta = t[ja + 1] - t[ja]
        q = RS.qconj(RS.interval_exp(om[ja], om[ja + 1], dta, sa))
        if ja == jb:
            q = RS.qmul(q, RS.interval_exp(om[ja], om[ja + 1], dta, sb))
        else:
            q = RS.qmul(q, RS.interval_exp(om[ja], om[ja + 1], dta, dta))
            for i in range(ja + 1, jb):
                dt = t[i + 1] - t[i]
                q = RS.qmul(q, RS.interval_exp(om[i], om[i + 1], dt, dt))
            q = RS.qmul(q, RS.interval_exp(om[jb], om[jb + 1], t[jb + 1] - t[jb], sb))
        Q[j] = SR.qnormalized(RS.qmul(P[k], q))
        world[j] = rotate(Q[j], cam[j])
    return world, frame_of, Q


def windows(sc, lv):
    """(lo [frames], hi [frames]) sample indices, both included (hi < lo: empty), of the used samples with |s_jk| <= 3 sigma_g."""
    first, count, _ = SR.on_path(sc)
    frame_of, _ = sample_frames(sc, lv)
    F = len(sc.frame_t)
    lo = np.zeros(F, np.int32); hi = np.full(F, -1, np.int32)
    for k in range(first, first + count):
        inside = np.where((frame_of >= 0) & (np.abs(sample_times(sc, lv, k)) <= 3.0 * lv.sigma))[0]
        if len(inside):
            lo[k], hi[k] = inside[0], inside[-1]
            assert hi[k] - lo[k] + 1 == len(inside)
    return lo, hi


def wrap(d, dtype):
    """Into (-pi, pi], for |d| <= 2 pi."""
    if d > dtype(PI):
        d = d - dtype(TWO_PI)
    if d <= -dtype(PI):
        d = d + dtype(TWO_PI)
    return d


def correction_of(p, L, max_correction, dtype):
    C = SR.qnormalized(RS.qmul(RS.qconj(p), L))
    if C[0] < 0:
        C = -C
    n = np.sqrt((C[1] * C[1] + C[2] * C[2]) + C[3] * C[3])
    if max_correction > 0 and 2 * np.arctan2(n, C[0]) > max_correction:
        h = dtype(max_correction) / 2
        C = np.concatenate([[np.cos(h)], (np.sin(h) / n) * C[1:]]).astype(dtype)
    return C


def level(sc, lv, path_q, smooth_q, correction_q, world, max_correction=0.0, dtype=np.float64):
    """G2: dict(level_q [frames, 4], correction_q [frames, 4], up [frames, 3], roll, level_angle, gravity [frames, 3] the mean in the
    world, gravity_samples, level_status [frames]).  Off the path: NaN, the correction as given, 0 samples, status 2."""
    first, count, _ = SR.on_path(sc)
    lo, hi = windows(sc, lv)
    F = len(sc.frame_t)
    g = gate(lv, dtype).astype(dtype)
    L_out = np.array(smooth_q, dtype=dtype); C_out = np.array(correction_q, dtype=dtype)
    up = np.full((F, 3), np.nan, dtype); roll = np.full(F, np.nan, dtype); angle = np.zeros(F, dtype); mean = np.full((F, 3), np.nan, dtype)
    samples = np.zeros(F, np.int32); status = np.full(F, 2, np.int32)
    ft = sc.frame_t.astype(dtype); at = lv.accl_t.astype(dtype)
    off, refd = dtype(sc.offset), dtype(sc.reference_row) * dtype(sc.line_delay)
    den = dtype(2) * (dtype(lv.sigma) * dtype(lv.sigma))
    roll_wanted = dtype(math.remainder(lv.roll, TWO_PI))
    for k in range(first, first + count):
        m = np.arange(lo[k], hi[k] + 1)
        if not len(m):
            continue
        s = ((at[m] - ft[k]) + off) - refd
        w = np.exp(-(s * s) / den) * g[m]
        u = np.where(g[m, None] > 0, world[m], 0)
        sums = SR._wave_sum(SR._lane_sums(np.concatenate([w[:, None], w[:, None] * u, g[m, None]], 1)))
        samples[k] = int(sums[4])
        if samples[k] == 0:
            continue
        gm = sums[1:4] / sums[0]
        norm = np.sqrt((gm[0] * gm[0] + gm[1] * gm[1]) + gm[2] * gm[2])
        mean[k] = gm
        if norm < dtype(0.5) * dtype(lv.g):
            continue
        nrm = gm / norm
        M = RS.qmat(smooth_q[k])
        nu = np.array([(M[0, c] * nrm[0] + M[1, c] * nrm[1]) + M[2, c] * nrm[2] for c in range(3)], dtype)
        h = np.sqrt(nu[0] * nu[0] + nu[1] * nu[1])
        rho = np.arctan2(nu[0], -nu[1])
        up[k], roll[k] = nu, rho
        if h < dtype(SIN10):
            status[k] = 1
            continue
        status[k] = 0
        fade = min(max((h - dtype(SIN10)) / (dtype(SIN20) - dtype(SIN10)), dtype(0)), dtype(1))
        theta = (dtype(lv.lock) * fade) * wrap(rho - roll_wanted, dtype)
        if theta == 0:
            continue
        angle[k] = theta
        half = theta / 2
        Lq = SR.qnormalized(RS.qmul(smooth_q[k], np.array([np.cos(half), 0, 0, np.sin(half)], dtype)))
        L_out[k] = Lq
        C_out[k] = correction_of(path_q[k], Lq, max_correction, dtype)
    return dict(level_q=L_out, correction_q=C_out, up=up, roll=roll, level_angle=angle, gravity=mean, gravity_samples=samples, level_status=status)


def plan(sc, lv, q_i_c, sigma, max_correction=0.0, zoom_mode=1, zoom_window_s=1.0, max_zoom=np.inf, dtype=np.float64, zoom=True):
    """dict of everything oicc_stab_plan_level returns (G3: the zoom of stabilization_restatement from the levelled correction)."""
    SR.check_scene(sc)
    P = SR.path(sc, dtype)
    S_, C, its = SR.smooth(sc, P, sigma, max_correction, dtype)
    world, frame_of, _ = accl_world(sc, lv, q_i_c, P, dtype)
    out = level(sc, lv, P, S_, C, world, max_correction, dtype)
    out.update(path_q=P, smooth_q=S_, iterations=its, world=world, frame_of=frame_of, frame_status=RS.frame_windows(sc)[0])
    if zoom:
        z, s, marched = SR.required_zoom(sc, out["correction_q"], dtype)
        Z, clamped = SR.applied_zoom(sc.frame_t, z, out["frame_status"], zoom_mode, zoom_window_s, max_zoom)
        out.update(required_zoom=z, zoom=Z, zoom_clamped=clamped)
    return out
