"""Deterministic synthetic calibration datasets.

Independent numpy forward model (analytic IMU trajectory, planar ChArUco-like
board, the six camera projections) used to synthesise corners and IMU samples
for tests and bench.py -- the reference's datasets are Google-Drive downloads
and there is no network.  This file does not use the spline code: the trajectory
is a sum of sinusoids, so the calibration problem is realistic (the spline has to
approximate it) and the generator is independent of both the HIP path and the
CPU checker.

Conventions follow the reference: T_w_c = T_w_i * T_i_c
(ceres_calib_split_residuals.h:356), accel = R_w_i^T (p'' + g) (:90), gyro =
body angular velocity (:143-144), quaternion memory order (x,y,z,w).
"""
from dataclasses import dataclass, field
import numpy as np

SEED = 20241115

CAM_PINHOLE = 0
CAM_PINHOLE_RADIAL_TANGENTIAL = 1
CAM_FISHEYE = 2
CAM_DIVISION_UNDISTORTION = 4
CAM_DOUBLE_SPHERE = 5
CAM_EXTENDED_UNIFIED = 6


# ----------------------------------------------------------------- small SO(3)
def hat(v):
    v = np.asarray(v, dtype=np.float64)
    z = np.zeros(v.shape[:-1])
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1),
                     np.stack([v[..., 2], z, -v[..., 0]], -1),
                     np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def so3_exp_mat(w):
    """Rodrigues, batched: w[...,3] -> R[...,3,3]."""
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w, axis=-1)[..., None, None]
    W = hat(w)
    W2 = W @ W
    small = th < 1e-8
    ths = np.where(small, 1.0, th)
    a = np.where(small, 1.0 - th**2 / 6.0, np.sin(ths) / ths)
    b = np.where(small, 0.5 - th**2 / 24.0, (1.0 - np.cos(ths)) / ths**2)
    return np.eye(3) + a * W + b * W2


def so3_right_jacobian(w):
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w, axis=-1)[..., None, None]
    W = hat(w)
    W2 = W @ W
    small = th < 1e-6
    ths = np.where(small, 1.0, th)
    a = np.where(small, 0.5 - th**2 / 24.0, (1.0 - np.cos(ths)) / ths**2)
    b = np.where(small, 1.0 / 6.0 - th**2 / 120.0, (ths - np.sin(ths)) / ths**3)
    return np.eye(3) - a * W + b * W2


def quat_from_mat(R):
    """R[...,3,3] -> unit quaternion (x,y,z,w), w >= 0."""
    R = np.asarray(R, dtype=np.float64)
    out = np.empty(R.shape[:-2] + (4,))
    Rf = R.reshape(-1, 3, 3)
    of = out.reshape(-1, 4)
    for i, m in enumerate(Rf):
        tr = m[0, 0] + m[1, 1] + m[2, 2]
        if tr > 0:
            s = np.sqrt(tr + 1.0) * 2
            q = [(m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s, 0.25 * s]
        elif m[0, 0] > m[1, 1] and m[0, 0] > m[2, 2]:
            s = np.sqrt(1.0 + m[0, 0] - m[1, 1] - m[2, 2]) * 2
            q = [0.25 * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s, (m[2, 1] - m[1, 2]) / s]
        elif m[1, 1] > m[2, 2]:
            s = np.sqrt(1.0 + m[1, 1] - m[0, 0] - m[2, 2]) * 2
            q = [(m[0, 1] + m[1, 0]) / s, 0.25 * s, (m[1, 2] + m[2, 1]) / s, (m[0, 2] - m[2, 0]) / s]
        else:
            s = np.sqrt(1.0 + m[2, 2] - m[0, 0] - m[1, 1]) * 2
            q = [(m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, 0.25 * s, (m[1, 0] - m[0, 1]) / s]
        q = np.asarray(q)
        if q[3] < 0:
            q = -q
        of[i] = q / np.linalg.norm(q)
    return out


def mat_from_quat(q):
    q = np.asarray(q, dtype=np.float64)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1 - 2 * (y * y + z * z); R[..., 0, 1] = 2 * (x * y - z * w); R[..., 0, 2] = 2 * (x * z + y * w)
    R[..., 1, 0] = 2 * (x * y + z * w); R[..., 1, 1] = 1 - 2 * (x * x + z * z); R[..., 1, 2] = 2 * (y * z - x * w)
    R[..., 2, 0] = 2 * (x * z - y * w); R[..., 2, 1] = 2 * (y * z + x * w); R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


# ------------------------------------------------------------ camera models
def project(model, intr, p):
    """Batched numpy projection p[...,3] -> (px[...,2], ok[...]).  Formulas as in
    SURVEY.md 8a row A13 (TheiaSfM CameraToPixelCoordinates)."""
    intr = np.asarray(intr, dtype=np.float64)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    ok = np.ones(x.shape, dtype=bool)
    if model == CAM_DIVISION_UNDISTORTION:
        f, a, cx, cy, k = intr[:5]
        ux, uy = f * x / z, f * a * y / z
        r2 = ux * ux + uy * uy
        denom = 2.0 * k * r2
        inner = 1.0 - 4.0 * k * r2
        ident = (np.abs(denom) < np.finfo(np.float64).eps) | (inner < 0)
        scale = np.where(ident, 1.0, (1.0 - np.sqrt(np.where(inner < 0, 0.0, inner))) / np.where(ident, 1.0, denom))
        return np.stack([ux * scale + cx, uy * scale + cy], -1), ok
    f, a, skew, cx, cy = intr[:5]
    if model == CAM_PINHOLE:
        nx, ny = x / z, y / z
        r2 = nx * nx + ny * ny
        d = 1.0 + r2 * (intr[5] + intr[6] * r2)
        dx, dy = nx * d, ny * d
    elif model == CAM_PINHOLE_RADIAL_TANGENTIAL:
        nx, ny = x / z, y / z
        r2 = nx * nx + ny * ny
        k1, k2, k3, t1, t2 = intr[5:10]
        d = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        dx = nx * d + 2 * t1 * nx * ny + t2 * (r2 + 2 * nx * nx)
        dy = ny * d + 2 * t2 * nx * ny + t1 * (r2 + 2 * ny * ny)
    elif model == CAM_FISHEYE:
        r2 = x * x + y * y
        r = np.sqrt(np.maximum(r2, 1e-300))
        th = np.arctan2(r, np.abs(z))
        t2 = th * th
        thd = th * (1 + intr[5] * t2 + intr[6] * t2**2 + intr[7] * t2**3 + intr[8] * t2**4)
        dx = np.where(r2 < 1e-8, x, thd * x / r)
        dy = np.where(r2 < 1e-8, y, thd * y / r)
        flip = (z < 0) & (r2 >= 1e-8)
        dx = np.where(flip, -dx, dx); dy = np.where(flip, -dy, dy)
    elif model == CAM_DOUBLE_SPHERE:
        xi, alpha = intr[5], intr[6]
        r2 = x * x + y * y
        d1 = np.sqrt(r2 + z * z)
        w1 = (1 - alpha) / alpha if alpha > 0.5 else alpha / (1 - alpha)
        w2 = (w1 + xi) / np.sqrt(2 * w1 * xi + xi * xi + 1)
        ok = z > -w2 * d1
        kk = xi * d1 + z
        d2 = np.sqrt(r2 + kk * kk)
        norm = alpha * d2 + (1 - alpha) * kk
        dx, dy = x / norm, y / norm
    elif model == CAM_EXTENDED_UNIFIED:
        alpha, beta = intr[5], intr[6]
        r2 = x * x + y * y
        rho = np.sqrt(beta * r2 + z * z)
        norm = alpha * rho + (1 - alpha) * z
        w = (1 - alpha) / alpha if alpha > 0.5 else alpha / (1 - alpha)
        ok = z > -w * rho
        dx, dy = x / norm, y / norm
    else:
        raise ValueError("unknown camera model %r" % (model,))
    return np.stack([f * dx + skew * dy + cx, f * a * dy + cy], -1), ok


# README intrinsics (Readme.md:33-38) used by the BASELINE configs.
CAMERAS = {
    "gopro9_division": (CAM_DIVISION_UNDISTORTION, [437.13, 1.0, 489.07, 270.87, -1.4386e-06], 960, 540),
    "gopro9_eucm": (CAM_EXTENDED_UNIFIED, [437.97, 1.0, 0.0, 489.47, 272.02, 0.5115, 1.062], 960, 540),
    "gopro6_fisheye": (CAM_FISHEYE, [439.13, 1.0, 0.0, 479.66, 273.19, 0.046, 0.064, -0.10, 0.052], 960, 540),
    "gopro6_double_sphere": (CAM_DOUBLE_SPHERE, [342.43, 1.0, 0.0, 472.60, 273.88, -0.215, 0.5129], 960, 540),
    "pinhole": (CAM_PINHOLE, [450.0, 1.0, 0.0, 480.0, 270.0, -0.05, 0.01], 960, 540),
    "pinhole_radtan": (CAM_PINHOLE_RADIAL_TANGENTIAL, [450.0, 1.0, 0.0, 480.0, 270.0, -0.05, 0.01, 0.001, 5e-4, -3e-4], 960, 540),
}


@dataclass
class Dataset:
    """Everything continuous_time_imu_to_camera_calibration.cc:91-199 reads."""
    name: str
    camera_model: int
    intrinsics: np.ndarray
    image_width: int
    image_height: int
    fps: float
    points: np.ndarray            # [np,4] homogeneous board points
    view_t_s: np.ndarray          # [nv] view timestamps (s)
    view_q_wc: np.ndarray         # [nv,4] initial camera orientation world<-cam (x,y,z,w)
    view_p_wc: np.ndarray         # [nv,3] initial camera position in world
    corner_offset: np.ndarray     # [nv+1] int64
    corner_uv: np.ndarray         # [nc,2]
    corner_point: np.ndarray      # [nc] int32
    imu_t_s: np.ndarray           # [ni]
    accel: np.ndarray             # [ni,3]
    gyro: np.ndarray              # [ni,3]
    dt_so3: float
    dt_r3: float
    std_so3: float
    std_r3: float
    q_i_c_init: np.ndarray        # [4] initial rotation of T_i_c
    line_delay_init: float
    gravity_init: np.ndarray
    truth: dict = field(default_factory=dict)

    @property
    def num_views(self):
        return len(self.view_t_s)

    @property
    def num_corners(self):
        return len(self.corner_point)

    def with_view_order(self, order):
        """The same data set with its views (and their corners) listed in another order -- e.g. the string order of the corner
        file's microsecond keys, in which the reference's application fills its reconstruction."""
        import copy
        order = np.asarray(order)
        d = copy.copy(self)
        d.view_t_s = self.view_t_s[order]; d.view_q_wc = self.view_q_wc[order]; d.view_p_wc = self.view_p_wc[order]
        uv, pt, off = [], [], [0]
        for v in order:
            a, b = self.corner_offset[v], self.corner_offset[v + 1]
            uv.append(self.corner_uv[a:b]); pt.append(self.corner_point[a:b]); off.append(off[-1] + (b - a))
        d.corner_uv = np.concatenate(uv); d.corner_point = np.concatenate(pt).astype(self.corner_point.dtype); d.corner_offset = np.asarray(off, dtype=np.int64)
        return d

    def file_key_order(self):
        """Order of the views as a string-keyed map of their microsecond timestamps lists them (nlohmann::json items())."""
        return np.array(sorted(range(self.num_views), key=lambda v: str(int(round(self.view_t_s[v] * 1e6)))))

    def shard(self, rank, world):
        """Time-contiguous shard of the measurements: rank r owns
        the views and IMU samples of the r-th time window; parameters (knots,
        calibration) stay whole on every rank."""
        t0, t1 = self.view_t_s.min(), self.view_t_s.max() + 1e-9
        edges = np.linspace(t0, t1, world + 1)
        lo, hi = edges[rank], edges[rank + 1]
        vsel = np.where((self.view_t_s >= lo) & (self.view_t_s < hi if rank + 1 < world else self.view_t_s <= hi))[0]
        isel = (self.imu_t_s >= lo) & (self.imu_t_s < hi if rank + 1 < world else self.imu_t_s <= hi + 1.0)
        off = [0]
        uv, pt = [], []
        for v in vsel:
            a, b = self.corner_offset[v], self.corner_offset[v + 1]
            uv.append(self.corner_uv[a:b]); pt.append(self.corner_point[a:b]); off.append(off[-1] + (b - a))
        import copy
        d = copy.copy(self)
        d.shard_view_index = vsel
        d.shard_view_t_s = self.view_t_s[vsel]
        d.shard_corner_offset = np.asarray(off, dtype=np.int64)
        d.shard_corner_uv = np.concatenate(uv) if uv else np.zeros((0, 2))
        d.shard_corner_point = np.concatenate(pt).astype(np.int32) if pt else np.zeros((0,), np.int32)
        d.shard_imu = isel
        return d


def _trajectory(rng, duration):
    """Analytic IMU trajectory: 3 sinusoids per axis (0.3-1.2 Hz), total amplitude
    ~0.15 m / ~0.4 rad."""
    f = rng.uniform(0.3, 1.2, size=(2, 3, 3))
    ph = rng.uniform(0, 2 * np.pi, size=(2, 3, 3))
    amp_p = rng.uniform(0.5, 1.0, size=(3, 3)); amp_p *= 0.15 / amp_p.sum(0, keepdims=True)
    amp_r = rng.uniform(0.5, 1.0, size=(3, 3)); amp_r *= 0.4 / amp_r.sum(0, keepdims=True)
    # slow drift keeps long trajectories (C5, 1000 s) from being periodic
    return dict(f=f, ph=ph, amp_p=amp_p, amp_r=amp_r)


def _eval_traj(tr, t, p0, R_base):
    t = np.asarray(t, dtype=np.float64)[..., None, None]
    w = 2 * np.pi * tr["f"]
    s_p = tr["amp_p"] * np.sin(w[0] * t + tr["ph"][0])
    pos = p0 + s_p.sum(-2)
    acc = (-(w[0] ** 2) * s_p).sum(-2)
    th = (tr["amp_r"] * np.sin(w[1] * t + tr["ph"][1])).sum(-2)
    thd = (tr["amp_r"] * w[1] * np.cos(w[1] * t + tr["ph"][1])).sum(-2)
    R = R_base @ so3_exp_mat(th)
    om = (so3_right_jacobian(th) @ thd[..., None])[..., 0]   # body rate of R_base*exp(theta(t))
    return pos, acc, R, om


def make_dataset(name="C2", num_views=200, corners_per_view=40, duration=20.0, camera="gopro9_division",
                 imu_rate=200.0, dt_so3=0.05, dt_r3=0.1, board=(8, 6), square=0.021, corner_noise_px=0.2,
                 accel_noise=0.21, gyro_noise=0.0156, std_r3=0.25, std_so3=0.02, rolling_shutter=True,
                 pose_noise=(0.002, 0.2), seed=SEED, fps=60.0, gravity=(0.0, 0.0, 9.811104)):
    rng = np.random.RandomState(seed)
    model, intr, W, Hh = CAMERAS[camera]
    intr = np.asarray(intr, dtype=np.float64)
    # board points on z=0, centred
    gx, gy = np.meshgrid(np.arange(board[0]), np.arange(board[1]), indexing="ij")
    pts = np.stack([(gx.ravel() - (board[0] - 1) / 2) * square, (gy.ravel() - (board[1] - 1) / 2) * square,
                    np.zeros(gx.size), np.ones(gx.size)], -1)
    n_pts = len(pts)
    cpv = min(corners_per_view, n_pts)
    # truth calibration (Readme.md:45 style)
    q_ic = np.array([-0.006, -0.7076, 0.7065, 0.0048]); q_ic /= np.linalg.norm(q_ic)   # (x,y,z,w)
    R_ic = mat_from_quat(q_ic)
    t_ic = np.array([0.007, -0.022, 0.001])
    g = np.asarray(gravity, dtype=np.float64)
    R_wc0 = np.diag([1.0, -1.0, -1.0])               # camera looks down the -z world axis at the board
    R_base = R_wc0 @ R_ic.T                           # R_w_i at rest
    # camera 0.25 m above the board: the 0.15 m wide board spans ~260 px of the 960x540 image
    p0 = np.array([0.0, 0.0, 0.25]) - R_base @ t_ic
    tr = _trajectory(rng, duration)
    tr["amp_p"] = tr["amp_p"] * (0.03 / 0.15)         # keep the board inside the image
    tr["amp_r"] = tr["amp_r"] * (0.25 / 0.4)
    ld_true = (1.0 / fps / Hh) if rolling_shutter else 0.0

    view_t = np.arange(num_views, dtype=np.float64) * (duration / num_views)
    X = pts[:, :3]

    def cam_project(tt, sel):
        """Project board points X[sel] as seen at times tt (same shape as sel)."""
        p_i, _, R_wi, _ = _eval_traj(tr, tt, p0, R_base)
        q = np.einsum("...ji,...j->...i", R_wi, X[sel] - p_i)           # R_wi^T (X - p_i)
        pc = np.einsum("ji,...j->...i", R_ic, q - t_ic)
        return project(model, intr, pc)

    # choose corners per view, then observation with rolling-shutter time shift (fixed point)
    sel = np.stack([rng.permutation(n_pts)[:cpv] for _ in range(num_views)])
    sel.sort(axis=1)
    tt = np.repeat(view_t[:, None], cpv, 1)
    uv, ok = cam_project(tt, sel)
    for _ in range(3):
        uv, ok = cam_project(view_t[:, None] + uv[..., 1] * ld_true, sel)
    inimg = ok & (uv[..., 0] > 2) & (uv[..., 0] < W - 2) & (uv[..., 1] > 2) & (uv[..., 1] < Hh - 2)
    uv = uv + rng.normal(0, corner_noise_px, uv.shape)
    counts = inimg.sum(1)
    corner_offset = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    corner_uv = uv[inimg]
    corner_point = sel[inimg].astype(np.int32)

    # initial camera poses (what estimate_camera_poses_from_checkerboard would give): truth + noise
    p_i, _, R_wi, _ = _eval_traj(tr, view_t, p0, R_base)
    R_wc = R_wi @ R_ic
    p_wc = p_i + np.einsum("nij,j->ni", R_wi, t_ic)
    dr = rng.normal(0, np.deg2rad(pose_noise[1]) / np.sqrt(3), (num_views, 3))
    R_wc_n = R_wc @ so3_exp_mat(dr)
    p_wc_n = p_wc + rng.normal(0, pose_noise[0] / np.sqrt(3), (num_views, 3))

    # IMU
    n_imu = int(round(duration * imu_rate))
    imu_t = (np.arange(n_imu) + 0.5) / imu_rate
    p_i, a_w, R_wi, om = _eval_traj(tr, imu_t, p0, R_base)
    accel = np.einsum("nji,nj->ni", R_wi, a_w + g) + rng.normal(0, accel_noise, (n_imu, 3))
    gyro = om + rng.normal(0, gyro_noise, (n_imu, 3))

    q_ic_init = quat_from_mat(R_ic @ so3_exp_mat(rng.normal(0, np.deg2rad(0.5) / np.sqrt(3), 3)))
    return Dataset(
        name=name, camera_model=model, intrinsics=intr, image_width=W, image_height=Hh, fps=fps,
        points=pts, view_t_s=view_t, view_q_wc=quat_from_mat(R_wc_n), view_p_wc=p_wc_n,
        corner_offset=corner_offset, corner_uv=corner_uv, corner_point=corner_point,
        imu_t_s=imu_t, accel=accel, gyro=gyro, dt_so3=dt_so3, dt_r3=dt_r3, std_so3=std_so3, std_r3=std_r3,
        q_i_c_init=q_ic_init, line_delay_init=(1.0 / fps / Hh) if rolling_shutter else 0.0,
        gravity_init=g + rng.normal(0, 0.05, 3),
        truth=dict(q_i_c=q_ic, t_i_c=t_ic, gravity=g, line_delay=ld_true),
    )


# BASELINE.json configs.  "tiny" is a seconds-scale parity case.
CONFIGS = {
    "tiny": dict(num_views=12, corners_per_view=12, duration=1.2, camera="gopro9_division", board=(5, 4)),
    "C1": dict(num_views=30, corners_per_view=40, duration=3.0, camera="pinhole"),
    "C2": dict(num_views=200, corners_per_view=40, duration=20.0, camera="gopro9_division"),
    "C3": dict(num_views=900, corners_per_view=40, duration=30.0, camera="gopro6_fisheye"),
    "C4": dict(num_views=2000, corners_per_view=40, duration=66.0, camera="gopro6_double_sphere"),
    "C5": dict(num_views=10000, corners_per_view=50, duration=1000.0, camera="gopro9_division", board=(9, 7)),
}


def make_config(name, **overrides):
    kw = dict(CONFIGS[name]); kw.update(overrides)
    return make_dataset(name=name, **kw)


# ----------------------------------------------------------------- stationary IMU (Allan variance input)
def make_stationary_imu(duration=7200.0, rate=200.0, gyro_white=2e-3, accel_white=2e-2, gyro_rrw=2e-5, accel_rrw=3e-4,
                        gyro_bias=(1e-3, -2e-3, 5e-4), accel_bias=(0.02, -0.01, 0.03), gravity=(0.0, 0.0, 9.811104), seed=SEED):
    """A still IMU with known noise, the input of fit_allan_variance (docs/imu_noise_parameters.md of the reference).
    Per axis: constant bias + rate random walk (increments K sqrt(dt) N(0,1), K in units/s/sqrt(s)) + white noise of
    density D (units/sqrt(Hz): sample std D sqrt(rate)).  Gyroscope in rad/s, accelerometer in m/s^2 (gravity added).
    Its Allan variance is sigma2(tau) = D^2/tau + K^2 tau/3.  Returns the telemetry dict (timestamps_ns, accelerometer,
    gyroscope as arrays) and the truth."""
    rng = np.random.RandomState(seed)
    n = int(round(duration * rate))
    dt = 1.0 / rate
    t_ns = np.round(np.arange(n) * (1e9 / rate)).astype(np.int64)

    def axes(white, rrw, bias):
        walk = np.cumsum(rng.standard_normal((n, 3)) * (rrw * np.sqrt(dt)), axis=0)
        return np.asarray(bias, dtype=np.float64) + walk + rng.standard_normal((n, 3)) * (white * np.sqrt(rate))

    gyro = axes(gyro_white, gyro_rrw, gyro_bias)
    accel = axes(accel_white, accel_rrw, accel_bias) + np.asarray(gravity, dtype=np.float64)
    truth = dict(rate=rate, gyro_white=gyro_white, accel_white=accel_white, gyro_rrw=gyro_rrw, accel_rrw=accel_rrw,
                 gyro_bias=np.asarray(gyro_bias, dtype=np.float64), accel_bias=np.asarray(accel_bias, dtype=np.float64))
    return dict(timestamps_ns=t_ns, accelerometer=accel, gyroscope=gyro), truth


def _so3_log(R):
    c = np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)
    a = np.arccos(c)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return v * (0.5 if a < 1e-12 else a / (2.0 * np.sin(a)))


def make_static_multipose_imu(num_poses=36, rate=200.0, init_s=14.0, hold_s=4.0, move_s=2.0, gravity=9.811107, acc_noise=2e-3,
                              gyro_noise=1e-4, acc_params=(1.5e-3, -2e-3, 1e-3, 1.01, 0.995, 1.004, 0.05, -0.03, 0.08),
                              gyro_params=(2e-3, -1e-3, 1.5e-3, -2.5e-3, 1e-3, 2e-3, 0.99, 1.007, 1.012, 4e-3, -6e-3, 2e-3), seed=SEED):
    """A multi-pose IMU recording (static_imu_calibration's input, imu_tk): still for init_s with gravity on +z, then
    num_poses orientations, each held for hold_s and reached by a rotation about the IMU origin (no linear acceleration)
    of move_s with the closed-form rate omega(t) = s'(t) phi, s = tau - sin(2 pi tau) / (2 pi).  True specific force
    R^T (0, 0, g), true rate the body rate; raw = (T K)^-1 true + b + N(0, noise^2) per triad, parameters in the
    reference's order (accelerometer 9: misYZ misZY misZX sX sY sZ bX bY bZ; gyroscope 12: + misXZ misXY misYX after
    misZX).  Returns the telemetry dict (timestamps_ns, accelerometer, gyroscope) and the truth."""
    rng = np.random.RandomState(seed)
    n_init, n_hold, n_move = int(round(init_s * rate)), int(round(hold_s * rate)), int(round(move_s * rate))
    n = n_init + num_poses * (n_move + n_hold)
    t = np.arange(n) / rate
    poses = [np.eye(3)]
    while len(poses) < num_poses + 1:
        q = rng.standard_normal(4); q /= np.linalg.norm(q)
        R = mat_from_quat(q)
        # a reachable, distinct orientation: rotation from the previous pose between 40 and 150 degrees
        ang = np.linalg.norm(_so3_log(poses[-1].T @ R))
        if np.deg2rad(40) < ang < np.deg2rad(150):
            poses.append(R)
    Rs = np.zeros((n, 3, 3)); w = np.zeros((n, 3))
    Rs[:n_init] = np.eye(3)
    k = n_init
    for p in range(num_poses):
        phi = _so3_log(poses[p].T @ poses[p + 1])
        tau = np.arange(n_move) / n_move
        s = tau - np.sin(2 * np.pi * tau) / (2 * np.pi)
        sd = (1.0 - np.cos(2 * np.pi * tau)) / move_s
        for j in range(n_move):
            Rs[k + j] = poses[p] @ so3_exp_mat(s[j] * phi)
            w[k + j] = sd[j] * phi
        k += n_move
        Rs[k:k + n_hold] = poses[p + 1]
        k += n_hold
    f_true = np.einsum("nji,j->ni", Rs, np.array([0.0, 0.0, gravity]))

    def raw(true, p12, noise):
        p = np.asarray(p12, dtype=np.float64)
        T = np.array([[1.0, -p[0], p[1]], [p[3], 1.0, -p[2]], [-p[4], p[5], 1.0]])
        MS = T @ np.diag(p[6:9])
        return np.linalg.solve(MS, true.T).T + p[9:12] + rng.standard_normal(true.shape) * noise

    a9 = np.asarray(acc_params, dtype=np.float64)
    a12 = np.r_[a9[:3], 0.0, 0.0, 0.0, a9[3:]]
    acc = raw(f_true, a12, acc_noise)
    gyr = raw(w, gyro_params, gyro_noise)
    t_ns = np.round(t * 1e9).astype(np.int64)
    truth = dict(acc_params=a9, gyro_params=np.asarray(gyro_params, dtype=np.float64), gravity=gravity, rate=rate,
                 acc_noise=acc_noise, gyro_noise=gyro_noise, num_poses=num_poses, n_init=n_init, n_hold=n_hold, n_move=n_move)
    return dict(timestamps_ns=t_ns, accelerometer=acc, gyroscope=gyr), truth


# ---- the radon marker checkerboard (extract_board_to_json --board_type radon) ----------------------------------------
# Geometry of the reference's resource/checkerboard_radon.png ("Target v1.0: 14x9 - 12.1 mm"), measured at 300 dpi:
# (W+1) x (H+1) squares around W x H inner corners; black squares on the border have their outer half rounded into a
# half disc; three dots of diameter 0.336 squares mark the origin ("Board extraction").
RADON_DOT_RADIUS = 0.168
RADON_BLACK, RADON_WHITE = 30.0, 220.0
_RAY_CACHE = {}


def radon_origin(W, H):
    """Inner corner (row, column) of the origin: column W/2-1, row (H-1)/2 -> (4, 6) for 14 x 9."""
    return (H - 1) // 2, W // 2 - 1


def radon_board_shade(u, v, W, H):
    """Reflectance (1 white, 0 black) at board coordinates u = X/s (pattern row) and v = Y/s (pattern column); torch or
    numpy arrays.  Square (ci, cj) has inner corner (ci, cj) at its top-left; the origin square is white."""
    import torch
    xp = torch if isinstance(u, torch.Tensor) else np
    r0, c0 = radon_origin(W, H)
    ci, cj = xp.floor(u), xp.floor(v)
    fu, fv = u - ci, v - cj
    inside = (ci >= -1) & (ci <= H - 1) & (cj >= -1) & (cj <= W - 1)
    black = inside & ((ci + cj + r0 + c0) % 2 == 1)
    d2 = (fu - 0.5) ** 2 + (fv - 0.5) ** 2
    # rounded tabs: on the outer half of a border square only points within 0.5 of the centre line's midpoint stay black
    outer = (((ci == -1) & (fu < 0.5)) | ((ci == H - 1) & (fu > 0.5)) | ((cj == -1) & (fv < 0.5)) | ((cj == W - 1) & (fv > 0.5)))
    black = black & ~(outer & (d2 > 0.25))
    dot = (d2 <= RADON_DOT_RADIUS ** 2) & (((ci == r0) & (cj == c0)) | ((ci == r0 - 1) & (cj == c0)) | ((ci == r0) & (cj == c0 + 1)))
    black = black ^ dot
    return 1.0 - black.to(u.dtype) if xp is torch else 1.0 - black.astype(u.dtype)


def _pixel_corner_rays(camera):
    """Normalised rays (x, y) at the (w+1) x (h+1) pixel corners (x - 0.5, y - 0.5) of one CAMERAS entry (cached)."""
    if camera not in _RAY_CACHE:
        from . import planar_init
        model, intr, w, h = CAMERAS[camera]
        yy, xx = np.mgrid[0:h + 1, 0:w + 1]
        uv = np.stack([xx.ravel() - 0.5, yy.ravel() - 0.5], 1).astype(np.float64)
        _RAY_CACHE[camera] = planar_init.pixel_to_normalized(model, intr, uv).reshape(h + 1, w + 1, 2)
    return _RAY_CACHE[camera]


def radon_view_pose(W, H, square, f_px, img_h, rotation_deg, tilt_deg, tilt_axis_deg, fill=0.8, offset=(0.0, 0.0), distance_scale=1.0):
    """Camera pose (R, t: X_cam = R X_board + t) that shows the board upright at rotation 0, turned in the image plane by
    rotation_deg and tilted by tilt_deg about an in-plane axis at tilt_axis_deg; the board diagonal spans fill * img_h."""
    def rot(axis, a):
        a = np.deg2rad(a); c, s = np.cos(a), np.sin(a)
        k = np.asarray(axis, dtype=np.float64); K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        return np.eye(3) + s * K + (1 - c) * K @ K
    R0 = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])    # board rows -> image down, columns -> right
    ta = np.deg2rad(tilt_axis_deg)
    R = rot([np.cos(ta), np.sin(ta), 0.0], tilt_deg) @ rot([0, 0, 1], rotation_deg) @ R0
    diag = square * np.hypot(W + 1, H + 1)
    D = distance_scale * f_px * diag / (fill * img_h)
    centre = np.array([(H - 1) * square / 2.0, (W - 1) * square / 2.0, 0.0])
    t = np.array([offset[0] * D, offset[1] * D, D]) - R @ centre
    return R, t


def render_radon_views(camera, num_views, W=14, H=9, square=0.0121, rotations=None, tilt_deg=20.0, supersample=4,
                       blur_sigma=0.0, noise_sigma=0.0, seed=SEED, device="cpu", cover_marker=False, offsets=None,
                       distance_scale=1.0):
    """Images of the radon target through one CAMERAS model and the true pixel positions of its W*H inner corners.
    Every pixel averages supersample^2 samples (a rank-1 lattice).  The exact rays (planar_init.pixel_to_normalized) are
    computed at the pixel corners only; a sample's board point is interpolated bilinearly between the board points of
    its pixel's four corners instead of unprojecting every sample (the error of that, second order in the distortion
    over one pixel, is far below the detector's tolerances), and reads radon_board_shade.  Optional Gaussian blur
    (sigma in px) and Gaussian noise (grey levels).  rotations: in-plane angles in degrees (default random);
    offsets: per-view image-plane offsets of the board centre (fractions of the distance); cover_marker paints the
    three marker squares grey.  Returns dict(images [n,h,w] u8, corners [n,W*H,2] with id i*W+j, visible [n] (all
    corners inside the image), model, intrinsics, width, height, R, t)."""
    import torch
    model, intr, w, h = CAMERAS[camera]
    rng = np.random.RandomState(seed)
    rays = torch.as_tensor(_pixel_corner_rays(camera), dtype=torch.float64, device=device)
    # supersample^2 samples per pixel on a rank-1 lattice (Korobov generator near N / golden ratio): every sample has
    # its own x and its own y offset, so an edge along a pixel axis is resolved to 1/N px, not 1/supersample
    N = int(supersample) ** 2
    gen = max(1, int(round(N / 1.618033988749895)))
    while np.gcd(gen, N) != 1:
        gen += 1
    images, corners, visible, Rs, ts = [], [], [], [], []
    r0, c0 = radon_origin(W, H)
    gi, gj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    board_pts = np.stack([gi.ravel() * square, gj.ravel() * square, np.zeros(W * H)], 1)
    for k in range(num_views):
        rotd = float(rotations[k % len(rotations)]) if rotations is not None else rng.uniform(0, 360)
        off = offsets[k % len(offsets)] if offsets is not None else rng.uniform(-0.08, 0.08, 2)
        R, t = radon_view_pose(W, H, square, intr[0], h, rotd, tilt_deg * (rng.uniform(0.5, 1.0) if rotations is None else 1.0),
                               rng.uniform(0, 360), offset=off, distance_scale=distance_scale)
        # board coordinates at the pixel corners: X = R^T (lam d - t) with (R^T (lam d - t))_z = 0
        Rt = torch.as_tensor(R.T, dtype=torch.float64, device=device)
        tb = Rt @ torch.as_tensor(t, dtype=torch.float64, device=device)
        d = torch.cat([rays, torch.ones_like(rays[..., :1])], -1) @ Rt.T
        lam = tb[2] / d[..., 2]
        XY = (lam[..., None] * d[..., :2] - tb[:2]) / square                   # [h+1, w+1, 2] board units (u, v)
        acc = torch.zeros(h, w, dtype=torch.float64, device=device)
        for q in range(N):
            sx, sy = (q + 0.5) / N, ((q * gen) % N + 0.5) / N
            top = XY[:-1, :-1] * (1 - sy) + XY[1:, :-1] * sy
            bot = XY[:-1, 1:] * (1 - sy) + XY[1:, 1:] * sy
            p = top * (1 - sx) + bot * sx
            sh = radon_board_shade(p[..., 0], p[..., 1], W, H)
            if cover_marker:
                ci, cj = torch.floor(p[..., 0]), torch.floor(p[..., 1])
                m = ((ci == r0) | (ci == r0 - 1)) & ((cj == c0) | (cj == c0 + 1))
                sh = torch.where(m, torch.full_like(sh, 0.5), sh)
            acc += sh
        img = RADON_BLACK + (RADON_WHITE - RADON_BLACK) * acc / N
        if blur_sigma > 0:
            rad = int(np.ceil(4 * blur_sigma))
            g = torch.exp(-0.5 * (torch.arange(-rad, rad + 1, dtype=torch.float64, device=device) / blur_sigma) ** 2)
            g = (g / g.sum())
            x = torch.nn.functional.pad(img[None, None], (rad, rad, rad, rad), mode="replicate")
            x = torch.nn.functional.conv2d(x, g.view(1, 1, 1, -1)); x = torch.nn.functional.conv2d(x, g.view(1, 1, -1, 1))
            img = x[0, 0]
        img = img.cpu().numpy()
        if noise_sigma > 0:
            img = img + rng.standard_normal(img.shape) * noise_sigma
        images.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
        uv, _ = project(model, intr, board_pts @ R.T + t)
        corners.append(uv)
        visible.append(bool(np.all((uv > 0) & (uv < [w - 1, h - 1]))))
        Rs.append(R); ts.append(t)
    return dict(images=np.stack(images), corners=np.stack(corners), visible=np.array(visible), model=model,
                intrinsics=np.asarray(intr, dtype=np.float64), width=w, height=h, R=np.stack(Rs), t=np.stack(ts), W=W, H=H,
                square=square)
