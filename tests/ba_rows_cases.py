"""The cases of the view bundle adjustment's 50-digit comparison (tests/ba_rows_reference.py), shared by the host test and the
device test: small problems placed at the edges of the code -- rotation branches, the camera models' branches, the Huber kink,
the chunk and column edges of the Gram kernels, the homogeneous-vector branches of the board points.

    row_datasets()   (a) one observation per view, one data set per camera model / division coefficient, and the Huber data set
    chunk_dataset()  (b) views of 1, 2, 63, 64, 65, 128, 129 and 0 observations
    points_dataset() (c) the unwarped board with homogeneous scales, points seen in 1, 64 and 65 views
    views_dataset()  (d) views of 4, 40 and 65 observations and one at w = 0 for the one-launch pose refinement
"""
import functools
import math

import mpmath as mp
import numpy as np

import ba_rows_reference as R
from openimucameracalibrator_amd import camera_calibrator as CC
from openimucameracalibrator_amd import synthetic as S

POSE = CC.BA_POSITION | CC.BA_ORIENTATION
AXIS = np.array([0.6, -0.48, 0.64])                     # unit
# 4-point scene; point 2 is homogeneous with w = 1.7
SCENE = np.array([[0.0, 0.0, 0.0, 1.0], [0.1, 0.05, 0.0, 1.0], [1.7 * 0.02, 1.7 * 0.13, 1.7 * 0.01, 1.7], [0.15, 0.1, -0.02, 1.0]])
THETA_LOSES_DIGITS = ("t1e-8_x", "t1e-8_y", "t1e-8_z", "t1.6e-8", "t0.0099", "t0.0101")    # 0 < theta < 0.02: the Jets are no yardstick


def _rot(w):
    return np.array(R.rodrigues(mp.fp, [float(v) for v in w]), dtype=np.float64)


def _place(w, point, target):
    """Pose [C | w] that puts scene point `point` at the camera-frame position `target` (float64 placement)."""
    Xe = SCENE[point, :3] / SCENE[point, 3]
    return np.concatenate([Xe - _rot(w).T @ np.asarray(target, dtype=np.float64), np.asarray(w, dtype=np.float64)])


def _common_views():
    g = np.array([0.31, -0.42, 0.25])
    return [("generic", g, 1, (0.05, -0.03, 0.4)),
            ("w0", np.zeros(3), 3, (-0.04, 0.02, 0.35)),
            ("t1e-8_x", np.array([1e-8, 0, 0]), 1, (0.03, 0.04, 0.38)),
            ("t1e-8_y", np.array([0, 1e-8, 0]), 3, (-0.05, 0.03, 0.33)),
            ("t1e-8_z", np.array([0, 0, 1e-8]), 1, (0.04, -0.05, 0.42)),
            ("t1.6e-8", 1.6e-8 * AXIS, 3, (0.05, 0.02, 0.36)),
            ("t0.0099", 0.0099 * AXIS, 1, (-0.03, -0.04, 0.39)),
            ("t0.0101", 0.0101 * AXIS, 1, (-0.03, -0.04, 0.39)),
            ("pi-1e-6", (math.pi - 1e-6) * AXIS, 3, (0.04, 0.03, 0.37)),
            ("t5.5", 5.5 * AXIS, 1, (-0.05, 0.04, 0.41)),
            ("hom1.7", np.array([-0.2, 0.35, 0.4]), 2, (0.03, -0.05, 0.34))]


def _edge_angle(model, intr):
    """Angle from the optical axis at which the model's domain ends (extended unified, double sphere)."""
    lo, hi = 0.0, math.pi
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        try:
            R.project(mp.fp, model, [float(v) for v in intr], [math.sin(mid), 0.0, math.cos(mid)])
            lo = mid
        except R.OutsideDomain:
            hi = mid
    return lo


def _extra_views(name, model, intr):
    g = np.array([0.31, -0.42, 0.25])
    z0 = np.zeros(3)
    if model == CC.CAM_FISHEYE:
        return [("r0.99e-4", z0, 1, (0.99e-4 * 0.6, 0.99e-4 * 0.8, 0.4)), ("r1.01e-4", z0, 1, (1.01e-4 * 0.6, 1.01e-4 * 0.8, 0.4)),
                ("r1.01e-4_rot", g, 3, (1.01e-4 * 0.6, -1.01e-4 * 0.8, 0.37)), ("z<0", g, 1, (0.05, -0.04, -0.3))]
    if model in (CC.CAM_EXTENDED_UNIFIED, CC.CAM_DOUBLE_SPHERE):
        phi = 0.8 * _edge_angle(model, intr)
        return [("axis", z0, 1, (0.0, 0.0, 0.4)),
                ("edge80", g, 3, (0.4 * math.sin(phi) * 0.8, 0.4 * math.sin(phi) * 0.6, 0.4 * math.cos(phi)))]
    if model == CC.CAM_DIVISION_UNDISTORTION:
        f, asp, k = intr[0], intr[1], intr[4]
        at = lambda r, z: (r * 0.6 / f * z, r * 0.8 / (f * asp) * z, z)          # undistorted radius r px
        out = [("axis", z0, 1, (0.0, 0.0, 0.4)), ("off1px", z0, 3, at(1.0, 0.4))]
        if name == "division_k+1e-5":
            out += [("4kr2=0.9", g, 1, at(math.sqrt(0.9 / (4 * k)), 0.4)), ("4kr2>1", g, 3, at(math.sqrt(1.09 / (4 * k)), 0.38))]
        return out
    return []


ROW_DATASETS = {"pinhole": ("pinhole", None), "pinhole_radtan": ("pinhole_radtan", None), "fisheye": ("gopro6_fisheye", None),
                "division": ("gopro9_division", None), "double_sphere": ("gopro6_double_sphere", None), "eucm": ("gopro9_eucm", None),
                "division_k-1e-10": ("gopro9_division", -1e-10), "division_k-1e-14": ("gopro9_division", -1e-14),
                "division_k+1e-7": ("gopro9_division", 1e-7), "division_k+1e-5": ("gopro9_division", 1e-5)}


@functools.lru_cache(maxsize=None)
def row_dataset(name):
    """(problem, view labels, huber width): flags POSE, every intrinsic free, one observation per view.  The features lie tens of
    pixels from the projections: r = px - uv cancels, and only a residual of that size leaves the cost a relative 1e-14 in float64."""
    if name == "huber":
        return _huber_dataset()
    camera, k = ROW_DATASETS[name]
    model, intr, _, _ = S.CAMERAS[camera]
    intr = np.array(intr, dtype=np.float64)
    if k is not None:
        intr[4] = k
    views = _common_views() + _extra_views(name, model, intr)
    rng = np.random.default_rng(7)
    poses = np.array([_place(w, pt, target) for _, w, pt, target in views])
    uv = np.array([R.pixel(model, intr, poses[i], SCENE[views[i][2]]) for i in range(len(views))]) + rng.normal(0, 40.0, (len(views), 2))
    prob = R.make_problem(model, intr, SCENE, poses, np.arange(len(views) + 1), uv, [v[2] for v in views])
    return prob, [v[0] for v in views], 0.0


def _huber_dataset():
    """pinhole, Huber width 1.345: residual norms just below and above the kink, far beyond it, and exactly 0 (the point on
    the optical axis of an unrotated camera projects onto the principal point without rounding)."""
    model, intr, _, _ = S.CAMERAS["pinhole"]
    intr = np.array(intr, dtype=np.float64)
    g = np.array([0.31, -0.42, 0.25])
    views = [("1.344", g, 1, (0.05, -0.03, 0.4), 1.344), ("1.346", g, 3, (-0.04, 0.03, 0.37), 1.346), ("1e4", g, 1, (0.03, 0.05, 0.36), 1e4)]
    poses = [_place(w, pt, target) for _, w, pt, target, _ in views]
    uv = [R.pixel(model, intr, poses[i], SCENE[views[i][2]]) + views[i][4] * np.array([0.6, -0.8]) for i in range(3)]
    poses.append(np.array([0.0, 0.0, -0.4, 0.0, 0.0, 0.0])); uv.append(np.array([intr[3], intr[4]]))
    prob = R.make_problem(model, intr, SCENE, np.array(poses), np.arange(5), np.array(uv), [1, 3, 1, 0])
    norms = np.hypot(*(np.array([R.pixel(model, intr, prob["poses"][i], SCENE[prob["point_ids"][i]]) for i in range(4)]) - prob["uv"]).T)
    assert norms[0] < 1.345 < norms[1] and norms[2] > 9e3 and norms[3] == 0.0
    return prob, [v[0] for v in views] + ["0"], 1.345


def jets_lose_digits(name, label):
    """Cases where the oracle's Jets themselves lose digits, so that their figure is no yardstick: 0 < theta < 0.02, and the
    division model with |k r^2| < 1e-3 (its literal quotient cancels)."""
    if label in THETA_LOSES_DIGITS:
        return True
    m = division_m(name, label)
    return m is not None and m < 1e-3


def division_m(name, label):
    """|k r^2| of a view of a division-model data set (None for the other models and for the corner)."""
    if not name.startswith("division") or label == "corner":
        return None
    prob, labels, _ = row_dataset(name)
    v = labels.index(label)
    q = prob["intrinsics"]
    px = R.pixel(prob["model"], np.array([q[0], q[1], 0.0, 0.0, 0.0]), prob["poses"][v], SCENE[prob["point_ids"][v]])   # k = 0: (ux, uy)
    return abs(q[4]) * float(px @ px)


def substitute(name, label):
    """The yardstick key a case of data set (a) borrows where its own Jet figure is none (None: its own): the generic view (the
    intrinsics corner) of the same camera with one observation per view -- the exact function is smooth there and its condition
    is that of the generic case."""
    if label == "corner":
        return "a/division/corner" if jets_lose_digits(name, "generic") else None
    if not jets_lose_digits(name, label):
        return None
    return "a/division/generic" if jets_lose_digits(name, "generic") else "a/%s/generic" % name


CHUNK_COUNTS = (1, 2, 63, 64, 65, 128, 129, 0)
CHUNK_CONFIGS = {   # name: (camera, flags, what is free, huber width)
    "radtan_all": ("pinhole_radtan", POSE, CC.ALL, 0.0),                     # 17 columns with the residual: two MFMA blocks
    "fisheye_all": ("gopro6_fisheye", POSE, CC.ALL, 0.0),                    # 16 columns: the residual in the last column of one block
    "radtan_skew": ("pinhole_radtan", 0, CC.SKEW, 0.0),                      # 2 columns
    "radtan_orientation_pp": ("pinhole_radtan", CC.BA_ORIENTATION, CC.PRINCIPAL_POINTS, 0.0),
    "radtan_all_huber": ("pinhole_radtan", POSE, CC.ALL, 1.345),            # 10 % outliers of 15 px
}


@functools.lru_cache(maxsize=None)
def chunk_dataset(camera):
    """Views of CHUNK_COUNTS observations (point ids repeat), 10 % outliers of 15 px, perturbed start poses."""
    ds = CC.make_calibration_dataset(camera, num_views=len(CHUNK_COUNTS), corners_per_view=40, outlier_fraction=0.1)
    off = ds["corner_offset"]
    uv, pid, o = [], [], [0]
    for v, n in enumerate(CHUNK_COUNTS):
        m = int(off[v + 1] - off[v])
        take = np.arange(n) % m
        uv.append(ds["uv"][off[v] + take] + 0.05 * (np.arange(n) // m)[:, None])
        pid.append(ds["point_ids"][off[v] + take])
        o.append(o[-1] + n)
    return R.make_problem(ds["model"], ds["intrinsics"], ds["points"], ds["pose_init"], o, np.concatenate(uv), np.concatenate(pid))


POINT_SCALES = (1.0, -1.5, 1e-3, 1e3)
SEEN_1, SEEN_64, SEEN_65, CONSTANT_POINTS = 20, 10, 5, (7, 13)


@functools.lru_cache(maxsize=None)
def points_dataset():
    """BA_POINTS: the unwarped 8 x 6 board (corner 0 is the origin: sigma = 0) with homogeneous scales POINT_SCALES by index, 65
    views at their true poses; point 20 is seen in 1 view, point 10 in 64, point 5 in 65; points 7 and 13 are constant.
    Feature noise 5 px: the cost sums r^2 with r = px - uv, |px| ~ 480, so one rounding of a pixel coordinate (eps |px| / 2) moves a
    term by eps |px| / |r| relative and the sum of 2 n = 780 such terms by about eps |px| / (|r| sqrt(2 n)) -- 2e-14 at 0.2 px, above the
    1e-14 the cost is held to whatever the arithmetic, 8e-16 at 5 px.  (Both sides of the Huber kink still occur.)"""
    ds = CC.make_calibration_dataset("pinhole_radtan", num_views=65, corners_per_view=20)   # (a negative scale mirrors a: x / z models only)
    pts = ds["points"] * np.array([POINT_SCALES[i % 4] for i in range(48)])[:, None]
    assert not pts[0, :3].any() and pts[0, 3] == 1.0
    rng = np.random.default_rng(11)
    uv, pid, o = [], [], [0]
    for v in range(65):
        ids = [SEEN_65] + ([SEEN_64] if v < 64 else []) + ([SEEN_1] if v == 0 else []) + ([0] if v % 4 == 0 else [])
        ids += [i for i in ((7 * v + j) % 48 for j in range(3)) if i not in (SEEN_1, SEEN_64, SEEN_65, 0)]
        for i in ids:
            uv.append(R.pixel(ds["model"], ds["intrinsics"], ds["pose_true"][v], pts[i]) + rng.normal(0, 5.0, 2))
            pid.append(i)
        o.append(len(pid))
    var = np.ones(48, np.uint8); var[list(CONSTANT_POINTS)] = 0
    prob = R.make_problem(ds["model"], ds["intrinsics"], pts, ds["pose_true"], o, np.array(uv), pid, var)
    counts = np.bincount(prob["point_ids"], minlength=48)
    assert counts[SEEN_1] == 1 and counts[SEEN_64] == 64 and counts[SEEN_65] == 65 and counts.min() >= 1
    return prob


VIEW_FLAGS = {"pose": POSE, "position": CC.BA_POSITION, "orientation": CC.BA_ORIENTATION}
VIEW_LABELS = ("4", "40", "65", "w0")


@functools.lru_cache(maxsize=None)
def views_dataset():
    """OptimizeViews: views of 4, 40 and 65 observations from perturbed start poses and one view that starts at w = 0."""
    ds = CC.make_calibration_dataset("gopro6_fisheye", num_views=3, corners_per_view=40, pose_noise=(0.01, 0.01), outlier_fraction=0.05)
    off = ds["corner_offset"]
    uv, pid, o = [], [], [0]
    for v, n in enumerate((4, 40, 65)):
        m = int(off[v + 1] - off[v])
        take = np.arange(n) % m if n > 4 else np.array([0, m // 3, 2 * m // 3, m - 1])
        uv.append(ds["uv"][off[v] + take] + 0.05 * (np.arange(n) // m)[:, None])
        pid.append(ds["point_ids"][off[v] + take]); o.append(o[-1] + n)
    # the camera of the fourth view looks along +z onto the board; its features come from a slightly turned and moved pose
    true = np.array([0.075, 0.055, -0.39, 0.012, -0.009, 0.006])
    ids = np.arange(0, 48, 2)
    rng = np.random.default_rng(5)
    uv.append(np.array([R.pixel(ds["model"], ds["intrinsics"], true, ds["points"][i]) for i in ids]) + rng.normal(0, 0.2, (len(ids), 2)))
    pid.append(ids); o.append(o[-1] + len(ids))
    poses = np.vstack([ds["pose_init"], [[0.07, 0.05, -0.4, 0.0, 0.0, 0.0]]])
    return R.make_problem(ds["model"], ds["intrinsics"], ds["points"], poses, o, np.concatenate(uv), np.concatenate(pid))


def view_blocks(problem, flags, mask):
    """Per view the tangent columns of its pose, and the columns of the intrinsics corner."""
    d = len(R.pose_columns(flags))
    nv = len(problem["poses"])
    a = bin(mask & ((1 << len(problem["intrinsics"])) - 1)).count("1")
    return [np.arange(v * d, (v + 1) * d) for v in range(nv)], np.arange(nv * d, nv * d + a)
