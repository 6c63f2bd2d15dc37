"""Robust start poses: RANSAC over the corners of every view of a corner file, all views in one call of the C-ABI entry
oicc_planar_ransac (csrc/planar_ransac.hip; one workgroup per view, one lane per hypothesis).

The reference gets a pose (and focal length) per view from TheiaSfM's RANSAC minimal solvers [EXT]
(camera_calibrator.cc:51-56,262-301, pose_estimator.cc:41-46,54-83) and, in the pose estimator, keeps only the RANSAC
inliers.  Here the hypothesis is the radial alignment constraint (Tsai's first stage): for a radially symmetric lens a
corner moves along its radius, never across it, so  u (q3 a + q4 b + q5) - v (q0 a + q1 b + q2) = 0  holds for every
camera model of this project, calibrated or not, with five correspondences per sample.  Calibrated features (mode 1) are
also tested against the full reprojection of the pose completed from q.  This module only SELECTS corners: the start
values stay the closed forms of planar_init.initialize_view, run on the inliers ("Robust start poses").
There is no CPU path in the product; `backend` takes anything with this module's `run` (tests pass the numpy
restatement)."""
import ctypes as C

import numpy as np

from . import _abi
from . import planar_init

UNCALIBRATED, CALIBRATED = 0, 1
DEFAULT_SEED = 20241115
DEFAULT_HYPOTHESES = 256
MIN_INLIERS = 6            # ransac_summary.inliers.size() < 6 (pose_estimator.cc:72-74)


class HipBackend:
    """oicc_planar_ransac of liboicc_hip.so."""

    def __init__(self):
        from . import _lib
        self.b = _lib.load_planar_ransac()     # raises without the HIP library
        self.device_ms = 0.0

    def run(self, corner_offsets, ab, xy, mode, threshold, num_hypotheses=DEFAULT_HYPOTHESES, seed=DEFAULT_SEED, device=0,
            want_counts=False):
        off = np.ascontiguousarray(corner_offsets, dtype=np.int64)
        ab = np.ascontiguousarray(ab, dtype=np.float64).reshape(-1, 2)
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        nv = len(off) - 1
        n = len(ab)
        if nv < 0 or len(xy) != n or (nv >= 0 and (off[0] != 0 or off[-1] != n)):
            raise ValueError("corner_offsets do not describe ab / xy")
        inlier = np.zeros(max(n, 1), np.uint8)
        num = np.zeros(max(nv, 1), np.int32)
        q = np.zeros((max(nv, 1), 6))
        pose = np.zeros((max(nv, 1), 12))
        counts = np.zeros((max(nv, 1), int(num_hypotheses)), np.int32) if want_counts else None
        ms = C.c_double(0.0)
        rc = self.b.ransac(int(device), nv, off.ctypes.data_as(_abi.c_i64p), ab.ctypes.data_as(_abi.c_dp), xy.ctypes.data_as(_abi.c_dp),
                        int(mode), float(threshold), int(num_hypotheses), int(seed), inlier.ctypes.data_as(_abi.c_u8p),
                        num.ctypes.data_as(_abi.c_i32p), q.ctypes.data_as(_abi.c_dp), pose.ctypes.data_as(_abi.c_dp),
                        counts.ctypes.data_as(_abi.c_i32p) if want_counts else None, C.byref(ms))
        if rc == -1:
            raise ValueError("oicc_planar_ransac: invalid argument")
        if rc != 0:
            raise RuntimeError("oicc_planar_ransac failed with %d (no usable HIP device?)" % rc)
        self.device_ms = ms.value
        return inlier[:n].astype(bool), num[:nv], q[:nv], pose[:nv], (counts[:nv] if want_counts else None)


def planar_ransac(corner_offsets, ab, xy, mode, threshold, num_hypotheses=DEFAULT_HYPOTHESES, seed=DEFAULT_SEED, device=0,
                  backend=None, want_counts=False):
    """All views in one call: (inlier [n] bool, num_inliers [nv], q [nv, 6], pose [nv, 12] = R row-major | t in the board
    plane frame (calibrated mode, zero otherwise), hypothesis counts [nv, H] or None)."""
    if backend is None:
        backend = HipBackend()
    return backend.run(corner_offsets, ab, xy, mode, threshold, num_hypotheses=num_hypotheses, seed=seed, device=device,
                       want_counts=want_counts)


def pack_views(points_xyzw, views):
    """views: list of (point_ids, features relative to the distortion centre).  Returns (offsets, ab, xy) in the layout
    of the entry, with the board plane coordinates of planar_init.board_frame."""
    c, E, _ = planar_init.board_frame(points_xyzw)
    P = np.asarray(points_xyzw, dtype=np.float64)
    X = P[:, :3] / P[:, 3:4]
    off = np.zeros(len(views) + 1, np.int64)
    ab, xy = [], []
    for i, (pid, feat) in enumerate(views):
        off[i + 1] = off[i] + len(pid)
        ab.append((X[np.asarray(pid, dtype=np.int64)] - c) @ E[:2].T)
        xy.append(np.asarray(feat, dtype=np.float64).reshape(-1, 2))
    ab = np.concatenate(ab) if ab else np.zeros((0, 2))
    xy = np.concatenate(xy) if xy else np.zeros((0, 2))
    return off, ab, xy


def select_inliers(points_xyzw, views, mode, threshold, num_hypotheses=DEFAULT_HYPOTHESES, seed=DEFAULT_SEED, device=0, backend=None):
    """One boolean mask per view of `views` (see pack_views)."""
    if not views:
        return []
    off, ab, xy = pack_views(points_xyzw, views)
    inlier = planar_ransac(off, ab, xy, mode, threshold, num_hypotheses, seed, device, backend)[0]
    return [np.asarray(inlier[off[i]:off[i + 1]], dtype=bool) for i in range(len(views))]
