"""Data sets and flag sets shared by the CPU tests of tests/normal_equations_reference.py and the GPU tests built on it."""
import dataclasses

import numpy as np

from openimucameracalibrator_amd import synthetic, estimator as E

FLAGS1 = E.SPLINE | E.T_I_C | E.GRAVITY_DIR
ALL = FLAGS1 | E.CAM_LINE_DELAY | E.IMU_BIASES | E.IMU_INTRINSICS
# FLAGS1, each arrow family alone on top of it, all of them, the line delay alone
FLAG_SETS = [("FLAGS1", FLAGS1), ("+LINE_DELAY", FLAGS1 | E.CAM_LINE_DELAY), ("+IMU_BIASES", FLAGS1 | E.IMU_BIASES),
             ("+IMU_INTRINSICS", FLAGS1 | E.IMU_INTRINSICS), ("ALL", ALL), ("LINE_DELAY", E.CAM_LINE_DELAY)]


def ragged():
    """Views of 80 corners (two work-list chunks of 64 + 16), one with 40 and one with none."""
    ds = synthetic.make_config("tiny", board=(10, 8), corners_per_view=80)
    keep = np.ones(ds.num_corners, dtype=bool)
    keep[ds.corner_offset[3]:ds.corner_offset[4]] = False
    keep[ds.corner_offset[5] + 40:ds.corner_offset[6]] = False
    counts = np.array([keep[ds.corner_offset[v]:ds.corner_offset[v + 1]].sum() for v in range(ds.num_views)])
    ds.corner_uv = ds.corner_uv[keep]; ds.corner_point = ds.corner_point[keep]
    ds.corner_offset = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return ds


def with_measurement_gap(ds, t0, t1):
    """The data set without the views and IMU samples of [t0, t1) s (relative to the first view)."""
    base = ds.view_t_s.min()
    keep_v = np.where(~((ds.view_t_s - base >= t0) & (ds.view_t_s - base < t1)))[0]
    keep_i = ~((ds.imu_t_s - base >= t0) & (ds.imu_t_s - base < t1))
    off, uv, pt = [0], [], []
    for v in keep_v:
        a, b = ds.corner_offset[v], ds.corner_offset[v + 1]
        uv.append(ds.corner_uv[a:b]); pt.append(ds.corner_point[a:b]); off.append(off[-1] + (b - a))
    return dataclasses.replace(ds, view_t_s=ds.view_t_s[keep_v], view_q_wc=ds.view_q_wc[keep_v], view_p_wc=ds.view_p_wc[keep_v],
                               corner_offset=np.asarray(off, np.int64), corner_uv=np.concatenate(uv), corner_point=np.concatenate(pt).astype(np.int32),
                               imu_t_s=ds.imu_t_s[keep_i], accel=ds.accel[keep_i], gyro=ds.gyro[keep_i])


def out_of_order():
    """C1 with the views in the string order of their file keys and the IMU samples reversed."""
    ds = synthetic.make_config("C1")
    d2 = ds.with_view_order(ds.file_key_order())
    d2.imu_t_s = d2.imu_t_s[::-1].copy(); d2.accel = d2.accel[::-1].copy(); d2.gyro = d2.gyro[::-1].copy()
    return d2


# name -> (yardstick configuration, builder, estimator options)
SHAPES = {
    "tiny": ("tiny", lambda: synthetic.make_config("tiny"), {}),
    "C1": ("C1", lambda: synthetic.make_config("C1"), {}),
    "C2": ("C2", lambda: synthetic.make_config("C2"), {}),
    "C3": ("C3", lambda: synthetic.make_config("C3"), {}),
    "gs_views": ("tiny", lambda: synthetic.make_config("tiny", rolling_shutter=False), {}),
    "gs_views_unit_loss": ("tiny", lambda: synthetic.make_config("tiny", rolling_shutter=False), {"gs_unit_loss": 1}),
    "knot_spacing_56_128": ("tiny", lambda: synthetic.make_config("tiny", dt_so3=0.056, dt_r3=0.128, duration=2.4, num_views=24), {}),
    "knot_spacing_200_17": ("tiny", lambda: synthetic.make_config("tiny", dt_so3=0.2, dt_r3=0.017, duration=2.0, num_views=20), {}),
    "gap": ("C1", lambda: with_measurement_gap(synthetic.make_config("C1"), 1.0, 2.1), {}),
    "ragged": ("tiny", ragged, {}),
    "out_of_order": ("C1", out_of_order, {}),
    "short_0.3s": ("tiny", lambda: synthetic.make_config("tiny", duration=0.3, num_views=3), {}),
    "short_0.75s": ("tiny", lambda: synthetic.make_config("tiny", duration=0.75, num_views=8), {}),
    "rs_time_in_seconds": ("tiny", lambda: synthetic.make_config("tiny"), {"rs_time_in_seconds": 1}),
}


def time_slices(Pb, P, width=400):
    """Columns of three time slices of the band -- the first windows, the middle of the trajectory, the last windows -- and the arrow
    (the slice form for C4 / C5)."""
    los = (0, (Pb // 2) - width // 2, Pb - width)
    return np.concatenate([np.arange(lo, lo + width) for lo in los] + [np.arange(Pb, P)])
