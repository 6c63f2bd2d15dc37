"""oicc_planar_ransac on the device against its numpy restatement (tests/planar_ransac_restatement.py)."""
import numpy as np
import pytest

import planar_ransac_cases as PC
import planar_ransac_restatement as PR
from openimucameracalibrator_amd import robust_init as RI

pytestmark = pytest.mark.gpu

FLAG_CAP = 0.05       # at most this share of the hypotheses may lie too close to a decision to be compared


def dirty_views(camera, calibrated, bad_per_view=6):
    """30 views of 40 corners, `bad_per_view` corners of each moved 10-60 px."""
    ds = PC.dataset(camera)
    uv, _ = PC.plant_moved(ds, bad_per_view / 40.0)
    return PC.packed(ds, uv, calibrated)


@pytest.mark.parametrize("camera,calibrated", [("gopro9_division", False), ("gopro6_fisheye", True)])
def test_hypothesis_counts_equal_the_restatement(camera, calibrated):
    """Equal scores on 40-corner views also show that both sides drew the same five corners."""
    off, ab, xy, thr, mode = dirty_views(camera, calibrated)
    _, _, _, _, counts = RI.planar_ransac(off, ab, xy, mode, thr, want_counts=True)
    assert counts.shape == (len(off) - 1, 256)
    flagged_total = compared = 0
    for v in range(len(off) - 1):
        s = slice(off[v], off[v + 1])
        c, _, _, flagged = PR.vote(v, ab[s, 0], ab[s, 1], xy[s, 0], xy[s, 1], thr, 256, PR.DEFAULT_SEED, flags=True)
        flagged_total += int(flagged.sum()); compared += int((~flagged).sum())
        assert np.array_equal(counts[v][~flagged], c[~flagged]), (v, np.where(counts[v] != c)[0])
    print("%s: %d of %d hypotheses flagged" % (camera, flagged_total, flagged_total + compared))
    assert flagged_total <= FLAG_CAP * (flagged_total + compared)


def sign_scale_distance(q, ref):
    """q and ref equal up to sign and scale: distance of the unit vectors."""
    q = q / np.linalg.norm(q); ref = ref / np.linalg.norm(ref)
    return min(np.abs(q - ref).max(), np.abs(q + ref).max())


@pytest.mark.parametrize("camera", ["gopro9_division", "gopro6_fisheye", "pinhole"])
@pytest.mark.parametrize("variant,fraction", [("moved", 0.15), ("moved", 0.30), ("swapped", 0.15)])
def test_masks_q_and_pose_equal_the_restatement(camera, variant, fraction):
    """Inlier masks and counts are identical.  The refitted q and the pose differ by rounding only (the order of the
    normal-matrix sums): the yardstick is the restatement in float64 against itself in numpy.longdouble on the same
    views, and the device may be ten times that away from the float64 restatement.  Measured on an MI355X over
    these nine data sets: yardstick q 2.4e-15 .. 8.3e-15, pose 2.8e-14 .. 1.1e-13; device q 3.0e-15 .. 1.0e-14, pose
    3.1e-14 .. 1.6e-13."""
    ds = PC.dataset(camera)
    uv, _ = (PC.plant_moved if variant == "moved" else PC.plant_swapped)(ds, fraction)
    for calibrated in (False, True):
        off, ab, xy, thr, mode = PC.packed(ds, uv, calibrated)
        inl, num, q, pose, _ = RI.planar_ransac(off, ab, xy, mode, thr)
        r_inl, r_num, r_q, r_pose, _ = PR.run(off, ab, xy, mode, thr)
        l_inl, _, l_q, l_pose, _ = PR.run(off, ab, xy, mode, thr, dtype=np.longdouble)
        assert np.array_equal(inl, r_inl) and np.array_equal(num, r_num)
        same = [v for v in range(len(off) - 1) if np.array_equal(r_inl[off[v]:off[v + 1]], l_inl[off[v]:off[v + 1]]) and r_num[v] > 0]
        assert len(same) >= len(off) - 3
        yard_q = max(sign_scale_distance(r_q[v], l_q[v].astype(np.float64)) for v in same)
        dev_q = max(sign_scale_distance(q[v], r_q[v]) for v in range(len(off) - 1) if r_num[v] > 0)
        print("%s %s %.2f mode %d: q device-restatement %.3g, yardstick %.3g" % (camera, variant, fraction, mode, dev_q, yard_q))
        assert yard_q > 0 and dev_q <= 10 * yard_q
        if calibrated:
            yard_p = max(np.abs(r_pose[v] - l_pose[v].astype(np.float64)).max() for v in same)
            dev_p = np.abs(pose - r_pose).max()
            print("    pose device-restatement %.3g, yardstick %.3g" % (dev_p, yard_p))
            assert yard_p > 0 and dev_p <= 10 * yard_p


def test_shapes_and_determinism():
    ds = PC.dataset("gopro9_division")
    off, ab, xy, thr, mode = PC.packed(ds, ds["uv"], True)
    n0 = int(off[1])
    # 2000 views of 40 corners: the 30 views over and over
    reps = 67
    big_off = np.concatenate([[0], np.cumsum(np.tile(np.diff(off), reps))])[:2001]
    big_ab, big_xy = np.tile(ab, (reps, 1))[:big_off[-1]], np.tile(xy, (reps, 1))[:big_off[-1]]
    a = RI.planar_ransac(big_off, big_ab, big_xy, mode, thr)
    b = RI.planar_ransac(big_off, big_ab, big_xy, mode, thr)
    for x, y in zip(a[:4], b[:4]):
        assert x.tobytes() == y.tobytes()                      # same seed, same bytes
    assert a[0].all() and np.array_equal(a[1], np.diff(big_off))
    # one view of 1500 corners (beyond the LDS staging): a dense board under the pose of view 0, 10 % of them bad
    from openimucameracalibrator_amd import camera_calibrator as CC
    g = np.stack(np.meshgrid(np.linspace(0, 0.147, 50), np.linspace(0, 0.105, 30)), -1).reshape(-1, 2)
    R = CC.angle_axis_to_rotation(ds["pose_true"][0, 3:])
    pc = (np.concatenate([g, np.zeros((1500, 1))], 1) - ds["pose_true"][0, :3]) @ R.T
    feat = pc[:, :2] / pc[:, 2:] + np.random.default_rng(5).normal(0, 2e-4, (1500, 2))
    bad = np.arange(0, 1500, 10)
    feat[bad] += 0.05
    for m in (0, 1):
        inl, num, q, pose, counts = RI.planar_ransac([0, 1500], g, feat, m, thr, num_hypotheses=1024, want_counts=True)
        r = PR.run([0, 1500], g, feat, m, thr, num_hypotheses=1024, want_counts=True)
        assert counts.shape == (1, 1024) and np.array_equal(inl, r[0]) and num[0] == r[1][0] >= 1300
        assert (m == 0 or not inl[bad].any()) and np.mean(counts == r[4]) > 0.95
    # views of 0-4 corners and a view whose corners are collinear on the board, between two good views
    line = np.where(np.abs(ab[:n0, 1] - ab[0, 1]) < 1e-9)[0]
    assert len(line) >= 5
    sizes = [n0, 0, 1, 2, 3, 4, len(line), int(off[2] - off[1])]
    o = np.concatenate([[0], np.cumsum(sizes)])
    pick = np.concatenate([np.arange(n0), np.arange(1), np.arange(2), np.arange(3), np.arange(4), line, np.arange(off[1], off[2])]).astype(int)
    for m in (0, 1):
        inl, num, q, pose, _ = RI.planar_ransac(o, ab[pick], xy[pick], m, thr)
        assert num[0] == n0 and list(num[1:6]) == [0] * 5 and num[6] < 6 and num[7] == sizes[7]
        assert not inl[o[1]:o[6]].any() and np.all(q[1:6] == 0)
    with pytest.raises(ValueError):
        RI.planar_ransac(o, np.full_like(ab[pick], np.inf), xy[pick], 0, thr)
    assert RI.planar_ransac([0], np.zeros((0, 2)), np.zeros((0, 2)), 0, thr)[1].shape == (0,)


@pytest.mark.parametrize("camera", ["gopro9_division", "gopro6_fisheye", "pinhole"])
def test_applications_survive_bad_corners_on_the_device(camera):
    """tests/test_planar_ransac.py's end-to-end case with the HIP library as the RANSAC and the bundle-adjustment backend."""
    from test_planar_ransac import run_applications
    run_applications(camera, None, None)
