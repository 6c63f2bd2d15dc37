"""View bundle adjustment on the device against the 50-digit restatement (ba_rows_reference.py) at the edges of the code:
Evaluate's cost to 1e-14 relative, J^T J and J^T r entry by entry -- every entry scaled by its own d_i d_j -- within
DEVICE_FACTOR x the float64 yardstick of the case (YARDSTICK; measured on the host by test_ba_rows_reference.py), and the first
LM step of the one-launch pose refinement.  Cases: ba_rows_cases.py.  Every figure is printed before it is asserted."""
import mpmath as mp
import numpy as np
import pytest

import ba_rows_cases as K
import ba_rows_reference as R
from openimucameracalibrator_amd import camera_calibrator as CC

pytestmark = pytest.mark.gpu

COST_BOUND = 1e-14


def device_adjuster(problem, huber_width):
    ba = CC.ViewBundleAdjuster()
    ba.SetOption("huber_width", huber_width)
    ba.SetCamera(problem["model"], problem["intrinsics"])
    ba.SetScenePoints(problem["points"])
    ba.SetViews(problem["poses"], problem["corner_offset"], problem["uv"], problem["point_ids"])
    if not problem["variable_points"].all():
        ba.SetVariablePoints(problem["variable_points"])
    return ba


def all_mask(problem):
    return (1 << len(problem["intrinsics"])) - 1


def check(figures):
    """figures: (name, value, bound).  Prints all, then asserts all."""
    worst = max(figures, key=lambda f: f[1] / f[2] if f[2] > 0 else (0.0 if f[1] == 0 else np.inf))
    for name, value, bound in figures:
        print("%-40s %.3e  bound %.3e  ratio %.3f" % (name, value, bound, value / bound if bound > 0 else (0.0 if value == 0 else np.inf)))
    print("largest: %s %.3e = %.3f x its bound" % (worst[0], worst[1], worst[1] / worst[2] if worst[2] > 0 else np.inf))
    bad = [f for f in figures if not f[1] <= f[2]]
    assert not bad, bad


@pytest.mark.parametrize("name", list(K.ROW_DATASETS) + ["huber"])
def test_rows_one_observation_per_view(name):
    """(a) the view's 6 x 6 block and its cross block with the intrinsics are the products of one row pair: rotation branches
    (theta = 0, 1e-8, 1.6e-8, around 0.01, near and beyond pi), the homogeneous point, the camera models' own edges, the Huber kink."""
    prob, labels, hw = K.row_dataset(name)
    cost, Href, gref = R.evaluate(prob, K.POSE, all_mask(prob), hw)
    ba = device_adjuster(prob, hw)
    c, H, g = ba.Evaluate(K.POSE, all_mask(prob))
    assert H.shape == Href.shape
    views, corner = K.view_blocks(prob, K.POSE, all_mask(prob))
    figures = [("cost", abs(float(c - cost)) / float(cost), COST_BOUND)]
    for v, lab in enumerate(labels):
        figures.append((lab, R.normal_equations_error(H, g, Href, gref, cost, views[v], np.concatenate([views[v], corner])),
                        R.DEVICE_FACTOR * R.yardstick("a/%s/%s" % (name, lab))))
    figures.append(("corner", R.normal_equations_error(H, g, Href, gref, cost, corner, corner), R.DEVICE_FACTOR * R.yardstick("a/%s/corner" % name)))
    check(figures)


@pytest.mark.parametrize("config", list(K.CHUNK_CONFIGS))
def test_chunk_and_column_edges(config):
    """(b) views of 1, 2, 63, 64, 65, 128, 129 and 0 observations; 17, 16 and 2 columns of the Gram kernel; orientation only; Huber."""
    camera, flags, free, hw = K.CHUNK_CONFIGS[config]
    prob = K.chunk_dataset(camera)
    mask = CC.intrinsics_mask(prob["model"], free)
    cost, Href, gref = R.evaluate(prob, flags, mask, hw)
    ba = device_adjuster(prob, hw)
    c, H, g = ba.Evaluate(flags, mask)
    assert H.shape == Href.shape
    d = len(R.pose_columns(flags))
    empty = K.CHUNK_COUNTS.index(0)
    assert not H[empty * d:(empty + 1) * d].any() and not g[empty * d:(empty + 1) * d].any()
    check([("cost", abs(float(c - cost)) / float(cost), COST_BOUND),
           ("H", R.entrywise_error(H, Href)[0], R.DEVICE_FACTOR * R.yardstick("b/" + config)),
           ("g", R.gradient_error(g, gref, Href, cost)[0], R.DEVICE_FACTOR * R.yardstick("b/" + config))])


def test_board_points_unwarped_board_and_homogeneous_scales():
    """(c) BA_POINTS on the unwarped board (the origin corner takes the sigma <= eps branch), scales 1, -1.5, 1e-3, 1e3 (x_w <= 0),
    points seen in 1, 64 and 65 views, two constant points; one LM iteration keeps every point's norm and the constant points."""
    prob = K.points_dataset()
    hw = R.LM_DEFAULTS["huber_width"]
    cost, Href, gref = R.evaluate(prob, CC.BA_POINTS, 0, hw)
    ba = device_adjuster(prob, hw)
    c, H, g = ba.Evaluate(CC.BA_POINTS, 0)
    assert H.shape == Href.shape == (3 * 46, 3 * 46)
    check([("cost", abs(float(c - cost)) / float(cost), COST_BOUND),
           ("H", R.entrywise_error(H, Href)[0], R.DEVICE_FACTOR * R.yardstick("c/points")),
           ("g", R.gradient_error(g, gref, Href, cost)[0], R.DEVICE_FACTOR * R.yardstick("c/points"))])
    s = ba.Optimize(1, CC.BA_POINTS, 0)
    assert s["num_iterations"] == 1
    pts = ba.GetScenePoints()
    var = prob["variable_points"].astype(bool)
    assert np.array_equal(pts[~var], prob["points"][~var])
    assert (pts[var] != prob["points"][var]).any(axis=1).all(), "the step was not taken"
    n0 = np.sqrt((prob["points"].astype(R.LD) ** 2).sum(axis=1)); n1 = np.sqrt((pts.astype(R.LD) ** 2).sum(axis=1))
    drift = (np.abs(n1 - n0) / n0).astype(np.float64)
    print("largest norm drift %.3e = %.2f eps" % (drift[var].max(), drift[var].max() / R.EPS))
    assert drift[var].max() <= 4 * R.EPS


def cost_allowance(problem, v, pose, huber_width):
    """What float64 leaves of one view's cost: every pixel coordinate carries a few roundings of its own size (8 eps |px| allowed),
    and the cost moves by rho' r per unit of residual."""
    sub = R.one_view(problem, v)
    q = [float(x) for x in sub["intrinsics"]]
    total = 0.0
    for c in range(len(sub["uv"])):
        r = R.residual(mp.fp, sub["model"], q, [float(x) for x in pose], [float(x) for x in sub["points"][sub["point_ids"][c]]], [float(x) for x in sub["uv"][c]])
        w = float(R.huber(mp.fp, huber_width, r[0] * r[0] + r[1] * r[1])[1]) ** 2
        total += w * sum(abs(r[e]) * (abs(r[e]) + abs(float(sub["uv"][c][e]))) for e in range(2))
    return 8 * R.EPS * total


@pytest.mark.parametrize("flag_name", list(K.VIEW_FLAGS))
def test_optimize_views_first_iteration(flag_name):
    """(d) OptimizeViews(1, flags) -- pose, position only, orientation only (ba_optimize_views_kernel<3> with idx = {3, 4, 5}) -- on
    views of 4, 40 and 65 observations and one that starts at w = 0: one iteration, the pose of lm_first_step on the 50-digit
    normal equations, and the 50-digit cost at the pose the kernel kept."""
    prob, flags = K.views_dataset(), K.VIEW_FLAGS[flag_name]
    hw = R.LM_DEFAULTS["huber_width"]
    ref = R.first_step_of_views(prob, flags)
    ba = device_adjuster(prob, hw)
    it, fc = ba.OptimizeViews(1, flags)
    poses = ba.GetPoses()
    assert np.array_equal(it, np.ones(len(it), dtype=it.dtype)), it
    figures = []
    for v, lab in enumerate(K.VIEW_LABELS):
        assert abs(ref[v]["relative_decrease"] - R.LM_DEFAULTS["min_relative_decrease"]) >= 0.1
        assert ref[v]["accepted"] == (not np.array_equal(poses[v], prob["poses"][v])), lab
        untouched = [k for k in range(6) if k not in R.pose_columns(flags)]
        assert np.array_equal(poses[v, untouched], prob["poses"][v, untouched])
        err = float(np.abs(poses[v] - ref[v]["kept"]).max() / np.abs(ref[v]["step"].astype(np.float64)).max())
        figures.append(("pose " + lab, err, R.DEVICE_FACTOR * R.yardstick("d/%s/%s" % (flag_name, lab))))
        kept_cost = float(R.cost_at(R.one_view(prob, v), poses[v:v + 1], hw)[0])
        figures.append(("final_cost " + lab, abs(fc[v] - kept_cost), cost_allowance(prob, v, poses[v], hw)))
    check(figures)
