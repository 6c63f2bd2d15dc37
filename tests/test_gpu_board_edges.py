"""The board detector's kernels (csrc/board.hip) on the MI355X against the restatement at their edges (tests/board_cases.py; the
premises of every case are asserted without a GPU in tests/test_board_cases.py): image sizes around the response kernel's
64 x 16 tile and its word staging, radii 1, 3 and 8, thresholds 0, 0.5 and 1, exact ties, frames over the candidate cap, resize
factors with tied and zero weights, single sub-pixel steps and the marker means against the restatement in extended precision."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import board_cases as K  # noqa: E402
from openimucameracalibrator_amd import board_extractor as BE  # noqa: E402

pytestmark = pytest.mark.gpu

# Allowed multiples of the yardstick (largest |float64 restatement - longdouble restatement| of the case, floored at eps64 * max(w, h)
# for points and eps64 * 255 for means): four times the largest multiple measured on the MI355X against the longdouble
# restatement, rounded up (DESIGN.md 3.z has the table).  Only the summation order and the device's exp differ, and the seeds are
# fixed.  Measured: one step 0.648 (random 50 x 197, r = 1), three steps 1.286 (small board 4, r = 5), marker means 1.000.
SUBPIX_MULTIPLE = {1: 3.0, 3: 6.0}
MARKER_MULTIPLE = 4.0


def _assert_integer_stages(st, ncand, ref, what):
    for key in ("gray", "blurred", "response", "polarity"):
        assert st[key].dtype == ref[key].dtype and np.array_equal(st[key], ref[key]), (what, key)
    for f, yx in enumerate(ref["candidates"]):
        assert ncand[f] == len(yx) and np.array_equal(st["candidates"][f], yx), (what, "candidates", f)


@pytest.mark.parametrize("r", K.RADII)
def test_integer_stages_at_tile_edges(r):
    """gray, blurred, response, polarity and candidates, bit for bit: random frames, a frame of only 0 and 255, the checker whose
    every candidate and thousands of whose polarities are ties, and a constant frame, at every size around the tile."""
    for h, w in K.sizes_for(r):
        frames = K.edge_frames(h, w)
        for thr in K.THRESHOLDS:
            corners, found, ncand, rep, st = BE.radon_detect(frames, 1.0, 4, 3, stages=True, radius=r, threshold_rel=thr, max_candidates=K.CAP_WIDE)
            ref = K.edge_stages(h, w, r, thr)
            _assert_integer_stages(st, ncand, ref, (h, w, r, thr))
            assert rep["frames_overflow"] == 0 and rep["num_candidates"] == ncand.sum() and (rep["output_height"], rep["output_width"]) == (h, w)
            if thr == 1.0:
                assert ncand.sum() == 0                 # the comparison is strict
            assert ncand[4] == 0 and not found.any() and np.isnan(corners).all()


@pytest.mark.parametrize("factor", K.RESIZE_FACTORS)
def test_resize_factors_gray_and_bgr(factor):
    for h, w in K.RESIZE_SOURCES:
        for channels in (1, 3):
            frames = K.random_frames(h, w, channels)
            corners, found, ncand, rep, st = BE.radon_detect(frames, factor, 4, 3, stages=True, radius=1, threshold_rel=0.5, max_candidates=K.CAP_WIDE)
            ref = K.stages(frames, factor, 1, 0.5)
            assert (rep["output_height"], rep["output_width"]) == ref["gray"].shape[1:]
            _assert_integer_stages(st, ncand, ref, (factor, h, w, channels))


@pytest.mark.parametrize("f", [0, 1])
def test_overflow_at_the_cap_and_one_below(f):
    ref, counts = K.overflow_counts()
    frame = K.random_frames(*K.OVERFLOW_SIZE)[f:f + 1]
    n = counts[f]
    opt = dict(radius=K.OVERFLOW_RADIUS, threshold_rel=0.0)
    corners, found, ncand, rep, st = BE.radon_detect(frame, 1.0, 4, 3, stages=True, max_candidates=n, **opt)
    assert ncand[0] == n and rep["frames_overflow"] == 0 and rep["num_candidates"] == n
    assert np.array_equal(st["candidates"][0], ref["candidates"][f])
    corners, found, ncand, rep, st = BE.radon_detect(frame, 1.0, 4, 3, stages=True, max_candidates=n - 1, **opt)
    assert ncand[0] == n and rep["frames_overflow"] == 1 and rep["num_candidates"] == n and rep["frames_found"] == 0
    assert not found[0] and np.isnan(corners).all() and tuple(st["grid_shape"][0]) == (0, 0)


def test_overflowing_frame_between_boards():
    """batch = 2 over constant | board, over the cap | board turned by 90 degrees, random (exactly at the cap): the frame that shares a
    launch with the overflowing one, and the frames after it, have exactly their own candidates."""
    frames, opt, counts, (rc, rf, dbg) = K.mixed_batch()
    corners, found, ncand, rep, st = BE.radon_detect(frames, 1.0, 4, 3, stages=True, batch=2, **opt)
    assert ncand.tolist() == counts
    assert rep["frames_found"] == rf.sum() == 2 and rep["frames_overflow"] == 1 and rep["num_candidates"] == sum(counts)
    assert np.array_equal(found, rf)
    for f in (0, 1, 3, 4):
        assert np.array_equal(st["candidates"][f], dbg["candidates"][f][0]), f
        assert np.abs(st["refined"][f] - dbg["refined"][f]).max(initial=0.0) <= 1e-3
    for f in (1, 3):
        assert tuple(st["grid_shape"][f]) == dbg["grid_shape"][f] and np.array_equal(st["grid"][f], dbg["grid"][f])
        assert np.abs(corners[f] - rc[f]).max() <= 1e-3            # the same ids: a different id moves a corner by a square
    assert np.isnan(corners[[0, 2, 4]]).all() and all(st["grid"][f] is None for f in (0, 2, 4))


def _check_subpix(name, got, case, limit):
    keep = ~case["aside"]
    assert got.shape == case["ld"].shape
    err = float(np.abs(got[keep].astype(K.LD) - case["ld"][keep]).max()) if keep.any() else 0.0
    multiple = err / case["yardstick"]
    print("MULTIPLE subpix %s candidates %d aside %d yardstick %.3e (floor %.3e) device-longdouble %.3e multiple %.3f"
          % (name, len(keep), int(case["aside"].sum()), case["yardstick"], case["floor"], err, multiple))
    assert multiple <= limit, (name, multiple)


@pytest.mark.parametrize("iterations", K.SUBPIX_STEPS)
@pytest.mark.parametrize("r,size", K.SUBPIX_RANDOM)
def test_subpix_steps_on_random_frames(r, size, iterations):
    """One and three steps with eps = 0 (no stopping rule can flip) from every candidate of random frames at threshold 0, a quarter to a
    half of which have clamped samples; the three-step cases take the reset and the leaves-the-image branches."""
    ref, cases = K.subpix_random_case(r, size, iterations)
    _, _, ncand, _, st = BE.radon_detect(K.random_frames(*size), 1.0, 4, 3, stages=True, radius=r, threshold_rel=0.0, max_candidates=K.CAP_WIDE,
                                         subpix_iterations=iterations, subpix_eps=0.0)
    _assert_integer_stages(st, ncand, ref, (r, size))
    for f, case in enumerate(cases):
        _check_subpix("random r=%d %dx%d steps=%d frame=%d" % (r, size[0], size[1], iterations, f), st["refined"][f], case, SUBPIX_MULTIPLE[iterations])


@pytest.mark.parametrize("iterations", K.SUBPIX_STEPS)
@pytest.mark.parametrize("k", range(len(K.SMALL_BOARDS)))
def test_subpix_steps_on_small_boards(k, iterations):
    W, H, sq, size, r, rot = K.SMALL_BOARDS[k]
    ref, cases = K.subpix_board_case(k, iterations)
    _, _, ncand, _, st = BE.radon_detect(K.board_frame(k)[None], 1.0, W, H, stages=True, radius=r, subpix_iterations=iterations, subpix_eps=0.0)
    _assert_integer_stages(st, ncand, ref, k)
    _check_subpix("board %d r=%d steps=%d" % (k, r, iterations), st["refined"][0], cases[0], SUBPIX_MULTIPLE[iterations])


@pytest.mark.parametrize("k", range(len(K.SMALL_BOARDS)))
def test_small_boards_grid_marker_means_and_corners(k):
    """The whole detector at the default options but the radius: grid, shape, found, ids and corners as the restatement; the marker
    kernel's disc and ring means against the longdouble cell_means of the very corners the kernel read."""
    W, H, sq, size, r, rot = K.SMALL_BOARDS[k]
    rc, rf, dbg = K.board_detection(k)
    corners, found, ncand, rep, st = BE.radon_detect(K.board_frame(k)[None], 1.0, W, H, stages=True, radius=r)
    assert np.array_equal(st["gray"], dbg["gray"]) and np.array_equal(st["blurred"], dbg["blurred"])
    assert np.array_equal(st["response"], dbg["response"]) and np.array_equal(st["polarity"], dbg["polarity"])
    assert ncand[0] == len(dbg["candidates"][0][0]) and np.array_equal(st["candidates"][0], dbg["candidates"][0][0])
    assert tuple(st["grid_shape"][0]) == dbg["grid_shape"][0] and np.array_equal(st["grid"][0], dbg["grid"][0])
    assert found[0] and rf[0] and rep["frames_found"] == 1
    assert np.abs(st["refined"][0] - dbg["refined"][0]).max() <= 1e-3
    assert np.abs(corners - rc).max() <= 1e-3                       # the same ids: a different id moves a corner by a square
    m = K.marker_case(st["blurred"][0], st["refined"][0][st["grid"][0]])
    for name in ("disc", "ring"):
        err = float(np.abs(st[name][0].astype(K.LD) - m[name]).max())
        multiple = err / m["yard_" + name]
        print("MULTIPLE marker board %d %s yardstick %.3e device-longdouble %.3e multiple %.3f" % (k, name, m["yard_" + name], err, multiple))
        assert multiple <= MARKER_MULTIPLE, (k, name, multiple)
