"""The premises of tests/board_cases.py, asserted with the restatement alone, so that no GPU test of the board detector's edges
(tests/test_gpu_board_edges.py) can pass vacuously: the ties are there, the boards are found, the overflow frames are over the cap,
the sub-pixel cases reach the branches they claim, and no candidate sits on a decision the comparison tolerance could flip."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import board_cases as K  # noqa: E402
import board_restatement as BR  # noqa: E402
from openimucameracalibrator_amd import _abi  # noqa: E402


def test_abi_struct_sizes():
    assert ctypes.sizeof(_abi.BoardOptions) == 32
    assert ctypes.sizeof(_abi.BoardReport) == 4 * 4 + 8 + 7 * 8
    assert ctypes.sizeof(_abi.BoardStages) == 4 * 8 + 2 * 4 + 6 * 8
    assert _abi.BoardStages.extended.offset == 36 and _abi.BoardStages.polarity.offset == 40      # the old struct is a prefix


def test_longdouble_is_extended_precision():
    assert np.finfo(K.LD).eps <= 2.0 ** -63


def test_sizes_cover_the_tile_edges():
    assert K.sizes_for(1)[0] == (5, 5) and K.sizes_for(8)[0] == (19, 19)
    assert (16, 64) in K.sizes_for(3) and (16, 64) not in K.sizes_for(8) and (17, 65) not in K.sizes_for(8)
    assert sorted({w % 4 for _, w in K.TILE_SIZES}) == [0, 1, 2, 3]
    for h, w in K.TILE_SIZES:
        f = K.edge_frames(h, w)
        assert f.shape == (5, h, w) and set(np.unique(f[2])) == {0, 255} and np.ptp(f[4]) == 0


@pytest.mark.parametrize("r", K.RADII)
def test_ties_are_present(r):
    """50 x 197: every candidate of the checker has an in-window tie and thousands of its pixels a tied brightest line; random
    frames have almost none of either, which is why the checker is there."""
    st = K.edge_stages(50, 197, r, 0.0)
    n = [len(c) for c in st["candidates"]]
    ties = [K.nms_ties(st["response"][f], st["candidates"][f], r) for f in range(5)]
    pt = K.polarity_ties(st["blur16"], r)
    print("r=%d candidates %s nms ties %s polarity ties %s" % (r, n, ties, pt.tolist()))
    assert n[3] == {1: 84, 3: 80, 8: 48}[r] and ties[3] == n[3]
    assert pt[3] >= 400 and pt[2] >= 100
    assert n[4] == 0 and st["response"][4].max() == 0.0            # the constant frame: maximum 0, the strict threshold keeps nothing
    assert pt[4] == (50 - 2 * r) * (197 - 2 * r)                   # and every interior pixel ties all four directions
    assert all(len(c) == 0 for c in K.edge_stages(50, 197, r, 1.0)["candidates"])        # strict: nothing survives 1.0
    assert sum(len(c) for c in K.edge_stages(50, 197, r, 0.5)["candidates"]) > 0


@pytest.mark.parametrize("k", range(len(K.SMALL_BOARDS)))
def test_small_boards_are_found(k):
    W, H, sq, size, r, rot = K.SMALL_BOARDS[k]
    corners, found, dbg = K.board_detection(k)
    assert K.board_frame(k).shape == size and found[0] and not np.isnan(corners).any()
    assert dbg["grid_shape"][0] == ((H, W) if k == 2 else (W, H))          # 97 degrees: A and B swapped
    assert dbg["disc"][0].shape == (dbg["grid_shape"][0][0] - 1, dbg["grid_shape"][0][1] - 1)
    # ids: corner i*W + j lies a square from its neighbours along both axes
    c = corners[0].reshape(H, W, 2)
    assert np.allclose(np.hypot(*np.diff(c, axis=1).reshape(-1, 2).T), sq, rtol=0.15)
    assert np.allclose(np.hypot(*np.diff(c, axis=0).reshape(-1, 2).T), sq, rtol=0.15)


def test_overflow_frames_exceed_the_cap():
    st, counts = K.overflow_counts()
    print("50 x 197, r = 1, threshold 0: candidates", counts)
    assert min(counts) > 1000 and max(counts) < K.CAP_WIDE
    frames, opt, counts, (corners, found, dbg) = K.mixed_batch()
    cap = opt["max_candidates"]
    print("mixed batch: candidates %s, cap %d" % (counts, cap))
    assert counts[0] == 0 and counts[2] > cap and counts[4] == cap          # none, over the cap, exactly at the cap
    assert counts[1] <= cap and counts[3] <= cap and cap >= 12
    assert found.tolist() == [False, True, False, True, False]
    assert dbg["grid_shape"][1] == (4, 3) and dbg["grid_shape"][3] == (3, 4)
    assert [bool(o) for _, o in dbg["candidates"]] == [False, False, True, False, False]


def _branches(cases):
    return {k: int(sum(c[k].sum() for c in cases)) for k in ("aside", "reset", "left", "singular")}


def test_subpix_cases_reach_their_branches():
    """Branches reached (longdouble run, eps = 0): the "moved more than the window" reset in every three-step case at r = 1 (a
    single step never moves that far here), the leaves-the-image stop in the three-step 50 x 197 case; the singular-matrix stop in
    none (a random frame has no flat window).  No candidate is set aside."""
    total = {}
    for r, size in K.SUBPIX_RANDOM:
        for it in K.SUBPIX_STEPS:
            st, cases = K.subpix_random_case(r, size, it)
            b = _branches(cases)
            n = sum(len(c["aside"]) for c in cases)
            print("r=%d %s steps=%d candidates %d %s yardstick/floor %s" % (r, size, it, n, b, ["%.2f" % (c["yardstick"] / c["floor"]) for c in cases]))
            total[(r, size, it)] = b
            for c in cases:
                assert c["aside"].sum() <= 0.02 * len(c["aside"])
                assert c["tol"] < 1e-9
            # a quarter to a half of the candidates have clamped samples: within win + 1 of the border
            if r == 1:
                h, w = size
                yx = np.concatenate(st["candidates"]); m = r + 3
                frac = np.mean((yx[:, 0] < m) | (yx[:, 0] >= h - m) | (yx[:, 1] < m) | (yx[:, 1] >= w - m))
                assert 0.15 <= frac <= 0.6, frac
    assert total[(1, (17, 65), 3)]["reset"] >= 5 and total[(1, (50, 197), 3)]["reset"] >= 50
    assert total[(1, (50, 197), 3)]["left"] >= 1
    for k in range(len(K.SMALL_BOARDS)):
        for it in K.SUBPIX_STEPS:
            st, cases = K.subpix_board_case(k, it)
            assert cases[0]["aside"].sum() == 0 and len(cases[0]["aside"]) >= K.SMALL_BOARDS[k][0] * K.SMALL_BOARDS[k][1]


def test_longdouble_restatement_agrees_with_float64():
    """The same statements in two precisions: they agree to a few eps64 * size on the boards (the yardstick of the GPU comparison),
    and the float64 path of cell_means is the one detect() uses."""
    for k in range(len(K.SMALL_BOARDS)):
        corners, found, dbg = K.board_detection(k)
        G = dbg["grid"][0]
        m = K.marker_case(dbg["blurred"][0], dbg["refined"][0][G])
        assert m["disc"].dtype == K.LD and m["yard_disc"] <= 8 * K.EPS64 * 255 and m["yard_ring"] <= 8 * K.EPS64 * 255
        d64, r64 = BR.cell_means(dbg["blurred"][0], dbg["refined"][0][G])
        assert np.array_equal(d64, dbg["disc"][0]) and np.array_equal(r64, dbg["ring"][0])
        st, cases = K.subpix_board_case(k, 3)
        assert cases[0]["ld"].dtype == K.LD and cases[0]["yardstick"] <= 8 * cases[0]["floor"]
