"""The elimination plan of the block cyclic reduction (kernels_bcr.hip: bcr_plan, exported as oicc_debug_bcr_plan), on the host alone.

Level l of the plan has the active blocks origin + k stride, k < active, and eliminates those of one parity.  An odd number of active
blocks takes the even positions (both ends are pivots), an even number the odd ones, so that the number of inversions in sequence is
floor(log2 n) + 1.  Checked for every n in 1..4096: the depth, that the levels partition the blocks, that the pivots of a level form an
independent set whose neighbours are exactly the next level's adjacent active blocks, and that the coupling tables of the levels are
disjoint and fit the workspace.  The distributed reduction's order (odd positions only, with and without a ghost block) is the order
the library had before and is checked to be exactly that."""
import ctypes

import numpy as np
import pytest

from openimucameracalibrator_amd import _abi, _lib

CAP = 40


def plan(n, ghost=0, odd_only=0):
    b = _lib.load_bcr_plan()
    levels = np.zeros((CAP, 6), dtype=np.int64)
    info = np.zeros(3, dtype=np.int64)
    nlev = b.plan(n, ghost, odd_only, levels.ctypes.data_as(_abi.c_i64p), CAP, info.ctypes.data_as(_abi.c_i64p))
    assert nlev >= 0, (n, nlev)
    return [tuple(int(v) for v in levels[l]) for l in range(nlev)], int(info[0]), int(info[1]), int(info[2])


def check_structure(n, ghost, odd_only):
    """What holds for every plan; returns (levels, last)."""
    levels, last, off_end, reserved = plan(n, ghost, odd_only)
    active = list(range(n))
    eliminated = []
    next_slot = 0
    for l, (o, s, p, m, npiv, off) in enumerate(levels):
        assert p in (0, 1) and m >= 2
        assert [o + k * s for k in range(m)] == active, (n, l)            # the survivors of the level before, in order
        piv_k = [k for k in range(m) if k % 2 == p]
        assert len(piv_k) == npiv and npiv >= 1
        assert all(b - a == 2 for a, b in zip(piv_k, piv_k[1:]))             # pairwise non-adjacent in the active list
        survivors = [active[k] for k in range(m) if k % 2 != p]
        where = {v: ix for ix, v in enumerate(survivors)}
        for k in piv_k:                                                      # a pivot's neighbours survive, and are adjacent afterwards
            nb = [active[j] for j in (k - 1, k + 1) if 0 <= j < m]
            assert nb and all(v in where for v in nb)
            if len(nb) == 2:
                assert where[nb[1]] == where[nb[0]] + 1
        # couplings (k, k + 1) at slot off + k, + the one to the ghost block: one table per level, behind the one before
        assert off == next_slot
        next_slot = off + (m - 1 + ghost)
        eliminated += [active[k] for k in piv_k]
        active = survivors
    assert active == [last]
    assert sorted(eliminated + [last]) == list(range(n))                     # every block is a pivot exactly once, or is the last one
    assert off_end == next_slot
    assert off_end + ghost <= reserved and reserved == 2 * (n + ghost) + 40  # the table behind the last level holds (last block, ghost)
    return levels, last


def test_depth_is_floor_log2_plus_one_for_every_block_count():
    for n in range(1, 4097):
        levels, last = check_structure(n, 0, 0)
        assert len(levels) + 1 == n.bit_length(), n                         # floor(log2 n) + 1 inversions in sequence
        for (o, s, p, m, npiv, off) in levels:
            assert p == (0 if m % 2 else 1)
            assert npiv == (m + 1) // 2
        if n & (n - 1) == 0:
            assert all(lv[2] == 1 for lv in levels) and last == 0            # a power of two: the order it always had


def test_the_cases_the_issue_names():
    levels, last = check_structure(29, 0, 0)
    assert [lv[4] for lv in levels] == [15, 7, 4, 2] and last == 13
    assert [lv[2] for lv in levels] == [0, 1, 0, 0]
    for n, depth in ((1407, 11), (3, 2), (5, 3), (9, 4), (17, 5), (513, 10)):
        levels, _ = check_structure(n, 0, 0)
        assert len(levels) + 1 == depth


@pytest.mark.parametrize("ghost", [0, 1])
def test_distributed_order_is_odd_positions_only(ghost):
    for n in list(range(1, 300)) + [511, 512, 513, 1407, 4096]:
        levels, last = check_structure(n, ghost, 1)
        assert last == 0
        assert len(levels) == (n - 1).bit_length()                           # ceil(log2 n) levels
        for l, (o, s, p, m, npiv, off) in enumerate(levels):
            assert (o, s, p, m, npiv) == (0, 1 << l, 1, (n + (1 << l) - 1) >> l, ((n + (1 << l) - 1) >> l) // 2)


def test_invalid_arguments():
    b = _lib.load_bcr_plan()
    levels = np.zeros((CAP, 6), dtype=np.int64); info = np.zeros(3, dtype=np.int64)
    lp, ip = levels.ctypes.data_as(_abi.c_i64p), info.ctypes.data_as(_abi.c_i64p)
    assert b.plan(0, 0, 0, lp, CAP, ip) == -1
    assert b.plan(29, 0, 0, lp, 3, ip) == -1                                 # four levels do not fit three rows
    assert b.plan(29, 0, 0, ctypes.cast(None, _abi.c_i64p), CAP, ip) == -1
    assert b.plan(1, 0, 0, lp, CAP, ip) == 0 and info[0] == 0
