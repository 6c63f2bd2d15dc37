"""Which level's back substitution rides in the last block's launch (kernels_bcr.hip: bcr_fold_level, exported as
oicc_debug_bcr_fold_plan), on the host alone.

The back substitution of the block cyclic reduction pairs the levels from the bottom up; an even number of levels leaves level
nlev - 2 alone in a launch (bcri_backward_kernel).  A whole-band solve runs that level inside the last block's launch instead
(bcri_last_backward_kernel: one workgroup per pivot of the level, each repeating the last block's work).  The rule is restated here
from the plan (oicc_debug_bcr_plan) for every n <= 4096:
  - folded iff the option is on, there is no ghost block and no block offset, and the level count is even and >= 2;
  - the folded level is nlev - 2 and has 2 to 4 pivots;
  - every neighbour of each of its pivots is the last block or one of the top level's pivots (last -+ the top stride) -- the blocks
    whose solution the last block's workgroup holds in LDS;
  - nothing folds with a ghost block, a block offset or the option off.
"""
import numpy as np

from openimucameracalibrator_amd import _abi, _lib

CAP = 40
INVALID = -2 ** 31


def plan_info(n, ghost=0, odd_only=0):
    b = _lib.load_bcr_plan()
    levels = np.zeros((CAP, 6), dtype=np.int64)
    info = np.zeros(3, dtype=np.int64)
    nlev = b.plan(n, ghost, odd_only, levels.ctypes.data_as(_abi.c_i64p), CAP, info.ctypes.data_as(_abi.c_i64p))
    assert nlev >= 0, (n, nlev)
    return [tuple(int(v) for v in levels[l]) for l in range(nlev)], int(info[0])


def fold_plan(n, ghost=0, odd_only=0, b0=0, on=1):
    return int(_lib.load_bcr_plan().fold_plan(n, ghost, odd_only, b0, on))


def pivots(level):
    """The blocks of a level's pivots, and for each its neighbours among the level's active blocks."""
    o, s, p, m, npiv, _ = level
    ks = [k for k in range(m) if k % 2 == p]
    assert len(ks) == npiv
    return [(o + k * s, [o + j * s for j in (k - 1, k + 1) if 0 <= j < m]) for k in ks]


def test_whole_band_every_block_count():
    folded = 0
    for n in range(1, 4097):
        levels, last = plan_info(n)
        nlev = len(levels)
        want = nlev - 2 if (nlev >= 2 and nlev % 2 == 0) else -1
        got = fold_plan(n)
        assert got == want, (n, nlev, got)
        assert fold_plan(n, on=0) == -1, n                        # the option off: the parent's launches
        if got < 0:
            continue
        folded += 1
        top = levels[nlev - 1]
        s_top = top[1]
        top_blocks = [last] + [b for b, _ in pivots(top)]
        assert set(top_blocks) <= {last, last - s_top, last + s_top} and len(top_blocks) in (2, 3)
        lv = levels[got]
        assert 2 <= lv[4] <= 4 and 4 <= lv[3] <= 7, (n, lv)
        for blk, nbs in pivots(lv):
            assert 1 <= len(nbs) <= 2 and blk not in top_blocks
            for nb in nbs:
                assert nb in top_blocks, (n, blk, nb, top_blocks)   # its solution is in the last block's LDS
    assert folded > 1000


def test_spot_values():
    assert fold_plan(29) == 2 and plan_info(29)[0][2][4] == 4     # the flagship: pivots 15 / 7 / 4 / 2
    assert fold_plan(17) == 2 and plan_info(17)[0][2][4] == 2     # 9 / 4 / 2 / 1
    assert fold_plan(4) == 0 and fold_plan(5) == 0 and fold_plan(7) == 0 and fold_plan(16) == 2
    assert fold_plan(1407) == 8 and len(plan_info(1407)[0]) == 10
    for n in (8, 9, 2, 3, 1):
        assert fold_plan(n) == -1, n
    # what the GPU cases rely on
    assert pivots(plan_info(4)[0][0]) == [(1, [0, 2]), (3, [2])] and plan_info(4)[1] == 0
    assert pivots(plan_info(5)[0][0]) == [(0, [1]), (2, [1, 3]), (4, [3])] and plan_info(5)[1] == 1
    assert plan_info(7)[0][0][4] == 4 and plan_info(7)[0][1][4] == 2
    assert plan_info(16)[1] == 0 and len(plan_info(16)[0]) == 4


def test_distributed_ranges_keep_their_launches():
    for n in list(range(1, 600)) + [1407, 4096]:
        for odd_only in (0, 1):
            for ghost, b0 in ((1, 0), (0, 3), (1, 3)):
                assert fold_plan(n, ghost, odd_only, b0, 1) == -1, (n, ghost, odd_only, b0)


def test_odd_only_order_of_a_whole_band():
    """The rule counts levels whatever the order of the plan (the solver reaches it with its own order only)."""
    for n in list(range(1, 300)) + [513]:
        nlev = len(plan_info(n, 0, 1)[0])
        assert fold_plan(n, 0, 1) == (nlev - 2 if nlev >= 2 and nlev % 2 == 0 else -1), n


def test_invalid_arguments():
    assert fold_plan(0) == INVALID and fold_plan(-3) == INVALID
    assert fold_plan(29, b0=-1) == INVALID
    assert fold_plan(29, ghost=2) == INVALID and fold_plan(29, ghost=-1) == INVALID
    assert fold_plan(29, on=7) == 2                               # any non-zero value is "on"
