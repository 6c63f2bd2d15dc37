"""Which levels of the block cyclic reduction run as ONE launch (kernels_bcr.hip: bcr_level_joined, exported as
oicc_debug_bcr_join_plan), on the host alone.

A joined level is one bcri_invert_schur_kernel launch of pivots x (12 + 3 rtf) workgroups instead of an inversion launch and a Schur
launch.  The rule is restated here from the plan (oicc_debug_bcr_plan) and compared level by level for every n <= 4096, rtf 1..4,
several budgets, with and without a ghost block / block offset:
  - level 0 is never joined when the build launch inverts it;
  - no level of a range with a ghost block or a block offset is joined (the distributed reduction keeps its launches; its carried
    couplings only exist there);
  - the workgroups of a joined level are at most the budget, and a level above the build's that fits the budget IS joined;
  - with the option off, nothing is joined.
"""
import ctypes

import numpy as np
import pytest

from openimucameracalibrator_amd import _abi, _lib

CAP = 40
BUDGETS = (0, 1, 14, 15, 30, 48, 105, 256, 304, 1 << 20)


def plan(n, ghost=0, odd_only=0):
    b = _lib.load_bcr_plan()
    levels = np.zeros((CAP, 6), dtype=np.int64)
    info = np.zeros(3, dtype=np.int64)
    nlev = b.plan(n, ghost, odd_only, levels.ctypes.data_as(_abi.c_i64p), CAP, info.ctypes.data_as(_abi.c_i64p))
    assert nlev >= 0, (n, nlev)
    return [tuple(int(v) for v in levels[l]) for l in range(nlev)]


def join_plan(n, ghost=0, odd_only=0, b0=0, rtf=1, on=1, budget=256, build_inverts=-1):
    b = _lib.load_bcr_plan()
    joined = np.full(CAP, -1, dtype=np.int32)
    nlev = b.join_plan(n, ghost, odd_only, b0, rtf, on, budget, build_inverts, joined.ctypes.data_as(_abi.c_i32p), CAP)
    assert nlev >= 0, (n, nlev)
    assert np.all(joined[nlev:] == -1)
    return [int(v) for v in joined[:nlev]]


def build_inverts_level0(n):
    return 2 <= n <= 512          # (kernels_bcr.hip: bcr_fused_build without phase clocks)


def test_whole_band_every_block_count():
    for n in range(1, 4097):
        levels = plan(n)
        npivs = [lv[4] for lv in levels]
        for rtf in (1, 2, 3, 4):
            groups = 12 + 3 * rtf
            for budget in BUDGETS:
                got = join_plan(n, rtf=rtf, budget=budget)
                assert len(got) == len(levels)
                for l, j in enumerate(got):
                    in_build = l == 0 and build_inverts_level0(n)
                    assert j == (0 if in_build else int(npivs[l] * groups <= budget)), (n, rtf, budget, l)
                    if j:
                        assert npivs[l] * groups <= budget and not in_build
        assert join_plan(n, rtf=1, on=0, budget=1 << 20) == [0] * len(levels)      # the option off: the parent's launches
        assert join_plan(n, rtf=4, on=0, budget=256) == [0] * len(levels)


def test_build_launch_argument():
    """build_inverts 1 / 0 overrides what the block count says (level 0 of a 513-block solve has a launch of its own)."""
    for n in (2, 3, 29, 512, 513, 1407):
        nlev = len(plan(n))
        assert join_plan(n, budget=1 << 20, build_inverts=1) == [0] + [1] * (nlev - 1)
        assert join_plan(n, budget=1 << 20, build_inverts=0) == [1] * nlev
        assert join_plan(n, budget=1 << 20) == ([0] if build_inverts_level0(n) else [1]) + [1] * (nlev - 1)


def test_the_flagship_plan():
    """29 blocks, one 16-row border tile, 256 compute units: 15 + 7, 4, 2 pivots -> the three levels above the build's join."""
    assert [lv[4] for lv in plan(29)] == [15, 7, 4, 2]
    assert join_plan(29, rtf=1, budget=256) == [0, 1, 1, 1]
    assert join_plan(29, rtf=1, budget=104) == [0, 0, 1, 1] and join_plan(29, rtf=1, budget=105) == [0, 1, 1, 1]   # 7 x 15 = 105
    assert join_plan(29, rtf=4, budget=167) == [0, 0, 1, 1] and join_plan(29, rtf=4, budget=168) == [0, 1, 1, 1]   # 7 x 24 = 168
    assert join_plan(17, rtf=1, budget=59) == [0, 0, 1, 1] and join_plan(17, rtf=1, budget=60) == [0, 1, 1, 1]     # 9, 4, 2, 1 pivots: 4 x 15 = 60


@pytest.mark.parametrize("ghost,b0", [(1, 0), (0, 3), (1, 3)])
def test_distributed_ranges_keep_their_launches(ghost, b0):
    for n in list(range(1, 600)) + [1407, 4096]:
        for odd_only in (0, 1):
            levels = plan(n, ghost, odd_only)
            for rtf in (1, 4):
                for build_inverts in (-1, 0):
                    assert join_plan(n, ghost, odd_only, b0, rtf, 1, 1 << 20, build_inverts) == [0] * len(levels), (n, ghost, b0)


def test_odd_only_order_of_a_whole_band():
    """The top system of the distributed reduction is a whole band in the odd-positions order: the rule is the same there."""
    for n in list(range(1, 300)) + [513]:
        levels = plan(n, 0, 1)
        got = join_plan(n, 0, 1, 0, 2, 1, 64, 0)
        assert got == [int(lv[4] * 18 <= 64) for lv in levels], n


def test_invalid_arguments():
    b = _lib.load_bcr_plan()
    joined = np.zeros(CAP, dtype=np.int32); jp = joined.ctypes.data_as(_abi.c_i32p)
    assert b.join_plan(0, 0, 0, 0, 1, 1, 256, -1, jp, CAP) == -1
    assert b.join_plan(29, 0, 0, 0, 0, 1, 256, -1, jp, CAP) == -1 and b.join_plan(29, 0, 0, 0, 5, 1, 256, -1, jp, CAP) == -1
    assert b.join_plan(29, 0, 0, 0, 1, 1, -1, -1, jp, CAP) == -1 and b.join_plan(29, 0, 0, -1, 1, 1, 256, -1, jp, CAP) == -1
    assert b.join_plan(29, 0, 0, 0, 1, 1, 256, -1, jp, 3) == -1                   # four levels do not fit three entries
    assert b.join_plan(29, 0, 0, 0, 1, 1, 256, -1, ctypes.cast(None, _abi.c_i32p), CAP) == -1
    assert b.join_plan(1, 0, 0, 0, 1, 1, 256, -1, jp, CAP) == 0
