"""Whether level 0 of the block cyclic reduction runs as ONE launch behind a plain build launch (kernels_bcr.hip:
bcr_level0_behind_build, exported as oicc_debug_bcr_level0_plan), on the host alone.

With the rule true a solve launches bcr_build_kernel and then bcri_invert_schur_kernel on level 0's pivots x (12 + 3 rtf) workgroups,
instead of bcri_build_invert_kernel (the build with level 0's inversions) and bcri_schur_kernel.  The rule is restated here from the
plan (oicc_debug_bcr_plan) and compared for every n <= 4096, rtf 1..4, the budgets of tests/test_bcr_join_plan.py, with and without
a ghost block / block offset, and the three values of option bcr_join_levels:
  - 0: nothing is joined; 2: the levels above level 0 only; 1: level 0 as well, where
  - the solve is the whole band (no ghost block, no block offset),
  - 8 <= n <= 512 (below eight blocks the parent's launches stay; above 512 the build is plain anyway and the rule of the other
    levels decides),
  - level 0's pivots x groups fit the workgroup budget.
oicc_debug_bcr_join_plan keeps its meaning (tests/test_bcr_join_plan.py, unchanged): with build_inverts < 0 it answers for the
levels above level 0 of an n <= 512 block solve under every value of the switch that is not 0.
"""
import numpy as np
import pytest

from openimucameracalibrator_amd import _lib
from test_bcr_join_plan import BUDGETS, join_plan, plan

SWITCH = (0, 1, 2)


def level0_plan(n, ghost=0, odd_only=0, b0=0, rtf=1, on=1, budget=256):
    got = int(_lib.load_bcr_plan().level0_plan(n, ghost, odd_only, b0, rtf, on, budget))
    assert got in (0, 1), (n, ghost, odd_only, b0, rtf, on, budget, got)
    return got


def rule(npiv0, n, ghost, b0, rtf, on, budget):
    """The rule, restated: npiv0 = pivots of level 0 (None: a plan without levels)."""
    return int(npiv0 is not None and on not in (0, 2) and ghost == 0 and b0 == 0 and 8 <= n <= 512 and npiv0 * (12 + 3 * rtf) <= budget)


def test_whole_band_every_block_count():
    for n in range(1, 4097):
        levels = plan(n)
        npiv0 = levels[0][4] if levels else None
        if levels:
            assert npiv0 == (n + 1) // 2          # an even count takes the odd positions, an odd one the even positions, both ends included
        for rtf in (1, 2, 3, 4):
            for budget in BUDGETS:
                for on in SWITCH:
                    assert level0_plan(n, rtf=rtf, on=on, budget=budget) == rule(npiv0, n, 0, 0, rtf, on, budget), (n, rtf, budget, on)


@pytest.mark.parametrize("ghost,b0", [(1, 0), (0, 3), (1, 3)])
def test_distributed_ranges_keep_their_launches(ghost, b0):
    for n in list(range(1, 600)) + [1407, 4096]:
        for odd_only in (0, 1):
            for rtf in (1, 4):
                for on in SWITCH:
                    assert level0_plan(n, ghost, odd_only, b0, rtf, on, 1 << 20) == 0, (n, ghost, odd_only, b0, rtf, on)


def test_named_cases():
    assert [lv[4] for lv in plan(29)] == [15, 7, 4, 2]
    assert level0_plan(29, rtf=1, budget=224) == 0 and level0_plan(29, rtf=1, budget=225) == 1      # the flagship: 15 x 15 = 225
    assert level0_plan(29, rtf=4, budget=359) == 0 and level0_plan(29, rtf=4, budget=360) == 1      # 15 x 24 = 360
    assert level0_plan(7, budget=1 << 20) == 0 and level0_plan(8, budget=1 << 20) == 1
    assert level0_plan(7) == 0 and level0_plan(8) == 1                                              # 4 x 15 = 60 <= 256
    assert level0_plan(512, budget=1 << 20) == 1 and level0_plan(513, budget=1 << 20) == 0
    assert [lv[4] for lv in plan(43)][0] == 22 and level0_plan(43, budget=256) == 0                 # 22 x 15 = 330 > 256
    assert level0_plan(17, budget=134) == 0 and level0_plan(17, budget=135) == 1                    # 9 x 15 = 135
    for n in (8, 29, 512):
        assert level0_plan(n, on=0, budget=1 << 20) == 0 and level0_plan(n, on=2, budget=1 << 20) == 0


def test_the_join_plan_keeps_its_meaning():
    """oicc_debug_bcr_join_plan with build_inverts < 0: level 0 of an n <= 512 block solve is not in its answer, whatever the switch
    says; the levels above it are joined under 1 and 2 alike."""
    for n in (8, 9, 17, 29, 43, 512):
        nlev = len(plan(n))
        for on in (1, 2):
            got = join_plan(n, rtf=1, on=on, budget=1 << 20)
            assert got == [0] + [1] * (nlev - 1), (n, on, got)
        assert join_plan(n, rtf=1, on=0, budget=1 << 20) == [0] * nlev
    assert join_plan(29, rtf=1, on=1, budget=256) == [0, 1, 1, 1] and join_plan(29, rtf=1, on=2, budget=256) == [0, 1, 1, 1]


def test_invalid_arguments():
    b = _lib.load_bcr_plan()
    assert b.level0_plan(0, 0, 0, 0, 1, 1, 256) == -1
    assert b.level0_plan(29, 0, 0, 0, 0, 1, 256) == -1 and b.level0_plan(29, 0, 0, 0, 5, 1, 256) == -1
    assert b.level0_plan(29, 0, 0, 0, 1, 1, -1) == -1 and b.level0_plan(29, 0, 0, -1, 1, 1, 256) == -1
    assert b.level0_plan(1, 0, 0, 0, 1, 1, 256) == 0                              # one block: no level at all
