"""The block cyclic reduction at block counts whose plan pivots the END blocks (kernels_bcr.hip, bcr_plan), against the
extended-precision host solve of tests/test_gpu_linear_solve_reference.py -- its run_case, dataset, check_step and bounds, unchanged.

With an odd number m of active blocks a level eliminates the even positions, both ends included.  What that adds to the kernels, and
the block counts that exercise it (asserted below from the plan itself, oicc_debug_bcr_plan, so that a change of the plan cannot
silently empty a category):
  - a pivot without a left neighbour at level 0, inverted by the fused build (odd n);
  - an odd m at an inner level only (n = 6, 10, 14, 30);
  - a top level of two pivots, whose back substitutions the last block's workgroup does (n = 3, 6, 7, 13, 29);
  - a last block that is not block 0 (every n that is no power of two);
  - in the two-level back substitution: a left-end orphan -- a lower pivot at position 0 whose right neighbour is no pivot of the
    upper level (n = 13, 29, 33) -- and an upper pivot at position 0 without a left child (n = 14, 30);
  - n = 29 (the benchmark's block count) and 30..33 around the power of two, where the old and the new depth agree only at 32.
"""
import numpy as np
import pytest

import test_gpu_linear_solve_reference as L
from test_bcr_plan import plan
from openimucameracalibrator_amd import estimator as E

pytestmark = pytest.mark.gpu

F = L.F
# duration of the tiny configuration -> blocks of 64 band columns (arrow 9, hb 50); the durations put Pb in the middle of a block
CASES = [(1.2, 3), (3.5, 6), (4.25, 7), (6.5, 10), (8.6, 13), (9.25, 14), (20.0, 29), (20.75, 30), (21.5, 31), (22.1, 32), (22.75, 33)]


def features(n):
    levels, last, _, _ = plan(n)
    f = set()
    if levels and levels[0][2] == 0:
        f.add("left_end_pivot_level0")
    if levels and levels[0][2] == 1 and any(lv[2] == 0 for lv in levels[1:]):
        f.add("odd_inner_only")
    if levels and levels[-1][2] == 0:
        f.add("two_pivot_top")
    if last != 0:
        f.add("last_is_not_block0")
    # the levels below the top one go two per launch from the bottom up: (0, 1), (2, 3), ...
    for lo in range(0, len(levels) - 2, 2):
        if levels[lo][2] == 0 and levels[lo + 1][2] == 1:
            f.add("left_orphan")
        if levels[lo][2] == 1 and levels[lo + 1][2] == 0:
            f.add("upper_pivot_without_left_child")
    if (len(levels) - 1) % 2 == 1 and len(levels) >= 2 and levels[len(levels) - 2][2] == 0:
        f.add("single_level_back_substitution_with_left_end_pivot")
    return f


def test_the_cases_cover_what_is_new():
    have = {n: features(n) for _, n in CASES}
    assert all("left_end_pivot_level0" in have[n] for n in (3, 7, 13, 29, 31, 33))
    assert all("odd_inner_only" in have[n] for n in (6, 10, 14, 30))
    assert all("two_pivot_top" in have[n] for n in (3, 6, 7, 13, 29))
    assert all("left_orphan" in have[n] for n in (13, 29, 33))
    assert all("upper_pivot_without_left_child" in have[n] for n in (14, 30))
    assert "single_level_back_substitution_with_left_end_pivot" in have[29]
    assert have[32] == set()                                               # a power of two: the order it always had
    assert plan(29)[1] == 13


@pytest.mark.parametrize("duration,n", CASES, ids=["n%d" % c[1] for c in CASES])
def test_end_pivot_block_counts(duration, n):
    """Radii 1e4 and 1e16, LDS poisoned (run_case's calibrator sets debug_poison_lds), geometry and route asserted."""
    L.run_case(L.dataset(duration), F, dict(n=n, a=9, hb=50, route="bcr_fused"), radii=(1e4, 1e16))


@pytest.mark.parametrize("duration,n", [(8.6, 13), (20.0, 29)], ids=["n13", "n29"])
def test_reused_diagonal_with_end_pivots(duration, n):
    """The rejected-step path (the fused build takes the stored diagonal) where level 0 has a pivot without a left neighbour."""
    tr = L.calibrator(L.dataset(duration)).trajectory_
    first = tr.DebugLmStep(F, 1e4)
    assert first["route"] == "bcr_fused" and first["n"] == n
    diag1 = L.check_step(first, 1e4, label="n%d first" % n)
    tr.SetOption("min_lm_diagonal", float(np.median(diag1)))
    second = tr.DebugLmStep(F, 0.5e4, reuse_diagonal=1)
    assert second["route"] == "bcr_fused" and second["n"] == n
    assert np.array_equal(second["diag"], first["diag"])
    L.check_step(second, 0.5e4, previous_diag=diag1, label="n%d reused" % n)


def test_poisoned_lds_and_stale_factor_rows():
    """debug_poison_lds, and a second solve over the workspace of the first: the rows of T that a pivot without a left (or right)
    neighbour never writes hold the other solve's values and must not be read."""
    tr = L.calibrator(L.dataset(20.0)).trajectory_
    tr.SetOption("debug_poison_lds", 1)
    for radius in (1e16, 1e4, 1e16):
        out = tr.DebugLmStep(F, radius)
        assert out["route"] == "bcr_fused" and out["n"] == 29
        L.check_step(out, radius, label="n29 repeated")


def test_three_blocks_solve_is_reproducible_bit_by_bit():
    """Three blocks: the two end pivots both update the middle block and the corner.  Two atomic additions would land in either
    order; the left pivot's updates go through a side buffer instead (BcrArgs::side) and the last block's workgroup adds them
    in a fixed order, so repeated solves of one system agree in every bit -- as they did when each level of it had one pivot
    (the device-side and the host-driven LM loop take bit-identical steps on such problems)."""
    tr = L.calibrator(L.dataset(1.2)).trajectory_
    for flags in (F, F | E.IMU_BIASES):
        for radius in (1e4, 1e9):
            outs = [tr.DebugLmStep(flags, radius) for _ in range(5)]
            assert outs[0]["n"] == 3 and outs[0]["route"] == "bcr_fused"
            assert all(np.array_equal(o["step_s"], outs[0]["step_s"]) for o in outs[1:]), (flags, radius)
