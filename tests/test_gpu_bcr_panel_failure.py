"""The failure reporting of the block cyclic reduction's 64 x 64 inversions, with ONE test per 16-column panel (kernels_bcr.hip,
bcri_invert_body: !(pivot of the panel's last column > 0)).

A pivot that is not positive makes rsq NaN or inf, so the factor column is NaN in every lane and with it every later column of the
panel, the last pivot included: the one test must see a bad pivot at ANY column of the panel.  A negative pivot is planted (option
debug_plant_pivot: the band diagonal of one column is -1 for one solve) at column 5 and 10 of the first panel -- seen through the NaN
they leave in column 15 -- , at the last column of the first panel, and at the first and last column of the last panel, behind which
nothing follows, of
  - the last block of a three-block band (block 1: bcri_invert_kernel<true, false>),
  - a pivot of a level that runs as one launch (n = 8, level 1, block 2: bcri_invert_schur_kernel, whose first group reports),
  - a pivot of a level with an inversion launch of its own (the same with bcr_join_levels = 0: bcri_invert_kernel<false, false>),
  - the last block of the flagship's plan (n = 29, block 13: bcri_last_backward_kernel, whose workgroup 0 reports).
chol_failed must be raised every time, and the same problem must solve once the pivot is taken out again (against the
extended-precision solve of tests/test_gpu_linear_solve_reference.py: its check_step and bounds, unchanged).
"""
import numpy as np
import pytest

import test_gpu_linear_solve_reference as L
from test_bcr_plan import plan

pytestmark = pytest.mark.gpu

RADIUS = 1e4
CASES = [   # (id, duration, n, block, options)
    ("n3_last_block", 1.2, 3, 1, {}),
    ("n8_joined_level", 5.0, 8, 2, {}),
    ("n8_own_launch", 5.0, 8, 2, dict(bcr_join_levels=0)),
    ("n29_folded_last_block", 20.0, 29, 13, {}),
]
COLUMNS = [5, 10, 15, 48, 63]


def test_the_planted_blocks_are_what_the_cases_say():
    assert plan(3)[1] == 1 and plan(29)[1] == 13                               # the last blocks
    levels = plan(8)[0]
    o, s, p = levels[1][0], levels[1][1], levels[1][2]                          # level 1 of eight blocks: origin, stride, parity
    assert o + s * p == 2                                                      # its first pivot is block 2


@pytest.mark.parametrize("column", COLUMNS, ids=["c%d" % c for c in COLUMNS])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_a_planted_pivot_is_reported(case, column):
    _, duration, n, block, opts = case
    col = 64 * block + column
    tr = L.calibrator(L.dataset(duration), debug_plant_pivot=col, **opts).trajectory_
    out = tr.DebugLmStep(L.F, RADIUS)
    assert out["route"] == "bcr_fused" and out["n"] == n and col < out["Pb"]
    assert out["band"][col, 0] == -1.0 and np.all(np.delete(out["band"][:, 0], col) > 0)     # one negative diagonal entry, where it was planted
    assert out["chol_failed"]
    if column == COLUMNS[0]:                                                   # (once per case: without the pivot the same problem solves)
        tr.SetOption("debug_plant_pivot", -1)
        again = tr.DebugLmStep(L.F, RADIUS)
        assert np.all(again["band"][:, 0] > 0)
        L.check_step(again, RADIUS, label="%s, pivot taken out" % case[0])
