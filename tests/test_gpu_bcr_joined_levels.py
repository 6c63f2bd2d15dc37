"""Levels of the block cyclic reduction that run as ONE launch (kernels_bcr.hip: bcri_invert_schur_kernel -- every workgroup of a pivot
inverts it itself and goes on with its Schur group, Z in LDS), against the extended-precision host solve of
tests/test_gpu_linear_solve_reference.py: its run_case, dataset, check_step and its BACKWARD / FORWARD_C bounds, unchanged.

Every case runs with option bcr_join_levels 0 (the two launches per level) and 1, at radii 1e4 and 1e16 (1e4 only with board
points, as there), with the LDS poisoned (run_case's calibrator), and asserts the geometry, the route and HOW MANY levels of the last
solve ran joined (estimator.BcrJoinInfo), against the host rule (oicc_debug_bcr_join_plan) and against the number written here.
The shapes are the smallest at which a joined level differs:
  n = 4     the first plan with a level above the build's: one pivot with a single neighbour (its left one);
  n = 5     the same with a left-end pivot at level 0;
  n = 7     the joined top level has two pivots, the left one writes through the side buffer (BcrArgs::side);
  n = 8, 9  three levels, the last launch of the solve retracts; n = 17: four levels;
  a = 15, 16, 33, 63 at n = 4 / 5: one to four 16-row border tiles (12 + 3 rtf groups per pivot) at a joined level;
  n = 17 with budgets 59 / 60 (level 1: 4 pivots x 15 groups = 60) and 14 / 15 (the top level's one pivot): both sides of the edge.
"""
import numpy as np
import pytest

import test_gpu_linear_solve_reference as L
import lm_step_reference as R
from test_bcr_join_plan import join_plan, plan
from openimucameracalibrator_amd import synthetic, estimator as E

pytestmark = pytest.mark.gpu

F = L.F
JOIN = [0, 1]


def expected_joined(n, a, budget, on=1):
    return sum(join_plan(n, rtf=(a + 1 + 15) // 16, on=on, budget=budget))


def run_joined(ds, flags, expect, join, joined, radii=(1e4, 1e16), **opts):
    """run_case with the option set; `joined`: levels of the last solve that must have run as one launch when the option is on."""
    tr = L.run_case(ds, flags, expect, radii=radii, bcr_join_levels=join, **opts)
    info = tr.BcrJoinInfo()
    assert info["on"] == bool(join)
    assert info["budget"] == opts.get("bcr_join_max_workgroups", info["budget"]) and info["budget"] >= 1   # (default: the compute units)
    want = joined if join else 0
    assert expected_joined(expect["n"], expect["a"], info["budget"], join) == want, (expect, info)     # the host rule says so ...
    assert info["last"] == want and info["total"] == want * len(radii), (expect, info)                 # ... and the solves did it
    return tr


# ---- block counts ---------------------------------------------------------------------------------------------------------------
BLOCKS = [   # (duration, Pb, n, joined levels under the default budget: every level above the build's)
    (2.5, 252, 4, 1), (3.0, 297, 5, 1), (4.25, 405, 7, 1), (5.0, 477, 8, 2), (6.0, 567, 9, 2), (11.5, 1062, 17, 3),
]


def test_the_plans_of_the_cases():
    """What the cases are chosen for, from the plan itself."""
    piv = {n: [lv[4] for lv in plan(n)] for _, _, n, _ in BLOCKS}
    par = {n: [lv[2] for lv in plan(n)] for _, _, n, _ in BLOCKS}
    assert piv[4] == [2, 1] and piv[5] == [3, 1] and piv[7] == [4, 2] and piv[8] == [4, 2, 1] and piv[9] == [5, 2, 1] and piv[17] == [9, 4, 2, 1]
    assert par[7][-1] == 0                                  # a top level of two pivots: the side buffer
    assert par[4][-1] == 1 and par[5][-1] == 1              # one pivot, right of the last block: a left neighbour only


@pytest.mark.parametrize("join", JOIN, ids=["two_launches", "joined"])
@pytest.mark.parametrize("duration,Pb,n,joined", BLOCKS, ids=["n%d" % c[2] for c in BLOCKS])
def test_block_counts(duration, Pb, n, joined, join):
    run_joined(L.dataset(duration), F, dict(Pb=Pb, n=n, a=9, hb=50, route="bcr_fused"), join, joined)


# ---- border tiles at a joined level ---------------------------------------------------------------------------------------------
ARROW = {c[0]: c for c in L.ARROWS}
TILES = [(15, 2.5, 252, 4), (16, 3.0, 297, 5), (33, 2.5, 252, 4), (63, 3.0, 297, 5)]    # (a, duration, Pb, n): rtf 1, 2, 3, 4


@pytest.mark.parametrize("join", JOIN, ids=["two_launches", "joined"])
@pytest.mark.parametrize("a,duration,Pb,n", TILES, ids=["a%d_n%d" % (c[0], c[3]) for c in TILES])
def test_border_tiles_at_a_joined_level(a, duration, Pb, n, join):
    _, flags, kw = ARROW[a]
    assert (a + 1 + 15) // 16 == {15: 1, 16: 2, 33: 3, 63: 4}[a]
    run_joined(L.dataset(duration, **kw), flags, dict(Pb=Pb, n=n, a=a, hb=50, route="bcr_fused"), join, 1,
               radii=(1e4,) if flags & E.POINTS else (1e4, 1e16))


# ---- the budget edge ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("budget,joined", [(14, 0), (15, 1), (59, 2), (60, 3)], ids=["b14", "b15", "b59", "b60"])
def test_budget_edge(budget, joined):
    """n = 17: 9, 4, 2, 1 pivots, 15 groups each.  59: level 1 keeps its two launches, the levels above it join; 60 = 4 x 15 joins it.
    14 / 15: the same edge at the top level's single pivot."""
    run_joined(L.dataset(11.5), F, dict(Pb=1062, n=17, a=9, route="bcr_fused"), 1, joined, bcr_join_max_workgroups=budget)


# ---- failure --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("join", JOIN, ids=["two_launches", "joined"])
@pytest.mark.parametrize("duration,n,joined", [(3.0, 5, 1), (6.0, 9, 2)], ids=["n5", "n9"])
def test_indefinite_system_is_reported(duration, n, joined, join):
    """As test_gpu_linear_solve_reference.py::test_indefinite_system_is_reported: every pivot negative, the flag must be raised --
    by the one workgroup per pivot of a joined level that reports."""
    tr = L.calibrator(L.dataset(duration), min_lm_diagonal=-1.0, max_lm_diagonal=-1.0, bcr_join_levels=join).trajectory_
    out = tr.DebugLmStep(F, 1e-3)
    assert out["route"] == "bcr_fused" and out["n"] == n
    _, diag, S = R.from_step(out, 1e-3, -1.0, -1.0)
    assert np.all(S.Mb[:, 0] < 0) and np.all(np.diag(S.Mc) < 0)
    assert tr.BcrJoinInfo()["last"] == (joined if join else 0)
    assert out["chol_failed"]


# ---- a whole calibration ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reference_options", [False, True], ids=["plain_lm", "reference_options"])
def test_c2_calibration_is_the_same_joined_and_not(reference_options):
    """Optimize(50, F) on C2 with the option 0 and 1: the same iteration counts and termination, the final cost to 1e-9 relative (the
    atomics of a level land in any order under both)."""
    ds = synthetic.make_config("C2")
    runs = {}
    for join in JOIN:
        tr = E.ImuCameraCalibrator().BatchInitSpline(ds).trajectory_
        if reference_options:
            tr.UseReferenceSolverOptions()
        tr.SetOption("bcr_join_levels", join)
        s = tr.Optimize(50, F)
        runs[join] = (s, tr.GetIterations(), tr.BcrJoinInfo())
        print("join %d: iterations %d (%d + %d) final cost %.12e joined levels %d" % (join, s["num_iterations"], s["num_successful_steps"],
                                                                                     s["num_unsuccessful_steps"], s["final_cost"], runs[join][2]["total"]))
    (s0, it0, j0), (s1, it1, j1) = runs[0], runs[1]
    assert j0["total"] == 0
    if not reference_options:
        assert j1["total"] >= 3 * s1["num_iterations"] and j1["last"] == 3       # 29 blocks: the levels of 7, 4 and 2 pivots
    for k in ("termination", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "message"):
        assert s1[k] == s0[k], (k, s1, s0)
    assert abs(s1["final_cost"] - s0["final_cost"]) <= 1e-9 * abs(s0["final_cost"]), (s1["final_cost"], s0["final_cost"])
    assert len(it1) == len(it0)
    for a, b in zip(it1, it0):
        assert a["iteration"] == b["iteration"] and a["step_is_successful"] == b["step_is_successful"], (a, b)
