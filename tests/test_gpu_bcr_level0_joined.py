"""Level 0 of the block cyclic reduction as ONE launch behind a plain build launch (kernels_bcr.hip: bcr_level0_behind_build ->
bcr_build_kernel, then bcri_invert_schur_kernel on level 0), against the extended-precision host solve of
tests/test_gpu_linear_solve_reference.py: its run_case, dataset, check_step and its BACKWARD / FORWARD_C bounds, unchanged.

Every case runs with option bcr_join_levels 1 (level 0 joins where the rule says so) and 2 (the levels above level 0 only: the build
launch inverts level 0's pivots and a Schur launch follows), at radii 1e4 and 1e16 (1e4 only with board points, as there), with the
LDS poisoned (run_case's calibrator), and asserts the geometry, the route, WHETHER level 0 of the last solve ran joined
(estimator.BcrJoinInfo: level0_last / level0_total) against the host rule (oicc_debug_bcr_level0_plan) and against the number written
here, and that the counters of the levels above level 0 (last / total) are what they are without it.  The shapes are the smallest
at which a joined level 0 differs:
  n = 8     the first block count of the rule: 4, 2, 1 pivots;
  n = 9     5, 2, 1 pivots: level 0 takes both end blocks, which have one neighbour each;
  n = 17    four levels; n = 29: the flagship's layout (15 pivots x 15 groups = 225 workgroups);
  a = 15, 16, 33, 63 at n = 8: one to four 16-row border tiles (12 + 3 rtf groups per pivot);
  n = 17 with budgets 134 / 135 (level 0: 9 pivots x 15 groups = 135): both sides of the edge.
Failure: behind the plain build, whose thread 0 resets chol_failed, the reporting workgroup of a joined level-0 pivot raises the flag
itself -- the all-negative diagonal at n = 9 and a planted negative pivot in a level-0 pivot block and in a block level 0 updates.
"""
import numpy as np
import pytest

import test_gpu_linear_solve_reference as L
import lm_step_reference as R
from test_bcr_join_plan import join_plan, plan
from test_bcr_level0_plan import level0_plan
from openimucameracalibrator_amd import synthetic, estimator as E

pytestmark = pytest.mark.gpu

F = L.F
JOIN = [1, 2]
IDS = ["level0_joined", "upper_levels_only"]


def run_level0(ds, flags, expect, join, level0, above, radii=(1e4, 1e16), **opts):
    """run_case with the switch set; `level0`: whether level 0 must join under switch value 1; `above`: joined levels above it."""
    tr = L.run_case(ds, flags, expect, radii=radii, bcr_join_levels=join, **opts)
    info = tr.BcrJoinInfo()
    assert info["on"] is True
    assert info["budget"] == opts.get("bcr_join_max_workgroups", info["budget"]) and info["budget"] >= 1   # (default: the compute units)
    rtf = (expect["a"] + 1 + 15) // 16
    want0 = level0 if join == 1 else 0
    assert level0_plan(expect["n"], rtf=rtf, on=join, budget=info["budget"]) == want0, (expect, info)       # the host rule says so ...
    assert info["level0_last"] == want0 and info["level0_total"] == want0 * len(radii), (expect, info)      # ... and the solves did it
    assert sum(join_plan(expect["n"], rtf=rtf, on=join, budget=info["budget"])) == above, (expect, info)
    assert info["last"] == above and info["total"] == above * len(radii), (expect, info)                    # the levels above: unchanged
    return tr


# ---- block counts ---------------------------------------------------------------------------------------------------------------
BLOCKS = [(5.0, 477, 8, 2), (6.0, 567, 9, 2), (11.5, 1062, 17, 3), (20.0, None, 29, 3)]   # (duration, Pb, n, joined levels above level 0)


def test_the_plans_of_the_cases():
    piv = {n: [lv[4] for lv in plan(n)] for _, _, n, _ in BLOCKS}
    par = {n: plan(n)[0][2] for _, _, n, _ in BLOCKS}
    assert piv[8] == [4, 2, 1] and piv[9] == [5, 2, 1] and piv[17] == [9, 4, 2, 1] and piv[29] == [15, 7, 4, 2]
    assert par[8] == 1 and par[9] == 0 and par[17] == 0 and par[29] == 0      # an odd count: both end blocks are pivots of level 0
    assert level0_plan(7, budget=1 << 20) == 0                                # (below eight blocks the parent's launches stay)


@pytest.mark.parametrize("join", JOIN, ids=IDS)
@pytest.mark.parametrize("duration,Pb,n,above", BLOCKS, ids=["n%d" % c[2] for c in BLOCKS])
def test_block_counts(duration, Pb, n, above, join):
    expect = dict(n=n, a=9, hb=50, route="bcr_fused")
    if Pb is not None:
        expect["Pb"] = Pb
    run_level0(L.dataset(duration), F, expect, join, 1, above)


# ---- border tiles ---------------------------------------------------------------------------------------------------------------
ARROW = {c[0]: c for c in L.ARROWS}


@pytest.mark.parametrize("join", JOIN, ids=IDS)
@pytest.mark.parametrize("a", [15, 16, 33, 63], ids=["a15", "a16", "a33", "a63"])
def test_border_tiles_at_level0(a, join):
    _, flags, kw = ARROW[a]
    assert (a + 1 + 15) // 16 == {15: 1, 16: 2, 33: 3, 63: 4}[a]
    run_level0(L.dataset(5.0, **kw), flags, dict(Pb=477, n=8, a=a, hb=50, route="bcr_fused"), join, 1, 2,
               radii=(1e4,) if flags & E.POINTS else (1e4, 1e16))


# ---- the budget edge ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("budget,level0", [(134, 0), (135, 1)], ids=["b134", "b135"])
def test_budget_edge(budget, level0):
    """n = 17: 9, 4, 2, 1 pivots, 15 groups each.  134: the build launch keeps level 0's inversions; 135 = 9 x 15 joins level 0.  The
    three levels above fit either budget."""
    run_level0(L.dataset(11.5), F, dict(Pb=1062, n=17, a=9, route="bcr_fused"), 1, level0, 3, bcr_join_max_workgroups=budget)


# ---- failure --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("join", JOIN, ids=IDS)
def test_indefinite_system_is_reported(join):
    """As test_gpu_bcr_joined_levels.py::test_indefinite_system_is_reported at n = 9: every pivot negative, the flag must be raised."""
    tr = L.calibrator(L.dataset(6.0), min_lm_diagonal=-1.0, max_lm_diagonal=-1.0, bcr_join_levels=join).trajectory_
    out = tr.DebugLmStep(F, 1e-3)
    assert out["route"] == "bcr_fused" and out["n"] == 9
    _, diag, S = R.from_step(out, 1e-3, -1.0, -1.0)
    assert np.all(S.Mb[:, 0] < 0) and np.all(np.diag(S.Mc) < 0)
    info = tr.BcrJoinInfo()
    assert info["level0_last"] == (1 if join == 1 else 0) and info["last"] == 2
    assert out["chol_failed"]


PLANTED = [("level0_pivot", 1), ("updated_block", 2)]   # (id, block): n = 8, level 0's pivots are the odd blocks; block 2 is level 1's first pivot
COLUMNS = [5, 15, 48, 63]


@pytest.mark.parametrize("column", COLUMNS, ids=["c%d" % c for c in COLUMNS])
@pytest.mark.parametrize("name,block", PLANTED, ids=[c[0] for c in PLANTED])
def test_a_planted_pivot_is_reported(name, block, column):
    """As tests/test_gpu_bcr_panel_failure.py, with level 0 joined: a negative band diagonal entry in a block level 0 inverts (the
    joined kernel's reporting workgroup raises the flag; the plain build does not invert) and in a block its Schur updates land on."""
    assert plan(8)[0][2] == 1 and block % 2 == (1 if name == "level0_pivot" else 0)
    col = 64 * block + column
    tr = L.calibrator(L.dataset(5.0), debug_plant_pivot=col).trajectory_
    out = tr.DebugLmStep(F, 1e4)
    assert out["route"] == "bcr_fused" and out["n"] == 8 and col < out["Pb"]
    assert out["band"][col, 0] == -1.0 and np.all(np.delete(out["band"][:, 0], col) > 0)
    assert tr.BcrJoinInfo()["level0_last"] == 1
    assert out["chol_failed"]
    if column == COLUMNS[0]:                                                   # (once per block: without the pivot the same problem solves)
        tr.SetOption("debug_plant_pivot", -1)
        again = tr.DebugLmStep(F, 1e4)
        assert np.all(again["band"][:, 0] > 0)
        L.check_step(again, 1e4, label="%s, pivot taken out" % name)


# ---- a whole calibration ----------------------------------------------------------------------------------------------------------
SETTINGS = [("plain_lm_device_loop", False, 1), ("plain_lm_host_loop", False, 0), ("reference_options", True, None)]


@pytest.mark.parametrize("name,reference_options,device_lm", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_c2_calibration_is_the_same_with_level0_joined_and_not(name, reference_options, device_lm):
    """Optimize(50, F) on C2 with the switch at 1 and 2: the same iteration counts, termination and per-iteration success flags, the
    final cost to 1e-9 relative (the bound of test_gpu_bcr_joined_levels.py: the atomics of a level land in any order under both).
    Every solve of the 29 blocks joins the three levels above level 0, so the solves are total / 3: level 0 must have joined in
    every one of them under 1 and in none under 2."""
    ds = synthetic.make_config("C2")
    runs = {}
    for join in JOIN:
        tr = E.ImuCameraCalibrator().BatchInitSpline(ds).trajectory_
        if reference_options:
            tr.UseReferenceSolverOptions()
        if device_lm is not None:
            tr.SetOption("device_lm", device_lm)
        tr.SetOption("bcr_join_levels", join)
        s = tr.Optimize(50, F)
        runs[join] = (s, tr.GetIterations(), tr.BcrJoinInfo())
        print("join %d: iterations %d (%d + %d) final cost %.12e joined levels %d level 0 joined %d" % (
            join, s["num_iterations"], s["num_successful_steps"], s["num_unsuccessful_steps"], s["final_cost"], runs[join][2]["total"], runs[join][2]["level0_total"]))
    (s1, it1, j1), (s2, it2, j2) = runs[1], runs[2]
    for j in (j1, j2):
        assert j["last"] == 3 and j["total"] % 3 == 0 and j["total"] >= 3, j
        if not reference_options:
            assert j["total"] >= 3 * s1["num_iterations"], j
    assert j1["level0_last"] == 1 and j1["level0_total"] == j1["total"] // 3, j1
    assert j2["level0_last"] == 0 and j2["level0_total"] == 0, j2
    for k in ("termination", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "message"):
        assert s1[k] == s2[k], (k, s1, s2)
    assert abs(s1["final_cost"] - s2["final_cost"]) <= 1e-9 * abs(s2["final_cost"]), (s1["final_cost"], s2["final_cost"])
    assert len(it1) == len(it2)
    for a, b in zip(it1, it2):
        assert a["iteration"] == b["iteration"] and a["step_is_successful"] == b["step_is_successful"], (a, b)
