"""The back substitution of the level below the top one inside the last block's launch (kernels_bcr.hip: bcri_last_backward_kernel --
one workgroup per pivot of level nlev - 2, each repeating the last block's work and taking its neighbours' solution from LDS), against
the extended-precision host solve of tests/test_gpu_linear_solve_reference.py: its run_case, dataset, check_step and its BACKWARD /
FORWARD_C bounds, unchanged.

Every case runs with option bcr_fold_back 0 (bcri_invert_kernel<true, false>, then bcri_backward_kernel on that level) and 1, at radii
1e4 and 1e16 (1e4 only with board points, as there), with the LDS poisoned (run_case's calibrator), and asserts the geometry, the route
and WHETHER the last solve folded (estimator.BcrFoldInfo) against the host rule (oicc_debug_bcr_fold_plan).  The shapes are the
smallest at which the folded level differs (tests/test_bcr_fold_plan.py states the plans):
  n = 4     two levels, the folded level is level 0: pivots 1 and 3, last = 0, top_r = 2; pivot 3 has a left neighbour only and is the
            partial last block;
  n = 5     pivots 0, 2, 4, last = 1: pivot 0 has a right neighbour only, and that neighbour is the last block;
  n = 7     four pivots; the top level has two (top_l, the side buffer);
  n = 16    four levels, last = 0, the folded level 2 is followed by the retracting pair; n = 17: the same with nine pivots at level 0;
  n = 29    the flagship's plan (pivots 15 / 7 / 4 / 2);
  n = 8, 9  three levels: nothing folds;
  a = 15, 16, 33, 63 at n = 4 / 5: one to four 16-row border tiles, rows 128..191 of T in the shared back-substitution body.
With the option on and off the step agrees within the sum of the two forward bounds (the atomics of the forward levels land in any
order, so bits are not compared across solves).
"""
import numpy as np
import pytest

import test_gpu_linear_solve_reference as L
import test_gpu_fused_retract as FR
import lm_step_reference as R
from test_bcr_fold_plan import fold_plan, plan_info
from openimucameracalibrator_amd import synthetic, estimator as E

pytestmark = pytest.mark.gpu

F = L.F
FOLD = [0, 1]
FOLD_IDS = ["own_launch", "folded"]


def run_folded(ds, flags, expect, fold, radii=(1e4, 1e16), **opts):
    """run_case with the option set; the fold count of the solves against the host rule."""
    tr = L.run_case(ds, flags, expect, radii=radii, bcr_fold_back=fold, **opts)
    info = tr.BcrFoldInfo()
    want = int(fold_plan(expect["n"], on=fold) >= 0)
    assert info["on"] == bool(fold)
    assert info["last"] == want and info["total"] == want * len(radii), (expect, info)
    if not fold:
        assert info["last"] == 0
    return tr


# ---- block counts ---------------------------------------------------------------------------------------------------------------
BLOCKS = [   # (duration, Pb, n, folded level with the option on)
    (2.5, 252, 4, 0), (3.0, 297, 5, 0), (4.25, 405, 7, 0), (5.0, 477, 8, -1), (6.0, 567, 9, -1), (11.0, 1017, 16, 2), (11.5, 1062, 17, 2),
    (20.0, 1827, 29, 2),
]


def test_the_plans_of_the_cases():
    for _, Pb, n, level in BLOCKS:
        assert (Pb + 63) // 64 == n
        assert fold_plan(n) == level and fold_plan(n, on=0) == -1
    piv = {n: [lv[4] for lv in plan_info(n)[0]] for _, _, n, _ in BLOCKS}
    assert piv[4] == [2, 1] and piv[5] == [3, 1] and piv[7] == [4, 2] and piv[16] == [8, 4, 2, 1] and piv[17] == [9, 4, 2, 1] and piv[29] == [15, 7, 4, 2]
    assert len(piv[8]) == 3 and len(piv[9]) == 3
    assert 252 % 64 != 0                                        # n = 4: pivot 3 is a partial block


@pytest.mark.parametrize("fold", FOLD, ids=FOLD_IDS)
@pytest.mark.parametrize("duration,Pb,n,level", BLOCKS, ids=["n%d" % c[2] for c in BLOCKS])
def test_block_counts(duration, Pb, n, level, fold):
    run_folded(L.dataset(duration), F, dict(Pb=Pb, n=n, a=9, hb=50, route="bcr_fused"), fold)


# ---- border tiles in the shared back-substitution body --------------------------------------------------------------------------
ARROW = {c[0]: c for c in L.ARROWS}
TILES = [(15, 2.5, 252, 4), (16, 3.0, 297, 5), (33, 2.5, 252, 4), (63, 3.0, 297, 5)]    # (a, duration, Pb, n): rtf 1, 2, 3, 4


@pytest.mark.parametrize("fold", FOLD, ids=FOLD_IDS)
@pytest.mark.parametrize("a,duration,Pb,n", TILES, ids=["a%d_n%d" % (c[0], c[3]) for c in TILES])
def test_border_tiles(a, duration, Pb, n, fold):
    _, flags, kw = ARROW[a]
    run_folded(L.dataset(duration, **kw), flags, dict(Pb=Pb, n=n, a=a, hb=50, route="bcr_fused"), fold,
               radii=(1e4,) if flags & E.POINTS else (1e4, 1e16))


# ---- the option both ways ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("duration,Pb,n", [(2.5, 252, 4), (4.25, 405, 7), (11.5, 1062, 17), (20.0, 1827, 29)], ids=["n4", "n7", "n17", "n29"])
def test_the_step_is_the_same_folded_and_not(duration, Pb, n):
    """Both steps lie within FORWARD_C kappa_1 eps of the extended-precision solution (check_step), so within twice that of each other."""
    steps = {}
    for fold in FOLD:
        tr = L.calibrator(L.dataset(duration), bcr_fold_back=fold).trajectory_
        out = tr.DebugLmStep(F, 1e4)
        assert out["route"] == "bcr_fused" and out["n"] == n and out["Pb"] == Pb
        L.check_step(out, 1e4, label="n%d fold %d" % (n, fold))
        assert tr.BcrFoldInfo()["last"] == fold
        steps[fold] = out
    _, _, S = R.from_step(steps[0], 1e4, L.MIN_DIAG, L.MAX_DIAG)
    xs = S.solve(); kappa = S.cond1()
    diff = np.abs(steps[1]["step_s"] - steps[0]["step_s"]).max() / np.abs(xs).max()
    print("n=%d: |step folded - step not| / |step| = %.3e (bound %.3e)" % (n, diff, 2 * L.FORWARD_C["bcr_fused"] * kappa * L.EPS))
    assert diff <= 2 * L.FORWARD_C["bcr_fused"] * kappa * L.EPS


# ---- failure --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", FOLD, ids=FOLD_IDS)
@pytest.mark.parametrize("duration,n", [(3.0, 5), (11.5, 17)], ids=["n5", "n17"])
def test_indefinite_system_is_reported(duration, n, fold):
    """As test_gpu_linear_solve_reference.py::test_indefinite_system_is_reported: every pivot negative, the flag must be raised --
    by workgroup 0 of the folded launch, the only one that reports."""
    tr = L.calibrator(L.dataset(duration), min_lm_diagonal=-1.0, max_lm_diagonal=-1.0, bcr_fold_back=fold).trajectory_
    out = tr.DebugLmStep(F, 1e-3)
    assert out["route"] == "bcr_fused" and out["n"] == n
    _, diag, S = R.from_step(out, 1e-3, -1.0, -1.0)
    assert np.all(S.Mb[:, 0] < 0) and np.all(np.diag(S.Mc) < 0)
    assert tr.BcrFoldInfo()["last"] == fold
    assert out["chol_failed"]


# ---- other options ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [0, 1], ids=["lm_retract_kernel", "fused_retract"])
def test_the_retracting_pair_follows_the_folded_level(fused):
    """n = 17: the folded level 2 is followed by the two-level launch on the levels (1, 0), which retracts when asked to: the candidate
    is the stand-alone kernel's bit for bit, the scalars within test_gpu_fused_retract.py's bound."""
    tr, out = FR.run(11.5, 17, F, bcr_fold_back=1, fused_retract=fused)
    assert out["fused"] == bool(fused)
    assert tr.BcrFoldInfo()["last"] == 1
    FR.check_same_candidate(out)
    assert np.all(FR.rel_dev(out["s_loop"], out, out["xc_loop"]) <= FR.TOL)


def test_two_launches_per_level_with_the_fold_on():
    tr = run_folded(L.dataset(4.25), F, dict(Pb=405, n=7, a=9, hb=50, route="bcr_fused"), 1, bcr_join_levels=0)
    assert tr.BcrJoinInfo()["last"] == 0


# ---- a whole calibration ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_lm", [1, 0], ids=["device_lm", "host_lm"])
def test_c2_calibration_is_the_same_folded_and_not(device_lm):
    """Optimize(50, F) on C2 with the option 0 and 1: the same iteration counts, termination and per-iteration success flags, the final
    cost to 1e-9 relative (the atomics of a level land in any order under both: test_gpu_bcr_joined_levels.py)."""
    ds = synthetic.make_config("C2")
    runs = {}
    for fold in FOLD:
        tr = E.ImuCameraCalibrator().BatchInitSpline(ds).trajectory_
        tr.SetOption("device_lm", device_lm); tr.SetOption("bcr_fold_back", fold)
        s = tr.Optimize(50, F)
        runs[fold] = (s, tr.GetIterations(), tr.BcrFoldInfo())
        print("fold %d: iterations %d (%d + %d) final cost %.12e folded solves %d" % (fold, s["num_iterations"], s["num_successful_steps"],
                                                                                     s["num_unsuccessful_steps"], s["final_cost"], runs[fold][2]["total"]))
    (s0, it0, f0), (s1, it1, f1) = runs[0], runs[1]
    assert f0["total"] == 0 and f0["last"] == 0
    assert f1["total"] >= s1["num_iterations"] and f1["last"] == 1       # 29 blocks, four levels: every solve folds level 2
    for k in ("termination", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "message"):
        assert s1[k] == s0[k], (k, s1, s0)
    assert abs(s1["final_cost"] - s0["final_cost"]) <= 1e-9 * abs(s0["final_cost"]), (s1["final_cost"], s0["final_cost"])
    assert len(it1) == len(it0)
    for a, b in zip(it1, it0):
        assert a["iteration"] == b["iteration"] and a["step_is_successful"] == b["step_is_successful"], (a, b)
