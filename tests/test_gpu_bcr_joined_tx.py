"""The T stage of the joined levels of the block cyclic reduction (kernels_bcr.hip: bcri_tx_stage in bcri_invert_schur_kernel), which
forms a Schur group's tile as T_x = (B_x X) X^T from X = L^-T in ten 4-MFMA chunks per factor and never builds Z = X X^T, against
the extended-precision host solve of tests/test_gpu_linear_solve_reference.py: its run_case (poisoned LDS), check_step and
BACKWARD / FORWARD_C bounds, unchanged.  tests/test_bcr_tx_restatement.py restates the chunk schedule on the host.

The shapes are the smallest at which the stage can go wrong:
  n = 4   one joined level, a pivot with a left neighbour only (the groups of the right side leave);
  n = 5   the same behind a level 0 with a left-end pivot;
  n = 7   two top pivots, the left one writes through the side buffer;
  n = 8   two joined levels, the last launch retracts;
  a = 0 (the border tile holds the rhs row alone), 9, 15 (one full border tile), 16 (two) at every n; a = 63 (four) at n = 5.
Radii 1e4 and 1e16; the board-point case a = 63 at 1e4 only, as in test_gpu_linear_solve_reference.py: the board points leave the
undamped system singular up to the gauge, and at radius 1e16 the factorisation fails on every route and library (measured on the
parent commit's library as well: scripts/tx_reproduce.py prints it).  Every case asserts
  - how many levels ran joined (estimator.BcrJoinInfo) with option bcr_join_levels 1 and 0;
  - check_step for both routes (inside run_case);
  - that the two routes' steps differ by no more than the sum of the forward bounds each is held to,
    FORWARD_C kappa_1 eps max|d*| each: they are two associations of one product, B (X X^T) and (B X) X^T;
  - REPRODUCES: where the parent commit's joined solve gave the same bits in every repetition, the solve is repeated and must give
    the same bits again -- the partial tiles of T_x are summed in a fixed order, so a difference there would be a race in the LDS
    partial sums.  Measured with scripts/tx_reproduce.py, 20 repetitions per case and radius on the parent commit's library: NO
    case reproduces itself at both radii (only n = 4, a = 0 at radius 1e16 did, and n = 7, a = 0 at 1e4 in some sessions): from
    four blocks on two pivots of level 0 add onto one neighbour, and with an arrow every pivot adds onto the corner, in either
    order.  So the set is empty and the assertion idle; every case still prints whether its three repetitions agreed.  What holds
    the partial sums instead: where solves did reproduce, the kernel with all ten chunks behind the factorisation and the one
    with the panels 0..2 in the shadow of the chains gave equal bits (n = 4, a = 0 at both radii; n = 7, a = 0 at 1e4; n = 8,
    a = 0 at 1e16), and run_case poisons the LDS ahead of every solve, so that a partial tile read before it was written is no stale copy of itself.

Measured on an MI355X over all cases (printed as MARGIN / TX lines; per case in DESIGN §6): backward error <= 8.0e-16 (bound 1e-13),
forward error / (kappa_1 eps) <= 3.1e-2 (bound 100), |joined - two launches| / bound <= 9.7e-5.
"""
import numpy as np
import pytest

import test_gpu_linear_solve_reference as L
import lm_step_reference as R
from openimucameracalibrator_amd import estimator as E

pytestmark = pytest.mark.gpu

F = L.F
RADII = (1e4, 1e16)
ARROW = {c[0]: c for c in L.ARROWS}
FLAGS = {0: (E.SPLINE, {}), 9: (F, {}), 15: ARROW[15][1:], 16: ARROW[16][1:], 63: ARROW[63][1:]}
BLOCKS = {4: (2.5, 252, 1), 5: (3.0, 297, 1), 7: (4.25, 405, 1), 8: (5.0, 477, 2)}    # n: (duration, Pb, joined levels)
CASES = [(n, a) for n in (4, 5, 7, 8) for a in (0, 9, 15, 16)] + [(5, 63)]
REPEATS = 3

# (n, a) whose joined solve reproduced itself bit for bit at both radii in every one of 20 repetitions on the parent commit's library: none
REPRODUCES = set()


def radii_of(flags):
    return RADII[:1] if flags & E.POINTS else RADII


def solve(n, a, join):
    duration, Pb, joined = BLOCKS[n]
    flags, kw = FLAGS[a]
    radii = radii_of(flags)
    tr = L.run_case(L.dataset(duration, **kw), flags, dict(Pb=Pb, n=n, a=a, route="bcr_fused"), radii=radii, bcr_join_levels=join)
    info = tr.BcrJoinInfo()
    want = joined if join else 0
    assert info["on"] == bool(join) and info["last"] == want and info["total"] == want * len(radii), (n, a, info)
    return tr, flags


@pytest.mark.parametrize("n,a", CASES, ids=["n%d_a%d" % c for c in CASES])
def test_joined_tx(n, a):
    tr1, flags = solve(n, a, 1)
    tr0, _ = solve(n, a, 0)
    for radius in radii_of(flags):
        out1, out0 = tr1.DebugLmStep(flags, radius), tr0.DebugLmStep(flags, radius)
        bound = 0.0
        for out in (out1, out0):
            S = R.from_step(out, radius, L.MIN_DIAG, L.MAX_DIAG)[2]
            bound += L.FORWARD_C["bcr_fused"] * S.cond1() * L.EPS * np.abs(S.solve()).max()
        diff = np.abs(out1["step_s"] - out0["step_s"]).max()
        same = all(np.array_equal(tr1.DebugLmStep(flags, radius)["step_s"], out1["step_s"]) for _ in range(REPEATS))
        print("TX n %d a %2d radius %.0e  |joined - two launches| %.3e  bound %.3e  ratio %.3e  reproduces %s"
              % (n, a, radius, diff, bound, diff / bound, same))
        assert diff <= bound, (n, a, radius, diff, bound)
        if (n, a) in REPRODUCES:
            assert same, (n, a, radius)
