"""The panel chain of the block cyclic reduction's 64 x 64 inversions (kernels_bcr.hip, bcri_invert_body) after its instruction count
was cut: the arithmetic of every entry and its order are those of the chain before, so wherever a solve reproduces itself bit for
bit it must reproduce the steps recorded from the library BEFORE that change.

Bits.  Bands of two and three blocks, each with no arrow column and with nine, at radius 1e4 -- the sizes at which one library's
solves agree in every bit (from eight blocks on the Schur atomics land in either order).  The Jacobian pass runs with
accumulation = 1 (every sum in a fixed order), and the fixture tests/golden/bcr_chain_bits.npz (scripts/make_bcr_chain_golden.py,
written on an MI355X from the commit before the change) holds a digest of the packed normal equations the solve read next to step_s,
D2 and scale: a case first asserts that it solves the recorded system.  These systems run the build launch, a top level with one and
with two end pivots and the last block with the side buffer.

Panel edges.  The planted negative pivots of tests/test_gpu_bcr_panel_failure.py run with the suite, unchanged.  Here: a diagonal
tile that is diagonal except ONE large entry (c + 2, c) (option debug_plant_tile: the sixteen variables of that tile are cut off from
every other variable for one solve), for c = 0 and c = 13 -- the first and the last column of a panel with an update that is not
the next column's: that entry is the only multiplier of such an update which is not zero.  check_step and its bounds, unchanged.

Sizes of the timed plan.  n = 8 with a level as one launch and as two, and n = 29: one solve each at radius 1e4 and 1e16; together
they run all five inverting kernels.
"""
import hashlib
import os

import numpy as np
import pytest

import test_gpu_linear_solve_reference as L
from openimucameracalibrator_amd import estimator as E

pytestmark = pytest.mark.gpu

RADIUS = 1e4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bcr_chain_bits.npz")
CASES = [   # (id, duration, n, flags, a)
    ("n2_a0", 0.75, 2, E.SPLINE, 0),
    ("n2_a9", 0.75, 2, L.F, 9),
    ("n3_a0", 1.2, 3, E.SPLINE, 0),
    ("n3_a9", 1.2, 3, L.F, 9),
]
KEPT = ("step_s", "D2", "scale")


def digest(out):
    """The packed normal equations a solve read, as one SHA-256."""
    h = hashlib.sha256()
    for k in ("band", "Et", "C", "g"):
        h.update(np.ascontiguousarray(out[k], dtype=np.float64).tobytes())
    return h.hexdigest()


def solve_twice(case):
    _, duration, n, flags, a = case
    tr = L.calibrator(L.dataset(duration), accumulation=1).trajectory_
    outs = [tr.DebugLmStep(flags, RADIUS) for _ in range(2)]
    for out in outs:
        assert out["route"] == "bcr_fused" and out["n"] == n and out["a"] == a, (out["route"], out["n"], out["a"])
        assert not out["chol_failed"]
    return outs


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_chain_reproduces_the_recorded_bits(case, golden):
    first, second = solve_twice(case)
    assert digest(first) == str(golden[case[0] + "__inputs_sha256"]), "the solve read another system than the recorded one"
    for k in KEPT:
        assert np.array_equal(first[k], second[k]), (case[0], k, "two consecutive solves differ")
        want = golden[case[0] + "__" + k]
        differ = np.flatnonzero(first[k] != want)
        assert differ.size == 0, (case[0], k, differ.size, differ[:8])


@pytest.mark.parametrize("c", [0, 13], ids=["c0", "c13"])
def test_one_deferred_multiplier(c):
    """Block 1 of three (the last block, with the side buffer), second panel: tile columns 80..95, the entry (c + 2, c) of the tile."""
    col = 64 + 16 + c
    tr = L.calibrator(L.dataset(1.2), debug_plant_tile=col).trajectory_
    out = tr.DebugLmStep(L.F, RADIUS)
    assert out["route"] == "bcr_fused" and out["n"] == 3 and col + 2 < out["Pb"]
    band, Et, Pb, W = out["band"], out["Et"], out["Pb"], out["W"]
    t0 = col - c
    H = np.zeros((Pb, Pb))                                           # the lower triangle the solve read: band[j, k] = H(j + k, j)
    for k in range(W):
        j = np.arange(Pb - k)
        H[j + k, j] = band[j, k]
    tile = np.zeros(Pb, bool)
    tile[t0:t0 + 16] = True
    cut = H.copy()
    cut[np.ix_(~tile, ~tile)] = 0.0                                  # what touches the tile's variables ...
    cut[np.arange(Pb), np.arange(Pb)] = 0.0                          # ... off the diagonal
    assert np.flatnonzero(cut).tolist() == [(col + 2) * Pb + col], "the tile's one off-diagonal entry is (col + 2, col)"
    assert np.all(Et[:, t0:t0 + 16] == 0.0) and np.all(band[t0:t0 + 16, 0] > 0)
    assert abs(band[col, 2]) == 0.875 * np.sqrt(band[col, 0] * band[col + 2, 0])   # large: the 2 x 2 block is just positive definite
    L.check_step(out, RADIUS, label="deferred multiplier, c = %d" % c)
    tr.SetOption("debug_plant_tile", -1)
    again = tr.DebugLmStep(L.F, RADIUS)
    assert np.count_nonzero(again["Et"][:, t0:t0 + 16]) > 0 and np.count_nonzero(again["band"][t0:t0 + 16, 1:]) > 16   # put back
    L.check_step(again, RADIUS, label="deferred multiplier taken out, c = %d" % c)


SIZES = [("n8_joined", 5.0, 8, {}), ("n8_own_launch", 5.0, 8, dict(bcr_join_levels=0)), ("n29", 20.0, 29, {})]


@pytest.mark.parametrize("name,duration,n,opts", SIZES, ids=[s[0] for s in SIZES])
def test_sizes_of_the_timed_plan(name, duration, n, opts):
    L.run_case(L.dataset(duration), L.F, dict(n=n, a=9, hb=50, route="bcr_fused"), radii=(1e4, 1e16), **opts)
