"""The panel chain of the 64 x 64 inversions (kernels_bcr.hip, bcri_invert_body) under the balanced schedule of its deferred updates
(bcr_chain_schedule.h): an update by column k on column c2 may now wait for the shadow of any column between them, so a schedule
can go wrong at every distance c2 - k, not only at the shortest one that option debug_plant_tile plants by default.

Every pair of one tile.  Option debug_plant_tile_dist = d moves the planted entry to (col + d, col): the tile's sixteen variables are
cut off from every other variable, and of the tile's Cholesky multipliers only l(col + d, col) is not zero -- the one deferred
update (k, c2) = (c, c + d) carries the whole coupling.  All 105 pairs c2 >= k + 2 of a tile, at two places of a three-block band
(duration 1.2 s): the second panel of block 1 (the last block, with the side buffer) and the third panel of block 0 (the build
launch).  Each solve is held to check_step and its bounds, unchanged, and its step over the tile's sixteen variables to the bits of
tests/golden/bcr_chain_schedule_bits.npz, which scripts/make_bcr_chain_schedule_golden.py wrote on an MI355X from the library of the
commit BEFORE the schedule changed (with this option added to it); the fixture holds a SHA-256 of the packed normal equations each
solve read, and a case first asserts that it solves the recorded system.  The Jacobian pass runs with accumulation = 1.

Sizes of the timed plan.  n = 8 with a level as one launch and as two, and n = 29, one solve each at radius 1e4: together they run
all five inverting kernels.
"""
import hashlib
import os

import numpy as np
import pytest

import test_gpu_linear_solve_reference as L

pytestmark = pytest.mark.gpu

RADIUS = 1e4
DURATION = 1.2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bcr_chain_schedule_bits.npz")
PLACES = [("last_block_panel1", 64 + 16), ("build_block0_panel2", 32)]   # (id, first band column of the tile)
PAIRS = [(c, d) for c in range(14) for d in range(2, 16 - c)]            # the entry (c + d, c) of the tile


def digest(out):
    """The packed normal equations a solve read, as one SHA-256."""
    h = hashlib.sha256()
    for k in ("band", "Et", "C", "g"):
        h.update(np.ascontiguousarray(out[k], dtype=np.float64).tobytes())
    return h.hexdigest()


def solve_pairs(t0, check=False):
    """One solve per pair of the tile at band column t0: (step_s over the tile [105, 16], the digests of the systems read)."""
    assert len(PAIRS) == 105
    tr = L.calibrator(L.dataset(DURATION), accumulation=1).trajectory_
    steps, digests = np.zeros((len(PAIRS), 16)), []
    for i, (c, d) in enumerate(PAIRS):
        col = t0 + c
        tr.SetOption("debug_plant_tile", col)
        tr.SetOption("debug_plant_tile_dist", d)
        out = tr.DebugLmStep(L.F, RADIUS)
        assert out["route"] == "bcr_fused" and out["n"] == 3 and t0 + 16 <= out["Pb"] and out["W"] > 15
        band, Et = out["band"], out["Et"]
        assert abs(band[col, d]) == 0.875 * np.sqrt(band[col, 0] * band[col + d, 0])      # the planted entry, large
        Pb, W = out["Pb"], out["W"]
        inside = (np.arange(t0, t0 + 16)[:, None] + np.arange(1, W)[None, :]) < Pb        # band[j, k] = H(j + k, j)
        planted = np.zeros_like(band[t0:t0 + 16, 1:])
        planted[c, d - 1] = band[col, d]
        assert np.array_equal(band[t0:t0 + 16, 1:][inside], planted[inside]), "the tile's one off-diagonal entry is (col + d, col)"
        for k in range(1, W):                                                             # nothing reaches into the tile from above
            assert np.all(band[max(0, t0 - k):max(0, min(t0, t0 + 16 - k)), k] == 0.0)
        assert np.all(Et[:, t0:t0 + 16] == 0.0) and np.all(band[t0:t0 + 16, 0] > 0) and not out["chol_failed"]
        if check:
            L.check_step(out, RADIUS, label="deferred multiplier (%d, %d) at %d" % (c, c + d, t0))
        steps[i] = out["step_s"][t0:t0 + 16]
        digests.append(digest(out))
    return steps, np.array(digests)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name,t0", PLACES, ids=[p[0] for p in PLACES])
def test_every_deferred_multiplier_of_a_tile(name, t0, golden):
    steps, digests = solve_pairs(t0, check=True)
    assert np.array_equal(digests, golden[name + "__inputs_sha256"]), "a solve read another system than the recorded one"
    want = golden[name + "__step_s"]
    differ = np.argwhere(steps != want)
    assert differ.size == 0, (name, len(differ), [(PAIRS[i], int(j)) for i, j in differ[:8]])
    assert np.all(np.count_nonzero(steps, axis=1) == 16)


def test_default_distance_is_two():
    """debug_plant_tile alone plants (col + 2, col), as before the distance option existed."""
    t0, c = 80, 5
    tr = L.calibrator(L.dataset(DURATION), debug_plant_tile=t0 + c).trajectory_
    band = tr.DebugLmStep(L.F, RADIUS)["band"]
    assert np.flatnonzero(band[t0:t0 + 16, 1:16]).tolist() == [c * 15 + 1]
    tr.SetOption("debug_plant_tile_dist", 16 - c)                     # out of range: nothing is planted
    assert np.count_nonzero(tr.DebugLmStep(L.F, RADIUS)["band"][t0:t0 + 16, 1:16]) > 16


SIZES = [("n8_joined", 5.0, 8, {}), ("n8_own_launch", 5.0, 8, dict(bcr_join_levels=0)), ("n29", 20.0, 29, {})]


@pytest.mark.parametrize("name,duration,n,opts", SIZES, ids=[s[0] for s in SIZES])
def test_sizes_of_the_timed_plan(name, duration, n, opts):
    L.run_case(L.dataset(duration), L.F, dict(n=n, a=9, hb=50, route="bcr_fused"), radii=(RADIUS,), **opts)
