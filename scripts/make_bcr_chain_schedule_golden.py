"""Writes tests/golden/bcr_chain_schedule_bits.npz, the fixture of tests/test_gpu_bcr_chain_schedule.py: for each of that test's two
tiles and each of the 105 planted entries (c + d, c) of a tile, step_s over the tile's sixteen variables and a SHA-256 of the packed
normal equations the solve read (three blocks, seeded synthetic data, accumulation = 1).  Run it on an MI355X with the library of the
commit whose bits are to be held -- the fixture in the tree was written from the commit BEFORE the deferred updates of the panel
chain were rescheduled, with nothing added to that commit but option debug_plant_tile_dist (as scripts/make_bcr_chain_golden.py's
fixture was written with option debug_plant_tile added):

    python scripts/make_bcr_chain_schedule_golden.py [output.npz]

Two consecutive passes over the 105 entries must agree in every bit, or nothing is written.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_gpu_bcr_chain_schedule as T   # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
arrays = {}
for name, t0 in T.PLACES:
    steps, digests = T.solve_pairs(t0)
    again, digests2 = T.solve_pairs(t0)
    assert np.array_equal(steps, again) and np.array_equal(digests, digests2), name
    assert np.all(np.isfinite(steps)) and len(set(digests.tolist())) == len(T.PAIRS), name
    arrays[name + "__step_s"] = steps
    arrays[name + "__inputs_sha256"] = digests
    print("%-22s tile at %3d  %d solves  |step_s| %.17g  inputs %s .. %s" % (name, t0, len(steps), np.abs(steps).max(), digests[0][:16], digests[-1][:16]))
np.savez_compressed(out_path, **arrays)
print("wrote %s (%d bytes)" % (out_path, os.path.getsize(out_path)))
