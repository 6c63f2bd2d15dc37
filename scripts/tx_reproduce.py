"""Which cases of tests/test_gpu_bcr_joined_tx.py reproduce their joined solve bit for bit: python scripts/tx_reproduce.py [repeats]
Run it on the PARENT's library (OICC_DEV_LIB=scratch_bin/liboicc_parent.so, scripts/build_variant.sh) to find the set REPRODUCES of
that test -- from four blocks on two pivots of level 0 add onto one neighbour in either order, so only some cases do -- and on this
tree's to see that the same cases still do."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_gpu_linear_solve_reference as L   # noqa: E402
import test_gpu_bcr_joined_tx as T            # noqa: E402

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 6
print("library:", os.environ.get("OICC_DEV_LIB", "this tree's"), " repeats:", repeats)
keep = []
for n, a in T.CASES:
    duration, Pb, joined = T.BLOCKS[n]
    flags, kw = T.FLAGS[a]
    tr = L.calibrator(L.dataset(duration, **kw), bcr_join_levels=1).trajectory_
    same, failed = [], []
    for radius in (1e4, 1e16):   # (both, also where the test solves at 1e4 only: the factorisation fails at 1e16 with board points)
        outs = [tr.DebugLmStep(flags, radius) for _ in range(repeats)]
        same.append(all(np.array_equal(o["step_s"], outs[0]["step_s"]) for o in outs[1:]))
        failed.append(any(o["chol_failed"] for o in outs))
    assert tr.BcrJoinInfo()["last"] == joined
    print("n %d a %2d  reproduces at radius 1e4: %-5s 1e16: %-5s   factorisation failed: %s %s" % (n, a, same[0], same[1], failed[0], failed[1]))
    if all(same):
        keep.append((n, a))
print("REPRODUCES =", keep)
