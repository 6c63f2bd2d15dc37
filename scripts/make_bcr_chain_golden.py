"""Writes tests/golden/bcr_chain_bits.npz, the fixture of tests/test_gpu_bcr_chain_bits.py: step_s, D2 and scale of that test's small
systems (two and three blocks, no arrow column and nine; seeded synthetic data, accumulation = 1) and a SHA-256 of the packed normal
equations each solve read.  Run it on an MI355X with the library of the commit whose bits are to be held -- the fixture in the tree
was written from the commit BEFORE the panel chain's instruction count was cut:

    python scripts/make_bcr_chain_golden.py [output.npz]

Two consecutive solves must agree in every bit, or nothing is written.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_gpu_bcr_chain_bits as T   # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
arrays = {}
for case in T.CASES:
    first, second = T.solve_twice(case)
    for k in T.KEPT:
        assert np.array_equal(first[k], second[k]), (case[0], k)
        arrays[case[0] + "__" + k] = first[k]
    arrays[case[0] + "__inputs_sha256"] = np.array(T.digest(first))
    print("%-8s Pb %4d a %2d P %4d  |step_s| %.17g  inputs %s" % (case[0], first["Pb"], first["a"], first["P"], np.abs(first["step_s"]).max(), T.digest(first)[:16]))
np.savez_compressed(out_path, **arrays)
print("wrote %s (%d bytes)" % (out_path, os.path.getsize(out_path)))
