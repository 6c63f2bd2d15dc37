"""The membership rule of tests/inner_evaluation_reference.py against the library's own plan of the inner iterations, without a GPU:
the plan is built on a host-only problem object (oicc_debug_create_host_only / oicc_debug_host_inner_plan), the reference on the oracle.

Unit of the item counts: the plan's InnerBlock::n_items counts ITEMS -- one per corner of a view that depends on the block, one per
accelerometer / gyroscope sample that depends on it -- and so does BlockSums.block(...)[4]; every block of these shapes (rolling-
shutter views only) is counted in that unit, the board points (all corners of the views that see the point) included."""
import numpy as np
import pytest

import oracle_backend
import normal_equations_cases as cases
import inner_evaluation_reference as R
from test_inner_plan_host import _HostOnly
from openimucameracalibrator_amd import estimator as E

FLAG_SETS = [("FLAGS1", cases.FLAGS1), ("ALL", cases.ALL)]


@pytest.mark.parametrize("shape", ["tiny", "gap", "ragged"])
def test_every_block_of_the_plan_has_its_columns_and_its_items(shape):
    _, build, options = cases.SHAPES[shape]
    ds = build()
    host = E.ImuCameraCalibrator(trajectory=_HostOnly()).BatchInitSpline(ds)
    cpu = E.ImuCameraCalibrator(backend=oracle_backend.load()).BatchInitSpline(ds)
    for k, v in options.items():
        host.trajectory_.SetOption(k, v); cpu.trajectory_.SetOption(k, v)
    for fname, flags in FLAG_SETS:
        blocks, n_sets, _ = host.trajectory_.plan(flags)          # [set, kind, idx, n_items, n_slots, ...]
        ref = R.block_sums(cpu, ds, flags)
        assert len(blocks) > 0 and ref.P > 0
        seen = np.zeros(ref.P, np.int64)
        g = np.zeros(ref.P, R.LD)
        for b in blocks:
            kind, idx = int(b[1]), int(b[2])
            assert ref.columns(kind, idx) is not None, (shape, fname, "block without columns", kind, idx)
            cols, H_b, g_b, cost_b, items = ref.block(kind, idx)
            seen[cols] += 1
            g[cols] += g_b
            assert items == int(b[3]), (shape, fname, R.describe_block(ref.L, kind, idx, cols), "items", items, int(b[3]))
            assert items > 0 and float(cost_b) > 0.0 and H_b.shape == (len(cols), len(cols))
            assert int(b[4]) >= items and int(b[4]) % 64 == 0          # slots: every run padded to a multiple of 64
        assert (seen == 1).all(), (shape, fname, "the blocks' columns do not partition [0, P)", np.flatnonzero(seen != 1)[:8])
        assert np.array_equal(g, ref.g), (shape, fname)
        # every residual block depends on at least one block, and the blocks of one set share none (the definition of an independent set)
        for s in range(n_sets):
            hit = {k: np.zeros(len(ref.block_cost[k]), np.int64) for k in (0, 1, 2)}
            for b in blocks[blocks[:, 0] == s]:
                dep = ref.dependents(int(b[1]), int(b[2]))
                for k in (0, 1, 2):
                    hit[k] += dep[k]
            assert all((hit[k] <= 1).all() for k in (0, 1, 2)), (shape, fname, "set", s)
