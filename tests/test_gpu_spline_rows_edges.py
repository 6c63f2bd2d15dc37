"""The spline calibration's residual rows on the device against the 50-digit restatement (spline_rows_reference.py) at the edges
of the row code -- identical knots, the log and series switches, rotations near pi, samples on knot times, rolling-shutter shifts
out of [0, 1), the first and last window (spline_rows_cases.py):

  * EvaluateBlocks of the three kinds: residual, family-relative and column-relative figure within DEVICE_FACTOR x the float64
    yardstick of the case (YARDSTICK; measured on the host by test_spline_rows_reference.py), with debug_poison_lds set;
  * Evaluate -- the production path: tiles, compact LDS rows, Gram product, slab merge, shared segment tables -- against the
    long-double sum of the 50-digit rows: cost to 1e-14, J^T J and J^T r entry by entry, every entry scaled by its own d_i d_j;
  * the first LM step of a trajectory with all segment angles zero.

Every figure is printed before it is asserted."""
import pytest

import normal_equations_reference as NE
import spline_rows_cases as K
import spline_rows_reference as R
from test_gpu_ba_edges import check

pytestmark = pytest.mark.gpu

ASSEMBLY_OPTIONS = {"default": {}, "assembly2": {"assembly": 2}, "narrow_cells": {"wide_cells": 0}}


@pytest.mark.parametrize("name", K.CASES)
def test_rows_at_the_edges(name):
    P = K.problem(name)
    tr = K.build(None, P, {"debug_poison_lds": 1})
    figures = []
    for kind in (0, 1, 2):
        r_ref, J_ref = R.rows(P, kind, P["flags"])
        r, J = tr.EvaluateBlocks(P["flags"], kind, len(r_ref))
        fig, _ = R.row_figures(P, kind, r, J, r_ref, J_ref, not P["residuals_only"])
        for f, v in fig.items():
            if f == "residual" or not P["residuals_only"]:
                key = "%s/%s/%s" % (name, R.KIND_NAMES[kind], f)
                figures.append((key, v, R.DEVICE_FACTOR * R.yardstick(key)))
    check(figures)


@pytest.mark.parametrize("name,variant", [(n, "default") for n in K.CASES] + [(n, v) for v in ("assembly2", "narrow_cells") for n in K.ASSEMBLY_SUBSET])
def test_normal_equations_of_the_edge_problems(name, variant):
    P = K.problem(name)
    tr = K.build(None, P, ASSEMBLY_OPTIONS[variant])
    cost, Href, gref = K.assemble(P, tr, P["flags"], rows_of=R.RowsBackend(P))
    c, H, g = tr.Evaluate(P["flags"])
    assert H.shape == Href.shape
    figures = [("cost", abs(float(c - cost)) / float(cost), R.COST_BOUND)]
    if not P["residuals_only"]:
        bound = R.DEVICE_FACTOR * R.yardstick(name + "/ne")
        figures += [("H", NE.entrywise_error(H, Href)[0], bound), ("g", NE.gradient_error(g, gref, Href, cost)[0], bound)]
    check(figures)


def test_first_lm_step_of_the_static_window():
    """all segment angles zero (inv_theta = 0 in every segment table entry): the step is finite, accepted, and the cost the
    iteration reports is the 50-digit cost at the parameters it left, to 1e-12"""
    P = K.problem("static/lm")
    K.check_first_lm_step(P, K.build(None, P))
