"""The 50-digit restatement of the spline calibration's residual rows (spline_rows_reference.py) against the oracle, on the host:
the reference's own checks (its stencil against the Jets, its blending matrices, its cases clear of branches, the floor cap), the
float64 yardsticks of the rows and of J^T J, J^T r (YARDSTICK in spline_rows_reference.py: the Jet oracle against the 50 digits), and
the oracle's ANALYTIC path -- the host compile of block_items.h / spline_seg.h / spline_math.h, the code the device runs -- held
to DEVICE_FACTOR x yardstick for every case and all three kinds."""
import numpy as np
import pytest

import normal_equations_reference as NE
import oracle_backend
import spline_rows_cases as K
import spline_rows_reference as R

SEEDS = (1, 2, 3)
_measured = {}


def sources(name, analytic):
    P = K.problem(name)
    tr = K.build(oracle_backend.load(), P)
    tr.SetOption("analytic_jacobians", analytic)
    return P, tr, K.EstimatorRows(P, tr, jets=not analytic)


def measure_rows(name, analytic):
    """{"view/residual": figure, ...}, (pairs on the floor, pairs) of the case."""
    key = ("rows", name, analytic)
    if key not in _measured:
        P, tr, src = sources(name, analytic)
        figures, floor = {}, np.zeros(2, np.int64)
        for kind in (0, 1, 2):
            r_ref, J_ref = R.rows(P, kind, P["flags"])
            r, J = src.EvaluateBlocks(P["flags"], kind, len(r_ref))
            fig, fl = R.row_figures(P, kind, r, J, r_ref, J_ref, not P["residuals_only"])
            floor += fl
            for f, v in fig.items():
                if f == "residual" or not P["residuals_only"]:
                    figures["%s/%s" % (R.KIND_NAMES[kind], f)] = v
        _measured[key] = (figures, floor)
    return _measured[key]


def ne_error(H, g, ref):
    cost, Href, gref = ref
    return max(NE.entrywise_error(H, Href)[0], NE.gradient_error(g, gref, Href, cost)[0])


def measure_normal_equations(name, analytic):
    """(entry-wise error of the float64 assembly of the source's rows, blocks shuffled, the largest of three seeds; relative cost error)."""
    key = ("ne", name, analytic)
    if key not in _measured:
        P, tr, src = sources(name, analytic)
        ref = K.assemble(P, tr, P["flags"], rows_of=R.RowsBackend(P))
        worst, cost_err = 0.0, 0.0
        for seed in SEEDS:
            c, H, g = K.assemble(P, tr, P["flags"], rows_of=src, dtype=np.float64, shuffle_seed=seed)
            worst = max(worst, ne_error(H, g, ref))
            cost_err = max(cost_err, abs(float(c - ref[0])) / float(ref[0]))
        _measured[key] = (worst, cost_err)
    return _measured[key]


# ---- the reference's own checks ------------------------------------------------------------------------------------------------
def test_stencil_agrees_with_the_jets_on_the_generic_case():
    """Settles the tangent conventions: every column of every item, relative to the column's norm in that item (columns below
    ROW_FLOOR x the largest of their family by that), to 1e-9; residuals to 1e-12 of their scale."""
    for name in ("generic", "generic_division"):
        figures, _ = measure_rows(name, 0)
        for key, v in figures.items():
            assert v <= (1e-12 if key.endswith("residual") else 1e-9), (name, key, v)


def test_blending_matrices_match_the_tables_and_the_oracle():
    """the closed formula against the constants of SURVEY.md 8a row A1 (kM6, kMc6, kM3 of spline_math.h) and, through the oracle's
    spline evaluation, as weights: R^3 value and derivatives of unit knots, the angle of a cumulative spline about one axis"""
    as_int = lambda M, s: [[int(v * s) for v in row] for row in M]
    assert all(v.denominator in (1, 2, 3, 4, 5, 6, 8, 10, 12, 15, 20, 24, 30, 40, 60, 120) for row in R.M6 + R.MC6 for v in row)
    assert as_int(R.M6, 120) == [[1, -5, 10, -10, 5, -1], [26, -50, 20, 20, -20, 5], [66, 0, -60, 0, 30, -10], [26, 50, 20, -20, -20, 10], [1, 5, 10, 10, 5, -5], [0, 0, 0, 0, 0, 1]]
    assert as_int(R.MC6, 120) == [[120, 0, 0, 0, 0, 0], [119, 5, -10, 10, -5, 1], [93, 55, -30, -10, 15, -4], [27, 55, 30, -10, -15, 6], [1, 5, 10, 10, 5, -4], [0, 0, 0, 0, 0, 1]]
    assert as_int(R.M3, 2) == [[1, -2, 1], [1, 2, -2], [0, 0, 1]]
    import ctypes
    import mpmath as mp
    lib = oracle_backend.load().raw
    dp = ctypes.POINTER(ctypes.c_double)
    lib.oicc_oracle_eval_r3.argtypes = [dp, ctypes.c_int, ctypes.c_double, ctypes.c_double, dp]
    lib.oicc_oracle_eval_so3.argtypes = [dp, ctypes.c_double, ctypes.c_double, dp, dp]
    for u in (0.0, 1e-9, 0.37, 1.0 - 1e-9, 1.2, -0.4):
        for j in range(6):
            knots = np.zeros((6, 3)); knots[j, 0] = 1.0
            for deriv in (0, 1, 2):
                out = np.zeros(3)
                lib.oicc_oracle_eval_r3(knots.ctypes.data_as(dp), deriv, u, 10.0, out.ctypes.data_as(dp))
                want = float(R._coeffs(mp.mp, R.M6, mp.mpf(u), deriv, mp.mpf(10))[j])
                assert abs(out[0] - want) <= 64 * R.EPS * 10.0 ** deriv * (1 + abs(u)) ** 5, (u, j, deriv, out[0], want)
            step = 0.3
            q = np.zeros((6, 4)); q[:, 3] = 1.0
            q[j:, 2], q[j:, 3] = np.sin(step / 2), np.cos(step / 2)
            qo, wo = np.zeros(4), np.zeros(3)
            lib.oicc_oracle_eval_so3(q.ctypes.data_as(dp), u, 10.0, qo.ctypes.data_as(dp), wo.ctypes.data_as(dp))
            k = float(R._coeffs(mp.mp, R.MC6, mp.mpf(u), 0, 1)[j]); dk = float(R._coeffs(mp.mp, R.MC6, mp.mpf(u), 1, mp.mpf(10))[j])
            assert abs(2 * np.arctan2(qo[2], qo[3]) - k * step) <= 64 * R.EPS * (1 + abs(u)) ** 5, (u, j)
            assert abs(wo[2] - dk * step) <= 64 * R.EPS * 10 * (1 + abs(u)) ** 5, (u, j)


@pytest.mark.parametrize("name", K.CASES)
def test_cases_are_clear_of_branches(name):
    R.assert_clear_of_branches(K.problem(name))


def test_floor_cap():
    """at most FLOOR_CAP of the (item, column) pairs of the whole case table are scaled by the floor instead of their own norm"""
    total = sum(measure_rows(name, 0)[1] for name in K.CASES)
    print("on the floor: %d of %d pairs" % (total[0], total[1]))
    assert total[0] <= R.FLOOR_CAP * total[1], total


# ---- yardsticks and the analytic path ----------------------------------------------------------------------------------------------
def _check_measured(key, fresh):
    entry = R.YARDSTICK[key]
    assert entry / 8 <= fresh <= entry, (key, fresh, entry)


@pytest.mark.parametrize("name", K.CASES)
def test_float64_yardstick_and_analytic_path_rows(name):
    """Residual, family-relative and column-relative figure of every kind: the Jet oracle's lie within [1/8, 1] of the table,
    those of the host compile of the device's closed forms within DEVICE_FACTOR x the table."""
    jets, _ = measure_rows(name, 0)
    closed, _ = measure_rows(name, 1)
    bad = []
    for f in jets:
        key = "%s/%s" % (name, f)
        _check_measured(key, jets[f])
        print("%-44s jets %.3e  closed forms %.3e  bound %.3e" % (key, jets[f], closed[f], R.DEVICE_FACTOR * R.yardstick(key)))
        if not closed[f] <= R.DEVICE_FACTOR * R.yardstick(key):
            bad.append((key, closed[f], R.yardstick(key)))
    assert not bad, bad


@pytest.mark.parametrize("name", [n for n in K.CASES if not K.problem(n)["residuals_only"]])
def test_float64_yardstick_and_analytic_path_normal_equations(name):
    """J^T J and J^T r of the case, every entry by its own d_i d_j: a float64 sum of the Jet oracle's rows within [1/8, 1] of the
    table, of the closed forms' rows within DEVICE_FACTOR x the table."""
    jets, cost_j = measure_normal_equations(name, 0)
    closed, cost_c = measure_normal_equations(name, 1)
    key = name + "/ne"
    print("%-44s jets %.3e  closed forms %.3e  bound %.3e   cost: %.2e %.2e" % (key, jets, closed, R.DEVICE_FACTOR * R.yardstick(key), cost_j, cost_c))
    _check_measured(key, jets)
    assert closed <= R.DEVICE_FACTOR * R.yardstick(key), (key, closed, R.yardstick(key))
    assert cost_c <= R.COST_BOUND, (key, cost_c)


def test_first_lm_step_of_the_static_window_on_the_oracle():
    """The check of the GPU test on the host: one LM iteration from all segment angles zero is finite and accepted (no coin toss:
    the relative decrease is 0.1 or more away from the threshold), and the cost it reports is the 50-digit cost at the parameters
    it left."""
    P = K.problem("static/lm")
    R.assert_clear_of_branches(P)
    for analytic in (0, 1):
        tr = K.build(oracle_backend.load(), P)
        tr.SetOption("analytic_jacobians", analytic)
        K.check_first_lm_step(P, tr)
