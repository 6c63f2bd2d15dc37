"""Host reference of what one block of the inner iterations sums at an evaluation: H_b, g_b and cost_b in extended precision.

A sweep of the inner iterations (csrc/inner_iterations.hip) minimises one parameter block at a time over the residual blocks that
depend on it.  At a fixed point the sums of a block's Jacobian evaluation have an exact meaning in terms of the WHOLE problem:
    H_b, g_b  = the diagonal block / the segment of J^T J and J^T r at the block's tangent columns,
    cost_b    = sum of r_k . r_k / 2 over the residual blocks k that depend on the block.
Residual blocks are Ceres': a view with ALL its corners, an accelerometer sample, a gyroscope sample.  Block k depends on block b when
its row of `normal_equations_reference.block_columns` names at least one column of b; a view depends on a board point when one of its
corners refers to the point (the block dump has no point columns) -- the cost of a point block is that of all corners of those views,
as for every other block a view depends on.
ITEMS, the unit the plan counts in (InnerBlock::n_items): one per corner of a dependent view, one per dependent IMU sample.

Built on normal_equations_reference (assemble, block_times, block_columns: nothing of it is restated here); every sum in np.longdouble.
"""
import numpy as np

import normal_equations_reference as N
from openimucameracalibrator_amd import estimator as E

LD = N.LD
# InnerKind (csrc/inner_plan.h)
IK_SO3, IK_R3, IK_TIC, IK_G, IK_LD, IK_AB, IK_GB, IK_AI, IK_GI, IK_PT = range(10)
_KNOT_LAYOUT = {IK_SO3: "so3", IK_R3: "r3", IK_AB: "accl_bias", IK_GB: "gyro_bias"}
_OTHER = {IK_TIC: (0, 6), IK_G: (1, 3), IK_LD: (2, 1), IK_AI: (3, 6), IK_GI: (4, 9)}          # kind -> (entry of layout["other"], tangent size)
ITEMS_PER_ROW = {0: 2, 1: 3, 2: 3}          # residual rows of one item: a corner, an IMU sample


def nv_of(dim):
    """Doubles of a block's sums: upper triangle of H_b, g_b, cost_b."""
    return dim * (dim + 1) // 2 + dim + 1


def unpack(row, dim):
    """[56] sums of the kernels (upper triangle of H row by row | g | cost | zeros) -> H [dim, dim], g [dim], cost, tail."""
    iu = np.triu_indices(dim)
    H = np.zeros((dim, dim), row.dtype)
    nh = len(iu[0])
    H[iu] = row[:nh]
    H = H + np.triu(H, 1).T
    return H, row[nh:nh + dim].copy(), row[nh + dim], row[nv_of(dim):]


class RowsAfterLoss:
    """A rows backend whose view dump holds the rows AFTER the loss function.  The Jet oracle's EvaluateBlocks returns them before it
    (DESIGN.md section 6); the two differ only for global-shutter views without weight (quirk Q2, HuberLoss(0), option gs_unit_loss = 0):
    there every Evaluate -- and the sweeps -- sum nothing for a view, so its rows are zero here."""

    class _Trajectory:
        def __init__(self, tr, views_have_weight):
            self._tr, self._w = tr, views_have_weight

        def EvaluateBlocks(self, flags, kind, n_rows, want_jac=True):
            r, J = self._tr.EvaluateBlocks(flags, kind, n_rows, want_jac)
            if kind == 0 and not self._w:
                r = np.zeros_like(r); J = np.zeros_like(J) if J is not None else None
            return r, J

    def __init__(self, calibrator, views_have_weight):
        self.trajectory_ = self._Trajectory(calibrator.trajectory_, views_have_weight)
        self.num_corners = calibrator.num_corners


class BlockSums:
    """The reference of one (data set, flags): `block(kind, idx)` -> (columns, H_b, g_b, cost_b, items)."""

    def __init__(self, calibrator, ds, flags, rows_backend=None, evaluate_backend=None):
        """rows_backend: whose EvaluateBlocks rows are summed (default: `calibrator`).  evaluate_backend: whose Evaluate gives H, g of
        the POINT columns (the block dump has none); without it point blocks have a cost and columns only."""
        rows_backend = calibrator if rows_backend is None else rows_backend
        tr = calibrator.trajectory_
        self.flags = flags
        self.L = tr.GetTangentLayout(flags)
        self.P = self.L["P"]
        self.kinds = N.column_kinds(self.L)
        self.pts = np.asarray(tr.GetScenePointOffsets(flags)) if flags & E.POINTS else np.zeros(0, np.int64)
        self.cost, self.H, self.g, self.touched = N.assemble(calibrator, ds, flags, rows_backend=rows_backend, want_touched=True)
        self.n_a = int(self.pts[self.pts >= 0].min()) if (self.pts >= 0).any() else self.P          # columns the block dump covers
        if evaluate_backend is not None and self.n_a < self.P:
            _, Hj, gj = evaluate_backend.trajectory_.Evaluate(flags)
            self.H = self.H.copy(); self.g = self.g.copy()
            self.H[self.n_a:, self.n_a:] = Hj[self.n_a:, self.n_a:]; self.g[self.n_a:] = gj[self.n_a:]
            self.touched[self.n_a:, self.n_a:] = Hj[self.n_a:, self.n_a:] != 0
            self.has_point_H = True
        else:
            self.has_point_H = False
        # per residual block: its cost, its items, the columns it names
        times = N.block_times(calibrator, ds)
        self.block_cost, self.block_items, self.block_cols, self.block_first_knot = {}, {}, {}, {}
        for kind in (0, 1, 2):
            t_ns, rpb = times[kind]
            nrows = int(rpb.sum())
            n_dump = 2 * int(rows_backend.num_corners) if kind == 0 else nrows
            r, _ = rows_backend.trajectory_.EvaluateBlocks(flags, kind, n_dump, want_jac=False)
            sq = r[:nrows].astype(LD) ** 2 / 2
            first = np.concatenate([[0], np.cumsum(rpb)]).astype(np.int64)
            self.block_cost[kind] = np.array([sq[first[k]:first[k + 1]].sum() for k in range(len(rpb))], dtype=LD)
            self.block_items[kind] = (rpb // ITEMS_PER_ROW[kind]).astype(np.int64)
            self.block_cols[kind] = N.block_columns(calibrator, self.L, kind, t_ns)
            rel = np.asarray(t_ns, dtype=np.int64) - int(tr.start_t_ns)          # first knots of the block's SO(3) / R^3 windows (CalcTimes)
            self.block_first_knot[kind] = (rel // int(tr.dt_so3_ns), rel // int(tr.dt_r3_ns))
        # the views that see a point: one of their corners refers to it (caller's order of the accepted views)
        acc_v = np.asarray(calibrator.views_accepted, dtype=bool)
        off = np.asarray(ds.corner_offset)
        self.view_points = [np.unique(np.asarray(ds.corner_point)[off[v]:off[v + 1]]) for v in np.flatnonzero(acc_v)]
        assert abs(float(sum(c.sum() for c in self.block_cost.values()) - self.cost)) <= 1e-15 * float(self.cost)

    def columns(self, kind, idx):
        """Tangent columns of block (kind, idx); None when the block is not a variable under the flags."""
        if kind in _KNOT_LAYOUT:
            o = np.asarray(self.L[_KNOT_LAYOUT[kind]], dtype=np.int64)
            return np.arange(o[idx], o[idx] + 3) if 0 <= idx < len(o) and o[idx] >= 0 else None
        if kind in _OTHER:
            e, n = _OTHER[kind]
            o = int(self.L["other"][e])
            return np.arange(o, o + n) if o >= 0 and idx == 0 else None
        if kind == IK_PT:
            return np.arange(self.pts[idx], self.pts[idx] + 3) if 0 <= idx < len(self.pts) and self.pts[idx] >= 0 else None
        return None

    def dependents(self, kind, idx):
        """{residual kind: boolean mask of the residual blocks that depend on block (kind, idx)}"""
        if kind == IK_PT:
            return {0: np.array([idx in p for p in self.view_points], dtype=bool), 1: np.zeros(len(self.block_cost[1]), bool), 2: np.zeros(len(self.block_cost[2]), bool)}
        cols = self.columns(kind, idx)
        return {k: np.isin(self.block_cols[k], cols).any(axis=1) if len(self.block_cols[k]) else np.zeros(0, bool) for k in (0, 1, 2)}

    def knots_read(self, kind, idx):
        """(first SO(3) knot, SO(3) knots, first R^3 knot, R^3 knots) the block's items read: the hull of their windows of SPLINE_N
        knots (gyroscope samples read no R^3 knot) -- what the kernels hold against kCapS / kCapR (csrc/inner_plan.h)."""
        dep = self.dependents(kind, idx)
        s = np.concatenate([self.block_first_knot[k][0][dep[k]] for k in (0, 1, 2)])
        r = np.concatenate([self.block_first_knot[k][1][dep[k]] for k in (0, 1)])
        return (int(s.min()), int(s.max() - s.min()) + E.SPLINE_N, int(r.min()) if len(r) else 0, int(r.max() - r.min()) + E.SPLINE_N if len(r) else 0)

    def block(self, kind, idx):
        cols = self.columns(kind, idx)
        assert cols is not None, (kind, idx)
        dep = self.dependents(kind, idx)
        cost = sum((self.block_cost[k][dep[k]].sum() for k in (0, 1, 2)), LD(0))
        items = int(sum(self.block_items[k][dep[k]].sum() for k in (0, 1, 2)))
        have_H = kind != IK_PT or self.has_point_H
        return cols, (self.H[np.ix_(cols, cols)] if have_H else None), (self.g[cols] if have_H else None), cost, items


def block_sums(calibrator, ds, flags, rows_backend=None, evaluate_backend=None):
    return BlockSums(calibrator, ds, flags, rows_backend, evaluate_backend)


def describe_block(layout, kind, idx, cols):
    """Name of a block through N.describe of its first column."""
    return N.describe(layout, int(cols[0])).rsplit(" [", 1)[0] if kind != IK_PT else "point %d" % idx


def compare(ref, info, sums, check_H=True):
    """Device rows (`DebugInnerFirstEvaluations`) against `ref` (BlockSums), every block on its own scale -- the scaling of
    N.entrywise_error / N.gradient_error: H entries by d_i d_j with d = sqrt(diag H_ref) (whole-problem matrix: the weak columns are
    those of the merged assembly tests), g entries by d_i sqrt(2 cost_b), cost_b relative.
    Returns dict(H=(err, block), g=(err, block), cost=(err, block)) with block = index into info of the worst block, and asserts the
    exact facts: zero tail behind NV, exact zeros where nothing contributes, cost exactly 0 where the reference's is."""
    P = ref.P
    Hd = np.zeros((P, P)); Hr = np.zeros((P, P), LD); gd = np.zeros(P); col_cost = np.zeros(P); owner = np.full(P, -1, np.int64)
    worst_c, worst_cb = 0.0, -1
    for b, (i8, row) in enumerate(zip(info, sums)):
        kind, idx, dim = int(i8[1]), int(i8[2]), int(i8[3])
        cols, H_ref, g_ref, cost_ref, _ = ref.block(kind, idx)
        assert len(cols) == dim, (b, kind, idx, dim)
        H, g, cost, tail = unpack(row, dim)
        assert not tail.any(), ("nonzero sums behind NV", b, kind, idx)
        assert (owner[cols] < 0).all(), ("two blocks on one column", b)
        owner[cols] = b
        if float(cost_ref) == 0.0:
            assert cost == 0.0, ("cost of a block without residuals", b, kind, idx, cost)
        else:
            e = abs(float(LD(cost) - cost_ref) / float(cost_ref))
            if e > worst_c:
                worst_c, worst_cb = e, b
        col_cost[cols] = float(cost_ref)
        if H_ref is None or not check_H:
            owner[cols] = -2 - b          # (no H / g reference: a point block without the Jets' Evaluate)
            continue
        Hd[np.ix_(cols, cols)] = H; Hr[np.ix_(cols, cols)] = H_ref; gd[cols] = g
        untouched = ~ref.touched[np.ix_(cols, cols)]
        assert not H[untouched].any(), ("nonzero entry where no item contributes", b, kind, idx)
    have = owner >= 0
    sel = np.flatnonzero(have)
    kinds = ref.kinds[sel]
    eh, (i, j) = N.entrywise_error(Hd[np.ix_(sel, sel)], Hr[np.ix_(sel, sel)], kinds)
    # g_b: |g_i - gref_i| / (d_i sqrt(2 cost_b)), the zero and weak columns as N.gradient_error treats them
    Hr_s = Hr[np.ix_(sel, sel)]
    d = np.sqrt(np.abs(np.diag(Hr_s)).astype(np.float64)); weak = N.weak_columns(Hr_s, kinds); zero = d == 0
    diff = np.abs(gd[sel] - ref.g[sel]).astype(np.float64)
    assert not gd[sel][zero].any(), "nonzero gradient entries in columns whose Jacobian column is exactly zero"
    if weak.any():
        assert diff[weak].max() <= 1e-10 * float(np.abs(ref.g[sel]).max())
    ok = ~(zero | weak)
    ratio = np.where(ok, diff / np.where(ok, d * np.sqrt(2.0 * col_cost[sel]), 1.0), 0.0)
    k = int(ratio.argmax()) if len(ratio) else 0
    return dict(H=(eh, int(owner[sel[i]]) if len(sel) else -1, int(sel[i]) if len(sel) else -1, int(sel[j]) if len(sel) else -1),
                g=(float(ratio[k]) if len(ratio) else 0.0, int(owner[sel[k]]) if len(sel) else -1, int(sel[k]) if len(sel) else -1),
                cost=(worst_c, worst_cb))
