"""Host reference of the normal equations J^T J, J^T r and the cost, summed block by block in extended precision.

The Jacobian pass of the library sums J_k^T J_k over every residual block k (time tiles, LDS ring accumulators, chains, slab merge,
the arrow corner by atomics).  `assemble` does that sum with nothing but public information: the residuals and block-local Jacobian
rows of `EvaluateBlocks` (any estimator: the oracle's or the device's own), the tangent layout of `GetTangentLayout`, and the knot
window of a block from its integer time, `(t_ns - start_ns) // dt_ns` (CalcTimes; six knots, three for the bias splines with their
own spacing).  Block-local column order as documented at oicc_evaluate_blocks (include/oicc_hip.h):
    view  43 = 6 SO(3) knots x 3 | 6 R^3 knots x 3 | T_i_c 6 | line delay 1
    accel 54 = 18 | 18 | gravity 3 | accelerometer-bias knots 3 x 3 | accelerometer intrinsics 6
    gyro  36 = 18 | gyroscope-bias knots 3 x 3 | gyroscope intrinsics 9
Every sum runs in np.longdouble (x86 80-bit: eps 1.08e-19), so the reference's own rounding is 3 to 4 orders below that of any
float64 summation order; `entrywise_error` / `gradient_error` then scale every entry by its OWN size (d_i d_j, d = sqrt(diag H)),
not by the largest entry of the matrix -- the entries of J^T J span more than ten orders of magnitude.

Dense form: all P columns (tiny ... C3, P up to a few thousand).  Slice form (`select`): a subset of the columns (a time slice of
the band plus the arrow) for problems whose dense matrix does not fit (C4, C5); entries whose two columns are both selected are
complete, and the arrow corner needs no band column at all.

Yardsticks (tests/test_normal_equations_reference.py: float64 assembly of the oracle's rows, block order shuffled, three seeds,
against the long-double one, entry-wise): see YARDSTICK below.
"""
import numpy as np

from openimucameracalibrator_amd import estimator as E

LD = np.longdouble
# x86 80-bit extended precision on every machine the suite runs on: a silent loss of it would make the reference a float64 sum
assert np.finfo(LD).eps <= 1.1e-19, "np.longdouble is not 80-bit extended precision here"

NCOLS = {0: 43, 1: 54, 2: 36}
BIAS_DT_NS = 10 * 10**9          # ImuCameraCalibrator.BatchInitSpline: InitBiasSplines(..., 10 s, 10 s, ...)
FLAGS1 = E.SPLINE | E.T_I_C | E.GRAVITY_DIR
ALL = FLAGS1 | E.CAM_LINE_DELAY | E.IMU_BIASES | E.IMU_INTRINSICS

# Entry-wise error (H and g) of a float64 sum of the oracle's rows against the long-double sum, per configuration: blocks in a
# shuffled order, the largest of three seeds over every shape and flag set of the configuration, rounded up to one digit.
# Measured by test_float64_assembly_yardstick* (which assert that a fresh measurement lies within [1/8, 1] of the figure):
#   tiny 1.3e-15 (9 shapes x 6 flag sets), C1 1.6e-15, C2 1.5e-15, C3 1.8e-15;
#   slice form (three time slices + arrow; the arrow corner is one long sequential sum there): C4 5.4e-15 ... 6.5e-15, C5 2.4e-15.
# The device comparison (a) allows DEVICE_FACTOR x this.
YARDSTICK = {"tiny": 2e-15, "C1": 2e-15, "C2": 2e-15, "C3": 2e-15, "C4": 7e-15, "C5": 3e-15}
DEVICE_FACTOR = 64


def _knot_columns(offsets, first, n):
    """[nb, 3 n] tangent columns of n consecutive knots from `first` (per block); -1 where the knot is not a variable."""
    offsets = np.asarray(offsets, dtype=np.int64)
    if len(offsets) == 0:
        return np.full((len(first), 3 * n), -1, np.int64)
    idx = first[:, None] + np.arange(n)[None, :]
    inside = (idx >= 0) & (idx < len(offsets))
    o = np.where(inside, offsets[np.clip(idx, 0, len(offsets) - 1)], -1)
    c = o[:, :, None] + np.arange(3)[None, None, :]
    c[o < 0] = -1
    return c.reshape(len(first), 3 * n)


def _fixed_columns(offset, n, nb):
    c = (int(offset) + np.arange(n)) if offset >= 0 else np.full(n, -1)
    return np.broadcast_to(c.astype(np.int64), (nb, n))


def block_times(calibrator, ds, shard=None):
    """Integer times (ns) of the accepted blocks in the caller's order, per kind, and the residual rows of every block."""
    if shard is not None:
        d = ds.shard(*shard)
        vt, off = d.shard_view_t_s, np.asarray(d.shard_corner_offset)
    else:
        vt, off = ds.view_t_s, np.asarray(ds.corner_offset)
    t_views = (np.asarray(vt) * E.S_TO_NS).astype(np.int64)          # as BatchInitSpline converts them
    acc_v = np.asarray(calibrator.views_accepted, dtype=bool)
    t_imu = np.asarray(calibrator.imu_t_ns, dtype=np.int64)
    ta = t_imu[np.asarray(calibrator.accl_accepted, dtype=bool)]
    tg = t_imu[np.asarray(calibrator.gyro_accepted, dtype=bool)]
    return {0: (t_views[acc_v], 2 * np.diff(off)[acc_v].astype(np.int64)),
            1: (ta, np.full(len(ta), 3, np.int64)), 2: (tg, np.full(len(tg), 3, np.int64))}


def block_columns(calibrator, layout, kind, t_ns, bias_dt_ns=(BIAS_DT_NS, BIAS_DT_NS)):
    """[nb, NCOLS[kind]] tangent column of every block-local column (-1: not a variable)."""
    tr = calibrator.trajectory_
    rel = np.asarray(t_ns, dtype=np.int64) - int(tr.start_t_ns)
    s_so3, s_r3 = rel // int(tr.dt_so3_ns), rel // int(tr.dt_r3_ns)
    nb, oth = len(rel), layout["other"]          # other: T_i_c, gravity, line delay, accl intrinsics, gyro intrinsics
    so3 = _knot_columns(layout["so3"], s_so3, E.SPLINE_N)
    if kind == 0:
        parts = [so3, _knot_columns(layout["r3"], s_r3, E.SPLINE_N), _fixed_columns(oth[0], 6, nb), _fixed_columns(oth[2], 1, nb)]
    elif kind == 1:
        parts = [so3, _knot_columns(layout["r3"], s_r3, E.SPLINE_N), _fixed_columns(oth[1], 3, nb),
                 _knot_columns(layout["accl_bias"], rel // int(bias_dt_ns[0]), E.BIAS_SPLINE_N), _fixed_columns(oth[3], 6, nb)]
    else:
        parts = [so3, _knot_columns(layout["gyro_bias"], rel // int(bias_dt_ns[1]), E.BIAS_SPLINE_N), _fixed_columns(oth[4], 9, nb)]
    cols = np.concatenate(parts, axis=1)
    assert cols.shape == (nb, NCOLS[kind])
    return cols


def assemble(calibrator, ds, flags, rows_backend=None, dtype=LD, select=None, shard=None, shuffle_seed=None,
             bias_dt_ns=(BIAS_DT_NS, BIAS_DT_NS), want_touched=False, chunk_rows=1 << 16):
    """cost, H, g (and the boolean matrix of entries some block contributes to): sum of J_k^T J_k, J_k^T r_k, r_k.r_k / 2 over the
    blocks of `rows_backend` (a calibrator built from the same data set; default: `calibrator`) in `dtype`.
    select: global tangent columns to keep, in the order of the result (None: all P); the cost is always the whole problem's.
    shuffle_seed: sum the blocks in a random order (the float64 yardstick)."""
    rows_backend = calibrator if rows_backend is None else rows_backend
    L = calibrator.trajectory_.GetTangentLayout(flags)
    P = L["P"]
    if select is None:
        local = np.arange(P, dtype=np.int64)
        n = P
    else:
        select = np.asarray(select, dtype=np.int64)
        assert len(np.unique(select)) == len(select) and select.min() >= 0 and select.max() < P
        local = np.full(P, -1, np.int64); local[select] = np.arange(len(select))
        n = len(select)
    H = np.zeros((n, n), dtype); g = np.zeros(n, dtype); cost = dtype(0)
    touched = np.zeros((n, n), bool) if want_touched else None
    rng = np.random.default_rng(shuffle_seed) if shuffle_seed is not None else None
    times = block_times(calibrator, ds, shard)
    for kind in (0, 1, 2):
        t_ns, rpb = times[kind]
        nrows = int(rpb.sum())
        # (the view dump is sized by every corner handed in; rows behind the accepted ones stay zero)
        n_dump = 2 * int(rows_backend.num_corners) if kind == 0 else nrows
        r, J = rows_backend.trajectory_.EvaluateBlocks(flags, kind, n_dump)
        assert not r[nrows:].any() and not J[nrows:].any(), "rows of rejected measurements must contribute nothing"
        r, J = r[:nrows], J[:nrows]
        if nrows == 0:
            continue
        cols = block_columns(calibrator, L, kind, t_ns, bias_dt_ns)
        blk_of_row = np.repeat(np.arange(len(t_ns)), rpb)
        for a in range(0, nrows, chunk_rows):      # columns mapped to "inactive" are exactly zero in the rows
            sl = slice(a, a + chunk_rows)
            assert not J[sl][cols[blk_of_row[sl]] < 0].any(), "nonzero Jacobian entry in an inactive column (kind %d)" % kind
        cols = np.concatenate([local, [-1]])[cols]          # (-1 indexes the appended -1)
        rl = r.astype(dtype)
        cost = cost + rl @ rl / 2
        # blocks with the same columns form one group: one Gram product per group
        uniq, inv = np.unique(cols, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        row_group = inv[blk_of_row]
        perm = rng.permutation(nrows) if rng is not None else np.arange(nrows)
        perm = perm[np.argsort(row_group[perm], kind="stable")]
        bounds = np.concatenate([[0], np.cumsum(np.bincount(row_group, minlength=len(uniq)))])
        for gi in (rng.permutation(len(uniq)) if rng is not None else range(len(uniq))):
            act = uniq[gi] >= 0
            if not act.any():
                continue
            idx = uniq[gi][act]
            rows = perm[bounds[gi]:bounds[gi + 1]]
            for a in range(0, len(rows), chunk_rows):
                rr = rows[a:a + chunk_rows]
                Jm = J[rr][:, act].astype(dtype)
                # (einsum, not BLAS: the float64 yardstick must not depend on a thread count)
                H[np.ix_(idx, idx)] += np.einsum("ri,rj->ij", Jm, Jm)
                g[idx] += np.einsum("ri,r->i", Jm, rl[rr])
            if touched is not None:
                touched[np.ix_(idx, idx)] = True
    return (cost, H, g, touched) if want_touched else (cost, H, g)


def column_kinds(layout, P=None):
    """Kind of every tangent column: 0 SO(3) knots, 1 R^3 knots, 2 accelerometer-bias knots, 3 gyroscope-bias knots,
    4 ... 8 T_i_c, gravity, line delay, accelerometer intrinsics, gyroscope intrinsics, 9 everything behind (board points)."""
    P = layout["P"] if P is None else P
    kinds = np.full(P, 9, np.int64)
    for k, name in enumerate(("so3", "r3", "accl_bias", "gyro_bias")):
        o = np.asarray(layout[name], dtype=np.int64); o = o[o >= 0]
        for c in range(3):
            kinds[o + c] = k
    for k, (o, n) in enumerate(zip(layout["other"], (6, 3, 1, 6, 9))):
        if o >= 0:
            kinds[o:o + n] = 4 + k
    return kinds


MAX_WEAK_COLUMNS = 6


def weak_from_diagonal(diag, kinds):
    """Columns whose reference diagonal is below 1e-24 x the median diagonal of their kind (the last knot of a spline can hold
    rounding noise only): decided from the reference alone, at most MAX_WEAK_COLUMNS per problem."""
    d = np.asarray(diag).astype(np.float64)
    weak = np.zeros(len(d), bool)
    for k in np.unique(kinds):
        m = kinds == k
        pos = d[m][d[m] > 0]
        if len(pos):
            weak[m] = (d[m] > 0) & (d[m] < 1e-24 * np.median(pos))
    assert weak.sum() <= MAX_WEAK_COLUMNS, "%d weak columns" % weak.sum()
    return weak


def weak_columns(H_ref, kinds):
    return weak_from_diagonal(np.diag(H_ref), kinds)


def _scales(H_ref, kinds):
    d = np.sqrt(np.abs(np.diag(H_ref)).astype(np.float64))
    weak = weak_columns(H_ref, kinds) if kinds is not None else np.zeros(len(d), bool)
    return d, weak


def entrywise_error(H, H_ref, kinds=None):
    """max |H_ij - Href_ij| / (d_i d_j), d = sqrt(diag Href), and its (i, j).  Columns with a zero reference diagonal have a zero
    Jacobian column (every entry of their row is exactly 0): H must be exactly 0 there.  Weak columns (`weak_columns`, when
    `kinds` is given) stay out of the ratio; their entries must be below 1e-10 max|Href| in absolute terms."""
    H = np.asarray(H)
    assert H.shape == H_ref.shape
    d, weak = _scales(H_ref, kinds)
    diff = np.abs(H - H_ref).astype(np.float64)
    zero = d == 0
    if zero.any():
        assert not np.asarray(H_ref)[zero].any()
        assert not H[zero].any() and not H[:, zero].any(), "nonzero entries in columns whose Jacobian column is exactly zero"
    if weak.any():
        bound = 1e-10 * float(np.abs(H_ref).max())
        assert diff[weak].max() <= bound and diff[:, weak].max() <= bound, "weak columns: %g > %g" % (max(diff[weak].max(), diff[:, weak].max()), bound)
    ok = ~(zero | weak)
    if not ok.any():
        return 0.0, (0, 0)
    ratio = diff[np.ix_(ok, ok)] / np.outer(d[ok], d[ok])
    k = np.unravel_index(int(ratio.argmax()), ratio.shape)
    where = np.flatnonzero(ok)
    return float(ratio[k]), (int(where[k[0]]), int(where[k[1]]))


def gradient_error(g, g_ref, H_ref, cost, kinds=None):
    """max |g_i - gref_i| / (d_i sqrt(2 cost)) and its i (|g_i| <= d_i sqrt(2 cost) by Cauchy-Schwarz: the scale of entry i)."""
    d, weak = _scales(H_ref, kinds)
    diff = np.abs(np.asarray(g) - g_ref).astype(np.float64)
    zero = d == 0
    if zero.any():
        assert not np.asarray(g)[zero].any(), "nonzero gradient entries in columns whose Jacobian column is exactly zero"
    if weak.any():
        assert diff[weak].max() <= 1e-10 * float(np.abs(g_ref).max())
    ok = ~(zero | weak)
    if not ok.any():
        return 0.0, 0
    ratio = diff[ok] / (d[ok] * np.sqrt(2.0 * float(cost)))
    k = int(ratio.argmax())
    return float(ratio[k]), int(np.flatnonzero(ok)[k])


def pattern(H_ref, touched=None):
    """Boolean matrix of the entries (i, j) no block contributes to: from the column tables (`touched` of
    assemble(..., want_touched=True)), else the entries whose long-double sum is exactly zero."""
    return ~touched if touched is not None else (np.asarray(H_ref) == 0)


def symmetry_error(H, H_ref):
    """max |H_ij - H_ji| / (d_i d_j) over the columns with a nonzero reference diagonal."""
    d = np.sqrt(np.abs(np.diag(H_ref)).astype(np.float64))
    ok = d > 0
    a = np.abs(H - H.T)[np.ix_(ok, ok)] / np.outer(d[ok], d[ok])
    return float(a.max()) if a.size else 0.0


def describe(layout, i):
    """Name of tangent column i through the layout (what a failing entry is reported with)."""
    names = ("so3", "r3", "accl_bias", "gyro_bias")
    for name in names:
        o = np.asarray(layout[name], dtype=np.int64)
        k = np.flatnonzero((o >= 0) & (o <= i) & (i < o + 3))
        if len(k):
            return "%s knot %d [%d]" % (name, int(k[0]), i - int(o[k[0]]))
    for name, o, n in zip(("T_i_c", "gravity", "line_delay", "accl_intrinsics", "gyro_intrinsics"), layout["other"], (6, 3, 1, 6, 9)):
        if o >= 0 and o <= i < o + n:
            return "%s [%d]" % (name, i - o)
    return "column %d (point)" % i


def old_rel_err(a, b):
    """The global-scale error the earlier tests use: max|a - b| / max|b|."""
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max() / max(float(np.abs(b).max()), 1e-300))
