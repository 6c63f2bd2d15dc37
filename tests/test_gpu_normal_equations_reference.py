"""GPU: J^T J, J^T r and the cost of the device's Jacobian + assembly pass, entry by entry.

Two comparisons per case (tests/normal_equations_reference.py; every entry on its own scale d_i d_j, d = sqrt(diag H)):
 (a) assembly alone: device Evaluate against the long-double sum of the DEVICE'S OWN EvaluateBlocks rows -- no Jacobian formula is
     involved, only the summation (tiles, LDS ring accumulators, chains, slab merge, atomics of the arrow corner) and the tile
     kernel's own evaluation of the rows.  Bound: 64 x the float64 yardstick of the configuration (YARDSTICK), cost included.
 (b) against the Jet oracle (analytic_jacobians = 0): H 1e-10, g 1e-10 entry-wise, cost 1e-11 relative.  With POINTS the only
     comparison of the point columns (the block dump has none); (a) then covers the other columns.
 pattern: H is exactly 0.0 wherever no block contributes and symmetric to 1e-13 d_i d_j.
Every check prints its measured margins (run with -s); DESIGN.md section 6 holds the table.
"""
import numpy as np
import pytest

import oracle_backend
import normal_equations_reference as N
import normal_equations_cases as cases
from openimucameracalibrator_amd import synthetic, estimator as E

pytestmark = pytest.mark.gpu

FLAGS1, ALL = cases.FLAGS1, cases.ALL
WHOLE = 100000          # chain_tiles: one chain for the whole problem
POINT_CASES = [("tiny", FLAGS1 | E.POINTS), ("tiny", E.T_I_C | E.POINTS), ("tiny", FLAGS1 | E.CAM_LINE_DELAY | E.IMU_BIASES | E.POINTS),
               ("C1", FLAGS1 | E.POINTS)]          # POINT_CASES of tests/test_gpu_parity.py

# assembly routes: options of the tile pass (include/oicc_hip.h)
ROUTES_TINY = ([{"assembly": 0, "tile_windows": tw, "wide_cells": w} for tw in (0, 1, 3, 7, 64) for w in (1, 0)]
               + [{"assembly": 2, "wide_cells": w} for w in (1, 0)]
               + [{"chain_tiles": c, "tile_windows": 1} for c in (1, 3, 25, WHOLE)]
               + [{"accumulation": 1}, {"debug_no_direct_rows": 1}, {"debug_poison_lds": 1}, {"debug_poison_lds": 1, "chain_tiles": 3, "tile_windows": 2}])
ROUTES_FULL = [{}, {"chain_tiles": 1}, {"chain_tiles": 3}, {"chain_tiles": 25}, {"chain_tiles": WHOLE}, {"assembly": 2}, {"accumulation": 1},
               {"debug_no_direct_rows": 1}, {"debug_poison_lds": 1, "tile_windows": 7}, {"wide_cells": 0, "tile_windows": 3}]


def make(ds, options=None, backend=None, jets=False, **kw):
    c = E.ImuCameraCalibrator(backend=backend).BatchInitSpline(ds, **kw)
    for k, v in (options or {}).items():
        c.trajectory_.SetOption(k, v)
    if jets:
        c.trajectory_.SetOption("analytic_jacobians", 0)
    return c


class Reference:
    """What one (data set, flags) is compared with: (a) the long-double sum of the device's own rows, (b) the Jet oracle."""

    def __init__(self, cfg, ds, flags, rows_from, oracle):
        self.cfg, self.flags = cfg, flags
        self.L = rows_from.trajectory_.GetTangentLayout(flags)
        self.kinds = N.column_kinds(self.L)
        self.cl, self.Hl, self.gl, touched = N.assemble(rows_from, ds, flags, want_touched=True)
        self.pattern = N.pattern(self.Hl, touched)
        self.cj, self.Hj, self.gj = oracle.trajectory_.Evaluate(flags)
        pts = rows_from.trajectory_.GetScenePointOffsets(flags) if flags & E.POINTS else np.array([-1])
        self.n_a = int(pts[pts >= 0].min()) if (pts >= 0).any() else self.L["P"]          # columns the block dump covers
        self.bound = N.DEVICE_FACTOR * N.YARDSTICK[cfg]


def check(ref, cg, Hg, gg, label):
    L, n = ref.L, ref.n_a
    name = lambda i: N.describe(L, i)
    # (a) the assembly alone
    ka = ref.kinds[:n]
    ah, (i, j) = N.entrywise_error(Hg[:n, :n], ref.Hl[:n, :n], ka)
    ag, k = N.gradient_error(gg[:n], ref.gl[:n], ref.Hl[:n, :n], ref.cl, ka)
    ac = abs(cg - float(ref.cl)) / float(ref.cl)
    # (b) against the Jets
    bh, (i2, j2) = N.entrywise_error(Hg, ref.Hj, ref.kinds)
    bg, k2 = N.gradient_error(gg, ref.gj, ref.Hj, ref.cj, ref.kinds)
    bc = abs(cg - ref.cj) / ref.cj
    sym = N.symmetry_error(Hg, ref.Hj)
    print("MARGIN %-34s (a) H %.2e g %.2e cost %.1e of %.1e | (b) H %.2e g %.2e cost %.1e | symmetry %.1e" % (label, ah, ag, ac, ref.bound, bh, bg, bc, sym))
    assert ah <= ref.bound, (label, "(a) H", ah, name(i), name(j))
    assert ag <= ref.bound, (label, "(a) g", ag, name(k))
    assert ac <= ref.bound, (label, "(a) cost", ac)
    assert bh <= 1e-10, (label, "(b) H", bh, name(i2), name(j2))
    assert bg <= 1e-10, (label, "(b) g", bg, name(k2))
    assert bc <= 1e-11, (label, "(b) cost", bc)
    bad = np.argwhere(ref.pattern[:n, :n] & (Hg[:n, :n] != 0))
    assert len(bad) == 0, (label, "nonzero where no block contributes", [(name(a), name(b)) for a, b in bad[:4]])
    if n < L["P"]:          # the point columns: zero where the Jets' sum is exactly zero (no view sees the point from that window)
        assert not Hg[(ref.Hj == 0) & (np.arange(L["P"])[:, None] >= n)].any(), label
    assert sym <= 1e-13, (label, "symmetry", sym)


def run_case(shape, flag_sets, routes, problem_options=None):
    cfg, build, options = cases.SHAPES[shape]
    options = dict(options); options.update(problem_options or {})
    ds = build()
    first = make(ds, options)
    oracle = make(ds, options, backend=oracle_backend.load(), jets=True)
    for fname, flags in flag_sets:
        if first.trajectory_.GetTangentLayout(flags)["P"] == 0:          # (global-shutter views have no line-delay block: nothing to compare)
            continue
        ref = Reference(cfg, ds, flags, first, oracle)
        for route in routes:
            gpu = first if not route else make(ds, {**options, **route})
            tag = ",".join("%s=%g" % kv for kv in route.items()) or "default"
            check(ref, *gpu.trajectory_.Evaluate(flags), "%s %s %s" % (shape, fname, tag))
            cc = gpu.trajectory_.EvaluateCost(flags)
            assert abs(cc - float(ref.cl)) <= ref.bound * float(ref.cl) and abs(cc - ref.cj) <= 1e-11 * ref.cj


@pytest.mark.parametrize("shape", [s for s in cases.SHAPES if s not in ("C2", "C3")])
def test_every_flag_set_on_every_shape(shape):
    run_case(shape, cases.FLAG_SETS, [{}])


@pytest.mark.parametrize("shape", ["tiny", "ragged", "gap"])
def test_assembly_routes_small(shape):
    run_case(shape, [cases.FLAG_SETS[0], cases.FLAG_SETS[4]], ROUTES_TINY)


@pytest.mark.parametrize("shape", ["C1", "C2", "C3"])
def test_assembly_routes_full_size(shape):
    run_case(shape, [cases.FLAG_SETS[0], cases.FLAG_SETS[4]], ROUTES_FULL)


@pytest.mark.parametrize("cfg,flags", POINT_CASES)
def test_points_flag(cfg, flags):
    run_case(cfg, [("POINTS|%d" % flags, flags)], [{}, {"assembly": 2}])


@pytest.mark.parametrize("cfg,flag_names", [("C4", ("FLAGS1", "ALL")), ("C5", ("FLAGS1", "ALL"))])
def test_time_slices_of_the_large_configurations(cfg, flag_names):
    """C4 / C5 (P = 6 k / 90 k) through EvaluateEntries: three time slices of 400 band columns -- the first windows, the middle of
    the trajectory, the last windows -- with EVERY entry among their columns (inside the band, and the zeros outside it), every
    arrow entry of those columns and the whole arrow corner.  A fine knot window holds 4.5 band columns (one SO(3) knot, half an R^3
    knot), so the default route at C5 (tiles of 10 windows, 8 per chain: 360 columns) puts a chain boundary into every slice; the
    second route, tiles of 8 windows in chains of 4 (144 columns), puts two or more into each at either size."""
    ds = synthetic.make_config(cfg)
    routes = [{}, {"tile_windows": 8, "chain_tiles": 4}]
    gpus = [make(ds, r) for r in routes]
    oracle = make(ds, backend=oracle_backend.load(), jets=True)
    for fname, flags in [fs for fs in cases.FLAG_SETS if fs[0] in flag_names]:
        L = gpus[0].trajectory_.GetTangentLayout(flags)
        Pb = 3 * int((L["so3"] >= 0).sum() + (L["r3"] >= 0).sum())
        sel = cases.time_slices(Pb, L["P"])
        kinds = N.column_kinds(L)[sel]
        rows, cols = [a.ravel() for a in np.meshgrid(sel, sel, indexing="ij")]
        cl, Hl, gl, touched = N.assemble(gpus[0], ds, flags, select=sel, want_touched=True)
        Hj = oracle.trajectory_.EvaluateEntries(flags, rows, cols).reshape(len(sel), len(sel))
        cj, _, gj = oracle.trajectory_.Evaluate(flags, want_H=False)
        bound = N.DEVICE_FACTOR * N.YARDSTICK[cfg]
        for route, gpu in zip(routes, gpus):
            label = "%s %s slices %s" % (cfg, fname, ",".join("%s=%g" % kv for kv in route.items()) or "default")
            Hg = gpu.trajectory_.EvaluateEntries(flags, rows, cols).reshape(len(sel), len(sel))
            cg, _, gg = gpu.trajectory_.Evaluate(flags, want_H=False)
            gg = gg[sel]
            ah, ija = N.entrywise_error(Hg, Hl, kinds); ag, _ = N.gradient_error(gg, gl, Hl, cl, kinds); ac = abs(cg - float(cl)) / float(cl)
            bh, ijb = N.entrywise_error(Hg, Hj, kinds); bg, _ = N.gradient_error(gg, gj[sel], Hj, cj, kinds); bc = abs(cg - cj) / cj
            sym = N.symmetry_error(Hg, Hj)
            print("MARGIN %-34s (a) H %.2e g %.2e cost %.1e of %.1e | (b) H %.2e g %.2e cost %.1e | symmetry %.1e" % (label, ah, ag, ac, bound, bh, bg, bc, sym))
            assert ah <= bound and ag <= bound and ac <= bound, (label, ah, ag, ac, [N.describe(L, sel[i]) for i in ija])
            assert bh <= 1e-10 and bg <= 1e-10 and bc <= 1e-11, (label, bh, bg, bc, [N.describe(L, sel[i]) for i in ijb])
            assert not Hg[N.pattern(Hl, touched)].any() and sym <= 1e-13, (label, sym)


@pytest.mark.parametrize("ranks", [2, 4])
def test_time_shards_sum_to_the_whole_entry_by_entry(ranks):
    """C2 in time shards built as rank r of `ranks` would (one process, each rank's problem in turn, remote measurements declared):
    the SUM of the ranks' H, g and cost against the whole problem's references; and every rank against the long-double sum of its
    own rows (its halo rows at the shard ends included)."""
    ds = synthetic.make_config("C2")
    whole = make(ds)
    oracle = make(ds, backend=oracle_backend.load(), jets=True)
    for fname, flags in (cases.FLAG_SETS[0], cases.FLAG_SETS[4]):
        ref = Reference("C2", ds, flags, whole, oracle)
        c_sum, H_sum, g_sum = 0.0, 0.0, 0.0
        for r in range(ranks):
            part = make(ds, shard=(r, ranks))
            c, H, g = part.trajectory_.Evaluate(flags)
            assert H.shape == ref.Hl.shape
            cl, Hl, gl, touched = N.assemble(part, ds, flags, shard=(r, ranks), want_touched=True)
            # (scales of the WHOLE problem: a rank's own diagonal is tiny in columns it only grazes)
            eh = (np.abs(H - Hl).astype(np.float64) / np.maximum(np.outer(*(2 * [np.sqrt(np.diag(ref.Hl).astype(np.float64))])), 1e-300))
            weak = N.weak_columns(ref.Hl, ref.kinds)
            eh[weak] = 0; eh[:, weak] = 0
            print("MARGIN C2 %s rank %d of %d          (a) H %.2e cost %.1e of %.1e" % (fname, r, ranks, eh.max(), abs(c - float(cl)) / float(cl), ref.bound))
            assert eh.max() <= ref.bound and abs(c - float(cl)) <= ref.bound * float(cl)
            assert not H[N.pattern(Hl, touched)].any()
            c_sum += c; H_sum = H_sum + H; g_sum = g_sum + g
        check(ref, c_sum, H_sum, g_sum, "C2 %s sum of %d shards" % (fname, ranks))
