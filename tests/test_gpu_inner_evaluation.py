"""GPU: what the inner sweeps sum for every block at its first evaluation, entry by entry, and the small Cholesky solve of their LM loops.

`DebugInnerFirstEvaluations` (oicc_debug_inner_first_evaluations) runs the launches of a sweep on a scratch copy of the parameters with
every block's loop ending right behind its first evaluation, and returns per block `tot` = [upper triangle of H_b | g_b | cost_b] and
the code that summed it (route 0 / 1 / 2: inner_set_kernel<0 / 1 / 2> with one workgroup, 3: inner_wave_kernel, 4: a shared block on
resident workgroups with atomics, 5: a shared block by (evaluation, advance) launches).  tests/inner_evaluation_reference.py says what
these sums are: the diagonal block / segment of the whole problem's J^T J / J^T r, and the cost of the residual blocks that depend on
the block.  Per case, every block on its own scale (d_i d_j, d = sqrt(diag H_ref); g: d_i sqrt(2 cost_b); cost_b relative):
 (b) against the Jet oracle (analytic_jacobians = 0): H 1e-10, g 1e-10, cost 1e-11 -- the project's bounds for Evaluate.
 (a) against the long-double sum of the device's own EvaluateBlocks rows (the tile pass: another evaluation of the same rows, another
     formula for the SO(3) segment): BOUND_A, measured -- see the table below.
 exact: zeros behind NV, zeros where no item contributes, a zero cost where no residual depends; two calls in a row bit-identical
 (routes 0, 1, 2, 3, 5; route 4 sums by fp64 atomics in the order the workgroups arrive and is exempt).
Every case prints a MARGIN line (run with -s).

MEASURED (a) / (b) margins and the solve's backward errors: DESIGN.md section 6 ("Inner sweeps, entry by entry").
Measured on an MI355X (largest over the blocks of the case; H / g / cost):
  case                                             routes      (a)                          (b)
  tiny FLAGS1 / ALL / line delay alone             0 1 / 0     2.9e-16 / 1.9e-16 / 2.2e-16  4.3e-15 / 2.2e-15 / 5.3e-15
  tiny, debug_inner_general_kernel                 0           2.9e-16 / 1.9e-16 / 2.2e-16  4.3e-15 / 2.2e-15 / 5.3e-15
  tiny FLAGS1 (| IMU_BIASES), inner_wave_blocks 1  0 3         2.9e-16 / 1.9e-16 / 2.2e-16  4.5e-15 / 2.1e-15 / 5.3e-15
  tiny FLAGS1 | POINTS, T_I_C | POINTS             1 2 / 2     2.5e-16 / 1.9e-16 / 2.2e-16  9.5e-15 / 2.2e-15 / 5.4e-15
  gs_views / gs_views_unit_loss                    0 1         1.7e-15 / 5.7e-16 / 9.9e-16  7.5e-15 / 6.7e-15 / 1.4e-14
  knot_spacing_56_128, short_0.3s                  0 1         4.3e-16 / 8.2e-16 / 8.5e-16  1.3e-14 / 1.2e-14 / 7.8e-15
  knot_spacing_200_17 (default, wave)              0 1 / 0 3   6.4e-16 / 4.7e-16 / 2.0e-15  2.0e-14 / 2.3e-14 / 2.5e-14
  gap under LDS poison                             0 1         2.3e-16 / 1.2e-16 / 1.0e-15  2.5e-14 / 1.9e-14 / 6.4e-15
  ragged FLAGS1 | line delay                       0 1         2.7e-16 / 1.5e-16 / 1.7e-15  1.3e-14 / 1.5e-14 / 1.4e-14
  C1 FLAGS1 / ALL, shared blocks on routes 4 and 5 0 1 4 5     2.3e-16 / 1.7e-16 / 1.0e-15  8.0e-15 / 4.7e-15 / 6.4e-15
  C1 FLAGS1 | POINTS                               1 2 4       2.5e-16 / 1.7e-16 / 1.0e-15  8.0e-15 / 4.7e-15 / 6.4e-15
Largest (a) figure 2.0e-15 (cost of SO(3) knot 0 at knot_spacing_200_17, route 0), far below the 1e-12 that would have asked for an
explanation: the sweeps' own evaluation of an item and the tile pass's agree to a few ulp.  BOUND_A = 8 x 2.0e-15 rounded up = 2e-14.
The same block by a wave and by a workgroup: 2.5e-16 (bound 1e-13); the shared blocks of C1 on routes 4 and 5: 2.4e-16.
"""
import numpy as np
import pytest

import oracle_backend
import normal_equations_reference as N
import normal_equations_cases as cases
import inner_evaluation_reference as R
from openimucameracalibrator_amd import _abi, _lib, estimator as E

pytestmark = pytest.mark.gpu

FLAGS1, ALL = cases.FLAGS1, cases.ALL
BOUND_A = 2e-14          # 8 x the largest measured (a) figure (2.0e-15: the table above), rounded up to one digit
KCAP_R = 16              # csrc/inner_plan.h: R^3 knots of a neighbourhood that fit the LDS copy
SHARED_ABOVE = 1024      # item slots above which a block is shared by several workgroups (oicc_inner.hip: kSharedAbove)

_data, _oracle, _ref_b = {}, {}, {}          # references are computed once per (shape, flags) and shared by the cases; nothing changes them


def _make(ds, options, backend=None, jets=False):
    c = E.ImuCameraCalibrator(backend=backend).BatchInitSpline(ds)
    for k, v in options.items():
        c.trajectory_.SetOption(k, v)
    if jets:
        c.trajectory_.SetOption("analytic_jacobians", 0)
    return c


def _shape(shape):
    if shape not in _data:
        _, build, options = cases.SHAPES[shape]
        _data[shape] = (build(), dict(options))
    return _data[shape]


def _jets(shape, flags):
    ds, options = _shape(shape)
    if shape not in _oracle:
        _oracle[shape] = _make(ds, options, backend=oracle_backend.load(), jets=True)
    if (shape, flags) not in _ref_b:
        o = _oracle[shape]
        weight = ds.line_delay_init != 0.0 or bool(options.get("gs_unit_loss"))          # global-shutter views carry HuberLoss(0) (quirk Q2): the Jet dump holds their rows before the loss
        _ref_b[(shape, flags)] = R.block_sums(o, ds, flags, rows_backend=R.RowsAfterLoss(o, weight), evaluate_backend=o)
    return _ref_b[(shape, flags)]


def _name(ref, info, b):
    if b < 0:
        return "-"
    kind, idx = int(info[b, 1]), int(info[b, 2])
    return "%s (set %d, route %d: %s, %d parts)" % (R.describe_block(ref.L, kind, idx, ref.columns(kind, idx)), info[b, 0], info[b, 6], _abi.INNER_ROUTES[info[b, 6]], info[b, 7])


def run_case(shape, flags, options=None, need=(), forbid=(), label=None):
    ds, shape_options = _shape(shape)
    gpu = _make(ds, {**shape_options, **(options or {})})
    tr = gpu.trajectory_
    info, sums = tr.DebugInnerFirstEvaluations(flags)
    rb = _jets(shape, flags)
    ra = R.block_sums(gpu, ds, flags)
    assert ra.P == rb.P == tr.GetTangentLayout(flags)["P"] and len(info) > 0
    label = label or "%s flags=%d %s" % (shape, flags, ",".join("%s=%g" % kv for kv in (options or {}).items()) or "default")
    # every block of the plan once, dimensions as the kinds say, the sums zero behind NV (R.compare asserts the exact facts)
    for i8, row in zip(info, sums):
        assert i8[3] == len(rb.columns(int(i8[1]), int(i8[2]))) and not row[R.nv_of(int(i8[3])):].any()
    ma, mb = R.compare(ra, info, sums), R.compare(rb, info, sums)
    routes = sorted(set(int(r) for r in info[:, 6]))
    print("MARGIN %-58s %4d blocks routes %s | (a) H %.2e g %.2e cost %.1e of %.0e | (b) H %.2e g %.2e cost %.1e | worst (a) H: %s; (b) H: %s"
          % (label, len(info), routes, ma["H"][0], ma["g"][0], ma["cost"][0], BOUND_A, mb["H"][0], mb["g"][0], mb["cost"][0], _name(ra, info, ma["H"][1]), _name(rb, info, mb["H"][1])))
    d = lambda ref, i: N.describe(ref.L, i)
    assert mb["H"][0] <= 1e-10, (label, "(b) H", mb["H"][0], _name(rb, info, mb["H"][1]), d(rb, mb["H"][2]), d(rb, mb["H"][3]))
    assert mb["g"][0] <= 1e-10, (label, "(b) g", mb["g"][0], _name(rb, info, mb["g"][1]), d(rb, mb["g"][2]))
    assert mb["cost"][0] <= 1e-11, (label, "(b) cost", mb["cost"][0], _name(rb, info, mb["cost"][1]))
    assert ma["H"][0] <= BOUND_A, (label, "(a) H", ma["H"][0], _name(ra, info, ma["H"][1]), d(ra, ma["H"][2]), d(ra, ma["H"][3]))
    assert ma["g"][0] <= BOUND_A, (label, "(a) g", ma["g"][0], _name(ra, info, ma["g"][1]), d(ra, ma["g"][2]))
    assert ma["cost"][0] <= BOUND_A, (label, "(a) cost", ma["cost"][0], _name(ra, info, ma["cost"][1]))
    for r in need:
        assert r in routes, (label, "route %d (%s) does not occur" % (r, _abi.INNER_ROUTES[r]), routes)
    for r in forbid:
        assert r not in routes, (label, "route %d (%s) occurs" % (r, _abi.INNER_ROUTES[r]), routes)
    # route and part count as the plan's rule says: more than SHARED_ABOVE item slots <=> shared (routes 4, 5; nparts from the plan)
    for i8 in info:
        assert (i8[6] in (4, 5)) == (i8[7] > 1 or i8[6] == 5) and (i8[6] < 4 or i8[5] > SHARED_ABOVE), (label, list(i8))
    # two calls in a row: bit-identical rows (route 4 adds its parts by atomics in arrival order: exempt)
    info2, sums2 = tr.DebugInnerFirstEvaluations(flags)
    fixed = info[:, 6] != 4
    assert np.array_equal(info, info2) and np.array_equal(sums[fixed], sums2[fixed]), (label, "two calls differ")
    return gpu, info, sums, rb


def _blockwise_difference(ref, info, sa, sb, rows):
    """max over the blocks `rows` of |a - b| entry-wise on the scale d_i d_j (g: d_i sqrt(2 cost_b), cost: relative) of `ref`."""
    worst = 0.0
    weak = N.weak_columns(ref.H, ref.kinds)          # (the weak columns of the merged assembly tests stay out of a ratio, as in N.entrywise_error)
    for b in rows:
        kind, idx, dim = int(info[b, 1]), int(info[b, 2]), int(info[b, 3])
        cols, H_ref, _, cost_ref, _ = ref.block(kind, idx)
        Ha, ga, ca, _ = R.unpack(sa[b], dim); Hb, gb, cb, _ = R.unpack(sb[b], dim)
        dd = np.sqrt(np.abs(np.diag(H_ref)).astype(np.float64)); ok = (dd > 0) & ~weak[cols]
        if ok.any():
            worst = max(worst, float((np.abs(Ha - Hb)[np.ix_(ok, ok)] / np.outer(dd[ok], dd[ok])).max()),
                        float((np.abs(ga - gb)[ok] / (dd[ok] * np.sqrt(2.0 * float(cost_ref)))).max()))
        worst = max(worst, abs(ca - cb) / float(cost_ref))
    return worst


# ---- the cases: shape x flags x options, and the routes that must occur --------------------------------------------------------------
@pytest.mark.parametrize("flags", [FLAGS1, ALL, E.CAM_LINE_DELAY])
def test_tiny_default(flags):
    run_case("tiny", flags, need=(0,) if flags == E.CAM_LINE_DELAY else (0, 1))          # (the line delay alone: one block, no R^3 set)


@pytest.mark.parametrize("flags", [FLAGS1, ALL])
def test_tiny_general_kernel_only(flags):
    run_case("tiny", flags, {"debug_inner_general_kernel": 1}, need=(0,), forbid=(1,))


@pytest.mark.parametrize("flags", [FLAGS1, FLAGS1 | E.IMU_BIASES])
def test_tiny_one_wave_per_block_against_one_workgroup_per_block(flags):
    """inner_wave_blocks = 1: every eligible set on inner_wave_kernel, both builds (sets of R^3 knots only: R3ONLY; sets with SO(3)
    knots: the general one); = 2: never.  The same block, summed by a wave or by a workgroup, agrees to 1e-13 entry-wise (the same
    items in the same order inside a round; the rounds' sums are grouped differently)."""
    _, i1, s1, rb = run_case("tiny", flags, {"inner_wave_blocks": 1}, need=(3,))
    wave = i1[:, 6] == 3
    assert (i1[wave, 1] == R.IK_SO3).any() and (i1[wave, 1] == R.IK_R3).any()
    sets = [set(int(k) for k in i1[wave & (i1[:, 0] == s), 1]) for s in np.unique(i1[wave, 0])]
    assert {R.IK_R3} in sets and any(R.IK_SO3 in s for s in sets), sets          # an R3ONLY launch and a general one
    _, i2, s2, _ = run_case("tiny", flags, {"inner_wave_blocks": 2}, forbid=(3,))
    assert np.array_equal(i1[:, :6], i2[:, :6])
    rows = np.flatnonzero(np.isin(i1[:, 6], (0, 1, 3)) & np.isin(i2[:, 6], (0, 1, 3)))
    assert len(rows) >= wave.sum()
    diff = _blockwise_difference(rb, i1, s1, s2, rows)
    print("MARGIN tiny flags=%d wave against workgroup: %.2e of 1e-13 over %d blocks" % (flags, diff, len(rows)))
    assert diff <= 1e-13


@pytest.mark.parametrize("flags", [FLAGS1 | E.POINTS, E.T_I_C | E.POINTS])
def test_tiny_board_points(flags):
    _, info, _, _ = run_case("tiny", flags, need=(2,))
    assert (info[info[:, 1] == R.IK_PT, 6] == 2).all() and (info[:, 1] == R.IK_PT).any()


@pytest.mark.parametrize("shape", ["gs_views", "gs_views_unit_loss", "knot_spacing_56_128", "short_0.3s"])
def test_shapes_default(shape):
    run_case(shape, FLAGS1, need=(0, 1))


@pytest.mark.parametrize("options", [{}, {"inner_wave_blocks": 1}])
def test_neighbourhoods_beyond_the_lds_copy(options):
    """knot_spacing_200_17: an SO(3) knot's items span 6 x 0.2 s = about 70 R^3 knots of 17 ms, more than the KCAP_R = 16 the LDS copy
    of a neighbourhood holds: such blocks read the parameter vector itself (inner_set_kernel, `local` false), and a set that holds one
    does not go to the wave kernel, whatever inner_wave_blocks says -- the route shows the fallback."""
    _, info, _, rb = run_case("knot_spacing_200_17", FLAGS1, options, need=(0,))
    beyond = np.array([rb.knots_read(int(k), int(i))[3] > KCAP_R for k, i in info[:, 1:3]])
    assert (beyond & (info[:, 6] == 0) & (info[:, 1] == R.IK_SO3)).any(), "no block beyond the LDS copy"
    sets_beyond = np.unique(info[beyond, 0])
    assert not (info[np.isin(info[:, 0], sets_beyond), 6] == 3).any(), "a set with a neighbourhood beyond the LDS copy on the wave kernel"
    if options:
        assert (info[~np.isin(info[:, 0], sets_beyond) & np.isin(info[:, 1], (R.IK_SO3, R.IK_R3)), 6] == 3).all()


def test_first_knot_behind_a_gap_under_lds_poison():
    """gap (C1 without 1.1 s of measurements): the first SO(3) knot behind the gap is the first knot of all its items' windows (ks0 ==
    idx), the pair in front of it lies outside the staged segment tables."""
    _, info, _, rb = run_case("gap", FLAGS1, {"debug_poison_lds": 1}, need=(0,))
    first = [int(i) for k, i, r in info[:, [1, 2, 6]] if k == R.IK_SO3 and r == 0 and i > 0 and rb.knots_read(int(k), int(i))[0] == i]
    assert first, "no SO(3) block whose own knot is the first its items read"


def test_ragged_views_with_the_line_delay():
    run_case("ragged", FLAGS1 | E.CAM_LINE_DELAY, need=(0,))


@pytest.mark.parametrize("flags", [FLAGS1, ALL])
def test_c1_shared_blocks_on_resident_workgroups_and_by_launches(flags):
    """C1: T_i_c has 1200 corner slots (> SHARED_ABOVE).  inner_shared_launch_slots = 0: parts on resident workgroups (route 4), = 1: every
    shared block by (evaluation, advance) launches (route 5, two parts or more).  The same shared block on either route: the parts cut
    the items differently and route 4 adds them in arrival order, so the two sums differ by summation order only -- at most
    2 n 2^-53 d_i d_j for n items (first-order bound of two recursive sums of n terms, sum |J_i J_j| <= d_i d_j)."""
    _, i4, s4, rb = run_case("C1", flags, {"inner_shared_launch_slots": 0}, need=(4,), forbid=(5,))
    _, i5, s5, _ = run_case("C1", flags, {"inner_shared_launch_slots": 1}, need=(5,), forbid=(4,))
    assert np.array_equal(i4[:, :6], i5[:, :6])
    shared = np.flatnonzero(i4[:, 6] == 4)
    assert len(shared) and (i5[shared, 6] == 5).all() and (i5[shared, 7] >= 2).all() and (i4[shared, 7] >= 2).all()
    assert R.IK_TIC in i4[shared, 1] and int(i4[shared][i4[shared, 1] == R.IK_TIC][0, 5]) > SHARED_ABOVE
    for b in shared:
        diff, bound = _blockwise_difference(rb, i4, s4, s5, [b]), 2 * int(i4[b, 4]) * 2.0 ** -53
        print("MARGIN C1 flags=%d %s routes 4 / 5: %.2e of %.2e" % (flags, _name(rb, i4, b), diff, bound))
        assert diff <= bound


def test_c1_board_points_next_to_shared_blocks():
    run_case("C1", FLAGS1 | E.POINTS, need=(2, 4))


# ---- the call leaves the problem as it is -------------------------------------------------------------------------------------------
def _state(tr):
    so3, r3 = tr.GetKnots(); ab, gb = tr.GetBiasKnots(); ai, gi = tr.GetIMUIntrinsics()
    return [np.array(a, dtype=np.float64).copy() for a in (so3, r3, tr.GetT_i_c(), tr.GetGravity(), ab, gb, ai, gi, tr.GetScenePoints(), [tr.GetRSLineDelay()])]


@pytest.mark.parametrize("flags", [FLAGS1, ALL | E.POINTS])
def test_the_read_out_leaves_the_problem_untouched(flags):
    """Parameters bit-identical before and after; a following Optimize with inner iterations gives the iterates of a fresh problem
    (counters of sweeps and per-block LM iterations included).  Two solves of one problem on one device differ by the order of the
    fp64 atomics of the assembly only: 1e-9 on the costs, the bound of the project's tests that compare two GPU runs
    (test_gpu_parity.py: the two builds of the set kernel)."""
    ds, options = _shape("tiny")
    out = []
    for read_out in (True, False):
        c = _make(ds, options); tr = c.trajectory_
        tr.SetOption("inner_iterations", 1)
        if read_out:
            before = _state(tr)
            tr.DebugInnerFirstEvaluations(flags)
            tr.DebugInnerFirstEvaluations(FLAGS1)
            for a, b in zip(before, _state(tr)):
                assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
        s = tr.Optimize(50, flags)
        out.append((s, tr.GetIterations(), _state(tr)))
    (s0, i0, x0), (s1, i1, x1) = out
    assert s0["num_iterations"] == s1["num_iterations"] and s0["inner_sweeps"] == s1["inner_sweeps"] >= 1, (s0, s1)
    assert abs(s0["inner_lm_iterations"] - s1["inner_lm_iterations"]) <= 0.002 * s1["inner_lm_iterations"] + 1, (s0["inner_lm_iterations"], s1["inner_lm_iterations"])
    assert len(i0) == len(i1) and all(a["step_is_successful"] == b["step_is_successful"] and abs(a["cost"] - b["cost"]) <= 1e-9 * b["cost"] for a, b in zip(i0, i1))
    assert np.abs(x0[2] - x1[2]).max() < 1e-8


# ---- inner_cholesky_solve<D> --------------------------------------------------------------------------------------------------------
LD = np.longdouble
N_SYSTEMS = 4096
PIVOT_CLEAR = 1e-12          # smallest long-double pivot, relative to its diagonal entry, of a system that must solve: 1000 x the
                             # rounding (D + 1) 2^-53 of a float64 pivot -- below that the reference alone could not say whether ok = 1


def _device_solve(D, M, rhs):
    fn = _abi.bind_inner_debug(_lib.load().lib, "oicc_debug_inner_cholesky")
    M = np.ascontiguousarray(M, dtype=np.float64); rhs = np.ascontiguousarray(rhs, dtype=np.float64)
    n = len(M)
    x = np.zeros((n, D)); ok = np.zeros(n, np.uint8)
    dp = lambda a: a.ctypes.data_as(_abi.c_dp)
    assert fn(0, D, n, dp(M), dp(rhs), dp(x), ok.ctypes.data_as(_abi.c_u8p)) == 0
    return x, ok.astype(bool)


def _ld_cholesky(M, rhs):
    """Plain Cholesky solve in np.longdouble, all systems at once, from the lower triangle (what the kernel reads).  Returns x, the
    pivots [n, D] (NaN behind the first non-positive one)."""
    n, D = rhs.shape
    M = M.astype(LD); rhs = rhs.astype(LD)
    L = np.zeros((n, D, D), LD); piv = np.full((n, D), np.nan, LD); alive = np.ones(n, bool)
    with np.errstate(all="ignore"):
        for j in range(D):
            s = M[:, j, j] - (L[:, j, :j] ** 2).sum(axis=1)
            piv[alive, j] = s[alive]
            alive &= s > 0
            L[:, j, j] = np.sqrt(np.where(s > 0, s, 1))
            for i in range(j + 1, D):
                L[:, i, j] = (M[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(axis=1)) / L[:, j, j]
        y = np.zeros((n, D), LD); x = np.zeros((n, D), LD)
        for i in range(D):
            y[:, i] = (rhs[:, i] - (L[:, i, :i] * y[:, :i]).sum(axis=1)) / L[:, i, i]
        for i in range(D - 1, -1, -1):
            x[:, i] = (y[:, i] - (L[:, i + 1:, i] * x[:, i + 1:]).sum(axis=1)) / L[:, i, i]
    return x, piv


def _lm_systems(D, rng):
    """Systems of the LM loop's own form (inner_lm_advance): M = S G S + diag(clamp(diag(G) s^2, 1e-6, 1e32)) / radius, rhs = -S A^T r,
    G = A^T A, s_i = 1 / (1 + sqrt(G_ii)), formed in float64 as the loop forms them.  A: 2 ... 40 rows, column scales 1e-6 ... 1e6,
    for D > 1 one system in four rank deficient (fewer rows than columns, or a column repeated); radius 1e-8 ... 1e16, drawn again
    while the smallest long-double pivot is not clear of rounding (PIVOT_CLEAR): only damping can make a rank-deficient system solve."""
    n = N_SYSTEMS
    G = np.zeros((n, D, D)); g = np.zeros((n, D))
    for k in range(n):
        m = int(rng.integers(2, 41))
        A = rng.standard_normal((m, D)) * 10.0 ** rng.uniform(-6, 6, D)
        if D > 1 and k % 4 == 0:
            if k % 8 == 0:
                A = A[:min(m, D - 1)] if m >= D else A
                A = A if len(A) >= 1 else rng.standard_normal((1, D))
            else:
                A[:, int(rng.integers(1, D))] = A[:, 0] * 10.0 ** rng.uniform(-3, 3)
        r = rng.standard_normal(len(A))
        G[k] = A.T @ A; g[k] = A.T @ r
    diagG = np.einsum("nii->ni", G)
    sc = 1.0 / (1.0 + np.sqrt(diagG))
    dg = np.clip(diagG * sc * sc, 1e-6, 1e32)
    radius = 10.0 ** rng.uniform(-8, 16, n)
    todo = np.ones(n, bool)
    M = np.zeros((n, D, D)); rhs = -g * sc
    for _ in range(40):
        inv_radius = 1.0 / radius
        Mn = G * sc[:, :, None] * sc[:, None, :]
        Mn[:, np.arange(D), np.arange(D)] += dg * inv_radius[:, None]
        M[todo] = Mn[todo]
        _, piv = _ld_cholesky(M, rhs)
        ratio = (piv / np.einsum("nii->ni", M).astype(LD)).astype(np.float64)
        todo = ~(np.nan_to_num(ratio, nan=-1.0).min(axis=1) >= PIVOT_CLEAR)
        if not todo.any():
            break
        radius[todo] = 10.0 ** rng.uniform(-8, 16, int(todo.sum()))
    assert not todo.any()
    low = np.tril(M)
    return low + np.transpose(np.tril(M, -1), (0, 2, 1)), rhs          # symmetric from the lower triangle the kernel reads


def _backward_error(M, x, rhs):
    M = M.astype(LD); x = x.astype(LD); rhs = rhs.astype(LD)
    res = np.abs(np.einsum("nij,nj->ni", M, x) - rhs).max(axis=1)
    return (res / (np.abs(M).sum(axis=2).max(axis=1) * np.abs(x).max(axis=1) + np.abs(rhs).max(axis=1))).astype(np.float64)


@pytest.mark.parametrize("D", [1, 3, 6, 9])
def test_inner_cholesky_solve_against_a_long_double_solve(D):
    """4096 seeded systems per D through inner_cholesky_solve<D> itself, one lane each.  D = 1 (no off-diagonal loop at all) and the last
    pivot of D = 9 (no row below it) are the edges where the unrolled loops degenerate: every one of the 4096 systems of D = 1 / D = 9
    passes through them, and the rejected matrices below put the bad pivot at the first, a middle and the last position.
    Backward error (normwise, inf-norm, evaluated in long double): the device's maximum over the batch <= 8 x that of numpy's float64
    solve on the same systems (not below D 2^-52); forward error against the long-double solve <= cond_inf 64 2^-52 for cond <= 1e6.
    Measured on an MI355X, maxima over the batch (device / numpy float64 / bound = max(8 x numpy, D 2^-52)): D = 1: 2.4e-16 / 5.5e-17 /
    4.4e-16; D = 3: 2.3e-16 / 1.5e-16 / 1.2e-15; D = 6: 2.2e-16 / 1.5e-16 / 1.3e-15; D = 9: 1.9e-16 / 1.8e-16 / 2.0e-15.  Forward error
    over the systems with cond <= 1e6: at most 0.033 of cond 64 2^-52."""
    rng = np.random.default_rng(20240 + D)
    M, rhs = _lm_systems(D, rng)
    x_ld, piv = _ld_cholesky(M, rhs)
    assert np.isfinite(piv.astype(np.float64)).all() and ((piv / np.einsum("nii->ni", M).astype(LD)).astype(np.float64) >= PIVOT_CLEAR).all()   # no borderline pivot: the reference alone says "solves"
    x, ok = _device_solve(D, M, rhs)
    assert ok.all(), (D, "ok = 0 for systems of the loop's own form", np.flatnonzero(~ok)[:8])
    cond = np.linalg.cond(M, np.inf)
    e_dev, e_np = _backward_error(M, x, rhs), _backward_error(M, np.linalg.solve(M, rhs[:, :, None])[:, :, 0], rhs)
    bound = max(8 * e_np.max(), D * 2.0 ** -52)
    small = cond <= 1e6
    fwd = (np.abs(x.astype(LD) - x_ld).max(axis=1) / np.abs(x_ld).max(axis=1)).astype(np.float64)
    fr = (fwd[small] / (cond[small] * 64 * 2.0 ** -52)).max()
    print("MARGIN inner_cholesky_solve<%d>: backward error device %.2e, numpy float64 %.2e (bound %.2e); cond %.1e ... %.1e, %d systems with cond <= 1e6: forward error / (cond 64 2^-52) = %.2e"
          % (D, e_dev.max(), e_np.max(), bound, cond.min(), cond.max(), small.sum(), fr))
    assert small.sum() >= N_SYSTEMS // 8 and (D == 1 or cond.max() >= 1e10)
    assert e_dev.max() <= bound, (D, int(e_dev.argmax()), e_dev.max(), bound)
    assert fr <= 1.0, (D, fr)


@pytest.mark.parametrize("D", [1, 3, 6, 9])
def test_inner_cholesky_solve_rejects_what_it_must(D):
    """ok = 0 for one clearly negative pivot (first, middle, last position), an exactly zero pivot (a zero row and column: every
    product that enters the pivot is an exact zero), a NaN or an Inf anywhere in M (both triangles) or rhs; the long-double solve alone
    decides each case: the pivot is negative by more than 1e-8 of its diagonal entry, or exactly zero.  Register arithmetic only."""
    rng = np.random.default_rng(777 + D)
    positions = sorted({0, D // 2, D - 1})
    Ms, rs, why = [], [], []
    for rep in range(8):
        Lu = np.tril(rng.uniform(-1, 1, (D, D)), -1) + np.eye(D)
        dd = rng.uniform(0.5, 2.0, D)
        good = Lu @ np.diag(dd) @ Lu.T; good = np.tril(good) + np.tril(good, -1).T
        r = rng.standard_normal(D)
        for j in positions:
            d2 = dd.copy(); d2[j] = -rng.uniform(0.5, 2.0)
            neg = Lu @ np.diag(d2) @ Lu.T; neg = np.tril(neg) + np.tril(neg, -1).T
            Ms.append(neg); rs.append(r); why.append(("negative", j))
            z = good.copy(); z[j, :] = 0.0; z[:, j] = 0.0
            Ms.append(z); rs.append(r); why.append(("zero", j))
            for bad in (np.nan, np.inf, -np.inf):
                i = int(rng.integers(0, D))
                m = good.copy(); m[i, j] = bad; m[j, i] = bad
                Ms.append(m); rs.append(r); why.append(("M[%d,%d]=%s" % (i, j, bad), j))
                rr = r.copy(); rr[j] = bad
                Ms.append(good); rs.append(rr); why.append(("rhs[%d]=%s" % (j, bad), j))
        Ms.append(good); rs.append(r); why.append(("good", -1))
    M, rhs = np.array(Ms), np.array(rs)
    _, piv = _ld_cholesky(np.nan_to_num(M, nan=0.0, posinf=0.0, neginf=0.0), np.nan_to_num(rhs, nan=0.0, posinf=0.0, neginf=0.0))
    for k, (w, j) in enumerate(why):          # the reference alone decides
        p = piv[k].astype(np.float64)
        if w == "negative":
            assert (p[:j] > 1e-8 * np.diag(M[k])[:j]).all() and p[j] < -1e-8 * abs(M[k, j, j]), (k, w, j, p)
        elif w == "zero":
            assert (p[:j] > 0).all() and p[j] == 0.0, (k, w, j, p)
        elif w == "good":
            assert (p > 1e-8 * np.diag(M[k])).all()
    x, ok = _device_solve(D, M, rhs)
    for k, (w, j) in enumerate(why):
        assert ok[k] == (w == "good"), (D, k, w, j, ok[k], x[k])
