"""numpy restatement of oicc_planar_ransac (csrc/planar_ransac.hip): the checker of the device entry and the
specification of its sampler, arithmetic and constants ("Robust start poses").  Usable as the `backend` of
openimucameracalibrator_amd.robust_init (it has the same `run`), in float64 or numpy.longdouble.

Per view with n >= 5 corners, board plane coordinates (a, b), features (u, v) relative to the distortion centre:

  1 sample      hypothesis h draws five distinct corners: partial Fisher-Yates over 0..n-1, draw j swaps position j with
                t = j + (mix64(seed * GOLDEN + (view << 24) + (h << 4) + j) >> 11) % (n - j), all in uint64
  2 hypothesis  q = null vector of the 5 x 6 system  u (q3 a + q4 b + q5) - v (q0 a + q1 b + q2) = 0  through its 5 x 5
                minors (Laplace expansion along the last row, rows added one at a time)
  3 vote        x = q0 a + q1 b + q2, y = q3 a + q4 b + q5; a corner passes when (u y - v x)^2 < thr^2 (x^2 + y^2) and
                it lies on the majority side of u x + v y; score = number passing, ties to the smaller h
  4 refit       normal matrix of the winner's inliers, eigenvector of its smallest eigenvalue by cyclic Jacobi
                (JACOBI_SWEEPS sweeps); a view whose second smallest eigenvalue is <= DEGENERATE_RATIO * largest is
                degenerate (board corners on one line) and reports no inliers; re-classification as in 3
  5 calibrated  pose from q by the orthonormality of the two rotation columns, two sign branches, t_z = median of the
                per-corner solutions over the inliers of 4, full reprojection test (x - u z)^2 + (y - v z)^2 < g^2 thr^2 z^2,
                z > 0 with the loose gate g = LOOSE_GATE; the branch with more corners wins, ties to the first; least-squares
                refit of (r31, r32, t_z) on the radial part of the error over the gated corners; the test again with g = 1
"""
import itertools

import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
MASK64 = (1 << 64) - 1
DEFAULT_SEED = 20241115
JACOBI_SWEEPS = 12
DEGENERATE_RATIO = 1e-12
MIN_SAMPLE = 5
LOOSE_GATE = 3.0            # calibrated mode: gate of the closed-form pose, in thresholds, before the depth refit
SOLVE3_RATIO = 1e-12
FLAG_MARGIN = 1e-6          # a hypothesis is flagged when a corner is this close (relative to thr) to a decision
FLAG_SINGULAR = 1e-6        # ... or when the 5 x 6 system's smallest / largest singular value is below this


# ---- 1 sampler ------------------------------------------------------------------------------------------------------
def mix64(x):
    """The 64-bit finaliser of MurmurHash3 on uint64 arrays."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(33))) * np.uint64(0xff51afd7ed558ccd)
        x = (x ^ (x >> np.uint64(33))) * np.uint64(0xc4ceb9fe1a85ec53)
    return x ^ (x >> np.uint64(33))


def sample5(seed, view, num_hypotheses, n):
    """[num_hypotheses, 5] corner indices.  The permutation array is virtual: positions 0..4 are kept in `first`, every
    other touched position in (mp, mv) -- what the device keeps in registers."""
    H = int(num_hypotheses)
    h = np.arange(H, dtype=np.uint64)
    base = np.uint64((int(seed) * GOLDEN + (int(view) << 24)) & MASK64)
    first = np.tile(np.arange(5, dtype=np.int64), (H, 1))
    mp = -np.ones((H, 5), np.int64)
    mv = np.zeros((H, 5), np.int64)
    for j in range(5):
        with np.errstate(over="ignore"):
            r = mix64(base + (h << np.uint64(4)) + np.uint64(j))
        t = j + ((r >> np.uint64(11)) % np.uint64(n - j)).astype(np.int64)
        low = t < 5
        vt = t.copy()
        for k in range(5):
            vt = np.where(low & (t == k), first[:, k], vt)
        for k in range(j):
            vt = np.where(~low & (mp[:, k] == t), mv[:, k], vt)
        vj = first[:, j].copy()
        for k in range(5):
            first[:, k] = np.where(low & (t == k), vj, first[:, k])
        hit_any = np.zeros(H, bool)
        for k in range(j):
            hit = ~low & (mp[:, k] == t)
            mv[:, k] = np.where(hit, vj, mv[:, k])
            hit_any |= hit
        new = ~low & ~hit_any
        mp[:, j] = np.where(new, t, -1)
        mv[:, j] = np.where(new, vj, 0)
        first[:, j] = vt
    return first


# ---- 2 hypothesis ---------------------------------------------------------------------------------------------------
def constraint_rows(a, b, u, v):
    """[..., 6] rows of the radial alignment constraint."""
    return np.stack([-(v * a), -(v * b), -v, u * a, u * b, u], -1)


def minors_plan():
    """The straight-line program of the null vector: for row r = 1..4, every (r+1)-column minor of rows 0..r as the
    signed sum, left to right, of A[r][c_k] * minor(rows 0..r-1, columns without c_k), sign (-1)^(r+k)."""
    plan = []
    for r in range(1, 5):
        for cols in itertools.combinations(range(6), r + 1):
            plan.append((r, cols, [((-1) ** (r + k), c, cols[:k] + cols[k + 1:]) for k, c in enumerate(cols)]))
    return plan


def null_vector(A):
    """A [H, 5, 6] -> q [H, 6] with q_k = (-1)^k det(A without column k)."""
    M = {(c,): A[:, 0, c] for c in range(6)}
    for r, cols, terms in minors_plan():
        acc = None
        for sign, c, rest in terms:
            t = A[:, r, c] * M[rest]
            if acc is None:
                acc = t if sign > 0 else -t
            else:
                acc = acc + t if sign > 0 else acc - t
        M[cols] = acc
    full = tuple(range(6))
    return np.stack([M[full[:k] + full[k + 1:]] if k % 2 == 0 else -M[full[:k] + full[k + 1:]] for k in range(6)], -1)


# ---- 3 vote ---------------------------------------------------------------------------------------------------------
def classify(q, a, b, u, v, thr2):
    """q [..., 6] against the corners [n]: (tangential test [..., n], side [..., n], x, y)."""
    q = q[..., None, :]
    x = (q[..., 0] * a + q[..., 1] * b) + q[..., 2]
    y = (q[..., 3] * a + q[..., 4] * b) + q[..., 5]
    cross = u * y - v * x
    side = u * x + v * y
    nrm2 = x * x + y * y
    return cross * cross < thr2 * nrm2, side, cross, nrm2


def majority(tang, side):
    """(flip, inlier mask): the sign of q is arbitrary, the corners must lie on the half-line of the majority."""
    n_pos = (side > 0).sum(-1)
    n_neg = (side < 0).sum(-1)
    flip = n_pos < n_neg
    return flip, tang & np.where(flip[..., None], side < 0, side > 0)


def vote(view, a, b, u, v, thr, num_hypotheses, seed, flags=False):
    """counts [H], sign-fixed q [H, 6]; with flags=True also which hypotheses lie too close to a decision to be compared."""
    dt = a.dtype
    S = sample5(seed, view, num_hypotheses, len(a))
    A = constraint_rows(a[S], b[S], u[S], v[S])
    q = null_vector(A)
    thr2 = dt.type(thr) * dt.type(thr)
    tang, side, cross, nrm2 = classify(q, a, b, u, v, thr2)
    flip, inl = majority(tang, side)
    counts = inl.sum(-1).astype(np.int32)
    q = np.where(flip[:, None], -q, q)
    if not flags:
        return counts, q, S
    with np.errstate(divide="ignore", invalid="ignore"):
        nrm = np.sqrt(nrm2.astype(np.float64))
        near = (np.abs(np.abs(cross.astype(np.float64)) / nrm - thr) < FLAG_MARGIN * thr) | (np.abs(side.astype(np.float64)) / nrm < FLAG_MARGIN * thr)
    near |= ~(nrm2 > 0)
    sv = np.linalg.svd(A.astype(np.float64), compute_uv=False)
    flagged = near.any(-1) | ~(sv[:, 4] >= FLAG_SINGULAR * sv[:, 0])
    return counts, q, S, flagged


# ---- 4 refit --------------------------------------------------------------------------------------------------------
def jacobi_eigh(N, sweeps=JACOBI_SWEEPS):
    """Cyclic Jacobi on a symmetric 6 x 6 (rows p < q in order, `sweeps` sweeps, a zero off-diagonal entry is skipped).
    Returns (diagonal, V) with N ~ V diag V^T."""
    A = np.array(N, copy=True)
    dt = A.dtype.type
    n = A.shape[0]
    V = np.eye(n, dtype=A.dtype)
    one = dt(1)
    for _ in range(sweeps):
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = A[p, q]
                if apq == 0:
                    continue
                with np.errstate(over="ignore"):
                    theta = (A[q, q] - A[p, p]) / (dt(2) * apq)
                    t = one / (np.abs(theta) + np.sqrt(theta * theta + one))
                if theta < 0:
                    t = -t
                c = one / np.sqrt(t * t + one)
                s = t * c
                A[p, p] = A[p, p] - t * apq
                A[q, q] = A[q, q] + t * apq
                A[p, q] = A[q, p] = dt(0)
                for r in range(n):
                    if r != p and r != q:
                        arp, arq = A[r, p], A[r, q]
                        A[r, p] = A[p, r] = c * arp - s * arq
                        A[r, q] = A[q, r] = s * arp + c * arq
                for r in range(n):
                    vrp, vrq = V[r, p], V[r, q]
                    V[r, p] = c * vrp - s * vrq
                    V[r, q] = s * vrp + c * vrq
    return np.diag(A).copy(), V


def refit(a, b, u, v, inl):
    """(q or None when degenerate, eigenvalues): smallest eigenvector of the normal matrix over the inliers."""
    R = constraint_rows(a[inl], b[inl], u[inl], v[inl])
    N = R.T @ R
    w, V = jacobi_eigh(N)
    k = 0
    for i in range(1, 6):         # first smallest
        if w[i] < w[k]:
            k = i
    rest = [w[i] for i in range(6) if i != k]
    if not (min(rest) > DEGENERATE_RATIO * max(w)):
        return None, w
    return V[:, k].copy(), w


# ---- 5 calibrated stage ---------------------------------------------------------------------------------------------
def median_of(values):
    """Median with the (value, index) order of the device's rank count: mean of the two middle ranks."""
    s = np.sort(values, kind="stable")
    m = len(s)
    return (s[(m - 1) // 2] + s[m // 2]) * values.dtype.type(0.5)


def pose_stage(q, a, b, u, v, inl, thr):
    """(mask, R [3,3], t [3]) of the better sign branch, or (all False, zeros, zeros) when q gives no rotation."""
    dt = a.dtype.type
    zero = (np.zeros(len(a), bool), np.zeros((3, 3), a.dtype), np.zeros(3, a.dtype))
    p = q[0] * q[0] + q[3] * q[3]
    r = q[1] * q[1] + q[4] * q[4]
    d = q[0] * q[1] + q[3] * q[4]
    det = p * r - d * d
    if not (det > 0):
        return zero
    tr = p + r
    k = (tr - np.sqrt(max(tr * tr - dt(4) * det, dt(0)))) / (dt(2) * det)       # 1 / scale^2: the smaller root
    if not (k > 0 and np.isfinite(k)):
        return zero
    s = np.sqrt(k)
    thr2 = dt(thr) * dt(thr)
    xc = s * ((q[0] * a + q[1] * b) + q[2])
    yc = s * ((q[3] * a + q[4] * b) + q[5])
    rho2 = u * u + v * v
    best = None
    for sg in (1.0, -1.0):
        r31 = dt(sg) * np.sqrt(max(dt(1) - p * k, dt(0)))
        r32 = -(d * k) / r31 if abs(r31) > 1e-12 else np.sqrt(max(dt(1) - r * k, dt(0)))
        zr = r31 * a + r32 * b
        with np.errstate(divide="ignore", invalid="ignore"):
            tzi = (xc * u + yc * v) / rho2 - zr
        use = inl & np.isfinite(tzi)
        if not use.any():
            continue
        tz = median_of(tzi[use])
        m = inl & reprojection_test(xc, yc, u, v, zr + tz, dt(LOOSE_GATE * LOOSE_GATE) * thr2)
        if best is None or m.sum() > best[0].sum():
            best = (m, r31, r32, tz)
    if best is None:
        return zero
    loose, r31, r32, tz = best
    # the third row from orthonormality is a square root of a small difference for a board seen head-on: refit
    # (r31, r32, t_z) by least squares on the radial part of the reprojection error over the loosely accepted corners
    g = np.stack([a, b, np.ones_like(a)], 1)[loose]
    G = (g * rho2[loose, None]).T @ g
    rhs = g.T @ (xc * u + yc * v)[loose]
    sol = solve3(G, rhs)
    if sol is not None:
        r31, r32, tz = sol
    m = inl & reprojection_test(xc, yc, u, v, (r31 * a + r32 * b) + tz, thr2)
    r1 = np.array([s * q[0], s * q[3], r31]); r2 = np.array([s * q[1], s * q[4], r32])
    return m, np.stack([r1, r2, np.cross(r1, r2)], 1), np.array([s * q[2], s * q[5], tz])


def reprojection_test(xc, yc, u, v, z, thr2):
    ex = xc - u * z
    ey = yc - v * z
    return (ex * ex + ey * ey < thr2 * (z * z)) & (z > 0)


def solve3(G, h):
    """Symmetric 3 x 3 by cofactors; None when det <= SOLVE3_RATIO * product of the diagonal."""
    c00 = G[1, 1] * G[2, 2] - G[1, 2] * G[1, 2]
    c01 = G[0, 2] * G[1, 2] - G[0, 1] * G[2, 2]
    c02 = G[0, 1] * G[1, 2] - G[0, 2] * G[1, 1]
    c11 = G[0, 0] * G[2, 2] - G[0, 2] * G[0, 2]
    c12 = G[0, 1] * G[0, 2] - G[0, 0] * G[1, 2]
    c22 = G[0, 0] * G[1, 1] - G[0, 1] * G[0, 1]
    det = (G[0, 0] * c00 + G[0, 1] * c01) + G[0, 2] * c02
    if not (det > G.dtype.type(SOLVE3_RATIO) * ((G[0, 0] * G[1, 1]) * G[2, 2])):
        return None
    return (((c00 * h[0] + c01 * h[1]) + c02 * h[2]) / det, ((c01 * h[0] + c11 * h[1]) + c12 * h[2]) / det,
            ((c02 * h[0] + c12 * h[1]) + c22 * h[2]) / det)


# ---- the whole entry ------------------------------------------------------------------------------------------------
def run_view(view, a, b, u, v, mode, thr, num_hypotheses, seed):
    """One view: dict(inlier, q, R, t, counts, winner)."""
    n = len(a)
    out = dict(inlier=np.zeros(n, bool), q=np.zeros(6, a.dtype), R=np.zeros((3, 3), a.dtype), t=np.zeros(3, a.dtype),
               counts=np.zeros(num_hypotheses, np.int32), winner=-1, stage1=np.zeros(n, bool))
    if n < MIN_SAMPLE:
        return out
    counts, qh, _ = vote(view, a, b, u, v, thr, num_hypotheses, seed)
    out["counts"] = counts
    win = int(np.argmax(counts))
    out["winner"] = win
    if counts[win] < MIN_SAMPLE:
        return out
    thr2 = a.dtype.type(thr) * a.dtype.type(thr)
    tang, side, _, _ = classify(qh[win], a, b, u, v, thr2)
    inl1 = tang & (side > 0)
    out["stage1"] = inl1
    q, _ = refit(a, b, u, v, inl1)
    if q is None:
        return out
    tang, side, _, _ = classify(q, a, b, u, v, thr2)
    flip, inl = majority(tang, side)
    if flip:
        q = -q
    out["q"] = q
    if mode == 0:
        out["inlier"] = inl
        return out
    out["inlier"], out["R"], out["t"] = pose_stage(q, a, b, u, v, inl, thr)
    return out


def run(corner_offsets, ab, xy, mode, threshold, num_hypotheses=256, seed=DEFAULT_SEED, device=0, want_counts=False, dtype=np.float64):
    """The backend interface of robust_init.planar_ransac: (inlier [n] bool, num_inliers [nv], q [nv, 6], pose [nv, 12],
    hypothesis counts [nv, H] or None)."""
    off = np.asarray(corner_offsets, dtype=np.int64)
    ab = np.asarray(ab, dtype=dtype).reshape(-1, 2)
    xy = np.asarray(xy, dtype=dtype).reshape(-1, 2)
    if not (np.all(np.isfinite(ab)) and np.all(np.isfinite(xy)) and threshold > 0 and 1 <= num_hypotheses <= 1024 and mode in (0, 1)):
        raise ValueError("oicc_planar_ransac: invalid argument")
    nv = len(off) - 1
    inlier = np.zeros(len(ab), bool)
    q = np.zeros((nv, 6), dtype)
    pose = np.zeros((nv, 12), dtype)
    counts = np.zeros((nv, num_hypotheses), np.int32)
    for view in range(nv):
        s = slice(off[view], off[view + 1])
        r = run_view(view, ab[s, 0], ab[s, 1], xy[s, 0], xy[s, 1], mode, threshold, num_hypotheses, seed)
        inlier[s] = r["inlier"]; q[view] = r["q"]; counts[view] = r["counts"]
        pose[view, :9] = r["R"].ravel(); pose[view, 9:] = r["t"]
    num = np.array([inlier[off[i]:off[i + 1]].sum() for i in range(nv)], np.int32)
    return inlier, num, q, pose, (counts if want_counts else None)
