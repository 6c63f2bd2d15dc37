"""Yardstick of oicc_ba_estimate_covariance (no GPU): from a dense J^T J of the view bundle adjustment, H = [[A, E], [E', C]] with
A block diagonal (nv blocks of d x d) and an a x a intrinsics corner, the inverse of the matrix scaled to unit diagonal,
Hs = S H S with s_i = H_ii^-1/2, in 50-digit arithmetic (mpmath):

    dense_inverse(H)            (S H S)^-1 by a dense 50-digit inversion -- small P
    schur_inverse(H, nv, d, a)  the same entries restated through the per-view Schur complement -- large P
    kappa1(H)                   the 1-norm condition number of S H S from a float64 inverse: it sizes the tests' bound and never
                                comes from the code under test

Views whose d x d block is all zero (no observations) are left out of the system by used_views() / reduce()."""
import mpmath as mp
import numpy as np

mp.mp.dps = 50
EPS = float(np.finfo(np.float64).eps)


def used_views(H, nv, d):
    """Indices of the views with a non-zero diagonal block."""
    return [v for v in range(nv) if d > 0 and np.any(H[v * d:(v + 1) * d, v * d:(v + 1) * d] != 0.0)]


def reduce(H, nv, d, a):
    """(H without the rows and columns of the unused views, the used views)."""
    used = used_views(H, nv, d)
    keep = [v * d + r for v in used for r in range(d)] + list(range(nv * d, nv * d + a))
    return H[np.ix_(keep, keep)], used


def scale_factors(H):
    """s_i = H_ii^-1/2 in float64: what a test divides the covariance by to get the scaled form Zs_ij = cov_ij / (s_i s_j)."""
    return 1.0 / np.sqrt(np.diag(H))


def scaled_mp(H):
    """S H S as an mpmath matrix, the scaling itself in 50 digits (unit diagonal)."""
    n = H.shape[0]
    s = [1 / mp.sqrt(mp.mpf(float(H[i, i]))) for i in range(n)]
    M = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            M[i, j] = mp.mpf(1) if i == j else mp.mpf(float(H[i, j])) * s[i] * s[j]
    return M


def scaled_longdouble(H):
    s = 1.0 / np.sqrt(np.diag(H).astype(np.longdouble))
    Hs = H.astype(np.longdouble) * np.outer(s, s)
    Hs[np.diag_indices_from(Hs)] = 1.0
    return Hs


def dense_inverse(H):
    """(S H S)^-1, 50 digits, as an mpmath matrix."""
    return mp.inverse(scaled_mp(H))


def _sub(M, r0, r1, c0, c1):
    out = mp.matrix(r1 - r0, c1 - c0)
    for i in range(r0, r1):
        for j in range(c0, c1):
            out[i - r0, j - c0] = M[i, j]
    return out


def schur_inverse(H, nv, d, a):
    """The handed-out entries of (S H S)^-1 through the per-view Schur complement, 50 digits; H holds used views only.
    Returns (theta [a x a], poses: nv matrices d x d, cross: nv matrices d x a) as mpmath matrices."""
    Pb = nv * d
    n = Pb + a
    s = [1 / mp.sqrt(mp.mpf(float(H[i, i]))) for i in range(n)]

    def blk(r0, r1, c0, c1):
        out = mp.matrix(r1 - r0, c1 - c0)
        for i in range(r0, r1):
            for j in range(c0, c1):
                out[i - r0, j - c0] = mp.mpf(1) if i == j else mp.mpf(float(H[i, j])) * s[i] * s[j]
        return out

    S = blk(Pb, n, Pb, n) if a else mp.matrix(0, 0)
    Ainv, W = [], []
    for v in range(nv):
        Ai = mp.inverse(blk(v * d, (v + 1) * d, v * d, (v + 1) * d))
        Ainv.append(Ai)
        if a:
            E = blk(v * d, (v + 1) * d, Pb, n)
            Wv = Ai * E
            W.append(Wv)
            S = S - E.T * Wv
    theta = mp.inverse(S) if a else mp.matrix(0, 0)
    if not a:
        return theta, Ainv, [mp.matrix(d, 0) for _ in range(nv)]
    poses = [Ainv[v] + W[v] * theta * W[v].T for v in range(nv)]
    cross = [-(W[v] * theta) for v in range(nv)]
    return theta, poses, cross


def to_float(M):
    return np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)], dtype=np.float64).reshape(M.rows, M.cols)


def handed_out_from_dense(Z, nv, d, a):
    """(theta, poses, cross) cut out of a dense inverse, as schur_inverse returns them."""
    Pb = nv * d
    theta = _sub(Z, Pb, Pb + a, Pb, Pb + a)
    poses = [_sub(Z, v * d, (v + 1) * d, v * d, (v + 1) * d) for v in range(nv)]
    cross = [_sub(Z, v * d, (v + 1) * d, Pb, Pb + a) for v in range(nv)]
    return theta, poses, cross


def max_abs(mats):
    m = mp.mpf(0)
    for M in mats:
        for i in range(M.rows):
            for j in range(M.cols):
                m = max(m, abs(M[i, j]))
    return m


def kappa1(H):
    """kappa_1(S H S) from a float64 inverse."""
    Hs = np.asarray(scaled_longdouble(H), dtype=np.float64)
    return float(np.abs(Hs).sum(axis=0).max() * np.abs(np.linalg.inv(Hs)).sum(axis=0).max())


def rcond_of(theta, poses):
    """1 / max_i Zs_ii over the handed-out diagonal entries (float)."""
    m = mp.mpf(0)
    for M in [theta] + list(poses):
        for i in range(M.rows):
            m = max(m, M[i, i])
    return float(1 / m)
