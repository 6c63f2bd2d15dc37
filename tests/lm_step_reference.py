"""Host reference of one damped Levenberg-Marquardt solve of the spline problem, in float64 with extended-precision residuals.

Ceres' LevenbergMarquardtStrategy defines the system the device solvers solve:
    s_i  = 1 / (1 + sqrt(h_ii))                                   (Jacobi scaling; 1 without it)
    d_i  = clamp(h_ii s_i^2, min_lm_diagonal, max_lm_diagonal)     (or the previous call's d_i when the diagonal is reused)
    M    = S H S + diag(d) / radius,   rhs = -S g
H arrives packed as the library keeps it: the lower band by columns, band[j, k] = H(j + k, j) for k = 0..hb, the arrow rows
Et[q, j] = H(Pb + q, j) and the dense corner C = H[Pb:, Pb:].  M is kept in the same band + arrow form.

`solve` factors M in float64 (dense Cholesky up to System.DENSE_LIMIT unknowns, else a banded Cholesky with the Schur complement of the arrow)
and refines the solution with residuals accumulated in np.longdouble; `cond1` estimates kappa_1(M) through the same factor.
"""
import numpy as np
import scipy.linalg as sla
from scipy.sparse.linalg import LinearOperator, onenormest

LD = np.longdouble
# x86 80-bit extended precision on every machine the suite runs on: a silent loss of it would make the refinement a no-op
assert np.finfo(LD).eps <= 1.1e-19, "np.longdouble is not 80-bit extended precision here"

EPS = np.finfo(np.float64).eps


def hdiag(band, C):
    """The diagonal of H from the packed form."""
    return np.concatenate([band[:, 0], np.diag(C)])


def jacobi_scale(band, C, jacobi=True):
    h = hdiag(band, C)
    return 1.0 / (1.0 + np.sqrt(h)) if jacobi else np.ones_like(h)


def lm_diagonal(band, C, scale, min_diag, max_diag, previous=None):
    """Ceres' clamped diagonal, or the previous call's when it is reused (a rejected step: same Jacobian, another radius)."""
    if previous is not None:
        return np.array(previous, dtype=np.float64, copy=True)
    h = hdiag(band, C)
    return np.minimum(np.maximum(h * scale * scale, min_diag), max_diag)


class System:
    """M = S H S + diag(D2), rhs = -S g in band + arrow form (entries in float64 and in longdouble)."""
    DENSE_LIMIT = 2500     # unknowns up to which the factor is a dense Cholesky

    def __init__(self, band, Et, C, g, scale, diag, radius):
        band, Et, C, g, scale, diag = (np.asarray(v, dtype=np.float64) for v in (band, Et, C, g, scale, diag))
        self.Pb, self.W = band.shape
        self.hb, self.a = self.W - 1, C.shape[0]
        self.P = self.Pb + self.a
        Pb, hb = self.Pb, self.hb
        self.D2 = diag / radius
        sb, sa = scale[:Pb], scale[Pb:]
        Mb = np.zeros((Pb, self.W))
        for k in range(self.W):
            if Pb - k > 0:
                Mb[:Pb - k, k] = band[:Pb - k, k] * sb[:Pb - k] * sb[k:]
        Mb[:, 0] += self.D2[:Pb]
        self.Mb = Mb
        self.Mt = Et * sa[:, None] * sb[None, :]
        self.Mc = C * sa[:, None] * sa[None, :] + np.diag(self.D2[Pb:])
        self.rhs = -g * scale
        self.Mb_l, self.Mt_l, self.Mc_l, self.rhs_l = (v.astype(LD) for v in (self.Mb, self.Mt, self.Mc, self.rhs))
        self._factor = None

    # ---- products ------------------------------------------------------------------------------------------------------
    def matvec(self, x, dtype=LD):
        """M x, accumulated in `dtype` (longdouble by default)."""
        Mb, Mt, Mc = (self.Mb_l, self.Mt_l, self.Mc_l) if dtype is LD else (self.Mb, self.Mt, self.Mc)
        x = np.asarray(x).astype(dtype)
        Pb = self.Pb
        xb, xa = x[:Pb], x[Pb:]
        y = np.zeros(self.P, dtype=dtype)
        yb = y[:Pb]
        yb += Mb[:, 0] * xb
        for k in range(1, self.W):
            if Pb - k <= 0:
                break
            yb[k:] += Mb[:Pb - k, k] * xb[:Pb - k]
            yb[:Pb - k] += Mb[:Pb - k, k] * xb[k:]
        if self.a:
            yb += Mt.T @ xa
            y[Pb:] = Mt @ xb + Mc @ xa
        return y

    def residual(self, x):
        return self.rhs_l - self.matvec(x)

    def norm_inf(self):
        """||M||_inf (= ||M||_1: M is symmetric), in float64."""
        Pb, Mb = self.Pb, np.abs(self.Mb)
        rows = np.zeros(self.P)
        rows[:Pb] += Mb[:, 0]
        for k in range(1, self.W):
            if Pb - k <= 0:
                break
            rows[k:Pb] += Mb[:Pb - k, k]
            rows[:Pb - k] += Mb[:Pb - k, k]
        if self.a:
            rows[:Pb] += np.abs(self.Mt).sum(axis=0)
            rows[Pb:] += np.abs(self.Mt).sum(axis=1) + np.abs(self.Mc).sum(axis=1)
        return rows.max()

    def backward_error(self, x):
        """Normwise backward error ||M x - rhs||_inf / (||M||_inf ||x||_inf + ||rhs||_inf), residual in longdouble."""
        r = np.abs(self.residual(x)).max()
        return float(r / (LD(self.norm_inf()) * np.abs(np.asarray(x, dtype=LD)).max() + np.abs(self.rhs_l).max()))

    def dense(self):
        P, Pb = self.P, self.Pb
        M = np.zeros((P, P))
        for k in range(self.W):
            if Pb - k <= 0:
                break
            idx = np.arange(Pb - k)
            M[idx + k, idx] = self.Mb[:Pb - k, k]
            M[idx, idx + k] = self.Mb[:Pb - k, k]
        M[Pb:, :Pb] = self.Mt
        M[:Pb, Pb:] = self.Mt.T
        M[Pb:, Pb:] = self.Mc
        return M

    def zero_rows(self):
        """Rows of M that are exactly zero (a parameter no residual touches, undamped)."""
        nz = np.zeros(self.P, dtype=bool)
        Pb = self.Pb
        nz[:Pb] |= self.Mb[:, 0] != 0
        for k in range(1, self.W):
            if Pb - k <= 0:
                break
            c = self.Mb[:Pb - k, k] != 0
            nz[k:Pb] |= c
            nz[:Pb - k] |= c
        if self.a:
            nz[:Pb] |= (self.Mt != 0).any(axis=0)
            nz[Pb:] |= (self.Mt != 0).any(axis=1) | (self.Mc != 0).any(axis=1)
        return np.flatnonzero(~nz)

    # ---- factorisation -------------------------------------------------------------------------------------------------
    def _factorise(self):
        if self._factor is not None:
            return self._factor
        if self.P <= self.DENSE_LIMIT:
            self._factor = ("dense", sla.cho_factor(self.dense(), lower=True))
        else:
            Pb, a = self.Pb, self.a
            ab = np.zeros((self.W, Pb))          # scipy's lower banded storage: ab[k, j] = M(j + k, j)
            ab[:, :] = self.Mb.T
            cb = sla.cholesky_banded(ab, lower=True)
            Y = sla.cho_solve_banded((cb, True), self.Mt.T) if a else np.zeros((Pb, 0))   # B^-1 E
            S = self.Mc - self.Mt @ Y                                                       # Schur complement of the band
            self._factor = ("band", cb, Y, sla.cho_factor(S, lower=True) if a else None)
        return self._factor

    def _solve64(self, r):
        f = self._factorise()
        r = np.asarray(r, dtype=np.float64)
        if f[0] == "dense":
            return sla.cho_solve(f[1], r)
        _, cb, Y, Sf = f
        Pb = self.Pb
        zb = sla.cho_solve_banded((cb, True), r[:Pb])
        if Sf is None:
            return zb
        xa = sla.cho_solve(Sf, r[Pb:] - self.Mt @ zb)
        return np.concatenate([zb - Y @ xa, xa])

    def solve(self, refinements=3):
        """x* of M x = rhs: float64 factor, `refinements` (>= 2) rounds of refinement with longdouble residuals."""
        x = self._solve64(self.rhs).astype(LD)
        for _ in range(max(refinements, 2)):
            x = x + self._solve64(self.residual(x)).astype(LD)
        return x.astype(np.float64)

    def cond1(self):
        """Estimate of kappa_1(M) = ||M||_1 ||M^-1||_1 (onenormest of the inverse through the host factor)."""
        op = LinearOperator((self.P, self.P), matvec=self._solve64, rmatvec=self._solve64, dtype=np.float64)
        if self.P <= 4:
            inv = np.column_stack([self._solve64(e) for e in np.eye(self.P)])
            return self.norm_inf() * np.abs(inv).sum(axis=0).max()
        return self.norm_inf() * onenormest(op)


def from_step(out, radius, min_diag, max_diag, jacobi=True, previous_diag=None):
    """Host scale, diag and the System for what oicc_debug_lm_step read (`out`: estimator.DebugLmStep's dict)."""
    scale = jacobi_scale(out["band"], out["C"], jacobi)
    diag = lm_diagonal(out["band"], out["C"], scale, min_diag, max_diag, previous_diag)
    return scale, diag, System(out["band"], out["Et"], out["C"], out["g"], scale, diag, radius)
