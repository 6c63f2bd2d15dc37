"""Reference of the covariance estimate (oicc_estimate_covariance), host only: the inverse of the dense J^T J that Evaluate(flags)
returns, in extended precision.

H is scaled to unit diagonal in np.longdouble, Hs = S H S with s_i = H_ii^-1/2 -- the same scaling the device applies; without it
the matrix of `tiny` at 3 s has cond ~ 2e25 and no fp64 inverse means anything --, inverted in float64 and refined by Newton's
iteration Z <- Z (2 I - Hs Z) in np.longdouble until ||Hs Z - I||_inf < 1e-17 kappa_1(Hs).  The iteration converges quadratically
from any start with ||I - Hs Z0|| < 1, which the float64 inverse gives for kappa eps_64 << 1 (the largest kappa of the test cases
is 6.5e7); its fixed point is limited by the rounding of the longdouble products, about P eps_ld kappa, under the target.
"""
import dataclasses

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


@dataclasses.dataclass
class Reference:
    Zs: np.ndarray        # [P, P] longdouble, (S H S)^-1
    s: np.ndarray         # [P] longdouble, H_ii^-1/2
    kappa1: float         # ||Hs||_1 ||Zs||_1
    lambda_min: float     # smallest eigenvalue of Hs (float64 eigvalsh: absolute error ~ P eps)
    rcond: float          # 1 / max_i Zs_ii
    residual: float       # ||Hs Zs - I||_inf
    iterations: int

    def covariance(self):
        """cov = S Zs S, longdouble."""
        return (self.Zs * self.s[:, None]) * self.s[None, :]


def scaled(H):
    H = np.asarray(H, dtype=np.float64)
    d = np.diag(H).astype(LD)
    assert np.all(d > 0), "a diagonal entry of J^T J is not positive"
    s = 1 / np.sqrt(d)
    return (H.astype(LD) * s[:, None]) * s[None, :], s


def invert(H, max_iterations=12):
    Hs, s = scaled(H)
    P = Hs.shape[0]
    eye = np.eye(P, dtype=LD)
    Z = np.linalg.inv(Hs.astype(np.float64)).astype(LD)
    Z = (Z + Z.T) / 2
    norm1 = lambda A: float(np.abs(A).sum(axis=0).max())
    norminf = lambda A: float(np.abs(A).sum(axis=1).max())
    kappa = norm1(Hs) * norm1(Z)
    res, it = np.inf, 0
    for it in range(max_iterations + 1):
        R = eye - Hs @ Z
        res = norminf(R)
        if res < 1e-17 * kappa or it == max_iterations:
            break
        Z = Z + Z @ R
    # (no symmetrisation at the end: Z is an accurate RIGHT inverse, ||Z - Hs^-1|| <= ||Z|| ||R||, while Z^T Hs - I can be kappa times
    # larger than R; averaging the two would bring that in)
    kappa = norm1(Hs) * norm1(Z)
    lam = float(np.linalg.eigvalsh(Hs.astype(np.float64))[0])
    return Reference(Zs=Z, s=s, kappa1=kappa, lambda_min=lam, rcond=float(1 / np.diag(Z).max()), residual=norminf(eye - Hs @ Z), iterations=it)


def arrow_std(ref, Pb):
    """Standard deviations of the arrow columns: sqrt of the diagonal of the unscaled covariance."""
    c = np.diag(ref.covariance())[Pb:]
    return np.sqrt(c).astype(np.float64)
