"""The host reference of the damped LM solve (tests/lm_step_reference.py) against mpmath at 50 digits: the solve with its
refinement, the kappa_1 estimate, the Jacobi scaling, the clamped diagonal and its reuse -- on random SPD band + arrow systems of a
few dozen unknowns whose half bandwidth and arrow width cross 0, 1 and 16.  The GPU tests of the linear solvers
(test_gpu_linear_solve_reference.py) rest on this reference."""
import mpmath
import numpy as np
import pytest

import lm_step_reference as R

mpmath.mp.dps = 50


def random_system(rng, Pb, hb, a, cond_spread=1e6):
    """A random SPD matrix of band + arrow structure, packed as the library packs H, with the gradient."""
    P = Pb + a
    B = np.zeros((P, P))
    for i in range(Pb):
        for j in range(max(0, i - hb), i + 1):
            B[i, j] = rng.standard_normal()
    B[Pb:, :] = rng.standard_normal((a, P))
    d = np.exp(rng.uniform(0, np.log(cond_spread), P))        # rows of very different scale, as a spline's knots and T_i_c have
    H = (B @ B.T + np.diag(np.abs(rng.standard_normal(P)) + 0.1)) * np.sqrt(d)[:, None] * np.sqrt(d)[None, :]
    # keep the band structure exact: B B^T of a lower band matrix is a band of the same width only up to hb; clear the rest
    for i in range(Pb):
        for j in range(Pb):
            if abs(i - j) > hb:
                H[i, j] = 0.0
    H += np.diag(np.abs(H).sum(axis=1))                        # diagonally dominant after the clearing: SPD
    band = np.zeros((Pb, hb + 1))
    for j in range(Pb):
        for k in range(hb + 1):
            if j + k < Pb:
                band[j, k] = H[j + k, j]
    return band, H[Pb:, :Pb].copy(), H[Pb:, Pb:].copy(), rng.standard_normal(P) * np.sqrt(d), H


def mp_matrix(S):
    return mpmath.matrix(S.dense().tolist())


@pytest.mark.parametrize("hb", [0, 1, 16])
@pytest.mark.parametrize("a", [0, 1, 16])
def test_solve_matches_mpmath(hb, a):
    rng = np.random.RandomState(100 * hb + a)
    Pb = 40 if hb < 16 else 48
    band, Et, C, g, H = random_system(rng, Pb, hb, a)
    scale = R.jacobi_scale(band, C)
    diag = R.lm_diagonal(band, C, scale, 1e-6, 1e32)
    S = R.System(band, Et, C, g, scale, diag, 1e4)
    x = S.solve()
    M = mp_matrix(S)
    rhs = mpmath.matrix((-g * scale).tolist())
    xs = mpmath.lu_solve(M, rhs)
    xs = np.array([float(v) for v in xs])
    assert np.abs(x - xs).max() <= 4 * R.EPS * np.abs(xs).max(), (np.abs(x - xs).max() / np.abs(xs).max())
    # the exact solution's backward error is at the rounding of the float64 entries; the reference's is as small
    assert S.backward_error(x) < 2 * R.EPS
    # kappa_1: onenormest is a lower bound, and on these sizes (nearly) exact
    Minv = mpmath.inverse(M)
    k_exact = float(mpmath.mnorm(M, 1) * mpmath.mnorm(Minv, 1))
    k_est = S.cond1()
    assert k_exact / 3 <= k_est <= k_exact * (1 + 1e-10), (k_est, k_exact)
    # the band + arrow matrix-vector product against mpmath
    y = S.matvec(x)
    ym = M * mpmath.matrix(x.tolist())
    assert max(abs(float(y[i]) - float(ym[i])) for i in range(S.P)) <= 1e-17 * float(mpmath.mnorm(ym, "inf")) + 1e-300


def test_large_band_path_matches_dense():
    """The banded factor with the arrow's Schur complement (systems above 2500 unknowns) against the dense factor."""
    rng = np.random.RandomState(7)
    band, Et, C, g, _ = random_system(rng, 60, 5, 7)
    scale = R.jacobi_scale(band, C)
    diag = R.lm_diagonal(band, C, scale, 1e-6, 1e32)
    S1 = R.System(band, Et, C, g, scale, diag, 1e2)
    S2 = R.System(band, Et, C, g, scale, diag, 1e2)
    xd = S1.solve()
    S2.DENSE_LIMIT = 0
    S2._factorise()
    assert S2._factor[0] == "band"
    xb = S2.solve()
    assert np.abs(xb - xd).max() <= 4 * R.EPS * np.abs(xd).max()
    assert 1 / 3 < S2.cond1() / S1.cond1() < 3      # (two runs of a randomised estimator)


def test_scaling_clamps_and_reuse_match_mpmath():
    rng = np.random.RandomState(3)
    band, Et, C, g, _ = random_system(rng, 30, 3, 4, cond_spread=1e12)
    h = R.hdiag(band, C)
    for jacobi in (True, False):
        scale = R.jacobi_scale(band, C, jacobi)
        ref = [1 / (1 + mpmath.sqrt(mpmath.mpf(v))) if jacobi else mpmath.mpf(1) for v in h]
        assert all(abs(float(r) - s) <= 0.5 * abs(float(r)) * R.EPS * 2 for r, s in zip(ref, scale))
        v = np.sort(h * scale * scale)
        lo, hi = v[len(v) // 4], v[3 * len(v) // 4]          # both clamps engage on a quarter of the rows each
        diag = R.lm_diagonal(band, C, scale, lo, hi)
        want = [min(max(mpmath.mpf(hv) * mpmath.mpf(s) ** 2, mpmath.mpf(lo)), mpmath.mpf(hi)) for hv, s in zip(h, scale)]
        assert all(abs(float(w) - d) <= 2 * R.EPS * abs(float(w)) for w, d in zip(want, diag))
        assert (diag == lo).sum() >= len(h) // 4 and (diag == hi).sum() >= len(h) // 4
        # reuse: the previous call's diagonal as it is, whatever the clamps now say
        again = R.lm_diagonal(band, C, scale, 0.0, 1e300, previous=diag)
        assert np.array_equal(again, diag) and again is not diag
        S = R.System(band, Et, C, g, scale, diag, 0.5e4)
        assert np.array_equal(S.D2, diag / 0.5e4)
        M = mp_matrix(S)
        for i in range(S.P):        # the damped diagonal entry is (s_i h_ii s_i) + d_i / radius
            want_ii = mpmath.mpf(h[i]) * mpmath.mpf(scale[i]) ** 2 + mpmath.mpf(diag[i]) / mpmath.mpf(0.5e4)
            assert abs(float(M[i, i]) - float(want_ii)) <= 2 * R.EPS * abs(float(want_ii))


def test_zero_rows_are_found():
    rng = np.random.RandomState(5)
    band, Et, C, g, _ = random_system(rng, 20, 2, 3)
    band[7, :] = 0.0; band[6, 1] = 0.0; band[5, 2] = 0.0; Et[:, 7] = 0.0
    scale = R.jacobi_scale(band, C)
    diag = R.lm_diagonal(band, C, scale, 0.0, 1e32)
    S = R.System(band, Et, C, g, scale, diag, 1e4)
    assert list(S.zero_rows()) == [7]
