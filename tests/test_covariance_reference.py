"""The covariance reference (tests/covariance_reference.py) itself, on the CPU checker's J^T J of `tiny`: no device needed."""
import numpy as np

import covariance_reference as CR
import normal_equations_cases as cases
import oracle_backend
from openimucameracalibrator_amd import synthetic, estimator as E

# Standard deviations sqrt(diag((J^T J)^-1)) of the arrow of `tiny` under FLAGS1 at the start point (BatchInitSpline), not
# multiplied by the variance factor: T_i_c upsilon | omega | gravity.  Recorded from this reference on the checker's H.
TINY_FLAGS1_ARROW_STD = np.array([
    0.014009322761677776, 0.01662302770885298, 0.01084378644158827,
    0.022631598655308463, 0.025049052966232596, 0.03291777556830337,
    0.269999624371315, 0.27267065625832193, 0.023924510709920542])


def _tiny_H(flags):
    cal = E.ImuCameraCalibrator(backend=oracle_backend.load()).BatchInitSpline(synthetic.make_config("tiny"))
    lay = cal.trajectory_.GetTangentLayout(flags)
    _, H, _ = cal.trajectory_.Evaluate(flags)
    return H, lay


def test_reference_inverse_of_tiny():
    H, lay = _tiny_H(cases.FLAGS1)
    Pb = int(lay["other"][0])
    assert H.shape == (138, 138) and Pb == 129
    ref = CR.invert(H)
    assert ref.residual < 1e-17 * ref.kappa1, (ref.residual, ref.kappa1)
    assert float(np.abs(ref.Zs - ref.Zs.T).max()) <= 1e-12 * float(np.abs(ref.Zs).max())
    assert 4e-6 < ref.lambda_min < 6e-6 and ref.lambda_min <= ref.rcond <= 138 * ref.lambda_min    # 5.2e-6, 8.3e-6
    std = CR.arrow_std(ref, Pb)
    assert np.all(np.abs(std - TINY_FLAGS1_ARROW_STD) <= 1e-6 * TINY_FLAGS1_ARROW_STD), std


def test_reference_needs_the_unit_diagonal():
    """`tiny` at 3 s: the unscaled J^T J has a diagonal entry ~1e-21 next to ~1e10; scaled to unit diagonal it is well conditioned."""
    cal = E.ImuCameraCalibrator(backend=oracle_backend.load()).BatchInitSpline(synthetic.make_config("tiny", duration=3.0, num_views=30))
    _, H, _ = cal.trajectory_.Evaluate(cases.ALL)
    d = np.diag(H)
    assert d.min() > 0 and d.max() / d.min() > 1e25
    ref = CR.invert(H)
    assert ref.kappa1 < 1e9 and ref.residual < 1e-17 * ref.kappa1
    assert ref.lambda_min <= ref.rcond <= H.shape[0] * ref.lambda_min
