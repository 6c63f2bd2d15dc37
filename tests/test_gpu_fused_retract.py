"""The retraction inside the last launch of the cyclic-reduction solve (kernels_bcr.hip: bcri_backward2_retract_kernel) against the
stand-alone retraction kernel (kernels_solve.hip: lm_retract_kernel) on the SAME step, through estimator.DebugLmRetract
(oicc_debug_lm_retract): both are the functions of lm_retract.h on the same inputs, so every candidate parameter agrees bit for bit.

The read-out fills the candidate buffer with 0xff bytes before each of the two retractions: an entry that a retraction did not write
reads back as that NaN pattern.  Comparing the two candidate buffers as 64-bit integers therefore checks at once that every active
entry agrees in every bit, that every inactive entry is untouched by both, and that the fused launch leaves nothing poisoned that the
stand-alone kernel writes: every active block has AT LEAST one owner among the workgroups.  That none has two is checked through
the scalars only -- sums over the owners, so a block retracted and counted twice shows there; a block written twice with the same
bits but counted once would not show, and rests on the ownership argument in kernels_bcr.hip.
The fall-back cases (fewer than three levels, band sweep, option off) compare the loop's call of the stand-alone kernel with the
read-out's own call of it: they show that the fall-back is taken and written completely, not more.

Block counts: those of tests/test_gpu_bcr_end_pivots.py from 6 blocks on -- a left-end orphan (13, 29, 33), an upper pivot without a
left child (14, 30), a two-pivot top (6, 7, 13, 29), a power of two (32) -- and n = 29 with the bias knots free (IMU_BIASES:
arrow-resident knots with the box projection, all in workgroup 0).  The retraction rides in the solve's last launch where the plan
(test_bcr_plan.plan) has at least three levels, so that this launch is the two-level back substitution on the levels (1, 0): every
count here but 6 and 7, whose plans have two levels (6 -> 3 -> 1) and end with the one-level kernel -- those two keep the separate
launch, and the comparison then checks the loop's way of calling it."""
import numpy as np
import pytest

import test_gpu_linear_solve_reference as L
from test_bcr_plan import plan
from openimucameracalibrator_amd import synthetic, estimator as E

pytestmark = pytest.mark.gpu

F = L.F
CASES = [(3.5, 6, F), (4.25, 7, F), (6.5, 10, F), (8.6, 13, F), (9.25, 14, F), (20.0, 29, F), (20.75, 30, F), (21.5, 31, F), (22.1, 32, F),
         (22.75, 33, F), (20.0, 29, F | E.IMU_BIASES)]
IDS = ["n%d%s" % (c[1], "_biases" if c[2] != F else "") for c in CASES]
POISON = np.uint64(0xFFFFFFFFFFFFFFFF)

# Relative deviation |device - reference| / |reference| of LmState's three scalars from a np.longdouble recomputation
# (reference_scalars below).  Measured on an MI355X over CASES at radius 1e4: the stand-alone kernel's largest deviation was 3.08e-16
# (step_norm_sq at n = 13; 2.88e-16 over a second pass with fused_retract = 0; its atomics land in any order, so the last bit moves
# from run to run), the fused launch's 2.0e-16 (step_norm_sq at n = 29).  The bound is twice the stand-alone kernel's figure.
STANDALONE_MAX_REL = 3.08e-16
TOL = 2.0 * STANDALONE_MAX_REL


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def reference_scalars(out, xc):
    """[model_cost_change, step_norm_sq, x_norm_sq] in np.longdouble from what the device read (step_s, scale, D2, g, x) and the
    candidate it wrote (the entries that are not poison: the active ones)."""
    ld = np.longdouble
    d, sc, D2, g = (out[k].astype(ld) for k in ("step_s", "scale", "D2", "g"))
    active = bits(xc) != POISON
    x0 = out["x"][active].astype(ld); x1 = xc[active].astype(ld)
    return np.array([(ld(0.5) * d * (D2 * d - g * sc)).sum(), ((x1 - x0) ** 2).sum(), (x0 ** 2).sum()], dtype=ld)


def rel_dev(s, out, xc):
    ref = reference_scalars(out, xc)
    return np.array([float(abs(s[k].astype(np.longdouble) - ref[k]) / abs(ref[k])) for k in range(3)])


def run(duration, n, flags, **opts):
    tr = L.calibrator(L.dataset(duration), **opts).trajectory_
    out = tr.DebugLmRetract(flags, 1e4)
    assert out["n"] == n, (out["n"], n)
    return tr, out


def check_same_candidate(out):
    loop, alone = bits(out["xc_loop"]), bits(out["xc_alone"])
    written = alone != POISON
    assert written.any() and not written.all()                      # the knots outside the problem's time span, fixed blocks: inactive
    assert np.array_equal(loop != POISON, written)                  # same set of entries written: nothing active left poisoned, nothing inactive touched
    assert np.array_equal(loop, alone)                              # every bit
    assert np.all(np.isfinite(out["xc_alone"][written]))


@pytest.mark.parametrize("duration,n,flags", CASES, ids=IDS)
def test_fused_retraction_is_the_standalone_kernel_bit_for_bit(duration, n, flags):
    """Candidate parameters: every bit, the same set of entries written.  Scalars: within TOL of the np.longdouble recomputation
    (measured on an MI355X: stand-alone kernel at most 3.08e-16, fused launch at most 2.0e-16; TOL = 6.16e-16)."""
    fused = len(plan(n)[0]) >= 3                                    # the last launch is the two-level back substitution on the levels (1, 0)
    assert fused == (n >= 8)
    tr, out = run(duration, n, flags)
    assert out["fused"] == fused
    check_same_candidate(out)
    dev_alone = rel_dev(out["s_alone"], out, out["xc_alone"]); dev_loop = rel_dev(out["s_loop"], out, out["xc_loop"])
    print("n=%d flags=%d  stand-alone rel dev %s   fused rel dev %s" % (n, flags, dev_alone, dev_loop))
    assert np.all(dev_loop <= TOL), (dev_loop, dev_alone)
    # a second call over the same buffers (the step of the first still in the workspace): the same again
    out2 = tr.DebugLmRetract(flags, 1e9)
    assert out2["fused"] == fused
    check_same_candidate(out2)
    assert np.all(rel_dev(out2["s_loop"], out2, out2["xc_loop"]) <= TOL)


def test_the_standalone_kernel_is_within_the_bound():
    """The kernel the bound was measured on (STANDALONE_MAX_REL, doubled: its atomics land in any order) stays within it."""
    worst = 0.0
    for duration, n, flags in CASES:
        _, out = run(duration, n, flags, fused_retract=0)
        assert not out["fused"]
        check_same_candidate(out)                                   # (both ways ARE the stand-alone kernel here)
        worst = max(worst, rel_dev(out["s_alone"], out, out["xc_alone"]).max(), rel_dev(out["s_loop"], out, out["xc_loop"]).max())
    print("stand-alone kernel, largest relative deviation: %.3e" % worst)
    assert worst <= TOL


@pytest.mark.parametrize("duration,n,opts", [(1.2, 3, {}), (20.0, 29, dict(solver_algorithm=1)), (20.0, 29, dict(fused_retract=0))],
                         ids=["n3", "band_sweep", "option_off"])
def test_fall_backs_keep_the_separate_launch(duration, n, opts):
    """Fewer than three levels, a band-sweep route, or the option off: the loop retracts through lm_retract_kernel, same bits."""
    for flags in (F, F | E.IMU_BIASES):
        _, out = run(duration, n, flags, **opts)
        assert not out["fused"]
        check_same_candidate(out)
        assert np.all(rel_dev(out["s_loop"], out, out["xc_loop"]) <= TOL)


@pytest.mark.parametrize("flags", [F, F | E.IMU_BIASES], ids=["stage1", "biases"])
def test_full_calibration_is_the_same_with_and_without_the_fused_retraction(flags):
    """Optimize on C2 with fused_retract 0 / 1 under the device-side and the host-driven loop: same iteration counts and termination,
    final cost to the tolerance of test_gpu_parity.py::test_device_side_lm_control_takes_the_steps_of_the_host_loop."""
    ds = synthetic.make_config("C2")
    runs = {}
    for dev in (1, 0):
        for fused in (0, 1):
            tr = E.ImuCameraCalibrator().BatchInitSpline(ds).trajectory_
            tr.SetOption("device_lm", dev); tr.SetOption("fused_retract", fused)
            s = tr.Optimize(50, flags)
            runs[(dev, fused)] = (s, tr.GetIterations(), tr.GetT_i_c())
    ref = runs[(0, 0)]
    for key, (s, its, tic) in runs.items():
        for k in ("termination", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "message"):
            assert s[k] == ref[0][k], (key, k, s, ref[0])
        assert abs(s["final_cost"] - ref[0]["final_cost"]) <= 1e-12 * ref[0]["initial_cost"] + 1e-11 * ref[0]["final_cost"], (key, s, ref[0])
        assert len(its) == len(ref[1])
        for a, b in zip(its, ref[1]):
            assert a["iteration"] == b["iteration"] and a["step_is_successful"] == b["step_is_successful"], (key, a, b)
            assert abs(a["step_norm"] - b["step_norm"]) <= 1e-7 * max(b["step_norm"], 1e-12), (key, a, b)
        assert np.abs(tic - ref[2]).max() < 1e-9
