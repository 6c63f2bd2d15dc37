"""The Allan variance on the MI355X (csrc/allan.hip: allan_scan_kernel, allan_partial_kernel, allan_reduce_kernel) against the exact
reference tests/allan_exact.py, at the sizes where the launch geometry changes: one scan pass of 8192 and one sample more, the
carry over three passes, factor groups of 256, of a count that is no power of two and of one, a span of exactly 1024, 0 to 3
chunks of 16384, one chunk plus one term, a factor with one term and with none, late members of a group without a term in a tile
its first member still has.  Inputs carry gravity, a 150 m/s^2 and a 0.5 rad/s channel; every factor of every channel is held to
B_m (allan_exact's docstring), which tests/test_allan_exact.py holds below 1e-10 and a float64 emulation of the scan order meets
at 0.044 at most.  Largest error / B_m of the device on the MI355X: 0.044 as well (n32769, gyr_x, the one-term factor 16384), 0.032
or less elsewhere."""
import numpy as np
import pytest

import allan_exact as X
from openimucameracalibrator_amd import allan as A

pytestmark = pytest.mark.gpu
SCALE = np.array([1.0, 1.0, 1.0, A.GYRO_SCALE, A.GYRO_SCALE, A.GYRO_SCALE])


@pytest.fixture(scope="module")
def reference():
    """The exact values per case, computed once (allan_exact caches them) and never written to."""
    return X.case_reference


def check(v, ref, channel_map, label, capsys):
    fac = ref["fac"]
    np.testing.assert_array_equal(v["factors"], fac)
    np.testing.assert_array_equal(v["taus"], fac * ref["period"])
    assert v["freq"] == ref["freq"] and v["period"] == ref["period"]
    np.testing.assert_array_equal(v["mean"], [ref["mean"][c] for c in channel_map])
    no_term = ref["n"] - 2 * fac <= 0
    assert v["sigma2"].shape == (len(channel_map), len(fac))
    assert (np.isnan(v["sigma2"]) == no_term[None, :]).all()
    r = X.ratios(v["sigma2"], ref, channel_map)
    worst = np.nanmax(r)
    row, f = np.unravel_index(np.nanargmax(r), r.shape)
    with capsys.disabled():
        print("\n  %s: largest error / B_m %.3g at channel %d, factor %d (B_m %.2e)" % (label, worst, channel_map[row], fac[f], ref["B"][channel_map[row], f]))
    bad = np.argwhere(r > 1.0)
    assert len(bad) == 0, (label, worst, [(channel_map[i], int(fac[j]), r[i, j]) for i, j in bad[:8]])


@pytest.mark.parametrize("name", sorted(X.CASES))
def test_every_factor_of_every_channel_within_the_bound(name, reference, capsys):
    assert np.array_equal(SCALE, X.SCALE)
    ref = reference(name)
    v = A.allan_variance(ref["w"], ref["t"], SCALE, ref["clusters"])
    check(v, ref, list(range(6)), name, capsys)
    if name in X.REPEAT_CASES:
        again = A.allan_variance(ref["w"], ref["t"], SCALE, ref["clusters"])
        assert again["sigma2"].tobytes() == v["sigma2"].tobytes()


def test_one_channel_and_seven(reference, capsys):
    ref = reference("n8193")
    six = A.allan_variance(ref["w"], ref["t"], SCALE, ref["clusters"])["sigma2"]
    c = X.GYRO_BIAS_CHANNEL
    one = A.allan_variance(ref["w"][c:c + 1], ref["t"], SCALE[c:c + 1], ref["clusters"])
    check(one, ref, [c], "n8193, 1 channel", capsys)
    assert one["sigma2"][0].tobytes() == six[c].tobytes()
    c = X.ACC_OFFSET_CHANNEL
    cm = list(range(6)) + [c]
    seven = A.allan_variance(ref["w"][cm], ref["t"], SCALE[cm], ref["clusters"])
    check(seven, ref, cm, "n8193, 7 channels", capsys)
    assert seven["sigma2"][6].tobytes() == seven["sigma2"][c].tobytes()
    assert seven["sigma2"][:6].tobytes() == six.tobytes()
