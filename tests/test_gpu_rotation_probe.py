"""One probe of the gyroscope-to-camera rotation search on the device (csrc/rotation_init.hip: rot_moments_kernel, the host Kabsch
step, rot_error_kernel) against the 50-digit restatement tests/rotation_probe_restatement.py, through the debug entry
oicc_debug_rotation_probe -- the same RotationProbe object the calibration entry drives.  Bound: DEVICE_FACTOR (64) x the float64
yardstick of the case's class, each quantity on its natural scale.  The end-to-end test (tests/test_rotation_init.py) only needs
`fc < fd` to come out the same way some 20 times; here the 15 moments, R, the bias and the error of single probes are compared at the
edges: block boundaries (n = 255 / 256 / 257), the grid-stride loop (grid_cap 1 / 2), exact ties, held and extrapolated samples,
the Huber switch, rank-deficient cross-covariances (where R is not unique: a rotation, and a finite error)."""
import ctypes as C

import numpy as np
import pytest

import rotation_probe_restatement as P

DP = C.POINTER(C.c_double)


def device_probe(ts, imu, vis, tds, estimate_bias, grid_cap):
    from openimucameracalibrator_amd import _lib
    fn = _lib.load().lib.oicc_debug_rotation_probe
    fn.restype = C.c_int
    fn.argtypes = [C.c_int32, C.c_int64, DP, DP, DP, C.c_int32, DP, C.c_int32, C.c_int32, DP, DP, DP, DP]
    ts = np.ascontiguousarray(ts, dtype=np.float64); imu = np.ascontiguousarray(imu, dtype=np.float64); vis = np.ascontiguousarray(vis, dtype=np.float64)
    tds = np.ascontiguousarray(tds, dtype=np.float64); k = len(tds)
    m = np.full((k, 15), np.nan); R = np.full((k, 3, 3), np.nan); b = np.full((k, 3), np.nan); e = np.full(k, np.nan)
    rc = fn(0, len(ts), ts.ctypes.data_as(DP), imu.ctypes.data_as(DP), vis.ctypes.data_as(DP), k, tds.ctypes.data_as(DP), int(estimate_bias), grid_cap,
            m.ctypes.data_as(DP), R.ctypes.data_as(DP), b.ctypes.data_as(DP), e.ctypes.data_as(DP))
    assert rc == 0, rc
    return m, R, b, e


@pytest.mark.gpu
@pytest.mark.parametrize("grid_cap", [0, 1, 2])
@pytest.mark.parametrize("estimate_bias", [True, False])
@pytest.mark.parametrize("name", sorted(P.SERIES))
def test_probe_against_the_restatement(name, estimate_bias, grid_cap, capsys):
    kind, n, _, tds = P.SERIES[name]
    ts, imu, vis = P.series(name)
    m, R, b, e = device_probe(ts, imu, vis, tds, estimate_bias, grid_cap)
    lines = []
    for i, td in enumerate(tds):
        cls = dict(P.TDS)[td]
        ref = P.restated(name, td)
        err = P.errors(ref, m[i], R[i], b[i], e[i], estimate_bias)
        yard = P.YARDSTICK[(kind, cls)]
        lines.append("  %s td %-9g bias %d cap %d: " % (name, td, estimate_bias, grid_cap) + ", ".join("%s %.2e (%.1f x)" % (q, v, v / yard[q]) for q, v in err.items()))
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    for i, td in enumerate(tds):
        cls = dict(P.TDS)[td]
        ref = P.restated(name, td)
        yard = P.YARDSTICK[(kind, cls)]
        for q, v in P.errors(ref, m[i], R[i], b[i], e[i], estimate_bias).items():
            assert v <= P.DEVICE_FACTOR * yard[q], (name, td, estimate_bias, grid_cap, q, v, yard[q])
        # always: R is a rotation, the error is finite and not negative, no bias where none is asked for
        assert np.abs(R[i] @ R[i].T - np.eye(3)).max() <= 1e-13 and abs(np.linalg.det(R[i]) - 1.0) <= 1e-13, (name, td, R[i])
        assert np.isfinite(e[i]) and e[i] >= 0.0
        if not estimate_bias:
            assert not b[i].any()
        assert ("R" in ref) == P.restate_R(name, td)


@pytest.mark.gpu
def test_calibration_entry_runs_the_same_probe():
    """The golden-section search of the calibration entry, replayed on the host with the debug probe on the library's own
    prepared series: same iteration count, same offset, the error and the bias of its last better probe bit for bit (one code path
    behind both doors)."""
    from openimucameracalibrator_amd import rotation_init as RI
    tv, qv, ti, gy, dt = P.PREPARE_CASES["cam30_starts_later"]
    r = RI.estimate_camera_imu_rotation(tv, qv, ti, gy, dt, True)
    rc, n, tI, sI, sV = P.library_prepare(tv, qv, ti, gy, dt)
    assert rc == 0
    g = (1.0 + np.sqrt(5.0)) / 2.0
    a, b = -1.0, 1.0
    c, d = b - (b - a) / g, a + (b - a) / g
    it, error, bias = 0, 0.0, np.zeros(3)
    while abs(c - d) > 1e-4:
        m, R, bb, e = device_probe(tI, sI, sV, [c, d], True, 0)
        if e[0] < e[1]:
            b, error, bias = d, e[0], bb[0]
        else:
            a, error, bias = c, e[1], bb[1]
        c, d = b - (b - a) / g, a + (b - a) / g
        it += 1
    assert it == r["iterations"] and (a + b) / 2.0 == r["time_offset"]
    assert error == r["error"] and np.array_equal(bias, r["gyro_bias"])
