"""CPU tests of tests/rotation_probe_restatement.py: the 50-digit restatement of one probe of the gyroscope-to-camera rotation
search against planted values and against the reference's literal scan, its conditions per case, the float64 yardsticks (a fresh
measurement within [1/8, 1] of every recorded figure), planted defects -- and the HOST PREPARATION of the device path
(prepare_rotation_series of csrc/rotation_init.hip through the debug export oicc_debug_rotation_prepare, which needs no device)
against its restatement.  The device comparison of the probe is tests/test_gpu_rotation_probe.py."""
import ctypes as C

import mpmath as mp
import numpy as np
import pytest

import rotation_probe_restatement as P
from rotation_probe_restatement import O

DP = C.POINTER(C.c_double)


def test_nearest_sample_rule_and_window_scan():
    grid = [mp.mpf(x) for x in (0.0, 1.0, 2.0, 4.0)]
    got = [P.nearest_first(grid, mp.mpf(t))[:2] for t in (-1.0, 0.4, 0.5, 0.6, 3.0, 9.0)]
    assert [k for k, _ in got] == [0, 0, 0, 1, 2, 3] and [float(d) for _, d in got] == [1.0, 0.4, 0.5, 0.4, 1.0, 5.0]   # ties: the earlier sample
    assert P.nearest_first(grid, mp.mpf(0.5))[2] == 0 and P.nearest_first(grid, mp.mpf(3.0))[2] == 0 and P.nearest_first(grid[:1], mp.mpf(3.0))[2] is None
    # the windowed scan of `resample` equals the reference's scan over every sample
    for name in ("rank3_n16", "rank3_n257"):
        ts, imu, vis = P.series(name)
        for td, cls in P.TDS:
            ks = P.restated(name, td)["ks"]
            with mp.workdps(P.DPS):
                shifted = [mp.mpf(float(x)) - mp.mpf(float(td)) for x in ts]
                assert ks == [P.nearest_first(shifted, mp.mpf(float(t)))[0] for t in ts], (name, td)


def test_probe_recovers_planted_values():
    rng = np.random.default_rng(5)
    ts = np.arange(64) / P.RATE
    imu = rng.standard_normal((64, 3))
    R0 = P._rot(P.Q_IC); b0 = np.array([0.1, -0.2, 0.3])
    vis = imu @ R0.T + b0
    ref = P.probe(ts, imu, vis, 0.0)
    assert max(abs(float(ref["R"][r, c]) - R0[r, c]) for r in range(3) for c in range(3)) < 1e-14
    assert max(abs(float(ref[("bias", True)][r]) - b0[r]) for r in range(3)) < 1e-14 and float(ref[("err", True)]) < 1e-27
    assert ref["held"] == 1 and all(f == 0 for f in ref["fs"])                 # td = 0: every sample meets itself; the last one is held
    # a reflection is refused: C(2,2) = -1 gives det R = +1
    ref = P.probe(ts, imu, imu * np.array([1.0, 1.0, -1.0]), 0.0)
    with mp.workdps(P.DPS):
        assert abs(mp.det(ref["R"]) - 1) < mp.mpf(10) ** -40
    # the tie rule and the blend towards k + 1 from the nearest sample: td = 1/512 averages each sample with its successor
    ref = P.probe(ts, imu, vis, 1.0 / 512.0, exact_ties=True)
    assert ref["ks"] == list(range(64)) and all(f == mp.mpf(1) / 2 for f in ref["fs"][:-1]) and ref["held"] == 1
    with mp.workdps(P.DPS):
        assert all(ref["q"][i][c] == (mp.mpf(vis[i, c]) + mp.mpf(vis[i + 1, c])) / 2 for i in range(63) for c in range(3))
    # td = -1: every sample is extrapolated backwards from the first pair, f = (1 - t) 256 up to 256
    ref = P.probe(ts, imu, vis, -1.0, want_R=False)
    assert set(ref["ks"]) == {0} and ref["fs"][0] == 256 and ref["held"] == 0
    # td = +1: every sample takes the last one as it is
    ref = P.probe(ts, imu, vis, 1.0, want_R=False)
    assert ref["held"] == 64 and all(ref["A"][r, c] == 0 for r in range(3) for c in range(3))


def test_cases_meet_their_conditions_and_reach_the_edges():
    assert sorted({v[1] for v in P.SERIES.values()}) == [16, 255, 256, 257, 600]
    restated_R = 0
    for name, (kind, n, _, tds) in P.SERIES.items():
        for td in tds:
            ref = P.restated(name, td)             # asserts the conditions of the case
            assert ("R" in ref) == P.restate_R(name, td)
            restated_R += "R" in ref
            if not P.restate_R(name, td) and kind != "axis":
                with mp.workdps(P.DPS):
                    s = mp.svd_r(ref["A"], compute_uv=False)
                    assert s[1] <= mp.mpf(10) ** -40 * max(s[0], 1), (name, td)     # rank <= 1: no unique rotation
    assert restated_R == 31          # of 48 (series, offset) pairs; the others are property-only
    assert P.restated("rank3_n600", 1.0)["held"] > 200 and P.restated("rank3_n256", 1.0)["held"] == 256
    assert max(P.restated("rank3_n600", -1.0)["fs"]) == 256 and max(P.restated("rank3_n600", -0.4)["fs"]) > 100
    assert not P.restate_R("rank3_n256", 1.0) and not P.restate_R("axis_n255", 0.0) and P.restate_R("planar_n256", 0.013)
    with mp.workdps(P.DPS):
        s = P.restated("planar_n256", 0.0)["sigma"]
        assert s[2] <= mp.mpf(10) ** -40 * s[0] and s[1] / s[0] >= P.SIGMA_RATIO


def test_float64_yardsticks(capsys):
    worst = P.measure_yardsticks()
    with capsys.disabled():
        print("\nrotation probe float64 yardsticks (measured / recorded):")
        for k, v in worst.items():
            print("  %-26s " % (k,) + ", ".join("%s %.2e / %.0e" % (q, e, P.YARDSTICK[k][q]) for q, e in v.items()))
    assert set(worst) == set(P.YARDSTICK)
    for k, v in worst.items():
        assert set(v) == set(P.YARDSTICK[k]), k
        for q, e in v.items():
            assert P.YARDSTICK[k][q] / 8 <= e <= P.YARDSTICK[k][q], (k, q, e)


def _exceeds(kind, cls, e):
    return any(v > P.DEVICE_FACTOR * P.YARDSTICK[(kind, cls)][q] for q, v in e.items())


def test_planted_defects_are_caught():
    """What a wrong kernel would hand back, planted on the float64 evaluation."""
    ts, imu, vis = P.series("rank3_n257")
    n = len(ts)
    # the tie `<=` -> `<` (the later sample) at td = 1/512
    td = 1.0 / 512.0
    ref = P.restated("rank3_n257", td)
    assert not _exceeds("rank3", "tie", P.errors(ref, P.float64_moments(ts, imu, vis, td)))
    k = np.minimum(np.arange(n) + 1, n - 1); k1 = np.minimum(k + 1, n - 1)
    q = np.where((k + 1 < n)[:, None], 0.5 * (vis[k] + vis[k1]), vis[k])
    assert _exceeds("rank3", "tie", P.errors(ref, np.concatenate([imu.sum(0), q.sum(0), (imu.T @ q).ravel()])))
    # `k + 1 < n` -> `k + 1 <= n - 2`: the sample before the last held instead of blended, at td = 0.013
    td = 0.013
    ref = P.restated("rank3_n257", td)
    shifted = ts - td
    k, dist = O.nearest(shifted, ts); k1 = np.minimum(k + 1, n - 1)
    inner = k + 1 <= n - 2
    f = np.where(inner, dist / np.where(inner, shifted[k1] - shifted[k], 1.0), 0.0)[:, None]
    q = np.where(inner[:, None], (1.0 - f) * vis[k] + f * vis[k1], vis[k])
    assert (k == n - 2).any()
    assert _exceeds("rank3", "generic", P.errors(ref, np.concatenate([imu.sum(0), q.sum(0), (imu.T @ q).ravel()])))
    # the Huber switch on 1.345^2 instead of 1.345
    ts, imu, vis = P.series("huber_n257")
    ref = P.restated("huber_n257", 0.0)
    err, R, b = O.solve_closed_form(ts, vis, imu, 0.0, True)
    m = P.float64_moments(ts, imu, vis, 0.0)
    assert not _exceeds("huber", "generic", P.errors(ref, m, R, b, err, True))
    e = np.sum((vis - (imu @ R.T + b)) ** 2, axis=1)
    bad = float(np.sum(np.where(e > P.HUBER_K ** 2, 2.0 * P.HUBER_K * np.sqrt(e) - P.HUBER_K ** 2, e)))
    assert P.errors(ref, m, R, b, bad, True)["err"] > 1e6 * P.DEVICE_FACTOR * P.YARDSTICK[("huber", "generic")]["err"]


# ---- the host preparation of the device path ------------------------------------------------------------------------------------
_lib_prepare = P.library_prepare


def test_prepare_cases_reach_the_edges():
    r = {name: P.prepared(name) for name in P.PREPARE_CASES}
    for name, ref in r.items():
        assert ref["margin"] >= 1e-6, (name, "a rate component within 1e-6 of 2 pi")
    a, b = r["cam30_starts_later"], r["cam10_imu_starts_later"]
    assert len(a["tI"]) == 303 and a["n_vis"] == 40 and a["tI"][0] > 0.0             # IMU samples before the first frame are cut; all frames kept
    assert len(b["tI"]) == 400 and b["n_vis"] == 12 and b["tI"][0] == 0.0 and b["last_held"] > 100      # frames before the IMU are cut; the IMU runs past the last frame
    assert r["cam32_ties_and_hits"]["ties"] >= 10 and r["cam32_ties_and_hits"]["hits"] >= 10
    held = r["flip_and_early_jump"]["held"]
    assert any(i <= 1 for i in held) and any(i > 1 for i in held) and (np.asarray(P.PREPARE_CASES["flip_and_early_jump"][1])[5:, 3] < 0).any()
    assert r["repeated_quaternions"]["linear"] >= 10 and all(x["linear"] == 0 for k, x in r.items() if k != "repeated_quaternions")
    assert len(r["window_of_16"]["tI"]) == 16


def test_prepare_float64_yardsticks(capsys):
    worst = P.measure_prepare_yardsticks()
    with capsys.disabled():
        print("\nrotation preparation float64 yardsticks (measured / recorded): " + ", ".join("%s %.2e / %.0e" % (k, v, P.PREPARE_YARDSTICK[k]) for k, v in worst.items()))
    for k, v in worst.items():
        assert P.PREPARE_YARDSTICK[k] / 8 <= v <= P.PREPARE_YARDSTICK[k], (k, v)


@pytest.mark.parametrize("name", sorted(P.PREPARE_CASES))
def test_library_preparation_against_the_restatement(name, capsys):
    tv, qv, ti, gy, dt = P.PREPARE_CASES[name]
    ref = P.prepared(name)
    rc, n, tI, sI, sV = _lib_prepare(tv, qv, ti, gy, dt)
    assert rc == 0 and n == len(ref["tI"])
    assert np.array_equal(tI, ref["tI"])
    eI, eV = P.array_error(sI, ref["sImu"]), P.array_error(sV, ref["sVis"])
    with capsys.disabled():
        print("\n  %s: sImu %.2e (%.1f x yardstick), sVis %.2e (%.1f x)" % (name, eI, eI / P.PREPARE_YARDSTICK["sImu"], eV, eV / P.PREPARE_YARDSTICK["sVis"]))
    assert eI <= P.DEVICE_FACTOR * P.PREPARE_YARDSTICK["sImu"] and eV <= P.DEVICE_FACTOR * P.PREPARE_YARDSTICK["sVis"]


def test_library_preparation_window_limits_and_arguments():
    tv, qv, ti, gy, dt = P.PREPARE_CASES["window_of_16"]
    assert _lib_prepare(tv, qv, ti, gy, dt)[:2] == (0, 16)                           # exactly 16 samples in the window: accepted
    assert _lib_prepare(tv, qv, ti[:15], gy[:15], dt)[0] == -1                       # exactly 15: refused
    late = tv + 0.5 / 256.0                                                          # the window opens at the first frame: IMU sample 0 is cut
    assert _lib_prepare(late, qv, ti, gy, dt)[0] == -1
    rc, n, *_ = _lib_prepare(tv, qv, ti, gy, dt, cap=15)                             # room for 15: refused, the count is reported
    assert rc == -1 and n == 16
    assert _lib_prepare(tv[::-1].copy(), qv, ti, gy, dt)[0] == -1 and _lib_prepare(tv, qv, ti[::-1].copy(), gy, dt)[0] == -1
    assert _lib_prepare(tv, qv, ti, gy, 0.0)[0] == -1 and _lib_prepare(tv[:1], qv[:1], ti, gy, dt)[0] == -1
    assert _lib_prepare(np.array([0.0, 10.0]), qv[:2], ti, gy, dt)[:2] == (0, 16)    # the LATER end closes the window: nothing is cut there


def test_debug_probe_refuses_bad_arguments():
    """oicc_debug_rotation_probe answers OICC_ERR_INVALID_ARG (-1) before it touches a device."""
    from openimucameracalibrator_amd import _lib
    fn = _lib.load().lib.oicc_debug_rotation_probe
    fn.restype = C.c_int
    fn.argtypes = [C.c_int32, C.c_int64, DP, DP, DP, C.c_int32, DP, C.c_int32, C.c_int32, DP, DP, DP, DP]
    ts = np.arange(16) / 256.0; x = np.zeros((16, 3)); tds = np.array([0.0]); m = np.zeros(15); R = np.zeros(9); b = np.zeros(3); e = np.zeros(1)

    def call(n=16, t=ts, imu=x, vis=x, num=1, td=tds, cap=0, out=(m, R, b, e)):
        p = [None if a is None else a.ctypes.data_as(DP) for a in (t, imu, vis, td) + tuple(out)]
        return fn(0, n, p[0], p[1], p[2], num, p[3], 1, cap, p[4], p[5], p[6], p[7])
    assert call(n=1) == -1 and call(t=None) == -1 and call(imu=None) == -1 and call(vis=None) == -1 and call(td=None) == -1
    assert call(num=0) == -1 and call(cap=-1) == -1 and call(n=2 ** 31) == -1
    assert call(out=(None, R, b, e)) == -1 and call(out=(m, None, b, e)) == -1 and call(out=(m, R, None, e)) == -1 and call(out=(m, R, b, None)) == -1
    assert call(t=ts[::-1].copy()) == -1 and call(t=np.zeros(16)) == -1 and call(td=np.array([float("nan")])) == -1 and call(td=np.array([float("inf")])) == -1
    bad = ts.copy(); bad[5] = float("nan")
    assert call(t=bad) == -1


def test_library_kabsch_step_returns_a_rotation_at_every_rank():
    """The host Kabsch step of the device path (debug export oicc_debug_rotation_kabsch, no device call).  The reference's full-U
    JacobiSVD hands back orthonormal factors whatever the rank, so R is always a rotation; the library's one-sided Jacobi has to
    complete the left vectors itself.  Found by tests/test_gpu_rotation_probe.py (planar_n256 at td = +1: rank 0 up to rounding,
    R came back with two zero rows).  Full rank and rank 2 (where R is unique) against numpy's SVD."""
    from openimucameracalibrator_amd import _lib
    fn = _lib.load().lib.oicc_debug_rotation_kabsch
    fn.restype = C.c_int
    fn.argtypes = [DP, DP]

    def kabsch(A):
        A = np.ascontiguousarray(A, dtype=np.float64); R = np.full((3, 3), np.nan)
        assert fn(A.ctypes.data_as(DP), R.ctypes.data_as(DP)) == 0
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(R) - 1.0) <= 1e-14, (A, R)
        return R
    u = np.array([0.36, -0.48, 0.8])
    for A in (np.zeros((3, 3)), np.outer(u, [1.0, 2.0, 3.0]), np.outer([0.0, 0.0, 1.0], [0.0, 3e-17, 0.0]), np.outer([0.0, 1.0, 0.0], [1.0, 0.0, 0.0]),
              np.array([[1e-17, -2e-17, 0.0], [3e-17, 1e-18, 0.0], [0.0, 0.0, 0.0]]), np.diag([1.0, 1.0, -1.0]), -np.eye(3)):
        kabsch(A)
    rng = np.random.default_rng(8)
    for rank in (3, 2):
        for _ in range(5):
            A = rng.standard_normal((3, 3))
            if rank == 2:
                A[2] = 0.0
            U, _, Vt = np.linalg.svd(A)
            Cm = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
            assert np.abs(kabsch(A) - Vt.T @ Cm @ U.T).max() <= 1e-13
    assert fn(None, np.zeros(9).ctypes.data_as(DP)) == -1 and fn(np.full(9, np.nan).ctypes.data_as(DP), np.zeros(9).ctypes.data_as(DP)) == -1
