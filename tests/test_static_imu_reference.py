"""The 50-digit restatement of the static IMU calibration (static_imu_reference.py) on the host: its derivatives against 50-digit
central differences, the float64 yardsticks (YARDSTICK, measured again and held to [1/4, 1] of the table), the product-form
integration -- what the device evaluates, DESIGN.md 3.y deviation (2) -- within DEVICE_FACTOR x the yardstick of the reference's
per-step-normalised form, and the detector cases of static_imu_cases.py against their construction and the plain per-sample loop."""
import functools

import mpmath as mp
import numpy as np
import pytest

import static_imu_cases as K
import static_imu_reference as R
import static_imu_restatement as S


# ---- measurements ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def float64_gyro(config, product_form):
    t, w, ranges, gv, p, ob, dt, _ = K.gyro_inputs(config)
    return S.gyro_blocks_eval(t, w, [tuple(int(v) for v in r) for r in ranges], gv, p, ob, dt, product_form=product_form)


def measure_gyro(config, cls, product_form=False):
    """(gyro/r, gyro/J) of the float64 restatement for one case."""
    r, J = float64_gyro(config, product_form)
    b = K.GYRO_CONFIGS[config][4].index(cls)
    return R.gyro_errors(r[3 * b:3 * b + 3], J[3 * b:3 * b + 3], config, cls)


def measure_gyro_class(cls):
    figs = [measure_gyro(cfg, c) for cfg, c in K.gyro_case_list() if c == cls]
    return max(f[0] for f in figs), max(f[1] for f in figs)


def measure_acc_rows():
    figs = []
    for name, p in K.ACC_PARAMS.items():
        r, J = S.acc_rows(K.acc_samples(), p, K.G)
        figs.append(R.acc_row_errors(r, J, name))
    return max(f[0] for f in figs), max(f[1] for f in figs)


def measure_acc_sums(count):
    figs = []
    for name, p in K.ACC_PARAMS.items():
        r, J = S.acc_rows(K.acc_samples()[:count], p, K.G)
        c, H, g = S.normal_eq(r, J)
        figs.append(R.acc_sum_errors(c, H, g, name, count))
    return tuple(max(f[k] for f in figs) for k in range(3))


def measure_all():
    """{key: fresh figure} of the whole table (what YARDSTICK is rounded up from)."""
    out = {}
    for cls in K.GYRO_CLASSES:
        out["gyro/r/" + cls], out["gyro/J/" + cls] = measure_gyro_class(cls)
    out["acc/r"], out["acc/J"] = measure_acc_rows()
    for n in K.ACC_COUNTS:
        out["acc/H/%d" % n], out["acc/g/%d" % n], out["acc/cost/%d" % n] = measure_acc_sums(n)
    return out


def _check_measured(key, fresh):
    """The table is at least the measurement and at most 4 times it (an exact case: the floor of one epsilon)."""
    entry = R.YARDSTICK[key]
    print("%-16s measured %.3e  table %.3e" % (key, fresh, entry))
    assert fresh <= entry <= 4 * max(fresh, R.EPS), (key, fresh, entry)


# ---- yardsticks ------------------------------------------------------------------------------------------------------------
def test_the_table_names_every_class():
    keys = ["gyro/%s/%s" % (f, c) for c in K.GYRO_CLASSES for f in "rJ"] + ["acc/r", "acc/J"] + \
           ["acc/%s/%d" % (f, n) for n in K.ACC_COUNTS for f in ("H", "g", "cost")]
    assert sorted(R.YARDSTICK) == sorted(keys)
    assert all(v >= R.EPS for v in R.YARDSTICK.values())


@pytest.mark.parametrize("config,cls", K.gyro_case_list())
def test_float64_gyro_within_the_table_and_product_form_within_the_bound(config, cls):
    """The per-step-normalised float64 integration defines the table; the product form of the same float64 arithmetic stays within
    DEVICE_FACTOR x it, so a device that evaluates the product form can meet the bound (deviation (2))."""
    er, ej = measure_gyro(config, cls)
    pr, pj = measure_gyro(config, cls, product_form=True)
    yr, yj = R.YARDSTICK["gyro/r/" + cls], R.YARDSTICK["gyro/J/" + cls]
    print("%s/%s  normalised r %.3e J %.3e   product form r %.3e (%.2f x table) J %.3e (%.2f x table)" % (config, cls, er, ej, pr, pr / yr, pj, pj / yj))
    assert er <= yr and ej <= yj, (er, yr, ej, yj)
    assert pr <= R.DEVICE_FACTOR * yr and pj <= R.DEVICE_FACTOR * yj, (pr, yr, pj, yj)
    if K.gyro_steps(cls) == 0:          # residual g0 - g1 exactly, every derivative zero
        g0, g1 = K.gyro_versors()[cls]
        ref_r, ref_J = R.gyro_reference(config, cls)
        assert [float(v) for v in ref_r] == list(g0 - g1) and not any(v != 0 for v in ref_J.ravel())
        assert er <= R.EPS and pr == er and ej == 0.0 and pj == 0.0          # one rounding of the difference


@pytest.mark.parametrize("cls", K.GYRO_CLASSES)
def test_gyro_table_is_the_measurement(cls):
    er, ej = measure_gyro_class(cls)
    _check_measured("gyro/r/" + cls, er)
    _check_measured("gyro/J/" + cls, ej)


def test_acc_rows_table_is_the_measurement():
    er, ej = measure_acc_rows()
    _check_measured("acc/r", er)
    _check_measured("acc/J", ej)


@pytest.mark.parametrize("count", K.ACC_COUNTS)
def test_acc_sums_table_is_the_measurement(count):
    eh, eg, ec = measure_acc_sums(count)
    _check_measured("acc/H/%d" % count, eh)
    _check_measured("acc/g/%d" % count, eg)
    _check_measured("acc/cost/%d" % count, ec)


# ---- the restatement's own derivatives ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.ACC_PARAMS))
@R.at_dps
def test_acc_derivatives_against_central_differences(name):
    """50-digit central differences of the 50-digit residual, h = 1e-20: truncation 1e-40, rounding 1e-30."""
    p = [mp.mpf(float(v)) for v in K.ACC_PARAMS[name]]
    g = mp.mpf(K.G)
    h = mp.mpf(10) ** -20
    ref_r, ref_J = R.acc_reference(name)
    for i in (0, 1, 2, 3, 4, 62, 255, 512):
        x = [mp.mpf(float(v)) for v in K.acc_samples()[i]]
        assert R.acc_residual(x, p, g) == ref_r[i]
        for k in range(9):
            pp, pm = list(p), list(p)
            pp[k] += h; pm[k] -= h
            fd = (R.acc_residual(x, pp, g) - R.acc_residual(x, pm, g)) / (2 * h)
            assert abs(fd - ref_J[i, k]) <= mp.mpf(10) ** -25, (i, k, fd, ref_J[i, k])


@pytest.mark.parametrize("optimize_bias,gyro_dt", [(True, -1.0), (False, -1.0), (True, 0.005)])
@R.at_dps
def test_gyro_jets_against_central_differences(optimize_bias, gyro_dt):
    """A 3-step block on the jittered series: every derivative column against the difference of the residual alone."""
    t, w = K.gyro_series()["jitter"]
    g0, g1 = K.gyro_versors()["2"]
    i0, i1 = 400, 403
    r, J = R.gyro_block(t, w, i0, i1, g0, g1, K.P_AWAY, optimize_bias, gyro_dt)
    ncols = 12 if optimize_bias else 9
    assert len(J[0]) == ncols
    h = mp.mpf(10) ** -20
    # mpf parameters pass through unrounded: the difference quotient needs p +- 1e-20
    p0 = [mp.mpf(float(v)) for v in K.P_AWAY]
    for k in range(12):
        pp, pm = list(p0), list(p0)
        pp[k] += h; pm[k] -= h
        rp = R.gyro_block(t, w, i0, i1, g0, g1, pp, optimize_bias, gyro_dt, ncols=0)[0]
        rm = R.gyro_block(t, w, i0, i1, g0, g1, pm, optimize_bias, gyro_dt, ncols=0)[0]
        for i in range(3):
            fd = (rp[i] - rm[i]) / (2 * h)
            if k < ncols:
                assert abs(fd - J[i][k]) <= mp.mpf(10) ** -25, (i, k, fd, J[i][k])
            else:
                assert fd == 0          # the bias is not a parameter: the residual does not move
    # the fixed step is what is used: with it the timestamps do not matter
    if gyro_dt > 0:
        r2, _ = R.gyro_block(K.gyro_series()["uniform"][0] * 3.0, w, i0, i1, g0, g1, K.P_AWAY, optimize_bias, gyro_dt, ncols=0)
        assert r2 == r


@R.at_dps
def test_normalisation_only_rescales():
    """Deviation (2) at 50 digits: the product of the un-normalised steps gives the same rotation as the reference's form."""
    t, w = K.gyro_series()["uniform"]
    g0, g1 = K.gyro_versors()["2"]
    ch = R.Chain(t, w, 50, K.P_AWAY, True, -1.0, 12)
    q = ch.q
    for s in range(50, 55):          # the same steps without NormalizeQuaternion
        w0 = R.unbias_normalize(ch.ms, ch.b, w[s], 12)
        w1 = R.unbias_normalize(ch.ms, ch.b, w[s + 1], 12)
        dt = R.mpf(t[s + 1]) - R.mpf(t[s])
        w01 = [R.jscale(mp.mpf(0.5), R.jadd(a, b)) for a, b in zip(w0, w1)]
        k1 = R.half_omega_q(w0, q)
        k2 = R.half_omega_q(w01, [R.jadd(a, R.jscale(dt / 2, k)) for a, k in zip(q, k1)])
        k3 = R.half_omega_q(w01, [R.jadd(a, R.jscale(dt / 2, k)) for a, k in zip(q, k2)])
        k4 = R.half_omega_q(w1, [R.jadd(a, R.jscale(dt, k)) for a, k in zip(q, k3)])
        q = [R.jadd(a, R.jscale(dt / 6, R.jadd(R.jadd(x1, R.jscale(2, x2)), R.jadd(R.jscale(2, x3), x4)))) for a, x1, x2, x3, x4 in zip(q, k1, k2, k3, k4)]
    a = R.residual_of_quaternion(q, g0, g1, 12)
    b = R.residual_of_quaternion(ch.after(5), g0, g1, 12)
    assert max(abs(x - y) for u, v in zip(a, b) for x, y in zip(u, v)) <= mp.mpf(10) ** -45


# ---- detector cases --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.DETECTOR_NAMES)
def test_detector_cases_give_the_lists_they_were_built_for(name):
    case = K.detector_cases()[name]
    acc, win, h = case["acc"], case["win"], case["h"]
    assert S.normalized_win(win) == 2 * h + 1 and len(case["thresholds"]) in (1, 2, 10)
    norms = S.window_norms(acc, win)
    if len(acc) == 2 * h + 1:          # win_size = n: no centre is looked at
        assert np.all(np.isnan(norms)) and all(e == [] for e in case["expected"])
    else:
        assert np.all(np.isnan(norms[:h])) and np.all(np.isnan(norms[len(acc) - h:])) and np.all(np.isfinite(norms[h:len(acc) - h]))
    for th, expected in zip(case["thresholds"], case["expected"]):
        got = [tuple(int(v) for v in iv) for iv in S.intervals_from_norms(norms, th, win)]
        assert got == K.plain_detector_loop(acc, th, win), (name, th)
        if expected is not None:
            assert got == [tuple(e) for e in expected], (name, th, got, expected)
    if name.startswith(("len_", "lanes", "span", "first", "table", "all_", "dense")) and len(acc) > 2 * h + 1:
        runs = case["expected"][list(case["thresholds"]).index(K.STILL_TH)]
        still = np.zeros(len(acc), bool)
        for a, b in runs:
            still[a:b + 1] = True
        inner = np.arange(len(acc))
        inner = (inner >= h) & (inner < len(acc) - h)
        assert np.all(norms[still] == 0.0) and np.all(norms[inner & ~still] > 1e-3)          # bit-zero, and far above


def test_detector_cases_cover_the_lanes_the_compaction_counts_at():
    """Where the cases put their edges, in the kernel's coordinates (h = 5): lane (i - 5) % 256 of workgroup (i - 5) // 256."""
    cases = K.detector_cases()
    runs = lambda n: cases[n]["expected"][list(cases[n]["thresholds"]).index(K.STILL_TH)]
    lane = lambda i: (i - 5) % 256
    group = lambda i: (i - 5) // 256
    assert {lane(a) for a, b in runs("lanes")} == {63, 255, 64, 0}
    assert any(lane(a) == 255 and a == b and lane(b + 1) == 0 for a, b in runs("lanes"))          # the fall is lane 0 of the next workgroup
    assert any(group(b) - group(a) == 2 for a, b in runs("span3"))
    assert any(group(b) - group(a) == 4 and b == len(cases["span4_to_the_end"]["acc"]) - 6 for a, b in runs("span4_to_the_end"))
    assert runs("first_and_last")[0][0] == 5 and runs("first_and_last")[-1] == (517, 517) and len(cases["first_and_last"]["acc"]) == 523
    assert runs("all_still") == [(5, 517)] and runs("all_loud") == []
    assert all(b == a and a2 - a == 12 for (a, b), (a2, _) in zip(runs("dense"), runs("dense")[1:])) and len(runs("dense")) == 86
    assert sorted({len(c["thresholds"]) for c in cases.values()}) == [1, 2, 10]
    sizes = {(c["win"], len(c["acc"]) - 2 * c["h"]) for c in cases.values()}
    assert {(w, M) for w in (11, 12, 41) for M in (1, 2, 255, 256, 257, 513)} <= sizes
    assert {(w, M) for w in (1025, 1024) for M in (1, 2, 257)} <= sizes
