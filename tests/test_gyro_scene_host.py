"""The host rules of the gyro warps (csrc/gyro_scene_host.h) on the host alone: tests/gyro_scene_host_driver.cpp calls them on scenes
written to a text file, plain and under the address and undefined-behaviour sanitizers, and what it prints is held against the numpy
restatements: camera rates and frame windows (rolling_shutter_restatement), the path, the smoothing windows and the applied zoom
(stabilization_restatement), the horizon lock's sample frames and gravity windows (horizon_restatement).  Integers, flags and return
codes are equal exactly; the rates and R(q_i_c) bit for bit (the same IEEE operations in the same order, no fused multiply-add on
either side); the applied zoom as test_stabilization_restatement.py holds it (exact in modes 0 and 1, within 4 eps of the largest
zoom in mode 2: exp of two libraries).  No device."""
import functools
import os
import subprocess

import numpy as np
import pytest

import horizon_cases as HC
import horizon_restatement as HR
import rolling_shutter_cases as K
import rolling_shutter_restatement as RS
import stabilization_cases as SC
import stabilization_restatement as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
STEP = SC.STEP
INVALID_ARG = -1
up, down = (lambda x: np.nextafter(x, np.inf)), (lambda x: np.nextafter(x, -np.inf))


@pytest.fixture(scope="module", params=(False, True), ids=("plain", "address-undefined"))
def driver(request, tmp_path_factory):
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if request.param else []
    exe = str(tmp_path_factory.mktemp("gyro_scene_host") / "gyro_scene_host_driver")
    csrc = os.path.join(ROOT, "openimucameracalibrator_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-I", csrc] + extra + [os.path.join(ROOT, "tests", "gyro_scene_host_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert r.returncode == 0 and "warning" not in r.stdout, r.stdout

    def run(records, path):
        with open(str(path), "w") as f:
            for key, values in records.items():
                v = np.asarray(values, dtype=np.float64).ravel()
                f.write("%s %d %s\n" % (key, v.size, " ".join(float(x).hex() for x in v)))
        r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        out = {}
        for line in r.stdout.splitlines():
            name, *values = line.split()
            floats = name in ("rates_cam", "Ric", "zoom")
            out[name] = np.array([float.fromhex(v) for v in values]) if floats else np.array([int(v) for v in values], dtype=np.int64)
        return out
    return run


# ---------------------------------------------------------------- scenes
def scene_records(kw):
    """The scene part of a driver file from the keyword arguments of the restatement's Scene (no restatement involved)."""
    src_h = kw["src"][3]
    ref = kw.get("reference_row")
    return dict(gyro_t=kw["gyro_t"], rates=kw["gyro_rates"], q_i_c=kw.get("q_i_c", (1.0, 0.0, 0.0, 0.0)), frame_t=kw["frame_t"],
                scene=[kw.get("time_offset_imu_to_cam", 0.0), kw["line_delay_s"], (src_h - 1) / 2.0 if ref is None else ref, src_h])


def grid_scene(reference, **over):
    """The dyadic telemetry of stabilization_cases (gyro sample j at j / 1024 s, reference delay 2^-7 s) with the frames' reference
    times given in seconds behind the first sample: every time difference of the rules is exact."""
    kw = SC.clip_args(2)
    kw["frame_t"] = SC.frame_times_for_reference(reference)
    kw.update(over)
    return kw


def coverage_edge_scene():
    """Frame windows whose span ends exactly on the first / the last gyro sample, and their neighbours one ulp outside: a_j = j / 1024
    exactly for frame_t = T_BASE, lo = 0, hi = 539 line delays."""
    last = 699 * STEP - 539 * SC.LINE_DELAY
    return grid_scene([0.0], frame_t=np.array([down(SC.T_BASE), SC.T_BASE, SC.T_BASE + last, up(SC.T_BASE + last)]))


def path_edge_scene():
    """Reference times exactly on the first and on the last gyro sample, one between, and one ulp outside at either end."""
    t = SC.frame_times_for_reference([0.0, 1.5 * STEP, 699 * STEP])
    return grid_scene([0.0], frame_t=np.array([down(t[0]), t[0], t[1], t[2], up(t[2])]))


def path_edge_samples():
    """Accelerometer samples exactly on the first and on the last on-path reference time of path_edge_scene, and one ulp outside."""
    t = HC.accl_times([0.0, 0.7 * STEP, 1.5 * STEP, 300.25 * STEP, 699 * STEP])
    return np.array([down(t[0]), t[0], t[1], t[2], t[3], t[4], up(t[4])])


def reach_edge_samples():
    """On the mixed scene at sigma_g = 1 / 1024 s: samples exactly 3 sigma_g before and behind frame 5's reference time (13.5 steps), one
    ulp further out, exactly on frame 3's (12 steps) and one ulp before it, before the first on-path reference time and behind the last."""
    t = HC.accl_times(np.array([5.0, 10.5, 10.5, 12.0, 12.0, 14.0, 15.7, 16.5, 16.5, 17.5, 315.2, 400.0]) * STEP)
    t[1], t[3], t[8] = down(t[1]), down(t[3]), up(t[8])
    return t


def _bad(name):
    kw = K.small_scene()
    K.BAD_SCENES[name](kw)
    return kw


# name -> (scene keyword arguments, smoothing sigmas, [(accl_t, sigma_g), ...]).  The rolling-shutter scenes' frame times need not increase,
# which the smoothing and gravity windows require (judge_scene of stabilization.hip): those scenes go without them.
SCENES = {
    "small": lambda: (K.small_scene(), (), []),
    "mixed": lambda: (SC.mixed_args(), (0.0, 2.5 * STEP, 1.0), [(HC.sample_case(9, "mixed")[1], 1.0), (HC.sample_case(65, "mixed")[1], 0.01),
                                                                (reach_edge_samples(), STEP)]),
    "path of 0": lambda: (grid_scene([-0.5, -0.4]), (0.0, 1.0), [(HC.accl_times([0.1, 0.2]), 1.0)]),
    "path of 1": lambda: (SC.clip_args(1), (0.0, 1.0), [(HC.sample_case(63, "clip")[1], 0.01)]),
    "path of 2": lambda: (SC.clip_args(2), (0.0, 1.0), [(HC.sample_case(63, "clip")[1], 0.01)]),
    "clip 65": lambda: (SC.clip_args(65), tuple(SC.SIGMAS.values()), [(HC.sample_case(na, "clip")[1], 0.02) for na in (1, 64, 257)]),
    "clip 257": lambda: (SC.clip_args(257), tuple(SC.SIGMAS.values()), []),
    "level": lambda: (HC.level_args(), (0.0, HC.LEVEL_SMOOTHING), [(HC.level_of(name)[0], HC.level_of(name)[2]["gravity_sigma_s"]) for name in HC.LEVEL_CASES]),
    "off the path in the middle": lambda: (grid_scene(np.array([10.2, -0.5, 12.0]) * STEP), (), []),
    "off the path in the middle, behind": lambda: (grid_scene(np.array([10.2, 900.0, 12.0, 13.0]) * STEP), (), []),
    "coverage ends on lo and hi": lambda: (coverage_edge_scene(), (0.0,), []),
    "reference times on the first and last sample": lambda: (path_edge_scene(), (0.0, 1.0), [(path_edge_samples(), 0.5 * STEP), (path_edge_samples(), 1.0)]),
}
SCENES.update({"rotation " + kind: (lambda kind=kind: (K.rotation_scene_args(kind), (), []))
               for kind in ("plain", "negative-delay", "zero-delay", "inside-one-interval", "row-on-a-sample", "uncovered", "window-256", "window-257")})
# what judge() refuses for the camera, the rotation or the norm of q_i_c alone: the rules see an ordinary scene
SCENES.update({"refused: " + name: (lambda name=name: (_bad(name), (), []))
               for name in ("inf reference row", "q_i_c not unit", "unknown source model", "nan intrinsics", "source width 0", "destination height 0", "nan rotation")})
# what judge() refuses before any rule runs (times that are not finite or do not increase, fewer than two samples, no frames): the rules
# promise nothing for these; the driver still has to end without a report from the sanitizers
BROKEN = ("one gyro sample", "gyro times repeat", "gyro times decrease", "nan gyro time", "inf rate", "nan frame time", "nan line delay",
          "nan time offset", "q_i_c nan", "no frames")
PREMISES = {                # what a scene is here for, from the restatement
    "path of 0": lambda e: e["path"] == (0, 0, 0),
    "path of 1": lambda e: e["path"] == (0, 0, 1),
    "path of 2": lambda e: e["path"] == (0, 0, 2),
    "mixed": lambda e: e["path"] == (0, 1, 7) and sorted(e["levels"][0]["frame_of"]) == sorted(HC.MIXED_FRAME_OF)
    and list(e["levels"][2]["frame_of"][[0, 3, 4, 11]]) == [-1, 2, 3, -1] and (e["levels"][2]["lo"][5], e["levels"][2]["hi"][5]) == (2, 7),
    "off the path in the middle": lambda e: e["path"][0] == INVALID_ARG,
    "off the path in the middle, behind": lambda e: e["path"][0] == INVALID_ARG,
    "coverage ends on lo and hi": lambda e: list(e["status"]) == [1, 0, 0, 1] and e["first"][1] == 0 and e["first"][2] + e["count"][2] == 700,
    "reference times on the first and last sample": lambda e: e["path"] == (0, 1, 3) and list(e["interval"][1:4]) == [0, 1, 698]
    and list(e["levels"][0]["frame_of"]) == [-1, 1, 1, 2, 2, 3, -1],
    "rotation window-256": lambda e: list(e["status"]) == [0] and list(e["count"]) == [RS.MAX_WINDOW],
    "rotation window-257": lambda e: list(e["status"]) == [2],
    "rotation uncovered": lambda e: list(e["status"]) == [1, 0, 1],
}


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatements' answers for a scene, computed once and shared by both builds of the driver."""
    kw, sigmas, levels = SCENES[name]()
    sc = SC.restatement_scene(kw)
    q = np.asarray(kw.get("q_i_c", (1.0, 0.0, 0.0, 0.0)), dtype=np.float64)
    q = q / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    status, first, count = RS.frame_windows(sc)
    e = dict(rates_cam=RS.camera_rates(kw["gyro_rates"], kw.get("q_i_c", (1.0, 0.0, 0.0, 0.0))).ravel(), Ric=RS.qmat(q).ravel(), status=status, first=first,
             count=count, smooth=[], levels=[])
    try:
        pf, pc, e["interval"] = SR.on_path(sc)
        e["path"] = (0, pf, pc)
    except AssertionError:                       # the restatement's word for "not contiguous"
        e["path"] = (INVALID_ARG, 0, 0)
        return e
    e["smooth"] = [SR.windows(sc, s) for s in sigmas]
    for accl_t, sigma_g in levels:
        lv = HR.Level(accl_t, np.zeros((len(accl_t), 3)), gravity_sigma_s=sigma_g)
        frame_of, interval = HR.sample_frames(sc, lv)
        lo, hi = HR.windows(sc, lv)
        e["levels"].append(dict(frame_of=frame_of, interval=interval, lo=lo, hi=hi))
    return e


@pytest.mark.parametrize("name", list(SCENES))
def test_rules_against_the_restatements(driver, tmp_path, name):
    kw, sigmas, levels = SCENES[name]()
    e = expected(name)
    assert PREMISES.get(name, lambda e: True)(e), "the scene is not the edge it was built for"
    runs = [dict(sigma=[s]) for s in sigmas] + [dict(accl_t=t, gravity_sigma=[g]) for t, g in levels] or [dict()]
    outs = [driver(dict(scene_records(kw), **more), tmp_path / "scene.txt") for more in runs]
    for o in outs:
        assert np.array_equal(o["rates_cam"].view(np.int64), e["rates_cam"].view(np.int64)) and np.array_equal(o["Ric"].view(np.int64), e["Ric"].view(np.int64))
        assert np.array_equal(o["status"], e["status"]) and np.array_equal(o["first"], e["first"]) and np.array_equal(o["count"], e["count"])
        assert tuple(o["path"]) == e["path"] if e["path"][0] == 0 else o["path"][0] == INVALID_ARG
        if e["path"][0] == 0:
            assert np.array_equal(o["interval"], e["interval"])
    for o, (lo, hi) in zip(outs, e["smooth"]):
        assert np.array_equal(o["smooth_lo"], lo) and np.array_equal(o["smooth_hi"], hi)
    for o, l in zip(outs[len(e["smooth"]):], e["levels"]):
        assert np.array_equal(o["frame_of"], l["frame_of"]) and np.array_equal(o["sample_interval"], l["interval"])
        some = l["hi"] >= l["lo"]
        assert np.array_equal(o["level_lo"][some], l["lo"][some]) and np.array_equal(o["level_hi"][some], l["hi"][some])
        # an empty window is (0, -1) in the restatement and (b, b - 1) at the place the search ended in the header: both hold no sample
        assert np.array_equal(o["level_hi"][~some], o["level_lo"][~some] - 1)


@pytest.mark.parametrize("name", BROKEN)
def test_refused_scenes_end_without_a_memory_error(driver, tmp_path, name):
    """judge() returns OICC_ERR_INVALID_ARG for these before it calls a rule; should one reach the rules all the same, they stay inside
    their arrays (the sanitizers' build ends with a non-zero code otherwise)."""
    o = driver(dict(scene_records(_bad(name)), sigma=[0.01], accl_t=HC.accl_times([0.01, 0.02]), gravity_sigma=[0.01]), tmp_path / "scene.txt")
    assert len(o["status"]) == len(_bad(name)["frame_t"])


# ---------------------------------------------------------------- the applied zoom
def zoom_cases():
    rng = np.random.RandomState(5)
    t = np.cumsum(0.02 + 0.03 * rng.rand(60))
    z = 1.0 + 0.3 * rng.rand(60) ** 3
    status = (rng.rand(60) < 0.1).astype(np.int32)
    z[status != 0] = np.nan
    spike = z.copy(); spike[np.where(status == 0)[0][[3, 20]]] = np.inf          # an invalid centre: infinite required zoom
    off = np.full(60, np.nan)
    return {"plain": (t, z, status), "infinite": (t, spike, status), "all off the path": (t, off, np.ones(60, np.int32)),
            "one frame": (t[:1], np.array([1.25]), np.zeros(1, np.int32))}


@pytest.mark.parametrize("mode", (0, 1, 2))
@pytest.mark.parametrize("case", ("plain", "infinite", "all off the path", "one frame"))
def test_applied_zoom_against_the_restatement(driver, tmp_path, case, mode):
    t, z, status = zoom_cases()[case]
    for window, max_zoom in ((0.0, np.inf), (0.1, np.inf), (0.1, 1.1), (100.0, 1e6)):
        with np.errstate(all="ignore"):
            Z, clamped = SR.applied_zoom(t, z, status, mode, window, max_zoom)
        o = driver(dict(frame_t=t, z=z, status=status, zoom=[mode, window, max_zoom]), tmp_path / "zoom.txt")
        assert np.array_equal(o["clamped"], clamped) and np.array_equal(np.isinf(o["zoom"]), np.isinf(Z)) and not np.isnan(o["zoom"]).any()
        fin = np.isfinite(Z)
        if mode == 2:
            assert np.abs(o["zoom"][fin] - Z[fin]).max(initial=0.0) <= 4 * EPS * Z[fin].max(initial=1.0)      # exp of the two libraries
        else:
            assert np.array_equal(o["zoom"], Z)
        ok = status == 0
        if mode != 0:                                                         # mode 0 is zoom 1: the borders show
            assert np.all(o["zoom"][ok] >= np.minimum(z[ok], max_zoom))      # an inequality, not a tolerance: the zoom covers what is required


# ---------------------------------------------------------------- the argument checks
GOOD_OPTIONS = dict(smoothing_sigma_s=0.5, max_correction_rad=0.0, zoom_mode=2, zoom_window_s=0.0, max_zoom=1.0)


def test_argument_checks(driver, tmp_path):
    def options_ok(**over):
        d = dict(GOOD_OPTIONS, **over)
        return driver(dict(options=[d[k] for k in ("smoothing_sigma_s", "max_correction_rad", "zoom_mode", "zoom_window_s", "max_zoom")]), tmp_path / "o.txt")["options_ok"]

    assert list(options_ok()) == [1, 0]                                        # good options; a null pointer
    for name, over in SC.BAD_OPTIONS.items():
        assert list(options_ok(**over)) == [0, 0], name
    for over in (dict(max_zoom=np.inf), dict(max_zoom=np.nan), dict(zoom_window_s=np.inf), dict(max_correction_rad=np.nan)):
        assert list(options_ok(**over)) == [0, 0], over

    def level_ok(t, a, o):
        o = dict(dict(gravity_sigma_s=1.0, gravity_const=HC.G, accl_gate=0.0, lock=1.0, roll_rad=0.0), **o)
        return driver(dict(accl_t=t, accl=a, level_opts=[o[k] for k in ("gravity_sigma_s", "gravity_const", "accl_gate", "lock", "roll_rad")]),
                      tmp_path / "l.txt")["level_ok"]

    assert list(level_ok(*HC.small_level())) == [1, 0]
    assert list(level_ok(*HC.small_level(lock=0.0, accl_gate=2.0, roll_rad=-7.0))) == [1, 0]
    for name, bad in HC.BAD_LEVELS.items():
        assert list(level_ok(*bad(*HC.small_level()))) == [0, 0], name
    assert list(level_ok(np.zeros(0), np.zeros((0, 3)), {})) == [0, 0]          # no samples

    def plan_ok(q, zoom):
        return list(driver(dict(plan_q=q, plan_zoom=zoom), tmp_path / "p.txt")["plan_arrays_ok"])

    q = np.tile([1.0, 0.0, 0.0, 0.0], (3, 1))
    assert plan_ok(q, np.ones(3)) == [1, 0]                                    # good arrays; a null pointer
    assert plan_ok(q * (1.0 + 0.9e-6), [1.0, 0.5, 7.0]) == [1, 0] and plan_ok(q * (1.0 + 1.1e-6), np.ones(3)) == [0, 0]
    for zoom in ([1.0, 0.0, 1.0], [1.0, -1.0, 1.0], [1.0, np.inf, 1.0], [np.nan, 1.0, 1.0]):
        assert plan_ok(q, zoom) == [0, 0], zoom
    bad = q.copy(); bad[2, 1] = np.nan
    assert plan_ok(bad, np.ones(3)) == [0, 0]
