"""The numpy specification of the stabilisation (tests/stabilization_restatement.py) against independent references, the premises
of the GPU cases, and what the library answers without a device.

Yardstick: max |float64 - numpy.longdouble| of the restatement on the case at hand, measured here and printed; a reference may be
ten times that away, plus the reference's own rounding where it has one (stated at the test)."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

import camera_maps_restatement as R
import rolling_shutter_cases as K
import rolling_shutter_restatement as RS
import stabilization_cases as SC
import stabilization_restatement as SR
from openimucameracalibrator_amd import _abi
from openimucameracalibrator_amd import rolling_shutter as rs
from openimucameracalibrator_amd import stabilization as stab
from openimucameracalibrator_amd import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float64).eps)


def _scipy_quat(q):
    q = np.asarray(q, dtype=np.float64)
    return Rot.from_quat(np.concatenate([q[..., 1:], q[..., :1]], -1))


# ---------------------------------------------------------------- path
@pytest.mark.parametrize("kind", ("mixed", 66))
def test_path_against_scipy_rotation_products(kind):
    """scipy chains one rotation-vector product per gyro interval from the first sample on: each product rounds in double, a few eps
    each, so its own error grows with the number of intervals (700 here); 8 eps per interval is granted to it."""
    kw = SC.mixed_args() if kind == "mixed" else SC.clip_args(kind)
    sc = SC.restatement_scene(kw)
    ref, _, yardstick = SC.path_reference(kind)
    t = (sc.gyro_t - SC.T_BASE) + sc.offset
    om = sc.rates

    def Q(x):                                # orientation at camera-clock time x behind T_BASE
        Rm = Rot.identity()
        j = 0
        while j + 2 < len(t) and t[j + 1] <= x:
            Rm = Rm * Rot.from_rotvec(0.5 * (om[j] + om[j + 1]) * (t[j + 1] - t[j]))
            j += 1
        s, dt = x - t[j], t[j + 1] - t[j]
        return Rm * Rot.from_rotvec(om[j] * s + (om[j + 1] - om[j]) * s * s / (2 * dt))

    on = np.where(~np.isnan(ref[:, 0]))[0]
    tref = (sc.frame_t - SC.T_BASE) + sc.reference_row * sc.line_delay
    Q0 = Q(tref[on[0]])
    worst = max(float((_scipy_quat(ref[k]).inv() * (Q0.inv() * Q(tref[k]))).magnitude()) for k in on)
    print("path %s: yardstick %.3e rad, restatement - scipy %.3e rad" % (kind, yardstick, worst))
    assert worst <= 10.0 * yardstick + 8 * EPS * len(t)


# ---------------------------------------------------------------- smoothing
def _fixed_axis_scene(rate_of_t):
    kw = SC.clip_args(41)
    j = np.arange(len(kw["gyro_t"]))
    axis = np.array([0.36, -0.48, 0.8])
    kw["gyro_rates"] = rate_of_t(j * SC.STEP)[:, None] * axis[None]
    kw["frame_t"] = SC.frame_times_for_reference((16 + 16 * np.arange(41)) * SC.STEP)      # uniform on the dyadic grid: exactly uniform
    return kw, RS.camera_rates(axis[None], K.Q_I_C)[0]


def test_smoothing_about_a_fixed_axis_is_the_weighted_mean_of_the_angles():
    kw, axis = _fixed_axis_scene(lambda x: 3.0 * np.sin(2 * np.pi * 2.0 * x) + 1.0)
    sc = SC.restatement_scene(kw)
    sigma = 0.05
    P, Pl = SR.path(sc), SR.path(sc, np.longdouble)
    S_, _, its = SR.smooth(sc, P, sigma)
    Sl = SR.smooth(sc, Pl, sigma, dtype=np.longdouble)[0]
    yardstick = float(K.quaternion_angle(S_, Sl).max())
    theta = 2 * np.arctan2(Pl[:, 1:] @ axis.astype(np.longdouble), Pl[:, 0])           # the angles of the path about the axis
    assert theta.max() - theta.min() > 0.3
    lo, hi = SR.windows(sc, sigma)
    worst = 0.0
    for k in range(41):
        m = np.arange(lo[k], hi[k] + 1)
        dt = (sc.frame_t[m] - sc.frame_t[k]).astype(np.longdouble)
        w = np.exp(-(dt * dt) / (2 * np.longdouble(sigma) ** 2))
        mean = float((w * theta[m]).sum() / w.sum())
        worst = max(worst, float((_scipy_quat(S_[k]).inv() * Rot.from_rotvec(axis * mean)).magnitude()))
    print("fixed axis: yardstick %.3e rad, restatement - closed form %.3e rad, iterations %d" % (yardstick, worst, its.max()))
    assert worst <= 10.0 * yardstick + 4 * EPS           # scipy's own rounding of Exp and of the product
    assert its.max() <= 3


def test_a_constant_rate_is_not_corrected():
    kw, axis = _fixed_axis_scene(lambda x: np.full(len(x), 1.7))
    sc = SC.restatement_scene(kw)
    sigma = 0.05
    P, Pl = SR.path(sc), SR.path(sc, np.longdouble)
    S_, C_, _ = SR.smooth(sc, P, sigma)
    Cl = SR.smooth(sc, Pl, sigma, dtype=np.longdouble)[1]
    lo, hi = SR.windows(sc, sigma)
    k = np.arange(41)
    whole = (k - lo == 9) & (hi - k == 9)                    # 3 sigma = 0.15 s = 9.6 frame intervals
    assert whole.sum() == 41 - 18
    yardstick = float(K.quaternion_angle(C_[whole], Cl[whole]).max())
    angle = SR.correction_angle(C_)
    print("constant rate: yardstick %.3e rad, largest correction of a whole window %.3e rad, of a cut one %.3e rad" % (yardstick, angle[whole].max(), angle[~whole].max()))
    assert angle[whole].max() <= 10.0 * yardstick + 4 * EPS
    assert angle[~whole].min() > 1e-4                        # the clip's ends pull the mean inwards


# ---------------------------------------------------------------- applied zoom
def _zoom_case(seed, n=120):
    rng = np.random.RandomState(seed)
    t = SC.T_BASE + np.cumsum(rng.uniform(0.02, 0.05, n))
    z = 1.0 + 0.3 * rng.rand(n) ** 3
    status = (rng.rand(n) < 0.1).astype(np.int32)
    z[status != 0] = np.nan
    return t, z, status


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_applied_zoom_covers_the_required_zoom(seed):
    t, z, status = _zoom_case(seed)
    ok = status == 0
    for T in (0.0, 0.1, 0.5, 100.0):
        Z, clamped = SR.applied_zoom(t, z, status, 2, T)
        lib, lib_clamped = stab.applied_zoom(t, z, status, stab.StabOptions(zoom_mode="dynamic", zoom_window_s=T, max_zoom=1e6))
        assert np.all(Z[ok] >= z[ok]) and np.all(lib[ok] >= z[ok])                    # an inequality, not a tolerance
        assert not clamped.any() and not lib_clamped.any()
        assert np.abs(lib - Z).max() <= 4 * EPS * Z.max()                             # exp of the two libraries
        if T == 0.0:
            assert np.array_equal(Z[ok], z[ok])
    Z, _ = SR.applied_zoom(t, z, status, 1)
    lib, _ = stab.applied_zoom(t, z, status, stab.StabOptions(zoom_mode="fixed", max_zoom=1e6))
    assert np.array_equal(Z, np.full(len(t), z[ok].max())) and np.array_equal(lib, Z)
    lib, _ = stab.applied_zoom(t, z, status, stab.StabOptions(zoom_mode="none"))
    assert np.array_equal(lib, np.ones(len(t)))
    # the clamp and its flag
    lib, lib_clamped = stab.applied_zoom(t, z, status, stab.StabOptions(zoom_mode="dynamic", zoom_window_s=0.1, max_zoom=1.1))
    Z, clamped = SR.applied_zoom(t, z, status, 2, 0.1, 1.1)
    assert np.array_equal(lib_clamped, clamped) and clamped.any() and not clamped.all() and np.all(lib[clamped == 1] == 1.1) and lib.max() == 1.1


def test_constant_required_zoom_gives_constant_zoom():
    t, z, status = _zoom_case(3)
    z[:] = 1.2345; status[:] = 0
    for mode in (1, 2):
        Z, _ = SR.applied_zoom(t, z, status, mode, 0.3)
        lib, _ = stab.applied_zoom(t, z, status, stab.StabOptions(zoom_mode=mode, zoom_window_s=0.3, max_zoom=10.0))
        assert np.abs(Z - 1.2345).max() <= 4 * EPS and np.abs(lib - 1.2345).max() <= 4 * EPS


# ---------------------------------------------------------------- premises of the GPU cases
@pytest.mark.parametrize("name", list(SC.SIGMAS))
def test_premises_of_the_gpu_smoothing_cases(name):
    r = SC.smooth_reference(name)
    print("premises smoothing %s: iterations float64 %d longdouble %d, windows %d .. %d" % (name, r["iterations"].max(), r["iterations_ld"].max(),
                                                                                          r["members"].min(), r["members"].max()))
    assert r["iterations"].max() <= 12 and r["iterations_ld"].max() <= 12
    assert K.quaternion_angle(r["S"], r["S_ld"]).max() <= 1e-13


@pytest.mark.parametrize("kind", SC.PATH_COUNTS + ("mixed",), ids=str)
def test_premises_of_the_gpu_path_cases(kind):
    a, b, yardstick = SC.path_reference(kind)
    assert np.array_equal(np.isnan(a[:, 0]), np.isnan(np.asarray(b[:, 0], dtype=np.float64)))
    assert yardstick <= 1e-13
    if kind == 1:
        assert yardstick == 0.0


@pytest.mark.parametrize("size,frames", ((s, 12 if s == (96, 54) else 6) for s in SC.ZOOM_SIZES), ids=str)
def test_premises_of_the_gpu_zoom_cases(size, frames):
    a, b = SC.shaky_plan(size, frames), SC.shaky_plan(size, frames, "longdouble")
    differs = int((a["marched"] != b["marched"]).sum())
    print("premises zoom %dx%d: marched samples that differ %d of %d, iterations %d / %d, z %.4f .. %.4f" % (
        size + (differs, a["marched"].size, a["iterations"].max(), b["iterations"].max(), a["required_zoom"].min(), a["required_zoom"].max())))
    assert differs <= 1e-3 * a["marched"].size
    assert a["iterations"].max() <= 12 and b["iterations"].max() <= 12
    assert np.all(a["frame_status"] == 0) and np.all(np.isfinite(a["required_zoom"]))
    assert K.quaternion_angle(a["path_q"], b["path_q"]).max() <= 1e-13


@pytest.mark.parametrize("mode", (1, 2))
def test_the_restatement_leaves_no_invalid_pixel(mode):
    p = SC.shaky_plan((96, 54), 40)
    sc = SC.restatement_scene(SC.shaky_args((96, 54), 40))
    Z, clamped = SR.applied_zoom(sc.frame_t, p["required_zoom"], p["frame_status"], mode, 0.1)
    assert np.all(Z >= p["required_zoom"]) and not clamped.any() and p["required_zoom"].max() > 1.02
    valid = SR.stab_map(sc, p["correction_q"], Z)[1]
    print("guarantee mode %d: zoom %.4f .. %.4f, invalid pixels %d" % (mode, Z.min(), Z.max(), int((valid == 0).sum())))
    assert np.all(valid == 1)
    bare = SR.stab_pixels(sc, p["correction_q"], np.ones(40), frames=[int(np.argmax(p["required_zoom"]))])[1]
    assert (bare[int(np.argmax(p["required_zoom"]))] == 0).any()


# ---------------------------------------------------------------- rendered scene
def _pattern(d):
    """A smooth pattern on the sphere of directions, 0 .. 255."""
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return 127.5 + 60.0 * np.sin(9.0 * d[..., 0] + 2.0 * d[..., 1]) + 55.0 * np.cos(11.0 * d[..., 1] - 3.0 * d[..., 0]) * d[..., 2]


@functools.lru_cache(maxsize=None)
def rendered_scene_errors():
    """(static interpolation error, stabilised error, unstabilised error) in gray levels, mean absolute over the valid pixels, for
    the gopro9_division camera at 480 x 270 and its balance-0 rectified pinhole, 9 shaking frames at fixed zoom, two of them
    rendered."""
    sm, si, _, _ = S.CAMERAS["gopro9_division"]
    sw, sh = 480, 270
    si = np.array(si, dtype=np.float64); si[0] *= 0.5; si[2] = (si[2] + 0.5) * 0.5 - 0.5; si[3] = (si[3] + 0.5) * 0.5 - 0.5; si[4] *= 4.0
    di = R.rectified_pinhole(sm, si, sw, sh, 0.0)
    kw = SC.clip_args(9)
    kw.update(src=(sm, si, sw, sh), dst=(S.CAM_PINHOLE, di, sw, sh), line_delay_s=2 * SC.LINE_DELAY, reference_row=128.0)
    kw["frame_t"] = (SC.T_BASE + 0.05 + 0.02 * np.arange(9)) - 128.0 * 2 * SC.LINE_DELAY
    sc = SC.restatement_scene(kw)
    p = SR.plan(sc, 0.05, 0.0, 1)
    assert np.all(p["frame_status"] == 0) and SR.correction_angle(p["correction_q"]).max() > 5e-3
    uv = R.pixel_grid(sw, sh)
    xy, status = R.unproject(sm, si, uv)
    assert np.all(status == 0)
    d = np.concatenate([xy, np.ones((len(xy), 1))], 1)
    gs = np.clip(np.floor(_pattern(d) + 0.5), 0, 255).astype(np.uint8).reshape(1, sh, sw)
    static_map, static_valid, _, _ = R.rectify_map(sm, si, sw, sh, S.CAM_PINHOLE, di, sw, sh)
    one = RS.Scene(**dict(kw, frame_t=kw["frame_t"][:1], gyro_rates=kw["gyro_rates"] * 0.0))
    truth_static = _pattern(RS.destination_rays(one)[0]).reshape(sh, sw)
    static_err = float(np.abs(R.remap(gs, static_map)[0].astype(np.float64) - truth_static)[static_valid == 1].mean())
    tabs = RS.tables(sc)[1]
    stab_err, bare_err = [], []
    for k in (3, 6):
        Pk = RS.qmat(p["path_q"][k]); Sk = RS.qmat(p["smooth_q"][k])
        # the source frame, per pixel at its own row time: its ray turned into the world (the first frame's reference orientation)
        M = RS.qmat(RS.table_rotation(tabs[k], RS.row_tau(sc, uv[:, 1], np.float64)))
        rolled = np.clip(np.floor(_pattern(np.einsum("ij,njk,nk->ni", Pk, M, d)) + 0.5), 0, 255).astype(np.uint8).reshape(1, sh, sw)
        # the virtual camera (S_k, Z_k), rendered directly
        virt = SR.frame_scene(sc, k, np.array([1.0, 0.0, 0.0, 0.0]), p["zoom"][k])
        truth = _pattern(RS.destination_rays(virt)[0] @ Sk.T).reshape(sh, sw)
        coords, valid, _, _ = SR.stab_pixels(sc, p["correction_q"], p["zoom"], frames=[k])
        assert np.all(valid[k] == 1)
        m = coords[k].astype(np.float32).reshape(sh, sw, 2)
        stab_err.append(float(np.abs(R.remap(rolled, m)[0].astype(np.float64) - truth).mean()))
        bare_err.append(float(np.abs(R.remap(rolled, static_map)[0].astype(np.float64) - truth)[static_valid == 1].mean()))
    return static_err, max(stab_err), min(bare_err), float(p["zoom"][0])


def test_stabilising_a_rendered_shaking_camera_approaches_the_render_of_the_virtual_camera():
    static, stabilised, bare, zoom = rendered_scene_errors()
    print("rendered scene: static-map interpolation error %.3f, stabilised %.3f, unstabilised %.3f gray levels, zoom %.4f" % (static, stabilised, bare, zoom))
    assert stabilised <= 1.25 * static
    assert bare >= 3.0 * static


# ---------------------------------------------------------------- the library without a device
def test_abi_table_and_structs_match_the_header():
    src = open(os.path.join(ROOT, "include", "oicc_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert set(re.findall(r"\boicc_stab_([a-z_]+)\s*\(", src)) == set(_abi.STABILIZATION_SIGNATURES)
    assert set(re.findall(r"\boicc_debug_stab_([a-z_]+)\s*\(", src)) == set(_abi.STABILIZATION_DEBUG_SIGNATURES)
    body = re.search(r"typedef struct oicc_stab_options \{(.*?)\} oicc_stab_options;", src, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*[,;]", body) == [n for n, _ in _abi.StabOptions._fields_]
    assert C.sizeof(_abi.StabOptions) == 40
    stab._bound()                        # binds every entry or raises


@pytest.mark.parametrize("name", list(SC.BAD_SCENES))
def test_bad_scenes_are_refused_before_the_device_is_looked_for(name):
    kw = SC.small_args()
    SC.BAD_SCENES[name](kw)
    assert SC.call_every_entry(rs.Scene(**kw)) == [-1] * 4                    # OICC_ERR_INVALID_ARG, with or without a device


@pytest.mark.parametrize("name", list(SC.BAD_OPTIONS))
def test_bad_options_are_refused_before_the_device_is_looked_for(name):
    scene = rs.Scene(**SC.small_args())
    assert SC.call_every_entry(scene, options=stab.StabOptions(**SC.BAD_OPTIONS[name]))[0] == -1
    t = np.arange(3.0); z = np.ones(3); st = np.zeros(3, np.int32)
    with pytest.raises(ValueError):
        stab.applied_zoom(t, z, st, stab.StabOptions(**SC.BAD_OPTIONS[name]))


def test_bad_plan_arrays_and_frame_arguments_are_refused():
    scene = rs.Scene(**SC.small_args())
    eye = np.tile([1.0, 0.0, 0.0, 0.0], (4, 1))
    for q, z in ((eye * 1.001, np.ones(4)), (eye, np.array([1.0, 0.0, 1.0, 1.0])), (eye, np.array([1.0, np.inf, 1.0, 1.0])), (eye * np.nan, np.ones(4))):
        assert SC.call_every_entry(scene, correction=q, zoom=z)[1:] == [-1] * 3
    assert SC.call_every_entry(scene, channels=2)[2:] == [-1, -1]
    assert SC.call_every_entry(scene, border=256)[2:] == [-1, -1]
    assert SC.call_every_entry(scene, batch=0)[2] == -1


def test_entries_without_a_device():
    import torch
    if torch.cuda.is_available():
        return                      # what a machine without a device answers
    scene = rs.Scene(**SC.small_args())
    assert SC.call_every_entry(scene) == [-2] * 4                           # OICC_ERR_NO_DEVICE
    F = np.zeros((4, 540, 960), np.uint8)
    eye = np.tile([1.0, 0.0, 0.0, 0.0], (4, 1))
    for call in (lambda: stab.stab_plan(scene), lambda: stab.stab_map(scene, eye, np.ones(4)), lambda: stab.stab_frames(F, scene, eye, np.ones(4))):
        with pytest.raises(RuntimeError):
            call()


# ---------------------------------------------------------------- host preparation of the programs, also under sanitizers
@pytest.mark.parametrize("sanitize", (False, True), ids=("plain", "address-undefined"))
def test_host_preparation_equals_the_python_twin(tmp_path, sanitize):
    from openimucameracalibrator_amd import stabilize_frames as prog
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    exe = str(tmp_path / "stabilization_host_driver")
    csrc = os.path.join(ROOT, "openimucameracalibrator_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I", csrc] + extra + [os.path.join(ROOT, "tests", "stabilization_host_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stdout
    rng = np.random.RandomState(8)
    for mode, n in (("none", 0), ("fixed", 1), ("dynamic", 7), ("Dynamic", 3), ("", 2)):
        times = [float(x) for x in rng.uniform(0, 1e4, n)]
        if n >= 3:
            times[2] = times[0]                                  # equal times keep their order
        names = ["%d.png" % rng.randint(0, 2 ** 40) for _ in range(n)]
        status = rng.randint(0, 3, n)
        q = rng.normal(0, 1, (n, 4)); required = 1.0 + rng.rand(n); zoom = 1.0 + rng.rand(n) / 3.0; clamped = rng.randint(0, 2, n)
        if n >= 3:
            required[1] = np.inf; required[2] = np.nan; q[0] = [1.0, 0.0, -0.0, 1e-300]
        args = [mode, str(n)] + [repr(t) for t in times]
        for k in range(n):
            args += [names[k], str(status[k])] + [repr(float(v)) for v in q[k]] + [repr(float(required[k])), repr(float(zoom[k])), str(clamped[k])]
        r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        expect = "mode %s\n" % (stab.ZOOM_MODES[mode] if mode in stab.ZOOM_MODES else "refused")
        expect += "order" + "".join(" %d" % i for i in prog.order_by_time(times)) + "\n"
        expect += prog.plan_json(names, status, q, required, zoom, clamped)
        assert r.stdout == expect
        import json
        doc = json.loads(prog.plan_json(names, status, q, required, zoom, clamped))
        assert [f["name"] for f in doc["frames"]] == names
        for k, f in enumerate(doc["frames"]):
            assert f["correction_q"] == list(q[k]) and f["zoom"] == zoom[k] and (f["required_zoom"] is None) == (not np.isfinite(required[k]))
