"""The stabilisation on the device (csrc/stabilization.hip) against its numpy specification tests/stabilization_restatement.py.

The yardstick of a case is the distance of the float64 restatement from its numpy.longdouble run; the device may be ten times that
away from the float64 restatement ("Stabilisation", holds the measured ratios).  The warp is held bit for bit: to the
rolling-shutter map called with R9 = M_k and the scaled destination, to the rolling-shutter frames for the identity plan, to the
static camera map for zero rates."""
import numpy as np
import pytest

import rolling_shutter_cases as K
import rolling_shutter_restatement as RS
import stabilization_cases as SC
import stabilization_restatement as SR
from openimucameracalibrator_amd import camera_maps as cm
from openimucameracalibrator_amd import rolling_shutter as rs
from openimucameracalibrator_amd import stabilization as stab

pytestmark = pytest.mark.gpu

NO_SMOOTHING = dict(smoothing_sigma_s=0.0, zoom_mode="none")


# ---------------------------------------------------------------- path
@pytest.mark.parametrize("kind", SC.PATH_COUNTS + ("mixed",), ids=str)
def test_path_against_restatement(kind):
    kw = SC.mixed_args() if kind == "mixed" else SC.clip_args(kind)
    ref, _, yardstick = SC.path_reference(kind)
    p = stab.stab_plan(rs.Scene(**kw), stab.StabOptions(**NO_SMOOTHING))
    on = ~np.isnan(ref[:, 0])
    assert np.array_equal(np.isnan(p.path_q[:, 0]), ~on)
    assert np.array_equal(p.frame_status, RS.frame_windows(SC.restatement_scene(kw))[0])
    if kind == "mixed":
        assert list(p.frame_status) == SC.MIXED_STATUS and list(on) == [s == 0 for s in SC.MIXED_STATUS]
    else:
        assert np.all(on) and SR.scan_run(kind) == 4
    first = int(np.argmax(on))
    assert np.array_equal(p.path_q[first], [1.0, 0.0, 0.0, 0.0])
    distance = float(K.quaternion_angle(ref[on], p.path_q[on]).max())
    print("path %s: yardstick (float64 vs longdouble) %.3e rad, device vs float64 %.3e rad" % (kind, yardstick, distance))
    assert distance <= 10.0 * yardstick
    assert np.abs(np.linalg.norm(p.path_q[on], axis=1) - 1.0).max() <= 1e-15 * 4
    # sigma 0: the smooth camera is the path bit for bit, the correction the identity, the zoom of mode 0 is 1
    assert np.array_equal(p.smooth_q[on], p.path_q[on]) and np.all(np.isnan(p.smooth_q[~on]))
    assert np.array_equal(p.correction_q, np.tile([1.0, 0.0, 0.0, 0.0], (len(on), 1)))
    assert np.all(p.iterations == 0) and np.all(p.zoom == 1.0) and not p.zoom_clamped.any()


# ---------------------------------------------------------------- smoothing
@pytest.mark.parametrize("name", list(SC.SIGMAS))
def test_smooth_camera_against_restatement(name):
    r = SC.smooth_reference(name)
    members = set(int(m) for m in r["members"])
    assert {"none": {1}, "65": {63, 64, 65}, "201": {200}, "clip": {257}}[name] <= members      # the window sizes this case covers
    p = stab.stab_plan(rs.Scene(**SC.clip_args(257)), stab.StabOptions(smoothing_sigma_s=SC.SIGMAS[name], zoom_mode="none"))
    if name == "none":
        assert np.array_equal(p.smooth_q, p.path_q) and np.array_equal(p.correction_q, np.tile([1.0, 0.0, 0.0, 0.0], (257, 1)))
        assert np.array_equal(RS.qmat(p.correction_q), np.tile(np.eye(3), (257, 1, 1)))
        return
    yard_s = float(K.quaternion_angle(r["S"], r["S_ld"]).max()); yard_c = float(K.quaternion_angle(r["C"], r["C_ld"]).max())
    dist_s = float(K.quaternion_angle(r["S"], p.smooth_q).max()); dist_c = float(K.quaternion_angle(r["C"], p.correction_q).max())
    print("smoothing %s: S yardstick %.3e rad, device %.3e rad; C yardstick %.3e rad, device %.3e rad; iterations device %d restatement %d" % (
        name, yard_s, dist_s, yard_c, dist_c, p.iterations.max(), r["iterations"].max()))
    assert dist_s <= 10.0 * yard_s and dist_c <= 10.0 * yard_c
    assert p.iterations.max() <= 12 and p.iterations.min() >= 1
    assert np.all(p.correction_q[:, 0] > 0)


def test_correction_clamp_just_below_and_just_above():
    r = SC.smooth_reference("clip")
    angles = SR.correction_angle(r["C"])
    k = int(np.argsort(angles)[len(angles) // 2])            # a frame in the middle of the angles
    scene = rs.Scene(**SC.clip_args(257))
    free = stab.stab_plan(scene, stab.StabOptions(smoothing_sigma_s=SC.SIGMAS["clip"], zoom_mode="none"))
    for factor, clamped in ((1.0 + 1e-9, False), (1.0 - 1e-9, True)):
        bound = float(angles[k]) * factor
        p = stab.stab_plan(scene, stab.StabOptions(smoothing_sigma_s=SC.SIGMAS["clip"], max_correction_rad=bound, zoom_mode="none"))
        ext = SC.smooth_reference("clip", bound)
        ref = ext["C"]
        yardstick = float(K.quaternion_angle(ext["C"], ext["C_ld"]).max())
        got = SR.correction_angle(p.correction_q)
        below = angles < bound * (1.0 - 1e-6); above = angles > bound * (1.0 + 1e-6)
        assert below.sum() > 50 and above.sum() > 50
        assert np.array_equal(p.correction_q[below], free.correction_q[below])           # untouched
        assert np.array_equal(p.smooth_q, free.smooth_q)                                 # the mean itself is not clamped
        assert np.abs(got[above] - bound).max() <= 4 * np.finfo(np.float64).eps
        assert np.array_equal(p.correction_q[k], free.correction_q[k]) != clamped
        assert K.quaternion_angle(ref, p.correction_q).max() <= 10.0 * yardstick
        # shortened along its own axis
        axis = lambda q: q[:, 1:] / np.linalg.norm(q[:, 1:], axis=1, keepdims=True)
        assert np.abs(axis(p.correction_q[above]) - axis(free.correction_q[above])).max() <= 1e-12


# ---------------------------------------------------------------- zoom
@pytest.mark.parametrize("size", SC.ZOOM_SIZES, ids=lambda s: "%dx%d" % s)
def test_still_camera_needs_no_zoom(size):
    p = stab.stab_plan(rs.Scene(**SC.still_args(size)), stab.StabOptions(smoothing_sigma_s=0.05, zoom_mode="fixed"))
    assert np.all(p.frame_status == 0)
    assert np.array_equal(p.required_zoom, np.ones(3)) and np.array_equal(p.zoom, np.ones(3)) and not p.zoom_clamped.any()


@pytest.mark.parametrize("alpha", (0.02, 0.1, -0.25))
def test_roll_of_a_centred_pinhole_is_the_closed_form(alpha):
    """Pixel offsets (a, b) from the centre, |a| <= W = (w - 1) / 2, |b| <= H = (h - 1) / 2, turn into s (a cos - b sin, a sin + b cos)
    and must stay inside the same rectangle.  Both coordinates are linear along an edge, so the corners bind: for the corner (W, H)
    and alpha > 0, s (W cos + H sin) <= W and s (W sin + H cos) <= H, i.e. 1 / s >= cos + max(H / W, W / H) sin; the other corners
    and the other sign give the same with |alpha|.  The corners are border pixels themselves: no sampling error.  The bisection
    keeps the valid end of an interval of 2^-16 / 32: z lies above the closed form by the relative 2^-16 / 32 at the most, and never below
    it but for the rounding of the arithmetic (1e-12)."""
    w, h = 96, 54
    p = stab.stab_plan(rs.Scene(**SC.still_args((w, h), R=SC.roll_matrix(alpha))), stab.StabOptions(smoothing_sigma_s=0.0, zoom_mode="fixed"))
    a = abs(alpha)
    z = np.cos(a) + max((w - 1.0) / (h - 1.0), (h - 1.0) / (w - 1.0)) * np.sin(a)
    print("roll %.2f: closed form %.9f, device %s" % (alpha, z, p.required_zoom))
    assert np.all(p.required_zoom >= z * (1.0 - 1e-12))
    assert np.all(p.required_zoom <= z * (1.0 + 2.0 ** -16 / 32.0) + 1e-12)
    assert np.array_equal(p.zoom, np.full(3, p.required_zoom.max()))


def test_invalid_centre_gives_infinite_zoom_and_the_clamp_flag():
    c, s = np.cos(1.8), np.sin(1.8)
    turned = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])          # the destination looks backwards: its centre ray has z < 0
    p = stab.stab_plan(rs.Scene(**SC.still_args((67, 5), R=turned)), stab.StabOptions(smoothing_sigma_s=0.0, zoom_mode="fixed", max_zoom=3.0))
    assert np.all(p.frame_status == 0) and np.all(np.isposinf(p.required_zoom))
    assert np.array_equal(p.zoom, np.full(3, 3.0)) and np.all(p.zoom_clamped == 1)


@pytest.mark.parametrize("size", SC.ZOOM_SIZES, ids=lambda s: "%dx%d" % s)
def test_required_zoom_against_restatement(size):
    """Device and restatement bisect towards the same boundary wherever their marched samples agree (a premise of the CPU tests for
    the two precisions of the restatement); each keeps a valid end at most 2^-16 / 32 below it.  So s may differ by that resolution,
    plus ten yardsticks."""
    frames = 12 if size == (96, 54) else 6
    ref, ext = SC.shaky_plan(size, frames), SC.shaky_plan(size, frames, "longdouble")
    p = stab.stab_plan(rs.Scene(**SC.shaky_args(size, frames)), stab.StabOptions(smoothing_sigma_s=SC.SHAKY_SIGMA, zoom_mode="fixed", max_zoom=100.0))
    assert np.all(p.frame_status == 0) and np.all(np.isfinite(p.required_zoom))
    yardstick = float(np.abs(1.0 / ref["required_zoom"] - 1.0 / ext["required_zoom"]).max())
    distance = float(np.abs(1.0 / p.required_zoom - 1.0 / ref["required_zoom"]).max())
    print("zoom %dx%d: s yardstick %.3e, device vs float64 %.3e, z from %.4f to %.4f" % (size + (yardstick, distance, p.required_zoom.min(), p.required_zoom.max())))
    assert distance <= 2.0 ** -21 + 10.0 * yardstick
    assert np.array_equal(p.zoom, np.full(frames, p.required_zoom.max())) and not p.zoom_clamped.any()
    if size == (1, 1):
        assert np.array_equal(p.required_zoom, np.ones(frames))


# ---------------------------------------------------------------- warp
WARP_ZOOMS = np.array([1.0, 1.1, 1.37, 2.0, 0.8])
WARP_SIGMA = 0.2          # five frames 0.16 s apart: every window holds them all


def _warp_scene(frames=5, size=(67, 5), uncovered_first=False):
    kw = SC.shaky_args(size, frames)
    c, s = np.cos(0.03), np.sin(0.03)
    kw["R"] = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, np.cos(0.02), -np.sin(0.02)], [0.0, np.sin(0.02), np.cos(0.02)]])
    if uncovered_first:
        kw["frame_t"] = np.concatenate([[kw["frame_t"][0] - 0.5], kw["frame_t"][1:]])
    return kw


@pytest.mark.parametrize("size", ((67, 5), (96, 54)), ids=lambda s: "%dx%d" % s)
def test_map_is_the_rolling_shutter_map_with_the_frame_rotation_and_zoom(size):
    kw = _warp_scene(5, size)
    scene = rs.Scene(**kw)
    p = stab.stab_plan(scene, stab.StabOptions(smoothing_sigma_s=WARP_SIGMA, zoom_mode="dynamic", zoom_window_s=0.1, max_zoom=100.0))
    assert np.all(p.frame_status == 0) and SR.correction_angle(p.correction_q).max() > 1e-3
    p.zoom = p.zoom * WARP_ZOOMS              # the entry takes any zoom; below 1 the borders show
    mapxy, valid, status, num_valid, evals = stab.stab_map(scene, p.correction_q, p.zoom, return_evaluations=True)
    assert mapxy.shape == (5, size[1], size[0], 2) and np.array_equal(num_valid, valid.reshape(5, -1).sum(1))
    sc = SC.restatement_scene(kw)
    for k in range(5):
        one = SR.frame_scene(sc, k, p.correction_q[k], p.zoom[k])          # M_k and the scaled intrinsics in the kernel's order
        kw1 = dict(kw, frame_t=kw["frame_t"][k:k + 1], dst=one.dst, R=one.Rm)
        m1, v1, s1, n1, e1 = rs.rs_rectify_map(rs.Scene(**kw1), return_evaluations=True)
        assert np.array_equal(mapxy[k].view(np.uint32), m1[0].view(np.uint32)), k
        assert np.array_equal(valid[k], v1[0]) and np.array_equal(evals[k], e1[0]) and num_valid[k] == n1[0]
    assert valid.any()


def test_zero_rates_with_a_constant_correction_give_the_static_map():
    kw = _warp_scene(3)
    kw["gyro_rates"] = kw["gyro_rates"] * 0.0
    (sm, si, sw, sh), (dm, di, dw, dh) = kw["src"], kw["dst"]
    q = np.array([np.cos(0.04), 0.6 * np.sin(0.04), -0.8 * np.sin(0.04), 0.0])
    zoom = np.array([1.0, 1.25, 1.7])
    mapxy, valid, status, num_valid = stab.stab_map(rs.Scene(**kw), np.tile(q, (3, 1)), zoom)
    sc = SC.restatement_scene(kw)
    for k in range(3):
        one = SR.frame_scene(sc, k, q, zoom[k])
        static_map, static_valid, static_num = cm.rectify_map(sm, si, sw, sh, dm, one.dst[1], dw, dh, R=one.Rm)
        assert np.array_equal(mapxy[k].view(np.uint32), static_map.view(np.uint32)), k
        assert np.array_equal(valid[k], static_valid) and num_valid[k] == static_num


def _random_frames(num_frames, channels, seed=0):
    rng = np.random.RandomState(seed + 10 * num_frames + channels)
    return rng.randint(0, 256, (num_frames, 540, 960) if channels == 1 else (num_frames, 540, 960, channels)).astype(np.uint8)


@pytest.mark.parametrize("num_frames", (1, 5))
@pytest.mark.parametrize("channels", (1, 3))
def test_frames_equal_remapping_through_the_maps_and_the_identity_plan_is_the_rolling_shutter_entry(channels, num_frames):
    kw = _warp_scene(num_frames, uncovered_first=num_frames == 5)     # at batch 2 the uncovered frame sits inside the first batch
    scene = rs.Scene(**kw)
    F = _random_frames(num_frames, channels)
    p = stab.stab_plan(scene, stab.StabOptions(smoothing_sigma_s=WARP_SIGMA, zoom_mode="dynamic", zoom_window_s=0.1, max_zoom=100.0))
    assert list(p.frame_status) == ([1, 0, 0, 0, 0] if num_frames == 5 else [0])
    p.zoom = p.zoom * WARP_ZOOMS[:num_frames][::-1]
    rep = {}
    out, status = stab.stab_frames(F, scene, p.correction_q, p.zoom, border_value=9, batch=2, report=rep)
    mapxy, valid, map_status, _ = stab.stab_map(scene, p.correction_q, p.zoom)
    assert np.array_equal(status, p.frame_status) and np.array_equal(map_status, p.frame_status)
    for k in range(num_frames):
        assert np.array_equal(out[k], cm.remap(F[k:k + 1], mapxy[k], border_value=9)[0]), k
        if status[k] != 0:
            assert np.all(out[k] == 9) and not valid[k].any()
    assert (out[-1] != 9).any() and rep["ms_kernel"] > 0 and rep["ms_total"] >= rep["ms_kernel"]
    # C = identity, Z = 1: the rolling-shutter entries byte for byte
    eye = np.tile([1.0, 0.0, 0.0, 0.0], (num_frames, 1)); ones = np.ones(num_frames)
    plain, plain_status = stab.stab_frames(F, scene, eye, ones, border_value=9, batch=2)
    rolled, rolled_status = rs.rs_rectify_frames(F, scene, border_value=9, batch=2)
    assert np.array_equal(plain, rolled) and np.array_equal(plain_status, rolled_status)
    m0, v0 = stab.stab_map(scene, eye, ones)[:2]
    m1, v1 = rs.rs_rectify_map(scene)[:2]
    assert np.array_equal(m0.view(np.uint32), m1.view(np.uint32)) and np.array_equal(v0, v1)


def test_frames_on_a_cuda_tensor_equal_the_host_route_and_host_arrays_are_refused():
    import ctypes as C
    import torch
    from openimucameracalibrator_amd import _abi
    kw = _warp_scene(5, uncovered_first=True)
    scene = rs.Scene(**kw)
    p = stab.stab_plan(scene, stab.StabOptions(smoothing_sigma_s=WARP_SIGMA, zoom_mode="fixed", max_zoom=100.0))
    for channels in (1, 3):
        F = _random_frames(5, channels)
        host, host_status = stab.stab_frames(F, scene, p.correction_q, p.zoom, border_value=17, batch=2)
        t = torch.from_numpy(F).cuda()
        out, status = stab.stab_frames(t, scene, p.correction_q, p.zoom, border_value=17)
        assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8
        assert np.array_equal(out.cpu().numpy(), host) and np.array_equal(status, host_status)
    b = stab._bound()
    F = _random_frames(5, 1); o_host = np.zeros((5, 5, 67), np.uint8); st = np.zeros(5, np.int32)
    t = torch.from_numpy(F).cuda(); o = torch.zeros((5, 5, 67), dtype=torch.uint8, device="cuda")
    q = np.ascontiguousarray(p.correction_q); z = np.ascontiguousarray(p.zoom)
    dp = lambda a: a.ctypes.data_as(_abi.c_dp)
    u8 = lambda x: C.cast(x.data_ptr(), _abi.c_u8p)
    i32 = st.ctypes.data_as(_abi.c_i32p)
    assert b.frames_device(None, scene.ref(), dp(q), dp(z), 1, u8(t), 0, u8(o), i32) == 0
    torch.cuda.synchronize()
    assert b.frames_device(None, scene.ref(), dp(q), dp(z), 1, F.ctypes.data_as(_abi.c_u8p), 0, u8(o), i32) == -1
    assert b.frames_device(None, scene.ref(), dp(q), dp(z), 1, u8(t), 0, o_host.ctypes.data_as(_abi.c_u8p), i32) == -1


# ---------------------------------------------------------------- the guarantee
@pytest.mark.parametrize("mode", ("fixed", "dynamic"))
def test_no_invalid_pixel_in_a_stabilised_frame(mode):
    kw = SC.shaky_args((96, 54), 40)
    scene = rs.Scene(**kw)
    p = stab.stab_plan(scene, stab.StabOptions(smoothing_sigma_s=SC.SHAKY_SIGMA, zoom_mode=mode, zoom_window_s=0.1, max_zoom=100.0))
    assert np.all(p.frame_status == 0) and not p.zoom_clamped.any()
    assert np.all(p.zoom >= p.required_zoom) and p.required_zoom.max() > 1.02
    mapxy, valid, status, num_valid = stab.stab_map(scene, p.correction_q, p.zoom)
    print("guarantee %s: zoom from %.4f to %.4f, invalid pixels %d" % (mode, p.zoom.min(), p.zoom.max(), int((valid == 0).sum())))
    assert np.all(num_valid == 96 * 54)
    # without the zoom the borders show: the guarantee is the zoom's doing
    bare = stab.stab_map(scene, p.correction_q, np.ones(40))[3]
    assert (bare < 96 * 54).any()
