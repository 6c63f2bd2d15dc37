"""Loader for the product library liboicc_hip.so (HIP kernels + C-ABI).

There is deliberately no fallback: if the shared object is missing or does not
export every symbol of include/oicc_hip.h this raises, and oicc_create itself
fails when no HIP device is usable.
"""
import ctypes
import os

from ._abi import Bound, BoundAllan, BoundBa, BoundBcrPlan, BoundBoard, BoundCameraMaps, BoundLmRetract, BoundPlanarRansac, BoundRollingShutter, BoundStabilization, BoundStaticImu

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OICC_DEV_LIB") or os.path.join(_HERE, "csrc", "liboicc_hip.so")   # OICC_DEV_LIB: another BUILD of the same library (developer A/B timing, scripts/build_variant.sh)
_bound = None
_bound_ba = None
_bound_allan = None
_bound_static_imu = None
_bound_board = None
_bound_planar_ransac = None
_bound_camera_maps = None
_bound_rolling_shutter = None
_bound_stabilization = None
_bound_bcr_plan = None
_bound_lm_retract = None


def load():
    global _bound
    if _bound is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "liboicc_hip.so not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C openimucameracalibrator_amd/csrc`; there is no CPU fallback." % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        _bound = Bound(lib, "oicc_", device=True)
    return _bound


def load_ba():
    """oicc_ba_* entry points (view bundle adjustment) of the same library."""
    global _bound_ba
    if _bound_ba is None:
        _bound_ba = BoundBa(load().lib, "oicc_ba_")
    return _bound_ba


def load_allan():
    """oicc_allan_* entry points (Allan variance and noise-model fit) of the same library."""
    global _bound_allan
    if _bound_allan is None:
        _bound_allan = BoundAllan(load().lib, "oicc_allan_")
    return _bound_allan


def load_static_imu():
    """oicc_static_imu_* entry points (static multi-pose IMU intrinsics) of the same library."""
    global _bound_static_imu
    if _bound_static_imu is None:
        _bound_static_imu = BoundStaticImu(load().lib, "oicc_static_imu_")
    return _bound_static_imu


def load_board():
    """oicc_board_* entry points (radon checkerboard extraction) of the same library."""
    global _bound_board
    if _bound_board is None:
        _bound_board = BoundBoard(load().lib, "oicc_board_")
    return _bound_board


def load_planar_ransac():
    """oicc_planar_ransac (robust start poses) of the same library."""
    global _bound_planar_ransac
    if _bound_planar_ransac is None:
        _bound_planar_ransac = BoundPlanarRansac(load().lib, "oicc_planar_")
    return _bound_planar_ransac


def load_camera_maps():
    """oicc_camera_* entry points (pixel -> ray, rectification maps, discrepancy, remap) of the same library."""
    global _bound_camera_maps
    if _bound_camera_maps is None:
        _bound_camera_maps = BoundCameraMaps(load().lib, "oicc_camera_")
    return _bound_camera_maps


def load_rolling_shutter():
    """oicc_rs_* entry points (rolling-shutter row maps, rectified frames, points, row rotations) of the same library."""
    global _bound_rolling_shutter
    if _bound_rolling_shutter is None:
        _bound_rolling_shutter = BoundRollingShutter(load().lib, "oicc_rs_")
    return _bound_rolling_shutter


def load_stabilization():
    """oicc_stab_* entry points (orientation path, smooth camera, zoom, stabilised maps and frames) of the same library."""
    global _bound_stabilization
    if _bound_stabilization is None:
        _bound_stabilization = BoundStabilization(load().lib, "oicc_stab_")
    return _bound_stabilization


def load_bcr_plan():
    """oicc_debug_bcr_plan (elimination plan of the block cyclic reduction; needs no device) of the same library."""
    global _bound_bcr_plan
    if _bound_bcr_plan is None:
        _bound_bcr_plan = BoundBcrPlan(load().lib, "oicc_debug_bcr_")
    return _bound_bcr_plan


def load_lm_retract():
    """oicc_debug_lm_retract (one LM solve with its retraction, and the stand-alone retraction kernel on the same step) of the same library."""
    global _bound_lm_retract
    if _bound_lm_retract is None:
        _bound_lm_retract = BoundLmRetract(load().lib, "oicc_debug_lm_")
    return _bound_lm_retract
