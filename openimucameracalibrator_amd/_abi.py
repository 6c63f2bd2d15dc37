"""ctypes description of the C-ABI declared in include/oicc_hip.h.

The same table binds any library that exports these entry points under a
prefix: the product library liboicc_hip.so uses ``oicc_``.  (The test suite
binds its CPU checker with another prefix; nothing in this package does.)
"""
import ctypes as C

c_i64p = C.POINTER(C.c_int64)
c_i32p = C.POINTER(C.c_int32)
c_dp = C.POINTER(C.c_double)
c_u8p = C.POINTER(C.c_uint8)


class Summary(C.Structure):
    """oicc_summary (include/oicc_hip.h)."""
    _fields_ = [
        ("termination", C.c_int32), ("num_iterations", C.c_int32),
        ("num_successful_steps", C.c_int32), ("num_unsuccessful_steps", C.c_int32),
        ("num_parameters_tangent", C.c_int32), ("band_dim", C.c_int32),
        ("arrow_dim", C.c_int32), ("half_bandwidth", C.c_int32),
        ("num_residual_blocks", C.c_int64), ("num_residuals", C.c_int64),
        ("initial_cost", C.c_double), ("final_cost", C.c_double),
        ("final_radius", C.c_double), ("final_gradient_max_norm", C.c_double),
        ("seconds_total", C.c_double), ("seconds_jacobian", C.c_double),
        ("seconds_residual", C.c_double), ("seconds_linear_solver", C.c_double),
        ("message", C.c_char * 128),
        ("inner_sweeps", C.c_int32), ("line_search_steps", C.c_int32), ("inner_lm_iterations", C.c_int64),
        ("seconds_inner", C.c_double),
        ("seconds_setup", C.c_double),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["message"] = self.message.decode()
        return d


class Iteration(C.Structure):
    """oicc_iteration (include/oicc_hip.h)."""
    _fields_ = [
        ("iteration", C.c_int32), ("step_is_successful", C.c_int32),
        ("cost", C.c_double), ("cost_change", C.c_double),
        ("gradient_max_norm", C.c_double), ("step_norm", C.c_double),
        ("relative_decrease", C.c_double), ("trust_region_radius", C.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class CovarianceInfo(C.Structure):
    """oicc_covariance_info (include/oicc_hip.h)."""
    _fields_ = [("status", C.c_int32), ("P", C.c_int32), ("Pb", C.c_int32), ("a", C.c_int32), ("hb", C.c_int32),
                ("num_residuals", C.c_int64), ("cost", C.c_double), ("variance_factor", C.c_double), ("rcond", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class BaCovarianceInfo(C.Structure):
    """oicc_ba_covariance_info (include/oicc_hip.h)."""
    _fields_ = [("status", C.c_int32), ("P", C.c_int32), ("pose_dim", C.c_int32), ("a", C.c_int32), ("views_used", C.c_int32),
                ("first_bad", C.c_int32), ("num_residuals", C.c_int64), ("cost", C.c_double), ("variance_factor", C.c_double),
                ("rcond", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ResidualInfo(C.Structure):
    """oicc_residual_info (include/oicc_hip.h)."""
    _fields_ = [("num_corners", C.c_int64), ("num_used", C.c_int64), ("num_failed", C.c_int64), ("num_gated", C.c_int64),
                ("num_views", C.c_int64), ("num_accl", C.c_int64), ("num_gyro", C.c_int64),
                ("mean_px", C.c_double), ("rms_px", C.c_double), ("median_px", C.c_double), ("sigma_px", C.c_double), ("max_px", C.c_double),
                ("accl_rms", C.c_double * 3), ("accl_rms_weighted", C.c_double * 3), ("gyro_rms", C.c_double * 3), ("gyro_rms_weighted", C.c_double * 3),
                ("ms_device", C.c_double)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if k.endswith(("_rms", "_rms_weighted")) else getattr(self, k)) for k, _ in self._fields_}


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p)   # oicc_exchange_fn

H = C.c_void_p  # oicc_problem*

# name -> (restype, argtypes); every entry is exported by liboicc_hip.so.
SIGNATURES = {
    "create": (C.c_int, [C.POINTER(H), C.c_int]),
    "destroy": (None, [H]),
    "last_error": (C.c_char_p, [H]),
    "version": (C.c_char_p, []),
    "set_option": (C.c_int, [H, C.c_char_p, C.c_double]),
    "set_times": (C.c_int, [H, C.c_int64, C.c_int64, C.c_int64, C.c_int64]),
    "get_num_so3_knots": (C.c_int64, [H]),
    "get_num_r3_knots": (C.c_int64, [H]),
    "get_min_time_ns": (C.c_int64, [H]),
    "get_max_time_ns": (C.c_int64, [H]),
    "set_so3_knots": (C.c_int, [H, c_dp, C.c_int64]),
    "set_r3_knots": (C.c_int, [H, c_dp, C.c_int64]),
    "get_so3_knots": (C.c_int, [H, c_dp, C.c_int64]),
    "get_r3_knots": (C.c_int, [H, c_dp, C.c_int64]),
    "init_bias_splines": (C.c_int, [H, c_dp, c_dp, C.c_int64, C.c_int64, C.c_double, C.c_double]),
    "set_T_i_c": (C.c_int, [H, c_dp]),
    "set_gravity": (C.c_int, [H, c_dp]),
    "set_camera_line_delay": (C.c_int, [H, C.c_double]),
    "set_imu_intrinsics": (C.c_int, [H, c_dp, c_dp]),
    "set_camera": (C.c_int, [H, C.c_int32, c_dp, C.c_int32]),
    "set_scene_points": (C.c_int, [H, c_dp, C.c_int64]),
    "get_scene_points": (C.c_int, [H, c_dp, C.c_int64]),
    "get_scene_point_offsets": (C.c_int, [H, C.c_int32, c_i32p]),
    "add_rs_camera_measurements": (C.c_int, [H, C.c_int64, c_i64p, c_i64p, c_dp, c_dp, c_i32p, c_u8p]),
    "add_gs_camera_measurements": (C.c_int, [H, C.c_int64, c_i64p, c_i64p, c_dp, c_dp, c_i32p, c_u8p]),
    "add_accelerometer_measurements": (C.c_int, [H, C.c_int64, c_i64p, c_dp, C.c_double, c_u8p]),
    "add_gyroscope_measurements": (C.c_int, [H, C.c_int64, c_i64p, c_dp, C.c_double, c_u8p]),
    "optimize": (C.c_int, [H, C.c_int32, C.c_int32, C.POINTER(Summary)]),
    "get_iterations": (C.c_int, [H, C.POINTER(Iteration), C.c_int32]),
    "get_inner_set_costs": (C.c_int, [H, c_dp, C.c_int32]),
    "get_tangent_layout": (C.c_int, [H, C.c_int32, c_i32p, c_i32p, c_i32p, c_i32p, c_i32p, c_i32p]),
    "evaluate": (C.c_int, [H, C.c_int32, c_dp, c_dp, c_dp, C.c_int32]),
    "evaluate_cost": (C.c_int, [H, C.c_int32, c_dp]),
    "evaluate_entries": (C.c_int, [H, C.c_int32, C.c_int64, c_i32p, c_i32p, c_dp]),
    "evaluate_blocks": (C.c_int, [H, C.c_int32, C.c_int32, c_dp, c_dp]),
    "get_T_i_c": (C.c_int, [H, c_dp]),
    "get_gravity": (C.c_int, [H, c_dp]),
    "get_rs_line_delay": (C.c_int, [H, c_dp]),
    "get_imu_intrinsics": (C.c_int, [H, c_dp, c_dp]),
    "get_bias_knots": (C.c_int, [H, c_dp, C.c_int64, c_dp, C.c_int64]),
    "get_num_accl_bias_knots": (C.c_int64, [H]),
    "get_num_gyro_bias_knots": (C.c_int64, [H]),
    "get_mean_reprojection_error": (C.c_int, [H, c_dp, c_i64p]),
    "declare_remote_measurements": (C.c_int, [H, C.c_int32, C.c_int64, c_i64p]),
    "get_trajectory": (C.c_int, [H, C.c_int64, c_i64p, c_dp, c_dp, c_dp, c_dp, c_dp, c_u8p]),
}

# Entry points that only the device library has (streams, collectives, timers).
DEVICE_ONLY = {
    "set_stream": (C.c_int, [H, C.c_void_p]),
    "set_allreduce": (C.c_int, [H, ALLREDUCE_FN, C.c_void_p]),
    "time_jacobian_pass": (C.c_int, [H, C.c_int32, C.c_int32, c_dp, c_dp]),
    "time_linear_solve": (C.c_int, [H, C.c_int32, C.c_int32, c_dp]),
    "solve_residual": (C.c_int, [H, C.c_int32, C.c_double, c_dp]),
    "run_lm_iterations": (C.c_int, [H, C.c_int32, C.c_int32]),
    "estimate_imu_to_camera_rotation": (C.c_int, [C.c_int32, C.c_int64, c_dp, c_dp, C.c_int64, c_dp, c_dp, C.c_double, C.c_int32,
                                                  c_dp, c_dp, c_dp, c_dp, c_i32p]),
    "rccl_get_unique_id": (C.c_int, [c_u8p]),
    "rccl_init": (C.c_int, [H, C.c_int32, C.c_int32, c_u8p]),
    "set_inner_iteration_source": (C.c_int, [H, H]),
    "time_allreduce": (C.c_int, [H, C.c_int32, C.c_int32, c_dp, c_i64p]),
    "time_exchange": (C.c_int, [H, C.c_int32, C.c_int32, c_dp, c_i64p]),
    "set_shard": (C.c_int, [H, C.c_int32, C.c_int32]),
    "set_exchange": (C.c_int, [H, EXCHANGE_FN, C.c_void_p]),
    "declare_remote_measurements_from": (C.c_int, [H, C.c_int32, C.c_int32, C.c_int64, c_i64p]),
    "estimate_covariance": (C.c_int, [H, C.c_int32, C.POINTER(CovarianceInfo)]),
    "get_covariance_arrow": (C.c_int, [H, c_dp, C.c_int32]),
    "get_covariance_knots": (C.c_int, [H, c_dp, C.c_int64, c_dp, C.c_int64]),
    "get_covariance_knot_arrow": (C.c_int, [H, C.c_int32, C.c_int64, c_dp]),
    "get_covariance_timing": (C.c_int, [H, c_dp]),
    "residual_report": (C.c_int, [H, C.POINTER(ResidualInfo)]),
    "get_corner_errors": (C.c_int, [H, c_dp, c_u8p, C.c_int64]),
    "get_view_errors": (C.c_int, [H, c_dp, c_dp, c_i32p, C.c_int64]),
    "get_imu_residuals": (C.c_int, [H, C.c_int32, c_dp, C.c_int64]),
    "gate_corners": (C.c_int, [H, C.c_double, c_i64p]),
    "get_corner_gate": (C.c_int, [H, c_u8p, C.c_int64]),
    "sew_knot_spacing_and_variance": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, c_dp, c_dp, C.c_double, C.c_double, C.c_double,
                                                c_dp, c_dp, c_i32p]),
}


HB = C.c_void_p  # oicc_ba*

# View bundle adjustment (oicc_ba_* in include/oicc_hip.h): name -> (restype, argtypes)
BA_SIGNATURES = {
    "create": (C.c_int, [C.POINTER(HB), C.c_int32]),
    "destroy": (None, [HB]),
    "last_error": (C.c_char_p, [HB]),
    "set_option": (C.c_int, [HB, C.c_char_p, C.c_double]),
    "set_camera": (C.c_int, [HB, C.c_int32, c_dp, C.c_int32]),
    "get_camera": (C.c_int, [HB, c_dp, C.c_int32]),
    "set_scene_points": (C.c_int, [HB, c_dp, C.c_int64]),
    "get_scene_points": (C.c_int, [HB, c_dp, C.c_int64]),
    "set_variable_points": (C.c_int, [HB, c_u8p, C.c_int64]),
    "set_views": (C.c_int, [HB, C.c_int64, c_dp, c_i64p, c_dp, c_i32p]),
    "set_poses": (C.c_int, [HB, c_dp, C.c_int64]),
    "get_poses": (C.c_int, [HB, c_dp, C.c_int64]),
    "evaluate": (C.c_int, [HB, C.c_int32, C.c_int32, c_dp, c_dp, c_dp, C.c_int32]),
    "optimize": (C.c_int, [HB, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Summary)]),
    "get_iterations": (C.c_int, [HB, C.POINTER(Iteration), C.c_int32]),
    "optimize_views": (C.c_int, [HB, C.c_int32, C.c_int32, c_i32p, c_dp]),
    "view_reprojection_errors": (C.c_int, [HB, c_dp]),
    "point_covariances": (C.c_int, [HB, c_dp, C.c_int64, c_dp]),
    "estimate_covariance": (C.c_int, [HB, C.c_int32, C.c_int32, C.POINTER(BaCovarianceInfo)]),
    "get_covariance_intrinsics": (C.c_int, [HB, c_dp, C.c_int32]),
    "get_covariance_poses": (C.c_int, [HB, c_dp, C.c_int64]),
    "get_covariance_pose_intrinsics": (C.c_int, [HB, c_dp, C.c_int64]),
    "get_covariance_timing": (C.c_int, [HB, c_dp]),
}
# Entries of BA_SIGNATURES that only the device library has: the CPU checker, bound with the same table, has no counterpart.
BA_DEVICE_ONLY = ("point_covariances", "estimate_covariance", "get_covariance_intrinsics", "get_covariance_poses",
                  "get_covariance_pose_intrinsics", "get_covariance_timing")


class BoundBa:
    """Bound oicc_ba_* entry points of one library + prefix (``oicc_ba_`` for liboicc_hip.so)."""

    def __init__(self, lib, prefix):
        self.lib = lib
        self.prefix = prefix
        for name, (res, args) in BA_SIGNATURES.items():
            if name in BA_DEVICE_ONLY and prefix != "oicc_ba_" and not hasattr(lib, prefix + name):
                continue
            fn = getattr(lib, prefix + name)  # AttributeError = missing symbol: fail loudly
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, fn)


class Bound:
    """Namespace of bound entry points for one library + prefix."""

    def __init__(self, lib, prefix, device=True):
        self.lib = lib
        self.prefix = prefix
        table = dict(SIGNATURES)
        if device:
            table.update(DEVICE_ONLY)
        for name, (res, args) in table.items():
            fn = getattr(lib, prefix + name)  # AttributeError = missing symbol: fail loudly
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, fn)
        self.device = device


# Debug read-outs of the inner iterations (device library only, outside include/oicc_hip.h: csrc/oicc_inner.hip, csrc/inner_iterations.hip):
# full symbol name -> (restype, argtypes); bound on first use (bind_inner_debug).
INNER_DEBUG_SIGNATURES = {
    "oicc_debug_inner_first_evaluations": (C.c_int, [H, C.c_int32, c_i32p, c_dp, C.c_int32]),
    "oicc_debug_inner_cholesky": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, c_dp, c_dp, c_dp, c_u8p]),
}
INNER_ROUTES = ("set_kernel<0>", "set_kernel<1>", "set_kernel<2>", "wave_kernel", "shared: resident workgroups", "shared: launches")
INNER_KINDS = ("so3", "r3", "T_i_c", "gravity", "line_delay", "accl_bias", "gyro_bias", "accl_intrinsics", "gyro_intrinsics", "point")   # InnerKind, csrc/inner_plan.h


def bind_inner_debug(lib, name, table=INNER_DEBUG_SIGNATURES):
    fn = getattr(lib, name)  # AttributeError = missing symbol: fail loudly
    fn.restype, fn.argtypes = table[name]
    return fn


# The option tables of the two problem objects (csrc/oicc_options.def, csrc/oicc_ba_options.def) and what an option holds (device
# library only, outside include/oicc_hip.h: csrc/oicc_problem.hip, csrc/oicc_ba.hip); bound on first use (bind_option_debug).
OPTION_DEBUG_SIGNATURES = {
    "oicc_debug_option_table": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_char_p), c_dp]),   # (which: 0 oicc_problem, 1 oicc_ba; index) -> number of options
    "oicc_debug_get_option": (C.c_int, [H, C.c_char_p, c_dp]),
    "oicc_debug_ba_get_option": (C.c_int, [HB, C.c_char_p, c_dp]),
}


def bind_option_debug(lib, name):
    return bind_inner_debug(lib, name, OPTION_DEBUG_SIGNATURES)


# IMU noise characterisation (oicc_allan_* in include/oicc_hip.h): name -> (restype, argtypes).  A table of its own:
# SIGNATURES is also bound against the CPU checker, which has no counterpart of these entries.
ALLAN_SIGNATURES = {
    "factors": (C.c_int, [C.c_int64, C.c_int32, c_i32p, c_i32p]),
    "variance": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, c_dp, c_dp, c_dp, C.c_int32, c_i32p, c_i32p, c_dp,
                           c_dp, c_dp, c_dp, c_dp, c_dp]),
    "fit": (C.c_int, [C.c_int32, C.c_int64, c_dp, c_dp, C.c_double, c_dp, c_dp, c_dp, c_i32p, c_i32p]),
}


class BoundAllan:
    """Bound oicc_allan_* entry points of one library + prefix (``oicc_allan_`` for liboicc_hip.so)."""

    def __init__(self, lib, prefix):
        self.lib = lib
        self.prefix = prefix
        for name, (res, args) in ALLAN_SIGNATURES.items():
            fn = getattr(lib, prefix + name)  # AttributeError = missing symbol: fail loudly
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, fn)


class StaticImuOptions(C.Structure):
    """oicc_static_imu_options (include/oicc_hip.h)."""
    _fields_ = [("gravity_magnitude", C.c_double), ("init_interval_duration_s", C.c_double), ("gyro_dt", C.c_double),
                ("interval_n_samples", C.c_int32), ("min_num_intervals", C.c_int32), ("win_size", C.c_int32),
                ("acc_use_means", C.c_int32), ("optimize_gyro_bias", C.c_int32), ("reserved", C.c_int32)]


class StaticImuReport(C.Structure):
    """oicc_static_imu_report (include/oicc_hip.h)."""
    _fields_ = [("th_mult", C.c_int32), ("num_intervals", C.c_int32 * 10), ("acc_iterations", C.c_int32 * 10),
                ("acc_termination", C.c_int32 * 10), ("gyro_num_blocks", C.c_int32), ("gyro_iterations", C.c_int32),
                ("gyro_termination", C.c_int32), ("norm_th", C.c_double), ("init_acc_bias", C.c_double * 3),
                ("acc_final_cost", C.c_double * 10), ("gyro_init_bias", C.c_double * 3), ("gyro_initial_cost", C.c_double),
                ("gyro_final_cost", C.c_double), ("ms_detector", C.c_double), ("ms_acc", C.c_double), ("ms_gyro", C.c_double)]


# Static multi-pose IMU intrinsics (oicc_static_imu_* in include/oicc_hip.h), a table of its own like ALLAN_SIGNATURES.
STATIC_IMU_SIGNATURES = {
    "intervals": (C.c_int, [C.c_int32, C.c_int64, c_dp, C.c_int32, c_dp, C.c_int32, C.c_int32, c_i32p, c_i32p, c_dp, c_dp]),
    "eval_acc": (C.c_int, [C.c_int32, C.c_int64, c_dp, C.c_double, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp]),
    "eval_gyro": (C.c_int, [C.c_int32, C.c_int64, c_dp, c_dp, C.c_int32, c_i32p, c_dp, C.c_int32, C.c_double, c_dp, c_dp, c_dp,
                            c_dp, c_dp, c_dp, c_dp]),
    "calibrate": (C.c_int, [C.c_int32, C.c_int64, c_dp, c_dp, c_dp, C.POINTER(StaticImuOptions), c_dp, c_dp,
                            C.POINTER(StaticImuReport)]),
}


class BoundStaticImu:
    """Bound oicc_static_imu_* entry points of one library + prefix (``oicc_static_imu_`` for liboicc_hip.so)."""

    def __init__(self, lib, prefix):
        self.lib = lib
        self.prefix = prefix
        for name, (res, args) in STATIC_IMU_SIGNATURES.items():
            fn = getattr(lib, prefix + name)  # AttributeError = missing symbol: fail loudly
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, fn)


class BoardOptions(C.Structure):
    """oicc_board_options (include/oicc_hip.h)."""
    _fields_ = [("radius", C.c_int32), ("threshold_rel", C.c_float), ("max_candidates", C.c_int32), ("subpix_iterations", C.c_int32),
                ("subpix_eps", C.c_double), ("batch", C.c_int32), ("reserved", C.c_int32)]


class BoardReport(C.Structure):
    """oicc_board_report (include/oicc_hip.h)."""
    _fields_ = [("frames_found", C.c_int32), ("frames_overflow", C.c_int32), ("output_width", C.c_int32), ("output_height", C.c_int32),
                ("num_candidates", C.c_int64), ("ms_resize", C.c_double), ("ms_response", C.c_double), ("ms_candidates", C.c_double),
                ("ms_subpix", C.c_double), ("ms_marker", C.c_double), ("ms_assembly_host", C.c_double), ("ms_total", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class BoardStages(C.Structure):
    """oicc_board_stages (include/oicc_hip.h)."""
    _fields_ = [("gray", c_u8p), ("response", C.POINTER(C.c_float)), ("candidates", c_i32p), ("refined", c_dp),
                ("capacity", C.c_int32), ("extended", C.c_int32), ("polarity", c_u8p), ("blurred", C.POINTER(C.c_float)),
                ("grid_shape", c_i32p), ("grid", c_i32p), ("disc", c_dp), ("ring", c_dp)]


# Radon checkerboard extraction (oicc_board_* in include/oicc_hip.h), a table of its own like ALLAN_SIGNATURES.
BOARD_SIGNATURES = {
    "output_size": (C.c_int, [C.c_int32, C.c_int32, C.c_double, c_i32p, c_i32p]),
    "radon_detect": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_u8p, C.c_double, C.c_int32, C.c_int32,
                               C.POINTER(BoardOptions), c_dp, c_i32p, c_i32p, C.POINTER(BoardReport), C.POINTER(BoardStages)]),
}


class BoundBoard:
    """Bound oicc_board_* entry points of one library + prefix (``oicc_board_`` for liboicc_hip.so)."""

    def __init__(self, lib, prefix):
        self.lib = lib
        self.prefix = prefix
        for name, (res, args) in BOARD_SIGNATURES.items():
            fn = getattr(lib, prefix + name)  # AttributeError = missing symbol: fail loudly
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, fn)


# Elimination plan of the block cyclic reduction (oicc_debug_bcr_plan in include/oicc_hip.h; host arithmetic, no device), a table of
# its own like ALLAN_SIGNATURES.
BCR_PLAN_SIGNATURES = {
    "plan": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, c_i64p, C.c_int32, c_i64p]),
    "join_plan": (C.c_int, [C.c_int32] * 8 + [c_i32p, C.c_int32]),   # which levels run as one launch (oicc_debug_bcr_join_plan)
    "level0_plan": (C.c_int, [C.c_int32] * 7),   # whether level 0 runs as one launch behind a plain build launch (oicc_debug_bcr_level0_plan)
    "level0_info": (C.c_int, [C.c_void_p, c_i64p]),   # whether level 0 of the last whole-band solve of a problem did, how many have (oicc_debug_bcr_level0_info)
    "fold_plan": (C.c_int, [C.c_int32] * 5),   # which level's back substitution rides in the last block's launch (oicc_debug_bcr_fold_plan)
    "chain_schedule": (C.c_int, [c_i32p, C.c_int32]),   # the panel chain's events in program order: where each deferred update is issued (oicc_debug_bcr_chain_schedule)
    "fold_info": (C.c_int, [C.c_void_p, c_i64p]),   # whether the last whole-band solve of a problem did, how many have (oicc_debug_bcr_fold_info)
}


class BoundBcrPlan:
    """Bound oicc_debug_bcr_* entry points of one library + prefix (``oicc_debug_bcr_`` for liboicc_hip.so)."""

    def __init__(self, lib, prefix):
        self.lib = lib
        self.prefix = prefix
        for name, (res, args) in BCR_PLAN_SIGNATURES.items():
            fn = getattr(lib, prefix + name)  # AttributeError = missing symbol: fail loudly
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, fn)


# One LM solve with the retraction as the loops run it, and the stand-alone retraction kernel on the same step (oicc_debug_lm_retract,
# outside include/oicc_hip.h: oicc_exchange.hip), a table of its own like BCR_PLAN_SIGNATURES.
LM_RETRACT_SIGNATURES = {
    "retract": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, c_i64p] + [c_dp] * 9),
}


class BoundLmRetract:
    """Bound oicc_debug_lm_retract of one library + prefix (``oicc_debug_lm_`` for liboicc_hip.so)."""

    def __init__(self, lib, prefix):
        self.lib = lib
        self.prefix = prefix
        for name, (res, args) in LM_RETRACT_SIGNATURES.items():
            fn = getattr(lib, prefix + name)  # AttributeError = missing symbol: fail loudly
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, fn)


# Robust start poses (oicc_planar_ransac in include/oicc_hip.h), a table of its own like ALLAN_SIGNATURES: SIGNATURES and
# BA_SIGNATURES are also bound against the CPU checker, which has no counterpart of this entry.
PLANAR_RANSAC_SIGNATURES = {
    "ransac": (C.c_int, [C.c_int32, C.c_int32, c_i64p, c_dp, c_dp, C.c_int32, C.c_double, C.c_int32, C.c_uint64, c_u8p, c_i32p, c_dp,
                         c_dp, c_i32p, c_dp]),
}


class BoundPlanarRansac:
    """Bound oicc_planar_* entry points of one library + prefix (``oicc_planar_`` for liboicc_hip.so)."""

    def __init__(self, lib, prefix):
        self.lib = lib
        self.prefix = prefix
        for name, (res, args) in PLANAR_RANSAC_SIGNATURES.items():
            fn = getattr(lib, prefix + name)  # AttributeError = missing symbol: fail loudly
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, fn)


class CameraRemapReport(C.Structure):
    """oicc_camera_remap_report (include/oicc_hip.h)."""
    _fields_ = [("ms_upload", C.c_double), ("ms_kernel", C.c_double), ("ms_download", C.c_double), ("ms_total", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


c_fp = C.POINTER(C.c_float)

# Camera maps (oicc_camera_* in include/oicc_hip.h), a table of its own like ALLAN_SIGNATURES: SIGNATURES is also bound against
# the CPU checker, which has no counterpart of these entries.
CAMERA_MAPS_SIGNATURES = {
    "unproject": (C.c_int, [C.c_int32, C.c_int32, c_dp, C.c_int32, C.c_int64, c_dp, c_dp, c_u8p, c_dp]),
    "rectify_map": (C.c_int, [C.c_int32, C.c_int32, c_dp, C.c_int32, C.c_int32, C.c_int32, c_dp, C.c_int32, C.c_int32, c_dp, c_fp,
                              c_u8p, c_i64p, c_dp]),
    "discrepancy": (C.c_int, [C.c_int32, C.c_int32, c_dp, C.c_int32, c_dp, C.c_int32, C.c_int32, c_dp, c_dp]),
    "remap": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_u8p, c_fp, C.c_int32, C.c_int32, C.c_int32,
                        C.c_int32, c_u8p, C.POINTER(CameraRemapReport)]),
    "remap_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_u8p, c_fp, C.c_int32, C.c_int32, C.c_int32,
                               c_u8p]),
}


class BoundCameraMaps:
    """Bound oicc_camera_* entry points of one library + prefix (``oicc_camera_`` for liboicc_hip.so)."""

    def __init__(self, lib, prefix):
        self.lib = lib
        self.prefix = prefix
        for name, (res, args) in CAMERA_MAPS_SIGNATURES.items():
            fn = getattr(lib, prefix + name)  # AttributeError = missing symbol: fail loudly
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, fn)


class RsScene(C.Structure):
    """oicc_rs_scene (include/oicc_hip.h): what every rolling-shutter entry takes."""
    _fields_ = [("src_model", C.c_int32), ("src_w", C.c_int32), ("src_h", C.c_int32), ("dst_model", C.c_int32), ("dst_w", C.c_int32),
                ("dst_h", C.c_int32), ("src_intr", c_dp), ("dst_intr", c_dp), ("R9", c_dp), ("num_gyro", C.c_int64), ("gyro_t", c_dp),
                ("gyro_rates", c_dp), ("q_i_c", C.c_double * 4), ("time_offset_imu_to_cam", C.c_double), ("num_frames", C.c_int32),
                ("reserved", C.c_int32), ("frame_t", c_dp), ("line_delay_s", C.c_double), ("reference_row", C.c_double)]


class RsFramesReport(C.Structure):
    """oicc_rs_frames_report (include/oicc_hip.h)."""
    _fields_ = [("ms_table", C.c_double), ("ms_rays", C.c_double), ("ms_upload", C.c_double), ("ms_kernel", C.c_double),
                ("ms_download", C.c_double), ("ms_total", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


c_scene = C.POINTER(RsScene)

# Rolling-shutter rectification (oicc_rs_* in include/oicc_hip.h), a table of its own like CAMERA_MAPS_SIGNATURES: the CPU checker
# has no counterpart of these entries.
ROLLING_SHUTTER_SIGNATURES = {
    "rectify_map": (C.c_int, [C.c_int32, c_scene, c_fp, c_u8p, c_u8p, c_i32p, c_i64p, c_dp]),
    "rectify_frames": (C.c_int, [C.c_int32, c_scene, C.c_int32, c_u8p, C.c_int32, C.c_int32, c_u8p, c_i32p, C.POINTER(RsFramesReport)]),
    "rectify_frames_device": (C.c_int, [C.c_void_p, c_scene, C.c_int32, c_u8p, C.c_int32, c_u8p, c_i32p]),
    "rectify_points": (C.c_int, [C.c_int32, c_scene, C.c_int64, c_i32p, c_dp, c_dp, c_u8p, c_i32p, c_dp]),
    "row_rotations": (C.c_int, [C.c_int32, c_scene, C.c_int64, c_i32p, c_dp, c_dp, c_u8p, c_i32p, c_dp]),
}


class BoundRollingShutter:
    """Bound oicc_rs_* entry points of one library + prefix (``oicc_rs_`` for liboicc_hip.so)."""

    def __init__(self, lib, prefix):
        self.lib = lib
        self.prefix = prefix
        for name, (res, args) in ROLLING_SHUTTER_SIGNATURES.items():
            fn = getattr(lib, prefix + name)  # AttributeError = missing symbol: fail loudly
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, fn)


class StabOptions(C.Structure):
    """oicc_stab_options (include/oicc_hip.h)."""
    _fields_ = [("smoothing_sigma_s", C.c_double), ("max_correction_rad", C.c_double), ("zoom_mode", C.c_int32), ("reserved", C.c_int32),
                ("zoom_window_s", C.c_double), ("max_zoom", C.c_double)]


c_stab_options = C.POINTER(StabOptions)


class StabLevel(C.Structure):
    """oicc_stab_level (include/oicc_hip.h): the accelerometer samples and the options of the horizon lock."""
    _fields_ = [("num_accl", C.c_int64), ("accl_t", c_dp), ("accl", c_dp), ("gravity_sigma_s", C.c_double), ("gravity_const", C.c_double),
                ("accl_gate", C.c_double), ("lock", C.c_double), ("roll_rad", C.c_double)]


c_stab_level = C.POINTER(StabLevel)

# Stabilisation (oicc_stab_* in include/oicc_hip.h), a table of its own like ROLLING_SHUTTER_SIGNATURES.
STABILIZATION_SIGNATURES = {
    "plan": (C.c_int, [C.c_int32, c_scene, c_stab_options, c_dp, c_dp, c_dp, c_dp, c_dp, c_i32p, c_i32p, c_u8p, c_dp]),
    "map": (C.c_int, [C.c_int32, c_scene, c_dp, c_dp, c_fp, c_u8p, c_u8p, c_i32p, c_i64p, c_dp]),
    "frames": (C.c_int, [C.c_int32, c_scene, c_dp, c_dp, C.c_int32, c_u8p, C.c_int32, C.c_int32, c_u8p, c_i32p, C.POINTER(RsFramesReport)]),
    "frames_device": (C.c_int, [C.c_void_p, c_scene, c_dp, c_dp, C.c_int32, c_u8p, C.c_int32, c_u8p, c_i32p]),
    # oicc_stab_plan with a level and, behind its outputs, level_q, up, roll, level_angle, gravity_samples, level_status
    "plan_level": (C.c_int, [C.c_int32, c_scene, c_stab_options, c_stab_level, c_dp, c_dp, c_dp, c_dp, c_dp, c_i32p, c_i32p, c_u8p,
                             c_dp, c_dp, c_dp, c_dp, c_i32p, c_i32p, c_dp]),
}
# oicc_debug_stab_zoom: the applied zoom from the required one (host arithmetic only); oicc_debug_stab_accl_world: step G1 of the
# horizon lock alone
STABILIZATION_DEBUG_SIGNATURES = {
    "zoom": (C.c_int, [C.c_int32, c_dp, c_dp, c_i32p, c_stab_options, c_dp, c_u8p]),
    "accl_world": (C.c_int, [C.c_int32, c_scene, c_stab_level, c_dp, c_i32p]),
}


class BoundStabilization:
    """Bound oicc_stab_* entry points of one library + prefix (``oicc_stab_`` for liboicc_hip.so), and the oicc_debug_stab_* entries as
    ``debug_zoom`` and ``debug_accl_world``."""

    def __init__(self, lib, prefix):
        self.lib = lib
        self.prefix = prefix
        for name, (res, args) in STABILIZATION_SIGNATURES.items():
            fn = getattr(lib, prefix + name)  # AttributeError = missing symbol: fail loudly
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, fn)
        for name, (res, args) in STABILIZATION_DEBUG_SIGNATURES.items():
            fn = getattr(lib, "oicc_debug_stab_" + name)
            fn.restype = res
            fn.argtypes = args
            setattr(self, "debug_" + name, fn)
