/*
 * oicc_hip.h -- C-ABI of the MI355X-native continuous-time IMU-camera spline
 * calibration solver (liboicc_hip.so).
 *
 * This is the drop-in boundary for ONE path of urbste/OpenImuCameraCalibrator:
 * the work done behind  OpenICC::core::SplineTrajectoryEstimator<6>
 *   reference: include/OpenCameraCalibrator/core/spline_trajectory_estimator.h:31-218
 *              include/OpenCameraCalibrator/core/spline_trajectory_estimator.impl.h
 * i.e. problem construction (Add*Measurement), ceres::Solve (residuals,
 * Jacobians, normal equations, Levenberg-Marquardt) and the trajectory getters.
 *
 * Conventions
 *  - plain C, no exceptions cross the ABI; every call returns OICC_OK (0) or a
 *    negative oicc_status; oicc_last_error() gives a message.
 *  - all floating point is IEEE fp64; timestamps are int64 nanoseconds.
 *  - caller-owned HOST buffers are copied on entry; the library owns all
 *    device memory.  One problem = one GPU (one process per GPU).
 *  - quaternions are (x, y, z, w) in memory (Eigen coeffs(), Sophus so3.hpp:185);
 *    SE(3) is [qx qy qz qw tx ty tz] (Sophus se3.hpp:511).
 *  - there is NO CPU fallback: if no HIP device is usable oicc_create fails.
 *  - thread-compatible, not thread-safe (same as the reference estimator).
 */
#ifndef OICC_HIP_H_
#define OICC_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OICC_SPLINE_N 6      /* imu_camera_calibrator.h:27  SPLINE_N            */
#define OICC_BIAS_SPLINE_N 3 /* ceres_calib_split_residuals.h:21 BIAS_SPLINE_N  */

typedef struct oicc_problem oicc_problem;

typedef enum oicc_status {
  OICC_OK = 0,
  OICC_ERR_INVALID_ARG = -1,
  OICC_ERR_NO_DEVICE = -2,
  OICC_ERR_HIP = -3,
  OICC_ERR_STATE = -4,
  OICC_ERR_UNSUPPORTED = -5
} oicc_status;

/* theia::CameraIntrinsicsModelType values (pyTheiaSfM 69c3d37, [EXT]); the
 * dispatch they drive is ceres_calib_split_residuals.h:247-270,366-389. */
typedef enum oicc_camera_model {
  OICC_CAM_PINHOLE = 0,                   /* f, aspect, skew, cx, cy, k1, k2           */
  OICC_CAM_PINHOLE_RADIAL_TANGENTIAL = 1, /* f, aspect, skew, cx, cy, k1,k2,k3, t1,t2  */
  OICC_CAM_FISHEYE = 2,                   /* f, aspect, skew, cx, cy, k1..k4           */
  OICC_CAM_DIVISION_UNDISTORTION = 4,     /* f, aspect, cx, cy, k                      */
  OICC_CAM_DOUBLE_SPHERE = 5,             /* f, aspect, skew, cx, cy, xi, alpha        */
  OICC_CAM_EXTENDED_UNIFIED = 6           /* f, aspect, skew, cx, cy, alpha, beta      */
} oicc_camera_model;

/* SplineOptimFlags, spline_trajectory_estimator.h:17-27 (same bit values). */
typedef enum oicc_optim_flags {
  OICC_POINTS = 1 << 0, /* impl.h:136-153: the board points the views observe become variables (homogeneous 4-vectors under
                         * ceres::HomogeneousVectorParameterization(4): 3 tangent dimensions each, the LAST arrow columns, in
                         * point order).  Never set by the reference CLI; here: complete, not tuned (csrc/kernels_points.hip).
                         * With the inner_iterations option (round 5) every board point is one more block of the sweep: it
                         * depends on every view that sees it and the points of a view are neighbours (one residual block). */
  OICC_T_I_C = 1 << 1,
  OICC_IMU_BIASES = 1 << 2,
  OICC_IMU_INTRINSICS = 1 << 3,
  OICC_GRAVITY_DIR = 1 << 4,
  OICC_CAM_LINE_DELAY = 1 << 5,
  OICC_SPLINE = 1 << 6,
  OICC_ACC_BIAS = 1 << 7,
  OICC_GYR_BIAS = 1 << 8
} oicc_optim_flags;

/* ceres::TerminationType subset reported by the LM loop (A9). */
typedef enum oicc_termination {
  OICC_CONVERGENCE = 0,
  OICC_NO_CONVERGENCE = 1,
  OICC_FAILURE = 2
} oicc_termination;

/* What ceres::Solver::Summary carries that the callers look at, plus timing
 * buckets mirroring Summary::FullReport() (impl.h:273). */
typedef struct oicc_summary {
  int32_t termination;            /* oicc_termination                           */
  int32_t num_iterations;         /* LM iterations run (successful+unsuccessful) */
  int32_t num_successful_steps;
  int32_t num_unsuccessful_steps;
  int32_t num_parameters_tangent; /* P: tangent dimension of the active set     */
  int32_t band_dim;               /* time-banded part of P                      */
  int32_t arrow_dim;              /* dense "arrow" part of P                    */
  int32_t half_bandwidth;         /* of the band part, in scalars               */
  int64_t num_residual_blocks;    /* views + accel samples + gyro samples       */
  int64_t num_residuals;
  double initial_cost;
  double final_cost;
  double final_radius;
  double final_gradient_max_norm;
  double seconds_total;           /* wall clock of oicc_optimize                */
  double seconds_jacobian;        /* residual+Jacobian+normal-equation passes   */
  double seconds_residual;        /* cost-only passes                           */
  double seconds_linear_solver;   /* damped band+arrow Cholesky solves          */
  char message[128];
  /* Ceres' optional minimiser stages (options inner_iterations / bounds_line_search; FullReport lines
   * "Inner iterations" / "Line search steps"): */
  int32_t inner_sweeps;           /* coordinate-descent sweeps run                       */
  int32_t line_search_steps;      /* trial step sizes beyond the first                   */
  int64_t inner_lm_iterations;    /* LM iterations of the per-block solves, all sweeps   */
  double seconds_inner;           /* wall clock of the sweeps (part of seconds_residual) */
  double seconds_setup;           /* host-side set-up inside this call (part of seconds_total): measurement upload, tangent
                                   * layout + buffers, tiles, inner-iteration plan; ~0 when all of them are still current  */
} oicc_summary;

/* Per-iteration trace (optional, for parity tests): cost, cost change,
 * gradient max norm, step norm, trust region radius, rho, success. */
typedef struct oicc_iteration {
  int32_t iteration;
  int32_t step_is_successful;
  double cost;
  double cost_change;
  double gradient_max_norm;
  double step_norm;
  double relative_decrease;
  double trust_region_radius;
} oicc_iteration;

/* ---- lifetime ---------------------------------------------------------- */
/* device_ordinal: HIP device index (LOCAL_RANK); fails with OICC_ERR_NO_DEVICE
 * when no gfx950-class HIP device is usable -- there is no CPU path. */
int oicc_create(oicc_problem** out, int device_ordinal);
void oicc_destroy(oicc_problem* p);
const char* oicc_last_error(const oicc_problem* p);
const char* oicc_version(void);
/* Run all device work on this hipStream_t (e.g. torch's current stream). */
int oicc_set_stream(oicc_problem* p, void* hip_stream);

/* ---- setup: mirrors SplineTrajectoryEstimator setters ------------------ */
/* SetTimes, impl.h:38-51. nr_knots = (end-start)/dt + 6 (integer division). */
int oicc_set_times(oicc_problem* p, int64_t dt_so3_ns, int64_t dt_r3_ns,
                   int64_t start_ns, int64_t end_ns);
int64_t oicc_get_num_so3_knots(const oicc_problem* p); /* impl.h:810 */
int64_t oicc_get_num_r3_knots(const oicc_problem* p);  /* impl.h:815 */
int64_t oicc_get_min_time_ns(const oicc_problem* p);   /* impl.h:825 */
int64_t oicc_get_max_time_ns(const oicc_problem* p);   /* impl.h:820 */

/* Knot values produced by BatchInitSO3R3VisPoses (impl.h:279-339; the slerp/
 * lerp resampling itself is host-side code in the C++ facade). */
int oicc_set_so3_knots(oicc_problem* p, const double* quat_xyzw, int64_t n);
int oicc_set_r3_knots(oicc_problem* p, const double* xyz, int64_t n);
int oicc_get_so3_knots(const oicc_problem* p, double* quat_xyzw, int64_t n);
int oicc_get_r3_knots(const oicc_problem* p, double* xyz, int64_t n);

/* InitBiasSplines, impl.h:54-90 (order-3 R^3 splines, constant init,
 * inv_dt = 1/dt_ns as in the reference, quirk Q3). */
int oicc_init_bias_splines(oicc_problem* p, const double accl_bias[3],
                           const double gyro_bias[3], int64_t dt_accl_ns,
                           int64_t dt_gyro_ns, double max_accl_range,
                           double max_gyro_range);

int oicc_set_T_i_c(oicc_problem* p, const double q_xyzw_t_xyz[7]); /* impl.h:862 */
int oicc_set_gravity(oicc_problem* p, const double g[3]);          /* impl.h:857 */
int oicc_set_camera_line_delay(oicc_problem* p, double seconds);   /* impl.h:873 */
/* SetIMUIntrinsics, impl.h:1237-1248: accl = [misYZ misZY misZX sX sY sZ],
 * gyro = [misYZ misZY misZX misXZ misXY misYX sX sY sZ]. */
int oicc_set_imu_intrinsics(oicc_problem* p, const double accl[6],
                            const double gyro[9]);
/* The per-view theia::Camera intrinsics copied at
 * ceres_calib_split_residuals.h:218-221,333-336 (constant on this path). */
int oicc_set_camera(oicc_problem* p, int32_t camera_model,
                    const double* intrinsics, int32_t num_intrinsics);
/* Board points = tracks of the reconstruction, homogeneous (x,y,z,w), w != 0.  They are the tail of the parameter vector:
 * oicc_optimize with OICC_POINTS refines them in place (as the reference refines image_data_'s tracks), oicc_get_scene_points
 * reads them back. */
int oicc_set_scene_points(oicc_problem* p, const double* xyzw, int64_t n);
int oicc_get_scene_points(const oicc_problem* p, double* xyzw, int64_t n);

/* ---- problem construction: mirrors Add*Measurement --------------------- */
/* AddRSCameraMeasurement (impl.h:539-613) / AddGSCameraMeasurement
 * (impl.h:479-536), batched over views.  t_ns[v] = int64(view timestamp * 1e9).
 * Corners of view v are [corner_offset[v], corner_offset[v+1]).
 * uv = observed pixel (x,y) pairs; cov_diag = per-corner (cov_xx, cov_yy) or
 * NULL for identity (continuous_time_imu_to_camera_calibration.cc:157).
 * accepted[v] (optional) receives the reference's bool return value.
 * GS views carry the reference's HuberLoss(0.0) (quirk Q2) unless
 * oicc_set_option("gs_unit_loss",1) is set. */
int oicc_add_rs_camera_measurements(oicc_problem* p, int64_t n_views,
                                    const int64_t* t_ns,
                                    const int64_t* corner_offset,
                                    const double* uv, const double* cov_diag,
                                    const int32_t* point_index,
                                    uint8_t* accepted);
int oicc_add_gs_camera_measurements(oicc_problem* p, int64_t n_views,
                                    const int64_t* t_ns,
                                    const int64_t* corner_offset,
                                    const double* uv, const double* cov_diag,
                                    const int32_t* point_index,
                                    uint8_t* accepted);
/* AddAccelerometerMeasurement impl.h:342-420 / AddGyroscopeMeasurement
 * impl.h:423-476, batched.  weight = 1/std (imu_camera_calibrator.cc:111,117). */
int oicc_add_accelerometer_measurements(oicc_problem* p, int64_t n,
                                        const int64_t* t_ns,
                                        const double* meas_xyz, double weight,
                                        uint8_t* accepted);
int oicc_add_gyroscope_measurements(oicc_problem* p, int64_t n,
                                    const int64_t* t_ns,
                                    const double* meas_xyz, double weight,
                                    uint8_t* accepted);

/* ---- solve: mirrors Optimize(max_iters, flags), impl.h:255-276 ---------- */
/* Named numeric options.  Ceres 2.1.0 defaults unless the reference overrides
 * them (impl.h:257-266):
 *   function_tolerance 1e-4, parameter_tolerance 1e-7, gradient_tolerance 1e-10,
 *   initial_trust_region_radius 1e4, max_trust_region_radius 1e16,
 *   min_trust_region_radius 1e-32, min_relative_decrease 1e-3,
 *   min_lm_diagonal 1e-6, max_lm_diagonal 1e32, jacobi_scaling 1,
 *   max_num_consecutive_invalid_steps 5,
 *   gs_unit_loss 0 (1: trivial loss on GS views instead of quirk Q2),
 *   rs_time_in_seconds 0 (1: documented fix of quirk Q1),
 *   verbose 0;
 * device-side choices (no effect on the result beyond rounding):
 *   solver_algorithm 0 (0 auto = 4 where it applies, 1 LDS-window band sweep, 2 block cyclic reduction with the Cholesky factor of
 *   every pivot block and its border rows, 3 its parallel form -- every block a pivot at every level, no back substitution levels,
 *   up to 256 blocks of 64 band columns --, 4 block cyclic reduction through the explicit inverses of the 64 x 64 pivot blocks:
 *   the border rows leave the serial factorisation and become matrix products; any geometry none of them takes goes to a
 *   global-memory band Cholesky), solver_partitions 0 (time partitions of algorithm 1; 0 = heuristic),
 *   assembly 0 (0: time tiles - LDS accumulators + slab merge, 2: time tiles adding straight into the packed matrix with
 *   fp64 atomics), tile_windows 0 (knot windows per tile; 0 = automatic),
 *   wide_cells 1 (IMU samples of neighbouring knot windows share one Gram product).
 * Ceres' inner iterations, which the reference switches on (impl.h:266), change the iterates and are therefore an
 * option of the RESULT, not of the device: inner_iterations 0|1 (1 = Solver::Options::use_inner_iterations with the
 * automatic ordering of Ceres 2.1.0, coordinate_descent_minimizer.cc / trust_region_minimizer.cc:352-412),
 * inner_iteration_tolerance 1e-3; bounds_line_search 0|1 (1 = the Armijo search along the projected path that Ceres runs
 * before every candidate evaluation once bias knots with box bounds, impl.h:206-240, are variable).
 * projected_gradient_norm 0|1 (1 = gradient_max_norm of such a bounds-constrained program as Ceres computes it).
 * The applications set all three to 1 as the reference's Ceres behaves; the library default
 * is 0 so that plain LM steps stay available to callers and tests.
 * device_lm 1|0 (round 5): plain LM steps (none of the three above in effect, one rank, tile assembly) take their trust-region
 * decisions ON THE DEVICE -- per iteration the host enqueues solve, retraction, ONE Jacobian pass at the candidate (cost, gradient
 * and normal equations together) and a one-thread decision kernel (accept / reject, radius, tolerances: LmCtl, csrc/oicc_device.h)
 * and polls a pinned word one iteration behind; 0 = the host-driven loop (a separate cost pass, one read-back per iteration).
 * owner_computes_sweeps 1|0, distributed_solve 1|0: see oicc_set_shard.
 * Inner iterations at scale (round 5; both are read when the plan of the sweeps is built): inner_wave_blocks 0|1|2 (0: sets of knot
 * blocks with at least 4 x compute-unit-count blocks run one wave per block, 1: every eligible set, 2: never),
 * inner_shared_launch_slots 65536 (a block every view / sample depends on with at least this many item slots is minimised by a
 * sequence of launches over the whole device instead of resident workgroups; 0: never).  Neither changes what is computed.
 * Measurements may be added in any order (the reference walks an unordered map of views): the library sorts them by time before
 * anything is derived from them; per-block dumps (oicc_evaluate_blocks) stay in the caller's order. */
int oicc_set_option(oicc_problem* p, const char* name, double value);
int oicc_optimize(oicc_problem* p, int32_t max_iters, int32_t flags,
                  oicc_summary* summary);
/* Trace of the last oicc_optimize call; returns number of entries written. */
int oicc_get_iterations(const oicc_problem* p, oicc_iteration* out,
                        int32_t capacity);
/* Debug read-out of the inner iterations (option "debug_inner_set_costs" = 1; Ceres' CoordinateDescentMinimizer has no counterpart,
 * it is how a test names the independent set at which two implementations part): for every sweep of the last oicc_optimize call
 * the pair [-1, total cost before the sweep] followed by one pair [number of parameter blocks in the set, total cost behind the
 * set] per independent set, in processing order.  Returns the number of doubles available (written: min(capacity, that)). */
int oicc_get_inner_set_costs(const oicc_problem* p, double* out, int32_t capacity);

/* ---- multi-GPU: residual blocks are sharded by the caller (each
 * rank adds only its own views / IMU samples, all ranks hold all parameters).
 * After every local normal-equation / cost pass the library calls
 *   reduce(user, device_ptr, count_doubles, hip_stream)
 * which must SUM the fp64 buffer across ranks in place, ordered on the given
 * stream (RCCL all-reduce; torch.distributed does this in bench.py).
 * NULL = single GPU. */
typedef int (*oicc_allreduce_fn)(void* user, void* device_ptr, int64_t count,
                                 void* hip_stream);
int oicc_set_allreduce(oicc_problem* p, oicc_allreduce_fn fn, void* user);
/* Native RCCL reduction (preferred): the library binds the RCCL of the process at run time (dlsym / dlopen of
 * librccl.so.1, no link-time dependency), builds a communicator from the 128-byte ncclUniqueId that rank 0 obtained
 * with oicc_rccl_get_unique_id and the caller distributed (MPI / torch.distributed broadcast / a file), and from then
 * on sums the packed normal-equation buffer IN PLACE with ncclAllReduce(ncclDouble, ncclSum) on the library's own
 * stream: no staging copies, no host involvement.  nranks = 1 is allowed (single-GPU test of the path).
 * Replaces any hook installed with oicc_set_allreduce; oicc_destroy releases the communicator. */
int oicc_rccl_get_unique_id(uint8_t id[128]);
int oicc_rccl_init(oicc_problem* p, int32_t nranks, int32_t rank, const uint8_t id[128]);
/* Inner iterations (the reference's use_inner_iterations = true, impl.h:266) on a time-sharded problem: the coordinate
 * descent sweep minimises every parameter block over ALL residual blocks that depend on it, so a rank that holds only its
 * shard cannot run it.  `whole` is a second problem on the same device with the same spline, calibration and options that
 * holds EVERY rank's measurements (a few MB even at BASELINE config 5); the sweeps of oicc_optimize(p) then run on p's
 * candidate over whole's measurements, identically (replicated) on every rank, with no collective; with the native RCCL
 * path rank 0's swept candidate is broadcast afterwards so that all ranks continue from identical bits.  The Jacobian and
 * cost passes of p stay sharded.  NULL removes the source.  `whole` must outlive p's solves. */
int oicc_set_inner_iteration_source(oicc_problem* p, oicc_problem* whole);
/* Measurement: `repeats` reductions of the packed normal-equation buffer through the installed hook / the native RCCL path,
 * timed with HIP events on the library's stream (every rank must call it with the same arguments: it is a collective).
 * ms_per_call: average; bytes: size of the reduced buffer.  OICC_ERR_STATE without a reduction path. */
int oicc_time_allreduce(oicc_problem* p, int32_t flags, int32_t repeats, double* ms_per_call, int64_t* bytes);
/* ---- multi-GPU, owner-computes assembly (SURVEY 8e "v2", round 4).  With time shards every band row (knot) is touched by one rank
 * or by two neighbours.  Instead of summing the whole packed buffer over all ranks (52 MB at BASELINE config 5), the band rows are
 * cut into one contiguous OWNED range per rank;  after its local pass a rank (1) sends the partial rows it holds of ranges it does not
 * own to their owners and adds what it receives (~50 rows per neighbour), (2) the owners' ranges are gathered by every rank (each
 * piece broadcast from its owner: the solve stays replicated), (3) only the arrow corner, the arrow gradient and the cost are
 * all-reduced (oicc_set_allreduce / the native RCCL communicator).  Half the bytes of the all-reduce, no reduction arithmetic on them.
 * The spline estimator of the reference has no counterpart (one process, Ceres threads: impl.h:260); the local support that makes
 * the band rows rank-local is impl.h:384-397,455-460,505-516.
 *   oicc_set_shard        this problem holds shard `rank` of `nranks` time-contiguous shards (ascending in time with the rank)
 *   oicc_declare_remote_measurements_from   as oicc_declare_remote_measurements, with the rank that holds them: every rank then
 *                         derives the same owned ranges and send / receive row lists
 *   oicc_set_exchange     transport twin of the native path (ncclSend / ncclRecv / ncclBroadcast of oicc_rccl_init) for callers with
 *                         their own transport (the tests: gloo through host memory).  op OICC_XCHG_SENDRECV: send `send_count` doubles
 *                         to rank `peer` and receive `recv_count` doubles from it (either may be 0); op OICC_XCHG_BROADCAST: `send`
 *                         (= `recv`) holds `send_count` doubles on rank `peer`, which every rank receives in place.  Ordered on the
 *                         given stream, like the all-reduce hook.
 * Without oicc_set_shard the all-reduce of the whole buffer ("v1") is what runs.
 * Round 5: (a) an owner's range travels as ONE contiguous message of packed rows [band | arrow | gradient] -- one in-place
 * ncclAllGather of equal slots (or one broadcast per owner: hook transport) instead of a + 2 strided pieces per owner --, the halo rows
 * of all peers in ONE send / receive group; (b) whether the exchange is used is AGREED ON by all ranks once per layout (a sum of
 * [ready, 1, hash, hash^2] through the installed reduction; any rank that is not ready or derived other cuts sends every rank to the
 * all-reduce of the whole buffer): oicc_set_shard with nranks > 1 is therefore a collective statement -- every rank must make it;
 * (c) with an inner-iteration source (oicc_set_inner_iteration_source) the SWEEPS are owner-computes too (option
 * owner_computes_sweeps, default 1): a rank minimises only the knot blocks whose band rows it owns (plus the few blocks every view /
 * sample depends on, replicated; rank 0's result counts) and after every independent set the owners broadcast the knot ranges the set
 * changed -- the sweep's work divides by the number of ranks instead of being replicated.
 * Round 6: (d) the LINEAR SOLVE is distributed too (option distributed_solve, default 1; the reference's solve is one
 * SPARSE_NORMAL_CHOLESKY on one host, impl.h:257-272).  The cuts between the owned ranges lie on multiples of 64 rows, the blocks of the
 * cyclic reduction: step (2) above shrinks to two doubles per row (diagonal and gradient: what every rank needs of ALL rows), every
 * rank reduces the blocks of ITS range down to the range's first block, ONE all-gather moves the ranks' separator blocks (0.11 MB each),
 * every rank solves the N-block top system and back-substitutes its own range, ONE all-gather moves the step -- the same bits on
 * every rank, so the candidate is not broadcast any more (only the step's scalars are).  The band rows never leave their owner.  The choice is part of what the ranks agree on in (b) (options distributed_solve, solver_algorithm and bcr_max_border
 * are in the hash; ranks that differ in one fall back together to the all-reduce of the whole buffer); where the geometry is not the cyclic reduction's (half
 * bandwidth > 64, more than 63 arrow columns) or a rank would own no block, all ranks gather the band and solve the whole system as
 * before.  Both gathers go through the same transport as (a): ncclAllGather, or OICC_XCHG_BROADCAST per owner on the hook. */
enum { OICC_XCHG_SENDRECV = 0, OICC_XCHG_BROADCAST = 1 };
typedef int (*oicc_exchange_fn)(void* user, int32_t op, void* send, int64_t send_count, void* recv, int64_t recv_count,
                                int32_t peer, void* hip_stream);
int oicc_set_shard(oicc_problem* p, int32_t nranks, int32_t rank);
int oicc_set_exchange(oicc_problem* p, oicc_exchange_fn fn, void* user);
int oicc_declare_remote_measurements_from(oicc_problem* p, int32_t owner_rank, int32_t kind, int64_t n, const int64_t* t_ns);
/* Measurement: `repeats` owner-computes exchanges of the packed normal equations (halo rows + gather + corner all-reduce), timed
 * with HIP events on the library's stream; bytes_moved: what this rank sent + received per exchange.  A collective -- except with
 * repeats < 0, which only answers (OICC_OK / OICC_ERR_STATE) whether the exchange is set up on this rank. */
int oicc_time_exchange(oicc_problem* p, int32_t flags, int32_t repeats, double* ms_per_call, int64_t* bytes_moved);
/* Tell this rank about measurements held by OTHER ranks (timestamps only), so
 * that every rank derives the same tangent layout (which knots are in the
 * problem, bandwidth, which parameter blocks exist).
 * kind: 0 = RS camera view, 1 = accelerometer, 2 = gyroscope, 3 = GS camera view. */
int oicc_declare_remote_measurements(oicc_problem* p, int32_t kind, int64_t n,
                                     const int64_t* t_ns);

/* ---- evaluation hooks (parity tests, bench) ----------------------------- */
/* Tangent layout of the active set for `flags`: band variables ordered by
 * (knot time in ns, kind: SO3 before R3), then the arrow in the fixed order
 * T_i_c(6: upsilon,omega) | gravity(3) | line_delay(1) | accl bias knots(3 each)
 * | gyro bias knots(3 each) | accl intrinsics(6) | gyro intrinsics(9).
 * Outputs (each optional) receive the tangent offset or -1 if inactive. */
int oicc_get_tangent_layout(oicc_problem* p, int32_t flags, int32_t* num_tangent,
                            int32_t* so3_offsets, int32_t* r3_offsets,
                            int32_t* accl_bias_offsets,
                            int32_t* gyro_bias_offsets,
                            int32_t other_offsets[5] /* T_i_c,g,ld,acc_intr,gyr_intr */);
/* Tangent offset of every board point for `flags`: -1 unless OICC_POINTS is set and a corner of some view refers to the
 * point (impl.h:136-153: tracks_in_problem_); the point columns follow the arrow blocks listed above, 3 per point, in
 * point order.  offsets: one entry per point of oicc_set_scene_points. */
int oicc_get_scene_point_offsets(oicc_problem* p, int32_t flags, int32_t* offsets);
/* One residual + Jacobian + normal-equation pass at the current parameters.
 * cost = 0.5*sum r^2.  H_dense (P*P row-major, symmetric) and g (P) optional.
 * Time-sharded problems (oicc_set_shard with a reduction installed): a collective that returns the WHOLE problem's cost, J^T J and
 * gradient on every rank -- the band is gathered for this call even where the ranks agreed on the distributed solve, which never
 * gathers it.  The same holds for oicc_evaluate_cost and oicc_evaluate_entries. */
int oicc_evaluate(oicc_problem* p, int32_t flags, double* cost, double* H_dense,
                  double* g, int32_t P_capacity);
/* Cost-only pass (what LM runs for a candidate point). */
int oicc_evaluate_cost(oicc_problem* p, int32_t flags, double* cost);
/* One pass as oicc_evaluate, then n entries H(rows[k], cols[k]) of J^T J in the tangent ordering above (0 outside the band +
 * arrow pattern) -- for problems whose dense P x P matrix does not fit (BASELINE config 5: P ~ 90 k), where parity tests compare
 * sampled entries.  The reference has no counterpart (ceres::Problem::Evaluate returns a CRS Jacobian, not J^T J). */
int oicc_evaluate_entries(oicc_problem* p, int32_t flags, int64_t n, const int32_t* rows, const int32_t* cols, double* values);
/* Per-block residuals and tangent Jacobians for parity tests.
 * kind: 0 = camera views, 1 = accelerometer, 2 = gyroscope.
 * Camera: residuals [2*total_corners]; jacobian rows hold the block-local
 * columns [6 SO3 knots x3 | 6 R3 knots x3 | T_i_c 6 | line delay 1] = 43.
 * Accel: residuals [3*n]; columns [18 | 18 | g 3 | bias knots 9 | intr 6] = 54.
 * Gyro : residuals [3*n]; columns [18 | bias knots 9 | intr 9] = 36.
 * Columns of inactive parameters are zero. jacobians may be NULL. */
int oicc_evaluate_blocks(oicc_problem* p, int32_t flags, int32_t kind,
                         double* residuals, double* jacobians);
/* Time `repeats` back-to-back Jacobian+assembly passes with HIP events on the
 * library's stream; returns average milliseconds per pass and, optionally, the
 * per-kernel averages [views, accel, gyro]. */
int oicc_time_jacobian_pass(oicc_problem* p, int32_t flags, int32_t repeats,
                            double* ms_per_pass, double kernel_ms[3]);
/* Run the device work and host synchronisation of `steps` successful LM
 * iterations at the current point without accepting the steps (bench.py's
 * "step": Jacobian+assembly, [all-reduce], damped solve, retraction, cost). */
int oicc_run_lm_iterations(oicc_problem* p, int32_t flags, int32_t steps);
/* Same for the damped band+arrow solve of the last assembled system. */
int oicc_time_linear_solve(oicc_problem* p, int32_t flags, int32_t repeats,
                           double* ms_per_solve);
/* Verification of the linear solver at any size: one damped solve (SPARSE_NORMAL_CHOLESKY step of ceres::Solve, called at
 * spline_trajectory_estimator.impl.h:272) at the current point with trust-region radius `radius`, then the residual of the step against
 * the packed normal equations themselves: out = {||M d - rhs|| / ||rhs||, ||rhs||, factorisation failure flag},
 * M = S JtJ S + clamp(diag)/radius, rhs = -S Jtr (S: Jacobi scaling). */
int oicc_solve_residual(oicc_problem* p, int32_t flags, double radius, double out[3]);

/* ---- covariance estimation -------------------------------------------------
 * What ceres::Covariance returns with the local parameterisations (the reference asks it for the board points only,
 * src/core/pose_estimator.cc:193-223): (J^T J)^-1 at the current parameters in the tangent space of
 * oicc_get_tangent_layout (T_i_c: upsilon | omega of the right perturbation).  The residuals are already weighted.
 * Computed on the device as a SELECTED inverse of the band + arrow normal equations of one Jacobian pass: the whole
 * a x a arrow block, the 3 x 3 diagonal block of every knot and the 3 x a block of every knot with the arrow -- never
 * a dense P x P inverse.  The matrix is scaled to unit diagonal first (S H S, s_i = H_ii^-1/2, no damping) and the
 * result unscaled, cov_ij = s_i s_j Zs_ij.
 *   status           OICC_COV_OK; OICC_COV_RANK_DEFICIENT: a pivot of the factorisation was not positive, or
 *                    rcond < option covariance_min_rcond (1e-12): no covariance is handed out;
 *                    OICC_COV_ZERO_COLUMN: a diagonal entry of J^T J is not finite and positive (oicc_last_error
 *                    names the column)
 *   rcond            1 / max_i Zs_ii over all P diagonal entries: lambda_min(S H S) <= rcond <= P lambda_min(S H S)
 *   variance_factor  2 cost / (num_residuals - P), num_residuals = 2 corners + 3 accelerometer + 3 gyroscope samples
 *                    of the accepted measurements; returned separately, nothing is multiplied by it
 * oicc_estimate_covariance returns OICC_OK for each of the three statuses (info->status tells them apart) and
 * OICC_ERR_UNSUPPORTED, with the reason in oicc_last_error, for OICC_POINTS in flags (the board gauge makes J^T J
 * singular), time-sharded problems (oicc_set_shard) and problems with a reduction across ranks installed (oicc_set_allreduce,
 * oicc_rccl_init), a half bandwidth above 120 and more than 63 arrow columns.
 * The getters return OICC_ERR_STATE unless the last estimate has status OICC_COV_OK and still belongs to the current
 * parameters: any setter, Add*Measurement, oicc_set_option and oicc_optimize invalidate it. */
typedef enum oicc_covariance_status { OICC_COV_OK = 0, OICC_COV_RANK_DEFICIENT = 1, OICC_COV_ZERO_COLUMN = 2 } oicc_covariance_status;
typedef struct oicc_covariance_info {
  int32_t status, P, Pb, a, hb;
  int64_t num_residuals;
  double cost, variance_factor, rcond;
} oicc_covariance_info;
int oicc_estimate_covariance(oicc_problem* p, int32_t flags, oicc_covariance_info* info);
/* cov [a][a] row major, in the arrow order of oicc_get_tangent_layout; a_capacity >= a */
int oicc_get_covariance_arrow(const oicc_problem* p, double* cov, int32_t a_capacity);
/* the 3 x 3 diagonal blocks of the knots, 9 doubles per knot (row major), NaN for knots outside the active set;
 * either pointer may be NULL; n_so3 / n_r3 = the knot counts */
int oicc_get_covariance_knots(const oicc_problem* p, double* so3_blocks, int64_t n_so3, double* r3_blocks, int64_t n_r3);
/* cross [3][a]: the covariance of one knot (kind 0 = SO(3), 1 = R^3) with the arrow; NaN outside the active set */
int oicc_get_covariance_knot_arrow(const oicc_problem* p, int32_t kind, int64_t knot, double* cross);
/* Device time of the last estimate's kernels in ms: build, forward factor, arrow corner, backward sweep (with the
 * knot / cross block kernel behind it). */
int oicc_get_covariance_timing(const oicc_problem* p, double ms[4]);

/* ---- residual report and corner gating --------------------------------------
 * Which corners and views fit badly, and whether the IMU residuals are at the sensors' noise level: two residual-only
 * kernels at the current parameters (kernels_report.hip).  Everything is UNWEIGHTED:
 *   corner error   e = pi(p_c) - z [px], through the functor the solve uses for that view (rolling-shutter views with
 *                  quirk Q1 or option rs_time_in_seconds, global-shutter views without the line-delay shift), without
 *                  1/sigma and without the quirk Q2 zeroing of global-shutter views
 *   corner status  OICC_CORNER_USED; OICC_CORNER_PROJECTION_FAILED: the functor's (1e10, 1e10) case, kept as e, in no
 *                  statistic; OICC_CORNER_GATED: weight 0 by oicc_gate_corners, its true error is still reported
 *   view figures   n_used (status used), rms_px = sqrt(sum |e|^2 / n_used), max_px = max |e| over the used corners
 *                  (0 for a view without a used corner)
 *   accelerometer  R^T (a_w + g) - MS_a (a_m - b) [m/s^2];  gyroscope  omega - MS_g (omega_m - b) [rad/s]
 * oicc_residual_info: counts by status; mean, rms, median and max of |e| over the used corners; sigma_px = median /
 * 1.17741, the Rayleigh scale of |e| for a per-axis standard deviation sigma (robust against gross outliers); per-axis
 * rms of both IMU families, unweighted and multiplied by the samples' weights (1 at the noise level the weights were
 * derived from); ms_device: device time of the report's kernels.
 * Every getter returns its data in the CALLER's order: corners, views (the accepted ones) and samples as they were
 * added.  The getters return OICC_ERR_STATE unless a report exists for the current parameters and measurements: any
 * setter, Add*Measurement, oicc_set_option, oicc_optimize and an oicc_gate_corners that changes a weight invalidate it.
 *
 * oicc_gate_corners, from the last report: a corner of status used or gated with |e| > threshold_px gets weight
 * exactly 0, every other corner the weight it was added with (the original 1/sigma is kept, so gating never
 * accumulates); threshold_px <= 0 lifts every gate and needs no report.  A view whose corners are all gated stays in
 * the problem as a block of zero rows.  oicc_get_mean_reprojection_error skips gated corners (their weighted residual
 * is zero).  The measurements count as changed: they travel again, tiles and the inner-iteration plan are rebuilt.
 * The usual sequence is optimize, report, gate at 5 sigma_px, optimize again (the facades' OptimizeGated).
 * oicc_residual_report and oicc_gate_corners return OICC_ERR_UNSUPPORTED on time-sharded problems (oicc_set_shard) and
 * with a reduction across ranks installed: the median would be a collective. */
enum { OICC_CORNER_USED = 0, OICC_CORNER_PROJECTION_FAILED = 1, OICC_CORNER_GATED = 2 };
typedef struct oicc_residual_info {
  int64_t num_corners, num_used, num_failed, num_gated, num_views, num_accl, num_gyro;
  double mean_px, rms_px, median_px, sigma_px, max_px;
  double accl_rms[3], accl_rms_weighted[3], gyro_rms[3], gyro_rms_weighted[3];
  double ms_device;
} oicc_residual_info;
int oicc_residual_report(oicc_problem* p, oicc_residual_info* info);
/* e_uv [n][2], status [n]; n = the number of corners of the accepted views; either pointer may be NULL */
int oicc_get_corner_errors(oicc_problem* p, double* e_uv, uint8_t* status, int64_t n);
/* [nv] each, nv = the number of accepted views; any pointer may be NULL */
int oicc_get_view_errors(oicc_problem* p, double* rms_px, double* max_px, int32_t* n_used, int64_t nv);
/* kind 1 accelerometer, 2 gyroscope (as oicc_evaluate_blocks); r_xyz [n][3], n = the number of accepted samples */
int oicc_get_imu_residuals(oicc_problem* p, int32_t kind, double* r_xyz, int64_t n);
int oicc_gate_corners(oicc_problem* p, double threshold_px, int64_t* n_gated);
/* gated [n]: 1 where the corner is gated now; n as in oicc_get_corner_errors.  Needs no report. */
int oicc_get_corner_gate(oicc_problem* p, uint8_t* gated, int64_t n);

/* ---- read-back: mirrors the getters ------------------------------------- */
int oicc_get_T_i_c(const oicc_problem* p, double q_xyzw_t_xyz[7]);  /* impl.h:1133 */
int oicc_get_gravity(const oicc_problem* p, double g[3]);           /* impl.h:1128 */
int oicc_get_rs_line_delay(const oicc_problem* p, double* seconds); /* impl.h:1138 */
int oicc_get_imu_intrinsics(const oicc_problem* p, double accl[6], double gyro[9]);
int oicc_get_bias_knots(const oicc_problem* p, double* accl_xyz, int64_t n_accl,
                        double* gyro_xyz, int64_t n_gyro);
int64_t oicc_get_num_accl_bias_knots(const oicc_problem* p);
int64_t oicc_get_num_gyro_bias_knots(const oicc_problem* p);
/* GetMeanReprojectionError, impl.h:994-1072 (always the RS functor; skips
 * corners with a zero residual component; 0.0 on an empty/out-of-range view). */
int oicc_get_mean_reprojection_error(oicc_problem* p, double* mean_px,
                                     int64_t* num_points);
/* Batched trajectory getters (impl.h:879-991, 1181-1234). valid[i]=0 where the
 * reference getter returns false (outputs untouched / zero bias).
 *  pose: [qx qy qz qw tx ty tz] = GetPose; gyro = GetAngularVelocity;
 *  accel = GetAcceleration (R^T (a_w + g)); biases = GetGyroBias / GetAcclBias.
 * Any output may be NULL. */
int oicc_get_trajectory(oicc_problem* p, int64_t n, const int64_t* t_ns,
                        double* pose7, double* gyro3, double* accel3,
                        double* gyro_bias3, double* accl_bias3, uint8_t* valid);


/* ---- Spline error weighting pre-stage ---------------------
 * knot_spacing_and_variance(signal, times, quality, min_dt, max_dt), python/sew.py:199-235,
 * as called by python/get_sew_for_dataset.py:38-39 for the accelerometer (q_r3, R3 spline) and
 * the gyroscope (q_so3, SO3 spline).  It fixes the knot spacings and the IMU residual weights
 * 1/sqrt(variance) the spline solve consumes.
 *   signal   [dims][n] row major (dims = 3 axes), times [n] in seconds (uniform sampling assumed,
 *            sample rate = 1 / mean(diff(times)), sew.py:144)
 *   spectrum Xhat_k = sqrt(1/dims) * || FFT(signal)[:, k] ||, DC removed (sew.py:170-179)
 *   quality  fraction of signal energy the cubic-B-spline interpolation response
 *            H(f, dt) = 3 sinc^4(f dt) / (2 + cos(2 pi f dt))  (sew.py:35-57, normalised :75-76)
 *            must keep; the largest such dt in [min_dt, max_dt] is found by the end-point test,
 *            halving back-off and Brent root finding of sew.py:83-137 (brentq defaults of SciPy:
 *            xtol 2e-12, rtol 4 eps, 100 iterations)
 *   variance signal_energy((1 - H) Xhat) / n at that dt (sew.py:192-195)
 * min_dt <= 0 / max_dt <= 0 select the reference defaults 1/rate and (n/4)/rate (sew.py:153-157).
 * FFT and the spectral reductions run on the device (hipFFT D2Z + one reduction launch per trial dt).
 * Returns OICC_ERR_INVALID_ARG for n < 8 or a non-increasing time base.
 * Thread safety: calls are serialised inside the library (the device buffers and the hipFFT plan of the last
 * (device, dims, n) are cached for the next call and live until the process ends). */
int oicc_sew_knot_spacing_and_variance(int32_t device_ordinal, int32_t dims, int64_t n, const double* signal,
                                       const double* times, double quality, double min_dt, double max_dt,
                                       double* dt, double* variance, int32_t* num_evaluations);


/* ---- Gyroscope-to-camera rotation / time-offset initialisation ------------
 * ImuToCameraRotationEstimator::EstimateCameraImuRotation + SolveClosedForm,
 * src/core/imu_to_camera_rotation_estimator.cc:39-274, as driven by
 * applications/estimate_imu_to_camera_rotation.cc:150-214; it produces the file
 * continuous_time_imu_to_camera_calibration reads with --gyro_to_cam_initial_calibration.
 *   t_vis_s / q_vis_xyzw  camera orientation samples, strictly increasing times; the quaternion of
 *                         theia::Camera::GetOrientationAsRotationMatrix() (world -> camera), (x,y,z,w)
 *   t_imu_s / gyro_xyz    gyroscope samples (rad/s, a known bias already removed), strictly increasing times
 *   dt_imu                mean IMU sample spacing [s] (estimate_imu_to_camera_rotation.cc:118-124)
 *   estimate_gyro_bias    EnableGyroBiasEstimation(): bias = mean_vis - R mean_imu of the best probe
 * Outputs: R_imu_to_camera as a quaternion (x,y,z,w; Eigen::Quaterniond(R)), the time offset in [-1, 1] s found by the
 * golden-section search (tolerance 1e-4), the gyro bias (untouched unless estimated), the Huber-type alignment error
 * of the last accepted probe and the number of search iterations.  The preparation (common window, slerp to the IMU
 * times, quaternion-difference rates, 15-tap moving averages) runs once on the host as in the reference; every probe of
 * the search is two reduction launches over the IMU samples on the device.  OICC_ERR_INVALID_ARG for unsorted times or
 * fewer than 16 IMU samples in the common window. */
int oicc_estimate_imu_to_camera_rotation(int32_t device_ordinal, int64_t n_vis, const double* t_vis_s, const double* q_vis_xyzw,
                                         int64_t n_imu, const double* t_imu_s, const double* gyro_xyz, double dt_imu,
                                         int32_t estimate_gyro_bias, double q_imu_to_cam_xyzw[4], double* time_offset_imu_to_cam,
                                         double gyro_bias[3], double* alignment_error, int32_t* iterations);

/* ---- IMU noise characterisation: Allan variance and noise-model fit ------------------------------------------
 * applications/fit_allan_variance.cc + core::AllanVarianceFitter (src/core/allan_variance_fitter.cc:12-128): a still
 * IMU's six channels, the overlapping Allan variance of each at ~num_clusters log-spaced cluster sizes, and the fit of
 * sigma2(tau) = Q^2/tau^2 + N^2/tau + B^2 + K^2 tau + R^2 tau^2 that gives white noise and bias instability. */
enum { OICC_ALLAN_GYRO = 0, OICC_ALLAN_ACC = 1, OICC_ALLAN_REPORT_SIZE = 6 };
/* AllanGyr::initStrides + getLogSpace (src/allanvariance/allan_gyr.cc:141-196), operation for operation: maxStride = the
 * largest power of two <= n/2 (shift loop), getLogSpace(0, float(log10(maxStride))), a float exponent
 * 1.0f/(num_clusters-1), cumulative double products, ceil, consecutive duplicates dropped.  factors has room for
 * num_clusters entries.  Host only: needs no device.  OICC_ERR_INVALID_ARG for n < 8 or num_clusters < 2. */
int oicc_allan_factors(int64_t n, int32_t num_clusters, int32_t* factors, int32_t* num_factors);
/* AllanGyr / AllanAcc ::calc + getVariance + getTimes (allan_gyr.cc:39-125, allan_acc.cc), all channels in one call:
 *   samples [channels][n] raw values, sample i of every channel at t_s[i] (strictly increasing, seconds);
 *   scale[c]  per-sample unit factor applied before the sum: 57.3*3600 for pushRadPerSec (:20-23), 1 for pushMPerSec2
 * Host, sequential as the reference: avgDt = sum(t[i]-t[i-1])/(n-1) (:205-214), *freq = 1/avgDt, *period = avgDt,
 * mean[c] = sum(samples*scale)/n (getAvgValue), factors / *num_factors as oicc_allan_factors, taus[f] = period*factors[f].
 * Device: scale and prefix scan to theta[k] = sum_{i<=k} w[i] / freq (:130-139; the channel mean is subtracted first,
 * which the second difference cancels), then for every channel and factor m
 *   sigma2[c][f] = sum_{k<n-2m} (theta[k+2m] - 2 theta[k+m] + theta[k])^2 / (2 (period m)^2 (n-2m))   (:104-125)
 * summed in fp64 without atomics (bitwise-repeatable).  Deviation: where n - 2m <= 0 (the last factor can be maxStride+1)
 * sigma2 is NaN; the reference gives 0/0 or -0.0 there.  sigma2 has room for channels*num_clusters entries, row stride
 * *num_factors.  device_ms (may be NULL): device time of the scan, variance and reduction launches.
 * OICC_ERR_INVALID_ARG for n < 8 or times that do not increase; OICC_ERR_NO_DEVICE without a usable HIP device. */
int oicc_allan_variance(int32_t device_ordinal, int32_t channels, int64_t n, const double* samples, const double* t_s,
                        const double* scale, int32_t num_clusters, int32_t* num_factors, int32_t* factors, double* taus,
                        double* sigma2, double* freq, double* period, double* mean, double* device_ms);
/* FitAllanGyr (kind OICC_ALLAN_GYRO, src/allanvariance/fitallan_gyr.cc:7-60) / FitAllanAcc (OICC_ALLAN_ACC,
 * fitallan_acc.cc:7-57), one axis.  Points with sigma2 not finite and positive are left out (see oicc_allan_variance);
 * the accelerometer then applies checkData (fitallan_acc.cc:120-139: for tau < 1 a point above the running maximum,
 * which starts at 0, is dropped and raises the maximum).  Start value |C|, C = (F^T F)^-1 F^T sqrt(sigma2) with
 * F = sqrt(tau)^(-2..2) (initValue :62-101; init_C, may be NULL, gets the signed C the reference prints).  Solve: the
 * residual log10(model) - log10(sigma2) per point (fitallan_*.h), Ceres 2.1 trust region with trust_region_strategy_type
 * DOGLEG and default Solver::Options, restated.  Outputs: params_QNBKR as the solver leaves them (signs included),
 * report (unit = 57.3*3600 for the gyroscope, 1 for the accelerometer; findMinNum / findMinIndex start at 1000.0):
 *   [0] min_i sqrt(model(tau_i)) / unit        getBiasInstability (:104-106)
 *   [1] tau_i of that minimum                  taus[findMinIndex(...)] (:53-54)
 *   [2] sqrt(freq) sqrt(model(1)) / unit       getWhiteNoise (:108-110)
 *   [3] |B| / 0.6642824703 / unit              getB() / (57.3*3600) (:51-52)
 *   [4] sqrt(freq) |N| / 57.3                  sqrt(freq) * getN() * 60 / 57.3 (:56-57)
 *   [5] final cost 0.5 sum r_i^2
 * num_used: points in the fit; iterations: trust-region iterations.  Host only: needs no device.
 * OICC_ERR_INVALID_ARG for a bad kind or fewer than 5 usable points. */
int oicc_allan_fit(int32_t kind, int64_t num, const double* taus, const double* sigma2, double freq, double params_QNBKR[5],
                   double init_C[5], double report[6], int32_t* num_used, int32_t* iterations);

/* ---- View bundle adjustment: camera intrinsics calibration and per-view pose refinement ------
 * What the reference does through TheiaSfM's bundle adjuster [EXT] in
 *   CameraCalibrator::RunCalibration      src/core/camera_calibrator.cc:131-219  (theia::BundleAdjustViews, three stages)
 *   PoseEstimator::EstimatePosePinhole    src/core/pose_estimator.cc:62-90       (theia::BundleAdjustView)
 *   PoseEstimator::OptimizeAllPoses       src/core/pose_estimator.cc:226-236     (theia::BundleAdjustView for every view)
 *   utils::GetReprojErrorOfView           src/utils/utils.cc:163-177
 * One residual block per observation: r = CameraToPixelCoordinates(intr, R(w)(X.xyz - X.w C)) - feature, camera
 * extrinsics [position C | angle axis w] updated by plain addition (no local parameterisation, as Theia), one shared
 * intrinsics block with constant entries held by a subset mask, scene points constant, ceres::HuberLoss(huber_width)
 * per block.  Tangent order of oicc_ba_evaluate: for every view [position 3 if active | angle axis 3 if active], then the
 * active intrinsics in ascending parameter index.  Jacobians are analytic and the normal equations (block diagonal +
 * intrinsics arrow) are assembled and solved on the device by the kernels of the spline path.
 * Options (oicc_ba_set_option): the trust-region options of oicc_set_option with Theia's defaults (function_tolerance
 * 1e-6, parameter_tolerance 1e-8, gradient_tolerance 1e-10, max_trust_region_radius 1e12), huber_width (1.345 as both
 * reference call sites set it; <= 0: trivial loss). */
typedef struct oicc_ba oicc_ba;
enum { OICC_BA_POSITION = 1, OICC_BA_ORIENTATION = 2,   /* !constant_camera_position / !constant_camera_orientation */
       /* theia::BundleAdjustTracks (camera_calibrator.cc:207-213, pose_estimator.cc:192-224): the board points are the
        * variables (homogeneous 4-vectors under ceres::HomogeneousVectorParameterization: 3 tangent dimensions each, as
        * use_homogeneous_point_parametrization selects), every camera constant; not combinable with the other flags or
        * with an intrinsics mask.  Tangent order: 3 per variable point in point order. */
       OICC_BA_POINTS = 4 };
int oicc_ba_create(oicc_ba** out, int32_t device_ordinal);
void oicc_ba_destroy(oicc_ba* p);
const char* oicc_ba_last_error(const oicc_ba* p);
int oicc_ba_set_option(oicc_ba* p, const char* name, double value);
/* model / parameter order as oicc_set_camera (theia::Camera intrinsics of the shared group) */
int oicc_ba_set_camera(oicc_ba* p, int32_t model, const double* intrinsics, int32_t n);
int oicc_ba_get_camera(const oicc_ba* p, double* intrinsics, int32_t n);
int oicc_ba_set_scene_points(oicc_ba* p, const double* xyzw, int64_t n);
int oicc_ba_get_scene_points(const oicc_ba* p, double* xyzw, int64_t n);
/* which points OICC_BA_POINTS may move (1) -- PoseEstimator::OptimizeBoardPoints adjusts only tracks with more than 30
 * observations (pose_estimator.cc:201-208); default after oicc_ba_set_scene_points: all */
int oicc_ba_set_variable_points(oicc_ba* p, const uint8_t* variable, int64_t n);
/* views: pose6 [nv][6] = theia::Camera position and angle axis (world -> camera); the observations of view v are
 * uv / point_ids [corner_offsets[v], corner_offsets[v+1]).  Replaces all views (the reference's RemoveView = resend). */
int oicc_ba_set_views(oicc_ba* p, int64_t nv, const double* pose6, const int64_t* corner_offsets, const double* uv,
                      const int32_t* point_ids);
int oicc_ba_set_poses(oicc_ba* p, const double* pose6, int64_t nv);
int oicc_ba_get_poses(const oicc_ba* p, double* pose6, int64_t nv);
/* cost (with the loss), dense J^T J [P][Pcap] and J^T r of the robustified problem at the current parameters */
int oicc_ba_evaluate(oicc_ba* p, int32_t flags, int32_t intrinsics_mask, double* cost, double* H, double* g, int32_t Pcap);
/* theia::BundleAdjustViews over all views: flags = OICC_BA_*, intrinsics_mask bit k = intrinsics parameter k variable
 * (theia's GetSubsetFromOptimizeIntrinsicsType, resolved by the host mirror per camera model). */
int oicc_ba_optimize(oicc_ba* p, int32_t max_iters, int32_t flags, int32_t intrinsics_mask, oicc_summary* summary);
int oicc_ba_get_iterations(const oicc_ba* p, oicc_iteration* out, int32_t cap);
/* theia::BundleAdjustView for EVERY view independently (intrinsics constant): one kernel launch, one wavefront per
 * view runs that view's whole Levenberg-Marquardt loop.  iterations / final_cost: [nv] or NULL; a view without
 * observations, or whose residuals cannot be evaluated at the start, is left untouched and reports -1 / NaN. */
int oicc_ba_optimize_views(oicc_ba* p, int32_t max_iters, int32_t flags, int32_t* iterations, double* final_cost);
/* The covariances the reference takes from theia::BundleAdjustTracks / ceres::Covariance [EXT] after the board point refinement
 * (pose_estimator.cc:193-223): for OICC_BA_POINTS with every camera constant the 3 x 3 diagonal blocks of J^T J are independent, and
 * cov9 [n][9] receives the inverse of every variable point's block at the current parameters (tangent space of the homogeneous
 * point, robustified residuals as oicc_ba_evaluate), NaN for constant points; n = the number of scene points.
 * variance_factor (may be NULL) = 2 cost / (2 observations - 3 variable points); nothing is multiplied by it. */
int oicc_ba_point_covariances(oicc_ba* p, double* cov9, int64_t n, double* variance_factor);
/* Covariance of the intrinsics and the view poses, variable TOGETHER (no counterpart in the reference): (J^T J)^-1 at the
 * current parameters for the J^T J that oicc_ba_evaluate returns for the same flags, intrinsics_mask and huber_width
 * (robustified residuals), in its tangent order.  J^T J is a block diagonal (one d x d block per view, d = pose_dim = 3 or 6)
 * with an intrinsics arrow of a <= 10 columns: once the intrinsics are eliminated the views are independent, so the device
 * computes a view-parallel Schur complement -- never a dense P x P inverse -- on the matrix scaled to unit diagonal
 * (S H S, s_i = H_ii^-1/2, no damping; cov_ij = s_i s_j Zs_ij).  A view without observations is left out of the system: it
 * counts neither in P nor in views_used and its blocks are NaN.  d = 0 (poses constant) and a = 0 (intrinsics constant) are
 * allowed.  Two estimates at the same parameters return the same bits in the arrays and in rcond, whatever the number of
 * observations of a view (sums that the assembly forms with atomics in arrival order are formed again in a fixed order); cost
 * and variance_factor come from the assembly pass and may differ in their last bits.
 *   status           as oicc_covariance_status above; OICC_COV_RANK_DEFICIENT when a pivot is not positive or
 *                    rcond < option covariance_min_rcond (oicc_ba_set_option, default 1e-12)
 *   first_bad        -1, else the view -- or nv + intrinsics column -- of the first pivot (or diagonal entry) that failed
 *   rcond            1 / max_i Zs_ii over every handed-out diagonal entry of the scaled inverse
 *   variance_factor  2 cost / (num_residuals - P), num_residuals = 2 observations; nothing is multiplied by it
 * oicc_ba_estimate_covariance returns OICC_OK for each status, OICC_ERR_INVALID_ARG for OICC_BA_POINTS in flags
 * (oicc_ba_point_covariances is the entry for the board points) and for an empty active set.  The getters return
 * OICC_ERR_STATE unless the last estimate has status OICC_COV_OK and still belongs to the current parameters: every setter,
 * oicc_ba_set_option, oicc_ba_optimize and oicc_ba_optimize_views invalidate it. */
typedef struct oicc_ba_covariance_info {
  int32_t status;            /* oicc_covariance_status */
  int32_t P, pose_dim, a;    /* P = pose_dim * views_used + a */
  int32_t views_used;        /* views with at least one observation */
  int32_t first_bad;
  int64_t num_residuals;
  double cost, variance_factor, rcond;
} oicc_ba_covariance_info;
int oicc_ba_estimate_covariance(oicc_ba* p, int32_t flags, int32_t intrinsics_mask, oicc_ba_covariance_info* info);
/* cov [a][a] row major, ascending parameter index of the variable intrinsics; a_capacity >= a */
int oicc_ba_get_covariance_intrinsics(const oicc_ba* p, double* cov, int32_t a_capacity);
/* blocks [nv][d][d]: the full covariance of every view's pose in the tangent order of oicc_ba_evaluate */
int oicc_ba_get_covariance_poses(const oicc_ba* p, double* blocks, int64_t nv);
/* cross [nv][d][a]: the covariance of every view's pose with the intrinsics */
int oicc_ba_get_covariance_pose_intrinsics(const oicc_ba* p, double* cross, int64_t nv);
/* Device time of the last estimate in ms, whatever its status: [0] the assembly pass -- the device work of one oicc_ba_evaluate --,
 * [1] the covariance kernels behind it.  Recorded (HIP events on the estimate's stream) only while option covariance_timing is 1
 * (oicc_ba_set_option, default 0: an estimate records nothing); OICC_ERR_STATE when the last estimate was not timed. */
int oicc_ba_get_covariance_timing(const oicc_ba* p, double ms[2]);
/* GetReprojErrorOfView for every view: mean pixel distance of its observations, [nv] */
int oicc_ba_view_reprojection_errors(oicc_ba* p, double* mean_px);

/* ---- Static multi-pose IMU intrinsics (imu_tk) ---------------------------------------------------------------
 * applications/static_imu_calibration.cc + core::StaticImuCalibrator (src/core/static_imu_calibrator.cc, residuals in
 * include/OpenCameraCalibrator/core/static_imu_calibrator.h): accelerometer and gyroscope triads T*K*(x - B) from an
 * initial still period and a series of still poses.  Parameter vectors, in the reference's order:
 *   accelerometer [9]  misYZ misZY misZX sX sY sZ bX bY bZ            (MultiPosAccResidual; misXZ = misXY = misYX = 0)
 *   gyroscope    [12]  misYZ misZY misZX misXZ misXY misYX sX sY sZ bX bY bZ   (MultiPosGyroResidual)
 * with T = [[1,-misYZ,misZY],[misXZ,1,-misZX],[-misXY,misYX,1]], K = diag(s) (utils/types.h:171-330).
 * Samples are [n][3] row-major, times in seconds.  No CPU fallback: OICC_ERR_NO_DEVICE without a usable HIP device. */
enum {
  OICC_SIMU_THRESHOLDS = 10,          /* th_mult = 1..10 (static_imu_calibrator.cc:79) */
  OICC_SIMU_ACC_IMPOSSIBLE = 1,       /* oicc_static_imu_calibrate: no threshold gave min_num_intervals intervals */
  OICC_SIMU_TERM_SKIPPED = -1,        /* threshold not solved: too few intervals */
  OICC_SIMU_TERM_GRADIENT = 0,        /* Ceres CONVERGENCE: gradient tolerance */
  OICC_SIMU_TERM_FUNCTION = 1,        /* Ceres CONVERGENCE: function tolerance */
  OICC_SIMU_TERM_PARAMETER = 2,       /* Ceres CONVERGENCE: parameter tolerance */
  OICC_SIMU_TERM_MAX_ITERATIONS = 3,  /* Ceres NO_CONVERGENCE */
  OICC_SIMU_TERM_MIN_RADIUS = 4,      /* Ceres CONVERGENCE: minimum trust region radius */
  OICC_SIMU_TERM_INVALID_STEPS = 5,   /* Ceres FAILURE: max_num_consecutive_invalid_steps */
  OICC_SIMU_TERM_EVAL_FAILED = 6      /* the residuals could not be evaluated at the start point */
};
/* The StaticImuCalibrator setters (static_imu_calibrator.h); class defaults in brackets (.cc:44-52). */
typedef struct oicc_static_imu_options {
  double gravity_magnitude;           /* SetGravityMagnitude [9.81; the application passes 9.811107] */
  double init_interval_duration_s;    /* SetInitStaticIntervalDuration [30; the application passes 10] */
  double gyro_dt;                     /* SetGyroDataPeriod [-1]: <= 0 integrates with the sample timestamps */
  int32_t interval_n_samples;         /* SetIntarvalsNumSamples [100] */
  int32_t min_num_intervals;          /* [12] */
  int32_t win_size;                   /* StaticIntervalsDetector window [101]; < 11 -> 11, even -> +1; at most 1025 here */
  int32_t acc_use_means;              /* EnableAccUseMeans [0] */
  int32_t optimize_gyro_bias;         /* EnableGyroBiasOptimization [0] */
  int32_t reserved;
} oicc_static_imu_options;
typedef struct oicc_static_imu_report {
  int32_t th_mult;                                 /* the threshold multiplier kept (strictly smallest final cost), or -1 */
  int32_t num_intervals[OICC_SIMU_THRESHOLDS];     /* extracted intervals (>= interval_n_samples samples) per th_mult */
  int32_t acc_iterations[OICC_SIMU_THRESHOLDS];    /* LM iterations after iteration 0 */
  int32_t acc_termination[OICC_SIMU_THRESHOLDS];   /* OICC_SIMU_TERM_* */
  int32_t gyro_num_blocks, gyro_iterations, gyro_termination;
  double norm_th;                                  /* |variance| of the initial interval (.cc:72-73) */
  double init_acc_bias[3];                         /* initial accelerometer bias (.cc:63-68) */
  double acc_final_cost[OICC_SIMU_THRESHOLDS];     /* 0.5 sum r^2 at the solution; NaN where skipped */
  double gyro_init_bias[3];                        /* mean of the initial interval of the gyroscope (.cc:209-211) */
  double gyro_initial_cost, gyro_final_cost;
  double ms_detector, ms_acc, ms_gyro;             /* device time: detector launches, batched fits, all gyro evaluations */
} oicc_static_imu_report;
/* utils::StaticIntervalsDetector (src/utils/imu_data_interval.cc:111-149) for num_thresholds (<= 10) thresholds in one
 * pass: norm[i] = |DataVariance(acc, [i-h, i+h])| for i in [h, n-h) (sequential mean, sequential squared differences,
 * / (w-1); |v| = sqrt((vx^2 + vy^2) + vz^2), no FMA contraction), compared with every threshold; an interval starts at
 * norm < th and ends before norm >= th, one still open closes at n-h-1; w >= n gives none.  counts[t] is the number of
 * intervals of threshold t; intervals[t][k] = (start, end) for k < min(counts[t], capacity) (row stride 2*capacity).
 * norms (may be NULL): [n], NaN outside [h, n-h).  Samples must be finite (OICC_ERR_INVALID_ARG otherwise). */
int oicc_static_imu_intervals(int32_t device_ordinal, int64_t n, const double* acc, int32_t num_thresholds,
                              const double* thresholds, int32_t win_size, int32_t capacity, int32_t* counts,
                              int32_t* intervals, double* norms, double* device_ms);
/* MultiPosAccResidual (static_imu_calibrator.h:18-58) at params[9] for num samples: r = g_mag - |T K (x - b)| and its
 * Jacobian (rows [num][9], may be NULL, as residuals), cost = 0.5 sum r^2, gram = J^T J [9][9] and gradient = J^T r
 * reduced on the device in the order the batched fit uses. */
int oicc_static_imu_eval_acc(int32_t device_ordinal, int64_t num, const double* samples, double g_mag, const double* params,
                             double* residuals, double* jacobian, double* cost, double* gram, double* gradient);
/* MultiPosGyroResidual (static_imu_calibrator.h:60-140) for num_blocks blocks: block b integrates the bias-free gyro
 * samples ranges[b][0]..ranges[b][1] (RK4, utils/gyro_integration.h; dt = gyro_dt if > 0, else timestamp differences)
 * and r_b = R^T g[b][0:3] - g[b][3:6].  Parameters: 9, or 12 with optimize_bias (params always has room for 12).
 * residuals [3 num_blocks], jacobian [3 num_blocks][np] (either may be NULL), cost, gram [np][np], gradient [np].
 * device_ms (may be NULL): time of the launch. */
int oicc_static_imu_eval_gyro(int32_t device_ordinal, int64_t n, const double* t_s, const double* gyro, int32_t num_blocks,
                              const int32_t* ranges, const double* g_versors, int32_t optimize_bias, double gyro_dt,
                              const double* params, double* residuals, double* jacobian, double* cost, double* gram,
                              double* gradient, double* device_ms);
/* StaticImuCalibrator::CalibrateAccGyro (static_imu_calibrator.cc:188-337, CalibrateAcc :54-186): acc and gyro share
 * the timestamps t_s [n].  acc_params: the accelerometer vector of the kept threshold; gyro_params: the final gyroscope
 * triad (bias = initial-interval mean + fitted bias terms).  Returns OICC_OK, or OICC_SIMU_ACC_IMPOSSIBLE when no
 * threshold leaves min_num_intervals intervals (then both outputs are the default triad: identity, zero bias, and the
 * gyroscope is not fitted), or an error.  opt may be NULL (the class defaults); report may be NULL. */
int oicc_static_imu_calibrate(int32_t device_ordinal, int64_t n, const double* t_s, const double* acc, const double* gyro,
                              const oicc_static_imu_options* opt, double* acc_params, double* gyro_params,
                              oicc_static_imu_report* report);

/* ---- radon checkerboard extraction (board.hip) ------------------------------------------------------------------------
 * applications/extract_board_to_json.cc + core::BoardExtractor (src/core/board_extractor.cc:200-225, 268-380) for
 * BoardType::RADON: the reference calls cv::findChessboardCornersSB(CALIB_CB_LARGER | CALIB_CB_MARKER |
 * CALIB_CB_EXHAUSTIVE) per frame after cv::resize(1 / downsample_factor) and BGR2GRAY.  This entry is our own detector
 * (localized Radon response after Duda & Frese 2018, cornerSubPix's saddle refinement, homography grid growth, the
 * target's three marker dots), specified by tests/board_restatement.py and DESIGN.md ("Board extraction").  A frame
 * reports all W*H corners with ids i*W + j (pattern row i, column j) or none. */
typedef struct oicc_board_options {
  int32_t radius;                     /* line half length r (1..8) [3]; sub-pixel window half size r + 2 */
  float threshold_rel;                /* candidates: response > threshold_rel * frame maximum [0.5] */
  int32_t max_candidates;             /* per-frame cap (>= W*H); a frame with more candidates reports nothing [512] */
  int32_t subpix_iterations;          /* cornerSubPix TermCriteria count [20] */
  double subpix_eps;                  /* cornerSubPix TermCriteria epsilon (compared squared, as OpenCV) [0.01] */
  int32_t batch;                      /* frames per launch chain; two batches are in flight [64] */
  int32_t reserved;
} oicc_board_options;
typedef struct oicc_board_report {
  int32_t frames_found, frames_overflow;           /* frames with a board; frames over max_candidates */
  int32_t output_width, output_height;             /* the image size after the resize */
  int64_t num_candidates;                          /* summed over frames */
  double ms_resize, ms_response, ms_candidates, ms_subpix, ms_marker;   /* device time per kernel, summed */
  double ms_assembly_host;                         /* grid assembly and marker decision on the host */
  double ms_total;                                 /* wall time of the call */
} oicc_board_report;
/* Optional per-stage outputs for checking (any pointer may be NULL): gray and response [frames][h'][w'], candidates
 * (x, y) and refined (x, y) [frames][capacity][2] in raster order of the candidates (entries beyond the frame's count
 * are left untouched).  extended = 0: the struct ends at that field, as callers built before it grew pass it, and nothing
 * behind it is read.  Non-zero: the fields behind it are present, each of which may be NULL again:
 *   polarity   [frames][h'][w']: the index of the brightest line (0 within the radius of the border);
 *   blurred    [frames][h'][w']: the 3x3 binomial blur as float, the image the sub-pixel and marker kernels read;
 *   grid_shape [frames][2]: (A, B) of the assembled grid, {A, B} = {W, H}, or (0, 0) when no grid was assembled;
 *   grid       [frames][W*H]: for grid cell a*B + b the index of its candidate in the frame's raster-ordered list;
 *   disc, ring [frames][(W-1)*(H-1)]: the marker kernel's means of square a*(B-1) + b of that grid.
 * grid, disc and ring of a frame without a grid are left untouched.  Every copy happens only when its pointer is set. */
typedef struct oicc_board_stages {
  uint8_t* gray;
  float* response;
  int32_t* candidates;
  double* refined;
  int32_t capacity;
  int32_t extended;
  uint8_t* polarity;
  float* blurred;
  int32_t* grid_shape;
  int32_t* grid;
  double* disc;
  double* ring;
} oicc_board_stages;
/* The resize of ExtractImageFolderToJson (board_extractor.cc:317-318): output size round(width / factor). */
int oicc_board_output_size(int32_t width, int32_t height, double downsample_factor, int32_t* out_width, int32_t* out_height);
/* frames [num_frames][height][width][channels] u8 (channels 1 = gray, 3 = BGR as cv::imread gives), resized by
 * 1 / downsample_factor and converted to gray (board_extractor.cc:317-322), then detected.  corners [num_frames][W*H][2]
 * (NaN where not found), found [num_frames], candidates_per_frame [num_frames] (may be NULL), report and stages may be
 * NULL. */
int oicc_board_radon_detect(int32_t device_ordinal, int32_t num_frames, int32_t width, int32_t height, int32_t channels,
                            const uint8_t* frames, double downsample_factor, int32_t W, int32_t H,
                            const oicc_board_options* opt, double* corners, int32_t* found, int32_t* candidates_per_frame,
                            oicc_board_report* report, const oicc_board_stages* stages);

/* ---- robust start poses: planar RANSAC over the views of a corner file (planar_ransac.hip) --------------------------------
 * The reference takes the start pose (and focal length) of every view from TheiaSfM's RANSAC minimal solvers [EXT]
 * (camera_calibrator.cc:262-301, pose_estimator.cc:54-83) and, in the pose estimator, keeps only the RANSAC inliers.  This
 * entry selects the inliers of ALL views in one launch (one workgroup per view, one lane per hypothesis); the start values
 * themselves stay the closed forms of the host side, run on the inliers.  Model: the radial alignment constraint
 *   u (q3 a + q4 b + q5) - v (q0 a + q1 b + q2) = 0
 * for board plane coordinates (a, b) and features (u, v) relative to the distortion centre, five corners per sample;
 * specified step by step by tests/planar_ransac_restatement.py and DESIGN.md ("Robust start poses").
 *   corner_offsets [num_views + 1] (first 0), ab and xy [n][2] with n = corner_offsets[num_views];
 *   mode 0: uncalibrated features (pixels relative to the principal point): vote, least-squares refit of q, tangential test;
 *   mode 1: calibrated features (normalised image coordinates, f = 1): additionally the pose completed from q and the full
 *           reprojection test;  threshold in the units of xy;  num_hypotheses 1..1024 per view, fixed;  seed of the sampler.
 *   inlier [n] (0 / 1), num_inliers [num_views], q [num_views][6] (unit norm, sign towards the corners),
 *   pose [num_views][12] = R row-major | t, board plane frame -> camera (mode 1; untouched in mode 0, may be NULL there),
 *   hypothesis_counts [num_views][num_hypotheses] (may be NULL): the score of every hypothesis, for checking,
 *   device_ms (may be NULL): kernel time by device events.
 * A view with fewer than 5 corners, without a hypothesis of 5 inliers, or with board corners on one line gets
 * num_inliers = 0 (zero q and pose), not an error.  OICC_ERR_INVALID_ARG for non-finite input, a threshold <= 0, a
 * hypothesis count outside 1..1024, offsets that decrease or a view of more than 2^20 corners; OICC_ERR_NO_DEVICE without
 * a usable HIP device (no CPU fallback). */
int oicc_planar_ransac(int32_t device_ordinal, int32_t num_views, const int64_t* corner_offsets, const double* ab, const double* xy,
                       int32_t mode, double threshold, int32_t num_hypotheses, uint64_t seed, uint8_t* inlier,
                       int32_t* num_inliers, double* q, double* pose, int32_t* hypothesis_counts, double* device_ms);

/* ---- camera maps: pixel -> ray, rectification maps, model discrepancy and image resampling (camera_maps.hip) ---------------
 * The device has the forward projection of the six camera models (camera_project, spline_math.h); these entries add its
 * inverse and what users build on it: undistorted frames and the same camera expressed in another model.  Specified step by
 * step by tests/camera_maps_restatement.py and DESIGN.md ("Camera maps").  Models and intrinsics as in oicc_set_camera; the
 * intrinsics arrays hold the model's own count (PINHOLE 7, PINHOLE_RADIAL_TANGENTIAL 10, FISHEYE 9, DIVISION_UNDISTORTION 5,
 * DOUBLE_SPHERE 7, EXTENDED_UNIFIED 7).
 *
 * oicc_camera_unproject: one lane per pixel; Newton on project(x, y, 1) = uv with the analytic Jacobian, from the pinhole start
 *   x0 = (u - cx) / f, y0 = (v - cy) / (f aspect), at most 20 steps, stop at max|step| <= 1e-13 (1 + max|xy|).
 *   uv [n][2] pixels, xy [n][2] rays (x, y, 1), status [n]: 0 a ray, 1 no ray on the principal branch (xy = NaN).
 *   Status 0 needs finite values, a projection that did not fail, max|project(x, y, 1) - uv| <= 1e-9 (1 + max|uv|) and, for
 *   A = d(px)/d(x, y) at the solution, det A > 0 and A00 / f + A11 / (f aspect) > 0: beyond the fold of a camera whose radial
 *   map turns back, Newton converges onto rays that reproject exactly but are not the ones the lens imaged.
 *   Limitations: rays are (x, y, 1), so fields of view of 180 degrees and more are out of scope; a model whose radial map
 *   folds twice can still offer a second branch on which both signs are positive.
 *   n_intr must be the model's count; device_ms (may be NULL): kernel time by device events.
 * oicc_camera_rectify_map: for every pixel of a destination camera the coordinates of the same ray in a source camera.
 *   Unproject through the destination camera (closed form for a PINHOLE without distortion, else the Newton above), rotate by
 *   R9 (row-major 3 x 3, destination camera -> source camera; NULL = identity), project through the source camera.
 *   map [dst_h][dst_w][2] float32 (x, y) source coordinates, the layout of OpenCV's CV_32FC2 maps; valid [dst_h][dst_w]: 1 iff
 *   the pixel has a ray, the rotated ray has z > 0, the projection succeeded and the coordinates lie in
 *   [0, src_w - 1] x [0, src_h - 1]; invalid pixels get NaN coordinates.  num_valid (may be NULL): the number of ones.
 * oicc_camera_discrepancy: every pixel of a w x h image is unprojected through camera A and projected through camera B;
 *   stats[3] = number of pixels with a ray and a projection, rms and maximum of the distance |px_B - px| over them (0 without
 *   one).  One partial row per wave by a fixed butterfly, added on the host in order: bit-identical between runs.
 * oicc_camera_remap: bilinear resampling of num_frames u8 frames [src_h][src_w][channels] (channels 1 or 3) through one map
 *   [dst_h][dst_w][2] float32, out [num_frames][dst_h][dst_w][channels].  Host pointers; frames travel in batches of `batch`
 *   through pinned staging, two batches in flight on two streams.  Value: ((1-a)(1-b) p00 + a(1-b) p01) + ((1-a) b p10 + a b p11)
 *   in double, (a, b) the fractions of the float32 coordinates, then floor(v + 0.5) clamped to 0..255; a neighbour of weight
 *   exactly 0 is not read, so coordinates on the last row or column are legal.  A map entry that is NaN or outside
 *   [0, src_w - 1] x [0, src_h - 1] gives border_value.  report (may be NULL): milliseconds by device events, summed over
 *   the batches, and the wall time of the call.
 * oicc_camera_remap_device: the same kernel on device pointers, asynchronous on hip_stream (a hipStream_t; NULL = the
 *   default stream), no copies, on the current device: frames that already live on the GPU stay there.  The stream and the
 *   three arrays must belong to the current device (OICC_ERR_INVALID_ARG otherwise).  oicc_camera_remap runs every batch
 *   through this entry.
 * OICC_ERR_INVALID_ARG for an unknown model, a wrong intrinsics count, non-finite intrinsics or R9, sizes < 1, channels
 * other than 1 or 3, a batch < 1, a null array or more than (2^31 - 1) * 256 pixels in one call; OICC_ERR_NO_DEVICE without a usable HIP device (no CPU fallback). */
typedef struct oicc_camera_remap_report {
  double ms_upload, ms_kernel, ms_download, ms_total;
} oicc_camera_remap_report;
int oicc_camera_unproject(int32_t device_ordinal, int32_t model, const double* intrinsics, int32_t n_intr, int64_t n, const double* uv,
                          double* xy, uint8_t* status, double* device_ms);
int oicc_camera_rectify_map(int32_t device_ordinal, int32_t src_model, const double* src_intr, int32_t src_w, int32_t src_h,
                            int32_t dst_model, const double* dst_intr, int32_t dst_w, int32_t dst_h, const double* R9, float* map,
                            uint8_t* valid, int64_t* num_valid, double* device_ms);
int oicc_camera_discrepancy(int32_t device_ordinal, int32_t model_a, const double* intr_a, int32_t model_b, const double* intr_b,
                            int32_t w, int32_t h, double stats[3], double* device_ms);
int oicc_camera_remap(int32_t device_ordinal, int32_t num_frames, int32_t src_w, int32_t src_h, int32_t channels, const uint8_t* frames,
                      const float* map, int32_t dst_w, int32_t dst_h, int32_t border_value, int32_t batch, uint8_t* out,
                      oicc_camera_remap_report* report);
int oicc_camera_remap_device(void* hip_stream, int32_t num_frames, int32_t src_w, int32_t src_h, int32_t channels,
                             const uint8_t* frames_dev, const float* map_dev, int32_t dst_w, int32_t dst_h, int32_t border_value,
                             uint8_t* out_dev);

/* ---- rolling shutter: gyro-driven row maps, rectified frames and features (rolling_shutter.hip) ----------------------------
 * What the calibrated line delay and gyro-to-camera rotation are for: taking the rolling shutter out of footage and features.
 * Specified step by step by tests/rolling_shutter_restatement.py and DESIGN.md ("Rolling-shutter rectification").
 *
 * Model: rotation only, the standard gyro correction.  The camera is taken to turn about its centre during the readout;
 * translation (parallax) is not modelled; smoothing between frames is the next section's.  Rays are (x, y, 1): fields of view of
 * 180 degrees and more are out of scope.
 *   Time.  Row y (continuous) of frame k is exposed at frame_t[k] + y line_delay_s in the camera clock; line_delay_s has any
 *   sign, 0 included.  A gyro sample at IMU time t lies at t + time_offset_imu_to_cam in the camera clock (the offset the
 *   spline calibration applies, same sign).  Times enter as differences: a_j = (gyro_t[j] - frame_t[k]) + time_offset, and
 *   tau_j = a_j - reference_row line_delay_s is sample j relative to t_ref,k = frame_t[k] + reference_row line_delay_s.
 *   Rates.  gyro_rates [n][3] are corrected rates MS_g (omega_m - b) in the IMU frame; they are rotated into the camera frame
 *   once, omega_c = R(q_i_c)^T omega_i, q_i_c (w, x, y, z) the rotation of T_i_c as result.json holds it (normalised first).
 *   Orientation.  Between samples j and j + 1 the rate is linear in time: Q(t) = Q_j Exp(phi_j(s)), s = t - t_j,
 *   phi_j(s) = omega_j s + (omega_{j+1} - omega_j) s^2 / (2 dt_j), Q_{j+1} = Q_j Exp(phi_j(dt_j)) (right multiplication, body
 *   rates).  R_rel,k(t) = Q(t_ref,k)^-1 Q(t); a ray d0 of the virtual global-shutter camera at t_ref is R_rel(t)^T d0 in the
 *   camera at time t.  Rows are clamped to [0, src_h - 1] before they become a time.
 *   Frame status, by time comparisons on the host.  The window of frame k is the span of (0, (src_h - 1) line_delay_s,
 *   reference_row line_delay_s).  0: the window lies inside [a_0, a_{n-1}] and touches at most 256 samples (the last sample
 *   with a_j <= the window's start up to the first with a_j >= its end); 1: no gyro coverage; 2: more than 256 samples.
 *   Frames with a status other than 0 get all-invalid maps, border_value pixels, NaN points and rotations: never uncorrected data.
 *   Per destination pixel.  The ray as in oicc_camera_rectify_map (closed form for a plain PINHOLE, else Newton), rotated by
 *   R9 the same way; then the fixed point y_0 = reference_row, tau = (clamp(y_n) - reference_row) line_delay_s,
 *   (x, y)_{n+1} = project_src(R_rel(tau)^T d0), stop at |y_{n+1} - y_n| <= 1e-10 (1 + |y_{n+1}|), at most 24 evaluations.
 *   Valid: a ray, z > 0 before and after R_rel, every projection succeeded with finite values, converged, and coordinates
 *   in [0, src_w - 1] x [0, src_h - 1]; otherwise NaN coordinates and validity 0.  Coordinates are rounded to float32.
 *
 * oicc_rs_rectify_map: map [num_frames][dst_h][dst_w][2] float32, valid [num_frames][dst_h][dst_w], evaluations (may be NULL)
 *   [num_frames][dst_h][dst_w] projections spent, frame_status [num_frames], num_valid (may be NULL) [num_frames],
 *   device_ms (may be NULL) [3] = table kernel, ray kernel, map kernel, by device events.
 * oicc_rs_rectify_frames: host pointers, frames [num_frames][src_h][src_w][channels] u8 (channels 1 or 3) -> out
 *   [num_frames][dst_h][dst_w][channels]; batches of `batch` frames through pinned staging, two in flight, as
 *   oicc_camera_remap.  The fixed point and the bilinear rule of oicc_camera_remap run in one kernel on the float32-rounded
 *   coordinates; no per-frame map is written.  The result equals oicc_camera_remap through oicc_rs_rectify_map's maps.
 * oicc_rs_rectify_frames_device: frames and out on the current device, work enqueued on hip_stream (NULL = the default
 *   stream); the stream and both arrays must belong to the current device (OICC_ERR_INVALID_ARG otherwise).  The small gyro
 *   and frame-time arrays come from the host; the call returns once the stream has run the work and has freed its tables.
 * oicc_rs_rectify_points: forward, no fixed point.  xy_in [n][2] observed in frame frame_index[i] -> source ray -> R_rel(tau(y))
 *   -> R9^T -> destination camera: xy_out [n][2] global-shutter-equivalent coordinates in double.  status [n]: 0 a point,
 *   1 none (no ray, z <= 0 or a failed projection), 2 the frame's status is not 0; 1 and 2 give NaN.
 * oicc_rs_row_rotations: q [n][4] (w, x, y, z) of R_rel at (frame_index[i], rows[i]); status [n] 0, or 2 with NaN.
 * OICC_ERR_INVALID_ARG for fewer than 2 gyro samples, gyro times that do not strictly increase, non-finite input, a q_i_c whose
 * norm is further than 1e-6 from 1, no frames, a frame index out of range, null arrays, and whatever oicc_camera_rectify_map
 * and oicc_camera_remap refuse.  Arguments are judged before the device is looked for; OICC_ERR_NO_DEVICE without one (no
 * CPU fallback). */
typedef struct oicc_rs_scene {
  int32_t src_model, src_w, src_h, dst_model, dst_w, dst_h;
  const double* src_intr;            /* the model's own count, as oicc_camera_rectify_map */
  const double* dst_intr;
  const double* R9;                  /* row-major, destination camera -> source camera; NULL = identity */
  int64_t num_gyro;
  const double* gyro_t;              /* [num_gyro] seconds, IMU clock, strictly increasing */
  const double* gyro_rates;          /* [num_gyro][3] corrected rates, IMU frame, rad/s */
  double q_i_c[4];                   /* w, x, y, z */
  double time_offset_imu_to_cam;
  int32_t num_frames, reserved;
  const double* frame_t;             /* [num_frames] seconds, camera clock: exposure of row 0 */
  double line_delay_s, reference_row;
} oicc_rs_scene;
typedef struct oicc_rs_frames_report {
  double ms_table, ms_rays, ms_upload, ms_kernel, ms_download, ms_total;
} oicc_rs_frames_report;
int oicc_rs_rectify_map(int32_t device_ordinal, const oicc_rs_scene* scene, float* map, uint8_t* valid, uint8_t* evaluations,
                        int32_t* frame_status, int64_t* num_valid, double* device_ms);
int oicc_rs_rectify_frames(int32_t device_ordinal, const oicc_rs_scene* scene, int32_t channels, const uint8_t* frames,
                           int32_t border_value, int32_t batch, uint8_t* out, int32_t* frame_status, oicc_rs_frames_report* report);
int oicc_rs_rectify_frames_device(void* hip_stream, const oicc_rs_scene* scene, int32_t channels, const uint8_t* frames_dev,
                                  int32_t border_value, uint8_t* out_dev, int32_t* frame_status);
int oicc_rs_rectify_points(int32_t device_ordinal, const oicc_rs_scene* scene, int64_t n, const int32_t* frame_index, const double* xy_in,
                           double* xy_out, uint8_t* status, int32_t* frame_status, double* device_ms);
int oicc_rs_row_rotations(int32_t device_ordinal, const oicc_rs_scene* scene, int64_t n, const int32_t* frame_index, const double* rows,
                          double* q, uint8_t* status, int32_t* frame_status, double* device_ms);

/* ---- stabilisation: the orientation path of a clip, a smooth virtual camera, the zoom, the warp (stabilization.hip) ---------
 * What footage is calibrated for: every frame seen from a camera that turns smoothly, the rolling shutter taken out on the way.
 * Specified step by step by tests/stabilization_restatement.py and DESIGN.md ("Stabilisation").  Everything not said here is
 * the rolling-shutter section's: times as differences first, Q(t) with the rate linear inside a gyro interval, right
 * multiplication, reference_row, frame status 0 / 1 / 2, and frames whose status is not 0 never passed through uncorrected.
 * The scene is an oicc_rs_scene with two further requirements (OICC_ERR_INVALID_ARG otherwise): frame_t strictly increasing, and
 * the destination camera a plain PINHOLE (no distortion coefficients), whose rays have a closed form.
 *   1. Path.  Frame k is on the path when t_ref,k lies inside the gyro coverage: tau_0 <= 0 <= tau_{n-1} with
 *   tau_j = ((gyro_t[j] - frame_t[k]) + time_offset) - reference_row line_delay_s.  Such frames are contiguous.  path_q of the first
 *   is the identity; path_{k+1} = path_k D_k, D_k = Q(t_ref,k)^-1 Q(t_ref,k+1) = Exp(phi_a(s_a))^-1 Exp(phi_a(dt_a)) ... Exp(phi_b(s_b)),
 *   chained from the left through the partial interval of t_ref,k, the whole intervals and the partial interval of t_ref,k+1 (one
 *   interval: Exp(phi_a(s_a))^-1 Exp(phi_a(s_b))), any number of gyro samples between two frames; s = -tau of the interval's first
 *   sample against the frame's own time, dt_j = gyro_t[j+1] - gyro_t[j].  The definition is the left-to-right product over the
 *   frames (the device chains runs of frames and scans the run products); each path_k is normalised once at the end.  Frames off
 *   the path have NaN path_q and smooth_q, the identity as correction_q, and a status other than 0.
 *   2. Smooth camera.  The window of frame k: the on-path frames m with |frame_t[m] - frame_t[k]| <= 3 sigma, weights
 *   exp(-dt^2 / (2 sigma^2)).  S_k is their weighted intrinsic mean: S = path_k, then S <- S Exp(sum w_m Log(S^-1 path_m) / sum w_m)
 *   until the step is <= 1e-12 rad, at most 16 times (iterations[k]; the step that meets the bound is applied and counted); S_k is
 *   normalised.  sigma = 0 or a window of one frame: S_k = path_k bit for bit, 0 iterations, correction (1, 0, 0, 0).  Correction
 *   C_k = path_k^-1 S_k, normalised, w >= 0: a ray d0 of the stabilised camera is C_k d0 in the real camera at t_ref,k.  With
 *   max_correction_rad > 0 a C_k of a larger angle is shortened along its own axis to that angle (smooth_q stays the mean).
 *   The warp's rotation of frame k is M_k = R(C_k) R9: R9 is applied to the destination ray first.
 *   3. Required zoom z_k.  Zoom Z multiplies the destination's focal length and skew: the ray of a pixel at zoom Z is its zoom-1
 *   ray divided by Z.  For every border pixel of the destination rectangle (2 (w + h) - 4 of them; all pixels of a rectangle one
 *   pixel wide or high) with zoom-1 ray p, s = j / 32, j = 1 .. 32, marches from the centre outwards; s p is valid when the fixed
 *   point of the rolling-shutter section, with M_k for R9, calls it valid.  At the first invalid sample 16 bisections between it
 *   and its predecessor keep the valid end; no invalid sample: s = 1; an invalid centre (ray (0, 0, 1)): s = 0.
 *   z_k = 1 / min s, +inf for an invalid centre; NaN for frames whose status is not 0.
 *   4. Applied zoom Z_k, on the host.  zoom_mode 0: 1 (borders show).  1: the maximum of z over the status-0 frames.  2: with
 *   T = zoom_window_s, Y_k = max z_m over the status-0 frames with |frame_t[m] - frame_t[k]| <= T (1 if there is none), then
 *   Z_k = sum g Y_m / sum g over the same window, g = exp(-dt^2 / (2 (T / 2)^2)), held inside [min Y_m, max Y_m] of that window:
 *   every Y_m there has z_k in its own window, so Z_k >= z_k.  A Z_k above max_zoom becomes max_zoom and zoom_clamped[k] = 1;
 *   such a frame's invalid pixels get border_value.
 *
 * oicc_stab_plan: the whole clip's frame times in the scene.  path_q, smooth_q, correction_q [num_frames][4] (w, x, y, z);
 *   required_zoom, zoom [num_frames]; iterations, frame_status [num_frames]; zoom_clamped [num_frames]; device_ms (may be NULL) [3]
 *   = path, smoothing and zoom kernels, by device events.
 * oicc_stab_map, oicc_stab_frames, oicc_stab_frames_device: oicc_rs_rectify_map, oicc_rs_rectify_frames and
 *   oicc_rs_rectify_frames_device with two more arrays for the frames of THAT CALL's scene, correction_q [num_frames][4] (unit
 *   within 1e-6, used as given) and zoom [num_frames] (finite, > 0): a program plans once over the clip and then streams chunks
 *   of frames.  Per frame the destination ray is (v - cy) / ((f Z) a), (u - cx - (skew Z) y) / (f Z), f Z and skew Z rounded once;
 *   the map equals oicc_rs_rectify_map's with R9 = M_k and those intrinsics bit for bit.  device_ms / the report's ms_rays: the
 *   kernel that forms M_k.
 * oicc_debug_stab_zoom: step 4 alone, host arithmetic only (needs no device): required_zoom [num_frames] (not NaN where the
 *   status is 0) -> zoom, zoom_clamped.
 * OICC_ERR_INVALID_ARG for what the rolling-shutter entries refuse, frame times that do not strictly increase, a destination
 * that is not a plain PINHOLE, a negative or non-finite smoothing_sigma_s, max_correction_rad or zoom_window_s, a zoom_mode other
 * than 0, 1, 2, a max_zoom below 1 or not finite.  Arguments are judged before the device is looked for; OICC_ERR_NO_DEVICE
 * without one (no CPU fallback). */
typedef struct oicc_stab_options {
  double smoothing_sigma_s, max_correction_rad;
  int32_t zoom_mode, reserved;
  double zoom_window_s, max_zoom;
} oicc_stab_options;
int oicc_stab_plan(int32_t device_ordinal, const oicc_rs_scene* scene, const oicc_stab_options* options, double* path_q, double* smooth_q,
                   double* correction_q, double* required_zoom, double* zoom, int32_t* iterations, int32_t* frame_status,
                   uint8_t* zoom_clamped, double* device_ms);
int oicc_stab_map(int32_t device_ordinal, const oicc_rs_scene* scene, const double* correction_q, const double* zoom, float* map,
                  uint8_t* valid, uint8_t* evaluations, int32_t* frame_status, int64_t* num_valid, double* device_ms);
int oicc_stab_frames(int32_t device_ordinal, const oicc_rs_scene* scene, const double* correction_q, const double* zoom, int32_t channels,
                     const uint8_t* frames, int32_t border_value, int32_t batch, uint8_t* out, int32_t* frame_status,
                     oicc_rs_frames_report* report);
int oicc_stab_frames_device(void* hip_stream, const oicc_rs_scene* scene, const double* correction_q, const double* zoom, int32_t channels,
                            const uint8_t* frames_dev, int32_t border_value, uint8_t* out_dev, int32_t* frame_status);
int oicc_debug_stab_zoom(int32_t num_frames, const double* frame_t, const double* required_zoom, const int32_t* frame_status,
                         const oicc_stab_options* options, double* zoom, uint8_t* zoom_clamped);

/* ---- horizon lock: the smooth camera levelled by gravity from the accelerometer (stabilization.hip) -------------------------
 * The smooth camera of the section above still carries the roll the operator held.  With the accelerometer the plan can take it
 * out: a different correction_q from the same path and smooth camera; the zoom and the warp are the section above's, unchanged.
 * Specified step by step by tests/horizon_restatement.py and DESIGN.md ("Horizon lock").
 *   Input.  accl [num_accl][3] is the corrected specific force MS_a (a_m - b_a) in the IMU frame, m/s^2: at rest it points up.
 *   accl_t [num_accl] are its times in the IMU clock, strictly increasing; they need not be the gyroscope's.
 *   G1.  Per sample j and on-path frame k, s_jk = ((accl_t[j] - frame_t[k]) + time_offset) - reference_row line_delay_s.  The
 *   sample's frame k(j) is the last on-path frame with s_jk >= 0; a sample before the first on-path frame's reference time or
 *   behind the last one's is unused (NaN vector, frame -1).  D_j is the chain D_k of the path with the sample's time in place of
 *   t_ref,k+1: through the partial interval of t_ref,k, the whole gyro intervals and the partial interval that holds the sample, the
 *   last i <= n - 2 with tau_i(k) <= s_jk, entered by s_jk - tau_i(k).  q_j = normalised(path_k D_j) and
 *   u_j = R(q_j) (R(q_i_c)^T a_j): the sample in the frame of the path.  Gate g_j = 1 if accl_gate == 0 or
 *   | |a_j| - gravity_const | <= accl_gate, else 0.
 *   G2.  Per on-path frame k the window is the used samples with |s_jk| <= 3 gravity_sigma_s, w = exp(-s^2 / (2 sigma_g^2)) g_j;
 *   gbar_k = sum w u / sum w; gravity_samples[k] counts the window's samples with g_j = 1.  level_status[k] = 2 when that count is 0
 *   or |gbar_k| < 0.5 gravity_const (and for frames off the path): no angle, NaN up and roll.  Otherwise
 *   up_k = R(S_k)^T gbar_k / |gbar_k| is up in the smooth camera (x right, y down, z forward), h = sqrt(up_x^2 + up_y^2),
 *   roll_k = atan2(up_x, -up_y), fade = clamp((h - sin 10 deg) / (sin 20 deg - sin 10 deg), 0, 1).  level_status[k] = 1 when
 *   h < sin 10 deg: the camera looks along gravity, the roll is undefined and not applied.  Otherwise status 0 and
 *   level_angle_k = lock fade wrap(roll_k - roll_rad), wrap into (-pi, pi] (roll_rad is reduced by the IEEE remainder of 2 pi first).
 *   L_k = normalised(S_k (cos angle/2, 0, 0, sin angle/2)); C_k = path_k^-1 L_k, normalised, w >= 0, then the max_correction_rad
 *   clamp of the section above.  A frame whose angle is exactly 0 (lock 0, status 1 or 2, a level camera) keeps level_q = smooth_q
 *   and the correction_q of oicc_stab_plan bit for bit.  This also runs at smoothing_sigma_s = 0 or a window of one frame, where
 *   S_k = path_k.  smooth_q stays the mean.  A partial lock is discontinuous at roll = +-pi (camera upside down): not solved.
 *   G3.  Required and applied zoom as in the section above, from the new C_k.
 *
 * oicc_stab_plan_level: oicc_stab_plan with a level (NULL: no horizon lock; every common output is oicc_stab_plan's bit for bit,
 *   level_q = smooth_q, NaN up and roll, zeros elsewhere) and six more arrays: level_q [num_frames][4], up [num_frames][3], roll,
 *   level_angle [num_frames], gravity_samples, level_status [num_frames].  device_ms (may be NULL) [5]: path, smoothing, zoom,
 *   G1 and G2 kernels.
 * oicc_debug_stab_accl_world: G1 alone: world [num_accl][3], frame_of [num_accl].
 * OICC_ERR_INVALID_ARG for everything oicc_stab_plan refuses, num_accl < 1, null arrays, accelerometer times that do not strictly
 * increase, non-finite samples, gravity_sigma_s <= 0, gravity_const <= 0, accl_gate < 0, lock outside [0, 1] or a non-finite
 * roll_rad.  Arguments are judged before the device is looked for; OICC_ERR_NO_DEVICE without one (no CPU fallback). */
typedef struct oicc_stab_level {
  int64_t num_accl;
  const double* accl_t;              /* [num_accl] seconds, IMU clock, strictly increasing */
  const double* accl;                /* [num_accl][3] corrected specific force, IMU frame, m/s^2 */
  double gravity_sigma_s, gravity_const, accl_gate, lock, roll_rad;
} oicc_stab_level;
int oicc_stab_plan_level(int32_t device_ordinal, const oicc_rs_scene* scene, const oicc_stab_options* options, const oicc_stab_level* level,
                         double* path_q, double* smooth_q, double* correction_q, double* required_zoom, double* zoom, int32_t* iterations,
                         int32_t* frame_status, uint8_t* zoom_clamped, double* level_q, double* up, double* roll, double* level_angle,
                         int32_t* gravity_samples, int32_t* level_status, double* device_ms);
int oicc_debug_stab_accl_world(int32_t device_ordinal, const oicc_rs_scene* scene, const oicc_stab_level* level, double* world,
                               int32_t* frame_of);

/* ---- the elimination plan of the block cyclic reduction (kernels_bcr.hip), host arithmetic only: needs no device ----------
 * The damped LM system of n 64-column blocks is reduced level by level.  Level l: the active blocks are origin + k stride,
 * k < active; those with k mod 2 == parity are its pivots (parity 0 when `active` is odd -- both ends are pivots --, else 1;
 * odd_only != 0: parity 1 at every level, the order of the distributed reduction; ghost != 0: that reduction's extra right
 * neighbour, one more coupling per level).  levels [cap_levels][6] = origin, stride, parity, active, pivots, first slot of
 * the level's couplings (active - 1 + ghost of them, slot + k: active blocks k and k + 1); info[3] = the block that is
 * left at the end, the slot behind the last level's couplings, the slots the solver's workspace reserves.
 * Returns the number of levels (= inversions in sequence - 1), OICC_ERR_INVALID_ARG for n < 1 or too small a cap_levels. */
int oicc_debug_bcr_plan(int32_t n, int32_t ghost, int32_t odd_only, int64_t* levels, int32_t cap_levels, int64_t info[3]);
/* Which levels of that plan the solver runs as ONE launch -- every workgroup of a pivot inverts it itself and goes on with its Schur
 * group -- instead of an inversion launch and a Schur launch (the solver's own rule, host arithmetic only).  joined [cap_levels] = 1 / 0
 * per level.  A level is joined when join_levels != 0 (option bcr_join_levels), the solve is the whole band (ghost == 0, b0 == 0: the
 * first block of a rank's range; no carried coupling), its inversions are not part of the build launch (level 0 when build_inverts
 * != 0; build_inverts < 0: as the solver decides for n blocks) and pivots x (12 + 3 rtf) <= budget (rtf: 16-row tiles of the arrow
 * rows + right-hand side, 1..4; budget: option bcr_join_max_workgroups, or the device's compute units).
 * Returns the number of levels, OICC_ERR_INVALID_ARG as above or for rtf, budget, b0 out of range. */
int oicc_debug_bcr_join_plan(int32_t n, int32_t ghost, int32_t odd_only, int32_t b0, int32_t rtf, int32_t join_levels, int32_t budget,
                             int32_t build_inverts, int32_t* joined, int32_t cap_levels);
/* Whether level 0 of that plan runs as ONE launch behind a plain build launch, instead of a build launch that also inverts level 0's
 * pivots and a Schur launch (the solver's own rule, host arithmetic only): join_levels (option bcr_join_levels) neither 0 nor 2, the
 * whole band (ghost == 0, b0 == 0), 8 <= n <= 512 and level 0's pivots x (12 + 3 rtf) <= budget.  oicc_debug_bcr_join_plan keeps
 * its meaning: with build_inverts < 0 it answers for the levels above level 0 of such a solve.
 * Returns 1 / 0, or OICC_ERR_INVALID_ARG for n < 1 or rtf, budget, b0 out of range. */
int oicc_debug_bcr_level0_plan(int32_t n, int32_t ghost, int32_t odd_only, int32_t b0, int32_t rtf, int32_t join_levels, int32_t budget);
/* Which level's back substitution the solver runs inside the last block's launch -- one workgroup per pivot of the level, each
 * repeating the last block's work and taking its neighbours' solution from LDS -- instead of a launch of its own (the solver's own
 * rule, host arithmetic only).  The back substitution pairs the levels from the bottom up; an even number of levels leaves level
 * nlev - 2 alone.  It is folded when on != 0 (option bcr_fold_back), the solve is the whole band (ghost == 0, b0 == 0) and the plan
 * has an even number of levels >= 2.  Returns that level, -1 when nothing folds, INT32_MIN for n < 1, b0 < 0 or a ghost other than 0 / 1. */
int oicc_debug_bcr_fold_plan(int32_t n, int32_t ghost, int32_t odd_only, int32_t b0, int32_t on);
/* The 16-column panel chain of the 64 x 64 inversions as its events in program order (host arithmetic only; the table the kernels
 * expand): rows of six int32 {type, column, gap, k, c2, aux} -- type 0 pivot read of `column`; 1 strip store of column k = `column`,
 * every lane, the doubles [aux, c2) of the wave's strips; 2 LDS read of the multiplier m(k, c2) at double aux; 3 deferred update
 * av[c2] -= l(k) m(k, c2) issued in gap `gap` of `column`; 4 the v_readlane hop (column, column + 1).  Returns the number of events;
 * rows beyond cap are not written. */
int oicc_debug_bcr_chain_schedule(int32_t* rows, int32_t cap);
/* out3 = [1 if the last whole-band cyclic-reduction solve of the problem folded a level that way, the solves that did so far, option
 * bcr_fold_back].  OICC_ERR_INVALID_ARG for a null argument. */
int oicc_debug_bcr_fold_info(oicc_problem* problem, int64_t out3[3]);

#ifdef __cplusplus
}
#endif
#endif /* OICC_HIP_H_ */
