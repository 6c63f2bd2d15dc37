// liboicc_hip, host side: the problem state behind the opaque oicc_problem of include/oicc_hip.h and the functions the host
// translation units share (internal; not part of the ABI).
//   oicc_problem.hip    C-ABI entry points, residual / Jacobian pass (eval_pass, asked for by a PassRequest below), Levenberg-Marquardt
//                       drivers (host loop, device-side control), timers, getters
//   oicc_layout.hip     parameter vector, uploads, tangent layout, buffers of the normal equations, prepare()
//   oicc_tiles.hip      time tiles, chains and row formats of the Jacobian pass (tiles.h)
//   oicc_inner.hip      plan and sweep of the inner iterations (inner_plan.h)
//   oicc_exchange.hip   RCCL binding, rank consistency, owner-computes exchange of the normal equations
//   oicc_report.hip     residual report (kernels_report.hip), corner gating
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // types and enums only: the entry points are bound with dlsym at run time
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>
#include <memory>
#include <type_traits>
#include <string>
#include <vector>

#include "../../include/oicc_hip.h"
#include "oicc_device.h"
#include "lm_launch.h"
#include "tiles.h"
#include "inner_plan.h"
#include "line_search.h"
#include "covariance.h"
#include "oicc_options.h"


namespace oicc {
// kernels_trajectory.hip
void launch_trajectory(const EvalCtx& ctx, int64_t n, const int32_t* s_so3, const int32_t* s_r3, const double* u_so3,
                       const double* u_r3, const int32_t* s_gb, const double* u_gb, const int32_t* s_ab, const double* u_ab,
                       double inv_gb_dt, double inv_ab_dt, double* pose7, double* gyro3, double* accel3, double* gb3, double* ab3,
                       hipStream_t st);
int launch_tile_pass(const TileStatic& hS, const TileStatic* dS, const TileDyn& dyn, bool jac, hipStream_t st);
void launch_lds_poison(hipStream_t st);
void launch_point_columns(const EvalCtx& ctx, const ViewData& vd, const uint8_t* view_rs, bool spline_active, hipStream_t st);   // kernels_points.hip
void launch_inner_seg(const double* so3, int n_pairs, double* seg, hipStream_t st);
void launch_inner_set(const InnerArgs* dA, double* xv, const InnerWg* wgs, long long* prof, int n_wgs, int mode, hipStream_t st, bool read_out = false);   // read_out: the instantiations of the debug read-out (InnerArgs::first_eval)
void launch_inner_wave(const InnerArgs* dA, double* xv, int b0, int n_blocks, bool r3_only, hipStream_t st, bool read_out = false);
void launch_inner_shared_eval(const InnerArgs* dA, double* xv, const InnerWg* wgs, int n_wgs, double* partials, int max_parts, hipStream_t st);
void launch_inner_shared_advance(const InnerArgs* dA, double* xv, const int32_t* block_ids, const int32_t* block_parts, int n_blocks, const double* partials, int max_parts, void* states, bool count_iterations, hipStream_t st, bool read_out = false);
size_t inner_lm_state_bytes();
void launch_inner_records(const ViewData& vd, const ImuData& ia, const ImuData& ig, InnerItemRec* rc, InnerItemRec* ra, InnerItemRec* rg, hipStream_t st);
int inner_set_resident_capacity(int n_cu);
void launch_rank_pack(const double* x, int64_t n, const LmState* s, double* pack, hipStream_t st);
void launch_rank_unpack(double* x, int64_t n, LmState* s, const double* pack, hipStream_t st);
void launch_ne_pack_rows(const NormalEq& ne, const TangentLayout& tl, const int32_t* rows, int n_rows, double* buf, hipStream_t st);
void launch_ne_add_rows(const NormalEq& ne, const TangentLayout& tl, const int32_t* rows, int n_rows, const double* buf, hipStream_t st);
void launch_ne_pack_range(const NormalEq& ne, const TangentLayout& tl, int row0, int n_rows, double* buf, hipStream_t st);
void launch_ne_pack_diag_g(const NormalEq& ne, const TangentLayout& tl, int row0, int n_rows, double* buf, hipStream_t st);
void launch_ne_unpack_diag_g(const NormalEq& ne, const TangentLayout& tl, const int32_t* cut, int n, int me, int64_t piece, const double* buf, hipStream_t st);
void launch_ne_unpack_ranges(const NormalEq& ne, const TangentLayout& tl, const int32_t* cut, int n, int me, int64_t piece, const double* buf, hipStream_t st);
void launch_inner_diff_norm(const double* x, const double* xc, const InnerBlock* blocks, int nb, double* step_norm_sq, hipStream_t st);
void launch_lm_retract(const double* x, double* xc, const ParamLayout& pl, const TangentLayout& tl, const SolveBuffers& sb,
                       const NormalEq& ne, double max_ab, double max_gb, hipStream_t st, double alpha = 1.0, int with_model = 1, double* seg_out = nullptr);
void launch_lm_step_slope(const double* g, const SolveBuffers& sb, int P, double* out, hipStream_t st);
void launch_lm_projected_gradient(const double* x, const ParamLayout& pl, const TangentLayout& tl, const NormalEq& ne, double max_ab, double max_gb, LmState* s, hipStream_t st);
// kernels_report.hip
void launch_report_views(const EvalCtx& ctx, const ViewData& vd, const uint8_t* gate, double* e_uv, uint8_t* status, int32_t* n_used,
                         double* sum_sq, double* max_e, hipStream_t st);
void launch_report_imu(const EvalCtx& ctx, const ImuData& id, int kind, double* r3, double* partials, hipStream_t st);
void launch_lm_decide(LmCtl* out, const LmCtl* prev, const LmState* st, int64_t off_cost, hipStream_t stream);   // the trust-region decision on the device (kernels_solve.hip)
}  // namespace oicc


namespace oicc {


constexpr int kN = OICC_SPLINE_N;
constexpr int kNb = OICC_BIAS_SPLINE_N;

struct ImuHost {
  std::vector<int32_t> s_so3, s_r3, s_b;
  std::vector<double> u_so3, u_r3, u_b, mx, my, mz, w;
  size_t size() const { return s_so3.size(); }
};
struct ImuDev { DevBuf<int32_t> s_so3, s_r3, s_b; DevBuf<double> u_so3, u_r3, u_b, mx, my, mz, w; };
struct ImuGroups { std::vector<int32_t> first, count; size_t size() const { return first.size(); } };   // runs of samples with identical knot windows

struct Active { bool tic, ld, g, spline, ab, gb, intr_a, intr_g, pts; };

struct HostLayout {
  std::vector<int32_t> so3, r3, ab, gb;
  int32_t other[5];
  int32_t P, Pb, a, hb;
  std::vector<int32_t> rmap;   // [P] entry map of the retraction inside the solve's last launch (oicc_device.h: RetractReq)
  std::vector<int32_t> pts; int32_t a_pts = 0;   // SplineOptimFlags::POINTS: the last a_pts arrow columns (3 per observed board point, in point order)
};

}  // namespace oicc

using namespace oicc;

struct InnerPlanOptions { int flags; bool gs_unit; bool general_kernel; int resident_wgs; double shared_share; int64_t layout_gen; int wave_blocks = 0; int n_cu = 256; int big_slots = 65536; };   // what the host part of the inner-iteration plan is built from (build_inner_plan_host)

struct oicc_problem {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;
  // spline meta (impl.h:38-51)
  int64_t dt_so3 = 0, dt_r3 = 0, start_ns = 0, end_ns = 0;
  double inv_so3_dt = 0, inv_r3_dt = 0;
  int64_t dt_ab = 0, dt_gb = 0; double inv_ab_dt = 0, inv_gb_dt = 0, max_ab = 1.0, max_gb = 1e-2;
  // host mirror of the parameter vector
  ParamLayout pl{};
  std::vector<double> x;
  bool x_host_dirty = true;       // host mirror newer than device
  bool x_host_dirty_pts = false;  // oicc_set_scene_points since the parameter vector was laid out: `pts` is newer than x's copy
  std::vector<char> so3_in, r3_in, ab_in, gb_in;   // *_knot_in_problem_, impl.h:282-283
  int cam_model = 0, n_intr = 0; double intr[10] = {0};
  std::vector<double> pts;
  // measurements (host SoA)
  int32_t max_corner_pt = -1;
  std::vector<int32_t> corner_view, corner_pt; std::vector<double> cu, cv, cisx, cisy;
  // corner gating (oicc_gate_corners): the 1/sigma every corner was added with next to the effective one above (0 where gated), so
  // that a gate can be lifted and gating never accumulates; permuted wherever cisx is (sort_views_by_time)
  std::vector<double> cisx0, cisy0; std::vector<uint8_t> cgate;
  std::vector<int64_t> view_c0{0}; std::vector<int32_t> view_s_so3, view_s_r3; std::vector<double> view_u_so3, view_u_r3;
  std::vector<uint8_t> view_rs;
  ImuHost acc, gyr;
  ImuGroups acc_groups, gyr_groups;   // (sync_measurements)
  // Everything behind the ABI (layout, tiles, the inner-iteration plan, the creation order of the parameter blocks that breaks Ceres'
  // degree ties) walks the measurements IN TIME ORDER.  Callers may add them in any order -- the reference iterates an unordered
  // map of views, its application fills it in the string order of the corner file's keys -- so a call that arrives out of order
  // raises a flag and sync_groups() sorts the host arrays (stable, by knot window and normalised time) before anything is derived
  // from them; *_orig maps the sorted position back to the position in the caller's order (empty: identity) for the per-block
  // dumps of oicc_evaluate_blocks, whose rows stay in the caller's order.
  bool views_unsorted = false, acc_unsorted = false, gyr_unsorted = false;
  std::vector<int64_t> corner_orig; std::vector<int32_t> acc_orig, gyr_orig;
  std::vector<int32_t> view_orig;   // the same for the accepted views (the per-view figures of the residual report)
  // knot windows of measurements held by OTHER ranks (multi-GPU): only for layout/bandwidth
  std::vector<int32_t> remote_so3, remote_r3;   // pairs; r3 = -1 for gyro
  std::vector<int32_t> remote_owner;            // the rank that holds the remote measurement (-1: not told; owner-computes exchange needs it)
  // owner-computes exchange (oicc_set_shard): owned band-row ranges of all ranks, the rows this rank sends to / receives from every other rank
  int shard_n = 1, shard_rank = 0;
  oicc_exchange_fn exchange = nullptr; void* exchange_user = nullptr;
  struct OwnerPlan { bool valid = false; std::vector<int32_t> cut; std::vector<std::vector<int32_t>> send_rows, recv_rows; std::vector<int32_t> flat, send_off, recv_off; int max_rows = 0;
                     int max_owned = 0;            // rows of the largest owned range: one slot of the gather buffer
                     int64_t agreed_gen = -1; bool agreed = false;   // all ranks agreed (once per layout, through the installed reduction) that every one of them can run the exchange on the same cuts
                     uint32_t hash = 0; } owner;
  DevBuf<int32_t> d_xrows, d_xcut; DevBuf<double> d_xsend, d_xrecv, d_xgather, d_xagree;
  // distributed linear solve (round 6; kernels_bcr.hip launch_bcr_dist_*, oicc_exchange.hip dist_solve): every rank reduces the 64-column
  // blocks of its own range, the ranks' separators are gathered and solved by all, the step is gathered -- the band never travels
  // usable: decided together with the exchange agreement of layout `gen` (owner_exchange_agree) -- never before it
  struct DistSolve { bool usable = false; int64_t gen = -1; BcrDist d; std::vector<int32_t> b0; DevBuf<int32_t> d_b0; DevBuf<double> ws, msg, xg; int64_t solves = 0;
                     bool last_step_gathered = false;   // the last solve left the SAME step, bit for bit, on every rank (the gathered pieces): its retraction needs no broadcast of the candidate
                   } dist;
  bool has_ld_block = false, has_tic_block = false, has_acc = false, has_gyr = false;
  std::vector<uint8_t> pts_seen_global; int64_t pts_seen_meas_gen = -1, meas_gen = 0;   // SplineOptimFlags::POINTS on time shards: which board points ANY rank's views observe (summed once through the reduction, prepare()); meas_gen counts the Add* calls
  bool has_remote_views = false;   // other ranks hold views too: under SplineOptimFlags::POINTS every board point is a variable on every rank (which points they see is not declared)
  bool meas_dirty = true, groups_dirty = true;
  std::thread plan_thread; InnerPlanOptions plan_job{}; bool plan_job_valid = false; double plan_ms[3] = {0, 0, 0};   // the plan's host part on a second thread (start_inner_plan)
  void wait_plan() { if (plan_thread.joinable()) plan_thread.join(); }
  int plan_wanted_flags = -2;   // oicc_optimize -> prepare: build the inner-iteration plan for these flags under the set-up
  OiccOptions opt;   // oicc_options.def
  std::vector<oicc_iteration> trace;
  std::vector<double> inner_set_costs; DevBuf<double> d_dbg_cost;   // option debug_inner_set_costs: per sweep [-1, cost before], then per independent set [blocks, cost behind it] (oicc_get_inner_set_costs)
  oicc_allreduce_fn reduce = nullptr; void* reduce_user = nullptr;
  void* rccl_comm = nullptr;   // ncclComm_t of oicc_rccl_init
  int rccl_nranks = 1;
  oicc_problem* inner_src = nullptr;   // time-sharded ranks: the problem whose measurements (all ranks') the inner-iteration sweeps run over
  // device
  DevBuf<double> d_x, d_xc;
  // segment tables (spline_seg.h) of the SO(3) knot pairs of the two parameter buffers, keyed by the buffer's address (d_x.p and
  // d_xc.p trade places when a step is accepted); valid = computed for the buffer's current contents
  struct SegTable { DevBuf<double> buf; const double* of = nullptr; bool valid = false; } seg_tab[2];
  SegTable* seg_of(const double* xbuf) { for (auto& t : seg_tab) if (t.of == xbuf) return &t; return nullptr; }
  void seg_invalidate(const double* xbuf) { if (SegTable* t = seg_of(xbuf)) t->valid = false; }
  // Tables once per parameter vector pay when the tiles run in several rounds (every tile would recompute its halo pairs and wait
  // 1.2 us for them); on a one-round problem the dependent chain they add to the retraction kernel (+9 us at C2) costs more.
  int n_cu = 256;
  int64_t bcr_joined[4] = {0, 0, 0, 0};   // cyclic-reduction levels that ran as one launch: in the last whole-band solve, in all of them (oicc_debug_bcr_join_info); [2..3]: the same for a level 0 that joined behind a plain build launch, counted apart (oicc_debug_bcr_level0_info)
  int64_t bcr_folded[2] = {0, 0};   // whether the last whole-band cyclic-reduction solve folded a back-substitution level into the last block's launch; solves that did (oicc_debug_bcr_fold_info)
  bool seg_precomputed() const { const int force = int(opt.debug_seg_precompute); return force == 1 || (force == 0 && tp.n_tiles > n_cu); }
  DevBuf<int32_t> d_corner_view, d_corner_pt, d_view_s_so3, d_view_s_r3;
  DevBuf<double> d_cu, d_cv, d_cisx, d_cisy, d_view_u_so3, d_view_u_r3;
  DevBuf<int64_t> d_view_c0; DevBuf<uint8_t> d_view_rs, d_view_rs_all, d_cgate; std::vector<uint8_t> h_view_rs_all;
  DevArena meas_arena, layout_arena, tile_arena, plan_arena;   // one device block + one copy per group of arrays
  ImuDev d_acc, d_gyr;
  DevBuf<int32_t> d_tl_so3, d_tl_r3, d_tl_ab, d_tl_gb, d_tl_pts, d_tl_rmap;
  DevBuf<double> d_ws;
  DevBuf<double> d_rank_pack;   // all-reduce hook path: [candidate | step scalars | rank count] (make_rank_consistent)
  DevBuf<double> d_ne2;   // second normal-equation buffer: the Jacobian pass at the candidate runs while the host decides
  DevBuf<double> d_ne, d_Mb, d_Mt, d_Mc, d_scale, d_diag, d_D2, d_step, d_dbg_res, d_dbg_jac, d_traj;
  DevBuf<int32_t> d_traj_i;
  DevBuf<LmState> d_state; DevBuf<double> d_ls; int64_t line_search_steps = 0;   // d_ls: slope and max norm of the step (bounds line search)
  // device-side LM control (oicc_device.h: LmCtl): the control block, the iteration records and kernel time stamps it fills, and the
  // pinned word the decision kernel writes for the host (polled one iteration behind; no copy, no event in the loop)
  DevBuf<LmCtl> d_ctl; DevBuf<LmIterRec> d_trace; DevBuf<long long> d_stamps; LmHostMsg* hmsg = nullptr; LmHostMsg* hmsg_dev = nullptr; double wall_clock_hz = 1e8;
  struct HostPin { LmState st; double cost; double radius; double ls[2]; unsigned int inner_words[32]; };   // inner_words: command words of a set's large shared blocks (inner_sweep)
  HostPin* pin = nullptr;   // pinned: one read-back (state + candidate cost) and one 8-byte write per LM iteration
  hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // time tiles of the Jacobian pass (tiles.h): work lists, row formats, slabs
  std::vector<TileDesc> h_tiles; std::vector<UnitDesc> h_units; std::vector<int32_t> h_tile_rows, h_merge_rows; std::vector<uint8_t> h_row_direct;
  DevBuf<int32_t> d_merge_rows, d_merge_ptr; DevBuf<int64_t> d_merge_src, d_merge_tab; DevBuf<uint8_t> d_row_direct; std::vector<int32_t> h_merge_ptr; std::vector<int64_t> h_merge_src, h_merge_tab;
  DevBuf<TileDesc> d_tiles; DevBuf<UnitDesc> d_units; DevBuf<int32_t> d_tile_rows; DevBuf<double> d_slabs;
  RowFmt fv{}, fa{}, fg{}; TileParams tp{}; int tile_T = 0;   // tile_T: knot windows per tile as chosen by the host part of the tiles
  std::unique_ptr<TileStatic> h_tstatic; DevBuf<TileStatic> d_tstatic; bool tstatic_valid = false;   // problem-constant kernel arguments in device memory
  // inner iterations (inner_plan.h): blocks in processing order, independent sets, item -> block maps per set
  struct InnerPlan {
    std::vector<InnerBlock> blocks; std::vector<int32_t> group_first; std::vector<InnerRun> runs; std::vector<InnerWg> wgs; std::vector<int32_t> group_wg0; std::vector<char> group_r3only;   // set g holds nothing but R^3 knots of at most 1024 item slots: the 8-wave build of the kernel   // workgroups of set g: wgs[group_wg0[g] .. group_wg0[g + 1])
    DevBuf<InnerBlock> d_blocks; DevBuf<InnerRun> d_runs; DevBuf<InnerWg> d_wgs; DevBuf<InnerCtl> d_ctls; DevBuf<unsigned long long> d_lm_iterations; DevBuf<double> d_seg; int n_ctls = 0;
    // shared blocks above a size threshold run as a SEQUENCE of launches (inner_shared_eval_kernel / inner_shared_advance_kernel): their parts
    // (as many as there is work: no residency limit), the blocks and their part counts per set, the partial-sum rows, the loops' states
    std::vector<InnerWg> big_wgs; std::vector<int32_t> group_bigwg0, big_blocks, big_parts, group_bigb0; int big_max_parts = 1;
    DevBuf<InnerWg> d_big_wgs; DevBuf<int32_t> d_big_blocks, d_big_parts; DevBuf<double> d_partials; DevBuf<unsigned char> d_lm_states;
    std::vector<char> group_wave;   // set g runs on the wave-per-block kernel (inner_wave_kernel: knot blocks whose neighbourhood fits the LDS copy, enough of them to fill the device)
    bool has_points = false;        // the plan holds board-point blocks (SplineOptimFlags::POINTS): the general build with the point path
    DevBuf<InnerItemRec> d_rec[3];  // per-item records of the wave-per-block kernel (corners, accelerometer, gyroscope samples)
    DevBuf<InnerArgs> d_args; std::unique_ptr<InnerArgs> h_args; bool args_valid = false;   // problem-constant kernel arguments in device memory (inner_plan.h)
    // owner-computes sweeps on time-sharded ranks (round 5): this rank's workgroups of every set (the knot blocks whose rows it owns +
    // the blocks every rank minimises redundantly), what a set changes (bit 0 SO(3) knots, 1 R^3 knots, 2 replicated blocks), and
    // the knot ranges every rank owns ([n + 1] boundaries per spline)
    struct RankPart { std::vector<InnerWg> wgs; std::vector<int32_t> group_wg0; std::vector<uint8_t> group_kinds; std::vector<int32_t> so3_lo, so3_hi, r3_lo, r3_hi;
                      DevBuf<InnerWg> d_wgs; uint64_t key = 0; bool valid = false; } rank_part;
    int flags = -2; int64_t layout_gen = -1; bool gs_unit = false;   // what the plan was built from: the tangent layout (make_layout generation) and the GS weighting
    size_t n_items = 0; int64_t lm_iterations = 0; int sweeps = 0;
  } inner;
  // cached layout
  // layout_flags = -1 invalidates (measurements, knot counts, line delay set by the caller); otherwise the layout and the tiles are
  // rebuilt only when the flags, the zero-ness of the line delay (active_set) or an option changed since they were built
  int layout_flags = -1; bool layout_ld_zero = false; int64_t opt_gen = 0, layout_opt_gen = -1, layout_gen = 0;
  // covariance estimate (oicc_covariance.hip): device buffers of the selected inverse and the host copy the getters hand out;
  // valid = made at the current parameters, measurements and options (every setter and oicc_optimize clear it)
  struct Cov { bool valid = false; int flags = 0; int P = 0, Pb = 0, a = 0; oicc_covariance_info info{};
               std::vector<int32_t> so3, r3;                 // first band column of every knot, -1 outside the active set
               std::vector<double> arrow, cov3, cross;       // [a][a], [Pb][3], [Pb][a]
               DevBuf<double> d_s, d_Cs, d_Sc, d_Zaa, d_aa, d_zb, d_G, d_cov3, d_cross, d_zs; DevBuf<int32_t> d_flags;
               double ms[4] = {0, 0, 0, 0};                  // device time of the last estimate: build, forward factor, corner, backward sweep + finish
             } cov;
  // residual report (oicc_report.hip): host copies in the layout's (time sorted) order, the getters hand them out in the caller's;
  // valid = made at the current parameters and measurements (invalidate_estimates)
  struct Report { bool valid = false;
                  std::vector<double> e_uv, view_sum, view_max; std::vector<uint8_t> status; std::vector<int32_t> view_n;
                  size_t n_acc = 0, n_gyr = 0;                  // samples behind d_acc_r / d_gyr_r (read back by oicc_get_imu_residuals)
                  DevBuf<double> d_e, d_vsum, d_vmax, d_acc_r, d_gyr_r, d_part; DevBuf<uint8_t> d_status; DevBuf<int32_t> d_vn;
                } report;
  void invalidate_estimates() { cov.valid = false; report.valid = false; }   // parameters, measurements or options changed: what was derived from them is stale
  HostLayout L; TangentLayout tl{}; TangentLayout tl_tiles{}; NormalEq ne{}; NormalEq ne2{};   // tl_tiles: tl without the point columns (SplineOptimFlags::POINTS), what the tile pass sees
  Active act{};
};

#define HIPCK(p, call)                                                                 \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess) {                                                            \
      (p)->err = std::string(#call) + ": " + hipGetErrorString(e_);                    \
      return OICC_ERR_HIP;                                                             \
    }                                                                                  \
  } while (0)
#define ARG(p, c, msg) do { if (!(c)) { (p)->err = msg; return OICC_ERR_INVALID_ARG; } } while (0)


namespace oicc {
// ---- shared host functions (defined in the translation units listed above) ----
double now_s();
bool calc_times(int64_t sensor_time, int64_t start_ns, int64_t dt_ns, size_t nr_knots, int N, double* u, int64_t* s);
double* xs(oicc_problem* p, int64_t off);
void rebuild_param_layout(oicc_problem* p, int64_t n_so3, int64_t n_r3, int64_t n_ab, int64_t n_gb);
int sync_params_to_device(oicc_problem* p);
int sync_params_to_host(oicc_problem* p);
void build_imu_groups(const ImuHost& h, bool accel, ImuGroups& g);
int sync_measurements(oicc_problem* p);
void sync_groups(oicc_problem* p);
Active active_set(const oicc_problem* p, int flags);
void build_owner_plan(oicc_problem* p);
void make_layout_host(oicc_problem* p, int flags);
void layout_scalars(oicc_problem* p);
int make_layout_device(oicc_problem* p, int flags, std::thread* tiles_thread = nullptr, int* tiles_rc = nullptr);
int build_tiles_host(oicc_problem* p);
int build_tiles_device(oicc_problem* p);
int prepare(oicc_problem* p, int flags);
EvalCtx make_ctx(oicc_problem* p, const double* x);
ViewData view_data(oicc_problem* p, bool force_rs = false);
ImuData imu_data(const ImuHost& h, const ImuDev& d);
void build_inner_plan_host(oicc_problem* p, const InnerPlanOptions& o, double t_ms[3]);
InnerPlanOptions inner_plan_options(oicc_problem* p, int flags, int64_t layout_gen);
void start_inner_plan(oicc_problem* p, int flags, int64_t layout_gen);
int build_inner_plan(oicc_problem* p, int flags);
// debug read-out of every block's first evaluation (oicc_debug_inner_first_evaluations): the sweep's own launches with InnerArgs::first_eval /
// stop_first set, on scratch segment tables, control blocks and arguments, without the sweep and LM-iteration counters
struct InnerFirstEval { double* rows; double* seg; InnerCtl* ctls; InnerArgs* d_args; };
int inner_sweep(oicc_problem* p, double* xv, hipStream_t st, oicc_problem* shard = nullptr, bool* owner_computes = nullptr, const InnerFirstEval* fe = nullptr);
// What one residual / Jacobian / cost pass is asked to do (eval_pass).  Everything but x has a default; the makers below fill the common shapes.
struct PassRequest {
  const double* x = nullptr;          // parameter buffer (device)
  bool jac = false;                   // Jacobian pass (normal equations, gradient and cost) or cost pass
  const NormalEq* target = nullptr;   // where the pass accumulates (nullptr: the problem's current system, p->ne)
  double* cost_out = nullptr;         // cost passes: device address the cost is added to instead of the target's cost slot
  bool cost_already_zero = false;     // cost passes: that address was cleared by an earlier launch
  const LmCtl* ctl = nullptr;         // device-side LM control: the pass runs at the control block's candidate into its second buffer
  double* dbg_res = nullptr; double* dbg_jac = nullptr;   // dumps of the residuals / Jacobian rows of the blocks ...
  int only_kind = -1;                 // ... of this residual family alone (0 views, 1 accelerometer, 2 gyroscope; -1: all)
  bool force_rs = false;              // every view through the rolling-shutter functor
  long long* prof = nullptr;          // cycle counters of the tile kernel
  LmState* gmax_into = nullptr;       // Jacobian passes: max |g| is wanted in this slot; the slab merge leaves it there where the gradient is final then
  bool* gmax_folded = nullptr;        // out: it did (else the caller launches lm_gradmax / the projected norm)
  bool local = false;                 // no exchange across ranks: this rank's sums only
  bool full_system = false;           // time shards: the exchange leaves the WHOLE system on every rank (the gathered band) even where they agreed on the distributed solve
};
inline PassRequest jacobian_pass(const double* x, const NormalEq* target = nullptr) { PassRequest rq; rq.x = x; rq.jac = true; rq.target = target; return rq; }
inline PassRequest cost_pass(const double* x, double* cost_out = nullptr) { PassRequest rq; rq.x = x; rq.cost_out = cost_out; rq.cost_already_zero = cost_out != nullptr; return rq; }   // (a cost_out is cleared by its owner)
inline PassRequest local_pass(const double* x, bool jac, int only_kind = -1) { PassRequest rq; rq.x = x; rq.jac = jac; rq.only_kind = only_kind; rq.local = true; return rq; }
int eval_pass(oicc_problem* p, const PassRequest& rq);
// events of one entry point, destroyed on every exit
struct EventPair { hipEvent_t a = nullptr, b = nullptr; ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } };
SolveBuffers solve_buffers(oicc_problem* p, long long* prof = nullptr);
// the retraction d_x -> d_xc a solve may do inside its last launch (oicc_device.h: RetractReq); off (on = 0) with option
// fused_retract = 0 and for problems whose retraction also writes the candidate's segment tables (multi-round problems keep the separate launch)
RetractReq retract_request(oicc_problem* p);
// solve + retraction of the trust-region candidate d_x -> d_xc: fused where the route allows, else lm_retract_kernel behind the solve
// (local: the single-rank solve even on agreed shards)
int lm_solve_and_retract(oicc_problem* p, const SolveBuffers& sb, double radius, int reuse_diagonal, double min_diag, double max_diag, hipStream_t st, bool* fused_out = nullptr, bool local = false);
// the opening of the solve entries and debug read-outs: Jacobian pass `rq` at the current point, column scaling into `scale`, LmState zero but for `radius`
int system_at_current_point(oicc_problem* p, const PassRequest& rq, double* scale, bool jacobi_scaling, double radius);
// ||M delta - rhs|| / ||rhs||, ||rhs|| (may be NULL) and the Cholesky failure flag of the solve just run on `sb`
int read_solve_residual(oicc_problem* p, const SolveBuffers& sb, double* relative, double* rhs_norm, double* chol_failed);
int read_cost(oicc_problem* p, double* cost);
void rccl_release(oicc_problem* p);   // destroys the problem's communicator, if any
int rccl_reduce_in_place(void* user, void* device_ptr, int64_t count, void* stream);
int rccl_broadcast_from_root(oicc_problem* p, void* device_ptr, int64_t count_doubles, hipStream_t stream);
int make_rank_consistent(oicc_problem* p, double* xv, bool with_state, hipStream_t st, bool x_identical = false);
bool owner_exchange_ready(const oicc_problem* p);
int owner_exchange_agree(oicc_problem* p, hipStream_t st, bool* use);   // collective (every rank of a sharded problem calls it at the same point)
int shard_broadcast_begin(oicc_problem* p);                                                      // pieces of the parameter vector from their owners, in place:
int shard_broadcast(oicc_problem* p, double* ptr, int64_t count, int root, hipStream_t st);      // native RCCL (one group) or the transport hook
int shard_broadcast_end(oicc_problem* p);
int owner_exchange(oicc_problem* p, const NormalEq& ne, hipStream_t st, bool full_system, int64_t* bytes_moved = nullptr);   // full_system: the gathered band even where the ranks agreed on the distributed solve
bool dist_solve_usable(const oicc_problem* p);   // (decided by the exchange agreement of the current layout: every rank answers alike; false before it)
int dist_solve(oicc_problem* p, const NormalEq& ne, const SolveBuffers& sb, double radius, int reuse_diagonal, double min_diag, double max_diag, hipStream_t st);
int lm_solve_any(oicc_problem* p, const NormalEq& ne, const SolveBuffers& sb, double radius, int reuse_diagonal, double min_diag, double max_diag, hipStream_t st, const RetractReq* retract = nullptr, bool* fused = nullptr, bool local = false);   // the distributed solve on agreed shards (unless local), else launch_lm_solve
}  // namespace oicc
