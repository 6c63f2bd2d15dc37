// What the rolling-shutter rectification (rolling_shutter.hip) and the stabilisation (stabilization.hip) share: quaternions, the
// exponential of a gyro interval with a linear rate, the per-frame table of relative rotations and its kernel, R_rel at a row, the
// fixed point on the source row, and on the host the judgement of an oicc_rs_scene (its rules by time comparisons live in
// gyro_scene_host.h, which needs no HIP), the scene stage that puts the tables on the device, and the drivers of the three output
// entries each unit has (map, frames on the caller's stream, batched frames).  Both units are compiled with -ffp-contract=off
// (csrc/Makefile): every sum here rounds as tests/rolling_shutter_restatement.py does.  The kernel is static and the host functions
// inline: each unit has its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include "camera_device.h"
#include "gyro_scene_host.h"

namespace oicc_rs {

using namespace oicc_camera;

constexpr int kEntry = 8;                // doubles per table entry: tau, Q' (w x y z), omega (x y z)
constexpr int kMaxEvaluations = 24;
constexpr double kRowTol = 1e-10;
constexpr int kFrameChunk = 32768;       // frames per launch (the grid's y dimension)

struct Q4 { double w, x, y, z; };

__device__ __forceinline__ Q4 qmul(const Q4& a, const Q4& b) {
  return Q4{((a.w * b.w - a.x * b.x) - a.y * b.y) - a.z * b.z, ((a.w * b.x + a.x * b.w) + a.y * b.z) - a.z * b.y,
            ((a.w * b.y - a.x * b.z) + a.y * b.w) + a.z * b.x, ((a.w * b.z + a.x * b.y) - a.y * b.x) + a.z * b.w};
}

// Exp of the rotation vector phi_j(s) = om0 s + (om1 - om0) s^2 / (2 dt): the rate is linear inside a gyro interval
__device__ __forceinline__ Q4 interval_exp(const double* om0, const double* om1, double dt, double s) {
  const double c = s * s / (2.0 * dt);
  const double p0 = om0[0] * s + (om1[0] - om0[0]) * c, p1 = om0[1] * s + (om1[1] - om0[1]) * c, p2 = om0[2] * s + (om1[2] - om0[2]) * c;
  const double th = sqrt((p0 * p0 + p1 * p1) + p2 * p2);
  const double half = th / 2.0;
  const double k = th < 1e-8 ? 0.5 - th * th / 48.0 : sin(half) / th;
  return Q4{cos(half), k * p0, k * p1, k * p2};
}

// R_rel(tau) from a frame's table (LDS or global): the interval j with tau_j <= tau, clipped to the window
__device__ __forceinline__ Q4 table_rotation(const double* tab, int count, double tau) {
  int lo = 0, hi = count - 1;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tab[mid * kEntry] <= tau) lo = mid; else hi = mid;
  }
  const double* e = tab + lo * kEntry;
  const Q4 q = {e[1], e[2], e[3], e[4]};
  return qmul(q, interval_exp(e + 5, e + kEntry + 5, e[kEntry] - e[0], tau - e[0]));
}

__device__ __forceinline__ void rotation_matrix(const Q4& q, double M[9]) {
  M[0] = 1.0 - 2.0 * (q.y * q.y + q.z * q.z); M[1] = 2.0 * (q.x * q.y - q.w * q.z); M[2] = 2.0 * (q.x * q.z + q.w * q.y);
  M[3] = 2.0 * (q.x * q.y + q.w * q.z); M[4] = 1.0 - 2.0 * (q.x * q.x + q.z * q.z); M[5] = 2.0 * (q.y * q.z - q.w * q.x);
  M[6] = 2.0 * (q.x * q.z - q.w * q.y); M[7] = 2.0 * (q.y * q.z + q.w * q.x); M[8] = 1.0 - 2.0 * (q.x * q.x + q.y * q.y);
}

struct RsParams {
  Camera src, dst;
  Rotation R;
  int src_w, src_h, dst_w, dst_h, src_closed_form, dst_closed_form;
  double line_delay, reference_row, time_offset;
};

__device__ __forceinline__ double row_tau(const RsParams& P, double row) {
  return (fmin(fmax(row, 0.0), double(P.src_h - 1)) - P.reference_row) * P.line_delay;
}

// gyro_t / rates: all samples (rates already in the camera frame); first / count: the frame's window.  table [frames][256][8].
static __global__ __launch_bounds__(64) void rs_frame_table_kernel(int num_frames, const double* __restrict__ gyro_t, const double* __restrict__ rates,
                                                                   const double* __restrict__ frame_t, const int64_t* __restrict__ first,
                                                                   const int32_t* __restrict__ count, double time_offset, double reference_delay,
                                                                   double* __restrict__ table) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= num_frames) return;
  const int n = count[k];
  if (n < 2) return;
  const double* t = gyro_t + first[k];
  const double* om = rates + 3 * first[k];
  double* tab = table + int64_t(k) * kMaxWindow * kEntry;
  const double tk = frame_t[k];
  // times as differences first: absolute times reach 1e4 s
  Q4 q = {1.0, 0.0, 0.0, 0.0};
  double tau = ((t[0] - tk) + time_offset) - reference_delay;
  int jr = 0;
  Q4 q_jr = q;
  double tau_jr = tau;
  for (int j = 0; j < n; ++j) {
    double* e = tab + j * kEntry;
    e[0] = tau; e[1] = q.w; e[2] = q.x; e[3] = q.y; e[4] = q.z; e[5] = om[3 * j]; e[6] = om[3 * j + 1]; e[7] = om[3 * j + 2];
    if (j <= n - 2 && (j == 0 || tau <= 0.0)) { jr = j; q_jr = q; tau_jr = tau; }     // the interval of t_ref, clipped to the window
    if (j + 1 < n) {
      const double next = ((t[j + 1] - tk) + time_offset) - reference_delay;
      q = qmul(q, interval_exp(om + 3 * j, om + 3 * j + 3, next - tau, next - tau));
      tau = next;
    }
  }
  const double dt = tab[(jr + 1) * kEntry] - tau_jr;
  const Q4 qref = qmul(q_jr, interval_exp(om + 3 * jr, om + 3 * jr + 3, dt, 0.0 - tau_jr));
  const Q4 inv = {qref.w, -qref.x, -qref.y, -qref.z};
  for (int j = 0; j < n; ++j) {
    double* e = tab + j * kEntry;
    const Q4 r = qmul(inv, Q4{e[1], e[2], e[3], e[4]});
    e[1] = r.w; e[2] = r.x; e[3] = r.y; e[4] = r.z;
  }
}

// The fixed point on the source row of one destination ray (x, y, 1), rotated by R (row-major: P.R of the call, or a frame's own in
// the stabilisation).  tab: the frame's table in LDS.
__device__ __forceinline__ bool solve_pixel(const RsParams& P, const double* R, const double* tab, int count, double x, double y, bool ok, double px[2],
                                            int& evaluations) {
  const double p[3] = {(R[0] * x + R[1] * y) + R[2], (R[3] * x + R[4] * y) + R[5], (R[6] * x + R[7] * y) + R[8]};
  px[0] = 0.0; px[1] = 0.0;
  evaluations = 0;
  ok = ok && p[2] > 0.0;
  if (!ok) return false;
  double row = P.reference_row;
  bool converged = false;
  for (int it = 0; it < kMaxEvaluations; ++it) {
    double M[9];
    rotation_matrix(table_rotation(tab, count, row_tau(P, row)), M);
    const double d[3] = {(M[0] * p[0] + M[3] * p[1]) + M[6] * p[2], (M[1] * p[0] + M[4] * p[1]) + M[7] * p[2], (M[2] * p[0] + M[5] * p[1]) + M[8] * p[2]};   // R_rel^T p
    ++evaluations;
    if (!(d[2] > 0.0) || !oicc::camera_project<false>(P.src.model, P.src.in, d, px, nullptr) || !isfinite(px[0]) || !isfinite(px[1])) return false;
    const double step = fabs(px[1] - row);
    row = px[1];
    if (step <= kRowTol * (1.0 + fabs(row))) { converged = true; break; }
  }
  return converged && px[0] >= 0.0 && px[0] <= double(P.src_w - 1) && px[1] >= 0.0 && px[1] <= double(P.src_h - 1);
}

// stages the table of frame blockIdx.y in LDS; false (for the whole workgroup) when the frame has none
__device__ __forceinline__ bool stage_table(const double* __restrict__ table, const int32_t* __restrict__ count, int frame, double* lds, int& n) {
  n = count[frame];
  if (n < 2) return false;
  const double* src = table + int64_t(frame) * kMaxWindow * kEntry;
  for (int i = threadIdx.x; i < n * kEntry; i += kThreads) lds[i] = src[i];
  __syncthreads();
  return true;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------

// What every entry judges before it looks for a device, and the frame windows, found by time comparisons only.
struct Judged {
  RsParams P;
  int num_frames = 0;
  int64_t num_gyro = 0;
  std::vector<double> rates_cam;       // [n][3]
  std::vector<int64_t> first;          // [frames] first window sample
  std::vector<int32_t> count, status;  // [frames] window samples (0 where status != 0), oicc frame status
  int64_t pixels() const { return int64_t(P.dst_w) * P.dst_h; }      // of the destination
};

inline double reference_delay(const RsParams& P) { return reference_delay(P.reference_row, P.line_delay); }

// the camera construction and the argument checks here; the rates and the windows by gyro_scene_host.h
inline int judge(const oicc_rs_scene* s, Judged* J) {
  if (!s) return OICC_ERR_INVALID_ARG;
  RsParams& P = J->P;
  if (!make_camera(s->src_model, s->src_intr, &P.src) || !make_camera(s->dst_model, s->dst_intr, &P.dst) || s->src_w < 1 || s->src_h < 1 ||
      s->dst_w < 1 || s->dst_h < 1 || int64_t(s->dst_w) * s->dst_h > kMaxLanes) return OICC_ERR_INVALID_ARG;
  P.R = Rotation{{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}};
  if (s->R9) {
    if (!all_finite(s->R9, 9)) return OICC_ERR_INVALID_ARG;
    for (int k = 0; k < 9; ++k) P.R.r[k] = s->R9[k];
  }
  if (s->num_gyro < 2 || !s->gyro_t || !s->gyro_rates || s->num_frames < 1 || !s->frame_t) return OICC_ERR_INVALID_ARG;
  if (!all_finite(s->gyro_t, s->num_gyro) || !all_finite(s->gyro_rates, 3 * s->num_gyro) || !all_finite(s->frame_t, s->num_frames) ||
      !all_finite(s->q_i_c, 4) || !std::isfinite(s->time_offset_imu_to_cam) || !std::isfinite(s->line_delay_s) ||
      !std::isfinite(s->reference_row)) return OICC_ERR_INVALID_ARG;
  for (int64_t j = 1; j < s->num_gyro; ++j) if (!(s->gyro_t[j] > s->gyro_t[j - 1])) return OICC_ERR_INVALID_ARG;
  if (!(std::fabs(quaternion_norm(s->q_i_c) - 1.0) <= 1e-6)) return OICC_ERR_INVALID_ARG;
  P.src_w = s->src_w; P.src_h = s->src_h; P.dst_w = s->dst_w; P.dst_h = s->dst_h;
  P.src_closed_form = is_plain_pinhole(P.src); P.dst_closed_form = is_plain_pinhole(P.dst);
  P.line_delay = s->line_delay_s; P.reference_row = s->reference_row; P.time_offset = s->time_offset_imu_to_cam;
  J->num_frames = s->num_frames; J->num_gyro = s->num_gyro;
  const size_t f = size_t(s->num_frames);
  J->rates_cam.resize(size_t(3 * s->num_gyro)); J->first.resize(f); J->count.resize(f); J->status.resize(f);
  rates_cam(s->num_gyro, s->gyro_rates, s->q_i_c, J->rates_cam.data());
  frame_windows(s->num_gyro, s->gyro_t, s->num_frames, s->frame_t, s->time_offset_imu_to_cam, s->line_delay_s, s->reference_row, s->src_h,
                J->first.data(), J->count.data(), J->status.data());
  return OICC_OK;
}

inline void copy_status(const Judged& J, int32_t* frame_status) { std::memcpy(frame_status, J.status.data(), sizeof(int32_t) * J.status.size()); }

inline bool frames_args_ok(int32_t channels, int32_t border_value) { return (channels == 1 || channels == 3) && border_value >= 0 && border_value <= 255; }

// The device side of a scene that both units share: the gyro samples, the frame windows and the per-frame tables.  allocate() makes
// every allocation; upload() and launch_tables() only queue work.  A unit allocates its own third-stage buffers (rays, or correction,
// zoom and records) between allocate() and upload(): no allocation follows the first asynchronous copy or sits inside a timed span.
struct SceneStage {
  oicc::DevBuf<double> gyro_t, rates, frame_t, table;
  oicc::DevBuf<int64_t> first;
  oicc::DevBuf<int32_t> count;
  oicc::Event ev[3];     // before the table kernel, behind it, behind the unit's third stage (the unit records that one)

  int allocate(const Judged& J) {
    const size_t n = size_t(J.num_gyro), f = size_t(J.num_frames);
    for (auto& e : ev) OICC_HIP_TRY(e.create());
    OICC_HIP_TRY(gyro_t.resize(n)); OICC_HIP_TRY(rates.resize(3 * n)); OICC_HIP_TRY(frame_t.resize(f));
    OICC_HIP_TRY(first.resize(f)); OICC_HIP_TRY(count.resize(f)); OICC_HIP_TRY(table.resize(size_t(kMaxWindow) * kEntry * f));
    return OICC_OK;
  }
  // J and the scene arrays must outlive the stream's work
  int upload(const oicc_rs_scene* s, const Judged& J, hipStream_t st) {
    OICC_HIP_TRY(gyro_t.copy_from(s->gyro_t, size_t(J.num_gyro), st)); OICC_HIP_TRY(rates.copy_from(J.rates_cam, st));
    OICC_HIP_TRY(frame_t.copy_from(s->frame_t, size_t(J.num_frames), st)); OICC_HIP_TRY(first.copy_from(J.first, st)); OICC_HIP_TRY(count.copy_from(J.count, st));
    return OICC_OK;
  }
  int launch_tables(const Judged& J, hipStream_t st) {
    OICC_HIP_TRY(hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(rs_frame_table_kernel, dim3(unsigned((J.num_frames + 63) / 64)), dim3(64), 0, st, J.num_frames, gyro_t.p, rates.p, frame_t.p,
                       first.p, count.p, J.P.time_offset, reference_delay(J.P), table.p);
    OICC_HIP_TRY(hipGetLastError());
    OICC_HIP_TRY(hipEventRecord(ev[1], st));
    return OICC_OK;
  }
};

// ---- the three output entries of a unit, written once ------------------------------------------------------------------------------
// D is the unit's Prepared: a SceneStage `scene`, the unit's third stage, and one launch each for a chunk of frames [first, first + m),
// m <= kFrameChunk: D.map_chunk(st, J, first, m, map, valid, evaluations) on whole-scene arrays [frames][pixels] (evaluations or null) and
// D.frames_chunk(st, J, first, m, channels, in, border, out), in / out starting at frame `first`.  prepare(st) fills D on a stream: the
// unit's allocations, then the uploads, the table kernel and the third stage, scene.ev[0..2] around them.

// frames [first, first + num) of the scene; frames_dev / out_dev start at frame `first`
template <class Prepared>
int launch_frames(hipStream_t st, const Judged& J, const Prepared& D, int first, int num, int channels, const uint8_t* frames_dev, int border,
                  uint8_t* out_dev) {
  const int64_t in_frame = int64_t(J.P.src_w) * J.P.src_h * channels, out_frame = int64_t(J.P.dst_w) * J.P.dst_h * channels;
  for (int done = 0; done < num; done += kFrameChunk) {
    D.frames_chunk(st, J, first + done, std::min(kFrameChunk, num - done), channels, frames_dev + done * in_frame, border, out_dev + done * out_frame);
    if (hipGetLastError() != hipSuccess) return OICC_ERR_HIP;
  }
  return OICC_OK;
}

// the map entry: a stream of its own, declared behind D (the caller's) and the map buffers
template <class Prepared, class Prepare>
int run_map(int32_t device_ordinal, const Judged& J, Prepared& D, Prepare&& prepare, float* map, uint8_t* valid, uint8_t* evaluations,
            int32_t* frame_status, int64_t* num_valid, double* device_ms) {
  if (int rc = oicc::select_device(device_ordinal)) return rc;
  const int64_t pixels = J.pixels();
  const size_t total = size_t(pixels) * size_t(J.num_frames);
  oicc::DevBuf<float2> d_map; oicc::DevBuf<uint8_t> d_valid, d_evals;
  oicc::Event e1;
  oicc::Stream st;
  float ms[3] = {0.0f, 0.0f, 0.0f};
  OICC_HIP_TRY(st.create());
  OICC_HIP_TRY(e1.create());
  OICC_HIP_TRY(d_map.resize(total));
  OICC_HIP_TRY(d_valid.resize(total));
  if (evaluations) OICC_HIP_TRY(d_evals.resize(total));
  if (int rc = prepare(st.s)) return rc;
  for (int first = 0; first < J.num_frames; first += kFrameChunk) {
    D.map_chunk(st, J, first, std::min(kFrameChunk, J.num_frames - first), d_map.p, d_valid.p, d_evals.p);
    OICC_HIP_TRY(hipGetLastError());
  }
  OICC_HIP_TRY(hipEventRecord(e1, st));
  OICC_HIP_TRY(hipMemcpyAsync(map, d_map.p, sizeof(float2) * total, hipMemcpyDeviceToHost, st));
  OICC_HIP_TRY(d_valid.download(valid, total, st));
  if (evaluations) OICC_HIP_TRY(d_evals.download(evaluations, total, st));
  OICC_HIP_TRY(hipStreamSynchronize(st));
  OICC_HIP_TRY(hipEventElapsedTime(&ms[0], D.scene.ev[0], D.scene.ev[1]));
  OICC_HIP_TRY(hipEventElapsedTime(&ms[1], D.scene.ev[1], D.scene.ev[2]));
  OICC_HIP_TRY(hipEventElapsedTime(&ms[2], D.scene.ev[2], e1));
  if (device_ms) for (int k = 0; k < 3; ++k) device_ms[k] = double(ms[k]);
  copy_status(J, frame_status);
  if (num_valid)
    for (int k = 0; k < J.num_frames; ++k) {
      int64_t c = 0;
      for (int64_t i = 0; i < pixels; ++i) c += valid[int64_t(k) * pixels + i];
      num_valid[k] = c;
    }
  return OICC_OK;
}

// the frames entry on the caller's stream: D is this call's own, so it returns once the stream has run the work, and the caller frees D
template <class Prepared, class Prepare>
int run_frames_device(hipStream_t stream, const Judged& J, Prepared& D, Prepare&& prepare, int32_t channels, const uint8_t* frames_dev,
                      int32_t border_value, uint8_t* out_dev, int32_t* frame_status) {
  if (int rc = oicc::on_current_device(stream, {frames_dev, out_dev})) return rc;
  int rc = prepare(stream);
  if (rc == OICC_OK) rc = launch_frames(stream, J, D, 0, J.num_frames, channels, frames_dev, border_value, out_dev);
  if (hipStreamSynchronize(stream) != hipSuccess && rc == OICC_OK) rc = OICC_ERR_HIP;
  if (rc == OICC_OK) copy_status(J, frame_status);
  return rc;
}

// the batched frames entry; report.ms_rays is the unit's third stage
template <class Prepared, class Prepare>
int run_frames(int32_t device_ordinal, const Judged& J, Prepared& D, Prepare&& prepare, int32_t channels, const uint8_t* frames, int32_t border_value,
               int32_t batch, uint8_t* out, int32_t* frame_status, oicc_rs_frames_report* report) {
  if (int rc = oicc::select_device(device_ordinal)) return rc;
  const auto t_start = std::chrono::steady_clock::now();
  oicc_rs_frames_report rep = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  FramePipeline pipe;      // behind D (the caller's): its streams are drained before the tables go
  if (int rc = pipe.open(J.num_frames, batch, int64_t(J.P.src_w) * J.P.src_h * channels, int64_t(J.P.dst_w) * J.P.dst_h * channels)) return rc;
  if (int rc = prepare(pipe.slot[0].st.s)) return rc;
  OICC_HIP_TRY(hipStreamSynchronize(pipe.slot[0].st));      // both streams read what D holds
  float ms = 0.0f;
  OICC_HIP_TRY(hipEventElapsedTime(&ms, D.scene.ev[0], D.scene.ev[1])); rep.ms_table = ms;
  OICC_HIP_TRY(hipEventElapsedTime(&ms, D.scene.ev[1], D.scene.ev[2])); rep.ms_rays = ms;
  const int rc = pipe.run(frames, out, [&](hipStream_t st, int first, int num, const uint8_t* d_in, uint8_t* d_out) {
    return launch_frames(st, J, D, first, num, channels, d_in, border_value, d_out);
  });
  if (rc != OICC_OK) return rc;
  copy_status(J, frame_status);
  rep.ms_upload = pipe.ms_upload; rep.ms_kernel = pipe.ms_kernel; rep.ms_download = pipe.ms_download;
  rep.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
  if (report) *report = rep;
  return OICC_OK;
}

}  // namespace oicc_rs
