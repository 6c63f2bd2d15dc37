// Rolling-shutter rectification from gyroscope rates (include/oicc_hip.h, "rolling shutter"; DESIGN.md section 3, "Rolling-shutter
// rectification").  Rotation only: the camera is taken to turn about its centre during the readout; translation (parallax) is
// out of scope, and so are fields of view of 180 degrees and more (rays are (x, y, 1), as in camera_maps.hip).
//
//   rs_frame_table_kernel  one lane per frame: the chain of at most 256 quaternion products over the frame's window of gyro
//                          samples, then (tau_j = t_j - t_ref, Q'_j = Q(t_ref)^-1 Q_j, omega_j) per window sample.  The host has
//                          found the window (first sample, count) by time comparisons, because it needs them for frame_status.
//                          It lives in rolling_shutter_device.h with the fixed point and judge(): stabilization.hip shares them.
//   rs_ray_kernel          one lane per destination pixel: its ray (closed form for a plain PINHOLE, else Newton), once per call.
//   rs_map_kernel          one lane per (frame, pixel), the frame in the grid's y: the workgroup stages its frame's table in LDS
//                          (16 KB), every lane runs the fixed point on its source row; float2 coordinates and a validity byte.
//   rs_rectify_kernel<CH>  the same fixed point, then the bilinear tap of camera_remap_kernel on the float32-rounded coordinates;
//                          no per-frame map reaches memory.
//   rs_points_kernel       forward: an observed pixel of frame k -> source ray -> R_rel(tau(y)) -> destination camera.
//   rs_rotation_kernel     R_rel as a quaternion for (frame, row) queries.
//
// tests/rolling_shutter_restatement.py restates every step in numpy.  Compiled with -ffp-contract=off like camera_maps.o: with
// all rates zero the map is bit-equal to camera_map_kernel's, and the fused frames are byte-equal to remapping through the map.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include "rolling_shutter_device.h"

namespace {

using namespace oicc_camera;
using namespace oicc_rs;       // quaternions, the frame table and its kernel, the fixed point, judge(): shared with stabilization.hip

__global__ __launch_bounds__(kThreads) void rs_ray_kernel(Camera dst, int closed_form, int dst_w, int64_t pixels, double2* __restrict__ rays,
                                                          uint8_t* __restrict__ ray_status) {
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= pixels) return;
  const double u = double(i % dst_w), v = double(i / dst_w);
  double x, y;
  bool ok = true;
  if (closed_form) {
    y = (v - dst.in[4]) / (dst.in[0] * dst.in[1]);
    x = (u - dst.in[3] - dst.in[2] * y) / dst.in[0];
  } else {
    ok = unproject(dst, u, v, x, y);
  }
  rays[i] = make_double2(x, y);
  ray_status[i] = ok ? 0 : 1;
}

// map [frames][pixels], valid [frames][pixels], evaluations [frames][pixels] or null
__global__ __launch_bounds__(kThreads) void rs_map_kernel(RsParams P, int first_frame, const double* __restrict__ table,
                                                          const int32_t* __restrict__ count, const double2* __restrict__ rays,
                                                          const uint8_t* __restrict__ ray_status, int64_t pixels, float2* __restrict__ map,
                                                          uint8_t* __restrict__ valid, uint8_t* __restrict__ evaluations) {
  __shared__ double lds[kMaxWindow * kEntry];
  const int frame = first_frame + blockIdx.y;
  int n;
  const bool have = stage_table(table, count, frame, lds, n);
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= pixels) return;
  double px[2] = {0.0, 0.0};
  int evals = 0;
  bool ok = false;
  if (have) {
    const double2 r = rays[i];
    ok = solve_pixel(P, P.R.r, lds, n, r.x, r.y, ray_status[i] == 0, px, evals);
  }
  const float qnan = __builtin_nanf("");
  const int64_t o = int64_t(frame) * pixels + i;
  map[o] = ok ? make_float2(float(px[0]), float(px[1])) : make_float2(qnan, qnan);
  valid[o] = ok ? 1 : 0;
  if (evaluations) evaluations[o] = uint8_t(evals);
}

// frames / out: the batch's first frame at index 0; table and count are indexed by first_frame + blockIdx.y
template <int CH>
__global__ __launch_bounds__(kThreads) void rs_rectify_kernel(RsParams P, int first_frame, const double* __restrict__ table,
                                                              const int32_t* __restrict__ count, const double2* __restrict__ rays,
                                                              const uint8_t* __restrict__ ray_status, int64_t pixels,
                                                              const uint8_t* __restrict__ frames, int border, uint8_t* __restrict__ out) {
  __shared__ double lds[kMaxWindow * kEntry];
  int n;
  const bool have = stage_table(table, count, first_frame + blockIdx.y, lds, n);
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= pixels) return;
  double px[2] = {0.0, 0.0};
  int evals = 0;
  bool ok = false;
  if (have) {
    const double2 r = rays[i];
    ok = solve_pixel(P, P.R.r, lds, n, r.x, r.y, ray_status[i] == 0, px, evals);
  }
  uint8_t* o = out + (int64_t(blockIdx.y) * pixels + i) * CH;
  BilinearTap<CH> tap;
  if (!ok || !tap.set(make_float2(float(px[0]), float(px[1])), P.src_w, P.src_h)) {
#pragma unroll
    for (int c = 0; c < CH; ++c) o[c] = uint8_t(border);
    return;
  }
  const uint8_t* s = frames + int64_t(blockIdx.y) * P.src_w * P.src_h * CH;
#pragma unroll
  for (int c = 0; c < CH; ++c) o[c] = tap.sample(s, c);
}

// status: 0 a point, 1 none (no ray, z <= 0, a failed projection; NaN), 2 the frame has no table (NaN)
__global__ __launch_bounds__(kThreads) void rs_points_kernel(RsParams P, const double* __restrict__ table, const int32_t* __restrict__ count,
                                                             int64_t n, const int32_t* __restrict__ frame, const double* __restrict__ xy_in,
                                                             double* __restrict__ xy_out, uint8_t* __restrict__ status) {
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= n) return;
  const double2 uv = *reinterpret_cast<const double2*>(xy_in + 2 * i);
  const int k = frame[i];
  const int cnt = count[k];
  double px[2] = {0.0, 0.0};
  int st = cnt < 2 ? 2 : 0;
  if (st == 0) {
    double x, y;
    bool ok = true;
    if (P.src_closed_form) {
      y = (uv.y - P.src.in[4]) / (P.src.in[0] * P.src.in[1]);
      x = (uv.x - P.src.in[3] - P.src.in[2] * y) / P.src.in[0];
      ok = isfinite(x) && isfinite(y);
    } else {
      ok = unproject(P.src, uv.x, uv.y, x, y);
    }
    if (ok) {
      double M[9];
      rotation_matrix(table_rotation(table + int64_t(k) * kMaxWindow * kEntry, cnt, row_tau(P, uv.y)), M);
      const double d0[3] = {(M[0] * x + M[1] * y) + M[2], (M[3] * x + M[4] * y) + M[5], (M[6] * x + M[7] * y) + M[8]};                  // R_rel d
      const double* R = P.R.r;
      const double d[3] = {(R[0] * d0[0] + R[3] * d0[1]) + R[6] * d0[2], (R[1] * d0[0] + R[4] * d0[1]) + R[7] * d0[2], (R[2] * d0[0] + R[5] * d0[1]) + R[8] * d0[2]};   // R9^T
      ok = d[2] > 0.0 && oicc::camera_project<false>(P.dst.model, P.dst.in, d, px, nullptr) && isfinite(px[0]) && isfinite(px[1]);
    }
    if (!ok) st = 1;
  }
  const double qnan = nan("");
  *reinterpret_cast<double2*>(xy_out + 2 * i) = st == 0 ? make_double2(px[0], px[1]) : make_double2(qnan, qnan);
  status[i] = uint8_t(st);
}

// q [n][4] (w, x, y, z) of R_rel at (frame, row); status 0, or 2 where the frame has no table (NaN)
__global__ __launch_bounds__(kThreads) void rs_rotation_kernel(RsParams P, const double* __restrict__ table, const int32_t* __restrict__ count,
                                                               int64_t n, const int32_t* __restrict__ frame, const double* __restrict__ rows,
                                                               double* __restrict__ q, uint8_t* __restrict__ status) {
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= n) return;
  const int k = frame[i];
  const int cnt = count[k];
  const double qnan = nan("");
  Q4 r = {qnan, qnan, qnan, qnan};
  if (cnt >= 2) r = table_rotation(table + int64_t(k) * kMaxWindow * kEntry, cnt, row_tau(P, rows[i]));
  double* o = q + 4 * i;
  o[0] = r.w; o[1] = r.x; o[2] = r.y; o[3] = r.z;
  status[i] = cnt >= 2 ? 0 : 2;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------

// The device side of a scene: the per-frame tables and, where wanted, the destination rays.
// The third stage is the ray kernel; the output drivers of rolling_shutter_device.h launch through map_chunk and frames_chunk.
struct Prepared {
  SceneStage scene;
  oicc::DevBuf<double2> rays;
  oicc::DevBuf<uint8_t> ray_status;

  // Enqueues the uploads, the table kernel and (with_rays) the ray kernel on st; J and the scene arrays must outlive the stream's work.
  int prepare(const oicc_rs_scene* s, const Judged& J, bool with_rays, hipStream_t st) {
    const int64_t pixels = J.pixels();
    if (int rc = scene.allocate(J)) return rc;
    // every allocation before the first copy and event: none sits inside a timed span
    if (with_rays) { OICC_HIP_TRY(rays.resize(size_t(pixels))); OICC_HIP_TRY(ray_status.resize(size_t(pixels))); }
    if (int rc = scene.upload(s, J, st)) return rc;
    if (int rc = scene.launch_tables(J, st)) return rc;
    if (with_rays) {
      hipLaunchKernelGGL(rs_ray_kernel, dim3(blocks_for(pixels)), dim3(kThreads), 0, st, J.P.dst, J.P.dst_closed_form, J.P.dst_w, pixels, rays.p, ray_status.p);
      OICC_HIP_TRY(hipGetLastError());
    }
    OICC_HIP_TRY(hipEventRecord(scene.ev[2], st));
    return OICC_OK;
  }

  void map_chunk(hipStream_t st, const Judged& J, int first, int m, float2* map, uint8_t* valid, uint8_t* evaluations) const {
    hipLaunchKernelGGL(rs_map_kernel, dim3(blocks_for(J.pixels()), unsigned(m)), dim3(kThreads), 0, st, J.P, first, scene.table.p, scene.count.p, rays.p,
                       ray_status.p, J.pixels(), map, valid, evaluations);
  }

  void frames_chunk(hipStream_t st, const Judged& J, int first, int m, int channels, const uint8_t* in, int border, uint8_t* out) const {
    const int64_t pixels = J.pixels();
    const dim3 grid(blocks_for(pixels), unsigned(m));
    if (channels == 1)
      hipLaunchKernelGGL(rs_rectify_kernel<1>, grid, dim3(kThreads), 0, st, J.P, first, scene.table.p, scene.count.p, rays.p, ray_status.p, pixels, in, border, out);
    else
      hipLaunchKernelGGL(rs_rectify_kernel<3>, grid, dim3(kThreads), 0, st, J.P, first, scene.table.p, scene.count.p, rays.p, ray_status.p, pixels, in, border, out);
  }
};

}  // namespace

extern "C" int oicc_rs_rectify_map(int32_t device_ordinal, const oicc_rs_scene* scene, float* map, uint8_t* valid, uint8_t* evaluations,
                                   int32_t* frame_status, int64_t* num_valid, double* device_ms) {
  Judged J;
  if (int rc = judge(scene, &J)) return rc;
  if (!map || !valid || !frame_status) return OICC_ERR_INVALID_ARG;
  Prepared D;
  return run_map(device_ordinal, J, D, [&](hipStream_t st) { return D.prepare(scene, J, true, st); }, map, valid, evaluations, frame_status, num_valid,
                 device_ms);
}

extern "C" int oicc_rs_rectify_frames_device(void* hip_stream, const oicc_rs_scene* scene, int32_t channels, const uint8_t* frames_dev,
                                             int32_t border_value, uint8_t* out_dev, int32_t* frame_status) {
  Judged J;
  if (int rc = judge(scene, &J)) return rc;
  if (!frames_args_ok(channels, border_value) || !frames_dev || !out_dev || !frame_status) return OICC_ERR_INVALID_ARG;
  Prepared D;
  return run_frames_device(static_cast<hipStream_t>(hip_stream), J, D, [&](hipStream_t st) { return D.prepare(scene, J, true, st); }, channels, frames_dev,
                           border_value, out_dev, frame_status);
}

extern "C" int oicc_rs_rectify_frames(int32_t device_ordinal, const oicc_rs_scene* scene, int32_t channels, const uint8_t* frames,
                                      int32_t border_value, int32_t batch, uint8_t* out, int32_t* frame_status, oicc_rs_frames_report* report) {
  Judged J;
  if (int rc = judge(scene, &J)) return rc;
  if (!frames_args_ok(channels, border_value) || batch < 1 || !frames || !out || !frame_status) return OICC_ERR_INVALID_ARG;
  Prepared D;
  return run_frames(device_ordinal, J, D, [&](hipStream_t st) { return D.prepare(scene, J, true, st); }, channels, frames, border_value, batch, out,
                    frame_status, report);
}

namespace {

// points (QUERY 0: xy_in [n][2] -> xy_out [n][2]) and row rotations (QUERY 1: rows [n] -> q [n][4]) share everything but the kernel
template <int QUERY>
int run_queries(int32_t device_ordinal, const oicc_rs_scene* scene, int64_t n, const int32_t* frame_index, const double* in, double* out,
                uint8_t* status, int32_t* frame_status, double* device_ms) {
  constexpr int kIn = QUERY == 0 ? 2 : 1, kOut = QUERY == 0 ? 2 : 4;
  Judged J;
  if (int rc = judge(scene, &J)) return rc;
  if (n < 1 || n > kMaxLanes || !frame_index || !in || !out || !status || !frame_status) return OICC_ERR_INVALID_ARG;
  for (int64_t i = 0; i < n; ++i) if (frame_index[i] < 0 || frame_index[i] >= J.num_frames) return OICC_ERR_INVALID_ARG;
  if (QUERY == 1 && !all_finite(in, n)) return OICC_ERR_INVALID_ARG;
  if (int rc = oicc::select_device(device_ordinal)) return rc;
  Prepared D;
  oicc::DevBuf<int32_t> d_frame; oicc::DevBuf<double> d_in, d_out; oicc::DevBuf<uint8_t> d_st;
  oicc::Event e0, e1;
  oicc::Stream st;
  float ms = 0.0f;
  OICC_HIP_TRY(st.create());
  OICC_HIP_TRY(e0.create()); OICC_HIP_TRY(e1.create());
  if (int rc = D.prepare(scene, J, false, st)) return rc;
  OICC_HIP_TRY(d_frame.resize(size_t(n)));
  OICC_HIP_TRY(d_in.resize(kIn * size_t(n)));
  OICC_HIP_TRY(d_out.resize(kOut * size_t(n)));
  OICC_HIP_TRY(d_st.resize(size_t(n)));
  OICC_HIP_TRY(hipMemcpyAsync(d_frame.p, frame_index, sizeof(int32_t) * size_t(n), hipMemcpyHostToDevice, st));
  OICC_HIP_TRY(hipMemcpyAsync(d_in.p, in, sizeof(double) * kIn * size_t(n), hipMemcpyHostToDevice, st));
  OICC_HIP_TRY(hipEventRecord(e0, st));
  if (QUERY == 0)
    hipLaunchKernelGGL(rs_points_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, st, J.P, D.scene.table.p, D.scene.count.p, n, d_frame.p, d_in.p, d_out.p, d_st.p);
  else
    hipLaunchKernelGGL(rs_rotation_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, st, J.P, D.scene.table.p, D.scene.count.p, n, d_frame.p, d_in.p, d_out.p, d_st.p);
  OICC_HIP_TRY(hipGetLastError());
  OICC_HIP_TRY(hipEventRecord(e1, st));
  OICC_HIP_TRY(hipMemcpyAsync(out, d_out.p, sizeof(double) * kOut * size_t(n), hipMemcpyDeviceToHost, st));
  OICC_HIP_TRY(hipMemcpyAsync(status, d_st.p, size_t(n), hipMemcpyDeviceToHost, st));
  OICC_HIP_TRY(hipStreamSynchronize(st));
  OICC_HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  if (device_ms) *device_ms = double(ms);
  copy_status(J, frame_status);
  return OICC_OK;
}

}  // namespace

extern "C" int oicc_rs_rectify_points(int32_t device_ordinal, const oicc_rs_scene* scene, int64_t n, const int32_t* frame_index,
                                      const double* xy_in, double* xy_out, uint8_t* status, int32_t* frame_status, double* device_ms) {
  return run_queries<0>(device_ordinal, scene, n, frame_index, xy_in, xy_out, status, frame_status, device_ms);
}

extern "C" int oicc_rs_row_rotations(int32_t device_ordinal, const oicc_rs_scene* scene, int64_t n, const int32_t* frame_index,
                                     const double* rows, double* q, uint8_t* status, int32_t* frame_status, double* device_ms) {
  return run_queries<1>(device_ordinal, scene, n, frame_index, rows, q, status, frame_status, device_ms);
}
