// Camera maps: pixel -> ray for the six camera models, rectification maps, the discrepancy between two models and bilinear
// resampling of u8 frames (include/oicc_hip.h, "camera maps"; DESIGN.md section 3, "Camera maps").
//
//   unproject    one lane per pixel: Newton on camera_project<true>(x, y, 1) = uv with columns 0 and 1 of the analytic 2 x 3
//                Jacobian, Cramer's rule, pinhole start.  A solution counts only on the principal branch: det A > 0 and
//                A00 / f + A11 / (f aspect) > 0 (beyond the fold of a folding camera Newton converges onto rays that reproject
//                exactly).
//   map          one lane per destination pixel: unproject (destination camera), rotate, project (source camera); float2
//                coordinates and one validity byte.
//   discrepancy  one lane per pixel, unproject through A, project through B; per wave one xor butterfly over (count, sum d^2,
//                max d), one row per wave, added by the host in order.
//   remap        one lane per destination pixel: the map entry and the four weights once, then all frames of the batch and all
//                channels.
//
// Limitations: rays are (x, y, 1), so fields of view of 180 degrees and more are out of scope; a model whose radial map folds
// twice can still offer a second branch on which both signs of the branch test are positive.
//
// tests/camera_maps_restatement.py restates every step in numpy.  This unit is compiled with -ffp-contract=off
// (csrc/Makefile): without fused multiply-adds the bilinear sum rounds as the restatement's and the u8 results agree byte
// for byte.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include "camera_device.h"

namespace {

using namespace oicc_camera;   // Camera, unproject and the bilinear tap: shared with rolling_shutter.hip

__global__ __launch_bounds__(kThreads) void camera_unproject_kernel(Camera cam, int64_t n, const double* __restrict__ uv,
                                                                    double* __restrict__ xy, uint8_t* __restrict__ status) {
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= n) return;
  const double2 p = *reinterpret_cast<const double2*>(uv + 2 * i);
  double x, y;
  const bool ok = unproject(cam, p.x, p.y, x, y);
  *reinterpret_cast<double2*>(xy + 2 * i) = make_double2(x, y);
  status[i] = ok ? 0 : 1;
}

__global__ __launch_bounds__(kThreads) void camera_map_kernel(Camera src, int src_w, int src_h, Camera dst, int closed_form, int dst_w,
                                                              int dst_h, Rotation R, float2* __restrict__ map,
                                                              uint8_t* __restrict__ valid) {
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= int64_t(dst_w) * dst_h) return;
  const double u = double(i % dst_w), v = double(i / dst_w);
  double x, y;
  bool ok = true;
  if (closed_form) {
    y = (v - dst.in[4]) / (dst.in[0] * dst.in[1]);
    x = (u - dst.in[3] - dst.in[2] * y) / dst.in[0];
  } else {
    ok = unproject(dst, u, v, x, y);
  }
  const double p[3] = {(R.r[0] * x + R.r[1] * y) + R.r[2], (R.r[3] * x + R.r[4] * y) + R.r[5], (R.r[6] * x + R.r[7] * y) + R.r[8]};
  double px[2] = {0.0, 0.0};
  ok = ok && p[2] > 0.0;
  if (ok) ok = oicc::camera_project<false>(src.model, src.in, p, px, nullptr);
  ok = ok && px[0] >= 0.0 && px[0] <= double(src_w - 1) && px[1] >= 0.0 && px[1] <= double(src_h - 1);
  const float qnan = __builtin_nanf("");
  map[i] = ok ? make_float2(float(px[0]), float(px[1])) : make_float2(qnan, qnan);
  valid[i] = ok ? 1 : 0;
}

// rows [waves][3] = count, sum d^2, max d of the wave's pixels, every lane of a wave holding the same values after the butterfly
__global__ __launch_bounds__(kThreads) void camera_discrepancy_kernel(Camera a, Camera b, int w, int h, double* __restrict__ rows) {
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  double cnt = 0.0, sum = 0.0, mx = 0.0;
  if (i < int64_t(w) * h) {
    const double u = double(i % w), v = double(i / w);
    double x, y;
    if (unproject(a, u, v, x, y)) {
      const double p[3] = {x, y, 1.0};
      double px[2];
      if (oicc::camera_project<false>(b.model, b.in, p, px, nullptr)) {
        const double ex = px[0] - u, ey = px[1] - v;
        const double d2 = ex * ex + ey * ey;
        if (isfinite(d2)) { cnt = 1.0; sum = d2; mx = sqrt(d2); }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    sum += __shfl_xor(sum, o, 64);
    mx = fmax(mx, __shfl_xor(mx, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    double* row = rows + 3 * (int64_t(blockIdx.x) * kWaves + (threadIdx.x >> 6));
    row[0] = cnt; row[1] = sum; row[2] = mx;
  }
}

template <int CH>
__global__ __launch_bounds__(kThreads) void camera_remap_kernel(const uint8_t* __restrict__ frames, int num_frames, int src_w, int src_h,
                                                                const float2* __restrict__ map, int64_t dst_pixels, int border,
                                                                uint8_t* __restrict__ out) {
  const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= dst_pixels) return;
  BilinearTap<CH> tap;
  const int64_t src_frame = int64_t(src_w) * src_h * CH, dst_frame = dst_pixels * CH;
  uint8_t* o = out + i * CH;
  if (!tap.set(map[i], src_w, src_h)) {
    for (int f = 0; f < num_frames; ++f, o += dst_frame)
#pragma unroll
      for (int c = 0; c < CH; ++c) o[c] = uint8_t(border);
    return;
  }
  const uint8_t* s = frames;
  for (int f = 0; f < num_frames; ++f, s += src_frame, o += dst_frame) {
#pragma unroll
    for (int c = 0; c < CH; ++c) o[c] = tap.sample(s, c);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------

bool remap_args_ok(int32_t num_frames, int32_t src_w, int32_t src_h, int32_t channels, int32_t dst_w, int32_t dst_h, int32_t border_value) {
  return num_frames >= 1 && src_w >= 1 && src_h >= 1 && dst_w >= 1 && dst_h >= 1 && (channels == 1 || channels == 3) &&
         border_value >= 0 && border_value <= 255 && int64_t(dst_w) * dst_h <= kMaxLanes;
}

int launch_remap(hipStream_t st, int num_frames, int src_w, int src_h, int channels, const uint8_t* frames, const float* map, int dst_w,
                 int dst_h, int border, uint8_t* out) {
  const int64_t pixels = int64_t(dst_w) * dst_h;
  const float2* m = reinterpret_cast<const float2*>(map);
  if (channels == 1)
    hipLaunchKernelGGL(camera_remap_kernel<1>, dim3(blocks_for(pixels)), dim3(kThreads), 0, st, frames, num_frames, src_w, src_h, m, pixels, border, out);
  else
    hipLaunchKernelGGL(camera_remap_kernel<3>, dim3(blocks_for(pixels)), dim3(kThreads), 0, st, frames, num_frames, src_w, src_h, m, pixels, border, out);
  return hipGetLastError() == hipSuccess ? OICC_OK : OICC_ERR_HIP;
}

}  // namespace

extern "C" int oicc_camera_unproject(int32_t device_ordinal, int32_t model, const double* intrinsics, int32_t n_intr, int64_t n,
                                     const double* uv, double* xy, uint8_t* status, double* device_ms) {
  Camera cam;
  if (n_intr != intrinsics_count(model) || !make_camera(model, intrinsics, &cam) || n < 1 || n > kMaxLanes || !uv || !xy || !status) return OICC_ERR_INVALID_ARG;
  if (int rc = oicc::select_device(device_ordinal)) return rc;
  oicc::DevBuf<double> d_uv, d_xy; oicc::DevBuf<uint8_t> d_st;
  oicc::Event e0, e1;
  oicc::Stream st;
  float ms = 0.0f;
  OICC_HIP_TRY(st.create());
  OICC_HIP_TRY(e0.create()); OICC_HIP_TRY(e1.create());
  OICC_HIP_TRY(d_uv.resize(2 * size_t(n)));
  OICC_HIP_TRY(d_xy.resize(2 * size_t(n)));
  OICC_HIP_TRY(d_st.resize(size_t(n)));
  OICC_HIP_TRY(hipMemcpyAsync(d_uv.p, uv, sizeof(double) * 2 * size_t(n), hipMemcpyHostToDevice, st));
  OICC_HIP_TRY(hipEventRecord(e0, st));
  hipLaunchKernelGGL(camera_unproject_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, st, cam, n, d_uv.p, d_xy.p, d_st.p);
  OICC_HIP_TRY(hipGetLastError());
  OICC_HIP_TRY(hipEventRecord(e1, st));
  OICC_HIP_TRY(hipMemcpyAsync(xy, d_xy.p, sizeof(double) * 2 * size_t(n), hipMemcpyDeviceToHost, st));
  OICC_HIP_TRY(hipMemcpyAsync(status, d_st.p, size_t(n), hipMemcpyDeviceToHost, st));
  OICC_HIP_TRY(hipStreamSynchronize(st));
  OICC_HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  if (device_ms) *device_ms = double(ms);
  return OICC_OK;
}

extern "C" int oicc_camera_rectify_map(int32_t device_ordinal, int32_t src_model, const double* src_intr, int32_t src_w, int32_t src_h,
                                       int32_t dst_model, const double* dst_intr, int32_t dst_w, int32_t dst_h, const double* R9,
                                       float* map, uint8_t* valid, int64_t* num_valid, double* device_ms) {
  Camera src, dst;
  if (!make_camera(src_model, src_intr, &src) || !make_camera(dst_model, dst_intr, &dst) || src_w < 1 || src_h < 1 || dst_w < 1 ||
      dst_h < 1 || int64_t(dst_w) * dst_h > kMaxLanes || !map || !valid) return OICC_ERR_INVALID_ARG;
  Rotation R = {{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}};
  if (R9)
    for (int k = 0; k < 9; ++k) {
      if (!std::isfinite(R9[k])) return OICC_ERR_INVALID_ARG;
      R.r[k] = R9[k];
    }
  if (int rc = oicc::select_device(device_ordinal)) return rc;
  const int closed_form = is_plain_pinhole(dst);
  const int64_t pixels = int64_t(dst_w) * dst_h;
  oicc::DevBuf<float2> d_map; oicc::DevBuf<uint8_t> d_valid;
  oicc::Event e0, e1;
  oicc::Stream st;
  float ms = 0.0f;
  OICC_HIP_TRY(st.create());
  OICC_HIP_TRY(e0.create()); OICC_HIP_TRY(e1.create());
  OICC_HIP_TRY(d_map.resize(size_t(pixels)));
  OICC_HIP_TRY(d_valid.resize(size_t(pixels)));
  OICC_HIP_TRY(hipEventRecord(e0, st));
  hipLaunchKernelGGL(camera_map_kernel, dim3(blocks_for(pixels)), dim3(kThreads), 0, st, src, int(src_w), int(src_h), dst, closed_form,
                     int(dst_w), int(dst_h), R, d_map.p, d_valid.p);
  OICC_HIP_TRY(hipGetLastError());
  OICC_HIP_TRY(hipEventRecord(e1, st));
  OICC_HIP_TRY(hipMemcpyAsync(map, d_map.p, sizeof(float2) * size_t(pixels), hipMemcpyDeviceToHost, st));
  OICC_HIP_TRY(hipMemcpyAsync(valid, d_valid.p, size_t(pixels), hipMemcpyDeviceToHost, st));
  OICC_HIP_TRY(hipStreamSynchronize(st));
  OICC_HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  if (device_ms) *device_ms = double(ms);
  if (num_valid) {
    int64_t c = 0;
    for (int64_t i = 0; i < pixels; ++i) c += valid[i];
    *num_valid = c;
  }
  return OICC_OK;
}

extern "C" int oicc_camera_discrepancy(int32_t device_ordinal, int32_t model_a, const double* intr_a, int32_t model_b,
                                       const double* intr_b, int32_t w, int32_t h, double stats[3], double* device_ms) {
  Camera a, b;
  if (!make_camera(model_a, intr_a, &a) || !make_camera(model_b, intr_b, &b) || w < 1 || h < 1 || int64_t(w) * h > kMaxLanes || !stats) return OICC_ERR_INVALID_ARG;
  if (int rc = oicc::select_device(device_ordinal)) return rc;
  const int64_t pixels = int64_t(w) * h;
  const unsigned blocks = blocks_for(pixels);
  std::vector<double> rows(size_t(blocks) * kWaves * 3);
  oicc::DevBuf<double> d_rows;
  oicc::Event e0, e1;
  oicc::Stream st;
  float ms = 0.0f;
  OICC_HIP_TRY(st.create());
  OICC_HIP_TRY(e0.create()); OICC_HIP_TRY(e1.create());
  OICC_HIP_TRY(d_rows.resize(rows.size()));
  OICC_HIP_TRY(hipEventRecord(e0, st));
  hipLaunchKernelGGL(camera_discrepancy_kernel, dim3(blocks), dim3(kThreads), 0, st, a, b, int(w), int(h), d_rows.p);
  OICC_HIP_TRY(hipGetLastError());
  OICC_HIP_TRY(hipEventRecord(e1, st));
  OICC_HIP_TRY(hipMemcpyAsync(rows.data(), d_rows.p, sizeof(double) * rows.size(), hipMemcpyDeviceToHost, st));
  OICC_HIP_TRY(hipStreamSynchronize(st));
  OICC_HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  if (device_ms) *device_ms = double(ms);
  double cnt = 0.0, sum = 0.0, mx = 0.0;
  for (size_t r = 0; r < rows.size() / 3; ++r) { cnt += rows[3 * r]; sum += rows[3 * r + 1]; mx = std::max(mx, rows[3 * r + 2]); }
  stats[0] = cnt; stats[1] = cnt > 0.0 ? std::sqrt(sum / cnt) : 0.0; stats[2] = mx;
  return OICC_OK;
}

extern "C" int oicc_camera_remap_device(void* hip_stream, int32_t num_frames, int32_t src_w, int32_t src_h, int32_t channels,
                                        const uint8_t* frames_dev, const float* map_dev, int32_t dst_w, int32_t dst_h,
                                        int32_t border_value, uint8_t* out_dev) {
  if (!remap_args_ok(num_frames, src_w, src_h, channels, dst_w, dst_h, border_value) || !frames_dev || !map_dev || !out_dev)
    return OICC_ERR_INVALID_ARG;
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (int rc = oicc::on_current_device(stream, {frames_dev, map_dev, out_dev})) return rc;
  return launch_remap(stream, num_frames, src_w, src_h, channels, frames_dev, map_dev, dst_w, dst_h,
                      border_value, out_dev);
}

extern "C" int oicc_camera_remap(int32_t device_ordinal, int32_t num_frames, int32_t src_w, int32_t src_h, int32_t channels,
                                 const uint8_t* frames, const float* map, int32_t dst_w, int32_t dst_h, int32_t border_value,
                                 int32_t batch, uint8_t* out, oicc_camera_remap_report* report) {
  if (!remap_args_ok(num_frames, src_w, src_h, channels, dst_w, dst_h, border_value) || batch < 1 || !frames || !map || !out)
    return OICC_ERR_INVALID_ARG;
  if (int rc = oicc::select_device(device_ordinal)) return rc;
  const auto t_start = std::chrono::steady_clock::now();
  const size_t map_floats = 2 * size_t(dst_w) * size_t(dst_h);
  oicc::DevBuf<float> d_map;
  FramePipeline pipe;      // behind the map: its streams are drained before the map goes
  OICC_HIP_TRY(d_map.resize(map_floats));
  OICC_HIP_TRY(hipMemcpy(d_map.p, map, sizeof(float) * map_floats, hipMemcpyHostToDevice));
  if (int rc = pipe.open(num_frames, batch, int64_t(src_w) * src_h * channels, int64_t(dst_w) * dst_h * channels)) return rc;
  const int rc = pipe.run(frames, out, [&](hipStream_t st, int, int num, const uint8_t* d_in, uint8_t* d_out) {
    return oicc_camera_remap_device(st, num, src_w, src_h, channels, d_in, d_map.p, dst_w, dst_h, border_value, d_out);
  });
  if (rc != OICC_OK) return rc;
  if (report) {
    const double ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    *report = oicc_camera_remap_report{pipe.ms_upload, pipe.ms_kernel, pipe.ms_download, ms_total};
  }
  return OICC_OK;
}
