// Device code shared by the camera maps (camera_maps.hip) and the rolling-shutter rectification (rolling_shutter.hip): the camera
// argument, pixel -> ray by Newton on the principal branch, and the bilinear sample of a u8 frame.  Both units are compiled with
// -ffp-contract=off (csrc/Makefile), so every sum here rounds as tests/camera_maps_restatement.py does.  Behind the device code,
// the host pipeline that both units' frame entries run their batches through (FramePipeline).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstring>
#include "../../include/oicc_hip.h"
#include "frame_batches.h"
#include "hip_resources.h"
#include "spline_math.h"

namespace oicc_camera {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kNewtonSteps = 20;
constexpr double kStepTol = 1e-13;
constexpr double kReprojectionTol = 1e-9;
constexpr int kMaxIntr = 10;

struct Camera { int model; double in[kMaxIntr]; };

__host__ __device__ inline int intrinsics_count(int model) {
  switch (model) {
    case oicc::CAM_PINHOLE: return 7;
    case oicc::CAM_PINHOLE_RADIAL_TANGENTIAL: return 10;
    case oicc::CAM_FISHEYE: return 9;
    case oicc::CAM_DIVISION_UNDISTORTION: return 5;
    case oicc::CAM_DOUBLE_SPHERE: return 7;
    case oicc::CAM_EXTENDED_UNIFIED: return 7;
    default: return 0;
  }
}

struct Rotation { double r[9]; };

inline bool make_camera(int32_t model, const double* intr, Camera* cam) {
  const int n = intrinsics_count(model);
  if (n == 0 || !intr) return false;
  cam->model = model;
  for (int k = 0; k < kMaxIntr; ++k) cam->in[k] = 0.0;
  for (int k = 0; k < n; ++k) {
    if (!std::isfinite(intr[k])) return false;
    cam->in[k] = intr[k];
  }
  return true;
}

// the destination camera whose rays have a closed form (camera_map_kernel)
inline int is_plain_pinhole(const Camera& cam) { return cam.model == oicc::CAM_PINHOLE && cam.in[5] == 0.0 && cam.in[6] == 0.0; }

constexpr int64_t kMaxLanes = ((int64_t(1) << 31) - 1) * kThreads;   // one lane per pixel: the grid's x dimension stays below 2^31 blocks

inline unsigned blocks_for(int64_t n) { return unsigned((n + kThreads - 1) / kThreads); }

__device__ __forceinline__ double max_abs2(double a, double b) { return fmax(fabs(a), fabs(b)); }

// The ray (x, y, 1) of pixel (u, v) on the principal branch; false (and NaN) where there is none.
__device__ inline bool unproject(const Camera& cam, double u, double v, double& x, double& y) {
  const bool division = cam.model == oicc::CAM_DIVISION_UNDISTORTION;
  const double f = cam.in[0], fa = cam.in[0] * cam.in[1];
  const double cx = division ? cam.in[2] : cam.in[3], cy = division ? cam.in[3] : cam.in[4];
  x = (u - cx) / f;
  y = (v - cy) / fa;
  double px[2], J[6];
  bool ok = true;
  for (int it = 0; it < kNewtonSteps; ++it) {
    const double p[3] = {x, y, 1.0};
    ok = oicc::camera_project<true>(cam.model, cam.in, p, px, J);
    if (!ok) break;
    const double ex = px[0] - u, ey = px[1] - v;
    const double det = J[0] * J[4] - J[1] * J[3];
    const double dx = (J[4] * ex - J[1] * ey) / det;
    const double dy = (J[0] * ey - J[3] * ex) / det;
    x -= dx;
    y -= dy;
    if (!(max_abs2(dx, dy) > kStepTol * (1.0 + max_abs2(x, y)))) break;    // also leaves on NaN
  }
  if (ok) {
    const double p[3] = {x, y, 1.0};
    ok = oicc::camera_project<true>(cam.model, cam.in, p, px, J);
    const double err = max_abs2(px[0] - u, px[1] - v);
    const double det = J[0] * J[4] - J[1] * J[3];
    const double tr = J[0] / f + J[4] / fa;
    ok = ok && isfinite(x) && isfinite(y) && isfinite(err) && isfinite(det) && isfinite(tr) &&
         err <= kReprojectionTol * (1.0 + max_abs2(u, v)) && det > 0.0 && tr > 0.0;
  }
  if (!ok) { x = nan(""); y = nan(""); }
  return ok;
}

// The four weights and offsets of one float32 map entry in a [src_h][src_w][CH] u8 frame.
template <int CH>
struct BilinearTap {
  double w00, w01, w10, w11;
  int64_t o00, o01, o10, o11;

  // false: the entry is NaN or outside [0, src_w - 1] x [0, src_h - 1] (NaN fails every comparison) and the pixel takes the border value
  __device__ __forceinline__ bool set(float2 m, int src_w, int src_h) {
    const bool inside = m.x >= 0.0f && m.x <= float(src_w - 1) && m.y >= 0.0f && m.y <= float(src_h - 1);
    if (!inside) return false;
    const double xf = double(m.x), yf = double(m.y);
    const double x0 = floor(xf), y0 = floor(yf);
    const double a = xf - x0, b = yf - y0;
    w00 = (1.0 - a) * (1.0 - b); w01 = a * (1.0 - b); w10 = (1.0 - a) * b; w11 = a * b;
    const bool right = a != 0.0, down = b != 0.0;       // a weight of exactly 0: the neighbour is not read (last row / column)
    o00 = (int64_t(y0) * src_w + int64_t(x0)) * CH;
    o01 = right ? o00 + CH : o00; o10 = down ? o00 + int64_t(src_w) * CH : o00;
    o11 = o10 + (right ? CH : 0);
    return true;
  }
  __device__ __forceinline__ uint8_t sample(const uint8_t* s, int c) const {
    const double p00 = double(s[o00 + c]), p01 = double(s[o01 + c]), p10 = double(s[o10 + c]), p11 = double(s[o11 + c]);
    const double val = (w00 * p00 + w01 * p01) + (w10 * p10 + w11 * p11);
    const double r = floor(val + 0.5);
    return uint8_t(r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r));
  }
};

// ---- host side: u8 frames through the device in batches ------------------------------------------------------------------------
// One batch per slot and stream: host copy into pinned memory, upload, the caller's kernels, download, host copy out; the other
// slot's batch overlaps.  open() makes every allocation, so none sits inside a timed span.  launch(stream, first, num, d_in,
// d_out) enqueues the kernels for frames [first, first + num), whose input lies at d_in and whose output goes to d_out.
struct FramePipeline {
  struct Slot {
    oicc::Stream st;      // ahead of the staging, so destroyed behind it: ~FramePipeline has drained it by then
    oicc::Event ev[4];    // upload start, upload end, kernel end, download end
    oicc::DevBuf<uint8_t> d_out, d_in;
    oicc::PinnedBuf<uint8_t> pin_out, pin_in;
  };
  Slot slot[2];
  // Both streams drained first, then (members, in reverse) per slot the staging freed and its stream destroyed last: drained
  // before freed, as the order rule of hip_resources.h asks, by this destructor and not by where the streams are declared.
  ~FramePipeline() { for (Slot& s : slot) if (s.st) (void)hipStreamSynchronize(s.st); }
  int num_frames = 0, batch = 0;
  int64_t in_frame = 0, out_frame = 0;     // bytes per source / destination frame
  double ms_upload = 0.0, ms_kernel = 0.0, ms_download = 0.0;    // summed over the batches

  int open(int num_frames_, int batch_, int64_t in_frame_, int64_t out_frame_) {
    num_frames = num_frames_; batch = std::min(batch_, num_frames_); in_frame = in_frame_; out_frame = out_frame_;
    for (int q = 0; q < oicc::frame_batch_slots(num_frames, batch); ++q) {
      Slot& s = slot[q];
      OICC_HIP_TRY(s.st.create());
      OICC_HIP_TRY(s.pin_in.alloc(size_t(batch * in_frame)));
      OICC_HIP_TRY(s.pin_out.alloc(size_t(batch * out_frame)));
      OICC_HIP_TRY(s.d_in.resize(size_t(batch * in_frame)));
      OICC_HIP_TRY(s.d_out.resize(size_t(batch * out_frame)));
      for (auto& e : s.ev) OICC_HIP_TRY(e.create());
    }
    return OICC_OK;
  }

  template <class Launch>
  int run(const uint8_t* frames, uint8_t* out, Launch&& launch) {
    return oicc::run_frame_batches(
        num_frames, batch,
        [&](int q, int first, int num) -> int {
          Slot& s = slot[q];
          std::memcpy(s.pin_in.p, frames + int64_t(first) * in_frame, size_t(num * in_frame));
          OICC_HIP_TRY(hipEventRecord(s.ev[0], s.st));
          OICC_HIP_TRY(hipMemcpyAsync(s.d_in.p, s.pin_in.p, size_t(num * in_frame), hipMemcpyHostToDevice, s.st));
          OICC_HIP_TRY(hipEventRecord(s.ev[1], s.st));
          if (launch(s.st.s, first, num, s.d_in.p, s.d_out.p) != OICC_OK) return OICC_ERR_HIP;
          OICC_HIP_TRY(hipEventRecord(s.ev[2], s.st));
          OICC_HIP_TRY(hipMemcpyAsync(s.pin_out.p, s.d_out.p, size_t(num * out_frame), hipMemcpyDeviceToHost, s.st));
          OICC_HIP_TRY(hipEventRecord(s.ev[3], s.st));
          return OICC_OK;
        },
        [&](int q, int first, int num) -> int {
          Slot& s = slot[q];
          OICC_HIP_TRY(hipStreamSynchronize(s.st));
          double* acc[3] = {&ms_upload, &ms_kernel, &ms_download};
          for (int j = 0; j < 3; ++j) {
            float ms = 0.0f;
            OICC_HIP_TRY(hipEventElapsedTime(&ms, s.ev[j], s.ev[j + 1]));
            *acc[j] += ms;
          }
          std::memcpy(out + int64_t(first) * out_frame, s.pin_out.p, size_t(num * out_frame));
          return OICC_OK;
        });
  }
};

}  // namespace oicc_camera
