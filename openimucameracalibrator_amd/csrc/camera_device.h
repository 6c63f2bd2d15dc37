// Device code shared by the camera maps (camera_maps.hip) and the rolling-shutter rectification (rolling_shutter.hip): the camera
// argument, pixel -> ray by Newton on the principal branch, and the bilinear sample of a u8 frame.  Both units are compiled with
// -ffp-contract=off (csrc/Makefile), so every sum here rounds as tests/camera_maps_restatement.py does.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include "../../include/oicc_hip.h"
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

inline int select_device(int32_t device_ordinal) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device_ordinal < 0 || device_ordinal >= ndev) return OICC_ERR_NO_DEVICE;   // no CPU fallback
  if (hipSetDevice(device_ordinal) != hipSuccess) return OICC_ERR_NO_DEVICE;
  return OICC_OK;
}

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

}  // namespace oicc_camera
