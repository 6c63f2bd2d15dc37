// Gyro video stabilisation (include/oicc_hip.h, "stabilisation"; DESIGN.md section 3, "Stabilisation").  Rotation only, on top of
// the rolling-shutter rectification: the orientation path of the clip, a smooth virtual camera on SO(3), the zoom that keeps the
// stabilised frame inside the source image, and the rolling-shutter warp with a per-frame rotation and focal length.
//
//   stab_path_delta_kernel  one lane per pair of consecutive on-path frames: D_k = Q(t_ref,k)^-1 Q(t_ref,k+1), chained through the
//                           partial interval, the whole intervals and the last partial interval (any number of gyro samples).
//   stab_path_scan_kernel   one workgroup: each lane chains a contiguous run of D, an LDS scan of the 256 run products, each lane
//                           applies its prefix; every path quaternion is normalised once at the end.
//   stab_smooth_kernel      one wave per on-path frame, lanes across the window members (strided by 64): the weighted intrinsic
//                           mean by a fixed butterfly, then the correction C_k and its clamp.
//   stab_accl_world_kernel  horizon lock, one lane per accelerometer sample: the orientation at the sample by the delta kernel's chain
//                           from its frame's t_ref, and the corrected specific force in the path's frame; the gate.
//   stab_level_kernel       horizon lock, one wave per on-path frame, lanes across the gravity window (strided by 64): the weighted mean
//                           of those vectors by the same butterfly, up and roll in the smooth camera, the levelled camera and its C_k.
//   stab_record_kernel      one lane per frame: M_k = R(C_k) R9 and the scaled focal length and skew.
//   stab_zoom_kernel        one lane per (frame, border point), the frame in the grid's y, its table in LDS: the march from the
//                           centre and the bisection; the minimum per wave.  stab_zoom_min_kernel: per frame, z = 1 / min s.
//   stab_map_kernel, stab_frames_kernel<CH>  rs_map_kernel and rs_rectify_kernel with the frame's record instead of the call-wide
//                           R and the ray buffer: the ray is rs_ray_kernel's closed form on the scaled intrinsics.
//
// tests/stabilization_restatement.py restates every step in numpy.  Compiled with -ffp-contract=off like rolling_shutter.o:
// oicc_stab_map is bit-equal to oicc_rs_rectify_map called with R9 = M_k and the scaled destination intrinsics.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>
#include "rolling_shutter_device.h"

namespace {

using namespace oicc_camera;
using namespace oicc_rs;

constexpr int kScanLanes = 256;          // lanes of the path scan: one run of frames each
constexpr int kMinRun = 4;               // frames per run, at least
constexpr int kMeanIterations = 16;
constexpr double kMeanTol = 1e-12;       // rad
constexpr int kMarch = 32;               // samples from the centre to a border point
constexpr int kBisections = 16;
constexpr double kPi = 3.141592653589793, kTwoPi = 6.283185307179586;
constexpr double kSin10 = 0.17364817766693033, kSin20 = 0.3420201433256687;      // the horizon lock fades in between these tilts

struct StabRecord { double M[9], f, skew; };      // per frame: R(C_k) R9, f Z_k, skew Z_k

__device__ __forceinline__ Q4 qconj(const Q4& q) { return Q4{q.w, -q.x, -q.y, -q.z}; }

__device__ __forceinline__ Q4 qnormalized(const Q4& q) {
  const double n = sqrt(((q.w * q.w + q.x * q.x) + q.y * q.y) + q.z * q.z);
  return Q4{q.w / n, q.x / n, q.y / n, q.z / n};
}

// Log of a quaternion of any norm as a rotation vector, the shorter way round
__device__ __forceinline__ void qlog(const Q4& q, double v[3]) {
  const double sg = q.w < 0.0 ? -1.0 : 1.0;
  const double w = sg * q.w, x = sg * q.x, y = sg * q.y, z = sg * q.z;
  const double n = sqrt((x * x + y * y) + z * z);
  const double k = n < 1e-8 ? 2.0 / w : 2.0 * atan2(n, w) / n;
  v[0] = k * x; v[1] = k * y; v[2] = k * z;
}

__device__ __forceinline__ Q4 qexp(const double v[3]) {
  const double th = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  const double half = th / 2.0;
  const double k = th < 1e-8 ? 0.5 - th * th / 48.0 : sin(half) / th;
  return Q4{cos(half), k * v[0], k * v[1], k * v[2]};
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, 64);
  return v;
}

// R(q) v, rows summed from the left
__device__ __forceinline__ void qrotate(const Q4& q, const double v[3], double o[3]) {
  double M[9];
  rotation_matrix(q, M);
  for (int r = 0; r < 3; ++r) o[r] = (M[3 * r] * v[0] + M[3 * r + 1] * v[1]) + M[3 * r + 2] * v[2];
}

// into (-pi, pi], for |d| <= 2 pi
__device__ __forceinline__ double wrap_angle(double d) {
  if (d > kPi) d = d - kTwoPi;
  if (d <= -kPi) d = d + kTwoPi;
  return d;
}

// C = path^-1 L, normalised, w >= 0, shortened along its own axis to max_correction (0: no bound): the rule of stab_smooth_kernel
__device__ __forceinline__ Q4 correction_of(const Q4& path, const Q4& L, double max_correction) {
  Q4 Cq = qnormalized(qmul(qconj(path), L));
  if (Cq.w < 0.0) Cq = Q4{-Cq.w, -Cq.x, -Cq.y, -Cq.z};
  const double n = sqrt((Cq.x * Cq.x + Cq.y * Cq.y) + Cq.z * Cq.z);
  if (max_correction > 0.0 && 2.0 * atan2(n, Cq.w) > max_correction) {
    const double h = max_correction / 2.0, sn = sin(h) / n;
    Cq = Q4{cos(h), sn * Cq.x, sn * Cq.y, sn * Cq.z};
  }
  return Cq;
}

// delta [pairs][4]: pair i joins the on-path frames first + i and first + i + 1; interval [frames]: the gyro interval of t_ref
__global__ __launch_bounds__(kThreads) void stab_path_delta_kernel(int pairs, int first, const double* __restrict__ gyro_t, const double* __restrict__ rates,
                                                                   const double* __restrict__ frame_t, const int64_t* __restrict__ interval,
                                                                   double time_offset, double reference_delay, double* __restrict__ delta) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= pairs) return;
  const int k = first + i;
  const int64_t ja = interval[k], jb = interval[k + 1] > ja ? interval[k + 1] : ja;
  // times as differences first, each reference time against its own frame
  const double sa = 0.0 - (((gyro_t[ja] - frame_t[k]) + time_offset) - reference_delay);
  const double sb = 0.0 - (((gyro_t[jb] - frame_t[k + 1]) + time_offset) - reference_delay);
  const double dta = gyro_t[ja + 1] - gyro_t[ja];
  Q4 q = qconj(interval_exp(rates + 3 * ja, rates + 3 * ja + 3, dta, sa));
  if (ja == jb) {
    q = qmul(q, interval_exp(rates + 3 * ja, rates + 3 * ja + 3, dta, sb));
  } else {
    q = qmul(q, interval_exp(rates + 3 * ja, rates + 3 * ja + 3, dta, dta));
    for (int64_t j = ja + 1; j < jb; ++j) {
      const double dt = gyro_t[j + 1] - gyro_t[j];
      q = qmul(q, interval_exp(rates + 3 * j, rates + 3 * j + 3, dt, dt));
    }
    q = qmul(q, interval_exp(rates + 3 * jb, rates + 3 * jb + 3, gyro_t[jb + 1] - gyro_t[jb], sb));
  }
  double* o = delta + 4 * int64_t(i);
  o[0] = q.w; o[1] = q.x; o[2] = q.y; o[3] = q.z;
}

// path [count][4]: path_0 = 1, path_i = path_{i-1} delta_{i-1}.  Lane r owns the frames [r run, (r + 1) run).
__global__ __launch_bounds__(kScanLanes) void stab_path_scan_kernel(int count, int run, const double* __restrict__ delta, double* __restrict__ path) {
  __shared__ Q4 lds[kScanLanes];
  const int r = threadIdx.x;
  const int b = min(r * run, count), e = min(b + run, count);
  auto element = [&](int i) { return i == 0 ? Q4{1.0, 0.0, 0.0, 0.0} : Q4{delta[4 * int64_t(i - 1)], delta[4 * int64_t(i - 1) + 1], delta[4 * int64_t(i - 1) + 2], delta[4 * int64_t(i - 1) + 3]}; };
  Q4 q = {1.0, 0.0, 0.0, 0.0};
  for (int i = b; i < e; ++i) q = qmul(q, element(i));
  lds[r] = q;
  __syncthreads();
  for (int d = 1; d < kScanLanes; d <<= 1) {
    const Q4 mine = lds[r];
    const Q4 v = r >= d ? qmul(lds[r - d], mine) : mine;      // the earlier frames on the left
    __syncthreads();
    lds[r] = v;
    __syncthreads();
  }
  q = r == 0 ? Q4{1.0, 0.0, 0.0, 0.0} : lds[r - 1];
  for (int i = b; i < e; ++i) {
    q = qmul(q, element(i));
    const Q4 u = qnormalized(q);
    double* o = path + 4 * int64_t(i);
    o[0] = u.w; o[1] = u.x; o[2] = u.y; o[3] = u.z;
  }
}

// All arrays are indexed by the frame; the on-path frames are [first, first + count).  win_lo / win_hi: the window of a frame, frame
// indices, both ends included.  smooth [frames][4], correction [frames][4], iterations [frames].
__global__ __launch_bounds__(kThreads) void stab_smooth_kernel(int count, int first, const double* __restrict__ frame_t, const double* __restrict__ path,
                                                               const int32_t* __restrict__ win_lo, const int32_t* __restrict__ win_hi, double sigma,
                                                               double max_correction, double* __restrict__ smooth, double* __restrict__ correction,
                                                               int32_t* __restrict__ iterations) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (i >= count) return;                                  // whole waves leave
  const int k = first + i;
  auto load = [&](int m) { return Q4{path[4 * int64_t(m)], path[4 * int64_t(m) + 1], path[4 * int64_t(m) + 2], path[4 * int64_t(m) + 3]}; };
  const Q4 qk = load(k);
  const int lo = win_lo[k], hi = win_hi[k];
  Q4 S = qk, Cq = {1.0, 0.0, 0.0, 0.0};
  int it = 0;
  if (sigma > 0.0 && hi > lo) {
    const double tk = frame_t[k], den = 2.0 * (sigma * sigma);
    double sw = 0.0;
    for (int m = lo + lane; m <= hi; m += 64) {
      const double dt = frame_t[m] - tk;
      sw = sw + exp(-(dt * dt) / den);
    }
    sw = wave_sum(sw);
    while (it < kMeanIterations) {
      const Q4 Sinv = qconj(S);
      double a0 = 0.0, a1 = 0.0, a2 = 0.0;
      for (int m = lo + lane; m <= hi; m += 64) {
        const double dt = frame_t[m] - tk;
        const double w = exp(-(dt * dt) / den);
        double v[3];
        qlog(qmul(Sinv, load(m)), v);
        a0 = a0 + w * v[0]; a1 = a1 + w * v[1]; a2 = a2 + w * v[2];
      }
      const double mean[3] = {wave_sum(a0) / sw, wave_sum(a1) / sw, wave_sum(a2) / sw};
      S = qmul(S, qexp(mean));
      ++it;
      if (sqrt((mean[0] * mean[0] + mean[1] * mean[1]) + mean[2] * mean[2]) <= kMeanTol) break;
    }
    S = qnormalized(S);
    Cq = qnormalized(qmul(qconj(qk), S));
    if (Cq.w < 0.0) Cq = Q4{-Cq.w, -Cq.x, -Cq.y, -Cq.z};
    const double n = sqrt((Cq.x * Cq.x + Cq.y * Cq.y) + Cq.z * Cq.z);
    if (max_correction > 0.0 && 2.0 * atan2(n, Cq.w) > max_correction) {       // shortened along its own axis
      const double h = max_correction / 2.0, sn = sin(h) / n;
      Cq = Q4{cos(h), sn * Cq.x, sn * Cq.y, sn * Cq.z};
    }
  }
  if (lane == 0) {
    double* s = smooth + 4 * int64_t(k);
    double* c = correction + 4 * int64_t(k);
    s[0] = S.w; s[1] = S.x; s[2] = S.y; s[3] = S.z;
    c[0] = Cq.w; c[1] = Cq.x; c[2] = Cq.y; c[3] = Cq.z;
    iterations[k] = it;
  }
}

// G1 of the horizon lock, one lane per accelerometer sample.  frame_of [na]: the sample's on-path frame k or -1; sample_interval [na]:
// its gyro interval; interval [frames]: the gyro interval of t_ref.  The chain is stab_path_delta_kernel's with the sample's time in
// place of t_ref,k+1.  world [na][3] = R(path_k D_j) R(q_i_c)^T a_j, NaN for an unused sample; gate [na] 1 / 0.
__global__ __launch_bounds__(kThreads) void stab_accl_world_kernel(int64_t na, const double* __restrict__ accl_t, const double* __restrict__ accl,
                                                                   const int32_t* __restrict__ frame_of, const int64_t* __restrict__ sample_interval,
                                                                   const double* __restrict__ gyro_t, const double* __restrict__ rates,
                                                                   const double* __restrict__ frame_t, const int64_t* __restrict__ interval,
                                                                   const double* __restrict__ path, Rotation Ric, double time_offset, double reference_delay,
                                                                   double gravity_const, double accl_gate, double* __restrict__ world,
                                                                   uint8_t* __restrict__ gate) {
  const int64_t j = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (j >= na) return;
  const double a[3] = {accl[3 * j], accl[3 * j + 1], accl[3 * j + 2]};
  const double norm = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
  gate[j] = (accl_gate == 0.0 || fabs(norm - gravity_const) <= accl_gate) ? 1 : 0;
  double* o = world + 3 * j;
  const int k = frame_of[j];
  if (k < 0) { o[0] = nan(""); o[1] = nan(""); o[2] = nan(""); return; }
  const int64_t ja = interval[k], jb = sample_interval[j] > ja ? sample_interval[j] : ja;
  const double s = ((accl_t[j] - frame_t[k]) + time_offset) - reference_delay;
  const double sa = 0.0 - (((gyro_t[ja] - frame_t[k]) + time_offset) - reference_delay);
  const double sb = s - (((gyro_t[jb] - frame_t[k]) + time_offset) - reference_delay);
  const double dta = gyro_t[ja + 1] - gyro_t[ja];
  Q4 q = qconj(interval_exp(rates + 3 * ja, rates + 3 * ja + 3, dta, sa));
  if (ja == jb) {
    q = qmul(q, interval_exp(rates + 3 * ja, rates + 3 * ja + 3, dta, sb));
  } else {
    q = qmul(q, interval_exp(rates + 3 * ja, rates + 3 * ja + 3, dta, dta));
    for (int64_t i = ja + 1; i < jb; ++i) {
      const double dt = gyro_t[i + 1] - gyro_t[i];
      q = qmul(q, interval_exp(rates + 3 * i, rates + 3 * i + 3, dt, dt));
    }
    q = qmul(q, interval_exp(rates + 3 * jb, rates + 3 * jb + 3, gyro_t[jb + 1] - gyro_t[jb], sb));
  }
  const double* p = path + 4 * int64_t(k);
  q = qnormalized(qmul(Q4{p[0], p[1], p[2], p[3]}, q));
  double cam[3];
  for (int c = 0; c < 3; ++c) cam[c] = (Ric.r[c] * a[0] + Ric.r[3 + c] * a[1]) + Ric.r[6 + c] * a[2];      // R(q_i_c)^T a
  qrotate(q, cam, o);
}

// G2 of the horizon lock, one wave per on-path frame, lanes across the gravity window (strided by 64): the weighted mean of the world
// vectors by the fixed butterfly, up and roll in the smooth camera, the levelled camera L_k and its correction.  win_lo / win_hi:
// sample indices, both ends included (hi < lo: empty).  A frame whose angle is 0 keeps smooth_q as level_q and the correction it has.
__global__ __launch_bounds__(kThreads) void stab_level_kernel(int count, int first, const double* __restrict__ frame_t, const double* __restrict__ accl_t,
                                                              const double* __restrict__ world, const uint8_t* __restrict__ gate,
                                                              const int64_t* __restrict__ win_lo, const int64_t* __restrict__ win_hi,
                                                              const double* __restrict__ path, const double* __restrict__ smooth, double time_offset,
                                                              double reference_delay, double sigma, double gravity_const, double lock, double roll_wanted,
                                                              double max_correction, double* __restrict__ level_q, double* __restrict__ correction,
                                                              double* __restrict__ up, double* __restrict__ roll, double* __restrict__ angle,
                                                              int32_t* __restrict__ samples, int32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (i >= count) return;                                  // whole waves leave
  const int k = first + i;
  const int64_t lo = win_lo[k], hi = win_hi[k];
  const double tk = frame_t[k], den = 2.0 * (sigma * sigma);
  double sw = 0.0, a0 = 0.0, a1 = 0.0, a2 = 0.0, cnt = 0.0;
  for (int64_t m = lo + lane; m <= hi; m += 64) {
    const double s = ((accl_t[m] - tk) + time_offset) - reference_delay;
    const double g = double(gate[m]);
    const double w = exp(-(s * s) / den) * g;
    const double* u = world + 3 * m;
    sw = sw + w; a0 = a0 + w * u[0]; a1 = a1 + w * u[1]; a2 = a2 + w * u[2]; cnt = cnt + g;
  }
  sw = wave_sum(sw); a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2); cnt = wave_sum(cnt);
  auto load = [&](const double* b) { return Q4{b[4 * int64_t(k)], b[4 * int64_t(k) + 1], b[4 * int64_t(k) + 2], b[4 * int64_t(k) + 3]}; };
  const Q4 S = load(smooth);
  Q4 L = S;
  double nu[3] = {nan(""), nan(""), nan("")}, rho = nan(""), theta = 0.0;
  int st = 2;
  if (cnt > 0.0) {
    const double gm[3] = {a0 / sw, a1 / sw, a2 / sw};
    const double norm = sqrt((gm[0] * gm[0] + gm[1] * gm[1]) + gm[2] * gm[2]);
    if (!(norm < 0.5 * gravity_const)) {
      const double n[3] = {gm[0] / norm, gm[1] / norm, gm[2] / norm};
      double M[9];
      rotation_matrix(S, M);
      for (int c = 0; c < 3; ++c) nu[c] = (M[c] * n[0] + M[3 + c] * n[1]) + M[6 + c] * n[2];        // R(S_k)^T: up in the smooth camera
      const double h = sqrt(nu[0] * nu[0] + nu[1] * nu[1]);
      rho = atan2(nu[0], -nu[1]);
      st = h < kSin10 ? 1 : 0;
      if (st == 0) {
        const double fade = fmin(fmax((h - kSin10) / (kSin20 - kSin10), 0.0), 1.0);
        theta = (lock * fade) * wrap_angle(rho - roll_wanted);
        if (theta == 0.0) theta = 0.0;                     // no -0
      }
    }
  }
  Q4 Cq = {1.0, 0.0, 0.0, 0.0};
  if (theta != 0.0) {
    const double half = theta / 2.0;
    L = qnormalized(qmul(S, Q4{cos(half), 0.0, 0.0, sin(half)}));
    Cq = correction_of(load(path), L, max_correction);
  }
  if (lane == 0) {
    double* l = level_q + 4 * int64_t(k);
    l[0] = L.w; l[1] = L.x; l[2] = L.y; l[3] = L.z;
    if (theta != 0.0) {
      double* c = correction + 4 * int64_t(k);
      c[0] = Cq.w; c[1] = Cq.x; c[2] = Cq.y; c[3] = Cq.z;
    }
    up[3 * int64_t(k)] = nu[0]; up[3 * int64_t(k) + 1] = nu[1]; up[3 * int64_t(k) + 2] = nu[2];
    roll[k] = rho; angle[k] = theta; samples[k] = int32_t(cnt); status[k] = st;
  }
}

// record [frames]: M_k = R(C_k) R9 (R9 is applied to the destination ray first), f Z_k and skew Z_k with one rounding each
__global__ __launch_bounds__(64) void stab_record_kernel(int num_frames, Rotation R9, double f, double skew, const double* __restrict__ correction,
                                                         const double* __restrict__ zoom, StabRecord* __restrict__ record) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= num_frames) return;
  const double* c = correction + 4 * int64_t(k);
  double C[9];
  rotation_matrix(Q4{c[0], c[1], c[2], c[3]}, C);
  StabRecord r;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r.M[3 * i + j] = (C[3 * i] * R9.r[j] + C[3 * i + 1] * R9.r[3 + j]) + C[3 * i + 2] * R9.r[6 + j];
  r.f = f * zoom[k];
  r.skew = skew * zoom[k];
  record[k] = r;
}

// rs_ray_kernel's closed form for a plain PINHOLE whose focal length and skew are the frame's
__device__ __forceinline__ void record_ray(const RsParams& P, double f, double skew, double u, double v, double& x, double& y) {
  y = (v - P.dst.in[4]) / (f * P.dst.in[1]);
  x = (u - P.dst.in[3] - skew * y) / f;
}

// border point i of a w x h rectangle: the top row, the bottom row, the left and the right column between them; a rectangle one
// pixel wide or high is all border
__device__ __forceinline__ void border_point(int i, int w, int h, double& u, double& v) {
  if (w == 1 || h == 1) { u = double(i % w); v = double(i / w); return; }
  if (i < w) { u = double(i); v = 0.0; return; }
  if (i < 2 * w) { u = double(i - w); v = double(h - 1); return; }
  const int j = i - 2 * w;
  if (j < h - 2) { u = 0.0; v = double(1 + j); return; }
  u = double(w - 1); v = double(1 + j - (h - 2));
}

// wave_min [frames][waves]: min over the wave's border points of the largest valid s found; NaN for a frame without a table
__global__ __launch_bounds__(kThreads) void stab_zoom_kernel(RsParams P, int first_frame, const double* __restrict__ table, const int32_t* __restrict__ count,
                                                             const StabRecord* __restrict__ record, int points, int waves, double* __restrict__ wave_min) {
  __shared__ double lds[kMaxWindow * kEntry];
  const int frame = first_frame + blockIdx.y;
  int n;
  const bool have = stage_table(table, count, frame, lds, n);
  const int i = blockIdx.x * kThreads + threadIdx.x;
  double s = INFINITY;                                     // lanes behind the last point stay for the butterfly
  if (have && i < points) {
    const StabRecord rec = record[frame];
    double u, v, x, y, px[2];
    int evals;
    border_point(i, P.dst_w, P.dst_h, u, v);
    record_ray(P, rec.f, rec.skew, u, v, x, y);
    s = 0.0;
    if (solve_pixel(P, rec.M, lds, n, 0.0, 0.0, true, px, evals)) {      // the centre
      s = 1.0;
      for (int j = 1; j <= kMarch; ++j) {
        const double sj = double(j) / double(kMarch);
        if (solve_pixel(P, rec.M, lds, n, sj * x, sj * y, true, px, evals)) continue;
        double lo = double(j - 1) / double(kMarch), hi = sj;       // lo is valid
        for (int b = 0; b < kBisections; ++b) {
          const double mid = 0.5 * (lo + hi);
          if (solve_pixel(P, rec.M, lds, n, mid * x, mid * y, true, px, evals)) lo = mid; else hi = mid;
        }
        s = lo;
        break;
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s = fmin(s, __shfl_xor(s, d, 64));
  if ((threadIdx.x & 63) == 0) wave_min[int64_t(frame) * waves + blockIdx.x * kWaves + (threadIdx.x >> 6)] = have ? s : nan("");
}

__global__ __launch_bounds__(64) void stab_zoom_min_kernel(int num_frames, int waves, const double* __restrict__ wave_min, double* __restrict__ required) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= num_frames) return;
  const double* w = wave_min + int64_t(k) * waves;
  double s = w[0];                                         // NaN: no table
  for (int j = 1; j < waves; ++j) s = fmin(s, w[j]);
  required[k] = 1.0 / s;
}

// map [frames][pixels], valid [frames][pixels], evaluations [frames][pixels] or null
__global__ __launch_bounds__(kThreads) void stab_map_kernel(RsParams P, int first_frame, const double* __restrict__ table, const int32_t* __restrict__ count,
                                                            const StabRecord* __restrict__ record, int64_t pixels, float2* __restrict__ map,
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
    const StabRecord rec = record[frame];
    double x, y;
    record_ray(P, rec.f, rec.skew, double(i % P.dst_w), double(i / P.dst_w), x, y);
    ok = solve_pixel(P, rec.M, lds, n, x, y, true, px, evals);
  }
  const float qnan = __builtin_nanf("");
  const int64_t o = int64_t(frame) * pixels + i;
  map[o] = ok ? make_float2(float(px[0]), float(px[1])) : make_float2(qnan, qnan);
  valid[o] = ok ? 1 : 0;
  if (evaluations) evaluations[o] = uint8_t(evals);
}

// frames / out: the batch's first frame at index 0; table, count and record are indexed by first_frame + blockIdx.y
template <int CH>
__global__ __launch_bounds__(kThreads) void stab_frames_kernel(RsParams P, int first_frame, const double* __restrict__ table, const int32_t* __restrict__ count,
                                                               const StabRecord* __restrict__ record, int64_t pixels, const uint8_t* __restrict__ frames,
                                                               int border, uint8_t* __restrict__ out) {
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
    const StabRecord rec = record[frame];
    double x, y;
    record_ray(P, rec.f, rec.skew, double(i % P.dst_w), double(i / P.dst_w), x, y);
    ok = solve_pixel(P, rec.M, lds, n, x, y, true, px, evals);
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

// ---- host side ---------------------------------------------------------------------------------------------------------------

// the rolling-shutter judgement and the two further requirements of the stabilisation
int judge_scene(const oicc_rs_scene* s, Judged* J) {
  if (int rc = judge(s, J)) return rc;
  if (!J->P.dst_closed_form) return OICC_ERR_INVALID_ARG;
  for (int k = 1; k < s->num_frames; ++k) if (!(s->frame_t[k] > s->frame_t[k - 1])) return OICC_ERR_INVALID_ARG;
  return OICC_OK;
}

bool options_ok(const oicc_stab_options* o) {
  return o && std::isfinite(o->smoothing_sigma_s) && o->smoothing_sigma_s >= 0.0 && std::isfinite(o->max_correction_rad) && o->max_correction_rad >= 0.0 &&
         o->zoom_mode >= 0 && o->zoom_mode <= 2 && std::isfinite(o->zoom_window_s) && o->zoom_window_s >= 0.0 && std::isfinite(o->max_zoom) &&
         o->max_zoom >= 1.0;
}

// correction_q [frames][4] unit within 1e-6 (used as given), zoom [frames] finite and positive
bool plan_arrays_ok(const double* correction_q, const double* zoom, int frames) {
  if (!correction_q || !zoom || !all_finite(correction_q, 4 * int64_t(frames)) || !all_finite(zoom, frames)) return false;
  for (int k = 0; k < frames; ++k) {
    const double* q = correction_q + 4 * k;
    if (!(std::fabs(std::sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]) - 1.0) <= 1e-6) || !(zoom[k] > 0.0)) return false;
  }
  return true;
}

// The device side of a scene with its plan: the per-frame tables and records.
struct Prepared {
  oicc::DevBuf<double> gyro_t, rates, frame_t, table, correction, zoom;
  oicc::DevBuf<int64_t> first;
  oicc::DevBuf<int32_t> count;
  oicc::DevBuf<StabRecord> record;
  oicc::Event ev[3];     // before the table kernel, behind it, behind the record kernel
};

int upload_scene(const oicc_rs_scene* s, const Judged& J, hipStream_t st, Prepared* D) {
  const size_t n = size_t(J.num_gyro), f = size_t(J.num_frames);
  for (auto& e : D->ev) OICC_HIP_TRY(e.create());
  OICC_HIP_TRY(D->gyro_t.resize(n));
  OICC_HIP_TRY(D->rates.resize(3 * n));
  OICC_HIP_TRY(D->frame_t.resize(f));
  OICC_HIP_TRY(D->first.resize(f));
  OICC_HIP_TRY(D->count.resize(f));
  OICC_HIP_TRY(D->table.resize(size_t(kMaxWindow) * kEntry * f));
  OICC_HIP_TRY(D->correction.resize(4 * f));
  OICC_HIP_TRY(D->zoom.resize(f));
  OICC_HIP_TRY(D->record.resize(f));
  OICC_HIP_TRY(hipMemcpyAsync(D->gyro_t.p, s->gyro_t, sizeof(double) * n, hipMemcpyHostToDevice, st));
  OICC_HIP_TRY(hipMemcpyAsync(D->rates.p, J.rates_cam.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice, st));
  OICC_HIP_TRY(hipMemcpyAsync(D->frame_t.p, s->frame_t, sizeof(double) * f, hipMemcpyHostToDevice, st));
  OICC_HIP_TRY(hipMemcpyAsync(D->first.p, J.first.data(), sizeof(int64_t) * f, hipMemcpyHostToDevice, st));
  OICC_HIP_TRY(hipMemcpyAsync(D->count.p, J.count.data(), sizeof(int32_t) * f, hipMemcpyHostToDevice, st));
  return OICC_OK;
}

int launch_tables(const Judged& J, hipStream_t st, Prepared* D) {
  OICC_HIP_TRY(hipEventRecord(D->ev[0], st));
  hipLaunchKernelGGL(rs_frame_table_kernel, dim3(unsigned((J.num_frames + 63) / 64)), dim3(64), 0, st, J.num_frames, D->gyro_t.p, D->rates.p,
                     D->frame_t.p, D->first.p, D->count.p, J.P.time_offset, J.P.reference_row * J.P.line_delay, D->table.p);
  OICC_HIP_TRY(hipGetLastError());
  OICC_HIP_TRY(hipEventRecord(D->ev[1], st));
  return OICC_OK;
}

// the records from D->correction and D->zoom, which the stream has been given before
int launch_records(const Judged& J, hipStream_t st, Prepared* D) {
  hipLaunchKernelGGL(stab_record_kernel, dim3(unsigned((J.num_frames + 63) / 64)), dim3(64), 0, st, J.num_frames, J.P.R, J.P.dst.in[0], J.P.dst.in[2],
                     D->correction.p, D->zoom.p, D->record.p);
  OICC_HIP_TRY(hipGetLastError());
  return OICC_OK;
}

// Enqueues the uploads, the table kernel and the record kernel on st; J, the scene arrays and the plan arrays must outlive the work.
int prepare(const oicc_rs_scene* s, const Judged& J, const double* correction_q, const double* zoom, hipStream_t st, Prepared* D) {
  const size_t f = size_t(J.num_frames);
  if (int rc = upload_scene(s, J, st, D)) return rc;
  OICC_HIP_TRY(hipMemcpyAsync(D->correction.p, correction_q, sizeof(double) * 4 * f, hipMemcpyHostToDevice, st));
  OICC_HIP_TRY(hipMemcpyAsync(D->zoom.p, zoom, sizeof(double) * f, hipMemcpyHostToDevice, st));
  if (int rc = launch_tables(J, st, D)) return rc;
  if (int rc = launch_records(J, st, D)) return rc;
  OICC_HIP_TRY(hipEventRecord(D->ev[2], st));
  return OICC_OK;
}

// frames [first, first + num) of the scene; frames_dev / out_dev start at frame `first`
int launch_frames(hipStream_t st, const Judged& J, const Prepared& D, int first, int num, int channels, const uint8_t* frames_dev, int border,
                  uint8_t* out_dev) {
  const int64_t pixels = int64_t(J.P.dst_w) * J.P.dst_h;
  const int64_t in_frame = int64_t(J.P.src_w) * J.P.src_h * channels, out_frame = pixels * channels;
  for (int done = 0; done < num; done += kFrameChunk) {
    const int m = std::min(kFrameChunk, num - done);
    const dim3 grid(blocks_for(pixels), unsigned(m));
    if (channels == 1)
      hipLaunchKernelGGL(stab_frames_kernel<1>, grid, dim3(kThreads), 0, st, J.P, first + done, D.table.p, D.count.p, D.record.p, pixels,
                         frames_dev + done * in_frame, border, out_dev + done * out_frame);
    else
      hipLaunchKernelGGL(stab_frames_kernel<3>, grid, dim3(kThreads), 0, st, J.P, first + done, D.table.p, D.count.p, D.record.p, pixels,
                         frames_dev + done * in_frame, border, out_dev + done * out_frame);
    if (hipGetLastError() != hipSuccess) return OICC_ERR_HIP;
  }
  return OICC_OK;
}

void copy_status(const Judged& J, int32_t* frame_status) { std::memcpy(frame_status, J.status.data(), sizeof(int32_t) * J.status.size()); }

bool frames_args_ok(int32_t channels, int32_t border_value) { return (channels == 1 || channels == 3) && border_value >= 0 && border_value <= 255; }

int border_points(int w, int h) { return (w == 1 || h == 1) ? w * h : 2 * (w + h) - 4; }

// The applied zoom from the required one, on the host: O(frames x window).  t [frames] strictly increasing, z [frames] (used where
// status is 0).  mode 0: 1; 1: the maximum; 2: the running maximum over |dt| <= T, then its Gaussian mean (sigma T / 2) over the same
// window, held inside the window's own range, so that Z_k >= z_k survives the rounding of the mean.
void applied_zoom(int frames, const double* t, const double* z, const int32_t* status, const oicc_stab_options& o, double* Z, uint8_t* clamped) {
  std::vector<double> Y(size_t(frames), 1.0);
  if (o.zoom_mode == 1) {
    double m = -std::numeric_limits<double>::infinity();
    for (int k = 0; k < frames; ++k) if (status[k] == 0) m = std::max(m, z[k]);
    for (int k = 0; k < frames; ++k) Z[k] = m == -std::numeric_limits<double>::infinity() ? 1.0 : m;
  } else if (o.zoom_mode == 2) {
    const double T = o.zoom_window_s, sg = T / 2.0;
    int lo = 0, hi = 0;                       // the window [lo, hi) of frame k
    std::vector<int> wlo(size_t(frames), 0), whi(size_t(frames), 0);
    for (int k = 0; k < frames; ++k) {
      while (t[k] - t[lo] > T) ++lo;
      if (hi < k + 1) hi = k + 1;
      while (hi < frames && t[hi] - t[k] <= T) ++hi;
      wlo[size_t(k)] = lo; whi[size_t(k)] = hi;
      double m = -std::numeric_limits<double>::infinity();
      for (int j = lo; j < hi; ++j) if (status[j] == 0) m = std::max(m, z[j]);
      Y[size_t(k)] = m == -std::numeric_limits<double>::infinity() ? 1.0 : m;
    }
    for (int k = 0; k < frames; ++k) {
      double num = 0.0, den = 0.0, ymin = Y[size_t(k)], ymax = Y[size_t(k)];
      for (int j = wlo[size_t(k)]; j < whi[size_t(k)]; ++j) {
        const double dt = t[j] - t[k];
        const double g = sg > 0.0 ? std::exp(-(dt * dt) / (2.0 * (sg * sg))) : 1.0;
        num += g * Y[size_t(j)]; den += g;
        ymin = std::min(ymin, Y[size_t(j)]); ymax = std::max(ymax, Y[size_t(j)]);
      }
      const double mean = ymax == ymin ? ymin : num / den;         // inf among the Y: inf, not NaN
      Z[k] = std::isnan(mean) ? ymax : std::min(std::max(mean, ymin), ymax);
    }
  } else {
    for (int k = 0; k < frames; ++k) Z[k] = 1.0;
  }
  for (int k = 0; k < frames; ++k) {
    clamped[k] = Z[k] > o.max_zoom ? 1 : 0;
    if (clamped[k]) Z[k] = o.max_zoom;
  }
}

// the path by time comparisons: tau_j = ((t_j - t_k) + offset) - reference delay, on the path when tau_0 <= 0 <= tau_{n-1};
// interval [frames]: the gyro interval of t_ref
int find_path(const oicc_rs_scene* scene, const Judged& J, std::vector<int64_t>* interval, int* first_out, int* count_out) {
  const int F = J.num_frames;
  const int64_t n = J.num_gyro;
  const double off = J.P.time_offset, refd = J.P.reference_row * J.P.line_delay;
  interval->assign(size_t(F), 0);
  int first = 0, count = 0;
  for (int k = 0; k < F; ++k) {
    auto tau = [&](int64_t j) { return ((scene->gyro_t[j] - scene->frame_t[k]) + off) - refd; };
    if (tau(0) > 0.0 || tau(n - 1) < 0.0) continue;
    if (count == 0) first = k;
    if (first + count != k) return OICC_ERR_INVALID_ARG;      // contiguous by the order of the times; anything else is not a clip
    ++count;
    int64_t b = 0, e = n;                                       // number of samples with tau_j <= 0
    while (b < e) { const int64_t m = (b + e) / 2; if (tau(m) <= 0.0) b = m + 1; else e = m; }
    (*interval)[size_t(k)] = std::min(b - 1, n - 2);
  }
  *first_out = first; *count_out = count;
  return OICC_OK;
}

// the delta and the scan kernel: d_path [frames][4] gets the on-path frames
int launch_path(const Judged& J, hipStream_t st, const Prepared& D, const int64_t* d_interval, int first, int count, double* d_delta, double* d_path) {
  if (count < 1) return OICC_OK;
  if (count > 1) {
    hipLaunchKernelGGL(stab_path_delta_kernel, dim3(blocks_for(count - 1)), dim3(kThreads), 0, st, count - 1, first, D.gyro_t.p, D.rates.p, D.frame_t.p,
                       d_interval, J.P.time_offset, J.P.reference_row * J.P.line_delay, d_delta);
    OICC_HIP_TRY(hipGetLastError());
  }
  const int run = std::max(kMinRun, (count + kScanLanes - 1) / kScanLanes);
  hipLaunchKernelGGL(stab_path_scan_kernel, dim3(1), dim3(kScanLanes), 0, st, count, run, d_delta, d_path + 4 * size_t(first));
  OICC_HIP_TRY(hipGetLastError());
  return OICC_OK;
}

bool level_ok(const oicc_stab_level* l) {
  if (!l || l->num_accl < 1 || !l->accl_t || !l->accl || !all_finite(l->accl_t, l->num_accl) || !all_finite(l->accl, 3 * l->num_accl)) return false;
  for (int64_t j = 1; j < l->num_accl; ++j) if (!(l->accl_t[j] > l->accl_t[j - 1])) return false;
  return std::isfinite(l->gravity_sigma_s) && l->gravity_sigma_s > 0.0 && std::isfinite(l->gravity_const) && l->gravity_const > 0.0 &&
         std::isfinite(l->accl_gate) && l->accl_gate >= 0.0 && l->lock >= 0.0 && l->lock <= 1.0 && std::isfinite(l->roll_rad);
}

// What the host decides for the horizon lock, by time comparisons only: s_jk = ((accl_t[j] - frame_t[k]) + offset) - reference delay
struct LevelHost {
  std::vector<int32_t> frame_of;            // [na] the last on-path frame with s_jk >= 0; -1 before the first reference time or behind the last
  std::vector<int64_t> sample_interval;     // [na] the last gyro interval i <= n - 2 with tau_i(k) <= s_jk
  std::vector<int64_t> win_lo, win_hi;      // [frames] the used samples with |s_jk| <= 3 sigma_g, both ends included; hi < lo: none
  Rotation Ric;                             // R(q_i_c), the quaternion normalised first
};

void level_host(const oicc_rs_scene* scene, const Judged& J, const oicc_stab_level* l, int first, int count, LevelHost* H) {
  const int64_t na = l->num_accl, n = J.num_gyro;
  const int F = J.num_frames;
  const double off = J.P.time_offset, refd = J.P.reference_row * J.P.line_delay, reach = 3.0 * l->gravity_sigma_s;
  auto s = [&](int64_t j, int k) { return ((l->accl_t[j] - scene->frame_t[k]) + off) - refd; };
  H->frame_of.assign(size_t(na), -1); H->sample_interval.assign(size_t(na), 0);
  H->win_lo.assign(size_t(F), 0); H->win_hi.assign(size_t(F), -1);
  {
    const double* qi = scene->q_i_c;
    const double norm = std::sqrt(((qi[0] * qi[0] + qi[1] * qi[1]) + qi[2] * qi[2]) + qi[3] * qi[3]);
    const double w = qi[0] / norm, x = qi[1] / norm, y = qi[2] / norm, z = qi[3] / norm;
    H->Ric = Rotation{{1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                       2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
                       2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)}};
  }
  if (count < 1) return;
  const int last = first + count - 1;
  int64_t used_lo = na, used_hi = -1;
  for (int64_t j = 0; j < na; ++j) {
    if (!(s(j, first) >= 0.0) || s(j, last) > 0.0) continue;
    int b = first, e = last + 1;                                 // number of on-path frames with s_jk >= 0, from `first`
    while (b < e) { const int m = (b + e) / 2; if (s(j, m) >= 0.0) b = m + 1; else e = m; }
    const int k = b - 1;
    const double sj = s(j, k);
    auto tau = [&](int64_t i) { return ((scene->gyro_t[i] - scene->frame_t[k]) + off) - refd; };
    int64_t gb = 0, ge = n;                                      // number of gyro samples with tau_i <= s_jk
    while (gb < ge) { const int64_t m = (gb + ge) / 2; if (tau(m) <= sj) gb = m + 1; else ge = m; }
    H->frame_of[size_t(j)] = k;
    H->sample_interval[size_t(j)] = std::max<int64_t>(std::min(gb - 1, n - 2), 0);
    used_lo = std::min(used_lo, j); used_hi = j;
  }
  for (int k = first; k <= last && used_hi >= used_lo; ++k) {
    int64_t b = used_lo, e = used_hi + 1;                        // the first used sample with s_jk >= -reach
    while (b < e) { const int64_t m = (b + e) / 2; if (s(m, k) < -reach) b = m + 1; else e = m; }
    const int64_t lo = b;
    b = used_lo; e = used_hi + 1;                                // the number of used samples with s_jk <= reach, from used_lo
    while (b < e) { const int64_t m = (b + e) / 2; if (s(m, k) <= reach) b = m + 1; else e = m; }
    H->win_lo[size_t(k)] = lo; H->win_hi[size_t(k)] = b - 1;
  }
}

// The device side of the horizon lock: the samples, what the host decided, the world vectors and the gate.
struct LevelDevice {
  oicc::DevBuf<double> accl_t, accl, world;
  oicc::DevBuf<int32_t> frame_of;
  oicc::DevBuf<int64_t> sample_interval, win_lo, win_hi;
  oicc::DevBuf<uint8_t> gate;
};

// uploads and G1: the path must be on the stream already
int launch_accl_world(const Judged& J, const oicc_stab_level* l, const LevelHost& H, hipStream_t st, const Prepared& D, const int64_t* d_interval,
                      const double* d_path, LevelDevice* V) {
  const size_t na = size_t(l->num_accl), f = size_t(J.num_frames);
  OICC_HIP_TRY(V->accl_t.resize(na)); OICC_HIP_TRY(V->accl.resize(3 * na)); OICC_HIP_TRY(V->world.resize(3 * na)); OICC_HIP_TRY(V->gate.resize(na));
  OICC_HIP_TRY(V->frame_of.resize(na)); OICC_HIP_TRY(V->sample_interval.resize(na)); OICC_HIP_TRY(V->win_lo.resize(f)); OICC_HIP_TRY(V->win_hi.resize(f));
  OICC_HIP_TRY(hipMemcpyAsync(V->accl_t.p, l->accl_t, sizeof(double) * na, hipMemcpyHostToDevice, st));
  OICC_HIP_TRY(hipMemcpyAsync(V->accl.p, l->accl, sizeof(double) * 3 * na, hipMemcpyHostToDevice, st));
  OICC_HIP_TRY(hipMemcpyAsync(V->frame_of.p, H.frame_of.data(), sizeof(int32_t) * na, hipMemcpyHostToDevice, st));
  OICC_HIP_TRY(hipMemcpyAsync(V->sample_interval.p, H.sample_interval.data(), sizeof(int64_t) * na, hipMemcpyHostToDevice, st));
  OICC_HIP_TRY(hipMemcpyAsync(V->win_lo.p, H.win_lo.data(), sizeof(int64_t) * f, hipMemcpyHostToDevice, st));
  OICC_HIP_TRY(hipMemcpyAsync(V->win_hi.p, H.win_hi.data(), sizeof(int64_t) * f, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(stab_accl_world_kernel, dim3(blocks_for(int64_t(na))), dim3(kThreads), 0, st, int64_t(na), V->accl_t.p, V->accl.p, V->frame_of.p,
                     V->sample_interval.p, D.gyro_t.p, D.rates.p, D.frame_t.p, d_interval, d_path, H.Ric, J.P.time_offset,
                     J.P.reference_row * J.P.line_delay, l->gravity_const, l->accl_gate, V->world.p, V->gate.p);
  OICC_HIP_TRY(hipGetLastError());
  return OICC_OK;
}

// What oicc_stab_plan_level returns on top of oicc_stab_plan
struct LevelOut {
  double *level_q, *up, *roll, *level_angle;
  int32_t *gravity_samples, *level_status;
};

// oicc_stab_plan (level and out null) and oicc_stab_plan_level; device_ms [3] or [5]
int plan_impl(int32_t device_ordinal, const oicc_rs_scene* scene, const oicc_stab_options* options, const oicc_stab_level* level, double* path_q,
              double* smooth_q, double* correction_q, double* required_zoom, double* zoom, int32_t* iterations, int32_t* frame_status,
              uint8_t* zoom_clamped, const LevelOut* out, double* device_ms) {
  Judged J;
  if (int rc = judge_scene(scene, &J)) return rc;
  if (!options_ok(options) || !path_q || !smooth_q || !correction_q || !required_zoom || !zoom || !iterations || !frame_status || !zoom_clamped)
    return OICC_ERR_INVALID_ARG;
  if (out && (!out->level_q || !out->up || !out->roll || !out->level_angle || !out->gravity_samples || !out->level_status)) return OICC_ERR_INVALID_ARG;
  if (level && !level_ok(level)) return OICC_ERR_INVALID_ARG;
  const int F = J.num_frames;
  const double sigma = options->smoothing_sigma_s;
  std::vector<int64_t> interval;
  int first = 0, count = 0;
  if (int rc = find_path(scene, J, &interval, &first, &count)) return rc;
  LevelHost H;
  if (level) level_host(scene, J, level, first, count, &H);
  // the smoothing windows, frame indices with both ends included: t_ref,m - t_ref,k = frame_t[m] - frame_t[k]
  std::vector<int32_t> win_lo(size_t(F), 0), win_hi(size_t(F), 0);
  {
    int lo = first, hi = first;
    for (int k = first; k < first + count; ++k) {
      while (scene->frame_t[k] - scene->frame_t[lo] > 3.0 * sigma) ++lo;
      if (hi < k) hi = k;
      while (hi + 1 < first + count && scene->frame_t[hi + 1] - scene->frame_t[k] <= 3.0 * sigma) ++hi;
      win_lo[size_t(k)] = lo; win_hi[size_t(k)] = hi;
    }
  }
  if (int rc = oicc::select_device(device_ordinal)) return rc;
  const double qnan = std::nan("");
  std::vector<double> h_path(size_t(4 * F), qnan), h_smooth(size_t(4 * F), qnan), h_corr(size_t(4 * F), 0.0), h_zoom(size_t(F), 1.0), h_req(size_t(F), qnan);
  std::vector<int32_t> h_iter(size_t(F), 0);
  for (int k = 0; k < F; ++k) h_corr[size_t(4 * k)] = 1.0;
  const int points = border_points(J.P.dst_w, J.P.dst_h);
  const int waves = int(blocks_for(points)) * kWaves;
  // the horizon lock's outputs as they are without a level: level_q = smooth_q (copied below), no up, no roll, angle 0
  std::vector<double> h_level, h_up(size_t(3 * F), qnan), h_roll(size_t(F), qnan), h_angle(size_t(F), 0.0);
  std::vector<int32_t> h_samples(size_t(F), 0), h_lstatus(size_t(F), level ? 2 : 0);
  float ms[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  {
    Prepared D;
    LevelDevice V;
    oicc::DevBuf<int64_t> d_interval;
    oicc::DevBuf<int32_t> d_lo, d_hi, d_iter, d_samples, d_lstatus;
    oicc::DevBuf<double> d_delta, d_path, d_smooth, d_wave, d_req, d_level, d_up, d_roll, d_angle;
    oicc::Event e1, e2, e3, g1, g2, g3;
    oicc::Stream st;
    OICC_HIP_TRY(st.create());
    OICC_HIP_TRY(e1.create()); OICC_HIP_TRY(e2.create()); OICC_HIP_TRY(e3.create());
    if (level) {
      OICC_HIP_TRY(g1.create()); OICC_HIP_TRY(g2.create()); OICC_HIP_TRY(g3.create());
      OICC_HIP_TRY(d_level.resize(size_t(4 * F))); OICC_HIP_TRY(d_up.resize(size_t(3 * F))); OICC_HIP_TRY(d_roll.resize(size_t(F)));
      OICC_HIP_TRY(d_angle.resize(size_t(F))); OICC_HIP_TRY(d_samples.resize(size_t(F))); OICC_HIP_TRY(d_lstatus.resize(size_t(F)));
    }
    OICC_HIP_TRY(d_interval.resize(size_t(F))); OICC_HIP_TRY(d_lo.resize(size_t(F))); OICC_HIP_TRY(d_hi.resize(size_t(F)));
    OICC_HIP_TRY(d_iter.resize(size_t(F))); OICC_HIP_TRY(d_delta.resize(size_t(4 * std::max(count - 1, 1))));
    OICC_HIP_TRY(d_path.resize(size_t(4 * F))); OICC_HIP_TRY(d_smooth.resize(size_t(4 * F)));
    OICC_HIP_TRY(d_wave.resize(size_t(F) * size_t(waves))); OICC_HIP_TRY(d_req.resize(size_t(F)));
    if (int rc = upload_scene(scene, J, st, &D)) return rc;
    OICC_HIP_TRY(hipMemcpyAsync(d_interval.p, interval.data(), sizeof(int64_t) * size_t(F), hipMemcpyHostToDevice, st));
    OICC_HIP_TRY(hipMemcpyAsync(d_lo.p, win_lo.data(), sizeof(int32_t) * size_t(F), hipMemcpyHostToDevice, st));
    OICC_HIP_TRY(hipMemcpyAsync(d_hi.p, win_hi.data(), sizeof(int32_t) * size_t(F), hipMemcpyHostToDevice, st));
    OICC_HIP_TRY(hipMemcpyAsync(d_iter.p, h_iter.data(), sizeof(int32_t) * size_t(F), hipMemcpyHostToDevice, st));
    OICC_HIP_TRY(hipMemcpyAsync(d_path.p, h_path.data(), sizeof(double) * size_t(4 * F), hipMemcpyHostToDevice, st));
    OICC_HIP_TRY(hipMemcpyAsync(d_smooth.p, h_smooth.data(), sizeof(double) * size_t(4 * F), hipMemcpyHostToDevice, st));
    OICC_HIP_TRY(hipMemcpyAsync(D.correction.p, h_corr.data(), sizeof(double) * size_t(4 * F), hipMemcpyHostToDevice, st));
    OICC_HIP_TRY(hipMemcpyAsync(D.zoom.p, h_zoom.data(), sizeof(double) * size_t(F), hipMemcpyHostToDevice, st));
    if (int rc = launch_tables(J, st, &D)) return rc;          // ev[1]: the path starts here
    if (int rc = launch_path(J, st, D, d_interval.p, first, count, d_delta.p, d_path.p)) return rc;
    OICC_HIP_TRY(hipEventRecord(e1, st));
    if (count > 0) {
      hipLaunchKernelGGL(stab_smooth_kernel, dim3(unsigned((count + kWaves - 1) / kWaves)), dim3(kThreads), 0, st, count, first, D.frame_t.p, d_path.p, d_lo.p,
                         d_hi.p, sigma, options->max_correction_rad, d_smooth.p, D.correction.p, d_iter.p);
      OICC_HIP_TRY(hipGetLastError());
    }
    OICC_HIP_TRY(hipEventRecord(e2, st));
    if (level) {                                               // between the smoothing and the zoom: device_ms [3] and [4]
      // level_q starts as smooth_q (NaN off the path), the rest as without gravity
      OICC_HIP_TRY(hipMemcpyAsync(d_level.p, d_smooth.p, sizeof(double) * size_t(4 * F), hipMemcpyDeviceToDevice, st));
      OICC_HIP_TRY(hipMemcpyAsync(d_up.p, h_up.data(), sizeof(double) * size_t(3 * F), hipMemcpyHostToDevice, st));
      OICC_HIP_TRY(hipMemcpyAsync(d_roll.p, h_roll.data(), sizeof(double) * size_t(F), hipMemcpyHostToDevice, st));
      OICC_HIP_TRY(hipMemcpyAsync(d_angle.p, h_angle.data(), sizeof(double) * size_t(F), hipMemcpyHostToDevice, st));
      OICC_HIP_TRY(hipMemcpyAsync(d_samples.p, h_samples.data(), sizeof(int32_t) * size_t(F), hipMemcpyHostToDevice, st));
      OICC_HIP_TRY(hipMemcpyAsync(d_lstatus.p, h_lstatus.data(), sizeof(int32_t) * size_t(F), hipMemcpyHostToDevice, st));
      OICC_HIP_TRY(hipEventRecord(g1, st));
      if (int rc = launch_accl_world(J, level, H, st, D, d_interval.p, d_path.p, &V)) return rc;
      OICC_HIP_TRY(hipEventRecord(g2, st));
      if (count > 0) {
        hipLaunchKernelGGL(stab_level_kernel, dim3(unsigned((count + kWaves - 1) / kWaves)), dim3(kThreads), 0, st, count, first, D.frame_t.p, V.accl_t.p,
                           V.world.p, V.gate.p, V.win_lo.p, V.win_hi.p, d_path.p, d_smooth.p, J.P.time_offset, J.P.reference_row * J.P.line_delay,
                           level->gravity_sigma_s, level->gravity_const, level->lock, std::remainder(level->roll_rad, kTwoPi),
                           options->max_correction_rad, d_level.p, D.correction.p, d_up.p, d_roll.p, d_angle.p, d_samples.p, d_lstatus.p);
        OICC_HIP_TRY(hipGetLastError());
      }
      OICC_HIP_TRY(hipEventRecord(g3, st));                    // the zoom starts here
    }
    if (int rc = launch_records(J, st, &D)) return rc;         // at zoom 1
    for (int f0 = 0; f0 < F; f0 += kFrameChunk) {
      const int m = std::min(kFrameChunk, F - f0);
      hipLaunchKernelGGL(stab_zoom_kernel, dim3(blocks_for(points), unsigned(m)), dim3(kThreads), 0, st, J.P, f0, D.table.p, D.count.p, D.record.p, points,
                         waves, d_wave.p);
      OICC_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(stab_zoom_min_kernel, dim3(unsigned((F + 63) / 64)), dim3(64), 0, st, F, waves, d_wave.p, d_req.p);
    OICC_HIP_TRY(hipGetLastError());
    OICC_HIP_TRY(hipEventRecord(e3, st));
    OICC_HIP_TRY(hipMemcpyAsync(h_path.data(), d_path.p, sizeof(double) * size_t(4 * F), hipMemcpyDeviceToHost, st));
    OICC_HIP_TRY(hipMemcpyAsync(h_smooth.data(), d_smooth.p, sizeof(double) * size_t(4 * F), hipMemcpyDeviceToHost, st));
    OICC_HIP_TRY(hipMemcpyAsync(h_corr.data(), D.correction.p, sizeof(double) * size_t(4 * F), hipMemcpyDeviceToHost, st));
    OICC_HIP_TRY(hipMemcpyAsync(h_iter.data(), d_iter.p, sizeof(int32_t) * size_t(F), hipMemcpyDeviceToHost, st));
    OICC_HIP_TRY(hipMemcpyAsync(h_req.data(), d_req.p, sizeof(double) * size_t(F), hipMemcpyDeviceToHost, st));
    if (level) {
      OICC_HIP_TRY(hipMemcpyAsync(h_up.data(), d_up.p, sizeof(double) * size_t(3 * F), hipMemcpyDeviceToHost, st));
      OICC_HIP_TRY(hipMemcpyAsync(h_roll.data(), d_roll.p, sizeof(double) * size_t(F), hipMemcpyDeviceToHost, st));
      OICC_HIP_TRY(hipMemcpyAsync(h_angle.data(), d_angle.p, sizeof(double) * size_t(F), hipMemcpyDeviceToHost, st));
      OICC_HIP_TRY(hipMemcpyAsync(h_samples.data(), d_samples.p, sizeof(int32_t) * size_t(F), hipMemcpyDeviceToHost, st));
      OICC_HIP_TRY(hipMemcpyAsync(h_lstatus.data(), d_lstatus.p, sizeof(int32_t) * size_t(F), hipMemcpyDeviceToHost, st));
      h_level.resize(size_t(4 * F));
      OICC_HIP_TRY(hipMemcpyAsync(h_level.data(), d_level.p, sizeof(double) * size_t(4 * F), hipMemcpyDeviceToHost, st));
    }
    OICC_HIP_TRY(hipStreamSynchronize(st));
    OICC_HIP_TRY(hipEventElapsedTime(&ms[0], D.ev[1], e1));
    OICC_HIP_TRY(hipEventElapsedTime(&ms[1], e1, e2));
    OICC_HIP_TRY(hipEventElapsedTime(&ms[2], level ? g3 : e2, e3));
    if (level) {
      OICC_HIP_TRY(hipEventElapsedTime(&ms[3], g1, g2));
      OICC_HIP_TRY(hipEventElapsedTime(&ms[4], g2, g3));
    }
  }
  std::memcpy(path_q, h_path.data(), sizeof(double) * size_t(4 * F));
  std::memcpy(smooth_q, h_smooth.data(), sizeof(double) * size_t(4 * F));
  std::memcpy(correction_q, h_corr.data(), sizeof(double) * size_t(4 * F));
  std::memcpy(iterations, h_iter.data(), sizeof(int32_t) * size_t(F));
  std::memcpy(required_zoom, h_req.data(), sizeof(double) * size_t(F));
  copy_status(J, frame_status);
  applied_zoom(F, scene->frame_t, required_zoom, frame_status, *options, zoom, zoom_clamped);
  if (device_ms) for (int k = 0; k < (out ? 5 : 3); ++k) device_ms[k] = double(ms[k]);
  if (out) {
    std::memcpy(out->level_q, level ? h_level.data() : h_smooth.data(), sizeof(double) * size_t(4 * F));
    std::memcpy(out->up, h_up.data(), sizeof(double) * size_t(3 * F));
    std::memcpy(out->roll, h_roll.data(), sizeof(double) * size_t(F));
    std::memcpy(out->level_angle, h_angle.data(), sizeof(double) * size_t(F));
    std::memcpy(out->gravity_samples, h_samples.data(), sizeof(int32_t) * size_t(F));
    std::memcpy(out->level_status, h_lstatus.data(), sizeof(int32_t) * size_t(F));
  }
  return OICC_OK;
}

}  // namespace

extern "C" int oicc_stab_plan(int32_t device_ordinal, const oicc_rs_scene* scene, const oicc_stab_options* options, double* path_q, double* smooth_q,
                              double* correction_q, double* required_zoom, double* zoom, int32_t* iterations, int32_t* frame_status,
                              uint8_t* zoom_clamped, double* device_ms) {
  return plan_impl(device_ordinal, scene, options, nullptr, path_q, smooth_q, correction_q, required_zoom, zoom, iterations, frame_status, zoom_clamped,
                   nullptr, device_ms);
}

extern "C" int oicc_stab_plan_level(int32_t device_ordinal, const oicc_rs_scene* scene, const oicc_stab_options* options, const oicc_stab_level* level,
                                    double* path_q, double* smooth_q, double* correction_q, double* required_zoom, double* zoom, int32_t* iterations,
                                    int32_t* frame_status, uint8_t* zoom_clamped, double* level_q, double* up, double* roll, double* level_angle,
                                    int32_t* gravity_samples, int32_t* level_status, double* device_ms) {
  const LevelOut out = {level_q, up, roll, level_angle, gravity_samples, level_status};
  return plan_impl(device_ordinal, scene, options, level, path_q, smooth_q, correction_q, required_zoom, zoom, iterations, frame_status, zoom_clamped,
                   &out, device_ms);
}

// G1 of the horizon lock alone: the path, then every accelerometer sample in the path's frame
extern "C" int oicc_debug_stab_accl_world(int32_t device_ordinal, const oicc_rs_scene* scene, const oicc_stab_level* level, double* world,
                                          int32_t* frame_of) {
  Judged J;
  if (int rc = judge_scene(scene, &J)) return rc;
  if (!level_ok(level) || !world || !frame_of) return OICC_ERR_INVALID_ARG;
  const int F = J.num_frames;
  std::vector<int64_t> interval;
  int first = 0, count = 0;
  if (int rc = find_path(scene, J, &interval, &first, &count)) return rc;
  LevelHost H;
  level_host(scene, J, level, first, count, &H);
  if (int rc = oicc::select_device(device_ordinal)) return rc;
  const size_t na = size_t(level->num_accl);
  const std::vector<double> h_path(size_t(4 * F), std::nan(""));
  Prepared D;
  LevelDevice V;
  oicc::DevBuf<int64_t> d_interval;
  oicc::DevBuf<double> d_delta, d_path;
  oicc::Stream st;
  OICC_HIP_TRY(st.create());
  OICC_HIP_TRY(d_interval.resize(size_t(F))); OICC_HIP_TRY(d_delta.resize(size_t(4 * std::max(count - 1, 1)))); OICC_HIP_TRY(d_path.resize(size_t(4 * F)));
  if (int rc = upload_scene(scene, J, st, &D)) return rc;
  OICC_HIP_TRY(hipMemcpyAsync(d_interval.p, interval.data(), sizeof(int64_t) * size_t(F), hipMemcpyHostToDevice, st));
  OICC_HIP_TRY(hipMemcpyAsync(d_path.p, h_path.data(), sizeof(double) * size_t(4 * F), hipMemcpyHostToDevice, st));
  if (int rc = launch_path(J, st, D, d_interval.p, first, count, d_delta.p, d_path.p)) return rc;
  if (int rc = launch_accl_world(J, level, H, st, D, d_interval.p, d_path.p, &V)) return rc;
  OICC_HIP_TRY(hipMemcpyAsync(world, V.world.p, sizeof(double) * 3 * na, hipMemcpyDeviceToHost, st));
  OICC_HIP_TRY(hipStreamSynchronize(st));
  std::memcpy(frame_of, H.frame_of.data(), sizeof(int32_t) * na);
  return OICC_OK;
}

// the zoom rule alone, host arithmetic only: what oicc_stab_plan applies to the required zoom it has measured
extern "C" int oicc_debug_stab_zoom(int32_t num_frames, const double* frame_t, const double* required_zoom, const int32_t* frame_status,
                                      const oicc_stab_options* options, double* zoom, uint8_t* zoom_clamped) {
  if (num_frames < 1 || !frame_t || !required_zoom || !frame_status || !options_ok(options) || !zoom || !zoom_clamped || !all_finite(frame_t, num_frames))
    return OICC_ERR_INVALID_ARG;
  for (int k = 1; k < num_frames; ++k) if (!(frame_t[k] > frame_t[k - 1])) return OICC_ERR_INVALID_ARG;
  for (int k = 0; k < num_frames; ++k) if (frame_status[k] == 0 && std::isnan(required_zoom[k])) return OICC_ERR_INVALID_ARG;
  applied_zoom(num_frames, frame_t, required_zoom, frame_status, *options, zoom, zoom_clamped);
  return OICC_OK;
}

extern "C" int oicc_stab_map(int32_t device_ordinal, const oicc_rs_scene* scene, const double* correction_q, const double* zoom, float* map,
                             uint8_t* valid, uint8_t* evaluations, int32_t* frame_status, int64_t* num_valid, double* device_ms) {
  Judged J;
  if (int rc = judge_scene(scene, &J)) return rc;
  if (!plan_arrays_ok(correction_q, zoom, J.num_frames) || !map || !valid || !frame_status) return OICC_ERR_INVALID_ARG;
  if (int rc = oicc::select_device(device_ordinal)) return rc;
  const int64_t pixels = int64_t(J.P.dst_w) * J.P.dst_h;
  const size_t total = size_t(pixels) * size_t(J.num_frames);
  Prepared D;
  oicc::DevBuf<float2> d_map; oicc::DevBuf<uint8_t> d_valid, d_evals;
  oicc::Event e1;
  oicc::Stream st;
  float ms[3] = {0.0f, 0.0f, 0.0f};
  OICC_HIP_TRY(st.create());
  OICC_HIP_TRY(e1.create());
  OICC_HIP_TRY(d_map.resize(total));
  OICC_HIP_TRY(d_valid.resize(total));
  if (evaluations) OICC_HIP_TRY(d_evals.resize(total));
  if (int rc = prepare(scene, J, correction_q, zoom, st, &D)) return rc;
  for (int first = 0; first < J.num_frames; first += kFrameChunk) {
    const int m = std::min(kFrameChunk, J.num_frames - first);
    hipLaunchKernelGGL(stab_map_kernel, dim3(blocks_for(pixels), unsigned(m)), dim3(kThreads), 0, st, J.P, first, D.table.p, D.count.p, D.record.p, pixels,
                       d_map.p, d_valid.p, d_evals.p);
    OICC_HIP_TRY(hipGetLastError());
  }
  OICC_HIP_TRY(hipEventRecord(e1, st));
  OICC_HIP_TRY(hipMemcpyAsync(map, d_map.p, sizeof(float2) * total, hipMemcpyDeviceToHost, st));
  OICC_HIP_TRY(hipMemcpyAsync(valid, d_valid.p, total, hipMemcpyDeviceToHost, st));
  if (evaluations) OICC_HIP_TRY(hipMemcpyAsync(evaluations, d_evals.p, total, hipMemcpyDeviceToHost, st));
  OICC_HIP_TRY(hipStreamSynchronize(st));
  OICC_HIP_TRY(hipEventElapsedTime(&ms[0], D.ev[0], D.ev[1]));
  OICC_HIP_TRY(hipEventElapsedTime(&ms[1], D.ev[1], D.ev[2]));
  OICC_HIP_TRY(hipEventElapsedTime(&ms[2], D.ev[2], e1));
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

extern "C" int oicc_stab_frames_device(void* hip_stream, const oicc_rs_scene* scene, const double* correction_q, const double* zoom, int32_t channels,
                                       const uint8_t* frames_dev, int32_t border_value, uint8_t* out_dev, int32_t* frame_status) {
  Judged J;
  if (int rc = judge_scene(scene, &J)) return rc;
  if (!plan_arrays_ok(correction_q, zoom, J.num_frames) || !frames_args_ok(channels, border_value) || !frames_dev || !out_dev || !frame_status)
    return OICC_ERR_INVALID_ARG;
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  if (int rc = oicc::on_current_device(stream, {frames_dev, out_dev})) return rc;
  Prepared D;
  int rc = prepare(scene, J, correction_q, zoom, stream, &D);
  if (rc == OICC_OK) rc = launch_frames(stream, J, D, 0, J.num_frames, channels, frames_dev, border_value, out_dev);
  // the tables and records are this call's own: it returns once the stream has run the work, and frees them
  if (hipStreamSynchronize(stream) != hipSuccess && rc == OICC_OK) rc = OICC_ERR_HIP;
  if (rc == OICC_OK) copy_status(J, frame_status);
  return rc;
}

extern "C" int oicc_stab_frames(int32_t device_ordinal, const oicc_rs_scene* scene, const double* correction_q, const double* zoom, int32_t channels,
                                const uint8_t* frames, int32_t border_value, int32_t batch, uint8_t* out, int32_t* frame_status,
                                oicc_rs_frames_report* report) {
  Judged J;
  if (int rc = judge_scene(scene, &J)) return rc;
  if (!plan_arrays_ok(correction_q, zoom, J.num_frames) || !frames_args_ok(channels, border_value) || batch < 1 || !frames || !out || !frame_status)
    return OICC_ERR_INVALID_ARG;
  if (int rc = oicc::select_device(device_ordinal)) return rc;
  const auto t_start = std::chrono::steady_clock::now();
  oicc_rs_frames_report rep = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  Prepared D;
  FramePipeline pipe;      // behind the tables: its streams are drained before the tables go
  if (int rc = pipe.open(J.num_frames, batch, int64_t(J.P.src_w) * J.P.src_h * channels, int64_t(J.P.dst_w) * J.P.dst_h * channels)) return rc;
  if (int rc = prepare(scene, J, correction_q, zoom, pipe.slot[0].st, &D)) return rc;
  OICC_HIP_TRY(hipStreamSynchronize(pipe.slot[0].st));      // both streams read the tables and records
  float ms = 0.0f;
  OICC_HIP_TRY(hipEventElapsedTime(&ms, D.ev[0], D.ev[1])); rep.ms_table = ms;
  OICC_HIP_TRY(hipEventElapsedTime(&ms, D.ev[1], D.ev[2])); rep.ms_rays = ms;      // here: the record kernel
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
