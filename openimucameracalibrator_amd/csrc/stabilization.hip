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
#include <cmath>
#include <cstdint>
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
// What the host decides by time comparisons (the path, the smoothing and gravity windows), the applied zoom and the argument checks
// are gyro_scene_host.h's; the scene stage and the drivers of the three output entries are rolling_shutter_device.h's.

// the rolling-shutter judgement and the two further requirements of the stabilisation
int judge_scene(const oicc_rs_scene* s, Judged* J) {
  if (int rc = judge(s, J)) return rc;
  if (!J->P.dst_closed_form) return OICC_ERR_INVALID_ARG;
  for (int k = 1; k < s->num_frames; ++k) if (!(s->frame_t[k] > s->frame_t[k - 1])) return OICC_ERR_INVALID_ARG;
  return OICC_OK;
}

int border_points(int w, int h) { return (w == 1 || h == 1) ? w * h : 2 * (w + h) - 4; }

// The device side of a scene with its plan: the per-frame tables and records.  The third stage is the record kernel from correction
// and zoom; the output drivers launch through map_chunk and frames_chunk.
struct Prepared {
  SceneStage scene;
  oicc::DevBuf<double> correction, zoom;
  oicc::DevBuf<StabRecord> record;

  int allocate(const Judged& J) {
    const size_t f = size_t(J.num_frames);
    if (int rc = scene.allocate(J)) return rc;
    OICC_HIP_TRY(correction.resize(4 * f)); OICC_HIP_TRY(zoom.resize(f)); OICC_HIP_TRY(record.resize(f));
    return OICC_OK;
  }

  // the records from correction and zoom, which the stream has been given before
  int launch_records(const Judged& J, hipStream_t st) {
    hipLaunchKernelGGL(stab_record_kernel, dim3(unsigned((J.num_frames + 63) / 64)), dim3(64), 0, st, J.num_frames, J.P.R, J.P.dst.in[0], J.P.dst.in[2],
                       correction.p, zoom.p, record.p);
    OICC_HIP_TRY(hipGetLastError());
    return OICC_OK;
  }

  // Enqueues the uploads, the table kernel and the record kernel on st; J, the scene arrays and the plan arrays must outlive the work.
  int prepare(const oicc_rs_scene* s, const Judged& J, const double* correction_q, const double* zoom_in, hipStream_t st) {
    const size_t f = size_t(J.num_frames);
    if (int rc = allocate(J)) return rc;
    if (int rc = scene.upload(s, J, st)) return rc;
    OICC_HIP_TRY(correction.copy_from(correction_q, 4 * f, st));
    OICC_HIP_TRY(zoom.copy_from(zoom_in, f, st));
    if (int rc = scene.launch_tables(J, st)) return rc;
    if (int rc = launch_records(J, st)) return rc;
    OICC_HIP_TRY(hipEventRecord(scene.ev[2], st));
    return OICC_OK;
  }

  void map_chunk(hipStream_t st, const Judged& J, int first, int m, float2* map, uint8_t* valid, uint8_t* evaluations) const {
    hipLaunchKernelGGL(stab_map_kernel, dim3(blocks_for(J.pixels()), unsigned(m)), dim3(kThreads), 0, st, J.P, first, scene.table.p, scene.count.p, record.p,
                       J.pixels(), map, valid, evaluations);
  }

  void frames_chunk(hipStream_t st, const Judged& J, int first, int m, int channels, const uint8_t* in, int border, uint8_t* out) const {
    const int64_t pixels = J.pixels();
    const dim3 grid(blocks_for(pixels), unsigned(m));
    if (channels == 1)
      hipLaunchKernelGGL(stab_frames_kernel<1>, grid, dim3(kThreads), 0, st, J.P, first, scene.table.p, scene.count.p, record.p, pixels, in, border, out);
    else
      hipLaunchKernelGGL(stab_frames_kernel<3>, grid, dim3(kThreads), 0, st, J.P, first, scene.table.p, scene.count.p, record.p, pixels, in, border, out);
  }
};

// A host array and its device twin of the same size: the array as it is before a kernel writes it goes up, the result comes down.
// An empty one (a stage that does not run) allocates and copies nothing.
template <class T>
struct Twin {
  std::vector<T> h;
  oicc::DevBuf<T> d;
  bool alloc() { return d.resize(h.size()); }
  bool up(hipStream_t st) { return h.empty() || d.copy_from(h, st); }
  bool down(hipStream_t st) { return h.empty() || d.download(h.data(), h.size(), st); }
};

// What oicc_stab_plan_level returns on top of oicc_stab_plan
struct LevelOut {
  double *level_q, *up, *roll, *level_angle;
  int32_t *gravity_samples, *level_status;
};

// One plan: what the host decided, the host arrays that asynchronous copies read or write, the device buffers, the events, and the
// stream LAST, so that every way out drains it before anything declared above it goes (hip_resources.h, the order rule).  open()
// makes every allocation; the stages behind it only queue work on st.
struct Plan {
  int F = 0, first = 0, count = 0;                 // frames; the on-path frames [first, first + count)
  int points = 0, waves = 0;                       // border points of the destination and the waves that march them
  Twin<int64_t> interval;                          // [frames] the gyro interval of t_ref
  Twin<int32_t> lo, hi, iter;                      // [frames] the smoothing windows, the iterations of the mean
  Twin<double> path, smooth, req;                  // [frames][4], [frames][4], [frames]
  std::vector<double> h_corr, h_zoom;              // [frames][4], [frames]: their device twins are D's
  Twin<int32_t> frame_of;                          // the horizon lock, as level_windows decides: [na]
  Twin<int64_t> sample_interval, g_lo, g_hi;       // [na], [frames], [frames]
  Rotation Ric;                                    // R(q_i_c)
  Twin<double> level, up, roll, angle;             // its outputs: [frames][4], [frames][3], [frames], [frames]
  Twin<int32_t> samples, lstatus;
  Prepared D;
  oicc::DevBuf<double> delta, wave, accl_t, accl, world;
  oicc::DevBuf<uint8_t> gate;
  oicc::Event e1, e2, e3, g1, g2, g3;              // behind the path, the smoothing and the zoom; before G1, behind it, behind G2
  float ms[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  oicc::Stream st;

  // The path and, with a level, each sample's frame and interval and the gravity windows: host only, before a device is looked for.
  int decide_path(const oicc_rs_scene* scene, const Judged& J, const oicc_stab_level* l) {
    F = J.num_frames;
    interval.h.resize(size_t(F));
    if (int rc = find_path(J.num_gyro, scene->gyro_t, F, scene->frame_t, J.P.time_offset, reference_delay(J.P), interval.h.data(), &first, &count)) return rc;
    path.h.assign(size_t(4 * F), std::nan(""));
    if (!l) return OICC_OK;
    frame_of.h.resize(size_t(l->num_accl)); sample_interval.h.resize(size_t(l->num_accl)); g_lo.h.resize(size_t(F)); g_hi.h.resize(size_t(F));
    unit_rotation(scene->q_i_c, Ric.r);
    level_windows(J.num_gyro, scene->gyro_t, F, scene->frame_t, J.P.time_offset, reference_delay(J.P), l->num_accl, l->accl_t, l->gravity_sigma_s, first, count,
                  frame_of.h.data(), sample_interval.h.data(), g_lo.h.data(), g_hi.h.data());
    return OICC_OK;
  }

  // The smoothing windows and every array as it is before a kernel writes it: NaN smooth camera and required zoom, the identity as
  // correction, zoom 1, and the horizon lock's outputs as they are without gravity (no up, no roll, angle 0; status 2 with a level).
  void decide_fills(const oicc_rs_scene* scene, const Judged& J, double sigma, bool with_level) {
    const size_t f = size_t(F);
    const double qnan = std::nan("");
    lo.h.resize(f); hi.h.resize(f);
    smoothing_windows(F, scene->frame_t, first, count, sigma, lo.h.data(), hi.h.data());
    smooth.h.assign(4 * f, qnan); h_corr.assign(4 * f, 0.0); h_zoom.assign(f, 1.0); req.h.assign(f, qnan); iter.h.assign(f, 0);
    for (size_t k = 0; k < f; ++k) h_corr[4 * k] = 1.0;
    up.h.assign(3 * f, qnan); roll.h.assign(f, qnan); angle.h.assign(f, 0.0); samples.h.assign(f, 0); lstatus.h.assign(f, with_level ? 2 : 0);
    if (with_level) level.h.resize(4 * f);
    points = border_points(J.P.dst_w, J.P.dst_h);
    waves = int(blocks_for(points)) * kWaves;
  }

  // The stream and every allocation; whole: with the events of oicc_stab_plan's spans.  What decide_fills has not sized stays empty.
  int open(const Judged& J, const oicc_stab_level* l, bool whole) {
    OICC_HIP_TRY(st.create());
    if (whole) for (oicc::Event* e : {&e1, &e2, &e3}) OICC_HIP_TRY(e->create());
    if (whole && l) for (oicc::Event* e : {&g1, &g2, &g3}) OICC_HIP_TRY(e->create());
    if (l) for (Twin<double>* t : {&level, &up, &roll, &angle}) OICC_HIP_TRY(t->alloc());
    if (l) for (Twin<int32_t>* t : {&samples, &lstatus, &frame_of}) OICC_HIP_TRY(t->alloc());
    for (Twin<int32_t>* t : {&lo, &hi, &iter}) OICC_HIP_TRY(t->alloc());
    for (Twin<int64_t>* t : {&interval, &sample_interval, &g_lo, &g_hi}) OICC_HIP_TRY(t->alloc());
    for (Twin<double>* t : {&path, &smooth, &req}) OICC_HIP_TRY(t->alloc());
    OICC_HIP_TRY(delta.resize(size_t(4 * std::max(count - 1, 1)))); OICC_HIP_TRY(wave.resize(size_t(F) * size_t(waves)));
    if (int rc = D.allocate(J)) return rc;
    if (!l) return OICC_OK;
    const size_t na = size_t(l->num_accl);
    OICC_HIP_TRY(accl_t.resize(na)); OICC_HIP_TRY(accl.resize(3 * na)); OICC_HIP_TRY(world.resize(3 * na)); OICC_HIP_TRY(gate.resize(na));
    return OICC_OK;
  }

  // the scene and the initial fills; the debug entry has the path's alone
  int upload(const oicc_rs_scene* scene, const Judged& J) {
    if (int rc = D.scene.upload(scene, J, st)) return rc;
    OICC_HIP_TRY(interval.up(st)); OICC_HIP_TRY(lo.up(st)); OICC_HIP_TRY(hi.up(st)); OICC_HIP_TRY(iter.up(st)); OICC_HIP_TRY(path.up(st)); OICC_HIP_TRY(smooth.up(st));
    if (!h_corr.empty()) { OICC_HIP_TRY(D.correction.copy_from(h_corr, st)); OICC_HIP_TRY(D.zoom.copy_from(h_zoom, st)); }
    return OICC_OK;
  }

  // the delta and the scan kernel: path.d [frames][4] gets the on-path frames
  int path_stage(const Judged& J) {
    if (count < 1) return OICC_OK;
    if (count > 1) {
      hipLaunchKernelGGL(stab_path_delta_kernel, dim3(blocks_for(count - 1)), dim3(kThreads), 0, st, count - 1, first, D.scene.gyro_t.p, D.scene.rates.p,
                         D.scene.frame_t.p, interval.d.p, J.P.time_offset, reference_delay(J.P), delta.p);
      OICC_HIP_TRY(hipGetLastError());
    }
    const int run = std::max(kMinRun, (count + kScanLanes - 1) / kScanLanes);
    hipLaunchKernelGGL(stab_path_scan_kernel, dim3(1), dim3(kScanLanes), 0, st, count, run, delta.p, path.d.p + 4 * size_t(first));
    OICC_HIP_TRY(hipGetLastError());
    return OICC_OK;
  }

  int smooth_stage(const oicc_stab_options* o) {
    if (count < 1) return OICC_OK;
    hipLaunchKernelGGL(stab_smooth_kernel, dim3(unsigned((count + kWaves - 1) / kWaves)), dim3(kThreads), 0, st, count, first, D.scene.frame_t.p, path.d.p,
                       lo.d.p, hi.d.p, o->smoothing_sigma_s, o->max_correction_rad, smooth.d.p, D.correction.p, iter.d.p);
    OICC_HIP_TRY(hipGetLastError());
    return OICC_OK;
  }

  // the samples and what the host decided for them go up, then G1: the path must be on the stream already
  int accl_world_stage(const Judged& J, const oicc_stab_level* l) {
    const size_t na = size_t(l->num_accl);
    OICC_HIP_TRY(accl_t.copy_from(l->accl_t, na, st)); OICC_HIP_TRY(accl.copy_from(l->accl, 3 * na, st));
    OICC_HIP_TRY(frame_of.up(st)); OICC_HIP_TRY(sample_interval.up(st)); OICC_HIP_TRY(g_lo.up(st)); OICC_HIP_TRY(g_hi.up(st));
    hipLaunchKernelGGL(stab_accl_world_kernel, dim3(blocks_for(int64_t(na))), dim3(kThreads), 0, st, int64_t(na), accl_t.p, accl.p, frame_of.d.p,
                       sample_interval.d.p, D.scene.gyro_t.p, D.scene.rates.p, D.scene.frame_t.p, interval.d.p, path.d.p, Ric, J.P.time_offset,
                       reference_delay(J.P), l->gravity_const, l->accl_gate, world.p, gate.p);
    OICC_HIP_TRY(hipGetLastError());
    return OICC_OK;
  }

  // between the smoothing and the zoom.  level_q starts as smooth_q (NaN off the path), the rest as without gravity; then G1 and G2
  int level_stage(const Judged& J, const oicc_stab_options* o, const oicc_stab_level* l) {
    OICC_HIP_TRY(hipMemcpyAsync(level.d.p, smooth.d.p, sizeof(double) * size_t(4 * F), hipMemcpyDeviceToDevice, st));
    OICC_HIP_TRY(up.up(st)); OICC_HIP_TRY(roll.up(st)); OICC_HIP_TRY(angle.up(st)); OICC_HIP_TRY(samples.up(st)); OICC_HIP_TRY(lstatus.up(st));
    OICC_HIP_TRY(hipEventRecord(g1, st));
    if (int rc = accl_world_stage(J, l)) return rc;
    OICC_HIP_TRY(hipEventRecord(g2, st));
    if (count > 0) {
      hipLaunchKernelGGL(stab_level_kernel, dim3(unsigned((count + kWaves - 1) / kWaves)), dim3(kThreads), 0, st, count, first, D.scene.frame_t.p, accl_t.p,
                         world.p, gate.p, g_lo.d.p, g_hi.d.p, path.d.p, smooth.d.p, J.P.time_offset, reference_delay(J.P), l->gravity_sigma_s,
                         l->gravity_const, l->lock, std::remainder(l->roll_rad, kTwoPi), o->max_correction_rad, level.d.p, D.correction.p, up.d.p,
                         roll.d.p, angle.d.p, samples.d.p, lstatus.d.p);
      OICC_HIP_TRY(hipGetLastError());
    }
    OICC_HIP_TRY(hipEventRecord(g3, st));                      // the zoom starts here
    return OICC_OK;
  }

  // the records at zoom 1, the march of every border point, the minimum per frame
  int zoom_stage(const Judged& J) {
    if (int rc = D.launch_records(J, st)) return rc;
    for (int f0 = 0; f0 < F; f0 += kFrameChunk) {
      const int m = std::min(kFrameChunk, F - f0);
      hipLaunchKernelGGL(stab_zoom_kernel, dim3(blocks_for(points), unsigned(m)), dim3(kThreads), 0, st, J.P, f0, D.scene.table.p, D.scene.count.p, D.record.p,
                         points, waves, wave.p);
      OICC_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(stab_zoom_min_kernel, dim3(unsigned((F + 63) / 64)), dim3(64), 0, st, F, waves, wave.p, req.d.p);
    OICC_HIP_TRY(hipGetLastError());
    return OICC_OK;
  }

  // the results into the host arrays, the wait, and the spans: path, smoothing, zoom, and with a level G1 and G2
  int download_stage(bool with_level) {
    OICC_HIP_TRY(path.down(st)); OICC_HIP_TRY(smooth.down(st)); OICC_HIP_TRY(D.correction.download(h_corr.data(), h_corr.size(), st));
    OICC_HIP_TRY(iter.down(st)); OICC_HIP_TRY(req.down(st));
    if (with_level) for (Twin<double>* t : {&up, &roll, &angle, &level}) OICC_HIP_TRY(t->down(st));
    if (with_level) for (Twin<int32_t>* t : {&samples, &lstatus}) OICC_HIP_TRY(t->down(st));
    OICC_HIP_TRY(hipStreamSynchronize(st));
    OICC_HIP_TRY(hipEventElapsedTime(&ms[0], D.scene.ev[1], e1));
    OICC_HIP_TRY(hipEventElapsedTime(&ms[1], e1, e2));
    OICC_HIP_TRY(hipEventElapsedTime(&ms[2], with_level ? g3 : e2, e3));
    if (with_level) { OICC_HIP_TRY(hipEventElapsedTime(&ms[3], g1, g2)); OICC_HIP_TRY(hipEventElapsedTime(&ms[4], g2, g3)); }
    return OICC_OK;
  }
};

template <class T>
void copy_out(T* to, const std::vector<T>& from) { std::memcpy(to, from.data(), sizeof(T) * from.size()); }

// oicc_stab_plan (level and out null) and oicc_stab_plan_level; device_ms [3] or [5].  Only an OK return touches the caller's arrays.
int plan_impl(int32_t device_ordinal, const oicc_rs_scene* scene, const oicc_stab_options* options, const oicc_stab_level* level, double* path_q,
              double* smooth_q, double* correction_q, double* required_zoom, double* zoom, int32_t* iterations, int32_t* frame_status,
              uint8_t* zoom_clamped, const LevelOut* out, double* device_ms) {
  Judged J;
  if (int rc = judge_scene(scene, &J)) return rc;
  if (!options_ok(options) || !path_q || !smooth_q || !correction_q || !required_zoom || !zoom || !iterations || !frame_status || !zoom_clamped)
    return OICC_ERR_INVALID_ARG;
  if (out && (!out->level_q || !out->up || !out->roll || !out->level_angle || !out->gravity_samples || !out->level_status)) return OICC_ERR_INVALID_ARG;
  if (level && !level_ok(level)) return OICC_ERR_INVALID_ARG;
  Plan p;
  if (int rc = p.decide_path(scene, J, level)) return rc;
  p.decide_fills(scene, J, options->smoothing_sigma_s, level != nullptr);
  if (int rc = oicc::select_device(device_ordinal)) return rc;
  if (int rc = p.open(J, level, true)) return rc;
  if (int rc = p.upload(scene, J)) return rc;
  if (int rc = p.D.scene.launch_tables(J, p.st)) return rc;          // ev[1]: the path starts here
  if (int rc = p.path_stage(J)) return rc;
  OICC_HIP_TRY(hipEventRecord(p.e1, p.st));
  if (int rc = p.smooth_stage(options)) return rc;
  OICC_HIP_TRY(hipEventRecord(p.e2, p.st));
  if (level) if (int rc = p.level_stage(J, options, level)) return rc;          // device_ms [3] and [4]
  if (int rc = p.zoom_stage(J)) return rc;
  OICC_HIP_TRY(hipEventRecord(p.e3, p.st));
  if (int rc = p.download_stage(level != nullptr)) return rc;
  copy_out(path_q, p.path.h); copy_out(smooth_q, p.smooth.h); copy_out(correction_q, p.h_corr); copy_out(iterations, p.iter.h); copy_out(required_zoom, p.req.h);
  copy_status(J, frame_status);
  applied_zoom(p.F, scene->frame_t, required_zoom, frame_status, *options, zoom, zoom_clamped);
  if (device_ms) for (int k = 0; k < (out ? 5 : 3); ++k) device_ms[k] = double(p.ms[k]);
  if (out) {
    copy_out(out->level_q, level ? p.level.h : p.smooth.h); copy_out(out->up, p.up.h); copy_out(out->roll, p.roll.h);
    copy_out(out->level_angle, p.angle.h); copy_out(out->gravity_samples, p.samples.h); copy_out(out->level_status, p.lstatus.h);
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

// G1 of the horizon lock alone: the plan's own path stage and G1 stage, then every accelerometer sample in the path's frame
extern "C" int oicc_debug_stab_accl_world(int32_t device_ordinal, const oicc_rs_scene* scene, const oicc_stab_level* level, double* world,
                                          int32_t* frame_of) {
  Judged J;
  if (int rc = judge_scene(scene, &J)) return rc;
  if (!level_ok(level) || !world || !frame_of) return OICC_ERR_INVALID_ARG;
  Plan p;
  if (int rc = p.decide_path(scene, J, level)) return rc;
  if (int rc = oicc::select_device(device_ordinal)) return rc;
  if (int rc = p.open(J, level, false)) return rc;
  if (int rc = p.upload(scene, J)) return rc;
  if (int rc = p.path_stage(J)) return rc;
  if (int rc = p.accl_world_stage(J, level)) return rc;
  OICC_HIP_TRY(p.world.download(world, 3 * size_t(level->num_accl), p.st));
  OICC_HIP_TRY(hipStreamSynchronize(p.st));
  copy_out(frame_of, p.frame_of.h);
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
  Prepared D;
  return run_map(device_ordinal, J, D, [&](hipStream_t st) { return D.prepare(scene, J, correction_q, zoom, st); }, map, valid, evaluations, frame_status,
                 num_valid, device_ms);
}

extern "C" int oicc_stab_frames_device(void* hip_stream, const oicc_rs_scene* scene, const double* correction_q, const double* zoom, int32_t channels,
                                       const uint8_t* frames_dev, int32_t border_value, uint8_t* out_dev, int32_t* frame_status) {
  Judged J;
  if (int rc = judge_scene(scene, &J)) return rc;
  if (!plan_arrays_ok(correction_q, zoom, J.num_frames) || !frames_args_ok(channels, border_value) || !frames_dev || !out_dev || !frame_status)
    return OICC_ERR_INVALID_ARG;
  Prepared D;
  return run_frames_device(static_cast<hipStream_t>(hip_stream), J, D, [&](hipStream_t st) { return D.prepare(scene, J, correction_q, zoom, st); }, channels,
                           frames_dev, border_value, out_dev, frame_status);
}

// the report's ms_rays is here the record kernel
extern "C" int oicc_stab_frames(int32_t device_ordinal, const oicc_rs_scene* scene, const double* correction_q, const double* zoom, int32_t channels,
                                const uint8_t* frames, int32_t border_value, int32_t batch, uint8_t* out, int32_t* frame_status,
                                oicc_rs_frames_report* report) {
  Judged J;
  if (int rc = judge_scene(scene, &J)) return rc;
  if (!plan_arrays_ok(correction_q, zoom, J.num_frames) || !frames_args_ok(channels, border_value) || batch < 1 || !frames || !out || !frame_status)
    return OICC_ERR_INVALID_ARG;
  Prepared D;
  return run_frames(device_ordinal, J, D, [&](hipStream_t st) { return D.prepare(scene, J, correction_q, zoom, st); }, channels, frames, border_value, batch,
                    out, frame_status, report);
}
