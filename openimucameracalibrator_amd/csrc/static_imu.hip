// Static multi-pose IMU intrinsics (applications/static_imu_calibration.cc, core::StaticImuCalibrator of the reference,
// restated from imu_tk): static-interval detection, the accelerometer fits and the gyroscope residuals on the device;
// the reference's sequential pieces on the host.
//   StaticIntervalsDetector     src/utils/imu_data_interval.cc:111-149   simu_norm / simu_edge_* kernels
//   MultiPosAccResidual         static_imu_calibrator.h:18-58            acc_row, simu_acc_lm_kernel (all thresholds)
//   MultiPosGyroResidual        static_imu_calibrator.h:60-140           simu_gyro_kernel (product-form RK4)
//   CalibrateAcc / AccGyro      src/core/static_imu_calibrator.cc:54-337 oicc_static_imu_calibrate (host)
//   InitialInterval, TimeToIndex, DataMean, DataVariance, ExtractIntervalsSamples: host, as the reference
//
// Detector: a workgroup stages 256 window centres plus a 2h halo in LDS; each lane sums its own window in the reference's
// sequential order.  The norm does not depend on the threshold, so one pass serves all ten.  Starts and ends of every
// threshold are compacted deterministically: per-workgroup counts of interval starts (wave ballots), a scan, then writes.
//
// Gyroscope: one RK4 step is linear in the quaternion, q <- A_k q, and the per-step renormalisation only rescales, which
// QuaternionToRotation's 1/|q|^2 removes.  A block is therefore the ordered product A_{S-1} ... A_0 applied to the
// identity quaternion, reduced as a tree over 256 lanes.  Derivative component c travels as the pair (A, dA/dtheta_c):
// (A2, D2)(A1, D1) = (A2 A1, D2 A1 + A2 D1).  One workgroup per (block, component).
//
// No atomics anywhere: repeated calls are bitwise identical.  No FMA contraction in this unit, so the detector's norms
// equal a sequential host restatement bit for bit (the reference's own compiler may contract).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>
#include "../../include/oicc_hip.h"
#include "hip_resources.h"
#include "lm_small.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxHalf = 512;          // largest half window (win_size <= 1025)
constexpr int kMaxTh = OICC_SIMU_THRESHOLDS;

__device__ __forceinline__ double wsum(double v) {   // xor butterfly: every lane ends with the same value
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- detector ---------------------------------------------------------------------------------------------------
// norms[i] = |DataVariance(acc, [i-h, i+h])| for the 256 centres i = h + 256 b + lane (DataMean / DataVariance of
// imu_data_interval.cc:35-61: sequential sums, then / n and / (n - 1)).
__global__ __launch_bounds__(kThreads) void simu_norm_kernel(const double* __restrict__ acc, int64_t n, int h, double* __restrict__ norms) {
  extern __shared__ double tile[];                       // [(256 + 2h)][3]
  const int64_t c0 = h + int64_t(blockIdx.x) * kThreads, s0 = c0 - h;
  const int W = kThreads + 2 * h;
  for (int k = threadIdx.x; k < 3 * W; k += kThreads) {
    const int64_t s = 3 * s0 + k;
    tile[k] = s < 3 * n ? acc[s] : 0.0;
  }
  __syncthreads();
  const int64_t i = c0 + threadIdx.x;
  if (i >= n - h) return;
  const int w = 2 * h + 1;
  const double* p = tile + 3 * threadIdx.x;
  double mx = 0.0, my = 0.0, mz = 0.0;
  for (int k = 0; k < w; ++k) { mx += p[3 * k]; my += p[3 * k + 1]; mz += p[3 * k + 2]; }
  mx /= double(w); my /= double(w); mz /= double(w);
  double vx = 0.0, vy = 0.0, vz = 0.0;
  for (int k = 0; k < w; ++k) {
    const double dx = p[3 * k] - mx, dy = p[3 * k + 1] - my, dz = p[3 * k + 2] - mz;
    vx += dx * dx; vy += dy * dy; vz += dz * dz;
  }
  vx /= double(w - 1); vy /= double(w - 1); vz /= double(w - 1);
  norms[i] = sqrt((vx * vx + vy * vy) + vz * vz);
}

struct Edges { bool rise, fall, last; };
__device__ __forceinline__ Edges simu_edges(const double* norms, int64_t i, int64_t n, int h, double th) {
  const bool valid = i < n - h;
  const bool f = valid && norms[i] < th;
  const bool fp = valid && i > h && norms[i - 1] < th;
  return Edges{f && !fp, valid && !f && fp, f && i == n - h - 1};
}

// counts[b][t] = interval starts among the centres of workgroup b
__global__ __launch_bounds__(kThreads) void simu_edge_count_kernel(const double* __restrict__ norms, int64_t n, int h, const double* __restrict__ th,
                                                                    int nt, int32_t* __restrict__ counts) {
  __shared__ int32_t wc[kMaxTh][kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i = h + int64_t(blockIdx.x) * kThreads + threadIdx.x;
  for (int t = 0; t < nt; ++t) {
    const unsigned long long m = __ballot(simu_edges(norms, i, n, h, th[t]).rise);
    if (lane == 0) wc[t][wave] = __popcll(m);
  }
  __syncthreads();
  if ((int)threadIdx.x < nt) {
    int32_t s = 0;
    for (int w = 0; w < kWaves; ++w) s += wc[threadIdx.x][w];
    counts[int64_t(blockIdx.x) * nt + threadIdx.x] = s;
  }
}

// exclusive scan over the workgroups, one thread per threshold, in block order
__global__ void simu_edge_scan_kernel(int32_t* __restrict__ counts, int64_t nb, int nt, int32_t* __restrict__ totals) {
  const int t = threadIdx.x;
  if (t >= nt) return;
  int32_t run = 0;
  for (int64_t b = 0; b < nb; ++b) { const int32_t c = counts[b * nt + t]; counts[b * nt + t] = run; run += c; }
  totals[t] = run;
}

// start k of threshold t -> starts[t][k]; its end -> ends[t][k]; k = starts before the centre (global)
__global__ __launch_bounds__(kThreads) void simu_edge_write_kernel(const double* __restrict__ norms, int64_t n, int h, const double* __restrict__ th,
                                                                    int nt, const int32_t* __restrict__ offs, int32_t cap,
                                                                    int32_t* __restrict__ starts, int32_t* __restrict__ ends) {
  __shared__ int32_t wc[kMaxTh][kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i = h + int64_t(blockIdx.x) * kThreads + threadIdx.x;
  unsigned long long masks[kMaxTh];
  for (int t = 0; t < nt; ++t) {
    masks[t] = __ballot(simu_edges(norms, i, n, h, th[t]).rise);
    if (lane == 0) wc[t][wave] = __popcll(masks[t]);
  }
  __syncthreads();
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  for (int t = 0; t < nt; ++t) {
    const Edges e = simu_edges(norms, i, n, h, th[t]);
    int64_t k = offs[int64_t(blockIdx.x) * nt + t];
    for (int w = 0; w < wave; ++w) k += wc[t][w];
    k += __popcll(masks[t] & below);                     // starts strictly before i
    int32_t* st = starts + int64_t(t) * cap;
    int32_t* en = ends + int64_t(t) * cap;
    if (e.rise && k < cap) st[k] = int32_t(i);
    if (e.fall && k >= 1 && k - 1 < cap) en[k - 1] = int32_t(i - 1);
    if (e.last) { const int64_t kk = k + (e.rise ? 1 : 0) - 1; if (kk >= 0 && kk < cap) en[kk] = int32_t(i); }
  }
}

// ---- accelerometer ----------------------------------------------------------------------------------------------
// ms = T K (Eigen's 3x3 product; the zero terms are exact) and c = ms (x - b) summed in column order
__device__ __host__ __forceinline__ void acc_row(const double* x, const double* p, double g_mag, double* r, double* J) {
  const double m0 = p[0], m1 = p[1], m2 = p[2], sx = p[3], sy = p[4], sz = p[5];
  const double u0 = x[0] - p[6], u1 = x[1] - p[7], u2 = x[2] - p[8];
  const double ms01 = -m0 * sy, ms02 = m1 * sz, ms12 = -m2 * sz;
  const double c0 = (sx * u0 + ms01 * u1) + ms02 * u2, c1 = sy * u1 + ms12 * u2, c2 = sz * u2;
  const double nrm = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
  *r = g_mag - nrm;
  if (J) {
    const double e0 = c0 / nrm, e1 = c1 / nrm, e2 = c2 / nrm;
    // dc/dtheta columns; dr/dtheta = -e . dc/dtheta
    J[0] = e0 * (sy * u1);
    J[1] = -e0 * (sz * u2);
    J[2] = e1 * (sz * u2);
    J[3] = -e0 * u0;
    J[4] = -(e0 * (-m0 * u1) + e1 * u1);
    J[5] = -((e0 * (m1 * u2) + e1 * (-m2 * u2)) + e2 * u2);
    J[6] = e0 * sx;
    J[7] = -(e0 * (m0 * sy) - e1 * sy);
    J[8] = -((e0 * (-m1 * sz) + e1 * (m2 * sz)) - e2 * sz);
  }
}

constexpr int kAccNH = 45;   // packed upper triangle of 9x9

// cost, H (packed), g over samples [0, num) of one problem; every thread of the workgroup gets the same values
__device__ void acc_normal_eq(const double* s, int64_t num, double g_mag, const double* p, bool jac, double* cost, double* H, double* g,
                              double (*red)[kAccNH + 10], double* res_out, double* jac_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double lc = 0.0, lH[kAccNH], lg[9];
  for (int k = 0; k < kAccNH; ++k) lH[k] = 0.0;
  for (int k = 0; k < 9; ++k) lg[k] = 0.0;
  for (int64_t j = threadIdx.x; j < num; j += kThreads) {
    double r, J[9];
    acc_row(s + 3 * j, p, g_mag, &r, jac ? J : nullptr);
    lc += r * r;
    if (res_out) res_out[j] = r;
    if (jac) {
      if (jac_out) for (int k = 0; k < 9; ++k) jac_out[9 * j + k] = J[k];
      int e = 0;
      for (int a = 0; a < 9; ++a) {
        lg[a] += J[a] * r;
        for (int b = a; b < 9; ++b) { lH[e] += J[a] * J[b]; ++e; }
      }
    }
  }
  const int nv = jac ? kAccNH + 10 : 1;
  for (int k = 0; k < nv; ++k) {
    const double v = wsum(k == 0 ? lc : (k <= 9 ? lg[k - 1] : lH[k - 10]));
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  double tot[kAccNH + 10];
  for (int k = 0; k < nv; ++k) { double v = red[0][k]; for (int w = 1; w < kWaves; ++w) v += red[w][k]; tot[k] = v; }
  __syncthreads();
  *cost = 0.5 * tot[0];
  if (jac) { for (int k = 0; k < 9; ++k) g[k] = tot[1 + k]; for (int k = 0; k < kAccNH; ++k) H[k] = tot[10 + k]; }
}

struct AccProblem { int64_t off, num; };

struct AccEval {
  const double* s; int64_t num; double g_mag; double (*red)[kAccNH + 10];
  __device__ bool operator()(const double* p, bool jac, double* cost, double* H, double* g) {
    acc_normal_eq(s, num, g_mag, p, jac, cost, H, g, red, nullptr, nullptr);
    return isfinite(*cost);
  }
};

// one workgroup = one threshold's whole LM loop
__global__ __launch_bounds__(kThreads) void simu_acc_lm_kernel(const double* __restrict__ samples, const AccProblem* __restrict__ probs, double g_mag,
                                                                const double* __restrict__ x0, oicc::BaLmOptions o, double* __restrict__ x_out,
                                                                double* __restrict__ cost_out, int32_t* __restrict__ iters_out,
                                                                int32_t* __restrict__ term_out) {
  __shared__ double red[kWaves][kAccNH + 10];
  const AccProblem pr = probs[blockIdx.x];
  double x[9];
  for (int k = 0; k < 9; ++k) x[k] = x0[k];
  AccEval ev{samples + 3 * pr.off, pr.num, g_mag, red};
  int iters = 0; double cost = 0.0;
  const int term = oicc::small_lm<9>(o, x, ev, &iters, &cost);
  if (threadIdx.x == 0) {
    for (int k = 0; k < 9; ++k) x_out[9 * blockIdx.x + k] = x[k];
    cost_out[blockIdx.x] = cost; iters_out[blockIdx.x] = iters; term_out[blockIdx.x] = term;
  }
}

__global__ __launch_bounds__(kThreads) void simu_acc_eval_kernel(const double* __restrict__ samples, int64_t num, double g_mag, const double* __restrict__ p,
                                                                  double* res, double* jac, double* out /* cost, g[9], H[45] */) {
  __shared__ double red[kWaves][kAccNH + 10];
  double pp[9], cost, H[kAccNH], g[9];
  for (int k = 0; k < 9; ++k) pp[k] = p[k];
  acc_normal_eq(samples, num, g_mag, pp, true, &cost, H, g, red, res, jac);
  if (threadIdx.x == 0) { out[0] = cost; for (int k = 0; k < 9; ++k) out[1 + k] = g[k]; for (int k = 0; k < kAccNH; ++k) out[10 + k] = H[k]; }
}

// ---- gyroscope --------------------------------------------------------------------------------------------------
struct Dd { double v, d; };
__device__ __forceinline__ Dd operator+(Dd a, Dd b) { return Dd{a.v + b.v, a.d + b.d}; }
__device__ __forceinline__ Dd operator-(Dd a, Dd b) { return Dd{a.v - b.v, a.d - b.d}; }
__device__ __forceinline__ Dd operator-(Dd a) { return Dd{-a.v, -a.d}; }
__device__ __forceinline__ Dd operator*(Dd a, Dd b) { return Dd{a.v * b.v, a.v * b.d + a.d * b.v}; }
__device__ __forceinline__ Dd operator*(double s, Dd b) { return Dd{s * b.v, s * b.d}; }

struct GyroParams { double p[12]; };
struct GyroBlock { int32_t i0, i1; double g0[3], g1[3]; };

// omega = T K (x - b) (UnbiasNormalize) with derivative along component c
__device__ __forceinline__ void gyro_omega(const Dd ms[3][3], const Dd b[3], const double* x, Dd w[3]) {
  const Dd u0 = Dd{x[0], 0.0} - b[0], u1 = Dd{x[1], 0.0} - b[1], u2 = Dd{x[2], 0.0} - b[2];
  for (int i = 0; i < 3; ++i) w[i] = (ms[i][0] * u0 + ms[i][1] * u1) + ms[i][2] * u2;
}

// 0.5 * Omega(w) q with Omega of ComputeOmegaSkew (gyro_integration.h)
__device__ __forceinline__ void half_skew(const Dd w[3], const Dd q[4], Dd k[4]) {
  k[0] = 0.5 * (((-w[0]) * q[1] - w[1] * q[2]) - w[2] * q[3]);
  k[1] = 0.5 * ((w[0] * q[0] + w[2] * q[2]) - w[1] * q[3]);
  k[2] = 0.5 * ((w[1] * q[0] - w[2] * q[1]) + w[0] * q[3]);
  k[3] = 0.5 * ((w[2] * q[0] + w[1] * q[1]) - w[0] * q[2]);
}

// QuatIntegrationStepRK4 without the normalisation: the image of q
__device__ __forceinline__ void rk4_apply(const Dd q[4], const Dd w0[3], const Dd w01[3], const Dd w1[3], double dt, Dd out[4]) {
  Dd k1[4], k2[4], k3[4], k4[4], t[4];
  half_skew(w0, q, k1);
  for (int i = 0; i < 4; ++i) t[i] = q[i] + (0.5 * dt) * k1[i];
  half_skew(w01, t, k2);
  for (int i = 0; i < 4; ++i) t[i] = q[i] + (0.5 * dt) * k2[i];
  half_skew(w01, t, k3);
  for (int i = 0; i < 4; ++i) t[i] = q[i] + dt * k3[i];
  half_skew(w1, t, k4);
  const double m1 = 1.0 / 6.0, m2 = 1.0 / 3.0;
  for (int i = 0; i < 4; ++i) out[i] = q[i] + dt * (((m1 * k1[i] + m2 * k2[i]) + m2 * k3[i]) + m1 * k4[i]);
}

constexpr int kPair = 32;   // A[16] then D[16], row-major

// grid (blocks, np): residuals [3 nb] (component 0 writes them), jac [3 nb][np]
__global__ __launch_bounds__(kThreads) void simu_gyro_kernel(const double* __restrict__ t_s, const double* __restrict__ gyro,
                                                              const GyroBlock* __restrict__ blocks, GyroParams gp, int optimize_bias, double gyro_dt,
                                                              int np, double* __restrict__ res, double* __restrict__ jac) {
  __shared__ double P[kThreads][kPair];
  const int bidx = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  const GyroBlock B = blocks[bidx];
  Dd th[12];
  for (int k = 0; k < 12; ++k) th[k] = Dd{gp.p[k], k == c ? 1.0 : 0.0};
  const Dd one{1.0, 0.0}, zero{0.0, 0.0};
  // T = [[1,-yz,zy],[xz,1,-zx],[-xy,yx,1]] (types.h:238-239), K = diag(s), ms = T K
  const Dd T[3][3] = {{one, -th[0], th[1]}, {th[3], one, -th[2]}, {-th[4], th[5], one}};
  Dd ms[3][3];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) ms[i][j] = T[i][j] * th[6 + j];
  Dd b[3];
  for (int k = 0; k < 3; ++k) b[k] = optimize_bias ? th[9 + k] : zero;

  const int64_t steps = (B.i0 >= 0 && B.i1 > B.i0) ? int64_t(B.i1 - B.i0) : 0;
  const int64_t cs = (steps + kThreads - 1) / kThreads;
  const int64_t k0 = std::min<int64_t>(int64_t(tid) * cs, steps), k1 = std::min<int64_t>(k0 + cs, steps);
  Dd A[16];
  for (int i = 0; i < 16; ++i) A[i] = (i % 5 == 0) ? one : zero;
  if (k0 < k1) {
    Dd w0[3], w1[3];
    gyro_omega(ms, b, gyro + 3 * (int64_t(B.i0) + k0), w0);
    for (int64_t k = k0; k < k1; ++k) {
      const int64_t s = int64_t(B.i0) + k;
      gyro_omega(ms, b, gyro + 3 * (s + 1), w1);
      const double dt = gyro_dt > 0.0 ? gyro_dt : t_s[s + 1] - t_s[s];
      Dd w01[3];
      for (int i = 0; i < 3; ++i) w01[i] = 0.5 * (w0[i] + w1[i]);
      Dd Ak[16];
      for (int j = 0; j < 4; ++j) {            // column j = the image of the basis quaternion e_j
        Dd e[4] = {zero, zero, zero, zero}, col[4];
        e[j] = one;
        rk4_apply(e, w0, w01, w1, dt, col);
        for (int i = 0; i < 4; ++i) Ak[4 * i + j] = col[i];
      }
      Dd N[16];
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) N[4 * i + j] = ((Ak[4 * i] * A[j] + Ak[4 * i + 1] * A[4 + j]) + Ak[4 * i + 2] * A[8 + j]) + Ak[4 * i + 3] * A[12 + j];
      for (int i = 0; i < 16; ++i) A[i] = N[i];
      for (int i = 0; i < 3; ++i) w0[i] = w1[i];
    }
  }
  for (int i = 0; i < 16; ++i) { P[tid][i] = A[i].v; P[tid][16 + i] = A[i].d; }
  __syncthreads();
  // ordered tree: the later chunk multiplies from the left
  for (int s = 1; s < kThreads; s <<= 1) {
    if ((tid % (2 * s)) == 0) {
      const double* L = P[tid + s];   // later steps
      const double* R = P[tid];
      double NA[16], ND[16];
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
          double a = 0.0, d = 0.0;
          for (int k = 0; k < 4; ++k) { a += L[4 * i + k] * R[4 * k + j]; d += L[16 + 4 * i + k] * R[4 * k + j] + L[4 * i + k] * R[16 + 4 * k + j]; }
          NA[4 * i + j] = a; ND[4 * i + j] = d;
        }
      for (int i = 0; i < 16; ++i) { P[tid][i] = NA[i]; P[tid][16 + i] = ND[i]; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    // q = A e_0 with its derivative; ceres::QuaternionToRotation (scaled by 1 / |q|^2)
    const Dd a{P[0][0], P[0][16]}, bq{P[0][4], P[0][20]}, cq{P[0][8], P[0][24]}, dq{P[0][12], P[0][28]};
    const Dd aa = a * a, ab = a * bq, ac = a * cq, ad = a * dq, bb = bq * bq, bc = bq * cq, bd = bq * dq, cc = cq * cq, cd = cq * dq, dd = dq * dq;
    Dd R[3][3];
    R[0][0] = ((aa + bb) - cc) - dd; R[0][1] = 2.0 * (bc - ad);          R[0][2] = 2.0 * (ac + bd);
    R[1][0] = 2.0 * (ad + bc);       R[1][1] = ((aa - bb) + cc) - dd;    R[1][2] = 2.0 * (cd - ab);
    R[2][0] = 2.0 * (bd - ac);       R[2][1] = 2.0 * (ab + cd);          R[2][2] = ((aa - bb) - cc) + dd;
    const Dd q2 = ((aa + bb) + cc) + dd;
    const Dd inv{1.0 / q2.v, -q2.d / (q2.v * q2.v)};
    for (int i = 0; i < 3; ++i) {
      Dd v = (Dd{B.g0[0], 0.0} * (R[0][i] * inv) + Dd{B.g0[1], 0.0} * (R[1][i] * inv)) + Dd{B.g0[2], 0.0} * (R[2][i] * inv);
      v = v - Dd{B.g1[i], 0.0};
      if (c == 0 && res) res[3 * bidx + i] = v.v;
      if (jac) jac[int64_t(3 * bidx + i) * np + c] = v.d;
    }
  }
}

// ---- host helpers -----------------------------------------------------------------------------------------------
int time_to_index(const double* t, int64_t n, double ts) {   // DataInterval::TimeToIndex (imu_data_interval.h)
  int idx0 = 0, idx1 = int(n) - 1, idxm;
  while (idx1 - idx0 > 1) { idxm = (idx1 + idx0) / 2; if (ts > t[idxm]) idx0 = idxm; else idx1 = idxm; }
  return (ts - t[idx0] < t[idx1] - ts) ? idx0 : idx1;
}
int initial_interval_end(const double* t, int64_t n, double duration) {   // DataInterval::InitialInterval
  const double end_ts = t[0] + duration;
  return end_ts >= t[n - 1] ? int(n) - 1 : time_to_index(t, n, end_ts);
}
void data_mean(const double* x, int s, int e, double m[3]) {
  m[0] = m[1] = m[2] = 0.0;
  for (int i = s; i <= e; ++i) for (int c = 0; c < 3; ++c) m[c] += x[3 * int64_t(i) + c];
  for (int c = 0; c < 3; ++c) m[c] /= double(e - s + 1);
}
void data_variance(const double* x, int s, int e, double v[3]) {
  double m[3];
  data_mean(x, s, e, m);
  v[0] = v[1] = v[2] = 0.0;
  for (int i = s; i <= e; ++i) for (int c = 0; c < 3; ++c) { const double d = x[3 * int64_t(i) + c] - m[c]; v[c] += d * d; }
  for (int c = 0; c < 3; ++c) v[c] /= double(e - s);
}
int normalized_win(int w) { if (w < 11) w = 11; if (!(w % 2)) w++; return w; }

using oicc::select_device;

// The detector on device memory d_acc [n][3]: per threshold the interval list.  ms: device time.
int run_detector(const double* d_acc, int64_t n, int w, int nt, const double* th, std::vector<std::vector<int32_t>>* out,
                 double* norms_host, double* ms, hipStream_t st) {
  const int h = w / 2;
  out->assign(size_t(nt), {});
  if (w >= n) { if (norms_host) for (int64_t i = 0; i < n; ++i) norms_host[i] = std::nan(""); return OICC_OK; }   // .cc:119
  const int64_t M = n - 2 * int64_t(h), nb = (M + kThreads - 1) / kThreads;
  const int64_t cap = (M + 1) / 2 + 1;
  oicc::DevBuf<double> d_norm, d_th;
  oicc::DevBuf<int32_t> d_cnt, d_tot, d_st, d_en;
  oicc::Event e0, e1;
  std::vector<int32_t> tot(size_t(nt), 0);
  oicc::DrainOnExit drain{st};      // st is the caller's: no way out of here leaves work on it that uses the buffers above
  float f = 0.0f;
  const size_t lds = sizeof(double) * 3 * size_t(kThreads + 2 * h);
  OICC_HIP_TRY(e0.create()); OICC_HIP_TRY(e1.create());
  OICC_HIP_TRY(d_norm.resize(size_t(n))); OICC_HIP_TRY(d_th.resize(size_t(nt)));
  OICC_HIP_TRY(d_cnt.resize(size_t(nb * nt))); OICC_HIP_TRY(d_tot.resize(size_t(nt)));
  OICC_HIP_TRY(d_st.resize(size_t(cap * nt))); OICC_HIP_TRY(d_en.resize(size_t(cap * nt)));
  OICC_HIP_TRY(hipMemcpyAsync(d_th.p, th, sizeof(double) * nt, hipMemcpyHostToDevice, st));
  OICC_HIP_TRY(hipEventRecord(e0, st));
  hipLaunchKernelGGL(simu_norm_kernel, dim3(unsigned(nb)), dim3(kThreads), lds, st, d_acc, n, h, d_norm.p);
  hipLaunchKernelGGL(simu_edge_count_kernel, dim3(unsigned(nb)), dim3(kThreads), 0, st, d_norm.p, n, h, d_th.p, nt, d_cnt.p);
  hipLaunchKernelGGL(simu_edge_scan_kernel, dim3(1), dim3(64), 0, st, d_cnt.p, nb, nt, d_tot.p);
  hipLaunchKernelGGL(simu_edge_write_kernel, dim3(unsigned(nb)), dim3(kThreads), 0, st, d_norm.p, n, h, d_th.p, nt, d_cnt.p, int32_t(cap), d_st.p, d_en.p);
  OICC_HIP_TRY(hipGetLastError());
  OICC_HIP_TRY(hipEventRecord(e1, st));
  OICC_HIP_TRY(hipMemcpyAsync(tot.data(), d_tot.p, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, st));
  OICC_HIP_TRY(hipStreamSynchronize(st));
  OICC_HIP_TRY(hipEventElapsedTime(&f, e0, e1));
  if (ms) *ms += double(f);
  for (int t = 0; t < nt; ++t) {
    const int64_t k = std::min<int64_t>(tot[size_t(t)], cap);
    std::vector<int32_t> s(static_cast<size_t>(k)), e(static_cast<size_t>(k));
    if (k > 0) {
      OICC_HIP_TRY(hipMemcpy(s.data(), d_st.p + int64_t(t) * cap, sizeof(int32_t) * k, hipMemcpyDeviceToHost));
      OICC_HIP_TRY(hipMemcpy(e.data(), d_en.p + int64_t(t) * cap, sizeof(int32_t) * k, hipMemcpyDeviceToHost));
    }
    auto& o = (*out)[size_t(t)];
    o.resize(size_t(2 * k));
    for (int64_t j = 0; j < k; ++j) { o[size_t(2 * j)] = s[size_t(j)]; o[size_t(2 * j + 1)] = e[size_t(j)]; }
  }
  if (norms_host) {
    OICC_HIP_TRY(hipMemcpy(norms_host + h, d_norm.p + h, sizeof(double) * M, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < h; ++i) { norms_host[i] = std::nan(""); norms_host[n - 1 - i] = std::nan(""); }
  }
  return OICC_OK;
}

// Gyro blocks on the device for repeated evaluation: samples, timestamps and the block table stay resident.
struct GyroDev {
  oicc::DevBuf<double> t, w, res, jac;
  oicc::DevBuf<GyroBlock> blk;
  int nb = 0, np = 9, optimize_bias = 0;
  double gyro_dt = -1.0, ms = 0.0;
  oicc::Event e0, e1;
  oicc::Stream st;      // behind the buffers and events (hip_resources.h)
  int init(const double* t_s, const double* gyro, int64_t n, const std::vector<GyroBlock>& blocks, int opt_bias, double dt) {
    nb = int(blocks.size()); optimize_bias = opt_bias; np = opt_bias ? 12 : 9; gyro_dt = dt;
    OICC_HIP_TRY(st.create()); OICC_HIP_TRY(e0.create()); OICC_HIP_TRY(e1.create());
    OICC_HIP_TRY(t.resize(size_t(n))); OICC_HIP_TRY(w.resize(3 * size_t(n)));
    OICC_HIP_TRY(res.resize(3 * size_t(std::max(nb, 1)))); OICC_HIP_TRY(jac.resize(3 * size_t(std::max(nb, 1)) * np));
    OICC_HIP_TRY(blk.resize(size_t(std::max(nb, 1))));
    OICC_HIP_TRY(hipMemcpy(t.p, t_s, sizeof(double) * n, hipMemcpyHostToDevice));
    OICC_HIP_TRY(hipMemcpy(w.p, gyro, sizeof(double) * 3 * n, hipMemcpyHostToDevice));
    if (nb > 0) OICC_HIP_TRY(hipMemcpy(blk.p, blocks.data(), sizeof(GyroBlock) * nb, hipMemcpyHostToDevice));
    return OICC_OK;
  }
  // r [3 nb], J [3 nb][np]
  int eval(const double* p, std::vector<double>* r, std::vector<double>* J) {
    if (nb == 0) { r->clear(); J->clear(); return OICC_OK; }
    GyroParams gp;
    for (int k = 0; k < 12; ++k) gp.p[k] = p[k];
    if (hipEventRecord(e0, st) != hipSuccess) return OICC_ERR_HIP;
    hipLaunchKernelGGL(simu_gyro_kernel, dim3(unsigned(nb), unsigned(np)), dim3(kThreads), 0, st, t.p, w.p, blk.p, gp, optimize_bias, gyro_dt, np, res.p, jac.p);
    if (hipGetLastError() != hipSuccess || hipEventRecord(e1, st) != hipSuccess) return OICC_ERR_HIP;
    r->resize(size_t(3 * nb)); J->resize(size_t(3 * nb * np));
    const bool copied = hipMemcpyAsync(r->data(), res.p, sizeof(double) * 3 * nb, hipMemcpyDeviceToHost, st) == hipSuccess &&
                        hipMemcpyAsync(J->data(), jac.p, sizeof(double) * 3 * nb * np, hipMemcpyDeviceToHost, st) == hipSuccess;
    if (hipStreamSynchronize(st) != hipSuccess || !copied) return OICC_ERR_HIP;      // r and J are the caller's: nothing writes them after the return
    float f = 0.0f;
    if (hipEventElapsedTime(&f, e0, e1) == hipSuccess) ms += double(f);
    return OICC_OK;
  }
};

// cost = 0.5 sum r^2, g = J^T r, H = J^T J (packed upper) in row order
void gyro_normal_eq(const std::vector<double>& r, const std::vector<double>& J, int np, double* cost, double* H, double* g) {
  double c = 0.0;
  const int nh = np * (np + 1) / 2;
  for (int k = 0; k < nh; ++k) H[k] = 0.0;
  for (int k = 0; k < np; ++k) g[k] = 0.0;
  for (size_t i = 0; i < r.size(); ++i) {
    const double* Ji = J.data() + i * size_t(np);
    c += r[i] * r[i];
    int e = 0;
    for (int a = 0; a < np; ++a) { g[a] += Ji[a] * r[i]; for (int b = a; b < np; ++b) { H[e] += Ji[a] * Ji[b]; ++e; } }
  }
  *cost = 0.5 * c;
}

template <int D>
struct GyroEval {
  GyroDev* dev; double full[12] = {0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0}; int status = OICC_OK;
  bool operator()(const double* x, bool, double* cost, double* H, double* g) {
    for (int k = 0; k < D; ++k) full[k] = x[k];
    std::vector<double> r, J;
    const int rc = dev->eval(full, &r, &J);
    if (rc != OICC_OK) { status = rc; *cost = std::nan(""); return false; }
    gyro_normal_eq(r, J, D, cost, H, g);
    return std::isfinite(*cost);
  }
};

void unpack_gram(const double* Hp, int np, double* full) {
  int e = 0;
  for (int a = 0; a < np; ++a) for (int b = a; b < np; ++b) { full[a * np + b] = Hp[e]; full[b * np + a] = Hp[e]; ++e; }
}

bool all_finite(const double* x, int64_t m) { for (int64_t i = 0; i < m; ++i) if (!std::isfinite(x[i])) return false; return true; }

}  // namespace

extern "C" int oicc_static_imu_intervals(int32_t device_ordinal, int64_t n, const double* acc, int32_t num_thresholds, const double* thresholds,
                                         int32_t win_size, int32_t capacity, int32_t* counts, int32_t* intervals, double* norms, double* device_ms) {
  if (!acc || !thresholds || !counts || !intervals || n < 1 || n > INT32_MAX || num_thresholds < 1 || num_thresholds > kMaxTh || capacity < 0)
    return OICC_ERR_INVALID_ARG;
  const int w = normalized_win(win_size);
  if (w > 2 * kMaxHalf + 1 || !all_finite(acc, 3 * n)) return OICC_ERR_INVALID_ARG;
  if (int rc = select_device(device_ordinal)) return rc;
  oicc::DevBuf<double> d_acc;
  oicc::Stream st;
  std::vector<std::vector<int32_t>> iv;
  double ms = 0.0;
  OICC_HIP_TRY(st.create());
  OICC_HIP_TRY(d_acc.upload(acc, 3 * size_t(n), st));
  if (int rc = run_detector(d_acc.p, n, w, num_thresholds, thresholds, &iv, norms, &ms, st)) return rc;
  for (int t = 0; t < num_thresholds; ++t) {
    const auto& o = iv[size_t(t)];
    counts[t] = int32_t(o.size() / 2);
    const size_t k = std::min<size_t>(o.size() / 2, size_t(capacity));
    std::memcpy(intervals + int64_t(t) * 2 * capacity, o.data(), sizeof(int32_t) * 2 * k);
  }
  if (device_ms) *device_ms = ms;
  return OICC_OK;
}

extern "C" int oicc_static_imu_eval_acc(int32_t device_ordinal, int64_t num, const double* samples, double g_mag, const double* params,
                                        double* residuals, double* jacobian, double* cost, double* gram, double* gradient) {
  if (!samples || !params || !cost || !gram || !gradient || num < 1 || num > INT32_MAX) return OICC_ERR_INVALID_ARG;
  if (int rc = select_device(device_ordinal)) return rc;
  oicc::DevBuf<double> d_s, d_p, d_r, d_j, d_o;      // the null stream runs the kernel, and the blocking copies behind it wait for it
  double out[10 + kAccNH];
  OICC_HIP_TRY(d_s.resize(3 * size_t(num))); OICC_HIP_TRY(d_p.resize(9));
  OICC_HIP_TRY(d_r.resize(size_t(num))); OICC_HIP_TRY(d_j.resize(9 * size_t(num)));
  OICC_HIP_TRY(d_o.resize(10 + kAccNH));
  OICC_HIP_TRY(hipMemcpy(d_s.p, samples, sizeof(double) * 3 * num, hipMemcpyHostToDevice));
  OICC_HIP_TRY(hipMemcpy(d_p.p, params, sizeof(double) * 9, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(simu_acc_eval_kernel, dim3(1), dim3(kThreads), 0, 0, d_s.p, num, g_mag, d_p.p, d_r.p, d_j.p, d_o.p);
  OICC_HIP_TRY(hipGetLastError());
  OICC_HIP_TRY(hipMemcpy(out, d_o.p, sizeof(out), hipMemcpyDeviceToHost));
  if (residuals) OICC_HIP_TRY(hipMemcpy(residuals, d_r.p, sizeof(double) * num, hipMemcpyDeviceToHost));
  if (jacobian) OICC_HIP_TRY(hipMemcpy(jacobian, d_j.p, sizeof(double) * 9 * num, hipMemcpyDeviceToHost));
  *cost = out[0];
  for (int k = 0; k < 9; ++k) gradient[k] = out[1 + k];
  unpack_gram(out + 10, 9, gram);
  return OICC_OK;
}

extern "C" int oicc_static_imu_eval_gyro(int32_t device_ordinal, int64_t n, const double* t_s, const double* gyro, int32_t num_blocks,
                                         const int32_t* ranges, const double* g_versors, int32_t optimize_bias, double gyro_dt,
                                         const double* params, double* residuals, double* jacobian, double* cost, double* gram,
                                         double* gradient, double* device_ms) {
  if (!t_s || !gyro || !params || !cost || !gram || !gradient || n < 1 || n > INT32_MAX || num_blocks < 1 || !ranges || !g_versors)
    return OICC_ERR_INVALID_ARG;
  std::vector<GyroBlock> blocks(static_cast<size_t>(num_blocks));
  for (int b = 0; b < num_blocks; ++b) {
    const int32_t i0 = ranges[2 * b], i1 = ranges[2 * b + 1];
    if (i0 < -1 || i1 < -1 || i0 >= n || i1 >= n) return OICC_ERR_INVALID_ARG;
    GyroBlock& B = blocks[size_t(b)];
    B.i0 = i0; B.i1 = i1;
    for (int k = 0; k < 3; ++k) { B.g0[k] = g_versors[6 * b + k]; B.g1[k] = g_versors[6 * b + 3 + k]; }
  }
  int rc = select_device(device_ordinal);
  if (rc != OICC_OK) return rc;
  GyroDev dev;
  rc = dev.init(t_s, gyro, n, blocks, optimize_bias ? 1 : 0, gyro_dt);
  if (rc != OICC_OK) return rc;
  std::vector<double> r, J;
  rc = dev.eval(params, &r, &J);
  if (rc != OICC_OK) return rc;
  const int np = dev.np;
  double Hp[78];
  gyro_normal_eq(r, J, np, cost, Hp, gradient);
  unpack_gram(Hp, np, gram);
  if (residuals) std::memcpy(residuals, r.data(), sizeof(double) * r.size());
  if (jacobian) std::memcpy(jacobian, J.data(), sizeof(double) * J.size());
  if (device_ms) *device_ms = dev.ms;
  return OICC_OK;
}

namespace {

// The calibration behind oicc_static_imu_calibrate's argument checks; rep and the two parameter sets hold their defaults.  The entry
// writes the report whatever this returns.
int calibrate(int64_t n, const double* t_s, const double* acc, const double* gyro, const oicc_static_imu_options& opt, int w,
              double* acc_params, double* gyro_params, oicc_static_imu_report& rep) {
  const oicc::BaLmOptions lmo = oicc::ceres_default_lm_options();

  // CalibrateAcc (.cc:54-186): initial bias and threshold
  const int init_end = initial_interval_end(t_s, n, opt.init_interval_duration_s);
  double acc_mean[3], acc_var[3];
  data_mean(acc, 0, init_end, acc_mean);
  int imax = 0;
  for (int c = 1; c < 3; ++c) if (acc_mean[c] > acc_mean[imax]) imax = c;   // maxCoeff: the first largest
  acc_mean[imax] -= opt.gravity_magnitude;
  for (int c = 0; c < 3; ++c) rep.init_acc_bias[c] = acc_mean[c];
  data_variance(acc, 0, init_end, acc_var);
  const double norm_th = std::sqrt((acc_var[0] * acc_var[0] + acc_var[1] * acc_var[1]) + acc_var[2] * acc_var[2]);
  rep.norm_th = norm_th;
  double th[kMaxTh];
  for (int t = 0; t < kMaxTh; ++t) th[t] = double(t + 1) * norm_th;

  oicc::DevBuf<double> d_acc, d_samp, d_x0, d_x, d_cost;
  oicc::DevBuf<AccProblem> d_prob;
  oicc::DevBuf<int32_t> d_it, d_term;
  oicc::Event e0, e1;
  std::vector<std::vector<int32_t>> iv;
  std::vector<std::vector<int32_t>> valid(kMaxTh);   // extracted intervals per threshold, (start, end) pairs
  std::vector<double> packed;
  std::vector<AccProblem> probs;
  std::vector<int> prob_th;
  const int ns = opt.interval_n_samples;
  int np_acc = 0;
  float f = 0.0f;
  double x0[9];
  for (int k = 0; k < 9; ++k) x0[k] = k < 3 ? 0.0 : (k < 6 ? 1.0 : rep.init_acc_bias[k - 6]);
  std::vector<double> xs, costs;
  std::vector<int32_t> its, terms;
  int best = -1;
  double min_cost = std::numeric_limits<double>::max();
  oicc::Stream st;      // behind the buffers, the events and the host vectors its copies fill (hip_resources.h)

  OICC_HIP_TRY(st.create());
  OICC_HIP_TRY(e0.create()); OICC_HIP_TRY(e1.create());
  OICC_HIP_TRY(d_acc.upload(acc, 3 * size_t(n), st));
  if (int rc = run_detector(d_acc.p, n, w, kMaxTh, th, &iv, nullptr, &rep.ms_detector, st)) return rc;
  // ExtractIntervalsSamples (imu_data_interval.cc:64-109), acc_use_means_ false: the first ns samples of every interval
  // with at least ns samples; true: the interval's mean
  for (int t = 0; t < kMaxTh; ++t) {
    const auto& o = iv[size_t(t)];
    for (size_t k = 0; k < o.size() / 2; ++k) if (o[2 * k + 1] - o[2 * k] + 1 >= ns) { valid[size_t(t)].push_back(o[2 * k]); valid[size_t(t)].push_back(o[2 * k + 1]); }
    const int cnt = int(valid[size_t(t)].size() / 2);
    rep.num_intervals[t] = cnt;
    if (cnt < opt.min_num_intervals || cnt == 0) continue;
    const int64_t off = int64_t(packed.size() / 3);
    for (int k = 0; k < cnt; ++k) {
      const int s = valid[size_t(t)][size_t(2 * k)], e = valid[size_t(t)][size_t(2 * k + 1)];
      if (opt.acc_use_means) { double m[3]; data_mean(acc, s, e, m); packed.insert(packed.end(), m, m + 3); }
      else packed.insert(packed.end(), acc + 3 * int64_t(s), acc + 3 * (int64_t(s) + ns));
    }
    probs.push_back(AccProblem{off, int64_t(packed.size() / 3) - off});
    prob_th.push_back(t);
  }
  np_acc = int(probs.size());
  if (np_acc > 0) {
    OICC_HIP_TRY(d_samp.resize(packed.size())); OICC_HIP_TRY(d_prob.resize(size_t(np_acc)));
    OICC_HIP_TRY(d_x0.resize(9)); OICC_HIP_TRY(d_x.resize(9 * size_t(np_acc)));
    OICC_HIP_TRY(d_cost.resize(size_t(np_acc))); OICC_HIP_TRY(d_it.resize(size_t(np_acc))); OICC_HIP_TRY(d_term.resize(size_t(np_acc)));
    OICC_HIP_TRY(hipMemcpyAsync(d_samp.p, packed.data(), sizeof(double) * packed.size(), hipMemcpyHostToDevice, st));
    OICC_HIP_TRY(hipMemcpyAsync(d_prob.p, probs.data(), sizeof(AccProblem) * np_acc, hipMemcpyHostToDevice, st));
    OICC_HIP_TRY(hipMemcpyAsync(d_x0.p, x0, sizeof(double) * 9, hipMemcpyHostToDevice, st));
    OICC_HIP_TRY(hipEventRecord(e0, st));
    hipLaunchKernelGGL(simu_acc_lm_kernel, dim3(unsigned(np_acc)), dim3(kThreads), 0, st, d_samp.p, d_prob.p, opt.gravity_magnitude, d_x0.p, lmo, d_x.p, d_cost.p, d_it.p, d_term.p);
    OICC_HIP_TRY(hipGetLastError());
    OICC_HIP_TRY(hipEventRecord(e1, st));
    xs.resize(size_t(9 * np_acc)); costs.resize(size_t(np_acc)); its.resize(size_t(np_acc)); terms.resize(size_t(np_acc));
    OICC_HIP_TRY(hipMemcpyAsync(xs.data(), d_x.p, sizeof(double) * xs.size(), hipMemcpyDeviceToHost, st));
    OICC_HIP_TRY(hipMemcpyAsync(costs.data(), d_cost.p, sizeof(double) * costs.size(), hipMemcpyDeviceToHost, st));
    OICC_HIP_TRY(hipMemcpyAsync(its.data(), d_it.p, sizeof(int32_t) * its.size(), hipMemcpyDeviceToHost, st));
    OICC_HIP_TRY(hipMemcpyAsync(terms.data(), d_term.p, sizeof(int32_t) * terms.size(), hipMemcpyDeviceToHost, st));
    OICC_HIP_TRY(hipStreamSynchronize(st));
    OICC_HIP_TRY(hipEventElapsedTime(&f, e0, e1));
    rep.ms_acc = double(f);
  }
  for (int q = 0; q < np_acc; ++q) {
    const int t = prob_th[size_t(q)];
    rep.acc_final_cost[t] = costs[size_t(q)]; rep.acc_iterations[t] = its[size_t(q)]; rep.acc_termination[t] = terms[size_t(q)];
    if (costs[size_t(q)] < min_cost) { min_cost = costs[size_t(q)]; best = q; }   // strictly smaller: ties keep the earlier
  }
  if (best < 0) return OICC_SIMU_ACC_IMPOSSIBLE;
  rep.th_mult = prob_th[size_t(best)] + 1;
  std::memcpy(acc_params, xs.data() + 9 * best, sizeof(double) * 9);

  {  // CalibrateAccGyro (.cc:188-337)
    const double* pa = acc_params;
    const double ms01 = -pa[0] * pa[4], ms02 = pa[1] * pa[5], ms12 = -pa[2] * pa[5];
    const auto& vt = valid[size_t(prob_th[size_t(best)])];
    const int npos = int(vt.size() / 2);
    std::vector<double> gv(size_t(3 * npos));
    for (int k = 0; k < npos; ++k) {   // static means of the calibrated accelerometer (only_means = true), normalised
      const int s = vt[size_t(2 * k)], e = vt[size_t(2 * k + 1)];
      double m[3] = {0, 0, 0};
      for (int i = s; i <= e; ++i) {
        const double* x = acc + 3 * int64_t(i);
        const double u0 = x[0] - pa[6], u1 = x[1] - pa[7], u2 = x[2] - pa[8];
        m[0] += (pa[3] * u0 + ms01 * u1) + ms02 * u2;
        m[1] += pa[4] * u1 + ms12 * u2;
        m[2] += pa[5] * u2;
      }
      for (int c = 0; c < 3; ++c) m[c] /= double(e - s + 1);
      const double nrm = std::sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
      for (int c = 0; c < 3; ++c) gv[size_t(3 * k + c)] = m[c] / nrm;
    }
    const int gend = initial_interval_end(t_s, n, opt.init_interval_duration_s);
    double gb[3];
    data_mean(gyro, 0, gend, gb);
    for (int c = 0; c < 3; ++c) rep.gyro_init_bias[c] = gb[c];
    std::vector<double> gw(size_t(3 * n));
    for (int64_t i = 0; i < n; ++i) for (int c = 0; c < 3; ++c) gw[size_t(3 * i + c)] = gyro[3 * i + c] - gb[c];
    std::vector<GyroBlock> blocks;
    int64_t t_idx = 0;
    for (int k = 0; k + 1 < npos; ++k) {   // the forward scan of .cc:250-265, t_idx carried over
      const double ts0 = t_s[vt[size_t(2 * k + 1)]], ts1 = t_s[vt[size_t(2 * k + 2)]];
      int32_t i0 = -1, i1 = -1;
      for (; t_idx < n; t_idx++) {
        if (i0 < 0) { if (t_s[t_idx] >= ts0) i0 = int32_t(t_idx); }
        else if (t_s[t_idx] >= ts1) { i1 = int32_t(t_idx - 1); break; }
      }
      GyroBlock B;
      B.i0 = i0; B.i1 = i1;
      for (int c = 0; c < 3; ++c) { B.g0[c] = gv[size_t(3 * k + c)]; B.g1[c] = gv[size_t(3 * k + 3 + c)]; }
      blocks.push_back(B);
    }
    rep.gyro_num_blocks = int(blocks.size());
    GyroDev dev;
    if (int rc = dev.init(t_s, gw.data(), n, blocks, opt.optimize_gyro_bias ? 1 : 0, opt.gyro_dt)) return rc;
    double x[12] = {0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0};   // init_gyro_calib_ (default triad), bias terms 0
    int it = 0, term = 0;
    double fc = 0.0;
    {
      std::vector<double> r0, J0;
      if (int rc = dev.eval(x, &r0, &J0)) return rc;
      double c0 = 0.0; for (double v : r0) c0 += v * v;
      rep.gyro_initial_cost = 0.5 * c0;
    }
    int rc = OICC_OK;
    if (opt.optimize_gyro_bias) { GyroEval<12> ev{&dev}; term = oicc::small_lm<12>(lmo, x, ev, &it, &fc); rc = ev.status; }
    else { GyroEval<9> ev{&dev}; term = oicc::small_lm<9>(lmo, x, ev, &it, &fc); rc = ev.status; }
    if (rc != OICC_OK) return rc;
    rep.gyro_iterations = it; rep.gyro_termination = term; rep.gyro_final_cost = fc; rep.ms_gyro = dev.ms;
    for (int k = 0; k < 9; ++k) gyro_params[k] = x[k];
    for (int c = 0; c < 3; ++c) gyro_params[9 + c] = gb[c] + (opt.optimize_gyro_bias ? x[9 + c] : 0.0);
  }
  return OICC_OK;
}

}  // namespace

extern "C" int oicc_static_imu_calibrate(int32_t device_ordinal, int64_t n, const double* t_s, const double* acc, const double* gyro,
                                         const oicc_static_imu_options* opt_in, double* acc_params, double* gyro_params,
                                         oicc_static_imu_report* report) {
  oicc_static_imu_options opt{9.81, 30.0, -1.0, 100, 12, 101, 0, 0, 0};   // StaticImuCalibrator() (.cc:44-52)
  if (opt_in) opt = *opt_in;
  if (!t_s || !acc || !gyro || !acc_params || !gyro_params || n < 3 || n > INT32_MAX || !(opt.init_interval_duration_s > 0) ||
      opt.interval_n_samples < 1 || opt.min_num_intervals < 0)
    return OICC_ERR_INVALID_ARG;   // InitialInterval throws for these (imu_data_interval.h)
  const int w = normalized_win(opt.win_size);
  if (w > 2 * kMaxHalf + 1 || !all_finite(acc, 3 * n) || !all_finite(gyro, 3 * n) || !all_finite(t_s, n)) return OICC_ERR_INVALID_ARG;
  if (int rc = select_device(device_ordinal)) return rc;
  oicc_static_imu_report rep;
  std::memset(&rep, 0, sizeof(rep));
  rep.th_mult = -1;
  for (int t = 0; t < kMaxTh; ++t) { rep.acc_final_cost[t] = std::nan(""); rep.acc_termination[t] = OICC_SIMU_TERM_SKIPPED; }
  rep.gyro_termination = OICC_SIMU_TERM_SKIPPED;
  rep.gyro_initial_cost = rep.gyro_final_cost = std::nan("");
  const double default_acc[9] = {0, 0, 0, 1, 1, 1, 0, 0, 0};
  const double default_gyro[12] = {0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0};
  std::memcpy(acc_params, default_acc, sizeof(default_acc));
  std::memcpy(gyro_params, default_gyro, sizeof(default_gyro));
  const int rc = calibrate(n, t_s, acc, gyro, opt, w, acc_params, gyro_params, rep);
  if (report) *report = rep;
  if (rc == OICC_SIMU_ACC_IMPOSSIBLE) { std::memcpy(acc_params, default_acc, sizeof(default_acc)); std::memcpy(gyro_params, default_gyro, sizeof(default_gyro)); }
  return rc;
}
