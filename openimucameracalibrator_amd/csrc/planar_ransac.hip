// Robust start poses: RANSAC over the corners of every view of a planar board, all views in one launch
// (include/oicc_hip.h, "Robust start poses").  One workgroup per view, one lane per hypothesis.
//
//   vote     hypothesis h of view v draws five corners (counter hash + partial Fisher-Yates, integers only), solves the
//            5 x 6 radial alignment system  u (q3 a + q4 b + q5) - v (q0 a + q1 b + q2) = 0  by its 5 x 5 minors in
//            registers and counts the corners within `threshold` of its radial line, on the majority half-line.  The
//            view's corners are staged once in LDS (up to kStage; longer views are read from global memory) and every
//            lane walks the same addresses (broadcast reads).  Scores are integers, ties go to the smaller h.
//   refit    normal matrix of the winner's inliers (fixed-order reduction), smallest eigenvector by cyclic Jacobi on one
//            lane, re-classification.
//   pose     calibrated features only: pose completed from q, depth offset as the median of the per-corner solutions
//            (rank by counting), loose gate, least-squares refit of the depth plane, full reprojection test.
//
// tests/planar_ransac_restatement.py restates every step in numpy and is the specification of the constants below.  This
// unit is compiled with -ffp-contract=off (csrc/Makefile): without fused multiply-adds the hypothesis and the tests round
// exactly as the restatement's, so the integer scores agree.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include "../../include/oicc_hip.h"
#include "hip_resources.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kStage = 1024;                 // corners of a view kept in LDS: 2 x 16 KB coordinates + 8 KB depths
constexpr int kMaxHypotheses = 1024;
constexpr int kMaxCornersPerView = 1 << 20;  // the packed vote key keeps the count above 10 bits of hypothesis index
constexpr int kJacobiSweeps = 12;
constexpr double kDegenerateRatio = 1e-12;
constexpr double kLooseGate = 3.0;
constexpr double kSolve3Ratio = 1e-12;
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ uint64_t mix64(uint64_t x) {       // the finaliser of MurmurHash3
  x = (x ^ (x >> 33)) * 0xff51afd7ed558ccdull;
  x = (x ^ (x >> 33)) * 0xc4ceb9fe1a85ec53ull;
  return x ^ (x >> 33);
}

// Five distinct indices below n: partial Fisher-Yates over a virtual array.  Positions 0..4 live in `first`, every other
// touched position in (mp, mv); all indices are compile-time constants after unrolling.
__device__ __forceinline__ void sample5(uint64_t base, int h, int n, int (&first)[5]) {
  int mp[5], mv[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) { first[k] = k; mp[k] = -1; mv[k] = 0; }
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const uint64_t r = mix64(base + (uint64_t(h) << 4) + uint64_t(j));
    const int t = j + int((r >> 11) % uint64_t(n - j));
    const bool low = t < 5;
    int vt = t;
#pragma unroll
    for (int k = 0; k < 5; ++k) if (low && t == k) vt = first[k];
#pragma unroll
    for (int k = 0; k < j; ++k) if (!low && mp[k] == t) vt = mv[k];
    const int vj = first[j];
#pragma unroll
    for (int k = 0; k < 5; ++k) if (low && t == k) first[k] = vj;
    bool hit = false;
#pragma unroll
    for (int k = 0; k < j; ++k) if (!low && mp[k] == t) { mv[k] = vj; hit = true; }
    const bool fresh = !low && !hit;
    mp[j] = fresh ? t : -1;
    mv[j] = fresh ? vj : 0;
    first[j] = vt;
  }
}

// q_k = (-1)^k det(A without column k): Laplace expansion along the last row, rows added one at a time (the
// straight-line program of minors_plan() in the restatement).
__device__ __forceinline__ void null_vector(const double (&A)[5][6], double (&q)[6]) {
  const double m01 = -(A[1][0] * A[0][1]) + A[1][1] * A[0][0];
  const double m02 = -(A[1][0] * A[0][2]) + A[1][2] * A[0][0];
  const double m03 = -(A[1][0] * A[0][3]) + A[1][3] * A[0][0];
  const double m04 = -(A[1][0] * A[0][4]) + A[1][4] * A[0][0];
  const double m05 = -(A[1][0] * A[0][5]) + A[1][5] * A[0][0];
  const double m12 = -(A[1][1] * A[0][2]) + A[1][2] * A[0][1];
  const double m13 = -(A[1][1] * A[0][3]) + A[1][3] * A[0][1];
  const double m14 = -(A[1][1] * A[0][4]) + A[1][4] * A[0][1];
  const double m15 = -(A[1][1] * A[0][5]) + A[1][5] * A[0][1];
  const double m23 = -(A[1][2] * A[0][3]) + A[1][3] * A[0][2];
  const double m24 = -(A[1][2] * A[0][4]) + A[1][4] * A[0][2];
  const double m25 = -(A[1][2] * A[0][5]) + A[1][5] * A[0][2];
  const double m34 = -(A[1][3] * A[0][4]) + A[1][4] * A[0][3];
  const double m35 = -(A[1][3] * A[0][5]) + A[1][5] * A[0][3];
  const double m45 = -(A[1][4] * A[0][5]) + A[1][5] * A[0][4];
  const double m012 = A[2][0] * m12 - A[2][1] * m02 + A[2][2] * m01;
  const double m013 = A[2][0] * m13 - A[2][1] * m03 + A[2][3] * m01;
  const double m014 = A[2][0] * m14 - A[2][1] * m04 + A[2][4] * m01;
  const double m015 = A[2][0] * m15 - A[2][1] * m05 + A[2][5] * m01;
  const double m023 = A[2][0] * m23 - A[2][2] * m03 + A[2][3] * m02;
  const double m024 = A[2][0] * m24 - A[2][2] * m04 + A[2][4] * m02;
  const double m025 = A[2][0] * m25 - A[2][2] * m05 + A[2][5] * m02;
  const double m034 = A[2][0] * m34 - A[2][3] * m04 + A[2][4] * m03;
  const double m035 = A[2][0] * m35 - A[2][3] * m05 + A[2][5] * m03;
  const double m045 = A[2][0] * m45 - A[2][4] * m05 + A[2][5] * m04;
  const double m123 = A[2][1] * m23 - A[2][2] * m13 + A[2][3] * m12;
  const double m124 = A[2][1] * m24 - A[2][2] * m14 + A[2][4] * m12;
  const double m125 = A[2][1] * m25 - A[2][2] * m15 + A[2][5] * m12;
  const double m134 = A[2][1] * m34 - A[2][3] * m14 + A[2][4] * m13;
  const double m135 = A[2][1] * m35 - A[2][3] * m15 + A[2][5] * m13;
  const double m145 = A[2][1] * m45 - A[2][4] * m15 + A[2][5] * m14;
  const double m234 = A[2][2] * m34 - A[2][3] * m24 + A[2][4] * m23;
  const double m235 = A[2][2] * m35 - A[2][3] * m25 + A[2][5] * m23;
  const double m245 = A[2][2] * m45 - A[2][4] * m25 + A[2][5] * m24;
  const double m345 = A[2][3] * m45 - A[2][4] * m35 + A[2][5] * m34;
  const double m0123 = -(A[3][0] * m123) + A[3][1] * m023 - A[3][2] * m013 + A[3][3] * m012;
  const double m0124 = -(A[3][0] * m124) + A[3][1] * m024 - A[3][2] * m014 + A[3][4] * m012;
  const double m0125 = -(A[3][0] * m125) + A[3][1] * m025 - A[3][2] * m015 + A[3][5] * m012;
  const double m0134 = -(A[3][0] * m134) + A[3][1] * m034 - A[3][3] * m014 + A[3][4] * m013;
  const double m0135 = -(A[3][0] * m135) + A[3][1] * m035 - A[3][3] * m015 + A[3][5] * m013;
  const double m0145 = -(A[3][0] * m145) + A[3][1] * m045 - A[3][4] * m015 + A[3][5] * m014;
  const double m0234 = -(A[3][0] * m234) + A[3][2] * m034 - A[3][3] * m024 + A[3][4] * m023;
  const double m0235 = -(A[3][0] * m235) + A[3][2] * m035 - A[3][3] * m025 + A[3][5] * m023;
  const double m0245 = -(A[3][0] * m245) + A[3][2] * m045 - A[3][4] * m025 + A[3][5] * m024;
  const double m0345 = -(A[3][0] * m345) + A[3][3] * m045 - A[3][4] * m035 + A[3][5] * m034;
  const double m1234 = -(A[3][1] * m234) + A[3][2] * m134 - A[3][3] * m124 + A[3][4] * m123;
  const double m1235 = -(A[3][1] * m235) + A[3][2] * m135 - A[3][3] * m125 + A[3][5] * m123;
  const double m1245 = -(A[3][1] * m245) + A[3][2] * m145 - A[3][4] * m125 + A[3][5] * m124;
  const double m1345 = -(A[3][1] * m345) + A[3][3] * m145 - A[3][4] * m135 + A[3][5] * m134;
  const double m2345 = -(A[3][2] * m345) + A[3][3] * m245 - A[3][4] * m235 + A[3][5] * m234;
  const double m01234 = A[4][0] * m1234 - A[4][1] * m0234 + A[4][2] * m0134 - A[4][3] * m0124 + A[4][4] * m0123;
  const double m01235 = A[4][0] * m1235 - A[4][1] * m0235 + A[4][2] * m0135 - A[4][3] * m0125 + A[4][5] * m0123;
  const double m01245 = A[4][0] * m1245 - A[4][1] * m0245 + A[4][2] * m0145 - A[4][4] * m0125 + A[4][5] * m0124;
  const double m01345 = A[4][0] * m1345 - A[4][1] * m0345 + A[4][3] * m0145 - A[4][4] * m0135 + A[4][5] * m0134;
  const double m02345 = A[4][0] * m2345 - A[4][2] * m0345 + A[4][3] * m0245 - A[4][4] * m0235 + A[4][5] * m0234;
  const double m12345 = A[4][1] * m2345 - A[4][2] * m1345 + A[4][3] * m1245 - A[4][4] * m1235 + A[4][5] * m1234;
  q[0] = m12345;
  q[1] = -m02345;
  q[2] = m01345;
  q[3] = -m01245;
  q[4] = m01235;
  q[5] = -m01234;
}

struct Corner { double a, b, u, v; };

__device__ __forceinline__ Corner load_corner(const double* pab, const double* pxy, int i) {
  const double2 ab = *reinterpret_cast<const double2*>(pab + 2 * i);
  const double2 xy = *reinterpret_cast<const double2*>(pxy + 2 * i);
  return Corner{ab.x, ab.y, xy.x, xy.y};
}

// the tangential test and the half-line value of one corner
__device__ __forceinline__ bool radial_test(const double (&q)[6], const Corner& c, double thr2, double& side) {
  const double x = (q[0] * c.a + q[1] * c.b) + q[2];
  const double y = (q[3] * c.a + q[4] * c.b) + q[5];
  const double cross = c.u * y - c.v * x;
  side = c.u * x + c.v * y;
  const double nrm2 = x * x + y * y;
  return cross * cross < thr2 * nrm2;
}

__device__ __forceinline__ bool reprojection_test(double xc, double yc, const Corner& c, double z, double gate2) {
  const double ex = xc - c.u * z;
  const double ey = yc - c.v * z;
  return (ex * ex + ey * ey < gate2 * (z * z)) && z > 0.0;
}

// Score of one hypothesis over all corners of the view; every lane reads the same address.  Returns the count on the
// majority half-line and whether q has to be negated.
__device__ __forceinline__ int score(const double (&q)[6], const double* pab, const double* pxy, int n, double thr2, bool& flip) {
  int n_pos = 0, n_neg = 0, c_pos = 0, c_neg = 0;
  for (int i = 0; i < n; ++i) {
    const Corner c = load_corner(pab, pxy, i);
    double side;
    const bool tang = radial_test(q, c, thr2, side);
    n_pos += side > 0.0; n_neg += side < 0.0;
    c_pos += tang && side > 0.0; c_neg += tang && side < 0.0;
  }
  flip = n_pos < n_neg;
  return flip ? c_neg : c_pos;
}

// Sum of K values per thread over the workgroup in a fixed order: butterfly inside a wave, then the waves in order.
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double* s_part, double* s_out) {
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < K; ++k) s_part[wave * K + k] = v[k];
  __syncthreads();
  if (threadIdx.x < K) {
    double s = s_part[threadIdx.x];
    for (int w = 1; w < kWaves; ++w) s += s_part[w * K + threadIdx.x];
    s_out[threadIdx.x] = s;
  }
  __syncthreads();
}

// Cyclic Jacobi on the symmetric 6 x 6 in s_n (upper triangle, row-major, 21 entries), one lane, everything in
// registers.  Writes the eigenvector of the smallest eigenvalue to q; false when the second smallest eigenvalue is not
// above kDegenerateRatio * the largest (board corners on one line).
__device__ bool smallest_eigenvector(const double* s_n, double (&q)[6]) {
  double A[6][6], V[6][6];
  {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) { A[i][j] = A[j][i] = s_n[k]; ++k; }
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  }
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
#pragma unroll
    for (int p = 0; p < 5; ++p) {
#pragma unroll
      for (int r0 = p + 1; r0 < 6; ++r0) {
        const int qq = r0;
        const double apq = A[p][qq];
        if (apq != 0.0) {
          const double theta = (A[qq][qq] - A[p][p]) / (2.0 * apq);
          double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
          if (theta < 0.0) t = -t;
          const double c = 1.0 / sqrt(t * t + 1.0);
          const double s = t * c;
          A[p][p] = A[p][p] - t * apq;
          A[qq][qq] = A[qq][qq] + t * apq;
          A[p][qq] = A[qq][p] = 0.0;
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            if (r != p && r != qq) {
              const double arp = A[r][p], arq = A[r][qq];
              A[r][p] = A[p][r] = c * arp - s * arq;
              A[r][qq] = A[qq][r] = s * arp + c * arq;
            }
          }
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            const double vrp = V[r][p], vrq = V[r][qq];
            V[r][p] = c * vrp - s * vrq;
            V[r][qq] = s * vrp + c * vrq;
          }
        }
      }
    }
  }
  int k = 0;
  double wk = A[0][0], wmax = A[0][0];
#pragma unroll
  for (int i = 1; i < 6; ++i) {
    if (A[i][i] < wk) { wk = A[i][i]; k = i; }
    if (A[i][i] > wmax) wmax = A[i][i];
  }
  double rest = INFINITY;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    if (i != k && A[i][i] < rest) rest = A[i][i];
#pragma unroll
    for (int r = 0; r < 6; ++r) if (i == k) q[r] = V[r][i];
  }
  return rest > kDegenerateRatio * wmax;
}

// Symmetric 3 x 3 by cofactors, G = (g00 g01 g02 g11 g12 g22); false when it does not determine the solution.
__device__ __forceinline__ bool solve3(const double* G, const double* h, double (&x)[3]) {
  const double g00 = G[0], g01 = G[1], g02 = G[2], g11 = G[3], g12 = G[4], g22 = G[5];
  const double c00 = g11 * g22 - g12 * g12;
  const double c01 = g02 * g12 - g01 * g22;
  const double c02 = g01 * g12 - g02 * g11;
  const double c11 = g00 * g22 - g02 * g02;
  const double c12 = g01 * g02 - g00 * g12;
  const double c22 = g00 * g11 - g01 * g01;
  const double det = (g00 * c00 + g01 * c01) + g02 * c02;
  if (!(det > kSolve3Ratio * ((g00 * g11) * g22))) return false;
  x[0] = ((c00 * h[0] + c01 * h[1]) + c02 * h[2]) / det;
  x[1] = ((c01 * h[0] + c11 * h[1]) + c12 * h[2]) / det;
  x[2] = ((c02 * h[0] + c12 * h[1]) + c22 * h[2]) / det;
  return true;
}

enum { C_POS = 0, C_NEG, C_INL, C_MED0, C_MED1, C_LOOSE0, C_LOOSE1, C_FINAL, C_NUM };

__global__ __launch_bounds__(kThreads) void planar_ransac_kernel(const int64_t* __restrict__ offsets, const double* __restrict__ g_ab,
                                                                 const double* __restrict__ g_xy, int mode, double thr2, int num_hyp,
                                                                 uint64_t seed_mul, uint8_t* __restrict__ g_inlier,
                                                                 int32_t* __restrict__ g_num, double* __restrict__ g_q,
                                                                 double* __restrict__ g_pose, int32_t* __restrict__ g_counts,
                                                                 double* g_tz) {
  __shared__ __attribute__((aligned(16))) double s_ab[2 * kStage];
  __shared__ __attribute__((aligned(16))) double s_xy[2 * kStage];
  __shared__ double s_tz[kStage];
  __shared__ double s_part[kWaves * 21];
  __shared__ double s_sum[21];
  __shared__ double s_q[6];
  __shared__ double s_med[2];
  __shared__ unsigned int s_best;
  __shared__ int s_cnt[C_NUM];
  __shared__ int s_ok;

  const int view = blockIdx.x, tid = threadIdx.x;
  const int64_t off = offsets[view];
  const int n = int(offsets[view + 1] - off);
  uint8_t* mask = g_inlier + off;

  auto give_up = [&](bool with_q, const double (&q)[6]) {       // a view without a result: no inliers, zero q and pose
    for (int i = tid; i < n; i += kThreads) mask[i] = 0;
    if (tid == 0) g_num[view] = 0;
    if (tid < 6) g_q[6 * view + tid] = with_q ? q[tid] : 0.0;
    if (mode == 1 && tid < 12) g_pose[12 * view + tid] = 0.0;
  };
  const double zero6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

  if (n < 5) {
    give_up(false, zero6);
    if (g_counts) for (int h = tid; h < num_hyp; h += kThreads) g_counts[int64_t(view) * num_hyp + h] = 0;
    return;
  }

  const bool staged = n <= kStage;
  if (staged) {
    for (int i = tid; i < 2 * n; i += kThreads) { s_ab[i] = g_ab[2 * off + i]; s_xy[i] = g_xy[2 * off + i]; }
  }
  if (tid < C_NUM) s_cnt[tid] = 0;
  if (tid == 0) { s_best = 0u; s_ok = 0; }
  __syncthreads();
  const double* pab = staged ? s_ab : g_ab + 2 * off;      // flat pointers for the passes outside the vote
  const double* pxy = staged ? s_xy : g_xy + 2 * off;
  double* ptz = staged ? s_tz : g_tz + off;

  // ---- vote ----------------------------------------------------------------------------------------------------------
  const uint64_t base = seed_mul + (uint64_t(view) << 24);
  unsigned int best_key = 0u;
  double best_q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int h = tid; h < num_hyp; h += kThreads) {
    int idx[5];
    sample5(base, h, n, idx);
    double A[5][6];
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const Corner c = staged ? load_corner(s_ab, s_xy, idx[r]) : load_corner(g_ab + 2 * off, g_xy + 2 * off, idx[r]);
      A[r][0] = -(c.v * c.a); A[r][1] = -(c.v * c.b); A[r][2] = -c.v;
      A[r][3] = c.u * c.a;    A[r][4] = c.u * c.b;    A[r][5] = c.u;
    }
    double q[6];
    null_vector(A, q);
    bool flip;
    const int cnt = staged ? score(q, s_ab, s_xy, n, thr2, flip) : score(q, g_ab + 2 * off, g_xy + 2 * off, n, thr2, flip);
    if (g_counts) g_counts[int64_t(view) * num_hyp + h] = cnt;
    const unsigned int key = (unsigned(cnt) << 10) | unsigned(kMaxHypotheses - 1 - h);
    if (key > best_key) {
      best_key = key;
#pragma unroll
      for (int k = 0; k < 6; ++k) best_q[k] = flip ? -q[k] : q[k];
    }
  }
  atomicMax(&s_best, best_key);
  __syncthreads();
  if (best_key == s_best && (best_key >> 10) >= 5u) {        // keys are unique: one owner
#pragma unroll
    for (int k = 0; k < 6; ++k) s_q[k] = best_q[k];
    s_ok = 1;
  }
  __syncthreads();
  if (!s_ok) { give_up(false, zero6); return; }

  // ---- refit on the winner's inliers -----------------------------------------------------------------------------------
  double q[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) q[k] = s_q[k];
  {
    double acc[21];
#pragma unroll
    for (int k = 0; k < 21; ++k) acc[k] = 0.0;
    for (int i = tid; i < n; i += kThreads) {
      const Corner c = load_corner(pab, pxy, i);
      double side;
      if (radial_test(q, c, thr2, side) && side > 0.0) {
        const double r[6] = {-(c.v * c.a), -(c.v * c.b), -c.v, c.u * c.a, c.u * c.b, c.u};
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
          for (int b = a; b < 6; ++b) { acc[k] += r[a] * r[b]; ++k; }
      }
    }
    block_sum<21>(acc, s_part, s_sum);
  }
  if (tid == 0) {
    double e[6];
    const bool ok = smallest_eigenvector(s_sum, e);
#pragma unroll
    for (int k = 0; k < 6; ++k) s_q[k] = e[k];
    s_ok = ok ? 1 : 0;
  }
  __syncthreads();
  if (!s_ok) { give_up(false, zero6); return; }
#pragma unroll
  for (int k = 0; k < 6; ++k) q[k] = s_q[k];

  // ---- re-classification: majority half-line, then the mask ------------------------------------------------------------
  {
    int n_pos = 0, n_neg = 0;
    for (int i = tid; i < n; i += kThreads) {
      double side;
      (void)radial_test(q, load_corner(pab, pxy, i), thr2, side);
      n_pos += side > 0.0; n_neg += side < 0.0;
    }
    if (n_pos) atomicAdd(&s_cnt[C_POS], n_pos);
    if (n_neg) atomicAdd(&s_cnt[C_NEG], n_neg);
  }
  __syncthreads();
  if (s_cnt[C_POS] < s_cnt[C_NEG]) {
#pragma unroll
    for (int k = 0; k < 6; ++k) q[k] = -q[k];
  }
  {
    int cnt = 0;
    for (int i = tid; i < n; i += kThreads) {
      double side;
      const bool in = radial_test(q, load_corner(pab, pxy, i), thr2, side) && side > 0.0;
      mask[i] = in ? 1 : 0;
      cnt += in;
    }
    if (cnt) atomicAdd(&s_cnt[C_INL], cnt);
  }
  __syncthreads();
  if (mode == 0) {
    if (tid == 0) g_num[view] = s_cnt[C_INL];
    if (tid < 6) g_q[6 * view + tid] = q[tid];
    return;
  }

  // ---- calibrated features: pose from q, every lane redundantly ------------------------------------------------------
  const double p = q[0] * q[0] + q[3] * q[3];
  const double r = q[1] * q[1] + q[4] * q[4];
  const double d = q[0] * q[1] + q[3] * q[4];
  const double det = p * r - d * d;
  const double tr = p + r;
  const double k = (tr - sqrt(fmax(tr * tr - 4.0 * det, 0.0))) / (2.0 * det);      // 1 / scale^2: the smaller root
  if (!(det > 0.0) || !(k > 0.0) || !(k < INFINITY)) { give_up(true, q); return; }
  const double s = sqrt(k);
  const double loose2 = (kLooseGate * kLooseGate) * thr2;
  double r31b[2], r32b[2], tzb[2];
  int loose_cnt[2] = {-1, -1};
#pragma unroll
  for (int br = 0; br < 2; ++br) {
    const double r31 = (br == 0 ? 1.0 : -1.0) * sqrt(fmax(1.0 - p * k, 0.0));
    const double r32 = fabs(r31) > 1e-12 ? -(d * k) / r31 : sqrt(fmax(1.0 - r * k, 0.0));
    r31b[br] = r31; r32b[br] = r32; tzb[br] = 0.0;
    int m = 0;
    for (int i = tid; i < n; i += kThreads) {
      const Corner c = load_corner(pab, pxy, i);
      const double xc = s * ((q[0] * c.a + q[1] * c.b) + q[2]);
      const double yc = s * ((q[3] * c.a + q[4] * c.b) + q[5]);
      const double zr = r31 * c.a + r32 * c.b;
      const double tzi = (xc * c.u + yc * c.v) / (c.u * c.u + c.v * c.v) - zr;
      const bool use = mask[i] && fabs(tzi) < INFINITY;
      ptz[i] = use ? tzi : INFINITY;
      m += use;
    }
    if (m) atomicAdd(&s_cnt[C_MED0 + br], m);
    __syncthreads();
    const int total = s_cnt[C_MED0 + br];
    if (total > 0) {                                         // uniform
      const int k1 = (total - 1) / 2, k2 = total / 2;
      for (int i = tid; i < n; i += kThreads) {
        const double ti = ptz[i];
        if (!(ti < INFINITY)) continue;
        int rank = 0;
        for (int j = 0; j < n; ++j) {
          const double tj = ptz[j];
          rank += (tj < ti) || (tj == ti && j < i);
        }
        if (rank == k1) s_med[0] = ti;
        if (rank == k2) s_med[1] = ti;
      }
      __syncthreads();
      const double tz = (s_med[0] + s_med[1]) * 0.5;
      tzb[br] = tz;
      int cnt = 0;
      for (int i = tid; i < n; i += kThreads) {
        if (!mask[i]) continue;
        const Corner c = load_corner(pab, pxy, i);
        const double xc = s * ((q[0] * c.a + q[1] * c.b) + q[2]);
        const double yc = s * ((q[3] * c.a + q[4] * c.b) + q[5]);
        cnt += reprojection_test(xc, yc, c, (r31 * c.a + r32 * c.b) + tz, loose2);
      }
      if (cnt) atomicAdd(&s_cnt[C_LOOSE0 + br], cnt);
      __syncthreads();
      loose_cnt[br] = s_cnt[C_LOOSE0 + br];
    }
  }
  if (loose_cnt[0] < 0 && loose_cnt[1] < 0) { give_up(true, q); return; }
  const int br = loose_cnt[1] > loose_cnt[0] ? 1 : 0;
  double r31 = br ? r31b[1] : r31b[0], r32 = br ? r32b[1] : r32b[0], tz = br ? tzb[1] : tzb[0];

  // least-squares refit of (r31, r32, tz) on the radial part of the reprojection error over the loosely accepted corners
  {
    double acc[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) acc[j] = 0.0;
    for (int i = tid; i < n; i += kThreads) {
      if (!mask[i]) continue;
      const Corner c = load_corner(pab, pxy, i);
      const double xc = s * ((q[0] * c.a + q[1] * c.b) + q[2]);
      const double yc = s * ((q[3] * c.a + q[4] * c.b) + q[5]);
      if (!reprojection_test(xc, yc, c, (r31 * c.a + r32 * c.b) + tz, loose2)) continue;
      const double rho2 = c.u * c.u + c.v * c.v;
      const double w = xc * c.u + yc * c.v;
      const double ar = c.a * rho2, br2 = c.b * rho2;
      acc[0] += ar * c.a; acc[1] += ar * c.b; acc[2] += ar; acc[3] += br2 * c.b; acc[4] += br2; acc[5] += rho2;
      acc[6] += c.a * w;  acc[7] += c.b * w;  acc[8] += w;
    }
    block_sum<9>(acc, s_part, s_sum);
    double x[3];
    if (solve3(s_sum, s_sum + 6, x)) { r31 = x[0]; r32 = x[1]; tz = x[2]; }
  }
  {
    int cnt = 0;
    for (int i = tid; i < n; i += kThreads) {
      const Corner c = load_corner(pab, pxy, i);
      const double xc = s * ((q[0] * c.a + q[1] * c.b) + q[2]);
      const double yc = s * ((q[3] * c.a + q[4] * c.b) + q[5]);
      const bool in = mask[i] && reprojection_test(xc, yc, c, (r31 * c.a + r32 * c.b) + tz, thr2);
      mask[i] = in ? 1 : 0;
      cnt += in;
    }
    if (cnt) atomicAdd(&s_cnt[C_FINAL], cnt);
  }
  __syncthreads();
  if (tid == 0) {
    g_num[view] = s_cnt[C_FINAL];
    const double r1[3] = {s * q[0], s * q[3], r31}, r2[3] = {s * q[1], s * q[4], r32};
    const double r3[3] = {r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]};
    double* P = g_pose + 12 * view;
#pragma unroll
    for (int i = 0; i < 3; ++i) { P[3 * i] = r1[i]; P[3 * i + 1] = r2[i]; P[3 * i + 2] = r3[i]; }
    P[9] = s * q[2]; P[10] = s * q[5]; P[11] = tz;
  }
  if (tid < 6) g_q[6 * view + tid] = q[tid];
}

}  // namespace

extern "C" int oicc_planar_ransac(int32_t device_ordinal, int32_t num_views, const int64_t* corner_offsets, const double* ab,
                                  const double* xy, int32_t mode, double threshold, int32_t num_hypotheses, uint64_t seed,
                                  uint8_t* inlier, int32_t* num_inliers, double* q, double* pose, int32_t* hypothesis_counts,
                                  double* device_ms) {
  if (num_views < 0 || !corner_offsets || (mode != 0 && mode != 1) || !(threshold > 0.0) || !std::isfinite(threshold) ||
      num_hypotheses < 1 || num_hypotheses > kMaxHypotheses || (num_views > 0 && (!num_inliers || !q || (mode == 1 && !pose))))
    return OICC_ERR_INVALID_ARG;
  if (corner_offsets[0] != 0) return OICC_ERR_INVALID_ARG;
  for (int32_t v = 0; v < num_views; ++v) {
    const int64_t c = corner_offsets[v + 1] - corner_offsets[v];
    if (c < 0 || c > kMaxCornersPerView) return OICC_ERR_INVALID_ARG;
  }
  const int64_t n = corner_offsets[num_views];
  if (n > 0 && (!ab || !xy || !inlier)) return OICC_ERR_INVALID_ARG;
  bool long_view = false;
  for (int32_t v = 0; v < num_views; ++v) long_view |= corner_offsets[v + 1] - corner_offsets[v] > kStage;
  for (int64_t i = 0; i < 2 * n; ++i)
    if (!std::isfinite(ab[i]) || !std::isfinite(xy[i])) return OICC_ERR_INVALID_ARG;
  if (int rc = oicc::select_device(device_ordinal)) return rc;
  if (device_ms) *device_ms = 0.0;
  if (num_views == 0) return OICC_OK;

  oicc::DevBuf<int64_t> d_off; oicc::DevBuf<double> d_ab, d_xy, d_q, d_pose, d_tz;
  oicc::DevBuf<uint8_t> d_in; oicc::DevBuf<int32_t> d_num, d_cnt;
  oicc::Event e0, e1;
  oicc::Stream st;
  const size_t n1 = size_t(n > 0 ? n : 1), nv = size_t(num_views);
  OICC_HIP_TRY(st.create());
  OICC_HIP_TRY(e0.create()); OICC_HIP_TRY(e1.create());
  OICC_HIP_TRY(d_off.resize(nv + 1)); OICC_HIP_TRY(d_ab.resize(2 * n1));
  OICC_HIP_TRY(d_xy.resize(2 * n1)); OICC_HIP_TRY(d_in.resize(n1)); OICC_HIP_TRY(d_num.resize(nv));
  OICC_HIP_TRY(d_q.resize(6 * nv)); OICC_HIP_TRY(d_pose.resize(12 * nv));
  if (long_view && mode == 1) OICC_HIP_TRY(d_tz.resize(n1));
  if (hypothesis_counts) OICC_HIP_TRY(d_cnt.resize(nv * size_t(num_hypotheses)));
  OICC_HIP_TRY(hipMemcpyAsync(d_off.p, corner_offsets, sizeof(int64_t) * (nv + 1), hipMemcpyHostToDevice, st));
  if (n > 0) {
    OICC_HIP_TRY(hipMemcpyAsync(d_ab.p, ab, sizeof(double) * 2 * size_t(n), hipMemcpyHostToDevice, st));
    OICC_HIP_TRY(hipMemcpyAsync(d_xy.p, xy, sizeof(double) * 2 * size_t(n), hipMemcpyHostToDevice, st));
  }
  OICC_HIP_TRY(hipEventRecord(e0, st));
  hipLaunchKernelGGL(planar_ransac_kernel, dim3(unsigned(num_views)), dim3(kThreads), 0, st, d_off.p, d_ab.p, d_xy.p, int(mode),
                     threshold * threshold, int(num_hypotheses), seed * kGolden, d_in.p, d_num.p, d_q.p, d_pose.p, d_cnt.p, d_tz.p);
  OICC_HIP_TRY(hipGetLastError());
  OICC_HIP_TRY(hipEventRecord(e1, st));
  if (n > 0) OICC_HIP_TRY(hipMemcpyAsync(inlier, d_in.p, size_t(n), hipMemcpyDeviceToHost, st));
  OICC_HIP_TRY(hipMemcpyAsync(num_inliers, d_num.p, sizeof(int32_t) * nv, hipMemcpyDeviceToHost, st));
  OICC_HIP_TRY(hipMemcpyAsync(q, d_q.p, sizeof(double) * 6 * nv, hipMemcpyDeviceToHost, st));
  if (mode == 1) OICC_HIP_TRY(hipMemcpyAsync(pose, d_pose.p, sizeof(double) * 12 * nv, hipMemcpyDeviceToHost, st));
  if (hypothesis_counts)
    OICC_HIP_TRY(hipMemcpyAsync(hypothesis_counts, d_cnt.p, sizeof(int32_t) * nv * size_t(num_hypotheses), hipMemcpyDeviceToHost, st));
  OICC_HIP_TRY(hipStreamSynchronize(st));
  float ms = 0.0f;
  OICC_HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  if (device_ms) *device_ms = double(ms);
  return OICC_OK;
}
