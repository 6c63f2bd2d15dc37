// Covariance of the view bundle adjustment (include/oicc_hip.h, oicc_ba_estimate_covariance; DESIGN.md, "Covariance of the view
// bundle adjustment"): intrinsics and view poses variable together.
//
//   H = [ A  E ]     A: block diagonal, one D x D block per view (D = 3 or 6), band storage with W = D
//       [ E' C ]     C: a x a intrinsics corner, a <= 10
//
// The assembly pass (ba_blocks_kernel) adds every chunk's Gram entries (<= 64 observations of one view per chunk) with fp64 atomics,
// in whatever order the waves arrive.  An entry of A_v or E_v of a view of one or two chunks gets one or two addends onto zero,
// which is commutative: its bits do not depend on the launch, and it is taken from the assembly.  The corner C gets an addend from
// every chunk of every view, and A_v, E_v of a view of THREE OR MORE chunks (more than 128 observations) get three or more: their
// last bits change from run to run.  Two estimates at the same parameters must return the same bits, so those sums are formed
// again here in chunk order:
//
//   ba_cov_corner_rows  one wave per chunk of the assembly's work list, lane = observation: its two rows sqrt(rho') [J_pose | J_theta],
//                       the chunk's a x a Gram matrix of the intrinsics columns by wave reductions, one partial per chunk -- and,
//                       for the chunks of a view of three or more, the D x D and D x a parts too.  The corner kernel adds the
//                       a x a partials in chunk order; ba_cov_views adds the D x D and D x a partials of such a view in chunk order.
//
// Everything works on Hs = S H S, s_i = H_ii^-1/2 (unit diagonal, no damping).  With the intrinsics eliminated the views are
// independent, so the inverse is a view-parallel Schur complement, S = C - sum_v E_v' A_v^-1 E_v.
//
// Three launches: ba_cov_front_kernel (ba_cov_views and ba_cov_corner_rows as two ranges of workgroups; two launches of it, chunk
// partials first, when a view has three or more chunks and its per-view step waits for them), ba_cov_corner_kernel,
// ba_cov_handout_kernel.
//
//   ba_cov_views           16 lanes = one view, 16 views per workgroup.  Every lane of a view factors the scaled block
//                          A_v = L L' in registers and forms A_v^-1 = L^-T L^-1; lane q < a owns arrow column q:
//                          e_q = E_v[:, q], w_q = A_v^-1 e_q.  Entry (q1, q2) of E_v' W_v is e_q1 . w_q2: lane q2 fetches
//                          e_q1 by a 16-wide shuffle.  The 16 views of the workgroup are summed in a fixed order (shuffle
//                          over the 4 views of a wave, LDS over the 4 waves) into ONE partial per workgroup: no atomics.
//   ba_cov_corner_kernel   one wave: S = C_s - (partials summed in workgroup order), its Cholesky factor, the inverse of
//                          the factor, Sigma = X'X; intrinsics covariance unscaled; starts the running maximum of the
//                          scaled diagonal.
//   ba_cov_handout_kernel  16 lanes = one view again: lane q forms column q of T = W_v Sigma (w_q' by shuffle), stores
//                          cov(pose_v, theta)[:, q] = -T[:, q]; the D x D sum T W_v' is reduced over the 16 lanes by
//                          xor shuffles; lane 0 adds A_v^-1, unscales and stores the full block.  The maximum of the scaled
//                          diagonal goes through an integer atomicMax (order independent).
//
// A view without observations (all-zero block) is left out: zero contribution, NaN outputs.  A failed pivot or diagonal is
// recorded by atomicMin of the view (or nv + corner column), so the FIRST failure is reported whatever the launch order.
#include <hip/hip_runtime.h>
#include "oicc_device.h"
#include "ba_math.h"
#include "gram.h"
#include "ba_device.h"

namespace oicc {

constexpr int kBcLanes = 16;                      // lanes per view (>= kBaIntr arrow columns)
constexpr int kBcViews = kBaCovViewsPerGroup;     // views per workgroup
constexpr int kBcThreads = kBcLanes * kBcViews;   // 256
static_assert(kBaIntr <= kBcLanes, "one lane per arrow column");

__device__ __forceinline__ bool ba_cov_positive(double d) { return d > 0.0 && d < __builtin_huge_val(); }

// A (symmetric, both halves given) -> Z = A^-1 through the Cholesky factor and its inverse; false: a pivot is not positive
template <int D>
__device__ __forceinline__ bool ba_cov_spd_inverse(double A[D][D], double Z[D][D]) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    double t = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) t = fma(-A[j][k], A[j][k], t);
    if (!(t > 0.0)) { ok = false; t = 1.0; }
    const double l = sqrt(t);
    A[j][j] = l;
#pragma unroll
    for (int i = j + 1; i < D; ++i) {
      double u = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) u = fma(-A[i][k], A[j][k], u);
      A[i][j] = u / l;
    }
  }
  double X[D][D];   // L^-1 (lower)
#pragma unroll
  for (int c = 0; c < D; ++c) {
#pragma unroll
    for (int r = c; r < D; ++r) {
      double v = r == c ? 1.0 : 0.0;
#pragma unroll
      for (int k = c; k < r; ++k) v = fma(-A[r][k], X[k][c], v);
      X[r][c] = v / A[r][r];
    }
  }
#pragma unroll
  for (int r = 0; r < D; ++r) {
#pragma unroll
    for (int c = r; c < D; ++c) {
      double v = 0.0;
#pragma unroll
      for (int k = c; k < D; ++k) v = fma(X[k][r], X[k][c], v);
      Z[r][c] = v; Z[c][r] = v;
    }
  }
  return ok;
}

// scale factors of the view's pose columns from the diagonal of its block; false: an entry is not finite and positive
template <int D>
__device__ __forceinline__ bool ba_cov_pose_scale(const double A[D][D], double s[D], int* first_bad) {
  bool ok = true;
#pragma unroll
  for (int r = D - 1; r >= 0; --r) {
    const double dg = A[r][r];
    const bool okr = ba_cov_positive(dg);
    if (!okr) { ok = false; *first_bad = r; }
    s[r] = okr ? 1.0 / sqrt(dg) : 0.0;
  }
  return ok;
}

// one wave = chunk `bid` of the assembly's work list: its a x a part of the intrinsics corner
__device__ __forceinline__ void ba_cov_corner_rows(const double* x, const BaData& d, const BaCovBuffers& cb, int bid, int lane) {
  const int a = d.n_arrow;
  double* const chunkC = cb.chunkC;
  const int c_count = d.chunk_n[bid];
  const int view = d.chunk_view[bid];
  const int64_t c = d.chunk_c0[bid] + lane;
  double j0[kBaMaxIntr], j1[kBaMaxIntr], p0[6], p1[6];
#pragma unroll
  for (int k = 0; k < kBaMaxIntr; ++k) { j0[k] = 0.0; j1[k] = 0.0; }
#pragma unroll
  for (int k = 0; k < 6; ++k) { p0[k] = 0.0; p1[k] = 0.0; }
  if (lane < c_count) {
    const double* pose = x + 6 * (int64_t)view;
    double R[9], Jr[9];
    angle_axis_matrix(pose + 3, R);
    so3_Jr(pose + 3, Jr);
    double px[2], Jp[12], Ji[2 * kBaMaxIntr];
    if (ba_observation<true>(d.model, x + 6 * d.n_views, pose, R, Jr, x + d.pts_off + 4 * (int64_t)d.pid[c], px, Jp, Ji, nullptr)) {
      const double r0 = px[0] - d.u[c], r1 = px[1] - d.v[c];
      double rho, s1;
      huber(d.huber, r0 * r0 + r1 * r1, &rho, &s1);
#pragma unroll
      for (int k = 0; k < kBaMaxIntr; ++k) { j0[k] = s1 * Ji[k]; j1[k] = s1 * Ji[kBaMaxIntr + k]; }
#pragma unroll
      for (int k = 0; k < 6; ++k) { p0[k] = s1 * Jp[k]; p1[k] = s1 * Jp[6 + k]; }
    }
  }
  double* out = chunkC + (int64_t)bid * a * a;
#pragma unroll
  for (int k1 = 0; k1 < kBaMaxIntr; ++k1) {
#pragma unroll
    for (int k2 = k1; k2 < kBaMaxIntr; ++k2) {
      const int a1 = d.intr_col[k1], a2 = d.intr_col[k2];
      if (a1 >= 0 && a2 >= 0) {
        const double v = wave_sum(fma(j0[k1], j0[k2], j1[k1] * j1[k2]));
        if (lane == 0) { out[a1 * a + a2] = v; out[a2 * a + a1] = v; }
      }
    }
  }
  // a view of three or more chunks: the chunk's part of A_v (upper triangle, [D][D]) and of E_v ([D][a]) as well
  const int D = d.pose_dim;
  if (cb.view_chunk0 == nullptr || D == 0 || cb.view_chunk0[view + 1] - cb.view_chunk0[view] < 3) return;
  double* outA = cb.chunkA + (int64_t)bid * D * D;
  double* outE = cb.chunkE + (int64_t)bid * D * a;
#pragma unroll
  for (int i1 = 0; i1 < 6; ++i1) {
    const int o1 = d.pose_off[i1 / 3];
    if (o1 < 0) continue;
    const int c1 = o1 + i1 % 3;
#pragma unroll
    for (int i2 = i1; i2 < 6; ++i2) {
      const int o2 = d.pose_off[i2 / 3];
      if (o2 >= 0) {
        const double v = wave_sum(fma(p0[i1], p0[i2], p1[i1] * p1[i2]));
        if (lane == 0) outA[c1 * D + o2 + i2 % 3] = v;
      }
    }
#pragma unroll
    for (int k = 0; k < kBaMaxIntr; ++k) {
      const int q = d.intr_col[k];
      if (q >= 0) {
        const double v = wave_sum(fma(p0[i1], j0[k], p1[i1] * j1[k]));
        if (lane == 0) outE[c1 * a + q] = v;
      }
    }
  }
}

// one workgroup = 16 views (16 lanes each): A_v^-1, W_v and the workgroup's part of the sum of E_v' W_v.  The arrow columns are
// scaled on the pose side only (E_v S_v); the corner kernel applies the intrinsics' own factors to the sum, so this step does not
// wait for the corner's diagonal.
template <int D>
__device__ __forceinline__ void ba_cov_views(const NormalEq& ne, const int64_t* view_c0, int nv, int a, const BaCovBuffers& cb, int group) {
  __shared__ double red[kBcThreads / 64][kBcLanes][kBaIntr];
  const int tid = threadIdx.x, q = tid & (kBcLanes - 1);
  const int v = group * kBcViews + (tid >> 4);
  const int Pb = nv * D;
  bool used = v < nv;
  if (used) used = view_c0[v + 1] > view_c0[v];
  double e[D], w[D];
#pragma unroll
  for (int r = 0; r < D; ++r) { e[r] = 0.0; w[r] = 0.0; }
  if (used) {
    // chunks [k0, k1) of a view of three or more: its block and arrow rows are the chunk partials added in chunk order
    int k0 = 0, k1 = 0;
    if (cb.view_chunk0 != nullptr && cb.view_chunk0[v + 1] - cb.view_chunk0[v] >= 3) { k0 = cb.view_chunk0[v]; k1 = cb.view_chunk0[v + 1]; }
    const double* b = ne.band() + (int64_t)v * D * D;   // band rows v*D + r of width D: b[r*D + (c-r)] = H(r, c), c >= r
    double A[D][D], Z[D][D];
#pragma unroll
    for (int r = 0; r < D; ++r) {
#pragma unroll
      for (int c = r; c < D; ++c) {
        double h = b[r * D + (c - r)];
        if (k1 > k0) { h = 0.0; for (int k = k0; k < k1; ++k) h += cb.chunkA[(int64_t)k * D * D + r * D + c]; }
        A[r][c] = h;
      }
    }
    double s[D];
    int bad_r = 0;
    bool ok = ba_cov_pose_scale<D>(A, s, &bad_r);
    if (!ok && q == 0) atomicMin(&cb.res->bad_diag, v * D + bad_r);
    if (q == 0) {
#pragma unroll
      for (int r = 0; r < D; ++r) cb.Sv[(int64_t)v * D + r] = s[r];   // the hand-out kernel unscales with these
    }
#pragma unroll
    for (int r = 0; r < D; ++r) {
      A[r][r] = 1.0;
#pragma unroll
      for (int c = r + 1; c < D; ++c) { const double h = A[r][c] * (s[r] * s[c]); A[r][c] = h; A[c][r] = h; }
    }
    if (ok) {
      ok = ba_cov_spd_inverse<D>(A, Z);
      if (!ok && q == 0) atomicMin(&cb.res->bad_pivot, v);
    }
    const double nanv = __builtin_nan("");
    if (q == 0) {
      double* out = cb.Ainv + (int64_t)v * (D * (D + 1) / 2);
      int k = 0;
#pragma unroll
      for (int r = 0; r < D; ++r) {
#pragma unroll
        for (int c = r; c < D; ++c) out[k++] = ok ? Z[r][c] : nanv;
      }
    }
    if (q < a) {
      double* wout = cb.Wv + ((int64_t)v * D) * a + q;
      if (ok) {
        const double* eg = ne.Et() + (int64_t)q * Pb + (int64_t)v * D;
#pragma unroll
        for (int r = 0; r < D; ++r) {
          double h = eg[r];
          if (k1 > k0) { h = 0.0; for (int k = k0; k < k1; ++k) h += cb.chunkE[((int64_t)k * D + r) * a + q]; }
          e[r] = h * s[r];
        }
#pragma unroll
        for (int r = 0; r < D; ++r) {
          double t = 0.0;
#pragma unroll
          for (int c = 0; c < D; ++c) t = fma(Z[r][c], e[c], t);
          w[r] = t;
          wout[(int64_t)r * a] = t;
        }
      } else {
#pragma unroll
        for (int r = 0; r < D; ++r) wout[(int64_t)r * a] = nanv;
      }
    }
  }
  if (a == 0) return;
  // column q of E_v' W_v, then the fixed-order sum over the 16 views of the workgroup
  double col[kBaIntr];
#pragma unroll
  for (int q1 = 0; q1 < kBaIntr; ++q1) {
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < D; ++r) acc = fma(__shfl(e[r], q1, kBcLanes), w[r], acc);
    acc += __shfl_xor(acc, 16, 64);
    acc += __shfl_xor(acc, 32, 64);
    col[q1] = acc;
  }
  if ((tid & 63) < kBcLanes) {
#pragma unroll
    for (int q1 = 0; q1 < kBaIntr; ++q1) red[tid >> 6][q][q1] = col[q1];
  }
  __syncthreads();
  if (tid < a) {
    double* out = cb.part + (int64_t)group * a * a;
#pragma unroll
    for (int q1 = 0; q1 < kBaIntr; ++q1)
      if (q1 < a) out[q1 * a + tid] = ((red[0][tid][q1] + red[1][tid][q1]) + red[2][tid][q1]) + red[3][tid][q1];
  }
}

// ONE launch for the two independent front steps: workgroups [0, groups) take 16 views each, the workgroups behind them four chunks
// of the corner sum each (one wave per chunk).  The branch is uniform per workgroup.
template <int D>
__global__ void __launch_bounds__(kBcThreads) ba_cov_front_kernel(const double* x, BaData d, NormalEq ne, int groups, BaCovBuffers cb) {
  if ((int)blockIdx.x < groups) { ba_cov_views<D>(ne, d.view_c0, int(d.n_views), d.n_arrow, cb, blockIdx.x); return; }
  const int chunk = ((int)blockIdx.x - groups) * (kBcThreads / 64) + (threadIdx.x >> 6);
  if (chunk < d.n_chunks) ba_cov_corner_rows(x, d, cb, chunk, threadIdx.x & 63);
}

__global__ void __launch_bounds__(64) ba_cov_corner_kernel(int nv, int Pb, int a, int n_chunks, int nparts, BaCovBuffers cb) {
  constexpr int LD = kBaIntr + 1;
  __shared__ double Lc[kBaIntr * LD], Xi[kBaIntr * LD], Cs[kBaIntr * kBaIntr], sc[kBaIntr];
  __shared__ int s_fail;
  const int lane = threadIdx.x;
  if (lane == 0) s_fail = -1;
  for (int e = lane; e < a * a; e += 64) {
    double acc = 0.0;
    for (int b = 0; b < n_chunks; ++b) acc += cb.chunkC[(int64_t)b * a * a + e];   // chunk order
    Cs[e] = acc;
    cb.C[e] = acc;   // the hand-out kernel takes the intrinsics' scale factors from its diagonal
  }
  for (int e = lane; e < kBaIntr * LD; e += 64) { Lc[e] = 0.0; Xi[e] = 0.0; }
  __syncthreads();
  if (lane < a) {
    const double c = Cs[lane * a + lane];
    const bool ok = ba_cov_positive(c);
    if (!ok) atomicMin(&cb.res->bad_diag, Pb + lane);
    sc[lane] = ok ? 1.0 / sqrt(c) : 0.0;
  }
  __syncthreads();
  for (int e = lane; e < a * a; e += 64) {
    const int r = e / a, c = e - r * a;
    double acc = 0.0;
    for (int b = 0; b < nparts; ++b) acc += cb.part[(int64_t)b * a * a + e];   // workgroup order
    Lc[r * LD + c] = (r == c ? 1.0 : Cs[e] * (sc[r] * sc[c])) - acc * (sc[r] * sc[c]);
  }
  __syncthreads();
  for (int c = 0; c < a; ++c) {
    if (lane == 0) { double piv = Lc[c * LD + c]; if (!(piv > 0.0)) { if (s_fail < 0) s_fail = c; piv = 1.0; } Lc[c * LD + c] = sqrt(piv); }
    __syncthreads();
    const double d = Lc[c * LD + c];
    if (lane > c && lane < a) Lc[lane * LD + c] /= d;
    __syncthreads();
    const int nrem = a - (c + 1);
    for (int e = lane; e < nrem * nrem; e += 64) {
      const int c2 = c + 1 + e / nrem, r = c + 1 + e % nrem;
      if (r >= c2) Lc[r * LD + c2] = fma(-Lc[r * LD + c], Lc[c2 * LD + c], Lc[r * LD + c2]);
    }
    __syncthreads();
  }
  if (lane < a) {   // X = L^-1: lane c solves L x = e_c
    const int c = lane;
    for (int r = c; r < a; ++r) {
      double v = r == c ? 1.0 : 0.0;
      for (int k = c; k < r; ++k) v = fma(-Lc[r * LD + k], Xi[k * LD + c], v);
      Xi[r * LD + c] = v / Lc[r * LD + r];
    }
  }
  __syncthreads();
  for (int e = lane; e < a * a; e += 64) {   // Sigma = X'X; (r, c) and (c, r) add the same products in the same order
    const int r = e / a, c = e - r * a;
    double v = 0.0;
    for (int k = r > c ? r : c; k < a; ++k) v = fma(Xi[k * LD + r], Xi[k * LD + c], v);
    cb.Zth[e] = v;
    cb.cov_th[e] = v * (sc[r] * sc[c]);
    if (r == c) Lc[r * LD + r] = v;   // the factor is no longer needed: keep the diagonal for the maximum
  }
  __syncthreads();
  if (lane == 0) {
    double zmax = 0.0;
    int fail = s_fail;
    for (int r = a - 1; r >= 0; --r) { const double z = Lc[r * LD + r]; if (ba_cov_positive(z)) zmax = fmax(zmax, z); else if (fail < 0 || r < fail) fail = r; }
    if (fail >= 0) atomicMin(&cb.res->bad_pivot, nv + fail);
    cb.res->zmax_bits = (unsigned long long)__double_as_longlong(zmax);   // the hand-out kernel raises it (stream ordered behind this store)
  }
}

template <int D>
__global__ void __launch_bounds__(kBcThreads) ba_cov_handout_kernel(const int64_t* view_c0, int nv, int a, BaCovBuffers cb) {
  __shared__ double Zs[kBaIntr * kBaIntr];
  const int tid = threadIdx.x, q = tid & (kBcLanes - 1);
  const int v = blockIdx.x * kBcViews + (tid >> 4);
  if (tid < a * a) Zs[tid] = cb.Zth[tid];
  __syncthreads();
  bool used = v < nv;
  if (used) used = view_c0[v + 1] > view_c0[v];
  double s[D], w[D], T[D];
  double sq = 0.0;
#pragma unroll
  for (int r = 0; r < D; ++r) { s[r] = 0.0; w[r] = 0.0; T[r] = 0.0; }
  if (used) {
#pragma unroll
    for (int r = 0; r < D; ++r) s[r] = cb.Sv[(int64_t)v * D + r];
    if (q < a) {
      const double cq = cb.C[(int64_t)q * a + q];
      sq = ba_cov_positive(cq) ? 1.0 / sqrt(cq) : 0.0;
      const double* wg = cb.Wv + ((int64_t)v * D) * a + q;
#pragma unroll
      for (int r = 0; r < D; ++r) w[r] = wg[(int64_t)r * a] * sq;   // (stored with the pose side scaled only)
    }
  }
  // column q of T = W_v Sigma
#pragma unroll
  for (int q1 = 0; q1 < kBaIntr; ++q1) {
    if (q1 < a) {
      const double z = q < a ? Zs[q1 * a + q] : 0.0;
#pragma unroll
      for (int r = 0; r < D; ++r) T[r] = fma(__shfl(w[r], q1, kBcLanes), z, T[r]);
    }
  }
  const double nanv = __builtin_nan("");
  if (v < nv && q < a) {
    double* out = cb.cross + ((int64_t)v * D) * a + q;
#pragma unroll
    for (int r = 0; r < D; ++r) out[(int64_t)r * a] = used ? -T[r] * (s[r] * sq) : nanv;
  }
  // W_v Sigma W_v' = sum over the lanes of T[:, q] w_q'
  double M[D][D];
#pragma unroll
  for (int r = 0; r < D; ++r) {
#pragma unroll
    for (int c = r; c < D; ++c) {
      double p = T[r] * w[c];
      p += __shfl_xor(p, 1, 64); p += __shfl_xor(p, 2, 64); p += __shfl_xor(p, 4, 64); p += __shfl_xor(p, 8, 64);
      M[r][c] = p;
    }
  }
  double zmax = 0.0;
  if (v < nv && q == 0) {
    double* out = cb.cov_pose + (int64_t)v * D * D;
    const double* ai = cb.Ainv + (int64_t)v * (D * (D + 1) / 2);
    bool ok = true;
    int k = 0;
#pragma unroll
    for (int r = 0; r < D; ++r) {
#pragma unroll
      for (int c = r; c < D; ++c) {
        const double z = used ? ai[k] + M[r][c] : nanv;
        ++k;
        const double o = z * (s[r] * s[c]);
        out[r * D + c] = o; out[c * D + r] = o;
        if (r == c && used) { if (ba_cov_positive(z)) zmax = fmax(zmax, z); else ok = false; }
      }
    }
    if (!ok) atomicMin(&cb.res->bad_pivot, v);
  }
  zmax = fmax(zmax, __shfl_xor(zmax, 16, 64));
  zmax = fmax(zmax, __shfl_xor(zmax, 32, 64));
  if ((tid & 63) == 0 && zmax > 0.0) atomicMax(&cb.res->zmax_bits, (unsigned long long)__double_as_longlong(zmax));
}

void launch_ba_covariance(const double* x, const NormalEq& ne, const BaData& d, const BaCovBuffers& cb, hipStream_t st) {
  const int nv = int(d.n_views), D = d.pose_dim, a = d.n_arrow;
  const int groups = (D > 0 && nv > 0) ? (nv + kBcViews - 1) / kBcViews : 0;
  const bool big = cb.view_chunk0 != nullptr && D > 0;              // a view of three or more chunks: its partials come first
  const int n_chunks = a > 0 ? d.n_chunks : 0;                       // the corner sum
  const int chunk_groups = ((a > 0 || big ? d.n_chunks : 0) + kBcThreads / 64 - 1) / (kBcThreads / 64);
  (void)hipMemsetAsync(&cb.res->bad_diag, 0x7f, 2 * sizeof(int32_t), st);   // "none": a large index (0x7f7f7f7f)
  auto front = [&](int g, int cg) {
    if (g + cg == 0) return;
    if (D == 6) hipLaunchKernelGGL(ba_cov_front_kernel<6>, dim3(g + cg), dim3(kBcThreads), 0, st, x, d, ne, g, cb);
    else hipLaunchKernelGGL(ba_cov_front_kernel<3>, dim3(g + cg), dim3(kBcThreads), 0, st, x, d, ne, g, cb);   // (D = 0: g = 0, chunk workgroups only)
  };
  if (big) { front(0, chunk_groups); front(groups, 0); }
  else front(groups, chunk_groups);
  hipLaunchKernelGGL(ba_cov_corner_kernel, dim3(1), dim3(64), 0, st, nv, nv * D, a, n_chunks, a > 0 ? groups : 0, cb);
  if (groups > 0) {
    if (D == 6) hipLaunchKernelGGL(ba_cov_handout_kernel<6>, dim3(groups), dim3(kBcThreads), 0, st, d.view_c0, nv, a, cb);
    else hipLaunchKernelGGL(ba_cov_handout_kernel<3>, dim3(groups), dim3(kBcThreads), 0, st, d.view_c0, nv, a, cb);
  }
}

}  // namespace oicc
