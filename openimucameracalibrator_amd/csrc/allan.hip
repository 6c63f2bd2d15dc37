// IMU noise characterisation (applications/fit_allan_variance.cc of the reference): the overlapping Allan variance of
// every channel at every cluster size on the device, the cluster-size list and the five-term noise-model fit on the host.
//   AllanGyr / AllanAcc          src/allanvariance/allan_gyr.cc, allan_acc.cc (same arithmetic, different units)
//     calc()                     :39-71    avgDt, theta, strides, variance
//     calcVariance               :104-125  sigma2(m) = sum (th[k+2m] - 2 th[k+m] + th[k])^2 / (2 (period m)^2 (n - 2m))
//     calcThetas                 :130-139  th[k] = (w[0] + ... + w[k]) / freq
//     initStrides / getLogSpace  :141-196  the cluster-size (factor) list
//     getAvgDt                   :205-214
//   FitAllanGyr / FitAllanAcc    src/allanvariance/fitallan_gyr.cc, fitallan_acc.cc, residual in fitallan_*.h
//
// Device layout (DESIGN.md "Allan variance"): a workgroup owns one channel, one chunk of kChunkTiles k-tiles of kTile
// samples and a group of consecutive factors m_1..m_G with m_G - m_1 <= kSpan.  Per tile it stages th[k0, k0+T),
// th[k0+m_1, k0+m_G+T) and th[k0+2m_1, k0+2m_G+T) in LDS once and evaluates all G*T terms from there.  Each factor gets
// 256/G' lanes (G' = G rounded up to a power of two); a lane sums its terms in fp64 over the whole chunk, the lanes of a
// factor are combined by a fixed tree, and one partial per (channel, factor, chunk) is written.  A second launch adds
// the partials of a factor in chunk order.  No atomics: repeated calls are bitwise identical.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>
#include "../../include/oicc_hip.h"
#include "hip_resources.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 1024;        // k samples per staged tile
constexpr int kSpan = 1024;        // largest m_G - m_1 inside a factor group
constexpr int kMaxGroup = 256;     // factors per group (one lane each at least)
constexpr int kChunkTiles = 16;    // tiles per workgroup: one partial per (channel, factor) for every kChunkTiles * kTile samples
constexpr int64_t kChunk = int64_t(kTile) * kChunkTiles;
constexpr int kScanThreads = 1024;
constexpr int kScanPerThread = 8;

// th[c][k] = (sum_{i<=k} (w[c][i] * scale[c] - mean[c])) / freq, one workgroup per channel.  Subtracting the mean removes a
// linear trend that the second difference annihilates exactly; what is left has far less cancellation.
__global__ __launch_bounds__(kScanThreads) void allan_scan_kernel(const double* __restrict__ w, int64_t n, const double* __restrict__ scale,
                                                                   const double* __restrict__ mean, double freq, double* __restrict__ theta) {
  __shared__ double wave_tot[kScanThreads / 64];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* src = w + int64_t(c) * n;
  double* dst = theta + int64_t(c) * n;
  const double s = scale[c], mu = mean[c];
  double carry = 0.0;
  for (int64_t base = 0; base < n; base += int64_t(kScanThreads) * kScanPerThread) {
    const int64_t i0 = base + int64_t(tid) * kScanPerThread;
    double v[kScanPerThread];
    double run = 0.0;
#pragma unroll
    for (int j = 0; j < kScanPerThread; ++j) {
      const int64_t i = i0 + j;
      run += i < n ? src[i] * s - mu : 0.0;
      v[j] = run;
    }
    // inclusive scan of the thread totals inside the wave, then over the waves
    double x = run;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const double y = __shfl_up(x, d, 64); if (lane >= d) x += y; }
    if (lane == 63) wave_tot[wave] = x;
    __syncthreads();
    double before = carry;
    for (int q = 0; q < wave; ++q) before += wave_tot[q];
    double block_total = 0.0;
    for (int q = 0; q < kScanThreads / 64; ++q) block_total += wave_tot[q];
    const double excl = before + (x - run);
#pragma unroll
    for (int j = 0; j < kScanPerThread; ++j) {
      const int64_t i = i0 + j;
      if (i < n) dst[i] = (excl + v[j]) / freq;
    }
    carry += block_total;
    __syncthreads();   // wave_tot is rewritten by the next chunk
  }
}

struct WorkItem { int32_t f_begin, count, span, chunk; int64_t out; };

__global__ __launch_bounds__(kThreads) void allan_partial_kernel(const double* __restrict__ theta, int64_t n, const int32_t* __restrict__ factors,
                                                                  const WorkItem* __restrict__ items, double* __restrict__ partial, int64_t part_stride) {
  __shared__ double sA[kTile], sB[kTile + kSpan], sC[kTile + 2 * kSpan], red[kThreads];
  const int c = blockIdx.y, tid = threadIdx.x;
  const WorkItem it = items[blockIdx.x];
  const double* th = theta + int64_t(c) * n;
  const int64_t m1 = factors[it.f_begin];
  int gp = 1; while (gp < it.count) gp <<= 1;
  const int L = kThreads / gp;                 // lanes per factor (power of two)
  const int g = tid / L, l = tid % L;
  const int64_t m = g < it.count ? factors[it.f_begin + g] : m1;
  const int64_t d = m - m1;
  const int64_t kend = n - 2 * m;              // terms k < kend
  const int64_t kend1 = n - 2 * m1;
  const int nb = kTile + it.span, nc = kTile + 2 * it.span;
  double acc = 0.0;
  for (int t = 0; t < kChunkTiles; ++t) {
    const int64_t k0 = int64_t(it.chunk) * kChunk + int64_t(t) * kTile;
    if (k0 >= kend1) break;                    // uniform over the workgroup
    __syncthreads();                           // the previous tile's reads are done
    for (int i = tid; i < kTile; i += kThreads) { const int64_t k = k0 + i; sA[i] = k < n ? th[k] : 0.0; }
    for (int i = tid; i < nb; i += kThreads) { const int64_t k = k0 + m1 + i; sB[i] = k < n ? th[k] : 0.0; }
    for (int i = tid; i < nc; i += kThreads) { const int64_t k = k0 + 2 * m1 + i; sC[i] = k < n ? th[k] : 0.0; }
    __syncthreads();
    if (g < it.count) {
      const int kmax = int(std::min<int64_t>(kTile, kend - k0));
      for (int i = l; i < kmax; i += L) {
        const double e = sC[i + 2 * d] - 2.0 * sB[i + d] + sA[i];
        acc = fma(e, e, acc);
      }
    }
  }
  red[tid] = acc;
  __syncthreads();
  for (int s = L >> 1; s > 0; s >>= 1) {       // fixed-order tree over the lanes of one factor
    if (l < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (l == 0 && g < it.count) partial[int64_t(c) * part_stride + it.out + g] = red[tid];
}

// sigma2[c][f] = sum over the chunks of f's group, in chunk order, / (2 (period m)^2 (n - 2m));  NaN where n - 2m <= 0
__global__ void allan_reduce_kernel(const double* __restrict__ partial, int64_t part_stride, const int64_t* __restrict__ f_out,
                                    const int32_t* __restrict__ f_stride, const int32_t* __restrict__ f_chunks, const int32_t* __restrict__ factors,
                                    int32_t nf, int64_t n, double period, double* __restrict__ sigma2) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
  if (f >= nf) return;
  const int64_t m = factors[f];
  double r = NAN;
  if (n - 2 * m > 0) {
    const double* p = partial + int64_t(c) * part_stride + f_out[f];
    double s = 0.0;
    for (int q = 0; q < f_chunks[f]; ++q) s += p[int64_t(q) * f_stride[f]];
    const double cp2 = (period * double(m)) * (period * double(m));
    r = s / (2.0 * cp2 * double(n - 2 * m));
  }
  sigma2[int64_t(c) * nf + f] = r;
}

// ---- host: factor list (initStrides + getLogSpace, allan_gyr.cc:141-196), kept operation for operation ----
int32_t factor_list(int64_t n, int32_t num_clusters, int32_t* out) {
  int mode = int(n / 2);
  unsigned int max_stride = 1;
  int shft = 0;
  while (mode) { mode = mode >> 1; max_stride = 1u << shft; shft++; }
  const float a = 0.0f, b = float(std::log10(double(max_stride)));     // getLogSpace(float a, float b)
  const double start = std::pow(10.0, double(a));
  const double end = std::pow(10.0, double(b));
  const double progression = std::pow(end / start, double(1.0f / float(num_clusters - 1)));
  double prev = std::ceil(start), v = start;
  int32_t nf = 1;
  out[0] = int32_t(prev);
  for (int i = 1; i < num_clusters; ++i) {
    v = v * progression;
    const double cv = std::ceil(v);
    if (cv != prev) out[nf++] = int32_t(cv);
    prev = cv;
  }
  return nf;
}

// ---- host: the fit (FitAllanGyr / FitAllanAcc) ----
// residual r_i(p) = log10(Q^2/tau^2 + N^2/tau + B^2 + K^2 tau + R^2 tau^2) - log10(sigma2_i)  (fitallan_*.h AllanSigmaError)
double model_sigma2(const double* p, double tau) {
  return p[0] * p[0] / (tau * tau) + p[1] * p[1] / tau + p[2] * p[2] + p[3] * p[3] * tau + p[4] * p[4] * tau * tau;
}

struct FitData { std::vector<double> tau, s2; };

double eval_cost(const FitData& D, const double* p, std::vector<double>* r, std::vector<double>* J) {
  const size_t m = D.tau.size();
  const double ln10 = std::log(10.0);
  double cost = 0.0;
  for (size_t i = 0; i < m; ++i) {
    const double t = D.tau[i], s = model_sigma2(p, t);
    const double ri = std::log(s) / ln10 - std::log(D.s2[i]) / ln10;
    if (r) (*r)[i] = ri;
    if (J) {
      const double k = 1.0 / (s * ln10);
      double* row = J->data() + 5 * i;
      row[0] = k * 2.0 * p[0] / (t * t); row[1] = k * 2.0 * p[1] / t; row[2] = k * 2.0 * p[2];
      row[3] = k * 2.0 * p[3] * t; row[4] = k * 2.0 * p[4] * t * t;
    }
    cost += ri * ri;
  }
  return 0.5 * cost;
}

// least squares min |A y - b| for A [rows][5] by Householder QR (what Ceres' DENSE_QR does on [J; D])
bool qr_solve5(std::vector<double> A, std::vector<double> b, double y[5]) {
  const size_t rows = b.size();
  for (int j = 0; j < 5; ++j) {
    double nrm = 0.0;
    for (size_t i = size_t(j); i < rows; ++i) nrm += A[5 * i + j] * A[5 * i + j];
    nrm = std::sqrt(nrm);
    if (!(nrm > 0.0) || !std::isfinite(nrm)) return false;
    const double alpha = A[5 * j + j] > 0 ? -nrm : nrm;
    // v = x - alpha e_j, stored in column j below the diagonal
    std::vector<double> v(rows - size_t(j));
    for (size_t i = size_t(j); i < rows; ++i) v[i - size_t(j)] = A[5 * i + j];
    v[0] -= alpha;
    double vv = 0.0; for (double e : v) vv += e * e;
    if (!(vv > 0.0)) continue;
    for (int k = j; k < 5; ++k) {
      double dot = 0.0; for (size_t i = size_t(j); i < rows; ++i) dot += v[i - size_t(j)] * A[5 * i + k];
      const double f = 2.0 * dot / vv;
      for (size_t i = size_t(j); i < rows; ++i) A[5 * i + k] -= f * v[i - size_t(j)];
    }
    double dot = 0.0; for (size_t i = size_t(j); i < rows; ++i) dot += v[i - size_t(j)] * b[i];
    const double f = 2.0 * dot / vv;
    for (size_t i = size_t(j); i < rows; ++i) b[i] -= f * v[i - size_t(j)];
  }
  for (int j = 4; j >= 0; --j) {
    double s = b[size_t(j)];
    for (int k = j + 1; k < 5; ++k) s -= A[5 * size_t(j) + k] * y[k];
    y[j] = s / A[5 * size_t(j) + j];
  }
  for (int j = 0; j < 5; ++j) if (!std::isfinite(y[j])) return false;
  return true;
}

// initValue (fitallan_gyr.cc:62-101): C = (F^T F)^-1 F^T Y, F_ik = sqrt(tau_i)^(k-2), Y_i = sqrt(sigma2_i); the inverse as
// Eigen's MatrixXd::inverse() forms it (partial-pivot LU, then the inverse times F^T Y)
void init_value(const FitData& D, double C[5]) {
  double A[5][5] = {}, B[5] = {};
  for (size_t i = 0; i < D.tau.size(); ++i) {
    double F[5];
    const double st = std::sqrt(D.tau[i]);
    for (int k = 0; k < 5; ++k) F[k] = std::pow(st, k - 2);
    const double y = std::sqrt(D.s2[i]);
    for (int r = 0; r < 5; ++r) { B[r] += F[r] * y; for (int k = 0; k < 5; ++k) A[r][k] += F[r] * F[k]; }
  }
  double LU[5][5]; int perm[5];
  for (int r = 0; r < 5; ++r) { perm[r] = r; for (int k = 0; k < 5; ++k) LU[r][k] = A[r][k]; }
  for (int j = 0; j < 5; ++j) {
    int p = j; for (int r = j + 1; r < 5; ++r) if (std::fabs(LU[r][j]) > std::fabs(LU[p][j])) p = r;
    if (p != j) { for (int k = 0; k < 5; ++k) std::swap(LU[p][k], LU[j][k]); std::swap(perm[p], perm[j]); }
    for (int r = j + 1; r < 5; ++r) {
      LU[r][j] /= LU[j][j];
      for (int k = j + 1; k < 5; ++k) LU[r][k] -= LU[r][j] * LU[j][k];
    }
  }
  double inv[5][5];
  for (int col = 0; col < 5; ++col) {
    double x[5];
    for (int r = 0; r < 5; ++r) x[r] = perm[r] == col ? 1.0 : 0.0;
    for (int r = 0; r < 5; ++r) for (int k = 0; k < r; ++k) x[r] -= LU[r][k] * x[k];
    for (int r = 4; r >= 0; --r) { for (int k = r + 1; k < 5; ++k) x[r] -= LU[r][k] * x[k]; x[r] /= LU[r][r]; }
    for (int r = 0; r < 5; ++r) inv[r][col] = x[r];
  }
  for (int r = 0; r < 5; ++r) { C[r] = 0.0; for (int k = 0; k < 5; ++k) C[r] += inv[r][k] * B[k]; }
}

// ceres::Solve with trust_region_strategy_type = DOGLEG and every other Solver::Options default (Ceres 2.1.0 [EXT]):
// TrustRegionMinimizer (Jacobi scaling fixed at iteration 0, step accepted when the relative decrease exceeds
// min_relative_decrease; parameter / function / gradient tolerances as there) and DoglegStrategy, TRADITIONAL_DOGLEG
// (Powell's dog leg, Nocedal & Wright, Numerical Optimization, 2nd ed., Alg. 4.1 and Section 4.1; Madsen, Nielsen &
// Tingleff, Methods for Non-Linear Least Squares Problems, 2004, Section 3.3): the trust region is the ellipsoid
// |D step| <= radius with D = sqrt(clamp(diag(J^T J), 1e-6, 1e32)); the Gauss-Newton point solves [J; sqrt(mu) D] y = [r; 0]
// (mu from 1e-8, x10 while the solve fails, back to max(1e-8, mu / 5) on acceptance); the Cauchy point is
// alpha = |g|^2 / |J D^-1 g|^2 along -g (g = D^-1 J^T r); radius halves on rejection, halves on a poor step (rho < 0.25) and
// grows to 3 |D step| on a good one (rho > 0.75).  Returns the number of iterations.
int dogleg_fit(const FitData& D, double p[5], double* final_cost) {
  const int max_iters = 50;
  const double ftol = 1e-6, gtol = 1e-10, ptol = 1e-8, min_rel_dec = 1e-3, min_radius = 1e-32, max_radius = 1e16;
  const double min_diag = 1e-6, max_diag = 1e32, min_mu = 1e-8, max_mu = 1.0, mu_inc = 10.0;
  const int max_invalid = 5;
  const size_t m = D.tau.size();
  std::vector<double> r(m), J(5 * m), rc(m);
  double cost = eval_cost(D, p, &r, &J);
  double scale[5];
  for (int k = 0; k < 5; ++k) { double s = 0; for (size_t i = 0; i < m; ++i) s += J[5 * i + k] * J[5 * i + k]; scale[k] = 1.0 / (1.0 + std::sqrt(s)); }
  auto scale_jac = [&]() { for (size_t i = 0; i < m; ++i) for (int k = 0; k < 5; ++k) J[5 * i + k] *= scale[k]; };
  auto grad_max = [&]() { double g = 0; for (int k = 0; k < 5; ++k) { double s = 0; for (size_t i = 0; i < m; ++i) s += J[5 * i + k] * r[i]; g = std::max(g, std::fabs(s / scale[k])); } return g; };
  scale_jac();
  double radius = 1e4, mu = min_mu;
  int iter = 0, invalid = 0;
  bool reuse = false;
  double diag[5], grad[5], gn[5], alpha = 0.0, step_norm_scaled = 0.0;
  double x_norm = 0; for (int k = 0; k < 5; ++k) x_norm += p[k] * p[k]; x_norm = std::sqrt(x_norm);
  *final_cost = cost;
  if (grad_max() <= gtol) return 0;
  while (true) {
    if (iter >= max_iters || radius <= min_radius) break;
    ++iter;
    bool valid = true;
    if (!reuse) {
      reuse = true;
      for (int k = 0; k < 5; ++k) {
        double s = 0; for (size_t i = 0; i < m; ++i) s += J[5 * i + k] * J[5 * i + k];
        diag[k] = std::sqrt(std::min(std::max(s, min_diag), max_diag));
      }
      for (int k = 0; k < 5; ++k) { double s = 0; for (size_t i = 0; i < m; ++i) s += J[5 * i + k] * r[i]; grad[k] = s / diag[k]; }
      // Cauchy point: J (D^-1 D^-1 g)
      double jg2 = 0, g2 = 0;
      for (size_t i = 0; i < m; ++i) { double s = 0; for (int k = 0; k < 5; ++k) s += J[5 * i + k] * grad[k] / diag[k]; jg2 += s * s; }
      for (int k = 0; k < 5; ++k) g2 += grad[k] * grad[k];
      alpha = g2 / jg2;
      bool solved = false;
      while (mu < max_mu) {
        std::vector<double> A(5 * (m + 5), 0.0), b(m + 5, 0.0);
        for (size_t i = 0; i < m; ++i) { for (int k = 0; k < 5; ++k) A[5 * i + k] = J[5 * i + k]; b[i] = r[i]; }
        for (int k = 0; k < 5; ++k) A[5 * (m + size_t(k)) + k] = diag[k] * std::sqrt(mu);
        double y[5];
        if (qr_solve5(A, b, y)) { for (int k = 0; k < 5; ++k) gn[k] = -y[k] * diag[k]; solved = true; break; }
        mu *= mu_inc;
      }
      if (!solved) valid = false;
    }
    double step[5] = {0, 0, 0, 0, 0};
    if (valid) {   // ComputeTraditionalDoglegStep, in the D-scaled space
      double gnorm = 0, gnn = 0; for (int k = 0; k < 5; ++k) { gnorm += grad[k] * grad[k]; gnn += gn[k] * gn[k]; }
      gnorm = std::sqrt(gnorm); gnn = std::sqrt(gnn);
      if (gnn <= radius) { for (int k = 0; k < 5; ++k) step[k] = gn[k]; step_norm_scaled = gnn; }
      else if (gnorm * alpha >= radius) { for (int k = 0; k < 5; ++k) step[k] = -(radius / gnorm) * grad[k]; step_norm_scaled = radius; }
      else {
        double gdotgn = 0; for (int k = 0; k < 5; ++k) gdotgn += grad[k] * gn[k];
        const double b_dot_a = -alpha * gdotgn;
        const double a2 = std::pow(alpha * gnorm, 2.0);
        const double bma2 = a2 - 2 * b_dot_a + std::pow(gnn, 2);
        const double c = b_dot_a - a2;
        const double dd = std::sqrt(c * c + bma2 * (std::pow(radius, 2.0) - a2));
        const double beta = (c <= 0) ? (dd - c) / bma2 : (radius * radius - a2) / (dd + c);
        double s2 = 0;
        for (int k = 0; k < 5; ++k) { step[k] = (-alpha * (1.0 - beta)) * grad[k] + beta * gn[k]; s2 += step[k] * step[k]; }
        step_norm_scaled = std::sqrt(s2);
      }
      for (int k = 0; k < 5; ++k) step[k] /= diag[k];
      // model cost change -(J s).(r + J s / 2) with the scaled Jacobian
      double mcc = 0;
      for (size_t i = 0; i < m; ++i) { double js = 0; for (int k = 0; k < 5; ++k) js += J[5 * i + k] * step[k]; mcc -= js * (r[i] + js / 2.0); }
      valid = mcc > 0.0 && std::isfinite(mcc);
      if (valid) {
        invalid = 0;
        double xc[5], sn = 0;
        for (int k = 0; k < 5; ++k) { const double dlt = step[k] * scale[k]; xc[k] = p[k] + dlt; }
        for (int k = 0; k < 5; ++k) sn += (p[k] - xc[k]) * (p[k] - xc[k]);
        sn = std::sqrt(sn);
        double cand = eval_cost(D, xc, nullptr, nullptr);
        if (!std::isfinite(cand)) cand = 1.79769313486231570e308;
        if (sn <= ptol * (x_norm + ptol)) break;                        // ParameterToleranceReached
        const double change = cost - cand;
        if (std::fabs(change) <= ftol * cost) break;                    // FunctionToleranceReached (candidate not taken)
        const double rho = change / mcc;
        if (rho > min_rel_dec) {                                        // HandleSuccessfulStep
          for (int k = 0; k < 5; ++k) p[k] = xc[k];
          x_norm = 0; for (int k = 0; k < 5; ++k) x_norm += p[k] * p[k]; x_norm = std::sqrt(x_norm);
          cost = eval_cost(D, p, &r, &J); scale_jac();
          *final_cost = cost;
          if (rho < 0.25) radius *= 0.5;                                // DoglegStrategy::StepAccepted
          if (rho > 0.75) radius = std::max(radius, 3.0 * step_norm_scaled);
          radius = std::min(radius, max_radius);
          mu = std::max(min_mu, 2.0 * mu / mu_inc);
          reuse = false;
          if (grad_max() <= gtol) break;
        } else {
          radius *= 0.5; reuse = true;                                  // StepRejected
        }
        continue;
      }
    }
    if (++invalid >= max_invalid) break;                                // HandleInvalidStep
    radius *= 0.5; reuse = false;                                       // StepIsInvalid
  }
  return iter;
}

}  // namespace

extern "C" int oicc_allan_factors(int64_t n, int32_t num_clusters, int32_t* factors, int32_t* num_factors) {
  if (!factors || !num_factors || n < 8 || n > INT32_MAX || num_clusters < 2) return OICC_ERR_INVALID_ARG;
  *num_factors = factor_list(n, num_clusters, factors);
  return OICC_OK;
}

extern "C" int oicc_allan_variance(int32_t device_ordinal, int32_t channels, int64_t n, const double* samples, const double* t_s,
                                   const double* scale, int32_t num_clusters, int32_t* num_factors, int32_t* factors, double* taus,
                                   double* sigma2, double* freq_out, double* period_out, double* mean_out, double* device_ms) {
  if (!samples || !t_s || !scale || !num_factors || !factors || !taus || !sigma2 || !freq_out || !period_out || !mean_out ||
      channels < 1 || n < 8 || n > INT32_MAX || num_clusters < 2) return OICC_ERR_INVALID_ARG;
  for (int64_t i = 1; i < n; ++i) if (!(t_s[i] > t_s[i - 1])) return OICC_ERR_INVALID_ARG;
  if (int rc = oicc::select_device(device_ordinal)) return rc;

  // host, sequential as the reference: getAvgDt (:205-214), freq = 1 / avgDt, period = avgDt, getAvgValue of the scaled samples
  double sum_dt = 0.0;
  for (int64_t i = 1; i < n; ++i) sum_dt += t_s[i] - t_s[i - 1];
  const double avg_dt = sum_dt / double(n - 1), freq = 1.0 / avg_dt, period = avg_dt;
  std::vector<double> mean(size_t(channels), 0.0);
  for (int c = 0; c < channels; ++c) {
    double s = 0.0; const double* w = samples + int64_t(c) * n;
    for (int64_t i = 0; i < n; ++i) s += w[i] * scale[c];
    mean[size_t(c)] = s / double(n);
  }
  const int32_t nf = factor_list(n, num_clusters, factors);
  *num_factors = nf; *freq_out = freq; *period_out = period;
  for (int c = 0; c < channels; ++c) mean_out[c] = mean[size_t(c)];
  for (int f = 0; f < nf; ++f) taus[f] = period * factors[f];          // getTimes

  // factor groups and work items; per factor: where its partials start, their stride and count
  std::vector<WorkItem> items;
  std::vector<int64_t> f_out(size_t(nf), 0);
  std::vector<int32_t> f_stride(size_t(nf), 1), f_chunks(size_t(nf), 0);
  int64_t out = 0;
  for (int f = 0; f < nf;) {
    int cnt = 1;
    while (f + cnt < nf && cnt < kMaxGroup && factors[f + cnt] - factors[f] <= kSpan) ++cnt;
    const int64_t kend1 = n - 2 * int64_t(factors[f]);
    const int32_t chunks = kend1 > 0 ? int32_t((kend1 + kChunk - 1) / kChunk) : 0;
    for (int32_t q = 0; q < chunks; ++q) items.push_back(WorkItem{f, cnt, factors[f + cnt - 1] - factors[f], q, out + int64_t(q) * cnt});
    for (int g = 0; g < cnt; ++g) { f_out[size_t(f + g)] = out + g; f_stride[size_t(f + g)] = cnt; f_chunks[size_t(f + g)] = chunks; }
    out += int64_t(chunks) * cnt;
    f += cnt;
  }
  const int64_t part_stride = std::max<int64_t>(out, 1);

  oicc::DevBuf<double> d_w, d_th, d_scale, d_mean, d_part, d_s2;
  oicc::DevBuf<int32_t> d_fac, d_fs, d_fc; oicc::DevBuf<int64_t> d_fo; oicc::DevBuf<WorkItem> d_items;
  oicc::Event e0, e1;
  oicc::Stream st;
  const size_t nw = size_t(channels) * size_t(n);
  OICC_HIP_TRY(st.create());
  OICC_HIP_TRY(e0.create()); OICC_HIP_TRY(e1.create());
  // every allocation ahead of the first copy, as ahead of the timed span
  OICC_HIP_TRY(d_w.resize(nw)); OICC_HIP_TRY(d_th.resize(nw));
  OICC_HIP_TRY(d_scale.resize(size_t(channels))); OICC_HIP_TRY(d_mean.resize(size_t(channels)));
  OICC_HIP_TRY(d_part.resize(size_t(channels) * size_t(part_stride))); OICC_HIP_TRY(d_s2.resize(size_t(channels) * nf));
  OICC_HIP_TRY(d_fac.resize(size_t(nf))); OICC_HIP_TRY(d_fs.resize(size_t(nf))); OICC_HIP_TRY(d_fc.resize(size_t(nf)));
  OICC_HIP_TRY(d_fo.resize(size_t(nf))); OICC_HIP_TRY(d_items.resize(std::max<size_t>(items.size(), 1)));
  OICC_HIP_TRY(hipMemcpyAsync(d_w.p, samples, sizeof(double) * nw, hipMemcpyHostToDevice, st));
  OICC_HIP_TRY(hipMemcpyAsync(d_scale.p, scale, sizeof(double) * channels, hipMemcpyHostToDevice, st));
  OICC_HIP_TRY(hipMemcpyAsync(d_mean.p, mean.data(), sizeof(double) * channels, hipMemcpyHostToDevice, st));
  OICC_HIP_TRY(hipMemcpyAsync(d_fac.p, factors, sizeof(int32_t) * nf, hipMemcpyHostToDevice, st));
  OICC_HIP_TRY(hipMemcpyAsync(d_fs.p, f_stride.data(), sizeof(int32_t) * nf, hipMemcpyHostToDevice, st));
  OICC_HIP_TRY(hipMemcpyAsync(d_fc.p, f_chunks.data(), sizeof(int32_t) * nf, hipMemcpyHostToDevice, st));
  OICC_HIP_TRY(hipMemcpyAsync(d_fo.p, f_out.data(), sizeof(int64_t) * nf, hipMemcpyHostToDevice, st));
  if (!items.empty()) OICC_HIP_TRY(hipMemcpyAsync(d_items.p, items.data(), sizeof(WorkItem) * items.size(), hipMemcpyHostToDevice, st));
  OICC_HIP_TRY(hipEventRecord(e0, st));
  hipLaunchKernelGGL(allan_scan_kernel, dim3(channels), dim3(kScanThreads), 0, st, d_w.p, n, d_scale.p, d_mean.p, freq, d_th.p);
  if (!items.empty())
    hipLaunchKernelGGL(allan_partial_kernel, dim3(unsigned(items.size()), channels), dim3(kThreads), 0, st, d_th.p, n, d_fac.p, d_items.p, d_part.p, part_stride);
  hipLaunchKernelGGL(allan_reduce_kernel, dim3(unsigned((nf + 255) / 256), channels), dim3(256), 0, st, d_part.p, part_stride, d_fo.p, d_fs.p, d_fc.p, d_fac.p,
                     nf, n, period, d_s2.p);
  OICC_HIP_TRY(hipGetLastError());
  OICC_HIP_TRY(hipEventRecord(e1, st));
  OICC_HIP_TRY(hipMemcpyAsync(sigma2, d_s2.p, sizeof(double) * size_t(channels) * nf, hipMemcpyDeviceToHost, st));
  OICC_HIP_TRY(hipStreamSynchronize(st));
  if (device_ms) {
    float ms = 0.0f;
    OICC_HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    *device_ms = double(ms);
  }
  return OICC_OK;
}

extern "C" int oicc_allan_fit(int32_t kind, int64_t num, const double* taus, const double* sigma2, double freq, double params_QNBKR[5],
                              double init_C[5], double report[6], int32_t* num_used, int32_t* iterations) {
  if ((kind != OICC_ALLAN_GYRO && kind != OICC_ALLAN_ACC) || num < 0 || (num > 0 && (!taus || !sigma2)) || !params_QNBKR || !report) return OICC_ERR_INVALID_ARG;
  FitData D;
  double running_max = 0.0;
  for (int64_t i = 0; i < num; ++i) {
    if (!(sigma2[i] > 0.0) || !std::isfinite(sigma2[i]) || !(taus[i] > 0.0)) continue;   // n - 2m <= 0 (NaN): left out, DESIGN.md
    if (kind == OICC_ALLAN_ACC && taus[i] < 1) {                                          // checkData, fitallan_acc.cc:120-139
      if (running_max < sigma2[i]) { running_max = sigma2[i]; continue; }
    }
    D.tau.push_back(taus[i]); D.s2.push_back(sigma2[i]);
  }
  if (D.tau.size() < 5) return OICC_ERR_INVALID_ARG;
  double C[5];
  init_value(D, C);
  if (init_C) for (int k = 0; k < 5; ++k) init_C[k] = C[k];
  double p[5];
  for (int k = 0; k < 5; ++k) p[k] = std::fabs(C[k]);
  for (int k = 0; k < 5; ++k) if (!std::isfinite(p[k])) return OICC_ERR_STATE;
  double cost = 0.0;
  const int it = dogleg_fit(D, p, &cost);
  for (int k = 0; k < 5; ++k) params_QNBKR[k] = p[k];
  // reported values (fitallan_gyr.cc:49-60,104-120; fitallan_acc.cc:52-56,104-118); findMinNum / findMinIndex start at 1000.0
  const double unit = kind == OICC_ALLAN_GYRO ? 57.3 * 3600 : 1.0;
  double mn = 1000.0; int mi = 0;
  for (size_t i = 0; i < D.tau.size(); ++i) {
    const double dev = std::sqrt(model_sigma2(p, D.tau[i]));
    mi = mn < dev ? mi : int(i);
    mn = mn < dev ? mn : dev;
  }
  report[0] = mn / unit;                                           // bias instability, min of the model deviation
  report[1] = D.tau[size_t(mi)];                                   // ... at tau*
  report[2] = std::sqrt(freq) * std::sqrt(model_sigma2(p, 1.0)) / unit;   // white noise from the model at tau = 1 s
  report[3] = std::sqrt(p[2] * p[2]) / 0.6642824703 / unit;        // bias instability from B (getB)
  report[4] = std::sqrt(freq) * (std::sqrt(p[1] * p[1]) / 60.0) * 60 / 57.3;   // white noise from N (getN), gyro line
  report[5] = cost;
  if (num_used) *num_used = int32_t(D.tau.size());
  if (iterations) *iterations = it;
  return OICC_OK;
}
