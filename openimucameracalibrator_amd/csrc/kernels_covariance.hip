// Covariance estimation: the selected inverse of the band + arrow normal equations (include/oicc_hip.h,
// oicc_estimate_covariance; DESIGN.md section 3, "Covariance").
//
//   M = [ B  E ]     B: Pb x Pb, half bandwidth hb (knots in time order)
//       [ E' C ]     C: a x a arrow corner
//
// (a) cov_scale_kernel / cov_build_kernel: Ms = S M S with s_i = 1 / sqrt(M_ii) -- unit diagonal, NO damping, NO clamp, zero
//     right-hand side -- in the storage of the LM solve (kernels_cholesky.hip: Mb[j*W + k] = Ms(j+k, j), Mt[q*Pb + j], Mc).
//     A diagonal entry that is not finite and positive is reported (smallest column index), never turned into a NaN.
// (b) the forward factor is the bordered band Cholesky of the LM solve (launch_band_arrow_cholesky, one workgroup, p = 1): it
//     leaves L in Mb (diagonal slot = 1 / L_jj) and Y = L^-1 Es in Mt.
// (c) cov_schur_kernel: Sc = Cs - Y'Y (one workgroup per entry, fixed summation order); cov_corner_kernel: Zaa = Sc^-1 by a
//     dense Cholesky and the inverse of its factor, one workgroup, a <= 63.
// (d) cov_sweep_kernel -- the hot path: ONE persistent workgroup walks the band columns j = Pb-1 ... 0 and keeps, in an LDS window,
//       Zb = Bs^-1 inside the band (Takahashi):  Z_ij = -(1/L_jj) sum_{j<k<=j+hb} L_kj Z_ik   (j < i <= j+hb)
//                                                Z_jj = 1/L_jj^2 - (1/L_jj) sum_k L_kj Z_kj
//       G = L^-T Y (Pb x a):                     G_j  = (Y_j - sum_{j<k<=j+hb} L_kj G_k) / L_jj
//     Per column it stores Z_jj, Z_j+1,j, Z_j+2,j (what the 3 x 3 knot blocks need) and the row G_j.
//     LDS budget (160 KiB per workgroup), window of MC x MC doubles, circular in both indices (MC a power of two > hb):
//       MC =  64 (hb <=  63): Z window  32 KiB + G window 64 x 64 doubles = 32 KiB + partial sums 16 KiB + columns 1.5 KiB =  82 KiB
//       MC = 128 (hb <= 120): Z window 128 KiB                            + partial sums 16 KiB + columns 3 KiB   = 147 KiB;
//                             no room for the G window (128 x 63 doubles = 63 KiB): its rows are re-read from the global table the
//                             sweep writes anyway (the last hb rows, L2 resident).
//     Work split of one column: the hb x hb products of the Z recurrence are spread as (entry i = lane, slice of k = wave group),
//     the hb x a products of the G recurrence as (arrow column q = lane, slice of k = wave); the window is symmetric and stored in
//     full, so a wave reads consecutive i at a fixed k: consecutive doubles, conflict free for ds_read_b64, and L_kj is a broadcast.
//     Three barriers per column; only one of them waits for global memory (the G rows of the MC = 128 build).
// (e) cov_finish_kernel: one wave per band column: T_i = G_i Zaa, the cross block -T_i, the in-band entries
//     Zb(i+d, i) + T_i . G_(i+d), d = 0..2, everything unscaled by s_i s_j; the scaled diagonal is kept for the condition estimate.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "oicc_device.h"
#include "covariance.h"

namespace oicc {

constexpr int kCovThreads = 1024;

__device__ __forceinline__ void cov_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- (a) scaling and build ---------------------------------------------------------------------------------------------------
__global__ void cov_scale_kernel(NormalEq ne, int Pb, int a, int W, double* s, int32_t* bad_column) {
  const int P = Pb + a;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < P; i += gridDim.x * blockDim.x) {
    const double d = i < Pb ? ne.band()[(int64_t)i * W] : ne.C()[(int64_t)(i - Pb) * a + (i - Pb)];
    const bool ok = d > 0.0 && d < __builtin_huge_val();
    if (!ok) atomicMin(bad_column, i);
    s[i] = ok ? 1.0 / sqrt(d) : 0.0;
  }
}

__global__ void cov_build_kernel(NormalEq ne, int Pb, int a, int W, const double* s, double* Mb, double* Mt, double* Mc, double* Cs) {
  const int ar = a + 1;
  const int64_t nb = (int64_t)Pb * W, nt = (int64_t)ar * Pb, nc = (int64_t)ar * ar;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = tid; e < nb + nt + nc; e += nth) {
    if (e < nb) {
      const int j = int(e / W), k = int(e - (int64_t)j * W);
      Mb[e] = k == 0 ? 1.0 : (j + k < Pb ? ne.band()[e] * (s[j] * s[j + k]) : 0.0);
    } else if (e < nb + nt) {
      const int64_t f = e - nb;
      const int q = int(f / Pb), i = int(f - (int64_t)q * Pb);
      Mt[f] = q < a ? ne.Et()[f] * (s[i] * s[Pb + q]) : 0.0;    // row a: the right-hand side of the LM solve, zero here
    } else {
      const int64_t f = e - nb - nt;
      const int r = int(f / ar), c = int(f - (int64_t)r * ar);
      const double v = (r < a && c < a) ? (r == c ? 1.0 : ne.C()[(int64_t)r * a + c] * (s[Pb + r] * s[Pb + c])) : 0.0;
      Mc[f] = v;
      if (r < a && c < a) Cs[(int64_t)r * a + c] = v;
    }
  }
}

// ---- (c) Schur complement onto the arrow and its inverse -------------------------------------------------------------------
__global__ void __launch_bounds__(256) cov_schur_kernel(const double* Mt, const double* Cs, int Pb, int a, double* Sc) {
  __shared__ double red[256];
  // entry (r, c), r >= c, from the linear index of the lower triangle
  int r = 0, c = blockIdx.x;
  while (c > r) { c -= r + 1; ++r; }
  const double* yr = Mt + (int64_t)r * Pb;
  const double* yc = Mt + (int64_t)c * Pb;
  double acc = 0.0;
  for (int i = threadIdx.x; i < Pb; i += 256) acc = fma(yr[i], yc[i], acc);
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) { if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h]; __syncthreads(); }
  if (threadIdx.x == 0) { const double v = Cs[(int64_t)r * a + c] - red[0]; Sc[(int64_t)r * a + c] = v; Sc[(int64_t)c * a + r] = v; }
}

// Zaa = Sc^-1 (scaled) and cov_aa = s s' Zaa; zs_diag[Pb + q] = Zaa_qq.  fail: a pivot that is not positive.
__global__ void __launch_bounds__(256) cov_corner_kernel(const double* Sc, int Pb, int a, const double* s, double* Zaa, double* cov_aa,
                                                         double* zs_diag, int32_t* fail) {
  extern __shared__ __attribute__((aligned(16))) double cov_corner_smem[];   // 65 KiB: above the static limit
  double* const Lc = cov_corner_smem;   // [64][65] Cholesky factor (lower part)
  double* const Xi = Lc + 64 * 65;      // [64][65] its inverse, X = L^-1 (lower triangular)
  __shared__ int s_fail;
  const int tid = threadIdx.x;
  if (tid == 0) s_fail = 0;
  for (int e = tid; e < 64 * 65; e += 256) { Lc[e] = 0.0; Xi[e] = 0.0; }
  __syncthreads();
  for (int e = tid; e < a * a; e += 256) { const int r = e / a, c = e - r * a; Lc[r * 65 + c] = Sc[e]; }
  __syncthreads();
  for (int c = 0; c < a; ++c) {
    if (tid == 0) { double piv = Lc[c * 65 + c]; if (!(piv > 0.0)) { s_fail = 1; piv = 1.0; } Lc[c * 65 + c] = sqrt(piv); }
    __syncthreads();
    const double d = Lc[c * 65 + c];
    for (int r = c + 1 + tid; r < a; r += 256) Lc[r * 65 + c] /= d;
    __syncthreads();
    const int nrem = a - (c + 1);
    for (int e = tid; e < nrem * nrem; e += 256) {
      const int c2 = c + 1 + e / nrem, r = c + 1 + e % nrem;
      if (r >= c2) Lc[r * 65 + c2] -= Lc[r * 65 + c] * Lc[c2 * 65 + c];
    }
    __syncthreads();
  }
  // X = L^-1: thread c solves L x = e_c (forward substitution)
  if (tid < a) {
    const int c = tid;
    for (int r = c; r < a; ++r) {
      double v = r == c ? 1.0 : 0.0;
      for (int k = c; k < r; ++k) v = fma(-Lc[r * 65 + k], Xi[k * 65 + c], v);
      Xi[r * 65 + c] = v / Lc[r * 65 + r];
    }
  }
  __syncthreads();
  // Zaa = X'X; entries (r, c) and (c, r) add the same products in the same order
  for (int e = tid; e < a * a; e += 256) {
    const int r = e / a, c = e - r * a;
    double v = 0.0;   // (fma rounds once and its product commutes: (r, c) and (c, r) get the same bits)
    for (int k = r > c ? r : c; k < a; ++k) v = fma(Xi[k * 65 + r], Xi[k * 65 + c], v);
    Zaa[e] = v;
    cov_aa[e] = v * (s[Pb + r] * s[Pb + c]);
    if (r == c) zs_diag[Pb + r] = v;
  }
  if (tid == 0 && s_fail) atomicOr(fail, 1);
}

// ---- (d) backward selected inverse --------------------------------------------------------------------------------------------
// Mb / Mt: the factor as kernels_cholesky.hip leaves it.  zb [Pb][3]: Z(j+d, j), d = 0..2 (band part only); G [Pb][a].
template <int MC, bool G_LDS>
__global__ void __launch_bounds__(kCovThreads) cov_sweep_kernel(const double* __restrict__ Mb, const double* __restrict__ Mt, int Pb, int W,
                                                                int hb, int a, double* zb, double* G) {
  extern __shared__ __attribute__((aligned(16))) double cov_smem[];
  constexpr int mask = MC - 1;
  constexpr int NSZ = kCovThreads / MC;   // slices of k in the Z recurrence
  constexpr int NSG = kCovThreads / 64;   // slices of k in the G recurrence
  double* const Zw = cov_smem;                          // [MC][MC]  Zw[(r & mask) * MC + (c & mask)], symmetric, both halves stored
  double* const pZ = Zw + MC * MC;                      // [NSZ][MC] partial sums of the Z recurrence
  double* const pG = pZ + NSZ * MC;                     // [NSG][64] partial sums of the G recurrence
  double* const lv = pG + NSG * 64;                     // [2][MC]   column j of L: lv[k] = L(j+k, j), lv[0] = 1 / L_jj; double buffered
  double* const pr = lv + 2 * MC;                       // [MC]      L(j+i, j) Z(j+i, j)
  double* const Gw = pr + MC;                           // [MC][64]  G rows of the window (G_LDS)
  const int tid = threadIdx.x, lane = tid & 63;
  const int zi = tid & mask, zs = tid / MC;             // Z recurrence: entry i = zi + 1, slice zs
  const int gq = lane, gs = tid >> 6;                   // G recurrence: arrow column gq, slice gs
  const int ksz = (hb + NSZ - 1) / NSZ, ksg = (hb + NSG - 1) / NSG;
  auto load_l = [&](int c, int k) -> double { return (c >= 0 && k <= hb && c + k < Pb) ? Mb[(int64_t)c * W + k] : 0.0; };

  for (int e = tid; e < MC * MC; e += kCovThreads) Zw[e] = 0.0;
  for (int e = tid; e < 2 * MC; e += kCovThreads) lv[e] = 0.0;
  if (G_LDS) for (int e = tid; e < MC * 64; e += kCovThreads) Gw[e] = 0.0;
  __syncthreads();
  // column Pb-1 goes to the first buffer; columns further down travel through registers one iteration ahead
  const bool l_thread = tid >= 256 && tid < 256 + MC;
  const bool y_thread = tid >= 192 && tid < 256 && lane < a;
  const int lk = tid - 256;
  double l_next = 0.0, y_next = 0.0;
  if (l_thread) { lv[lk] = load_l(Pb - 1, lk); l_next = load_l(Pb - 2, lk); }
  if (y_thread) y_next = Mt[(int64_t)lane * Pb + (Pb - 1)];
  __syncthreads();

  int buf = 0;
  for (int j = Pb - 1; j >= 0; --j, buf ^= 1) {
    const double* const lc = lv + buf * MC;
    const double dinv = lc[0];
    // ---- step 1: partial sums
    {
      double acc = 0.0;
      if (zi < hb) {
        const int k0 = 1 + zs * ksz, k1 = min(hb, k0 + ksz - 1);
        const int col = (j + 1 + zi) & mask;
        for (int k = k0; k <= k1; ++k) acc = fma(lc[k], Zw[((j + k) & mask) * MC + col], acc);
      }
      pZ[zs * MC + zi] = acc;
      double accg = 0.0;
      if (gq < a) {
        const int k0 = 1 + gs * ksg, k1 = min(hb, k0 + ksg - 1);
        if (G_LDS) { for (int k = k0; k <= k1; ++k) accg = fma(lc[k], Gw[((j + k) & mask) * 64 + gq], accg); }
        else { for (int k = k0; k <= k1 && j + k < Pb; ++k) accg = fma(lc[k], __hip_atomic_load(&G[(int64_t)(j + k) * a + gq], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), accg); }   // (agent scope: see the store)
      }
      pG[gs * 64 + gq] = accg;
    }
    cov_lds_barrier();
    // ---- step 2: the off-diagonal entries of column j of Z (threads 0..hb-1) and the row G_j (threads 192..255)
    if (tid < MC) {
      double zv = 0.0, pv = 0.0;
      if (tid < hb) {
        double sum = 0.0;
#pragma unroll
        for (int s2 = 0; s2 < NSZ; ++s2) sum += pZ[s2 * MC + tid];
        zv = -dinv * sum;
        const int r = (j + 1 + tid) & mask, c = j & mask;
        Zw[r * MC + c] = zv; Zw[c * MC + r] = zv;
        pv = lc[1 + tid] * zv;
        if (tid < 2) zb[(int64_t)j * 3 + 1 + tid] = zv;
      } else if (tid < 2) zb[(int64_t)j * 3 + 1 + tid] = 0.0;
      pr[tid] = pv;
    }
    if (y_thread) {
      double sum = 0.0;
#pragma unroll
      for (int s2 = 0; s2 < NSG; ++s2) sum += pG[s2 * 64 + lane];
      const double gv = (y_next - sum) * dinv;
      if (G_LDS) Gw[(j & mask) * 64 + lane] = gv;
      G[(int64_t)j * a + lane] = gv;
      // MC = 128: later columns read this row back from global memory.  The row is released at agent scope (the store leaves for
      // L2 before the barrier) and read with agent-scope loads, which go past the L1 -- a line fetched there for row j + 1 may
      // hold this row's bytes from before the store; workgroup scope alone would allow the read to be served from that line.
      if (!G_LDS) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    }
    __syncthreads();
    // ---- step 3: the diagonal entry (wave 0), the next column of L and row of Y (through registers)
    if (tid < 64) {
      double sum = 0.0;
#pragma unroll
      for (int t = 0; t < MC / 64; ++t) sum += pr[lane + 64 * t];
      for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
      if (lane == 0) {
        const double zjj = dinv * dinv - dinv * sum;
        Zw[(j & mask) * MC + (j & mask)] = zjj;
        zb[(int64_t)j * 3] = zjj;
      }
    }
    if (l_thread) { lv[(buf ^ 1) * MC + lk] = l_next; l_next = load_l(j - 2, lk); }
    if (y_thread) y_next = j >= 1 ? Mt[(int64_t)lane * Pb + (j - 1)] : 0.0;
    cov_lds_barrier();
  }
}

// ---- (e) knot blocks, cross blocks, unscaling ---------------------------------------------------------------------------------
// One wave per band column i.  cov3 [Pb][3]: cov(i+d, i); cross [Pb][a]: cov(i, Pb+q); zs_diag [Pb]: scaled diagonal.
__global__ void __launch_bounds__(256) cov_finish_kernel(const double* zb, const double* G, const double* Zaa, const double* s, int Pb, int a,
                                                         double* cov3, double* cross, double* zs_diag) {
  __shared__ double Zs[63 * 63];
  __shared__ double Gs[4][64];
  for (int e = threadIdx.x; e < a * a; e += 256) Zs[e] = Zaa[e];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + w;
  if (i < Pb && lane < a) Gs[w][lane] = G[(int64_t)i * a + lane];
  __syncthreads();
  if (i >= Pb) return;
  double t = 0.0;
  if (lane < a) {
    for (int q = 0; q < a; ++q) t = fma(Gs[w][q], Zs[q * a + lane], t);
    cross[(int64_t)i * a + lane] = -t * (s[i] * s[Pb + lane]);
  }
  for (int d = 0; d < 3; ++d) {
    double v = (lane < a && i + d < Pb) ? t * G[(int64_t)(i + d) * a + lane] : 0.0;
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) {
      const double z = i + d < Pb ? zb[(int64_t)i * 3 + d] + v : 0.0;
      cov3[(int64_t)i * 3 + d] = i + d < Pb ? z * (s[i] * s[i + d]) : 0.0;
      if (d == 0) zs_diag[i] = z;
    }
  }
}

// ---- board points of view bundle adjustment (oicc_ba_point_covariances) ----------------------------------------------------------
// OICC_BA_POINTS with constant cameras: J^T J is block diagonal, one 3 x 3 block per variable point (band storage, half bandwidth 2:
// band[i*3 + k] = H(i, i+k)).  One lane per point: the block scaled to unit diagonal, its Cholesky factor, the inverse of the factor,
// X'X, unscaled.  NaN for constant points (tangent offset -1) and for blocks that are not positive definite.
__global__ void ba_point_cov_kernel(const double* band, const int32_t* point_tangent, int64_t n, double* cov9) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double* out = cov9 + 9 * i;
  const double nanv = __builtin_nan("");
  const int t = point_tangent[i];
  bool ok = t >= 0;
  double c00 = nanv, c10 = nanv, c11 = nanv, c20 = nanv, c21 = nanv, c22 = nanv;
  if (ok) {
    const double* b = band + (int64_t)t * 3;
    const double h00 = b[0], h01 = b[1], h02 = b[2], h11 = b[3], h12 = b[4], h22 = b[6];
    ok = h00 > 0.0 && h11 > 0.0 && h22 > 0.0;
    if (ok) {
      const double s0 = 1.0 / sqrt(h00), s1 = 1.0 / sqrt(h11), s2 = 1.0 / sqrt(h22);
      const double a10 = h01 * (s0 * s1), a20 = h02 * (s0 * s2), a21 = h12 * (s1 * s2);
      // L (unit-diagonal matrix): l00 = 1
      const double d1 = 1.0 - a10 * a10;
      if (d1 > 0.0) {
        const double l11 = sqrt(d1), l21 = (a21 - a20 * a10) / l11;
        const double d2 = 1.0 - a20 * a20 - l21 * l21;
        if (d2 > 0.0) {
          const double l22 = sqrt(d2);
          // X = L^-1 (lower): x00 = 1
          const double x11 = 1.0 / l11, x22 = 1.0 / l22;
          const double x10 = -a10 * x11, x21 = -l21 * x11 * x22, x20 = -(a20 + l21 * x10) * x22;
          // Z = X'X, then unscale
          c00 = (1.0 + x10 * x10 + x20 * x20) * (s0 * s0);
          c10 = (x11 * x10 + x21 * x20) * (s0 * s1);
          c20 = (x22 * x20) * (s0 * s2);
          c11 = (x11 * x11 + x21 * x21) * (s1 * s1);
          c21 = (x22 * x21) * (s1 * s2);
          c22 = (x22 * x22) * (s2 * s2);
        }
      }
    }
  }
  out[0] = c00; out[1] = c10; out[2] = c20; out[3] = c10; out[4] = c11; out[5] = c21; out[6] = c20; out[7] = c21; out[8] = c22;
}

void launch_ba_point_covariances(const double* band, const int32_t* point_tangent, int64_t n, double* cov9, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(ba_point_cov_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, band, point_tangent, n, cov9);
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
size_t cov_sweep_lds_bytes(int mc, bool g_lds) {
  return sizeof(double) * (size_t(mc) * mc + size_t(kCovThreads / mc) * mc + size_t(kCovThreads / 64) * 64 + 2 * size_t(mc) + mc + (g_lds ? size_t(mc) * 64 : 0));
}

void launch_cov_build(const NormalEq& ne, const TangentLayout& tl, const CovBuffers& cb, double* Mb, double* Mt, double* Mc, hipStream_t st) {
  (void)hipMemsetAsync(cb.flags, 0x7f, sizeof(int32_t), st);       // bad column: a large index (0x7f7f7f7f)
  (void)hipMemsetAsync(cb.flags + 1, 0, sizeof(int32_t), st);      // corner failure
  hipLaunchKernelGGL(cov_scale_kernel, dim3(std::min(1024, (tl.P + 255) / 256)), dim3(256), 0, st, ne, tl.Pb, tl.a, tl.W, cb.s, cb.flags);
  hipLaunchKernelGGL(cov_build_kernel, dim3(1024), dim3(256), 0, st, ne, tl.Pb, tl.a, tl.W, (const double*)cb.s, Mb, Mt, Mc, cb.Cs);
}

void launch_cov_corner(const TangentLayout& tl, const CovBuffers& cb, const double* Mt, hipStream_t st) {
  if (tl.a == 0) return;
  hipLaunchKernelGGL(cov_schur_kernel, dim3(tl.a * (tl.a + 1) / 2), dim3(256), 0, st, Mt, (const double*)cb.Cs, tl.Pb, tl.a, cb.Sc);
  const size_t lds = 2 * 64 * 65 * sizeof(double);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(cov_corner_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(cov_corner_kernel, dim3(1), dim3(256), lds, st, (const double*)cb.Sc, tl.Pb, tl.a, (const double*)cb.s, cb.Zaa, cb.cov_aa,
                     cb.zs_diag, cb.flags + 1);
}

int launch_cov_sweep(const TangentLayout& tl, const CovBuffers& cb, const double* Mb, const double* Mt, hipStream_t st) {
  if (tl.Pb == 0) return 0;
  if (tl.hb > kCovMaxHalfBandwidth || tl.a > kCovMaxArrow) return -1;
  if (tl.hb <= 63) {
    const size_t lds = cov_sweep_lds_bytes(64, true);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(cov_sweep_kernel<64, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((cov_sweep_kernel<64, true>), dim3(1), dim3(kCovThreads), lds, st, Mb, Mt, tl.Pb, tl.W, tl.hb, tl.a, cb.zb, cb.G);
  } else {
    const size_t lds = cov_sweep_lds_bytes(128, false);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(cov_sweep_kernel<128, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((cov_sweep_kernel<128, false>), dim3(1), dim3(kCovThreads), lds, st, Mb, Mt, tl.Pb, tl.W, tl.hb, tl.a, cb.zb, cb.G);
  }
  return 0;
}

void launch_cov_finish(const TangentLayout& tl, const CovBuffers& cb, hipStream_t st) {
  if (tl.Pb == 0) return;
  hipLaunchKernelGGL(cov_finish_kernel, dim3((tl.Pb + 3) / 4), dim3(256), 0, st, (const double*)cb.zb, (const double*)cb.G, (const double*)cb.Zaa,
                     (const double*)cb.s, tl.Pb, tl.a, cb.cov3, cb.cross, cb.zs_diag);
}

}  // namespace oicc
