// micro-benchmark: what follows the panel chain in a workgroup of bcri_invert_schur_kernel (kernels_bcr.hip), in isolation, on operands
// in LDS -- one workgroup of 16 waves, the same layouts (W column major with LD = 145, X = L^-T upper triangular in rows 64..127, the
// parked B_x tile as [variable][16 rows]), the same loads, MFMA counts and barriers as the kernel's code, clock64 of wave 0 between
// workgroup barriers:
//   (z)  the parent's sequence: Z = X X^T (ten tiles, 80 MFMAs, tile t on wave t) into rows 0..63, barrier, T_x = B_x Z on four waves
//        (16 MFMAs each, two accumulators), barrier
//   (t10) T_x = (B_x X) X^T in ten chunks of 4 MFMAs per factor, one per wave: Y partials, barrier, T partials, barrier
//   (t4) the same with panel 3's four chunks only (the panels 0..2 formed in the shadow of the chains)
//   (s)  one wave forming panel 2's six chunks alone, as the shadow wave does (Y_2 through LDS behind a wave-local wait)
// The sums of (t10) are checked against a host product.
// hipcc -O3 -std=c++17 --offload-arch=gfx950 scripts/micro/tx_tail.hip -o tx_tail && ./tx_tail
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>
typedef double v4d __attribute__((ext_vector_type(4)));
constexpr int LD = 145, TS = 17, TT = 16 * TS;
constexpr int kW = 64 * LD, kP = 1024, kTP = 10 * TT, kTs = 16 * 68, kLds = kW + kP + kTP + kTs + TT;
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ void tri10(int t, int& xt, int& yt) { xt = t < 1 ? 0 : (t < 3 ? 1 : (t < 6 ? 2 : 3)); yt = t - (xt * (xt + 1)) / 2; }
__device__ __forceinline__ double* ytile(double* W, int t) { return W + 16 * (t & 3) * LD + 16 * (t >> 2); }

template <int XT>
__device__ __forceinline__ v4d z_tile(const double* W, int yt, int li, int lq) {
  constexpr int K0 = 4 * XT, NK = 16 - K0;
  const double* py = W + lq * LD + 64 + 16 * yt + li;
  const double* px = W + lq * LD + 64 + 16 * XT + li;
  double vy[NK], vx[NK];
#pragma unroll
  for (int kk = 0; kk < NK; ++kk) { vy[kk] = py[4 * (K0 + kk) * LD]; vx[kk] = px[4 * (K0 + kk) * LD]; }
  asm volatile("" ::: "memory");
  v4d g = {0, 0, 0, 0}, g2 = {0, 0, 0, 0};
#pragma unroll
  for (int kk = 0; kk < NK; kk += 2) {
    g = __builtin_amdgcn_mfma_f64_16x16x4f64(vy[kk], vx[kk], g, 0, 0, 0);
    g2 = __builtin_amdgcn_mfma_f64_16x16x4f64(vy[kk + 1], vx[kk + 1], g2, 0, 0, 0);
  }
  return g + g2;
}

// the two chunk stages; T0: first chunk (0: all ten, 6: panel 3's)
template <int T0>
__device__ __forceinline__ void tx_stage(double* W, const double* P, double* TP, int wave, int li, int lq) {
  const int chunk = wave + T0;
  int p, q; tri10(chunk < 10 ? chunk : 0, p, q);
  if (chunk < 10) {
    const double* pb = P + (16 * q + lq) * 16 + li;
    const double* px = W + (16 * p + li) * LD + 64 + 16 * q + lq;
    double vb[4], vx[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) { vb[kk] = pb[64 * kk]; vx[kk] = px[4 * kk]; }
    asm volatile("" ::: "memory");
    v4d y = {0, 0, 0, 0};
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) y = __builtin_amdgcn_mfma_f64_16x16x4f64(vb[kk], vx[kk], y, 0, 0, 0);
    double* yp = ytile(W, chunk) + li * LD + lq;
#pragma unroll
    for (int r = 0; r < 4; ++r) yp[4 * r] = y[r];
  }
  lds_barrier();
  if (chunk < 10) {
    const int c0 = (p * (p + 1)) / 2;
    const double* px = W + (16 * p + lq) * LD + 64 + 16 * q + li;
    double yv[4][4], vx[4];
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      const double* yp = ytile(W, c0 + (qq <= p ? qq : 0)) + lq * LD + li;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) yv[qq][kk] = qq <= p ? yp[4 * kk * LD] : 0.0;
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) vx[kk] = px[4 * kk * LD];
    asm volatile("" ::: "memory");
    v4d t = {0, 0, 0, 0};
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      double ys = yv[0][kk];
#pragma unroll
      for (int qq = 1; qq < 4; ++qq) if (qq <= p) ys += yv[qq][kk];
      t = __builtin_amdgcn_mfma_f64_16x16x4f64(ys, vx[kk], t, 0, 0, 0);
    }
    double* tp = TP + chunk * TT + li * TS + lq;
#pragma unroll
    for (int r = 0; r < 4; ++r) tp[4 * r] = t[r];
  }
  lds_barrier();
}

// MODE 0: (z), 1: (t10), 2: (t4), 3: (s)
template <int MODE>
__global__ __launch_bounds__(1024) void tail(const double* Xg, const double* Bg, double* out, long long* cyc, int reps) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* W = lds; double* P = W + kW; double* TP = P + kP; double (*Ts)[68] = reinterpret_cast<double (*)[68]>(TP + kTP); double* YS = TP + kTP + kTs;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, lq = lane >> 4;
  for (int e = tid; e < kW; e += 1024) W[e] = 0.0;
  for (int e = tid; e < kTP + kTs + TT; e += 1024) TP[e] = 0.0;
  __syncthreads();
  for (int e = tid; e < 4096; e += 1024) W[(e >> 6) * LD + 64 + (e & 63)] = Xg[e];   // X(r, c) at W[c * LD + 64 + r]
  P[tid] = Bg[tid];                                                                  // B(row l, variable k) at P[k * 16 + l]
  __syncthreads();
  long long total = 0;
#pragma unroll 1
  for (int r = 0; r < reps; ++r) {
    lds_barrier();
    const long long t0 = clock64();
    if (MODE == 0) {
      if (wave < 10) {
        int xt, yt; tri10(wave, xt, yt);
        const v4d g = xt == 0 ? z_tile<0>(W, yt, li, lq) : (xt == 1 ? z_tile<1>(W, yt, li, lq) : (xt == 2 ? z_tile<2>(W, yt, li, lq) : z_tile<3>(W, yt, li, lq)));
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int x = 16 * xt + li, y = 16 * yt + lq + 4 * k; W[y * LD + x] = g[k]; if (xt != yt) W[x * LD + y] = g[k]; }
      }
      __syncthreads();
      if (wave < 4) {
        const double* px = P + lq * 16 + li; const double* pz = W + lq * LD + 16 * wave + li;
        double vx[16], vz[16];
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) { vx[kk] = px[64 * kk]; vz[kk] = pz[4 * kk * LD]; }
        asm volatile("" ::: "memory");
        v4d tq = {0, 0, 0, 0}, tq2 = {0, 0, 0, 0};
#pragma unroll
        for (int kk = 0; kk < 16; kk += 2) {
          tq = __builtin_amdgcn_mfma_f64_16x16x4f64(vx[kk], vz[kk], tq, 0, 0, 0);
          tq2 = __builtin_amdgcn_mfma_f64_16x16x4f64(vx[kk + 1], vz[kk + 1], tq2, 0, 0, 0);
        }
        tq += tq2;
#pragma unroll
        for (int k = 0; k < 4; ++k) Ts[lq + 4 * k][16 * wave + li] = tq[k];
      }
      __syncthreads();
    } else if (MODE == 1) {
      tx_stage<0>(W, P, TP, wave, li, lq);
    } else if (MODE == 2) {
      tx_stage<6>(W, P, TP, wave, li, lq);
    } else {
      if (wave == 11) {   // panel 2 alone on one wave
        constexpr int pp = 2;
        const double* pb = P + lq * 16 + li; const double* px = W + (16 * pp + li) * LD + 64 + lq;
        double vb[3][4], vx[3][4];
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) { vb[q][kk] = pb[256 * q + 64 * kk]; vx[q][kk] = px[16 * q + 4 * kk]; }
        asm volatile("" ::: "memory");
        v4d y = {0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          v4d yq = {0, 0, 0, 0};
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) yq = __builtin_amdgcn_mfma_f64_16x16x4f64(vb[q][kk], vx[q][kk], yq, 0, 0, 0);
          if (q == 0) y = yq; else y += yq;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) YS[li * TS + lq + 4 * k] = y[k];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const double* px2 = W + (16 * pp + lq) * LD + 64 + li;
        double vy[4], vx2[3][4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) vy[kk] = YS[(4 * kk + lq) * TS + li];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) vx2[i][kk] = px2[4 * kk * LD + 16 * i];
        asm volatile("" ::: "memory");
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          v4d t = {0, 0, 0, 0};
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) t = __builtin_amdgcn_mfma_f64_16x16x4f64(vy[kk], vx2[i][kk], t, 0, 0, 0);
          double* tp = TP + (3 + i) * TT + li * TS + lq;
#pragma unroll
          for (int k = 0; k < 4; ++k) tp[4 * k] = t[k];
        }
      }
      lds_barrier();
    }
    total += clock64() - t0;
    if (MODE == 0) {   // Z overwrote rows 0..63 only: X is intact
      __syncthreads();
    }
  }
  if (tid == 0) cyc[0] = total / reps;
  if (MODE == 1) {   // T_x(row, col) = sum over the panels p >= col / 16 of TP(p, col / 16)
    const int row = tid & 15, col = tid >> 4, i = col >> 4;
    double v = 0.0;
    for (int p = i; p < 4; ++p) v += TP[((p * (p + 1)) / 2 + i) * TT + (col & 15) * TS + row];
    out[row * 64 + col] = v;
  }
}

int main() {
  std::vector<double> X(4096, 0.0), B(1024), T(1024, 0.0), got(1024);
  unsigned s = 12345u; auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / (1 << 24) - 0.5; };
  for (int c = 0; c < 64; ++c) for (int r = 0; r <= c; ++r) X[c * 64 + r] = r == c ? 1.0 + 0.1 * rnd() : 0.2 * rnd();   // X(r, c), upper triangular
  for (int k = 0; k < 64; ++k) for (int l = 0; l < 16; ++l) B[k * 16 + l] = rnd();
  for (int l = 0; l < 16; ++l) for (int c = 0; c < 64; ++c) { double v = 0; for (int j = 0; j < 64; ++j) { double y = 0; for (int k = 0; k < 64; ++k) y += B[k * 16 + l] * X[j * 64 + k]; v += y * X[j * 64 + c]; } T[l * 64 + c] = v; }
  double *dX, *dB, *dout; long long* dc;
  (void)hipMalloc(&dX, 4096 * 8); (void)hipMalloc(&dB, 1024 * 8); (void)hipMalloc(&dout, 1024 * 8); (void)hipMalloc(&dc, 8);
  (void)hipMemcpy(dX, X.data(), 4096 * 8, hipMemcpyHostToDevice); (void)hipMemcpy(dB, B.data(), 1024 * 8, hipMemcpyHostToDevice);
  const size_t lds = kLds * sizeof(double);
  (void)hipFuncSetAttribute((const void*)tail<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  (void)hipFuncSetAttribute((const void*)tail<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  (void)hipFuncSetAttribute((const void*)tail<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  (void)hipFuncSetAttribute((const void*)tail<3>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  printf("cycles per tail between workgroup barriers (wave 0's clock64), one workgroup of 16 waves; every line is run three times\n");
  long long c;
  for (int rep = 0; rep < 3; ++rep) {
    hipLaunchKernelGGL(tail<0>, dim3(1), dim3(1024), lds, 0, dX, dB, dout, dc, 100); (void)hipDeviceSynchronize(); (void)hipMemcpy(&c, dc, 8, hipMemcpyDeviceToHost);
    printf("(z)   Z = X X^T (80 MFMAs on ten waves), barrier, T_x = B_x Z (4 x 16 MFMAs), barrier   %6lld\n", c);
    hipLaunchKernelGGL(tail<1>, dim3(1), dim3(1024), lds, 0, dX, dB, dout, dc, 100); (void)hipDeviceSynchronize(); (void)hipMemcpy(&c, dc, 8, hipMemcpyDeviceToHost);
    printf("(t10) ten Y chunks, barrier, ten T chunks, barrier (4 MFMAs per chunk)                  %6lld\n", c);
    hipLaunchKernelGGL(tail<2>, dim3(1), dim3(1024), lds, 0, dX, dB, dout, dc, 100); (void)hipDeviceSynchronize(); (void)hipMemcpy(&c, dc, 8, hipMemcpyDeviceToHost);
    printf("(t4)  panel 3's four Y chunks, barrier, its four T chunks, barrier                      %6lld\n", c);
    hipLaunchKernelGGL(tail<3>, dim3(1), dim3(1024), lds, 0, dX, dB, dout, dc, 100); (void)hipDeviceSynchronize(); (void)hipMemcpy(&c, dc, 8, hipMemcpyDeviceToHost);
    printf("(s)   panel 2's six chunks on one wave (24 MFMAs, Y_2 through LDS), barrier             %6lld\n", c);
  }
  hipLaunchKernelGGL(tail<1>, dim3(1), dim3(1024), lds, 0, dX, dB, dout, dc, 1); (void)hipDeviceSynchronize();
  (void)hipMemcpy(got.data(), dout, 1024 * 8, hipMemcpyDeviceToHost);
  double err = 0, mx = 0;
  for (int e = 0; e < 1024; ++e) { err = fmax(err, fabs(got[e] - T[e])); mx = fmax(mx, fabs(T[e])); }
  printf("(t10) against the host's (B X) X^T: max error %.3e of %.3e: %s\n", err, mx, err <= 1e-13 * mx ? "ok" : "WRONG");
  return hipGetLastError() == hipSuccess && err <= 1e-13 * mx ? 0 : 1;
}
