// micro-benchmark: what the multiplier broadcasts of the 16-column panel chain (kernels_bcr.hip, bcri_invert_body) cost the wave in
// ISSUE time -- v_readlane_b32 pairs into an SGPR pair against LDS broadcast reads of a strip the wave wrote itself.
// One wave per SIMD (one workgroup of four waves, every wave on a strip of its own), clock64 around straight-line code.
//   (a) the 120 deferred updates of a panel as the compiler emits them today: 2 v_readlane_b32 + v_fma_f64 on the SGPR pair
//   (b1) the same 120 updates with every multiplier from LDS: per column one ds_write_b64 of lanes 0..15, then broadcast reads
//        (ds_read_b128 for an aligned pair of multipliers, ds_read_b64 for a single one), then the v_fma_f64
//   (b2) as (b1), but the update of column c + 1 -- the hop the next pivot waits for -- stays on v_readlane
//   (c) cycles per instruction, 64 of a kind back to back: v_readlane_b32, v_cndmask_b32, v_fma_f64, broadcast ds_read_b128
//   (d) the dependent hop: write -> broadcast read -> fma inside one wave, against v_readlane -> fma
//   (e) a WHOLE 16-column panel with the real column body between the updates -- v_readlane pivot, v_rsq_f64, the two Goldschmidt
//       steps, the strip store, the v_readlane of l(c + 1) and the next column's v_fma -- since (a)-(b2) price the updates alone, with
//       no dependent sequence to hide in: the plain column loop (three rotating strips, a column's updates where the compiler puts
//       them), and csrc/bcr_chain_body.h -- the body the kernels run -- under candidate tables of csrc/bcr_chain_schedule.h: column
//       c - 1's updates between the steps of column c, and balanced tables (7 or 8 updates per column) with different gap weights
// hipcc -O3 -std=c++17 --offload-arch=gfx950 scripts/micro/chain_issue.hip -o chain_issue && ./chain_issue
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include "../../openimucameracalibrator_amd/csrc/bcr_chain_body.h"
typedef double d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double rl(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
// the stores of this wave's lanes are visible to the loads of its other lanes behind this (LDS operations of a wave execute in
// issue order): an ordering for the compiler, no instruction
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// MODE 0: (a), 1: (b1), 2: (b2)
template <int MODE>
__global__ __launch_bounds__(256) void updates(const double* in, double* out, long long* cyc, int reps) {
  __shared__ __attribute__((aligned(16))) double strips[4][3][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double av[16];
  for (int c = 0; c < 16; ++c) av[c] = in[lane * 16 + c];
  double accum = 0.0;
  const long long t0 = clock64();
#pragma unroll 1
  for (int r = 0; r < reps; ++r) {
    double a[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) a[c] = av[c] + accum * 1e-300;
#pragma unroll
    for (int c = 0; c < 15; ++c) {
      const double l = a[c];
      if (MODE == 0) {
#pragma unroll
        for (int c2 = c + 1; c2 < 16; ++c2) a[c2] = fma(-l, rl(l, c2), a[c2]);
      } else {
        double* strip = strips[wave][c % 3];
        if (lane < 16) strip[lane] = l;
        wave_sync();
        int first = c + 1;
        if (MODE == 2) { a[c + 1] = fma(-l, rl(l, c + 1), a[c + 1]); first = c + 2; }
        double m[16];
#pragma unroll
        for (int c2 = first; c2 < 16; ++c2) {   // (an odd c2 behind `first` came with the pair before it)
          if ((c2 & 1) == 0) { const d2 v = *reinterpret_cast<const d2*>(strip + c2); m[c2] = v[0]; m[c2 + 1] = v[1]; }
          else if (c2 == first) m[c2] = strip[c2];
        }
#pragma unroll
        for (int c2 = first; c2 < 16; ++c2) a[c2] = fma(-l, m[c2], a[c2]);
      }
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) accum += a[c];
  }
  const long long t1 = clock64();
  out[threadIdx.x] = accum;
  if (lane == 0) cyc[wave] = (t1 - t0) / reps;
}

// (c): KIND 0 v_readlane_b32, 1 v_cndmask_b32, 2 v_fma_f64, 3 ds_read_b128 (every lane the same address), 4 the empty loop
#define REP4(s) s s s s
#define REP16(s) REP4(s) REP4(s) REP4(s) REP4(s)
#define REP64(s) REP16(s) REP16(s) REP16(s) REP16(s)
template <int KIND>
__global__ __launch_bounds__(256) void per_instruction(const double* in, double* out, long long* cyc, int reps) {
  __shared__ __attribute__((aligned(16))) double strips[4][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane < 16) strips[wave][lane] = in[lane];
  __syncthreads();
  double x = in[lane], y = in[lane + 64], z = in[lane + 128], w = 0.0;
  int xi = __double2loint(x), yi = __double2loint(y), wi = 0;
  const unsigned lds_addr = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const double*)(&strips[wave][2]);   // (LDS byte address)
  d2 q = {0.0, 0.0};
  const long long t0 = clock64();
#pragma unroll 1
  for (int r = 0; r < reps; ++r) {
    if (KIND == 0) asm volatile(REP64("v_readlane_b32 s20, %0, 3\n\t") :: "v"(xi) : "s20");
    if (KIND == 1) asm volatile("s_nop 4\n\t" REP64("v_cndmask_b32 %0, %1, %2, vcc\n\t") : "=&v"(wi) : "v"(xi), "v"(yi) : "vcc");
    if (KIND == 2) asm volatile(REP64("v_fma_f64 %0, %1, %2, %3\n\t") : "=&v"(w) : "v"(x), "v"(y), "v"(z));
    if (KIND == 3) asm volatile(REP64("ds_read_b128 %0, %1\n\t") "s_waitcnt lgkmcnt(0)\n\t" : "=&v"(q) : "v"(lds_addr) : "memory");
    if (KIND == 4) asm volatile("" ::: "memory");
  }
  const long long t1 = clock64();
  out[threadIdx.x] = w + wi + q[0] + q[1];
  if (lane == 0) cyc[wave] = t1 - t0;
}

// (d): HOP 0 v_readlane -> fma, 1 ds_write_b64 -> broadcast ds_read_b64 -> fma, 64 dependent hops
template <int HOP>
__global__ __launch_bounds__(256) void hop(const double* in, double* out, long long* cyc, int reps) {
  __shared__ __attribute__((aligned(16))) double strips[4][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double x = in[lane];
  const double k = in[64 + lane] * 1e-3;
  const long long t0 = clock64();
#pragma unroll 1
  for (int r = 0; r < reps; ++r) {
#pragma unroll
    for (int h = 0; h < 64; ++h) {
      double m;
      if (HOP == 0) m = rl(x, 3);
      else { if (lane < 16) strips[wave][lane] = x; wave_sync(); m = strips[wave][3]; wave_sync(); }
      x = fma(m, k, x);
    }
  }
  const long long t1 = clock64();
  out[threadIdx.x] = x;
  if (lane == 0) cyc[wave] = (t1 - t0) / reps;
}

// (e): V < 0 the plain column loop; V >= 0 bcr_chain_panel under table V of this list
struct TableSpec { int w[8]; int hop_clear; bool previous_column_only; };
constexpr int kTables = 16;
constexpr TableSpec kSpec[kTables] = {
  {{0, 3, 3, 3, 3, 2, 0, 0}, 0, true},    // column c - 1's updates between the steps of column c
  {{1, 2, 1, 1, 1, 1, 0, 1}, 2, false},   // balanced from here on: 7 or 8 updates per column
  {{0, 2, 2, 1, 1, 1, 0, 1}, 2, false},
  {{0, 4, 0, 2, 0, 2, 0, 0}, 2, false},
  {{1, 1, 1, 1, 1, 1, 1, 1}, 2, false},
  {{1, 2, 1, 1, 1, 1, 0, 1}, 4, false},
  {{1, 1, 1, 1, 1, 1, 0, 2}, 2, false},
  {{2, 1, 1, 1, 1, 0, 0, 2}, 2, false},
  {{2, 1, 1, 1, 1, 0, 0, 2}, 4, false},   // csrc's kChainSchedule
  {{2, 2, 1, 1, 0, 0, 0, 2}, 2, false},
  {{3, 1, 1, 1, 0, 0, 0, 2}, 2, false},
  {{2, 1, 1, 1, 0, 0, 0, 3}, 3, false},
  {{3, 1, 1, 0, 0, 0, 0, 3}, 3, false},
  {{3, 2, 0, 0, 0, 0, 0, 3}, 3, false},
  {{4, 1, 0, 0, 0, 0, 0, 3}, 3, false},
  {{3, 1, 1, 1, 1, 0, 0, 1}, 2, false},
};
template <int V> struct TableOf {
  static constexpr oicc::BcrChainSchedule S = oicc::bcr_chain_schedule(kSpec[V].w, kSpec[V].hop_clear, kSpec[V].previous_column_only);
  static_assert(S.ok, "every update has a gap");
};

// (one wave per SIMD is all the inverting kernels have, 1024 threads: without the attribute the compiler trades the plain loop's load
// clumps for registers it has no use for -- a ds_read_b128 and a full wait per pair of updates, 5.2 k cycles per panel)
template <int V>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void panel(const double* in, double* out, long long* cyc, int reps) {
  __shared__ __attribute__((aligned(16))) double strips[4][oicc::kChainStripDoubles];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double a0[16];
  for (int c = 0; c < 16; ++c) a0[c] = (lane < 16 && c > lane) ? 0.0 : in[lane * 16 + c];   // lanes 0..15: the diagonal tile's rows, zeros above
  double accum = 0.0;
  const long long t0 = clock64();
#pragma unroll 1
  for (int r = 0; r < reps; ++r) {
    double av[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) av[c] = a0[c] + accum * 1e-300;
    bool bad = false;
    if constexpr (V < 0) {
      double* const strip_w = strips[wave] + (lane < 16 ? lane : 32 + lane);
      const double* const strip_r = strips[wave];
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        const double piv = rl(av[c], c);
        if (c == 15) bad = !(piv > 0.0);
        const double y0 = __builtin_amdgcn_rsq(piv);
        const double g0 = piv * y0, h0 = 0.5 * y0;
        const double r0 = fma(-g0, h0, 0.5);
        const double g1 = fma(g0, r0, g0), h1 = fma(h0, r0, h0);
        const double r1 = fma(-g1, h1, 0.5);
        const double u = (av[c] + av[c]) * h1;
        const double l = fma(u, r1, u);
        av[c] = l;
        if (c < 14) { strip_w[(c % 3) * 16] = l; wave_sync(); }
        if (c < 15) av[c + 1] = fma(-l, rl(l, c + 1), av[c + 1]);
        if (c < 14) {
          double m[16];
#pragma unroll
          for (int c2 = c + 2; c2 < 16; ++c2) {
            if ((c2 & 1) == 0) { const d2 v = *reinterpret_cast<const d2*>(strip_r + (c % 3) * 16 + c2); m[c2] = v[0]; m[c2 + 1] = v[1]; }
            else if (c2 == c + 2) m[c2] = strip_r[(c % 3) * 16 + c2];
          }
#pragma unroll
          for (int c2 = c + 2; c2 < 16; ++c2) av[c2] = fma(-l, m[c2], av[c2]);
        }
      }
    } else {
      bad = oicc::bcr_chain_panel<TableOf<V < 0 ? 0 : V>::S>(av, strips[wave] + lane, strips[wave]);
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) accum += av[c];
    if (bad) accum += 1.0;
  }
  const long long t1 = clock64();
  out[threadIdx.x] = accum;
  if (lane == 0) cyc[wave] = (t1 - t0) / reps;
}

template <class F, int... Vs> void for_tables(F f, std::integer_sequence<int, Vs...>) { (f(std::integral_constant<int, Vs>()), ...); }

int main() {
  double h[64 * 16];
  for (int r = 0; r < 64; ++r) for (int c = 0; c < 16; ++c) h[r * 16 + c] = (r == c ? 10.0 : 0.0) + 0.3 / (1 + abs(r - c));
  double *din, *dout; long long* dc; (void)hipMalloc(&din, sizeof(h)); (void)hipMalloc(&dout, 256 * 8); (void)hipMalloc(&dc, 4 * 8);
  (void)hipMemcpy(din, h, sizeof(h), hipMemcpyHostToDevice);
  long long c[4];
  auto show = [&](const char* name, const char* unit, double div) {
    (void)hipDeviceSynchronize(); (void)hipMemcpy(c, dc, sizeof(c), hipMemcpyDeviceToHost);
    printf("%-86s %8.1f %8.1f %8.1f %8.1f %s\n", name, c[0] / div, c[1] / div, c[2] / div, c[3] / div, unit);
  };
  printf("cycles of the four waves of one workgroup (one per SIMD); every line is run three times\n");
  for (int rep = 0; rep < 3; ++rep) {
    hipLaunchKernelGGL(updates<0>, dim3(1), dim3(256), 0, 0, din, dout, dc, 200); show("(a)  120 x {2 v_readlane_b32, v_fma_f64}", "cycles per panel", 1.0);
    hipLaunchKernelGGL(updates<1>, dim3(1), dim3(256), 0, 0, din, dout, dc, 200); show("(b1) 120 x {LDS broadcast, v_fma_f64}, 15 ds_write_b64", "cycles per panel", 1.0);
    hipLaunchKernelGGL(updates<2>, dim3(1), dim3(256), 0, 0, din, dout, dc, 200); show("(b2) 15 x v_readlane pair + 105 x LDS broadcast, 15 ds_write_b64", "cycles per panel", 1.0);
  }
  const int R = 100;
  for (int rep = 0; rep < 3; ++rep) {
    long long base[4];
    hipLaunchKernelGGL(per_instruction<4>, dim3(1), dim3(256), 0, 0, din, dout, dc, R); (void)hipDeviceSynchronize(); (void)hipMemcpy(base, dc, sizeof(base), hipMemcpyDeviceToHost);
    auto showc = [&](const char* name) {
      (void)hipDeviceSynchronize(); (void)hipMemcpy(c, dc, sizeof(c), hipMemcpyDeviceToHost);
      printf("%-62s %8.2f %8.2f %8.2f %8.2f cycles per instruction\n", name, (c[0] - base[0]) / (64.0 * R), (c[1] - base[1]) / (64.0 * R), (c[2] - base[2]) / (64.0 * R), (c[3] - base[3]) / (64.0 * R));
    };
    hipLaunchKernelGGL(per_instruction<0>, dim3(1), dim3(256), 0, 0, din, dout, dc, R); showc("(c)  v_readlane_b32 back to back");
    hipLaunchKernelGGL(per_instruction<1>, dim3(1), dim3(256), 0, 0, din, dout, dc, R); showc("(c)  v_cndmask_b32 back to back");
    hipLaunchKernelGGL(per_instruction<2>, dim3(1), dim3(256), 0, 0, din, dout, dc, R); showc("(c)  v_fma_f64 back to back (independent)");
    hipLaunchKernelGGL(per_instruction<3>, dim3(1), dim3(256), 0, 0, din, dout, dc, R); showc("(c)  ds_read_b128 broadcast back to back, one wait per 64");
  }
  for (int rep = 0; rep < 3; ++rep) {
    hipLaunchKernelGGL(hop<0>, dim3(1), dim3(256), 0, 0, din, dout, dc, 50); show("(d)  v_readlane pair -> v_fma_f64, dependent", "cycles per hop", 64.0);
    hipLaunchKernelGGL(hop<1>, dim3(1), dim3(256), 0, 0, din, dout, dc, 50); show("(d)  ds_write_b64 -> broadcast ds_read_b64 -> v_fma_f64", "cycles per hop", 64.0);
  }
  // (e) every table must give the plain loop's bits: the sums of one panel
  double ref[256], got[256];
  hipLaunchKernelGGL(panel<-1>, dim3(1), dim3(256), 0, 0, din, dout, dc, 1); (void)hipDeviceSynchronize(); (void)hipMemcpy(ref, dout, sizeof(ref), hipMemcpyDeviceToHost);
  int same = 1;
  for_tables([&](auto v) {
    constexpr int V = decltype(v)::value;
    hipLaunchKernelGGL(panel<V>, dim3(1), dim3(256), 0, 0, din, dout, dc, 1); (void)hipDeviceSynchronize(); (void)hipMemcpy(got, dout, sizeof(got), hipMemcpyDeviceToHost);
    for (int t = 0; t < 256; ++t) if (memcmp(&ref[t], &got[t], 8) != 0) { same = 0; printf("(e) table %d differs from the plain loop at thread %d: %.17g %.17g\n", V, t, ref[t], got[t]); break; }
  }, std::make_integer_sequence<int, kTables>());
  printf("(e) bits of all %d tables equal the plain loop's: %s\n", kTables, same ? "yes" : "NO");
  for (int rep = 0; rep < 3; ++rep) {
    hipLaunchKernelGGL(panel<-1>, dim3(1), dim3(256), 0, 0, din, dout, dc, 200); show("(e)  plain column loop (three strips, a column's updates where the compiler puts them)", "cycles per panel", 1.0);
    for_tables([&](auto v) {
      constexpr int V = decltype(v)::value;
      char name[96];
      const int* w = kSpec[V].w;
      snprintf(name, sizeof(name), "(e)  %s, gaps %d %d %d %d %d %d %d %d, hop clear %d", kSpec[V].previous_column_only ? "column c - 1's in column c" : "balanced",
               w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], kSpec[V].hop_clear);
      hipLaunchKernelGGL(panel<V>, dim3(1), dim3(256), 0, 0, din, dout, dc, 200); show(name, "cycles per panel", 1.0);
    }, std::make_integer_sequence<int, kTables>());
  }
  return hipGetLastError() == hipSuccess && same ? 0 : 1;
}
