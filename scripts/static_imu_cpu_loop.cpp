// Reference-shaped CPU timing loops for scripts/time_static_imu.py, one core, written from the reference's algorithm:
//   detector: StaticIntervalsDetector for th_mult = 1..10 (src/utils/imu_data_interval.cc:111-149 called from
//             static_imu_calibrator.cc:97): every threshold recomputes the 101-sample window variance at every sample;
//   gyro:     one evaluation of every MultiPosGyroResidual block (static_imu_calibrator.h:60-140) with 9-component dual
//             numbers, as ceres::AutoDiffCostFunction<..., 3, 9> does: per-step-normalised RK4 (gyro_integration.h).
// usage: static_imu_cpu_loop detector acc.f64 n norm_th
//        static_imu_cpu_loop gyro t.f64 gyro.f64 n ranges.i32 num_blocks
// prints: seconds and a checksum
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct J9 { double a, v[9]; };
static J9 mk(double a) { J9 r; r.a = a; for (double& x : r.v) x = 0; return r; }
static J9 operator+(const J9& x, const J9& y) { J9 r; r.a = x.a + y.a; for (int i = 0; i < 9; ++i) r.v[i] = x.v[i] + y.v[i]; return r; }
static J9 operator-(const J9& x, const J9& y) { J9 r; r.a = x.a - y.a; for (int i = 0; i < 9; ++i) r.v[i] = x.v[i] - y.v[i]; return r; }
static J9 operator*(const J9& x, const J9& y) { J9 r; r.a = x.a * y.a; for (int i = 0; i < 9; ++i) r.v[i] = x.a * y.v[i] + x.v[i] * y.a; return r; }
static J9 operator*(double s, const J9& y) { J9 r; r.a = s * y.a; for (int i = 0; i < 9; ++i) r.v[i] = s * y.v[i]; return r; }
static J9 jsqrt(const J9& x) { J9 r; r.a = std::sqrt(x.a); for (int i = 0; i < 9; ++i) r.v[i] = x.v[i] / (2 * r.a); return r; }
static J9 jdiv(const J9& x, const J9& y) { J9 r; r.a = x.a / y.a; for (int i = 0; i < 9; ++i) r.v[i] = (x.v[i] - r.a * y.v[i]) / y.a; return r; }

static void hs(const J9 w[3], const J9 q[4], J9 k[4]) {
  k[0] = 0.5 * (mk(0) - w[0] * q[1] - w[1] * q[2] - w[2] * q[3]); k[1] = 0.5 * (w[0] * q[0] + w[2] * q[2] - w[1] * q[3]);
  k[2] = 0.5 * (w[1] * q[0] - w[2] * q[1] + w[0] * q[3]); k[3] = 0.5 * (w[2] * q[0] + w[1] * q[1] - w[0] * q[2]);
}

template <class T> static bool rd(const char* p, std::vector<T>& v) { FILE* f = std::fopen(p, "rb"); if (!f) return false; const bool ok = std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); std::fclose(f); return ok; }

int main(int argc, char** argv) {
  if (argc >= 5 && !std::strcmp(argv[1], "detector")) {
    const long n = std::atol(argv[3]); const double norm_th = std::atof(argv[4]);
    std::vector<double> a(static_cast<size_t>(3 * n)); if (!rd(argv[2], a)) return 1;
    const auto t0 = std::chrono::steady_clock::now();
    long total = 0;
    for (int th_mult = 1; th_mult <= 10; ++th_mult) {
      const double th = th_mult * norm_th; bool look = true; long cnt = 0;
      for (long i = 50; i < n - 50; ++i) {
        double m[3] = {0, 0, 0}, v[3] = {0, 0, 0};
        for (long j = i - 50; j <= i + 50; ++j) for (int c = 0; c < 3; ++c) m[c] += a[size_t(3 * j + c)];
        for (int c = 0; c < 3; ++c) m[c] /= 101.0;
        for (long j = i - 50; j <= i + 50; ++j) for (int c = 0; c < 3; ++c) { const double d = a[size_t(3 * j + c)] - m[c]; v[c] += d * d; }
        for (int c = 0; c < 3; ++c) v[c] /= 100.0;
        const double nrm = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        if (look) { if (nrm < th) look = false; } else if (nrm >= th) { look = true; ++cnt; }
      }
      total += cnt + (look ? 0 : 1);
    }
    std::printf("%.6f %ld\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), total);
    return 0;
  }
  if (argc >= 7 && !std::strcmp(argv[1], "gyro")) {
    const long n = std::atol(argv[4]); const int nb = std::atoi(argv[6]);
    std::vector<double> t(static_cast<size_t>(n)), g(static_cast<size_t>(3 * n)); std::vector<int> rg(static_cast<size_t>(2 * nb));
    if (!rd(argv[2], t) || !rd(argv[3], g) || !rd(argv[5], rg)) return 1;
    const double p0[9] = {1e-3, -2e-3, 5e-4, 1e-3, -1e-3, 2e-3, 0.99, 1.01, 1.005};
    const auto t0 = std::chrono::steady_clock::now();
    J9 th[9];
    for (int k = 0; k < 9; ++k) { th[k] = mk(p0[k]); th[k].v[k] = 1.0; }
    const J9 one = mk(1.0);
    const J9 T[3][3] = {{one, mk(0) - th[0], th[1]}, {th[3], one, mk(0) - th[2]}, {mk(0) - th[4], th[5], one}};
    J9 ms[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) ms[i][j] = T[i][j] * th[6 + j];
    double sum = 0;
    for (int b = 0; b < nb; ++b) {
      std::vector<J9> w; w.reserve(size_t(rg[size_t(2 * b + 1)] - rg[size_t(2 * b)] + 1));
      for (int s = rg[size_t(2 * b)]; s <= rg[size_t(2 * b + 1)]; ++s) {   // UnbiasNormalize of every sample, as the residual copies them
        for (int i = 0; i < 3; ++i) w.push_back(ms[i][0] * mk(g[size_t(3 * s)]) + ms[i][1] * mk(g[size_t(3 * s + 1)]) + ms[i][2] * mk(g[size_t(3 * s + 2)]));
      }
      J9 q[4] = {one, mk(0), mk(0), mk(0)};
      const int m = int(w.size() / 3);
      for (int k = 0; k + 1 < m; ++k) {
        const double dt = t[size_t(rg[size_t(2 * b)] + k + 1)] - t[size_t(rg[size_t(2 * b)] + k)];
        const J9* w0 = &w[size_t(3 * k)]; const J9* w1 = &w[size_t(3 * k + 3)];
        J9 w01[3], k1[4], k2[4], k3[4], k4[4], tq[4];
        for (int i = 0; i < 3; ++i) w01[i] = 0.5 * (w0[i] + w1[i]);
        hs(w0, q, k1); for (int i = 0; i < 4; ++i) tq[i] = q[i] + (0.5 * dt) * k1[i];
        hs(w01, tq, k2); for (int i = 0; i < 4; ++i) tq[i] = q[i] + (0.5 * dt) * k2[i];
        hs(w01, tq, k3); for (int i = 0; i < 4; ++i) tq[i] = q[i] + dt * k3[i];
        hs(w1, tq, k4);
        for (int i = 0; i < 4; ++i) q[i] = q[i] + dt * ((1.0 / 6) * k1[i] + (1.0 / 3) * k2[i] + (1.0 / 3) * k3[i] + (1.0 / 6) * k4[i]);
        const J9 nq = jsqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        for (int i = 0; i < 4; ++i) q[i] = jdiv(q[i], nq);
      }
      sum += q[0].a + q[1].v[3];
    }
    std::printf("%.6f %.17g\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), sum);
    return 0;
  }
  std::fprintf(stderr, "usage: %s detector acc.f64 n norm_th | gyro t.f64 gyro.f64 n ranges.i32 num_blocks\n", argv[0]);
  return 2;
}
