// Reference-shaped CPU timing loop for scripts/time_allan.py: AllanGyr::calcThetas + calcVariance of the reference
// (src/allanvariance/allan_gyr.cc:104-139), one pass, one core, on samples read from a raw float64 file.
// usage: allan_cpu_loop samples.f64 n freq period factors.i32 num_factors
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 7) { std::fprintf(stderr, "usage: %s samples.f64 n freq period factors.i32 num_factors\n", argv[0]); return 2; }
  const long n = std::atol(argv[2]); const double freq = std::atof(argv[3]), period = std::atof(argv[4]); const int nf = std::atoi(argv[6]);
  std::vector<double> w(size_t(n), 0.0); std::vector<int> fac(size_t(nf), 0);
  FILE* f = std::fopen(argv[1], "rb"); if (!f || std::fread(w.data(), 8, size_t(n), f) != size_t(n)) return 1; std::fclose(f);
  f = std::fopen(argv[5], "rb"); if (!f || std::fread(fac.data(), 4, size_t(nf), f) != size_t(nf)) return 1; std::fclose(f);
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<double> th; th.reserve(size_t(n));
  double sum = 0;
  for (long i = 0; i < n; ++i) { sum += w[size_t(i)]; th.push_back(sum / freq); }
  std::vector<double> s2(size_t(nf), 0.0);
  for (int i = 0; i < nf; ++i) {
    const long m = fac[size_t(i)];
    const double cp2 = (period * m) * (period * m), divided = 2 * cp2 * (n - 2 * m);
    const long mx = n - 2 * m;
    for (long k = 0; k < mx; ++k) { const double t = th[size_t(k + 2 * m)] - 2 * th[size_t(k + m)] + th[size_t(k)]; s2[size_t(i)] += t * t; }
    s2[size_t(i)] = s2[size_t(i)] / divided;
  }
  const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::printf("%.6f %.17g\n", s, s2[0]);
  return 0;
}
