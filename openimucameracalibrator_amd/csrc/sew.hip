// Spline error weighting pre-stage on the device: the knot spacings and IMU
// weights the spline solve consumes.  Follows python/sew.py of the reference:
//   make_reference_spectrum :170-179, spline_interpolation_response / bspline_interp_freq_func
//   :35-76, signal_energy :79-80, find_uniform_knot_spacing_spectrum :141-159,
//   find_max_quality_dt :83-137 (end-point test, halving back-off, scipy.optimize.brentq [EXT]),
//   dt_to_variance_spectrum :192-195, knot_spacing_and_variance :199-235.
// The real-to-complex FFT is hipFFT's (a plain library transform); the spectrum power and the
// per-trial-dt spectral reduction are HIP kernels; the scalar search runs on the host.
#include <hip/hip_runtime.h>
#include <hipfft/hipfft.h>
#include <cmath>
#include <cstdint>
#include <mutex>
#include <vector>
#include "../../include/oicc_hip.h"
#include "hip_resources.h"

namespace {

// power spectrum of the half spectrum with the multiplicity of the mirrored bins:
//   pw[k] = w_k * (1/dims) * sum_axes |S_axis[k]|^2,  k = 0..n/2,  pw[0] = 0 (DC removed)
__global__ void sew_power_kernel(const hipfftDoubleComplex* spec, int dims, int64_t n, int64_t nh, double* pw) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nh) return;
  double s = 0.0;
  for (int a = 0; a < dims; ++a) { const hipfftDoubleComplex z = spec[(int64_t)a * nh + k]; s = fma(z.x, z.x, fma(z.y, z.y, s)); }
  const bool self_mirrored = (k == 0) || (2 * k == n);   // DC and, for even n, the Nyquist bin appear once in the full spectrum
  pw[k] = k == 0 ? 0.0 : (self_mirrored ? 1.0 : 2.0) * s / dims;
}

// out[0] += sum_k pw[k]                      (energy of the reference spectrum * n)
// out[1] += sum_k pw[k] * (1 - H(f_k, dt))^2 (energy removed by a spline of knot spacing dt * n)
__global__ void sew_reduce_kernel(const double* pw, int64_t nh, double bin_hz, double dt, double* out) {
  __shared__ double sm[2][256];
  double e = 0.0, r = 0.0;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nh; k += (int64_t)gridDim.x * blockDim.x) {
    const double p = pw[k];
    const double x = double(k) * bin_hz * dt;                 // f dt
    double sinc = 1.0;
    if (x != 0.0) { const double px = M_PI * x; sinc = sin(px) / px; }
    const double s2 = sinc * sinc;
    const double H = 3.0 * s2 * s2 / (2.0 + cos(2.0 * M_PI * x));
    const double d = 1.0 - H;
    e += p; r = fma(p, d * d, r);
  }
  sm[0][threadIdx.x] = e; sm[1][threadIdx.x] = r;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) { if ((int)threadIdx.x < s) { sm[0][threadIdx.x] += sm[0][threadIdx.x + s]; sm[1][threadIdx.x] += sm[1][threadIdx.x + s]; } __syncthreads(); }
  if (threadIdx.x == 0) { unsafeAtomicAdd(out, sm[0][0]); unsafeAtomicAdd(out + 1, sm[1][0]); }
}

constexpr int kSewGridCap = 1024;   // workgroups of the spectral reduction; longer spectra go round its grid-stride loop

// The spectrum of one series on the device: buffers, stream and hipFFT plan for a (device, dims, n), the transform
// (upload -> hipfftExecD2Z -> power kernel) and the two spectral sums for a trial knot spacing.  The calibration entry and the
// debug entry below both drive this one object.
// Buffers and plan are kept for the next call with the same (device, dims, n): get_sew_for_dataset.py calls the entry twice
// per data set (accelerometer, gyroscope) and plan creation costs milliseconds.
struct SewSpectrum {
  int device = -1, dims = 0; int64_t n = 0, nh = 0;
  oicc::DevBuf<double> d_sig; oicc::DevBuf<hipfftDoubleComplex> d_spec; oicc::DevBuf<double> pw, acc;
  oicc::Stream st; hipfftHandle plan = 0; bool have_plan = false;
  double bin_hz = 0.0; int evals = 0; int grid_cap = kSewGridCap;   // of the series loaded last
  // the object outlives its resources (g_sew below): the plan first, then the stream, drained, then the buffers its work used
  void release() {
    if (have_plan) (void)hipfftDestroy(plan);
    have_plan = false; device = -1;
    st.reset();
    d_sig.release(); d_spec.release(); pw.release(); acc.release();
  }
  // buffers and plan for (device, dims, n): kept when they fit, rebuilt when they do not
  int bind(int device_ordinal, int dims_, int64_t n_) {
    if (device == device_ordinal && dims == dims_ && n == n_) return OICC_OK;
    release();
    const int64_t nh_ = n_ / 2 + 1;
    if (!st.create() || !d_sig.resize(size_t(dims_ * n_)) || !d_spec.resize(size_t(dims_ * nh_)) || !pw.resize(size_t(nh_)) || !acc.resize(2)) { release(); return OICC_ERR_HIP; }
    int len = int(n_);
    if (hipfftPlanMany(&plan, 1, &len, nullptr, 1, len, nullptr, 1, int(nh_), HIPFFT_D2Z, dims_) != HIPFFT_SUCCESS) { release(); return OICC_ERR_HIP; }
    have_plan = true;
    if (hipfftSetStream(plan, st) != HIPFFT_SUCCESS) { release(); return OICC_ERR_HIP; }
    device = device_ordinal; dims = dims_; n = n_; nh = nh_;
    return OICC_OK;
  }
  // signal [dims, n] (host) -> pw[0 .. n/2] on the device
  int transform(const double* signal, double sample_rate, int cap) {
    bin_hz = sample_rate / double(n); evals = 0; grid_cap = cap;
    if (hipMemcpyAsync(d_sig.p, signal, sizeof(double) * dims * n, hipMemcpyHostToDevice, st) != hipSuccess) { release(); return OICC_ERR_HIP; }
    if (hipfftExecD2Z(plan, d_sig.p, d_spec.p) != HIPFFT_SUCCESS) { release(); return OICC_ERR_HIP; }
    hipLaunchKernelGGL(sew_power_kernel, dim3(int((nh + 255) / 256)), dim3(256), 0, st, d_spec.p, dims, n, nh, pw.p);
    return OICC_OK;
  }
  // h[0] = sum_k pw[k], h[1] = sum_k pw[k] (1 - H(f_k, dt))^2
  bool sums(double dt, double h[2]) {
    if (hipMemsetAsync(acc.p, 0, 2 * sizeof(double), st) != hipSuccess) return false;
    int grid = int((nh + 255) / 256); if (grid > grid_cap) grid = grid_cap;
    hipLaunchKernelGGL(sew_reduce_kernel, dim3(grid), dim3(256), 0, st, pw.p, nh, bin_hz, dt, acc.p);
    if (hipMemcpyAsync(h, acc.p, 2 * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return false;
    ++evals;
    return true;
  }
  // (signal energy, removed energy) for a knot spacing, both as sew.py's signal_energy (sum |.|^2 / n)
  bool energies(double dt, double* energy, double* removed) {
    double h[2];
    if (!sums(dt, h)) return false;
    *energy = h[0] / double(n); *removed = h[1] / double(n);
    return true;
  }
};

SewSpectrum& g_sew = *new SewSpectrum;   // never destroyed: at process exit the HIP runtime may be gone before a static's destructor runs
std::mutex g_sew_mutex;   // one call at a time: concurrent callers (other devices, other sizes) would rebuild each other's plan mid-use

}  // namespace

extern "C" int oicc_sew_knot_spacing_and_variance(int32_t device_ordinal, int32_t dims, int64_t n, const double* signal,
                                                  const double* times, double quality, double min_dt, double max_dt,
                                                  double* dt_out, double* var_out, int32_t* num_evaluations) {
  if (!signal || !times || !dt_out || !var_out || dims < 1 || n < 8 || !(quality > 0.0 && quality < 1.0)) return OICC_ERR_INVALID_ARG;
  if (int rc = oicc::select_device(device_ordinal)) return rc;
  // sample rate = 1 / mean(diff(times))  (sew.py:144)
  const double span = times[n - 1] - times[0];
  if (!(span > 0.0)) return OICC_ERR_INVALID_ARG;
  const double sample_rate = double(n - 1) / span;
  if (!(min_dt > 0.0)) min_dt = 1.0 / sample_rate;                       // sew.py:153-154
  if (!(max_dt > 0.0)) max_dt = (double(n) / 4.0) / sample_rate;         // sew.py:156-157

  std::lock_guard<std::mutex> lock(g_sew_mutex);
  SewSpectrum& D = g_sew;
  int rc = D.bind(device_ordinal, dims, n);
  if (rc != OICC_OK) return rc;
  rc = D.transform(signal, sample_rate, kSewGridCap);
  if (rc != OICC_OK) return rc;

  // quality_func(dt) = max_remove / removed(dt), max_remove = signal_energy(Xhat) (1 - quality)  (sew.py:146-151)
  bool ok = true;
  double energy = 0.0;
  auto quality_func = [&](double dt) -> double {
    double e = 0.0, r = 0.0;
    if (!D.energies(dt, &e, &r)) { ok = false; return 0.0; }
    energy = e;
    return e * (1.0 - quality) / r;
  };
  const double min_q = 1.0;
  double found = max_dt;
  // ---- find_max_quality_dt (sew.py:83-137)
  double q = quality_func(max_dt);
  if (ok && !(q >= min_q)) {
    double dt = max_dt, step = max_dt * 0.5, best_q = 0.0, best_dt = std::nan("");
    while (ok) {
      dt -= step;
      dt = std::fmax(dt, min_dt);
      q = quality_func(dt);
      if (!ok) break;
      if (q > min_q) {
        // scipy.optimize.brentq(root, dt, max_dt) [EXT], root(dt) = quality_func(dt) - min_q
        const double xtol = 2e-12, rtol = 8.881784197001252e-16; const int maxiter = 100;
        double xpre = dt, xcur = max_dt, fpre = q - min_q, fcur = quality_func(max_dt) - min_q;
        double xblk = 0.0, fblk = 0.0, spre = 0.0, scur = 0.0;
        found = xcur;
        if (fpre == 0.0) { found = xpre; break; }
        if (fcur == 0.0) { found = xcur; break; }
        for (int it = 0; it < maxiter && ok; ++it) {
          if (fpre != 0.0 && fcur != 0.0 && (std::signbit(fpre) != std::signbit(fcur))) { xblk = xpre; fblk = fpre; spre = scur = xcur - xpre; }
          if (std::fabs(fblk) < std::fabs(fcur)) { xpre = xcur; xcur = xblk; xblk = xpre; fpre = fcur; fcur = fblk; fblk = fpre; }
          const double delta = (xtol + rtol * std::fabs(xcur)) / 2.0;
          const double sbis = (xblk - xcur) / 2.0;
          if (fcur == 0.0 || std::fabs(sbis) < delta) break;
          if (std::fabs(spre) > delta && std::fabs(fcur) < std::fabs(fpre)) {
            double stry;
            if (xpre == xblk) stry = -fcur * (xcur - xpre) / (fcur - fpre);                      // secant
            else { const double dpre = (fpre - fcur) / (xpre - xcur), dblk = (fblk - fcur) / (xblk - xcur);
                   stry = -fcur * (fblk * dblk - fpre * dpre) / (dblk * dpre * (fblk - fpre)); }   // inverse quadratic
            if (2.0 * std::fabs(stry) < std::fmin(std::fabs(spre), 3.0 * std::fabs(sbis) - delta)) { spre = scur; scur = stry; }
            else { spre = sbis; scur = sbis; }
          } else { spre = sbis; scur = sbis; }
          xpre = xcur; fpre = fcur;
          if (std::fabs(scur) > delta) xcur += scur; else xcur += (sbis > 0.0 ? delta : -delta);
          fcur = quality_func(xcur) - min_q;
        }
        found = xcur;
        break;
      }
      step *= 0.5;
      if (q > best_q) { best_q = q; best_dt = dt; }
      if (dt <= min_dt) { found = best_dt; break; }     // no dt satisfies the condition: the best one seen (sew.py:133-137)
    }
  }
  if (ok && found == found) {
    double e = 0.0, r = 0.0;
    ok = D.energies(found, &e, &r);
    *dt_out = found;
    *var_out = r / double(n);                            // dt_to_variance_spectrum, sew.py:192-195
  } else if (ok) { rc = OICC_ERR_STATE; }
  if (num_evaluations) *num_evaluations = D.evals;
  if (!ok) rc = OICC_ERR_HIP;
  return rc;
}

// Debug export (outside include/oicc_hip.h): the power spectrum and the raw sums of the spectral reduction (not divided by n)
// for a list of knot spacings, through the SewSpectrum the calibration entry drives.  grid_cap 0: the production cap of the
// reduction's grid; a positive value replaces it (the grid-stride loop at a test-sized spectrum).
extern "C" int oicc_debug_sew_spectrum(int32_t device_ordinal, int32_t dims, int64_t n, const double* signal, double sample_rate,
                                       int32_t num_dt, const double* dts, int32_t grid_cap, double* pw_out, double* sums_out) {
  if (!signal || !pw_out || dims < 1 || n < 8 || n > INT32_MAX || !(sample_rate > 0.0) || !std::isfinite(sample_rate) || num_dt < 0 || grid_cap < 0 ||
      (num_dt > 0 && (!dts || !sums_out))) return OICC_ERR_INVALID_ARG;
  for (int32_t i = 0; i < num_dt; ++i) if (!(dts[i] > 0.0) || !std::isfinite(dts[i])) return OICC_ERR_INVALID_ARG;
  if (int rc = oicc::select_device(device_ordinal)) return rc;
  std::lock_guard<std::mutex> lock(g_sew_mutex);
  SewSpectrum& D = g_sew;
  int rc = D.bind(device_ordinal, dims, n);
  if (rc != OICC_OK) return rc;
  rc = D.transform(signal, sample_rate, grid_cap > 0 ? grid_cap : kSewGridCap);
  if (rc != OICC_OK) return rc;
  if (hipMemcpyAsync(pw_out, D.pw.p, sizeof(double) * D.nh, hipMemcpyDeviceToHost, D.st) != hipSuccess || hipStreamSynchronize(D.st) != hipSuccess) return OICC_ERR_HIP;
  for (int32_t i = 0; i < num_dt; ++i) if (!D.sums(dts[i], sums_out + 2 * i)) return OICC_ERR_HIP;
  return OICC_OK;
}
