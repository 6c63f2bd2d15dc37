// fit_allan_variance -- CLI with the reference's flags: IMU noise parameters from a still recording.
//
// Mirrors applications/fit_allan_variance.cc of the reference and core::AllanVarianceFitter
// (src/core/allan_variance_fitter.cc:12-128): telemetry JSON in, the Allan variance of the three accelerometer and the
// three gyroscope channels (here one oicc_allan_variance call, on the MI355X), then FitAllanGyr / FitAllanAcc per axis
// (oicc_allan_fit) and the reference's result lines in its order and units.  Extra flags: --device, --dry_run (read the
// file, print n / span / rate, no device), --result_output_json (the fitted values as JSON), --nr_clusters (10000 as the
// reference hard-codes).
#include <cmath>
#include <exception>
#include <fstream>
#include <iostream>
#include <vector>

#include "cli_common.hpp"

using namespace oicc_cli;

static int run_main(int argc, char* argv[]) {
  Flags F({{"telemetry_json", ""}, {"verbose", "false"}, {"device", "0"}, {"dry_run", "false"}, {"result_output_json", ""},
           {"nr_clusters", "10000"}});
  if (!F.parse(argc, argv)) return 2;
  CameraTelemetryData telemetry;
  CHECK_MSG(ReadTelemetryJSON(F.str("telemetry_json"), &telemetry), "Could not read: " << F.str("telemetry_json"));
  const int64_t n = int64_t(telemetry.accelerometer.size());
  CHECK_MSG(n >= 8, "telemetry too short");
  const int nr_clusters = int(F.d("nr_clusters"));
  std::vector<double> t(static_cast<size_t>(n), 0.0), w(static_cast<size_t>(6 * n), 0.0);
  for (int64_t i = 0; i < n; ++i) {
    t[size_t(i)] = telemetry.accelerometer[size_t(i)].t_s;
    for (int c = 0; c < 3; ++c) {
      w[size_t(c * n + i)] = telemetry.accelerometer[size_t(i)].v[size_t(c)];          // pushMPerSec2
      w[size_t((3 + c) * n + i)] = telemetry.gyroscope[size_t(i)].v[size_t(c)];        // pushRadPerSec (scaled below)
    }
  }
  const double span = t[size_t(n - 1)] - t[0];
  if (F.b("dry_run")) {
    std::cout << "Inputs: " << n << " IMU samples over " << span << " s, " << double(n - 1) / span << " Hz\n";
    return 0;
  }
  const char* names[6] = {"acc_x", "acc_y", "acc_z", "gyr_x", "gyr_y", "gyr_z"};
  std::cout << "Loading datastructes\n";
  for (int c = 0; c < 6; ++c) std::cout << names[c] << "  num of Cluster " << nr_clusters << "\n";
  const double gs = 57.3 * 3600;
  const double scale[6] = {1.0, 1.0, 1.0, gs, gs, gs};
  std::vector<int32_t> factors(static_cast<size_t>(nr_clusters), 0);
  std::vector<double> taus(static_cast<size_t>(nr_clusters), 0.0), sigma2(static_cast<size_t>(6 * nr_clusters), 0.0);
  int32_t nf = 0; double freq = 0, period = 0, mean[6], ms = 0;
  const int rc = oicc_allan_variance(int(F.d("device")), 6, n, w.data(), t.data(), scale, nr_clusters, &nf, factors.data(), taus.data(),
                                     sigma2.data(), &freq, &period, mean, &ms);
  CHECK_MSG(rc == 0, "Allan variance on the device failed with status " << rc);
  // AllanGyr::calc's report (allan_gyr.cc:39-67), gyroscope channels first as RunFit calls them
  auto calc_report = [&](const char* name) {
    std::cout << name << "  numData " << n << "\n";
    if (n < 10000) std::cout << name << "  Too few number\n";
    std::cout << name << "  start_t " << t[0] << "\n" << name << "  end_t " << t[size_t(n - 1)] << "\n"
              << name << " dt \n-------------" << span << " s\n-------------" << span / 60 << " min\n-------------" << span / 3600 << " h\n";
    if (span / 60 < 10) std::cout << name << "  Too short time!!!!\n";
    std::cout << name << "  freq " << freq << "\n" << name << "  period " << period << "\n";
  };
  Value out;
  out["num_samples"] = Value(n); out["freq"] = Value(freq); out["period"] = Value(period); out["num_factors"] = Value(int64_t(nf));
  Value axes;
  auto fit_axis = [&](int c, int kind, const char* title) {
    double p[5], C[5], rep[6]; int32_t used = 0, iters = 0;
    const int frc = oicc_allan_fit(kind, nf, taus.data(), sigma2.data() + size_t(c) * size_t(nf), freq, p, C, rep, &used, &iters);
    CHECK_MSG(frc == 0, "noise model fit of " << names[c] << " failed with status " << frc);
    std::cout << title << " \nC " << C[0] << " " << C[1] << " " << C[2] << " " << C[3] << " " << C[4] << "\n";
    if (kind == OICC_ALLAN_GYRO) {
      std::cout << " Bias Instability " << rep[3] << " rad/s\n"
                << " Bias Instability " << rep[0] << " rad/s, at " << rep[1] << " s\n"
                << " White Noise " << rep[4] << " rad/s\n"
                << " White Noise " << rep[2] << " rad/s\n"
                << "  bias " << mean[c] / 3600 << " degree/s\n";
    } else {
      std::cout << " Bias Instability " << rep[0] << " m/s^2\n" << " White Noise " << rep[2] << " m/s^2\n";
    }
    std::cout << "-------------------\n";
    if (F.b("verbose")) {
      std::cout << names[c] << " Q N B K R " << p[0] << " " << p[1] << " " << p[2] << " " << p[3] << " " << p[4] << ", " << used << " points, "
                << iters << " iterations, cost " << rep[5] << "\n";
    }
    Value a;
    a["Q"] = Value(p[0]); a["N"] = Value(p[1]); a["B"] = Value(p[2]); a["K"] = Value(p[3]); a["R"] = Value(p[4]);
    a["bias_instability"] = Value(rep[0]); a["tau_at_min"] = Value(rep[1]); a["white_noise"] = Value(rep[2]);
    a["bias_instability_B"] = Value(rep[3]); a["white_noise_N"] = Value(rep[4]); a["num_used"] = Value(int64_t(used));
    a["iterations"] = Value(int64_t(iters)); a["final_cost"] = Value(rep[5]);
    if (kind == OICC_ALLAN_GYRO) a["bias"] = Value(mean[c] / 3600);
    axes[names[c]] = a;
  };
  for (int c = 3; c < 6; ++c) calc_report(names[c]);
  fit_axis(3, OICC_ALLAN_GYRO, "Gyro X");
  fit_axis(4, OICC_ALLAN_GYRO, "Gyro y");
  fit_axis(5, OICC_ALLAN_GYRO, "Gyro z");
  std::cout << "==============================================\n==============================================\n";
  for (int c = 0; c < 3; ++c) calc_report(names[c]);
  fit_axis(0, OICC_ALLAN_ACC, "acc X");
  fit_axis(1, OICC_ALLAN_ACC, "acc y");
  fit_axis(2, OICC_ALLAN_ACC, "acc z");
  if (F.b("verbose")) std::cout << "Allan variance of " << nf << " cluster sizes x 6 channels: " << ms << " ms on the device\n";
  out["axes"] = axes;
  if (!F.str("result_output_json").empty()) {
    std::ofstream f(F.str("result_output_json"));
    CHECK_MSG(f.is_open(), "cannot write " << F.str("result_output_json"));
    oicc_json::dump(out, f, 2); f << std::endl;
  }
  return 0;
}

// A malformed input file ends with a message and exit code 1, not in std::terminate.
int main(int argc, char* argv[]) {
  try { return run_main(argc, argv); }
  catch (const std::exception& e) { std::cerr << "error: " << e.what() << "\n"; return 1; }
}
