// static_imu_calibration -- CLI with the reference's flags: accelerometer and gyroscope intrinsics from a multi-pose
// recording (an initial still period, then the IMU held still in many orientations).
//
// Mirrors applications/static_imu_calibration.cc of the reference and core::StaticImuCalibrator::CalibrateAccGyro
// (src/core/static_imu_calibrator.cc:54-337): telemetry JSON in, one oicc_static_imu_calibrate call (static-interval
// detection, the accelerometer fits of all ten thresholds and the gyroscope residuals on the MI355X), the reference's
// progress lines in its order, and the calibration JSON (.cc:55-85, indent 4) that
// continuous_time_imu_to_camera_calibration --imu_intrinsics reads.  As the reference's main, a failed accelerometer
// calibration is reported and the default triads (identity, zero bias) are written.  Extra flags: --device, --dry_run
// (read the file, print n / span / rate, no device).  With --verbose a one-line solver summary per fit replaces Ceres'
// per-iteration table and FullReport.
#include <cmath>
#include <exception>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "cli_common.hpp"

using namespace oicc_cli;

namespace {

const char* kTerm[] = {"GRADIENT_TOLERANCE", "FUNCTION_TOLERANCE", "PARAMETER_TOLERANCE", "MAX_ITERATIONS", "MIN_TRUST_REGION_RADIUS",
                       "INVALID_STEPS", "EVALUATION_FAILED"};
const char* term_name(int t) { return t >= 0 && t <= 6 ? kTerm[t] : "SKIPPED"; }

// Eigen's default matrix print: every entry at the stream's precision, right-aligned to the widest, " " between columns
std::string eigen_print(const double* m, int rows, int cols) {
  std::vector<std::string> s(size_t(rows * cols));
  size_t w = 0;
  for (int i = 0; i < rows * cols; ++i) { std::ostringstream o; o << m[i]; s[size_t(i)] = o.str(); w = std::max(w, s[size_t(i)].size()); }
  std::ostringstream o;
  for (int r = 0; r < rows; ++r) {
    if (r) o << "\n";
    for (int c = 0; c < cols; ++c) { if (c) o << " "; o << std::setw(int(w)) << s[size_t(r * cols + c)]; }
  }
  return o.str();
}

// T = [[1,-yz,zy],[xz,1,-zx],[-xy,yx,1]], K = diag(s) (utils/types.h:238-241)
void triad(const double* p12, double T[9], double K[9]) {
  const double t[9] = {1.0, -p12[0], p12[1], p12[3], 1.0, -p12[2], -p12[4], p12[5], 1.0};
  for (int i = 0; i < 9; ++i) { T[i] = t[i]; K[i] = 0.0; }
  K[0] = p12[6]; K[4] = p12[7]; K[8] = p12[8];
}

void print_triad(const char* name, const double* p12) {
  double T[9], K[9];
  triad(p12, T, K);
  std::cout << name << " misalignment matrix: \n" << eigen_print(T, 3, 3) << std::endl
            << name << " scale matrix: \n" << eigen_print(K, 3, 3) << std::endl
            << name << " bias: \n" << eigen_print(p12 + 9, 1, 3) << std::endl
            << name << " inverse scale factors: " << 1.0 / p12[6] << " " << 1.0 / p12[7] << " " << 1.0 / p12[8] << std::endl;
}

Value row(double a, double b, double c) { Value v; v.push_back(Value(a)); v.push_back(Value(b)); v.push_back(Value(c)); return v; }

}  // namespace

static int run_main(int argc, char* argv[]) {
  Flags F({{"telemetry_json", ""}, {"gravity_magnitude", "9.811107"}, {"initial_static_interval_s", "10.0"},
           {"output_calibration_path", ""}, {"verbose", "false"}, {"device", "0"}, {"dry_run", "false"}});
  if (!F.parse(argc, argv)) return 2;
  CameraTelemetryData telemetry;
  CHECK_MSG(ReadTelemetryJSON(F.str("telemetry_json"), &telemetry), "Could not read: " << F.str("telemetry_json"));
  const int64_t n = int64_t(telemetry.accelerometer.size());
  CHECK_MSG(n >= 3, "Invalid data samples vector");
  std::vector<double> t(static_cast<size_t>(n)), acc(static_cast<size_t>(3 * n)), gyr(static_cast<size_t>(3 * n));
  for (int64_t i = 0; i < n; ++i) {
    t[size_t(i)] = telemetry.accelerometer[size_t(i)].t_s;
    for (int c = 0; c < 3; ++c) {
      acc[size_t(3 * i + c)] = telemetry.accelerometer[size_t(i)].v[size_t(c)];
      gyr[size_t(3 * i + c)] = telemetry.gyroscope[size_t(i)].v[size_t(c)];
    }
  }
  const double span = t[size_t(n - 1)] - t[0];
  if (F.b("dry_run")) {
    std::cout << "Inputs: " << n << " IMU samples over " << span << " s, " << double(n - 1) / span << " Hz\n";
    return 0;
  }
  const bool verbose = F.b("verbose");
  oicc_static_imu_options opt{F.d("gravity_magnitude"), F.d("initial_static_interval_s"), -1.0, 100, 12, 101, 0, 0, 0};
  double ap[9], gp[12];
  oicc_static_imu_report rep;
  const int rc = oicc_static_imu_calibrate(int(F.d("device")), n, t.data(), acc.data(), gyr.data(), &opt, ap, gp, &rep);
  CHECK_MSG(rc == OICC_OK || rc == OICC_SIMU_ACC_IMPOSSIBLE, "static IMU calibration on the device failed with status " << rc);

  // CalibrateAcc's lines (.cc:55-186)
  std::cout << "Accelerometers calibration: calibrating...";
  std::cout << "Setting initial accelerometer bias: " << eigen_print(rep.init_acc_bias, 1, 3) << "\n";
  for (int k = 0; k < OICC_SIMU_THRESHOLDS; ++k) {
    if (verbose)
      std::cout << "Accelerometers calibration: extracted " << rep.num_intervals[k] << " intervals using threshold multiplier " << k + 1 << " -> ";
    if (rep.acc_termination[k] == OICC_SIMU_TERM_SKIPPED) {
      if (verbose) std::cout << "Not enough intervals, calibration is not possible";
      continue;
    }
    if (verbose) std::cout << "\nLM: " << rep.acc_iterations[k] << " iterations, " << term_name(rep.acc_termination[k]) << "\n";
    std::cout << "Accelerometer residual " << rep.acc_final_cost[k] << "\n";
  }
  if (rc == OICC_SIMU_ACC_IMPOSSIBLE) {
    if (verbose) std::cout << "Accelerometers calibration: Can't obtain any calibratin with the current dataset";
    std::cerr << "Failed to calibra accelerometer\n";
  } else {
    const double a12[12] = {ap[0], ap[1], ap[2], 0, 0, 0, ap[3], ap[4], ap[5], ap[6], ap[7], ap[8]};
    print_triad("Accelerometer", a12);
    std::cout << std::endl;
    std::cout << "Gyroscopes calibration: calibrating...";
    if (verbose)
      std::cout << "\nLM: " << rep.gyro_num_blocks << " residual blocks, cost " << rep.gyro_initial_cost << " -> " << rep.gyro_final_cost << " in "
                << rep.gyro_iterations << " iterations, " << term_name(rep.gyro_termination) << "\n";
    std::cout << "Gyroscopes calibration: residual " << rep.gyro_final_cost << std::endl;
    print_triad("Gyroscope", gp);
  }
  if (verbose)
    std::cout << "Device time: detector " << rep.ms_detector << " ms, accelerometer fits " << rep.ms_acc << " ms, gyroscope evaluations "
              << rep.ms_gyro << " ms\n";

  // the output document (.cc:55-85): on failure ap / gp hold the default triads
  Value out, a, g, m, s, b;
  m.push_back(row(1.0, -ap[0], ap[1])); m.push_back(row(0.0, 1.0, -ap[2])); m.push_back(row(0.0, 0.0, 1.0));
  s.push_back(row(ap[3], 0.0, 0.0)); s.push_back(row(0.0, ap[4], 0.0)); s.push_back(row(0.0, 0.0, ap[5]));
  a["misalignment_matrix"] = m; a["scale_matrix"] = s; a["bias"] = row(ap[6], ap[7], ap[8]);
  Value mg, sg;
  mg.push_back(row(1.0, -gp[0], gp[1])); mg.push_back(row(gp[3], 1.0, -gp[2])); mg.push_back(row(-gp[4], gp[5], 1.0));
  sg.push_back(row(gp[6], 0.0, 0.0)); sg.push_back(row(0.0, gp[7], 0.0)); sg.push_back(row(0.0, 0.0, gp[8]));
  g["misalignment_matrix"] = mg; g["scale_matrix"] = sg; g["bias"] = row(gp[9], gp[10], gp[11]);
  out["accelerometer"] = a; out["gyroscope"] = g;
  std::ofstream f(F.str("output_calibration_path"));
  CHECK_MSG(f.is_open(), "cannot write " << F.str("output_calibration_path"));
  oicc_json::dump(out, f, 4); f << std::endl;
  return 0;
}

// A malformed input file ends with a message and exit code 1, not in std::terminate.
int main(int argc, char* argv[]) {
  try { return run_main(argc, argv); }
  catch (const std::exception& e) { std::cerr << "error: " << e.what() << "\n"; return 1; }
}
