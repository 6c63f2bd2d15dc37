// Test driver of the C++ facade's covariance methods (csrc/host/estimator.hpp, cli_common.hpp), built by
// tests/test_gpu_covariance_facade.py into a shared library and called through ctypes ON THE PROBLEM OF THE PYTHON MIRROR: the facade
// wraps the mirror's handle, so both sides describe the same parameters and measurements.  Writes
//   {"covariance": covariance_json(GetCalibrationStdDevs(flags, scaled)), "estimate": EstimateCovariance(flags) as arrays}
#include <fstream>

#include "../openimucameracalibrator_amd/csrc/host/cli_common.hpp"

extern "C" int covariance_facade_driver(oicc_problem* problem, int flags, int scaled, const char* json_path) {
  try {
    using oicc_json::Value;
    OpenICC::core::ImuCameraCalibrator calibrator(problem);
    Value out;
    out["covariance"] = oicc_cli::covariance_json(calibrator.GetCalibrationStdDevs(flags, scaled != 0));
    const OpenICC::CovarianceEstimate c = calibrator.trajectory_.EstimateCovariance(flags);
    Value& e = out["estimate"];
    auto arr = [](const std::vector<double>& v) { Value o; o.type = Value::Array; for (double x : v) o.push_back(Value(x)); return o; };
    auto iarr = [](const int32_t* v, size_t n) { Value o; o.type = Value::Array; for (size_t i = 0; i < n; ++i) o.push_back(Value(int64_t(v[i]))); return o; };
    e["status"] = Value(int64_t(c.info.status)); e["P"] = Value(int64_t(c.info.P)); e["Pb"] = Value(int64_t(c.info.Pb)); e["a"] = Value(int64_t(c.info.a));
    e["hb"] = Value(int64_t(c.info.hb)); e["num_residuals"] = Value(int64_t(c.info.num_residuals));
    e["cost"] = Value(c.info.cost); e["variance_factor"] = Value(c.info.variance_factor); e["rcond"] = Value(c.info.rcond);
    e["arrow"] = arr(c.arrow); e["so3"] = arr(c.so3); e["r3"] = arr(c.r3);
    e["so3_offsets"] = iarr(c.so3_offsets.data(), c.so3_offsets.size()); e["r3_offsets"] = iarr(c.r3_offsets.data(), c.r3_offsets.size());
    e["accl_bias_offsets"] = iarr(c.accl_bias_offsets.data(), c.accl_bias_offsets.size());
    e["gyro_bias_offsets"] = iarr(c.gyro_bias_offsets.data(), c.gyro_bias_offsets.size());
    e["other_offsets"] = iarr(c.other_offsets, 5);
    std::ofstream f(json_path);
    if (!f.is_open()) return 2;
    oicc_json::dump(out, f, 1); f << std::endl;
    return 0;
  } catch (const std::exception& ex) {
    std::cerr << "covariance_facade_driver: " << ex.what() << "\n";
    return 1;
  }
}
