// liboicc_hip, host side: residual report and corner gating of the spline problem (include/oicc_hip.h; kernels: kernels_report.hip).
// The report needs the measurements and the parameters on the device, not the tangent layout: it runs at whatever flags the problem
// was last laid out for and rebuilds nothing.  Gating changes 1/sigma of corners on the host and marks the measurements changed exactly
// as Add*Measurement does, so the next pass uploads them and rebuilds the tiles and the inner-iteration plan.
#include "oicc_problem.h"

namespace oicc {
namespace {

int unsupported(oicc_problem* p, const char* entry) {
  p->err = std::string(entry) + ": time-sharded problems (oicc_set_shard) and problems with a reduction across ranks installed are not supported (the median would be a collective)";
  return OICC_ERR_UNSUPPORTED;
}

// measurements (time sorted) and parameters on the device
int measurements_and_parameters_on_device(oicc_problem* p) {
  ARG(p, p->pl.n_so3 > 0, "oicc_set_times has not been called");
  ARG(p, p->max_corner_pt < p->pl.n_pts, "a corner refers to a board point beyond those of oicc_set_scene_points");
  HIPCK(p, hipSetDevice(p->device));
  p->wait_plan();   // (a plan job on the second thread reads the measurement vectors sync_groups may sort)
  sync_groups(p);
  int rc = sync_measurements(p); if (rc) return rc;
  return sync_params_to_device(p);
}

// sorted position -> position in the caller's order (an empty map is the identity)
template <class I> size_t caller_index(const std::vector<I>& orig, size_t i) { return orig.empty() ? i : size_t(orig[i]); }

}  // namespace
}  // namespace oicc

extern "C" {

int oicc_residual_report(oicc_problem* p, oicc_residual_info* info) {
  ARG(p, info != nullptr, "info");
  std::memset(info, 0, sizeof(*info));
  oicc_problem::Report& R = p->report;
  R.valid = false;
  if (p->shard_n > 1 || p->reduce != nullptr) return unsupported(p, "oicc_residual_report");
  int rc = measurements_and_parameters_on_device(p); if (rc) return rc;
  hipStream_t st = p->stream;
  const size_t nc = p->corner_view.size(), nv = p->view_rs.size(), na = p->acc.size(), ng = p->gyr.size();
  const size_t rows_a = (na + 63) / 64, rows_g = (ng + 63) / 64;
  if (!R.d_e.resize(std::max<size_t>(2 * nc, 1)) || !R.d_status.resize(std::max<size_t>(nc, 1)) || !R.d_vn.resize(std::max<size_t>(nv, 1)) ||
      !R.d_vsum.resize(std::max<size_t>(nv, 1)) || !R.d_vmax.resize(std::max<size_t>(nv, 1)) || !R.d_acc_r.resize(std::max<size_t>(3 * na, 1)) ||
      !R.d_gyr_r.resize(std::max<size_t>(3 * ng, 1)) || !R.d_part.resize(std::max<size_t>(6 * (rows_a + rows_g), 1))) { p->err = "hipMalloc residual report"; return OICC_ERR_HIP; }
  EventPair ev;
  HIPCK(p, hipEventCreate(&ev.a)); HIPCK(p, hipEventCreate(&ev.b));
  const EvalCtx ctx = make_ctx(p, p->d_x.p);
  HIPCK(p, hipEventRecord(ev.a, st));
  launch_report_views(ctx, view_data(p, false), p->d_cgate.p, R.d_e.p, R.d_status.p, R.d_vn.p, R.d_vsum.p, R.d_vmax.p, st);
  launch_report_imu(ctx, imu_data(p->acc, p->d_acc), 1, R.d_acc_r.p, R.d_part.p, st);
  launch_report_imu(ctx, imu_data(p->gyr, p->d_gyr), 2, R.d_gyr_r.p, R.d_part.p + 6 * rows_a, st);
  HIPCK(p, hipEventRecord(ev.b, st));
  HIPCK(p, hipGetLastError());
  R.e_uv.assign(2 * nc, 0.0); R.status.assign(nc, 0); R.view_n.assign(nv, 0); R.view_sum.assign(nv, 0.0); R.view_max.assign(nv, 0.0);
  std::vector<double> part(6 * (rows_a + rows_g), 0.0);
  if (nc) { HIPCK(p, hipMemcpyAsync(R.e_uv.data(), R.d_e.p, 2 * nc * sizeof(double), hipMemcpyDeviceToHost, st));
            HIPCK(p, hipMemcpyAsync(R.status.data(), R.d_status.p, nc, hipMemcpyDeviceToHost, st)); }
  if (nv) { HIPCK(p, hipMemcpyAsync(R.view_n.data(), R.d_vn.p, nv * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIPCK(p, hipMemcpyAsync(R.view_sum.data(), R.d_vsum.p, nv * sizeof(double), hipMemcpyDeviceToHost, st));
            HIPCK(p, hipMemcpyAsync(R.view_max.data(), R.d_vmax.p, nv * sizeof(double), hipMemcpyDeviceToHost, st)); }
  if (!part.empty()) HIPCK(p, hipMemcpyAsync(part.data(), R.d_part.p, part.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCK(p, hipStreamSynchronize(st));
  { float ms = 0; (void)hipEventElapsedTime(&ms, ev.a, ev.b); info->ms_device = ms; }
  R.n_acc = na; R.n_gyr = ng;

  info->num_corners = int64_t(nc); info->num_views = int64_t(nv); info->num_accl = int64_t(na); info->num_gyro = int64_t(ng);
  std::vector<double> mag; mag.reserve(nc);
  double sum = 0.0;
  for (size_t c = 0; c < nc; ++c) {
    if (R.status[c] == OICC_CORNER_PROJECTION_FAILED) { ++info->num_failed; continue; }
    if (R.status[c] == OICC_CORNER_GATED) { ++info->num_gated; continue; }
    const double m = std::sqrt(R.e_uv[2 * c] * R.e_uv[2 * c] + R.e_uv[2 * c + 1] * R.e_uv[2 * c + 1]);
    mag.push_back(m); sum += m;
  }
  info->num_used = int64_t(mag.size());
  if (!mag.empty()) {
    double ss = 0.0;
    for (size_t v = 0; v < nv; ++v) { ss += R.view_sum[v]; info->max_px = std::max(info->max_px, R.view_max[v]); }   // (the device's per-view sums, in view order)
    info->mean_px = sum / double(mag.size()); info->rms_px = std::sqrt(ss / double(mag.size()));
    const size_t h = mag.size() / 2;   // the median as numpy takes it: the middle value, or the mean of the two middle ones
    std::nth_element(mag.begin(), mag.begin() + h, mag.end());
    double med = mag[h];
    if (mag.size() % 2 == 0) med = 0.5 * (med + *std::max_element(mag.begin(), mag.begin() + h));
    info->median_px = med; info->sigma_px = med / 1.17741;   // Rayleigh: median = sigma sqrt(2 ln 2)
  }
  auto imu_rms = [&](const double* rows, size_t nrows, size_t n, double* rms, double* rms_w) {
    double s[6] = {0, 0, 0, 0, 0, 0};
    for (size_t r = 0; r < nrows; ++r) for (int k = 0; k < 6; ++k) s[k] += rows[6 * r + k];
    for (int k = 0; k < 3; ++k) { rms[k] = n ? std::sqrt(s[k] / double(n)) : 0.0; rms_w[k] = n ? std::sqrt(s[3 + k] / double(n)) : 0.0; }
  };
  imu_rms(part.data(), rows_a, na, info->accl_rms, info->accl_rms_weighted);
  imu_rms(part.data() + 6 * rows_a, rows_g, ng, info->gyro_rms, info->gyro_rms_weighted);
  R.valid = true;
  return OICC_OK;
}

int oicc_get_corner_errors(oicc_problem* p, double* e_uv, uint8_t* status, int64_t n) {
  const oicc_problem::Report& R = p->report;
  if (!R.valid) { p->err = "no residual report for the current parameters and measurements"; return OICC_ERR_STATE; }
  ARG(p, n == int64_t(R.status.size()), "corner count");
  for (size_t c = 0; c < R.status.size(); ++c) {
    const size_t o = caller_index(p->corner_orig, c);
    if (e_uv) { e_uv[2 * o] = R.e_uv[2 * c]; e_uv[2 * o + 1] = R.e_uv[2 * c + 1]; }
    if (status) status[o] = R.status[c];
  }
  return OICC_OK;
}

int oicc_get_view_errors(oicc_problem* p, double* rms_px, double* max_px, int32_t* n_used, int64_t nv) {
  const oicc_problem::Report& R = p->report;
  if (!R.valid) { p->err = "no residual report for the current parameters and measurements"; return OICC_ERR_STATE; }
  ARG(p, nv == int64_t(R.view_n.size()), "view count");
  for (size_t v = 0; v < R.view_n.size(); ++v) {
    const size_t o = caller_index(p->view_orig, v);
    if (rms_px) rms_px[o] = R.view_n[v] > 0 ? std::sqrt(R.view_sum[v] / double(R.view_n[v])) : 0.0;
    if (max_px) max_px[o] = R.view_max[v];
    if (n_used) n_used[o] = R.view_n[v];
  }
  return OICC_OK;
}

int oicc_get_imu_residuals(oicc_problem* p, int32_t kind, double* r_xyz, int64_t n) {
  const oicc_problem::Report& R = p->report;
  if (!R.valid) { p->err = "no residual report for the current parameters and measurements"; return OICC_ERR_STATE; }
  ARG(p, kind == 1 || kind == 2, "kind");
  const size_t ns = kind == 1 ? R.n_acc : R.n_gyr;
  ARG(p, r_xyz != nullptr && n == int64_t(ns), "sample count");
  if (ns == 0) return OICC_OK;
  const std::vector<int32_t>& orig = kind == 1 ? p->acc_orig : p->gyr_orig;
  std::vector<double> sorted; double* dst = r_xyz;
  if (!orig.empty()) { sorted.resize(3 * ns); dst = sorted.data(); }
  HIPCK(p, hipSetDevice(p->device));
  HIPCK(p, hipMemcpyAsync(dst, (kind == 1 ? R.d_acc_r : R.d_gyr_r).p, 3 * ns * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  HIPCK(p, hipStreamSynchronize(p->stream));
  if (!orig.empty()) for (size_t i = 0; i < ns; ++i) std::copy(sorted.begin() + 3 * i, sorted.begin() + 3 * i + 3, r_xyz + 3 * size_t(orig[i]));
  return OICC_OK;
}

int oicc_gate_corners(oicc_problem* p, double threshold_px, int64_t* n_gated) {
  if (n_gated) *n_gated = 0;
  if (p->shard_n > 1 || p->reduce != nullptr) return unsupported(p, "oicc_gate_corners");
  const oicc_problem::Report& R = p->report;
  const bool lift = !(threshold_px > 0.0);
  if (!lift && !R.valid) { p->err = "oicc_gate_corners: no residual report for the current parameters and measurements"; return OICC_ERR_STATE; }
  p->wait_plan();   // (a plan job on the second thread reads the measurement vectors)
  const size_t nc = p->corner_view.size();
  bool changed = false; int64_t count = 0;
  for (size_t c = 0; c < nc; ++c) {
    bool g = false;
    if (!lift && R.status[c] != OICC_CORNER_PROJECTION_FAILED) g = std::sqrt(R.e_uv[2 * c] * R.e_uv[2 * c] + R.e_uv[2 * c + 1] * R.e_uv[2 * c + 1]) > threshold_px;
    count += g;
    if (g == (p->cgate[c] != 0)) continue;
    changed = true;
    p->cgate[c] = g ? 1 : 0;
    p->cisx[c] = g ? 0.0 : p->cisx0[c]; p->cisy[c] = g ? 0.0 : p->cisy0[c];
  }
  if (n_gated) *n_gated = count;
  if (changed) {   // as Add*Measurement leaves the problem: upload, tiles, inner-iteration plan, covariance and report
    p->meas_dirty = true; p->groups_dirty = true; p->layout_flags = -1; p->inner.flags = -2; p->invalidate_estimates();
  }
  return OICC_OK;
}

int oicc_get_corner_gate(oicc_problem* p, uint8_t* gated, int64_t n) {
  ARG(p, gated != nullptr && n == int64_t(p->cgate.size()), "corner count");
  for (size_t c = 0; c < p->cgate.size(); ++c) gated[caller_index(p->corner_orig, c)] = p->cgate[c];
  return OICC_OK;
}

}  // extern "C"
