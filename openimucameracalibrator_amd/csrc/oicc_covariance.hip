// liboicc_hip: covariance estimation behind oicc_estimate_covariance and its getters (include/oicc_hip.h) -- the host side that
// sequences the kernels of kernels_covariance.hip around the forward factor of the LM solve (kernels_cholesky.hip).  No arithmetic
// of the inverse runs here; the host only reads the result back, takes the maximum of the scaled diagonal and keeps the copy the
// getters hand out.
#include "oicc_problem.h"

namespace oicc {
namespace {

// Name of tangent column i through the layout (the style of describe() in tests/normal_equations_reference.py).
std::string describe_column(const HostLayout& L, int i) {
  char buf[96];
  const std::vector<int32_t>* fam[4] = {&L.so3, &L.r3, &L.ab, &L.gb};
  const char* names[4] = {"so3", "r3", "accl_bias", "gyro_bias"};
  for (int f = 0; f < 4; ++f)
    for (size_t k = 0; k < fam[f]->size(); ++k) {
      const int o = (*fam[f])[k];
      if (o >= 0 && o <= i && i < o + 3) { std::snprintf(buf, sizeof(buf), "%s knot %d [%d]", names[f], int(k), i - o); return buf; }
    }
  const char* onames[5] = {"T_i_c", "gravity", "line_delay", "accl_intrinsics", "gyro_intrinsics"};
  const int on[5] = {6, 3, 1, 6, 9};
  for (int f = 0; f < 5; ++f) {
    const int o = L.other[f];
    if (o >= 0 && o <= i && i < o + on[f]) { std::snprintf(buf, sizeof(buf), "%s [%d]", onames[f], i - o); return buf; }
  }
  std::snprintf(buf, sizeof(buf), "column %d (point)", i);
  return buf;
}

int unsupported(oicc_problem* p, const std::string& why) { p->err = "oicc_estimate_covariance: " + why; return OICC_ERR_UNSUPPORTED; }

}  // namespace
}  // namespace oicc

extern "C" {

int oicc_estimate_covariance(oicc_problem* p, int32_t flags, oicc_covariance_info* info) {
  ARG(p, info != nullptr, "info");
  std::memset(info, 0, sizeof(*info));
  oicc_problem::Cov& cv = p->cov;
  cv.valid = false;
  if (flags & OICC_POINTS) return unsupported(p, "OICC_POINTS is not supported (the gauge freedom of the board makes J^T J singular)");
  if (p->shard_n > 1) return unsupported(p, "time-sharded problems (oicc_set_shard) are not supported");
  if (p->reduce != nullptr) return unsupported(p, "problems with a reduction across ranks installed (oicc_set_allreduce / oicc_rccl_init) are not supported: one rank holds only its part of the normal equations");
  int rc = prepare(p, flags); if (rc) return rc;
  hipStream_t st = p->stream;
  const TangentLayout& tl = p->tl;
  const int P = tl.P, Pb = tl.Pb, a = tl.a;
  info->P = P; info->Pb = Pb; info->a = a; info->hb = tl.hb;
  info->num_residuals = int64_t(2 * p->corner_view.size() + 3 * p->acc.size() + 3 * p->gyr.size());
  if (tl.a_pts > 0) return unsupported(p, "board point columns are not supported");
  if (tl.hb > kCovMaxHalfBandwidth) return unsupported(p, "half bandwidth " + std::to_string(tl.hb) + " exceeds " + std::to_string(kCovMaxHalfBandwidth) + " (the LDS window of the backward sweep)");
  if (a > kCovMaxArrow) return unsupported(p, std::to_string(a) + " arrow columns exceed " + std::to_string(kCovMaxArrow));
  ARG(p, P > 0, "no active parameters");
  rc = eval_pass(p, jacobian_pass(p->d_x.p)); if (rc) return rc;

  const size_t aa = std::max<size_t>(size_t(a) * a, 1), pb = std::max<size_t>(Pb, 1);
  if (!cv.d_s.resize(P) || !cv.d_Cs.resize(aa) || !cv.d_Sc.resize(aa) || !cv.d_Zaa.resize(aa) || !cv.d_aa.resize(aa) || !cv.d_zb.resize(pb * 3) ||
      !cv.d_G.resize(pb * std::max(a, 1)) || !cv.d_cov3.resize(pb * 3) || !cv.d_cross.resize(pb * std::max(a, 1)) || !cv.d_zs.resize(P) || !cv.d_flags.resize(2)) {
    p->err = "hipMalloc covariance buffers"; return OICC_ERR_HIP; }
  const CovBuffers cb{cv.d_s.p, cv.d_Cs.p, cv.d_Sc.p, cv.d_Zaa.p, cv.d_aa.p, cv.d_zb.p, cv.d_G.p, cv.d_cov3.p, cv.d_cross.p, cv.d_zs.p, cv.d_flags.p};
  SolveBuffers sb = solve_buffers(p);
  sb.force_p = 1; sb.algo = 1;   // the single-workgroup sweep (window 64 / 128), or the global-memory factorisation where its LDS does not fit
  const bool poison = p->opt.debug_poison_lds != 0.0;
  struct Events { hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}; ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); } } events;   // (released on every return)
  hipEvent_t* const ev = events.e;
  for (int k = 0; k < 5; ++k) HIPCK(p, hipEventCreate(&ev[k]));
  HIPCK(p, hipMemsetAsync(p->d_state.p, 0, sizeof(LmState), st));
  if (poison) launch_lds_poison(st);
  HIPCK(p, hipEventRecord(ev[0], st));
  launch_cov_build(p->ne, tl, cb, sb.Mb, sb.Mt, sb.Mc, st);
  HIPCK(p, hipEventRecord(ev[1], st));
  if (Pb > 0) launch_band_arrow_cholesky(tl, sb, st);
  else HIPCK(p, hipMemsetAsync(cv.d_zs.p, 0, sizeof(double) * P, st));
  HIPCK(p, hipEventRecord(ev[2], st));
  launch_cov_corner(tl, cb, sb.Mt, st);
  HIPCK(p, hipEventRecord(ev[3], st));
  if (poison) launch_lds_poison(st);
  if (launch_cov_sweep(tl, cb, sb.Mb, sb.Mt, st) != 0) return unsupported(p, "geometry");
  launch_cov_finish(tl, cb, st);
  HIPCK(p, hipEventRecord(ev[4], st));
  HIPCK(p, hipGetLastError());

  int32_t hflags[2] = {0, 0}; LmState hs; double cost = 0.0;
  std::vector<double> zs(P);
  cv.arrow.assign(size_t(a) * a, 0.0); cv.cov3.assign(size_t(Pb) * 3, 0.0); cv.cross.assign(size_t(Pb) * a, 0.0);
  HIPCK(p, hipMemcpyAsync(hflags, cv.d_flags.p, sizeof(hflags), hipMemcpyDeviceToHost, st));
  HIPCK(p, hipMemcpyAsync(&hs, p->d_state.p, sizeof(hs), hipMemcpyDeviceToHost, st));
  HIPCK(p, hipMemcpyAsync(&cost, p->ne.cost(), sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCK(p, hipMemcpyAsync(zs.data(), cv.d_zs.p, sizeof(double) * P, hipMemcpyDeviceToHost, st));
  if (a > 0) HIPCK(p, hipMemcpyAsync(cv.arrow.data(), cv.d_aa.p, sizeof(double) * a * a, hipMemcpyDeviceToHost, st));
  if (Pb > 0) HIPCK(p, hipMemcpyAsync(cv.cov3.data(), cv.d_cov3.p, sizeof(double) * Pb * 3, hipMemcpyDeviceToHost, st));
  if (Pb > 0 && a > 0) HIPCK(p, hipMemcpyAsync(cv.cross.data(), cv.d_cross.p, sizeof(double) * Pb * a, hipMemcpyDeviceToHost, st));
  HIPCK(p, hipStreamSynchronize(st));
  for (int k = 0; k < 4; ++k) { float ms = 0; (void)hipEventElapsedTime(&ms, ev[k], ev[k + 1]); cv.ms[k] = ms; }

  info->cost = cost;
  const double dof = double(info->num_residuals) - double(P);
  info->variance_factor = dof > 0.0 ? 2.0 * cost / dof : std::nan("");
  cv.flags = flags; cv.P = P; cv.Pb = Pb; cv.a = a; cv.so3 = p->L.so3; cv.r3 = p->L.r3;
  if (hflags[0] < P) {
    info->status = OICC_COV_ZERO_COLUMN;
    p->err = "oicc_estimate_covariance: the diagonal entry of J^T J at " + describe_column(p->L, hflags[0]) + " is not finite and positive";
    cv.info = *info; return OICC_OK;
  }
  double zmax = 0.0; bool bad = hs.chol_failed != 0 || hflags[1] != 0;
  for (int i = 0; i < P; ++i) { if (!(zs[i] > 0.0) || !std::isfinite(zs[i])) bad = true; else zmax = std::max(zmax, zs[i]); }
  info->rcond = (bad || zmax <= 0.0) ? 0.0 : 1.0 / zmax;
  if (bad || info->rcond < p->opt.covariance_min_rcond) {
    info->status = OICC_COV_RANK_DEFICIENT;
    char buf[160]; std::snprintf(buf, sizeof(buf), "oicc_estimate_covariance: rank deficient (%s, rcond %.3e)", bad ? "a pivot is not positive" : "below covariance_min_rcond", info->rcond);
    p->err = buf; cv.info = *info; return OICC_OK;
  }
  info->status = OICC_COV_OK;
  cv.info = *info; cv.valid = true;
  return OICC_OK;
}

int oicc_get_covariance_arrow(const oicc_problem* p, double* cov, int32_t a_capacity) {
  if (!p->cov.valid) return OICC_ERR_STATE;
  if (cov == nullptr || a_capacity < p->cov.a) return OICC_ERR_INVALID_ARG;
  std::copy(p->cov.arrow.begin(), p->cov.arrow.end(), cov);
  return OICC_OK;
}

int oicc_get_covariance_knots(const oicc_problem* p, double* so3_blocks, int64_t n_so3, double* r3_blocks, int64_t n_r3) {
  const oicc_problem::Cov& cv = p->cov;
  if (!cv.valid) return OICC_ERR_STATE;
  if ((so3_blocks && n_so3 != int64_t(cv.so3.size())) || (r3_blocks && n_r3 != int64_t(cv.r3.size()))) return OICC_ERR_INVALID_ARG;
  auto fill = [&](const std::vector<int32_t>& off, double* out) {
    for (size_t k = 0; k < off.size(); ++k) {
      double* b = out + 9 * k;
      const int o = off[k];
      if (o < 0 || o + 3 > cv.Pb) { for (int e = 0; e < 9; ++e) b[e] = std::nan(""); continue; }
      for (int r = 0; r < 3; ++r) for (int d = 0; r + d < 3; ++d) { const double v = cv.cov3[size_t(o + r) * 3 + d]; b[r * 3 + r + d] = v; b[(r + d) * 3 + r] = v; }
    }
  };
  if (so3_blocks) fill(cv.so3, so3_blocks);
  if (r3_blocks) fill(cv.r3, r3_blocks);
  return OICC_OK;
}

int oicc_get_covariance_knot_arrow(const oicc_problem* p, int32_t kind, int64_t knot, double* cross) {
  const oicc_problem::Cov& cv = p->cov;
  if (!cv.valid) return OICC_ERR_STATE;
  const std::vector<int32_t>& off = kind == 0 ? cv.so3 : cv.r3;
  if (cross == nullptr || (kind != 0 && kind != 1) || knot < 0 || knot >= int64_t(off.size())) return OICC_ERR_INVALID_ARG;
  const int o = off[size_t(knot)];
  for (int r = 0; r < 3; ++r) for (int q = 0; q < cv.a; ++q) cross[r * cv.a + q] = (o < 0 || o + 3 > cv.Pb) ? std::nan("") : cv.cross[size_t(o + r) * cv.a + q];
  return OICC_OK;
}

int oicc_get_covariance_timing(const oicc_problem* p, double ms[4]) {
  if (ms == nullptr) return OICC_ERR_INVALID_ARG;
  std::copy(p->cov.ms, p->cov.ms + 4, ms);
  return OICC_OK;
}

}  // extern "C"
