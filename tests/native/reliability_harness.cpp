// CPU harness around caliscope_amd/csrc/reliability_math.h and covariance_math.h — TEST INFRASTRUCTURE (built by g++ in
// tests/reliability_native.py).  It evaluates cba_observation_reliability on the host: the checks and the steps up to C = St^-1 as
// tests/native/covariance_harness.cpp does them (serially, cov_spd_inverse for the dense factor and inverse of the device), then the work
// of k_rel_point with the per-element functions reliability_lib.hip uses, row after row of G_o.  The non-GPU suite checks the whole call
// against the dense projector with it and drives CaptureVolume.observation_reliability through its `_solver` hook.  It is not a CPU
// fallback: nothing in caliscope_amd/ loads it.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "ba_math.h"
#include "covariance_math.h"
#include "reliability_math.h"

using namespace cba;

namespace {
std::string g_error;
}

extern "C" {

const char* rh_last_error() { return g_error.c_str(); }

// REL_R_TINY
void rh_constants(double* out) { out[0] = REL_R_TINY; }

// rel_w of reliability_math.h
double rh_w(double f_scaled, double r, double sigma0) { return rel_w(f_scaled, r, sigma0); }

// cba_observation_reliability on the host: 0 or a CBA_ERR_* with rh_last_error() set
int rh_observation_reliability(const cba_cov_desc* d, cba_rel_out* out) {
  const std::string what = "cba_observation_reliability";
  if (!d || !out) { g_error = what + ": null argument"; return CBA_ERR_INVALID; }
  CovPlan plan;
  const int rc = cov_validate(d, plan, g_error, what.c_str(), true);
  if (rc) return rc;
  constexpr int G = COV_GAUGE, WB = 3 * MAX_NC;
  const int32_t n_cams = d->n_cams, ncp = plan.ncp();
  const int64_t n_obs = d->n_obs, n_points = d->n_points;
  // k_unc_cam
  std::vector<CamTab> tab((size_t)n_cams);
  std::vector<double> B((size_t)ncp * G, 0.0);
  for (int32_t c = 0; c < n_cams; ++c) {
    const int32_t off = plan.cam_off[(size_t)c], np = plan.cam_off[(size_t)c + 1] - off;
    double xc[MAX_NC] = {0};
    for (int i = 0; i < np; ++i) xc[i] = d->cam_x[(size_t)c * MAX_NC + i];
    cam_prepare(xc, d->cam_const + (size_t)c * CAM_CONST_STRIDE, d->cam_model[c], np, &tab[(size_t)c], off);
    double N[MAX_NC][G];
    cov_gauge_cam(tab[(size_t)c], N);
    for (int r = 0; r < np; ++r)
      for (int j = 0; j < G; ++j) B[(size_t)(off + r) * G + j] = N[r][j];
  }
  // k_unc_obs
  std::vector<double> Wblk((size_t)n_obs * WB), Vobs((size_t)n_obs * 6), U((size_t)n_cams * MAX_NC * MAX_NC, 0.0), Y((size_t)n_obs * WB);
  std::vector<int32_t> cam_sorted((size_t)n_obs);
  double cost = 0.0;
  for (int64_t i = 0; i < n_obs; ++i) {
    const int64_t o = plan.order[(size_t)i];
    const int32_t cam = d->obs_cam[o];
    double A[2][MAX_NC], Bo[2][3];
    cost += 0.5 * cov_obs_jacobian(tab[(size_t)cam], d->points + 3 * (size_t)d->obs_pt[o], d->obs_uv + 2 * (size_t)o, d->loss, d->f_scale, A, Bo);
    cov_obs_products(A, Bo, &Wblk[(size_t)i * WB], &Vobs[(size_t)i * 6]);
    cam_sorted[(size_t)i] = cam;
    for (int r = 0; r < MAX_NC; ++r)
      for (int q = r; q < MAX_NC; ++q) U[((size_t)cam * MAX_NC + r) * MAX_NC + q] += A[0][r] * A[0][q] + A[1][r] * A[1][q];
  }
  // k_unc_point, k_unc_d
  std::vector<double> Vinv((size_t)n_points * 6), St((size_t)ncp * ncp, 0.0), D((size_t)G * G, 0.0);
  for (int64_t p = 0; p < n_points; ++p) {
    const int64_t s = plan.pt_start[(size_t)p], k = plan.pt_start[(size_t)p + 1] - s;
    double V[6] = {0, 0, 0, 0, 0, 0};
    for (int64_t a = 0; a < k; ++a)
      for (int e = 0; e < 6; ++e) V[e] += Vobs[(size_t)(s + a) * 6 + e];
    double* Vi = &Vinv[(size_t)p * 6];
    if (!cov_point_vinv(V, Vi)) {
      g_error = what + ": point " + std::to_string(p) + ": its observations do not determine it (rays parallel or not finite)";
      return CBA_ERR_NUMERIC;
    }
    double Z[3][G], N[3][G];
    cov_point_z(Vi, d->points + 3 * (size_t)p, Z);
    cov_gauge_point(d->points[3 * p], d->points[3 * p + 1], d->points[3 * p + 2], N);
    for (int j = 0; j < G; ++j)
      for (int m = j; m < G; ++m) D[(size_t)j * G + m] += N[0][j] * Z[0][m] + N[1][j] * Z[1][m] + N[2][j] * Z[2][m];
    for (int64_t a = 0; a < k; ++a) {
      const double* w = &Wblk[(size_t)(s + a) * WB];
      double* y = &Y[(size_t)(s + a) * WB];
      const int32_t off = plan.cam_off[(size_t)cam_sorted[(size_t)(s + a)]], np = plan.cam_off[(size_t)cam_sorted[(size_t)(s + a)] + 1] - off;
      for (int r = 0; r < MAX_NC; ++r) {
        for (int q = 0; q < 3; ++q) y[3 * r + q] = w[3 * r] * cov_sym3(Vi, 0, q) + w[3 * r + 1] * cov_sym3(Vi, 1, q) + w[3 * r + 2] * cov_sym3(Vi, 2, q);
        if (r < np)
          for (int j = 0; j < G; ++j) B[(size_t)(off + r) * G + j] -= w[3 * r] * Z[0][j] + w[3 * r + 1] * Z[1][j] + w[3 * r + 2] * Z[2][j];
      }
    }
    for (int64_t a = 0; a < k; ++a)
      for (int64_t b = 0; b < k; ++b) {
        const int32_t ca = cam_sorted[(size_t)(s + a)], cb = cam_sorted[(size_t)(s + b)];
        const int32_t off_a = plan.cam_off[(size_t)ca], np_a = plan.cam_off[(size_t)ca + 1] - off_a;
        const int32_t off_b = plan.cam_off[(size_t)cb], np_b = plan.cam_off[(size_t)cb + 1] - off_b;
        for (int r = 0; r < np_a; ++r)
          for (int c = 0; c < np_b; ++c) {
            if (off_a + r > off_b + c) continue;
            const double* y = &Y[(size_t)(s + a) * WB + 3 * r];
            const double* w = &Wblk[(size_t)(s + b) * WB + 3 * c];
            St[(size_t)(off_a + r) * ncp + off_b + c] -= y[0] * w[0] + y[1] * w[1] + y[2] * w[2];
          }
      }
  }
  for (int j = 0; j < G; ++j)
    for (int m = j + 1; m < G; ++m) D[(size_t)m * G + j] = D[(size_t)j * G + m];
  if (!std::isfinite(cost) || !cov_spd_inverse(D, G)) {
    g_error = what + ": the points do not fix the seven gauge directions (all on one line, or not finite)";
    return CBA_ERR_NUMERIC;
  }
  const double sigma0_sq = 2.0 * cost / (double)plan.dof;
  // k_unc_assemble, the factorisation and k_unc_ttt
  for (int32_t row = 0; row < ncp; ++row)
    for (int32_t col = row; col < ncp; ++col) {
      double v = St[(size_t)row * ncp + col];
      int32_t cr = 0, cc = 0;
      while (plan.cam_off[(size_t)cr + 1] <= row) ++cr;
      while (plan.cam_off[(size_t)cc + 1] <= col) ++cc;
      if (cr == cc) v += U[((size_t)cr * MAX_NC + (row - plan.cam_off[(size_t)cr])) * MAX_NC + (col - plan.cam_off[(size_t)cr])];
      for (int j = 0; j < G; ++j) {
        double sdb = 0.0;
        for (int m = 0; m < G; ++m) sdb += D[(size_t)j * G + m] * B[(size_t)col * G + m];
        v += B[(size_t)row * G + j] * sdb;
      }
      St[(size_t)row * ncp + col] = v;
      St[(size_t)col * ncp + row] = v;
    }
  if (!cov_spd_inverse(St, ncp)) {
    g_error = what + ": the reduced camera system is not positive definite beyond the gauge (a pivot is not safely positive): "
                     "the scene does not determine every camera parameter";
    return CBA_ERR_NUMERIC;
  }
  const std::vector<double>& C = St;
  for (double v : C)
    if (!std::isfinite(v)) { g_error = what + ": a camera covariance is not finite"; return CBA_ERR_NUMERIC; }
  // k_rel_point
  const double sigma0 = std::sqrt(sigma0_sq);
  std::vector<double> red((size_t)n_obs * 3), w((size_t)n_obs * 2), f((size_t)n_obs * 2);
  int64_t bad = 0;
  for (int64_t p = 0; p < n_points; ++p) {
    const int64_t s = plan.pt_start[(size_t)p], k = plan.pt_start[(size_t)p + 1] - s;
    const double* X = d->points + 3 * (size_t)p;
    double Q[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t b = 0; b < k; ++b) {
      const int64_t o = plan.order[(size_t)(s + b)];
      const int32_t cam = cam_sorted[(size_t)(s + b)], off = plan.cam_off[(size_t)cam], np = plan.cam_off[(size_t)cam + 1] - off;
      double A[2][MAX_NC], Bo[2][3], M[6] = {0, 0, 0, 0, 0, 0}, S[3] = {0, 0, 0}, T[3];
      cov_obs_jacobian(tab[(size_t)cam], X, d->obs_uv + 2 * (size_t)o, d->loss, d->f_scale, A, Bo);
      for (int r = 0; r < np; ++r) {
        const double* crow = &C[(size_t)(off + r) * ncp];
        double g[3] = {0, 0, 0}, h[2], a[2];
        for (int64_t bp = 0; bp < k; ++bp) {
          const int32_t cb = cam_sorted[(size_t)(s + bp)], off_b = plan.cam_off[(size_t)cb], np_b = plan.cam_off[(size_t)cb + 1] - off_b;
          rel_row_times_y(crow + off_b, np_b, &Y[(size_t)(s + bp) * WB], g);
        }
        rel_row_times_a(crow + off, np, A, h);
        rel_a_column(A, r, a);
        rel_row_terms(a, &Y[(size_t)(s + b) * WB + 3 * r], g, h, Q, M, S);
      }
      rel_camera_part(S, M, Bo, T);
      for (int e = 0; e < 3; ++e) red[(size_t)o * 3 + e] = T[e];
    }
    for (int64_t b = 0; b < k; ++b) {
      const int64_t o = plan.order[(size_t)(s + b)];
      double A[2][MAX_NC], Bo[2][3];
      cov_obs_jacobian(tab[(size_t)cam_sorted[(size_t)(s + b)]], X, d->obs_uv + 2 * (size_t)o, d->loss, d->f_scale, A, Bo, &f[(size_t)o * 2]);
      const double T[3] = {red[(size_t)o * 3], red[(size_t)o * 3 + 1], red[(size_t)o * 3 + 2]};
      bad += rel_finish(Bo, &Vinv[(size_t)p * 6], Q, T, sigma0, &f[(size_t)o * 2], &red[(size_t)o * 3], &w[(size_t)o * 2]);
    }
  }
  for (double v : red)
    if (!std::isfinite(v)) { g_error = what + ": a redundancy number is not finite"; return CBA_ERR_NUMERIC; }
  if (out->redundancy) std::copy(red.begin(), red.end(), out->redundancy);
  if (out->w) std::copy(w.begin(), w.end(), out->w);
  if (out->residual) std::copy(f.begin(), f.end(), out->residual);
  if (out->sigma0_sq) *out->sigma0_sq = sigma0_sq;
  if (out->dof) *out->dof = plan.dof;
  if (out->cost) *out->cost = cost;
  if (out->n_uncontrolled) *out->n_uncontrolled = bad;
  return CBA_OK;
}

}
