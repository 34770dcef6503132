// CPU harness around caliscope_amd/csrc/covariance_math.h — TEST INFRASTRUCTURE (built by g++ in tests/covariance_native.py).
// It evaluates cba_parameter_covariance with the checks, the gauge rows, the per-observation products and the per-point 3 x 3 pieces that
// covariance_lib.hip uses; the kernels' work runs serially (observation after observation, point after point) and the dense factor and
// inverse of the device (k_chol_step, k_unc_ttt) are cov_spd_inverse here, so that the non-GPU suite can check the whole call against an
// eigenvalue pseudo-inverse and drive CaptureVolume.parameter_uncertainty through its `_solver` hook.  It is not a CPU fallback: nothing
// in caliscope_amd/ loads it.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "ba_math.h"
#include "covariance_math.h"

using namespace cba;

namespace {
std::string g_error;
}

extern "C" {

const char* ch_last_error() { return g_error.c_str(); }

// COV_GAUGE, COV_BLOCK, COV_POINT_THREADS, COV_MAX_NCP
void ch_constants(int32_t* out) { out[0] = COV_GAUGE; out[1] = COV_BLOCK; out[2] = COV_POINT_THREADS; out[3] = COV_MAX_NCP; }

// gauge rows of one camera (N[9][7], rows behind nparams zero) and of one point (N[3][7])
void ch_gauge_cam(const double* x9, const double* cconst, int32_t model, int32_t nparams, double* N) {
  double xc[MAX_NC] = {0};
  for (int i = 0; i < nparams; ++i) xc[i] = x9[i];
  CamTab t;
  cam_prepare(xc, cconst, model, nparams, &t, 0);
  cov_gauge_cam(t, reinterpret_cast<double (*)[COV_GAUGE]>(N));
}
void ch_gauge_point(const double* X, double* N) { cov_gauge_point(X[0], X[1], X[2], reinterpret_cast<double (*)[COV_GAUGE]>(N)); }

// cba_parameter_covariance on the host: 0 or a CBA_ERR_* with ch_last_error() set
int ch_parameter_covariance(const cba_cov_desc* d, cba_cov_out* out) {
  const std::string what = "cba_parameter_covariance";
  if (!d || !out) { g_error = what + ": null argument"; return CBA_ERR_INVALID; }
  CovPlan plan;
  const int rc = cov_validate(d, plan, g_error);
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
  std::vector<double> Vinv((size_t)n_points * 6), Zall((size_t)n_points * 3 * G), St((size_t)ncp * ncp, 0.0), D((size_t)G * G, 0.0);
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
    double (*Z)[G] = reinterpret_cast<double (*)[G]>(&Zall[(size_t)p * 3 * G]);
    cov_point_z(Vi, d->points + 3 * (size_t)p, Z);
    double N[3][G];
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
  // k_unc_point_cov
  std::vector<double> point_cov;
  if (out->point_cov) {
    std::vector<double> E, F;
    cov_gauge_terms(ncp, C.data(), B.data(), D.data(), E, F);
    point_cov.resize((size_t)n_points * 6);
    for (int64_t p = 0; p < n_points; ++p) {
      const int64_t s = plan.pt_start[(size_t)p], k = plan.pt_start[(size_t)p + 1] - s;
      const double (*Z)[G] = reinterpret_cast<const double (*)[G]>(&Zall[(size_t)p * 3 * G]);
      double full[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
      for (int64_t a = 0; a < k; ++a) {
        const int32_t ca = cam_sorted[(size_t)(s + a)], off_a = plan.cam_off[(size_t)ca], np_a = plan.cam_off[(size_t)ca + 1] - off_a;
        const double* ya = &Y[(size_t)(s + a) * WB];
        for (int64_t b = 0; b < k; ++b) {
          const int32_t cb = cam_sorted[(size_t)(s + b)], off_b = plan.cam_off[(size_t)cb], np_b = plan.cam_off[(size_t)cb + 1] - off_b;
          const double* yb = &Y[(size_t)(s + b) * WB];
          for (int r = 0; r < np_a; ++r) {
            double t3[3] = {0, 0, 0};
            for (int c = 0; c < np_b; ++c)
              for (int q = 0; q < 3; ++q) t3[q] += C[(size_t)(off_a + r) * ncp + off_b + c] * yb[3 * c + q];
            for (int pp = 0; pp < 3; ++pp)
              for (int q = 0; q < 3; ++q) full[pp][q] += ya[3 * r + pp] * t3[q];
          }
        }
        for (int r = 0; r < np_a; ++r) {
          double t3[3] = {0, 0, 0};
          for (int j = 0; j < G; ++j)
            for (int q = 0; q < 3; ++q) t3[q] += E[(size_t)(off_a + r) * G + j] * Z[q][j];
          for (int pp = 0; pp < 3; ++pp)
            for (int q = 0; q < 3; ++q) full[pp][q] += 2.0 * ya[3 * r + pp] * t3[q];
        }
      }
      double P[6];
      cov_point_base(&Vinv[(size_t)p * 6], Z, F.data(), P);
      int e = 0;
      for (int pp = 0; pp < 3; ++pp)
        for (int q = pp; q < 3; ++q) {
          point_cov[(size_t)p * 6 + e] = sigma0_sq * (P[e] + 0.5 * (full[pp][q] + full[q][pp]));
          ++e;
        }
    }
    for (double v : point_cov)
      if (!std::isfinite(v)) { g_error = what + ": a point covariance is not finite"; return CBA_ERR_NUMERIC; }
  }
  for (double v : C)
    if (!std::isfinite(v)) { g_error = what + ": a camera covariance is not finite"; return CBA_ERR_NUMERIC; }
  if (out->point_cov) std::copy(point_cov.begin(), point_cov.end(), out->point_cov);
  if (out->cam_cov_full)
    for (size_t i = 0; i < C.size(); ++i) out->cam_cov_full[i] = sigma0_sq * C[i];
  if (out->cam_cov)
    for (int32_t c = 0; c < n_cams; ++c) {
      const int32_t off = plan.cam_off[(size_t)c], np = plan.cam_off[(size_t)c + 1] - off;
      for (int r = 0; r < MAX_NC; ++r)
        for (int q = 0; q < MAX_NC; ++q)
          out->cam_cov[((size_t)c * MAX_NC + r) * MAX_NC + q] = (r < np && q < np) ? sigma0_sq * C[(size_t)(off + r) * ncp + off + q] : 0.0;
    }
  if (out->sigma0_sq) *out->sigma0_sq = sigma0_sq;
  if (out->dof) *out->dof = plan.dof;
  if (out->cost) *out->cost = cost;
  return CBA_OK;
}

}
