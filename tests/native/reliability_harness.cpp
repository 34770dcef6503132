// CPU harness around caliscope_amd/csrc/reliability_math.h — TEST INFRASTRUCTURE (built by g++ in tests/reliability_native.py).  It
// evaluates cba_observation_reliability on the host: everything up to C = St^-1 is the host replay of the pipeline (covariance_replay.h
// beside this file, with the canonical order of a point's observations, as the library asks cov_pipeline for it), then the work of
// k_rel_point with the per-element functions reliability_lib.hip uses, row after row of G_o.  The non-GPU suite checks the whole call
// against the dense projector with it and drives CaptureVolume.observation_reliability through its `_solver` hook.  It is not a CPU
// fallback: nothing in caliscope_amd/ loads it.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "covariance_replay.h"
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
  CovReplay rp;
  const int rc = cov_replay<COV_GAUGE>(d, nullptr, true, what, g_error, rp);
  if (rc) return rc;
  constexpr int WB = 3 * MAX_NC;
  const CovPlan& plan = rp.plan;
  const std::vector<CamTab>& tab = rp.tab;
  const std::vector<int32_t>& cam_sorted = rp.cam_sorted;
  const std::vector<double> &Y = rp.Y, &Vinv = rp.Vinv, &C = rp.C;
  const int32_t ncp = plan.ncp();
  const int64_t n_obs = d->n_obs, n_points = d->n_points;
  for (double v : C)
    if (!std::isfinite(v)) { g_error = cov_msg_not_finite(what, "camera"); return CBA_ERR_NUMERIC; }
  // k_rel_point
  const double sigma0 = std::sqrt(rp.sigma0_sq);
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
  if (out->sigma0_sq) *out->sigma0_sq = rp.sigma0_sq;
  if (out->dof) *out->dof = plan.dof;
  if (out->cost) *out->cost = rp.cost;
  if (out->n_uncontrolled) *out->n_uncontrolled = bad;
  return CBA_OK;
}

}
