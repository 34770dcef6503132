// CPU harness around caliscope_amd/csrc/covariance_constraint_plan.h and covariance_constraint_math.h — TEST INFRASTRUCTURE (built by g++ in
// tests/covariance_constrained_native.py).  cba_parameter_covariance_constrained on the host is the replay of the pipeline (covariance_replay.h
// beside this file) with the plan of the constraint rows and six gauge columns; without a row of positive weight it is the very call
// covariance_harness.cpp makes (seven columns, no plan), so the bytes are the same by construction.  Here are that dispatch and the probes of the
// host plan.  It is not a CPU fallback: nothing in caliscope_amd/ loads it.
#include <cstdint>
#include <string>

#include "covariance_replay.h"

using namespace cba;

namespace {
std::string g_error;
CovConPlan g_plan;  // of the last cch_plan

template <int G>
int run(const cba_cov_desc* d, CovConPlan* con, cba_cov_out* out, const std::string& what) {
  CovReplay rp;
  const int rc = cov_replay<G>(d, con, false, what, g_error, rp);
  return rc ? rc : cov_replay_outputs<G>(d, con, rp, what, g_error, out);
}
}  // namespace

extern "C" {

const char* cch_last_error() { return g_error.c_str(); }

// COV_COMPONENT_CAP, COV_GAUGE_RIGID, COV_GAUGE, doubles of LDS at the cap
void cch_constants(int64_t* out) { out[0] = COV_COMPONENT_CAP; out[1] = COV_GAUGE_RIGID; out[2] = COV_GAUGE; out[3] = (int64_t)cov_con_lds_doubles(COV_COMPONENT_CAP); }

// cba_parameter_covariance_constrained on the host: 0 or a CBA_ERR_* with cch_last_error() set; gauge_out: 6 or 7, rows_out: the kept rows
int cch_parameter_covariance_constrained(const cba_cov_desc* d, const cba_cov_constraints* con, cba_cov_out* out, int32_t* gauge_out, int64_t* rows_out) {
  const std::string what = "cba_parameter_covariance_constrained";
  if (!d || !out) { g_error = what + ": null argument"; return CBA_ERR_INVALID; }
  CovConPlan plan;
  if (d->n_points > 0 && d->n_points <= INT32_MAX) {
    const int rc = cov_con_components(d->n_points, con, plan, g_error, what.c_str());
    if (rc) return rc;
  }
  if (gauge_out) *gauge_out = plan.n_rows ? COV_GAUGE_RIGID : COV_GAUGE;
  if (rows_out) *rows_out = plan.n_rows;
  if (plan.n_rows == 0) return run<COV_GAUGE>(d, nullptr, out, "cba_parameter_covariance");
  return run<COV_GAUGE_RIGID>(d, &plan, out, what);
}

// The plan of a problem, kept for cch_plan_copy.  desc may be NULL (components only; no camera tables).  sizes: n_rows, n_comp, max_m, points in
// components, free points, (component, camera) pairs, component observations, entries.
int cch_plan(int64_t n_points, const cba_cov_desc* d, const cba_cov_constraints* con, int32_t cap, int64_t* sizes) {
  const int rc = cov_con_components(n_points, con, g_plan, g_error, "cba_parameter_covariance_constrained", cap);
  if (rc) return rc;
  if (d && g_plan.n_rows) {
    CovPlan plan;
    const int rv = cov_validate(d, plan, g_error, "cba_parameter_covariance_constrained", false, COV_GAUGE_RIGID, g_plan.in_row.data(), g_plan.n_rows);
    if (rv) return rv;
    cov_con_tables(plan, d->obs_cam, d->n_cams, d->n_points, g_plan);
  }
  sizes[0] = g_plan.n_rows; sizes[1] = g_plan.n_comp; sizes[2] = g_plan.max_m; sizes[3] = (int64_t)g_plan.pts.size(); sizes[4] = (int64_t)g_plan.free_pts.size();
  sizes[5] = (int64_t)g_plan.cams.size(); sizes[6] = (int64_t)g_plan.obs_pos.size(); sizes[7] = g_plan.n_entries();
  return CBA_OK;
}

// which: 0 comp_pt, 1 pts, 2 comp_row, 3 row_src, 4 row_loc, 5 free_pts, 6 comp_cam, 7 cams, 8 cc_obs, 9 obs_pos, 10 obs_loc, 11 entry_start, 12 entry_cam
// (all as int64)
void cch_plan_copy(int32_t which, int64_t* dst) {
  auto put = [&](const auto& v) { for (size_t i = 0; i < v.size(); ++i) dst[i] = (int64_t)v[i]; };
  switch (which) {
    case 0: put(g_plan.comp_pt); break;
    case 1: put(g_plan.pts); break;
    case 2: put(g_plan.comp_row); break;
    case 3: put(g_plan.row_src); break;
    case 4: put(g_plan.row_loc); break;
    case 5: put(g_plan.free_pts); break;
    case 6: put(g_plan.comp_cam); break;
    case 7: put(g_plan.cams); break;
    case 8: put(g_plan.cc_obs); break;
    case 9: put(g_plan.obs_pos); break;
    case 10: put(g_plan.obs_loc); break;
    case 11: put(g_plan.entry_start); break;
    default: put(g_plan.entry_cam); break;
  }
}

// one constraint row: u[3], coef[8], returns rho
double cch_row(const double* points, const int32_t* pt8, double dist, double weight, int32_t loss, double f_scale, double* u, double* coef) {
  return cov_con_row(points, pt8, dist, weight, loss, f_scale, u, coef);
}

// the bytes the device call would allocate for the last cch_plan (with desc), and the check against a limit
double cch_device_bytes(const cba_cov_desc* d) {
  int32_t ncp = 0;
  for (int32_t c = 0; c < d->n_cams; ++c) ncp += d->cam_nparams[c];
  return cov_con_device_bytes(d, ncp, g_plan);
}
int cch_memory_check(double need, double limit) { return cov_con_memory_check(need, limit, g_error); }

}
