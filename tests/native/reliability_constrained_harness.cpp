// CPU harness around caliscope_amd/csrc/reliability_constraint_math.h — TEST INFRASTRUCTURE (built by g++ in tests/reliability_constrained_native.py).
// cba_observation_reliability_constrained on the host: everything up to C = St^-1 is the host replay of the pipeline (covariance_replay.h, as it
// is, with the canonical order of a point's observations and the plan of the constraint rows), the steps behind it are
// reliability_constrained_replay.h.  Without a row of positive weight it is the unconstrained call: seven gauge columns, no plan.  The non-GPU
// suite checks the whole call against the dense projector with it and drives CaptureVolume.observation_reliability(include_constraints=True)
// through its `_solver` hook.  It is not a CPU fallback: nothing in caliscope_amd/ loads it.
#include <cstdint>
#include <string>

#include "reliability_constrained_replay.h"

using namespace cba;

namespace {
std::string g_error;
}

extern "C" {

const char* rch_last_error() { return g_error.c_str(); }

// cba_observation_reliability_constrained on the host: 0 or a CBA_ERR_* with rch_last_error() set; gauge_out: 6 or 7
int rch_observation_reliability_constrained(const cba_cov_desc* d, const cba_cov_constraints* constraints, cba_rel_out* out, cba_rel_con_out* con_out,
                                            int32_t* gauge_out) {
  const std::string what = "cba_observation_reliability_constrained";
  if (!d) { g_error = what + ": null argument"; return CBA_ERR_INVALID; }
  CovConPlan plan;
  if (d->n_points > 0 && d->n_points <= INT32_MAX) {
    const int rc = cov_con_components(d->n_points, constraints, plan, g_error, what.c_str());
    if (rc) return rc;
  }
  const int64_t n_con = constraints && constraints->n_con > 0 ? constraints->n_con : 0;
  if (gauge_out) *gauge_out = plan.n_rows ? COV_GAUGE_RIGID : COV_GAUGE;
  CovReplay rp;
  if (plan.n_rows == 0) {
    const int rc = cov_replay<COV_GAUGE>(d, nullptr, true, what, g_error, rp);
    return rc ? rc : rel_con_replay(d, nullptr, rp, what, g_error, out, n_con, con_out);
  }
  const int rc = cov_replay<COV_GAUGE_RIGID>(d, &plan, true, what, g_error, rp);
  return rc ? rc : rel_con_replay(d, &plan, rp, what, g_error, out, n_con, con_out);
}

}
