// CPU harness around caliscope_amd/csrc/trajectory_skeleton_math.h — TEST INFRASTRUCTURE (built by g++ in
// tests/trajectory_skeleton_native.py).  It evaluates cba_adjust_skeleton with the checks and the routines that skeleton_lib.hip uses: the
// workgroup of k_skel_adjust as one thread of one (skel_adjust_group with t = 0, NT = 1: the same operations in the same order), the
// select of k_skel_length by std::nth_element, its sums lane by lane.  It is not a CPU fallback: nothing in caliscope_amd/ loads it.
// Every pointer of `out` must be given.
#include <cstdint>
#include <string>
#include <vector>

#include "trajectory_skeleton_math.h"

using namespace cba;

namespace {
std::string g_error;
}

extern "C" {

const char* tkh_last_error() { return g_error.c_str(); }

// cba_adjust_skeleton on the host: 0, -1 (invalid) or -4 (unsupported) with tkh_last_error() set
int tkh_adjust_skeleton(const cba_skeleton_desc* d, cba_skeleton_out* o) {
  if (!d || !o) { g_error = "cba_adjust_skeleton: null argument"; return -1; }
  SkelPlan plan;
  bool launch = false;
  const int rc = skel_validate(d, (double)d->memory_limit, plan, g_error, &launch);
  if (rc) return rc;
  skel_nothing(d, plan.n_comp, o);
  if (!launch) return 0;
  for (int64_t s = 0; s < d->n_seg; ++s) skel_length_host(d, s, o->length + s, o->med + s, o->mad + s, o->frames + s);
  const SkelTables T = plan.tables();
  const SkelOut O = {o->pos, o->pos_cov, o->status, o->len_before, o->w_before, o->len_after, o->chi2, o->rows, o->iterations, o->comp_status};
  std::vector<double> lds((size_t)skel_lds_bytes(plan.max_m) / 8 + 1);
  for (int64_t f = 0; f < d->n_frames; ++f)
    for (int32_t k = 0; k < plan.n_comp; ++k)
      skel_adjust_group(0, 1, f, k, plan.n_comp, d->n_traj, d->n_seg, d->xyz, d->meas_cov, d->measured, o->length, d->seg_sigma, d->max_iter, d->tol, T,
                        O, lds.data());
  return 0;
}

}
