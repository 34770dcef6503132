// CPU harness of cba_parameter_covariance — TEST INFRASTRUCTURE (built by g++ in tests/covariance_native.py).  The call itself is the host
// replay of the pipeline, covariance_replay.h beside this file (the library's checks, refusal texts and per-element arithmetic of
// caliscope_amd/csrc/covariance_math.h, run serially), with seven gauge columns and no constraint rows; here are the entry point and the small
// probes of covariance_math.h.  The non-GPU suite checks the whole call against an eigenvalue pseudo-inverse with it and drives
// CaptureVolume.parameter_uncertainty through its `_solver` hook.  It is not a CPU fallback: nothing in caliscope_amd/ loads it.
#include <cstdint>
#include <string>

#include "covariance_replay.h"

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
  CovReplay rp;
  const int rc = cov_replay<COV_GAUGE>(d, nullptr, false, what, g_error, rp);
  return rc ? rc : cov_replay_outputs<COV_GAUGE>(d, nullptr, rp, what, g_error, out);
}

}
