// The part of cba_parameter_covariance that cba_observation_reliability needs too (covariance_lib.hip defines it, reliability_lib.hip is
// its second caller): the host checks, the uploads, every launch up to C = St^-1 (k_unc_cam .. k_unc_ttt, the header of covariance_lib.hip
// lists them) and the numeric refusals on the way.  `finish` runs while the device buffers of the call are alive and returns the call's
// code; whatever it allocates it owns.  Nothing is written to a caller's array before `finish` does so.  `canonical` is cov_validate's: the
// order of a point's observations in the sorted table (cba_parameter_covariance keeps the input order, as it always has).
// tests/native/covariance_replay.h is this pipeline on the host for the CPU suite (CovReplay mirrors CovPipeline): a step added here is added there.
// cov_pipeline_constrained is the same with the rows of cba_parameter_covariance_constrained (six gauge columns; without a row of positive
// weight it IS cov_pipeline) for cba_observation_reliability_constrained: it also has k_unc_component leave s_j = |X c_j^T|^2 per row and hands
// on the device tables of the rows.  Those steps (s_j, and everything behind C) are replayed in tests/native/reliability_constrained_replay.h.
#pragma once
#include <cstdint>
#include <functional>
#include <vector>

#include "covariance_math.h"
#include "../../include/caliscope/uncertainty_constrained.h"

namespace cba {

struct CovConPlan;  // covariance_constraint_plan.h

struct CovPipeline {
  const CovPlan* plan;  // order, pt_start, cam_off, dof (host)
  int32_t n_cams, ncp;
  int64_t n_obs, n_points;
  // device: the point-ordered observation table and what the kernels left
  const int64_t* order;       // [n_obs] sorted position -> the caller's row
  const int64_t* pt_start;    // [n_points + 1]
  const int32_t* cam_sorted;  // [n_obs] camera of a sorted position
  const int32_t* cam_off;     // [n_cams + 1]
  const double* tab;          // [n_cams] CamTab
  const double* points;       // [n_points][3]
  const double* obs_uv;       // [n_obs][2], the caller's order
  const double* Y;            // [n_obs][27] Y_a = W_a V^-1, sorted order
  const double* Vinv;         // [n_points][6]
  const double* Z;            // [n_points][21]
  const double* C;            // [ncp][ncp] St^-1, both triangles
  // host
  const std::vector<double>* C_host;     // [ncp][ncp]
  const std::vector<double>* B_host;     // [ncp][7]
  const std::vector<double>* Dinv_host;  // [7][7]
  double sigma0_sq, cost;
  // cba_parameter_covariance_constrained (covariance_lib.hip alone reads these; cov_pipeline itself always has gauge = 7, no lists, no entries)
  int gauge;                   // columns of B, D^-1 and of a point's Z: 7, or 6 with constraint rows
  const int32_t* free_list;    // device: the points in no constraint row, or nullptr for "every point"
  int64_t n_free;
  const int32_t* con_list;     // device: the points of the constraint components
  int64_t n_con_pts;
  const int64_t* entry_start;  // device [n_points + 1]: a constrained point's (component camera, Y block) entries
  const int32_t* entry_cam;    // device [entries]
  const double* Yc;            // device [entries][27]
  // cov_pipeline_constrained with rows (reliability_lib.hip reads these; otherwise null / 0): the kept rows, grouped by component
  const CovConPlan* con;       // host plan
  int64_t n_rows;
  const int32_t* row_pt;       // device [n_rows][8]
  const double* row_u;         // device [n_rows][3]
  const double* row_coef;      // device [n_rows][8]
  const double* row_dist;      // device [n_rows]
  const double* row_weight;    // device [n_rows]
  const int64_t* row_src;      // device [n_rows] the caller's row
  const double* row_s;         // device [n_rows] |X c_j^T|^2
  const int64_t* comp_row;     // device [n_comp + 1]
  const int64_t* comp_cam;     // device [n_comp + 1] into cams
  const int32_t* cams;         // device: the cameras that see a component, ascending
};

__attribute__((visibility("hidden"))) int cov_pipeline(const cba_cov_desc* d, int32_t device, const char* what, bool canonical,
                                                       const std::function<int(const CovPipeline&)>& finish);
__attribute__((visibility("hidden"))) int cov_pipeline_constrained(const cba_cov_desc* d, const cba_cov_constraints* constraints, int32_t device, const char* what,
                                                                   bool canonical, const std::function<int(const CovPipeline&)>& finish);

}  // namespace cba
