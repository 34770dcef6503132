// Host plan of cba_parameter_covariance_constrained (include/caliscope/uncertainty_constrained.h): the checks of the constraint rows, the
// connected components of the constraint graph and every table the component kernel of covariance_lib.hip walks.  Plain C++ without HIP:
// compiled by hipcc into the library and by g++ into tests/native/covariance_constrained_harness.cpp.
//
// cov_con_components  rows of weight 0 dropped, every index / weight / distance checked (the message names the offender), union-find over
//                     the eight points of every kept row, components ordered by their smallest point, their points ascending, their rows in
//                     the caller's order, the cap on the points of a component.  Deterministic: nothing depends on addresses or hashing.
// cov_con_tables      (after cov_validate has sorted the observations by point) per component the cameras that see it, ascending, with the
//                     observations of each, and per constrained point the range of (component camera) entries the point pass reads.
// cov_con_device_bytes / cov_con_memory_check   what the call allocates on the device, against what is free there.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <numeric>
#include <string>
#include <vector>

#include "chol_schedule.h"
#include "covariance_math.h"
#include "../../include/caliscope/uncertainty_constrained.h"

namespace cba {

struct CovConPlan {
  int64_t n_rows = 0;               // kept rows (weight > 0)
  int64_t n_caller = 0;             // the caller's rows (n_con)
  int32_t n_comp = 0;               // components with at least one row
  int32_t max_m = 0;                // points of the largest component
  std::vector<int64_t> row_src;     // [n_rows] the caller's row, grouped by component
  std::vector<int32_t> row_pt;      // [n_rows][8] points (a then b)
  std::vector<int32_t> row_loc;     // [n_rows][8] their positions in the component's point list
  std::vector<double> row_dist, row_weight;  // [n_rows]
  std::vector<int64_t> comp_row;    // [n_comp + 1] rows of a component
  std::vector<int64_t> comp_pt;     // [n_comp + 1] into pts
  std::vector<int32_t> pts;         // the components' points, ascending within a component
  std::vector<uint8_t> in_row;      // [n_points] 1: some kept row names the point
  std::vector<int32_t> free_pts;    // points in no row, ascending (the per-point kernels take these)
  // cov_con_tables
  std::vector<int64_t> comp_cam;    // [n_comp + 1] into cams
  std::vector<int32_t> cams;        // cameras that see a component, ascending within it
  std::vector<int64_t> cc_obs;      // [cams.size() + 1] observations of a (component, camera), into obs_pos / obs_loc
  std::vector<int64_t> obs_pos;     // position in the point-sorted observation table
  std::vector<int32_t> obs_loc;     // the observation's point as a position in the component's point list
  std::vector<int64_t> entry_start; // [n_points + 1] a constrained point has one entry per camera of its component, a free point none
  std::vector<int32_t> entry_cam;   // [entries] the camera of an entry
  int64_t n_entries() const { return entry_start.empty() ? 0 : entry_start.back(); }
};

// CBA_DETERMINISTIC as cov_pipeline reads it
inline bool cov_fixed_order_requested() {
  const char* e = std::getenv("CBA_DETERMINISTIC");
  return e && e[0] != '\0' && !(e[0] == '0' && e[1] == '\0');
}

// The refusals only a call with constraint rows knows (the others: cov_msg_* of covariance_math.h), each text once
inline std::string cov_con_msg_fixed_order(const std::string& what) {
  return what + ": CBA_DETERMINISTIC=1 with constraint rows: the fixed-order sums are not built for the component kernel";
}
inline std::string cov_con_msg_component(const std::string& what, int64_t first_point) {
  return what + ": the constraint component of point " + std::to_string(first_point) + ": its observations and rows do not determine its points (no positive pivot)";
}

// 0 or a CBA_ERR_* with `msg` naming the offender.  plan.n_rows == 0 afterwards: the call is the unconstrained one.
inline int cov_con_components(int64_t n_points, const cba_cov_constraints* con, CovConPlan& plan, std::string& msg,
                              const char* call = "cba_parameter_covariance_constrained", int cap = COV_COMPONENT_CAP) {
  const std::string what = std::string(call) + ": ";
  auto fail = [&](int code, const std::string& m) { msg = what + m; return code; };
  plan = CovConPlan();
  plan.in_row.assign((size_t)(n_points > 0 ? n_points : 0), 0);
  if (!con || con->n_con == 0) return CBA_OK;
  if (con->n_con < 0) return fail(CBA_ERR_INVALID, "n_con must not be negative, got " + std::to_string(con->n_con));
  if (!con->groups_a || !con->groups_b || !con->distances || !con->weights) return fail(CBA_ERR_INVALID, "null constraint array");
  plan.n_caller = con->n_con;
  std::vector<int64_t> kept;
  for (int64_t r = 0; r < con->n_con; ++r) {
    const double w = con->weights[r], dd = con->distances[r];
    if (!std::isfinite(w) || w < 0.0) return fail(CBA_ERR_INVALID, "constraint row " + std::to_string(r) + ": weight " + std::to_string(w) + " is not finite or is negative");
    if (!std::isfinite(dd) || dd < 0.0) return fail(CBA_ERR_INVALID, "constraint row " + std::to_string(r) + ": distance " + std::to_string(dd) + " is not finite or is negative");
    for (int s = 0; s < 8; ++s) {
      const int32_t p = s < 4 ? con->groups_a[4 * r + s] : con->groups_b[4 * r + s - 4];
      if (p < 0 || p >= n_points)
        return fail(CBA_ERR_INVALID, "constraint row " + std::to_string(r) + ": point index " + std::to_string(p) + " out of range (groups_" + (s < 4 ? "a" : "b") + ")");
    }
    if (w > 0.0) kept.push_back(r);
  }
  if (kept.empty()) return CBA_OK;
  // union-find; the root of a set is its smallest point, so that a component is known by its first point
  std::vector<int32_t> parent((size_t)n_points);
  std::iota(parent.begin(), parent.end(), 0);
  auto find = [&](int32_t p) {
    while (parent[(size_t)p] != p) { parent[(size_t)p] = parent[(size_t)parent[(size_t)p]]; p = parent[(size_t)p]; }
    return p;
  };
  auto point_of = [&](int64_t r, int s) { return s < 4 ? con->groups_a[4 * r + s] : con->groups_b[4 * r + s - 4]; };
  for (int64_t r : kept) {
    for (int s = 0; s < 8; ++s) plan.in_row[(size_t)point_of(r, s)] = 1;
    int32_t root = find(point_of(r, 0));
    for (int s = 1; s < 8; ++s) {
      const int32_t other = find(point_of(r, s));
      if (other == root) continue;
      if (other < root) { parent[(size_t)root] = other; root = other; } else parent[(size_t)other] = root;
    }
  }
  // components in the order of their smallest point; points ascending
  std::vector<int32_t> comp_of((size_t)n_points, -1), local((size_t)n_points, -1);
  std::vector<int32_t> count;
  for (int32_t p = 0; p < n_points; ++p) {
    if (!plan.in_row[(size_t)p]) { plan.free_pts.push_back(p); continue; }
    const int32_t root = find(p);
    if (comp_of[(size_t)root] < 0) { comp_of[(size_t)root] = (int32_t)count.size(); count.push_back(0); }  // (root == p here: the smallest comes first)
    comp_of[(size_t)p] = comp_of[(size_t)root];
    local[(size_t)p] = count[(size_t)comp_of[(size_t)p]]++;
  }
  plan.n_comp = (int32_t)count.size();
  plan.comp_pt.assign((size_t)plan.n_comp + 1, 0);
  for (int32_t k = 0; k < plan.n_comp; ++k) plan.comp_pt[(size_t)k + 1] = plan.comp_pt[(size_t)k] + count[(size_t)k];
  plan.pts.resize((size_t)plan.comp_pt.back());
  for (int32_t p = 0; p < n_points; ++p)
    if (plan.in_row[(size_t)p]) plan.pts[(size_t)(plan.comp_pt[(size_t)comp_of[(size_t)p]] + local[(size_t)p])] = p;
  for (int32_t k = 0; k < plan.n_comp; ++k) {
    if (count[(size_t)k] > cap)
      return fail(CBA_ERR_UNSUPPORTED, "the constraint component of point " + std::to_string(plan.pts[(size_t)plan.comp_pt[(size_t)k]]) + " has " +
                                           std::to_string(count[(size_t)k]) + " points: a component holds at most " + std::to_string(cap));
    plan.max_m = std::max(plan.max_m, count[(size_t)k]);
  }
  // rows grouped by component, in the caller's order within one
  plan.comp_row.assign((size_t)plan.n_comp + 1, 0);
  for (int64_t r : kept) ++plan.comp_row[(size_t)comp_of[(size_t)point_of(r, 0)] + 1];
  for (int32_t k = 0; k < plan.n_comp; ++k) plan.comp_row[(size_t)k + 1] += plan.comp_row[(size_t)k];
  plan.n_rows = (int64_t)kept.size();
  plan.row_src.resize(kept.size()); plan.row_pt.resize(kept.size() * 8); plan.row_loc.resize(kept.size() * 8);
  plan.row_dist.resize(kept.size()); plan.row_weight.resize(kept.size());
  std::vector<int64_t> next(plan.comp_row.begin(), plan.comp_row.end() - 1);
  for (int64_t r : kept) {
    const size_t at = (size_t)next[(size_t)comp_of[(size_t)point_of(r, 0)]]++;
    plan.row_src[at] = r; plan.row_dist[at] = con->distances[r]; plan.row_weight[at] = con->weights[r];
    for (int s = 0; s < 8; ++s) { plan.row_pt[at * 8 + s] = point_of(r, s); plan.row_loc[at * 8 + s] = local[(size_t)point_of(r, s)]; }
  }
  return CBA_OK;
}

// The cameras and observations of every component and the entries of the point pass.  `order`, `pt_start`: the point-sorted
// observation table of cov_validate; obs_cam: the caller's.
inline void cov_con_tables(const CovPlan& cov, const int32_t* obs_cam, int32_t n_cams, int64_t n_points, CovConPlan& plan) {
  plan.comp_cam.assign((size_t)plan.n_comp + 1, 0);
  plan.cams.clear(); plan.cc_obs.assign(1, 0); plan.obs_pos.clear(); plan.obs_loc.clear();
  plan.entry_start.assign((size_t)n_points + 1, 0);
  std::vector<int64_t> per_cam((size_t)n_cams), slot((size_t)n_cams);
  for (int32_t k = 0; k < plan.n_comp; ++k) {
    std::fill(per_cam.begin(), per_cam.end(), 0);
    const int64_t p0 = plan.comp_pt[(size_t)k], p1 = plan.comp_pt[(size_t)k + 1];
    for (int64_t i = p0; i < p1; ++i)
      for (int64_t a = cov.pt_start[(size_t)plan.pts[(size_t)i]]; a < cov.pt_start[(size_t)plan.pts[(size_t)i] + 1]; ++a) ++per_cam[(size_t)obs_cam[cov.order[(size_t)a]]];
    int64_t at = (int64_t)plan.obs_pos.size();
    int32_t n_seen = 0;
    for (int32_t c = 0; c < n_cams; ++c) {
      if (!per_cam[(size_t)c]) continue;
      plan.cams.push_back(c);
      slot[(size_t)c] = at;
      at += per_cam[(size_t)c];
      plan.cc_obs.push_back(at);
      ++n_seen;
    }
    plan.comp_cam[(size_t)k + 1] = (int64_t)plan.cams.size();
    plan.obs_pos.resize((size_t)at); plan.obs_loc.resize((size_t)at);
    for (int64_t i = p0; i < p1; ++i) {  // points ascending, a point's observations in sorted order: a fixed order within a camera
      const int32_t p = plan.pts[(size_t)i];
      for (int64_t a = cov.pt_start[(size_t)p]; a < cov.pt_start[(size_t)p + 1]; ++a) {
        const size_t dst = (size_t)slot[(size_t)obs_cam[cov.order[(size_t)a]]]++;
        plan.obs_pos[dst] = a; plan.obs_loc[dst] = (int32_t)(i - p0);
      }
      plan.entry_start[(size_t)p + 1] = n_seen;
    }
  }
  for (int64_t p = 0; p < n_points; ++p) plan.entry_start[(size_t)p + 1] += plan.entry_start[(size_t)p];
  plan.entry_cam.resize((size_t)plan.entry_start.back());
  for (int32_t k = 0; k < plan.n_comp; ++k)
    for (int64_t i = plan.comp_pt[(size_t)k]; i < plan.comp_pt[(size_t)k + 1]; ++i) {
      const int64_t e0 = plan.entry_start[(size_t)plan.pts[(size_t)i]];
      for (int64_t q = plan.comp_cam[(size_t)k]; q < plan.comp_cam[(size_t)k + 1]; ++q) plan.entry_cam[(size_t)(e0 + q - plan.comp_cam[(size_t)k])] = plan.cams[(size_t)q];
    }
}

// doubles of LDS the component kernel asks for with components of at most max_m points: the packed triangle, two n x 9 panels, Z (n x 6),
// a saved column and the starting diagonal
inline size_t cov_con_lds_doubles(int max_m) {
  const size_t n = 3 * (size_t)max_m;
  return n * (n + 1) / 2 + 2 * n * MAX_NC + n * COV_GAUGE_RIGID + 2 * n;
}

// Bytes of device memory the call allocates: the buffers of the unconstrained call (six gauge columns) and the tables and stores of the rows,
// the components and the entries.  As a double: a size beyond 2^63 must still compare.
inline double cov_con_device_bytes(const cba_cov_desc* d, int32_t ncp, const CovConPlan& plan) {
  const double n_cams = d->n_cams, n_obs = (double)d->n_obs, n_points = (double)d->n_points, G = COV_GAUGE_RIGID, NBW = NB;
  const double ldw = std::ceil(ncp / NBW) * NBW, nbk = ldw / NBW;
  double b = 0.0;
  b += n_cams * (4 + 4 + 8 * 12 + 8 * MAX_NC + 8 * 48) + 4;                     // models, offsets, constants, parameters, tables
  b += n_points * (8 * 3 + 8 + 8 * 6 + 8 * 3 * G) + 8;                          // points, pt_start, V^-1, Z
  b += n_obs * (4 + 4 + 8 * 2 + 8 + 8 * 27 + 8 * 6 + 8 * 27 + 4);               // the observation tables, W blocks, B^T B, Y, cameras
  b += 8.0 * ncp * (1 + 1 + G + 1 + ncp) + 8 * G * G;                           // parameter maps, B, the scale, C, D^-1
  b += 8.0 * (2 * (nbk + 1) + 1) * NBW * NBW;                                   // the diagonal-block inverses and side slots of the Cholesky (chol_xinv_blocks)
  b += 8.0 * (n_cams * 81 + (double)ncp * ncp + G * G + 1 + (ldw + 1) * ldw + ldw * ldw + 8);  // the zeroed block
  b += (double)plan.n_rows * (8 * 4 + 8 * 4 + 8 + 8 + 8 * 3 + 8 * 8);           // row points, positions, distances, weights, u, coefficients
  b += (double)(plan.n_comp + 1) * 8 * 3 + (double)plan.pts.size() * 4 * 2 + (double)plan.free_pts.size() * 4;
  b += (double)plan.cams.size() * (4 + 8) + 8 + (double)plan.obs_pos.size() * (8 + 4);
  b += (n_points + 1) * 8 + (double)plan.n_entries() * (4 + 8 * 27);            // entries: camera and Y block
  b += n_points * 8 * 6 + 8.0 * ncp * G;                                        // the point pass: output and E
  return b;
}

// cameras of the component that the most cameras see (cov_con_tables done)
inline int64_t cov_con_max_cams(const CovConPlan& plan) {
  int64_t m = 0;
  for (int32_t k = 0; k < plan.n_comp; ++k) m = std::max(m, plan.comp_cam[(size_t)k + 1] - plan.comp_cam[(size_t)k]);
  return m;
}

// What cba_observation_reliability_constrained allocates on top: s_j, the caller's row and the component of every row, the G store laid out as
// Yc, v (nine doubles per camera of the widest component, per row), seven doubles per observation, three per constraint row of the caller, the counts
inline double cov_con_reliability_bytes(const cba_cov_desc* d, const CovConPlan& plan) {
  return (double)plan.n_rows * (8 + 8 + 4 + 8.0 * 9 * (double)cov_con_max_cams(plan)) + (double)plan.n_entries() * 8 * 27 + (double)d->n_obs * 8 * 7 +
         (double)plan.n_caller * 8 * 3 + 8 * 3;
}

// CBA_OK, or CBA_ERR_UNSUPPORTED with `msg` when the call needs more than `limit` bytes
inline int cov_con_memory_check(double need, double limit, std::string& msg, const char* call = "cba_parameter_covariance_constrained") {
  if (need <= limit) return CBA_OK;
  msg = std::string(call) + ": the call needs " + std::to_string((long long)need) + " bytes of device memory, " + std::to_string((long long)limit) + " are free";
  return CBA_ERR_UNSUPPORTED;
}

}  // namespace cba
