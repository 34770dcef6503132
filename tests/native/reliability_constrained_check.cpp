// Stand-alone program around tests/native/reliability_constrained_harness.cpp — TEST INFRASTRUCTURE (built by g++ with
// -fsanitize=address,undefined by tests/test_reliability_constrained.py): the whole harness call on the scene of covariance_constrained_check.cpp
// (a six-wide and two nine-wide cameras, five four-point components with corner rows, a centroid row, a row of weight 0 and a row with coincident
// endpoints, five points in no row, a constrained point with a single observation, a repeated observation, soft_l1), with full, partial and null
// outputs; then the call without rows and the calls the host refuses.  The indexing of the three passes there is the indexing of k_rel_point,
// k_rel_con_point and k_rel_con_rows.  Prints what failed and exits 1, or exits 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "reliability_constrained_harness.cpp"

namespace {
int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) { std::printf("FAILED: %s (%s)\n", what, rch_last_error()); ++failures; }
}
double uniform(unsigned& state) {  // a small LCG: the scene must be the same everywhere
  state = state * 1664525u + 1013904223u;
  return (double)(state >> 8) / 16777216.0;
}
}  // namespace

int main() {
  const int32_t n_cams = 3;
  const int64_t n_points = 25;
  unsigned seed = 12345u;
  std::vector<int32_t> model(n_cams, 0), nparams = {6, 9, 9};
  std::vector<double> cconst((size_t)n_cams * CAM_CONST_STRIDE, 0.0), cam_x((size_t)n_cams * MAX_NC, 0.0), points((size_t)n_points * 3);
  for (int32_t c = 0; c < n_cams; ++c) {
    double* k = &cconst[(size_t)c * CAM_CONST_STRIDE];
    k[0] = k[1] = 600.0; k[2] = 640.0; k[3] = 360.0; k[4] = -0.05; k[5] = 0.01;
    double* x = &cam_x[(size_t)c * MAX_NC];
    x[0] = 0.05 * c; x[1] = 0.3 * (c - 1); x[2] = -0.02 * c;  // rvec
    x[3] = -0.8 * (c - 1); x[4] = 0.1 * c; x[5] = 3.0 + 0.4 * c;  // tvec
    x[6] = 1.0; x[7] = -0.05; x[8] = 0.01;
  }
  for (double& v : points) v = 1.6 * uniform(seed) - 0.8;
  std::vector<int32_t> obs_cam, obs_pt;
  std::vector<double> obs_uv;
  for (int64_t p = 0; p < n_points; ++p)
    for (int32_t c = 0; c < n_cams + 1; ++c) {  // the last round observes camera 0 again: a repeated (camera, point) pair
      const int32_t cam = c % n_cams;
      if (c == n_cams && p % 5) continue;
      if (p == 6 && c > 0) continue;  // point 6 (in a component) keeps one observation
      CamTab t;
      cam_prepare(&cam_x[(size_t)cam * MAX_NC], &cconst[(size_t)cam * CAM_CONST_STRIDE], 0, nparams[(size_t)cam], &t, 0);
      double e[2];
      project_residual(t, points[3 * p], points[3 * p + 1], points[3 * p + 2], 0.0, 0.0, e);  // e = projection / fx0
      obs_cam.push_back(cam);
      obs_pt.push_back((int32_t)p);
      obs_uv.push_back(e[0] * t.fx0 + 0.6 * (uniform(seed) - 0.5));
      obs_uv.push_back(e[1] * t.fx0 + 0.6 * (uniform(seed) - 0.5));
    }
  // components {4k .. 4k + 3}, k = 0 .. 4, given from the last to the first; points 20 .. 24 in no row
  std::vector<int32_t> ga, gb;
  std::vector<double> dist, weight;
  auto row = [&](std::initializer_list<int32_t> a, std::initializer_list<int32_t> b, double w) {
    ga.insert(ga.end(), a); gb.insert(gb.end(), b);
    double ma[3] = {0, 0, 0}, mb[3] = {0, 0, 0};
    for (int32_t p : a) for (int k = 0; k < 3; ++k) ma[k] += 0.25 * points[3 * (size_t)p + k];
    for (int32_t p : b) for (int k = 0; k < 3; ++k) mb[k] += 0.25 * points[3 * (size_t)p + k];
    dist.push_back(std::sqrt((ma[0] - mb[0]) * (ma[0] - mb[0]) + (ma[1] - mb[1]) * (ma[1] - mb[1]) + (ma[2] - mb[2]) * (ma[2] - mb[2])) + 0.004);
    weight.push_back(w);
  };
  for (int32_t k = 4; k >= 0; --k) {
    const int32_t p = 4 * k;
    for (int32_t i = 0; i < 4; ++i)
      for (int32_t j = i + 1; j < 4; ++j) row({p + i, p + i, p + i, p + i}, {p + j, p + j, p + j, p + j}, 0.8);
    row({p, p + 1, p + 2, p + 3}, {p + 3, p + 3, p + 3, p + 3}, 0.5);   // centroid against a corner
    row({p, p + 1, p + 2, p + 3}, {p + 3, p + 2, p + 1, p}, 0.5);       // the same cell on both ends: a zero Jacobian row
    row({p, p, p, p}, {20, 20, 20, 20}, 0.0);                           // weight 0: dropped, point 20 stays free
  }
  const int64_t n_obs = (int64_t)obs_cam.size(), n_con = (int64_t)dist.size();
  cba_cov_desc d = {n_cams, n_points, n_obs, model.data(), nparams.data(), cconst.data(), cam_x.data(), points.data(),
                    obs_cam.data(), obs_pt.data(), obs_uv.data(), LOSS_SOFT_L1, 1.0 / 600.0};
  cba_cov_constraints con = {(int32_t)n_con, ga.data(), gb.data(), dist.data(), weight.data()};
  const int ncp = 24;
  std::vector<double> red((size_t)n_obs * 3), w((size_t)n_obs * 2), f((size_t)n_obs * 2), cr((size_t)n_con), cw((size_t)n_con), cf((size_t)n_con);
  double sigma0_sq = 0.0, cost = 0.0;
  int64_t dof = 0, bad = -1, bad_con = -1;
  int32_t gauge = 0;
  cba_rel_out out = {red.data(), w.data(), f.data(), &sigma0_sq, &dof, &cost, &bad};
  cba_rel_con_out con_out = {cr.data(), cw.data(), cf.data(), &bad_con};
  expect(rch_observation_reliability_constrained(&d, &con, &out, &con_out, &gauge) == CBA_OK, "the call succeeds");
  expect(gauge == 6 && dof == 2 * n_obs + 40 - (ncp + 3 * n_points) + 6 && sigma0_sq > 0.0 && cost > 0.0 && bad == 0 && bad_con == 0, "gauge, dof, sigma0, cost, counts");
  double sum = 0.0;
  bool in_range = true, nan_rows = true, unit_rows = true;
  for (int64_t o = 0; o < n_obs; ++o) {
    sum += red[(size_t)o * 3] + red[(size_t)o * 3 + 2];
    in_range = in_range && red[(size_t)o * 3] > 0.0 && red[(size_t)o * 3] < 1.0 && red[(size_t)o * 3 + 2] > 0.0 && red[(size_t)o * 3 + 2] < 1.0 && std::isfinite(w[(size_t)o * 2]);
  }
  for (int64_t j = 0; j < n_con; ++j) {
    if (weight[(size_t)j] == 0.0) { nan_rows = nan_rows && std::isnan(cr[(size_t)j]) && std::isnan(cw[(size_t)j]) && std::isnan(cf[(size_t)j]); continue; }
    sum += cr[(size_t)j];
    in_range = in_range && cr[(size_t)j] > 0.0 && cr[(size_t)j] <= 1.0 && std::isfinite(cw[(size_t)j]);
    if (j % 9 == 7) unit_rows = unit_rows && cr[(size_t)j] == 1.0;  // the zero Jacobian row of every component
  }
  expect(std::fabs(sum - (double)dof) <= 1e-9 * (double)dof, "the redundancy numbers of all rows sum to dof");
  expect(in_range, "every r lies in (0, 1], that of the observation of the point seen once too, and every w is finite");
  expect(nan_rows, "a row of weight 0 is NaN in all three arrays");
  expect(unit_rows, "a row with coincident endpoints has r == 1");
  cba_rel_out some = {nullptr, w.data(), nullptr, nullptr, &dof, nullptr, nullptr};
  cba_rel_con_out con_some = {nullptr, nullptr, cf.data(), nullptr};
  expect(rch_observation_reliability_constrained(&d, &con, &some, &con_some, nullptr) == CBA_OK, "every output is optional");
  expect(rch_observation_reliability_constrained(&d, &con, nullptr, nullptr, nullptr) == CBA_OK, "both structures are optional");
  expect(rch_observation_reliability_constrained(&d, nullptr, &out, &con_out, &gauge) == CBA_ERR_INVALID && gauge == 7, "without rows point 6 has one observation: refused");
  ga[5] = (int32_t)n_points;
  expect(rch_observation_reliability_constrained(&d, &con, &out, &con_out, &gauge) == CBA_ERR_INVALID, "a group index out of range is refused");
  ga[5] = 16;
  weight[2] = -1.0;
  expect(rch_observation_reliability_constrained(&d, &con, &out, &con_out, &gauge) == CBA_ERR_INVALID, "a negative weight is refused");
  weight[2] = 0.8;
  obs_pt[3] = (int32_t)n_points;
  expect(rch_observation_reliability_constrained(&d, &con, &out, &con_out, &gauge) == CBA_ERR_INVALID, "a point index out of range is refused");
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
