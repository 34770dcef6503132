// Stand-alone program around tests/native/reliability_harness.cpp — TEST INFRASTRUCTURE (built by g++ with
// -fsanitize=address,undefined by tests/test_reliability.py): the whole harness call on one scene with a six-wide and two nine-wide
// cameras, a repeated observation, a robust loss and null outputs, then two calls the host checks refuse and the NaN rule of rel_w.
// Prints what failed and exits 1, or exits 0.
#include <cstdio>
#include <cstdlib>

#include "reliability_harness.cpp"

namespace {
int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) { std::printf("FAILED: %s (%s)\n", what, rh_last_error()); ++failures; }
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
      CamTab t;
      cam_prepare(&cam_x[(size_t)cam * MAX_NC], &cconst[(size_t)cam * CAM_CONST_STRIDE], 0, nparams[(size_t)cam], &t, 0);
      double e[2];
      project_residual(t, points[3 * p], points[3 * p + 1], points[3 * p + 2], 0.0, 0.0, e);  // e = projection / fx0
      obs_cam.push_back(cam);
      obs_pt.push_back((int32_t)p);
      obs_uv.push_back(e[0] * t.fx0 + 0.6 * (uniform(seed) - 0.5));
      obs_uv.push_back(e[1] * t.fx0 + 0.6 * (uniform(seed) - 0.5));
    }
  const int64_t n_obs = (int64_t)obs_cam.size();
  cba_cov_desc d = {n_cams, n_points, n_obs, model.data(), nparams.data(), cconst.data(), cam_x.data(), points.data(),
                    obs_cam.data(), obs_pt.data(), obs_uv.data(), LOSS_SOFT_L1, 1.0 / 600.0};
  const int ncp = 24;
  std::vector<double> red((size_t)n_obs * 3, -7.0), w((size_t)n_obs * 2, -7.0), f((size_t)n_obs * 2, -7.0);
  double sigma0_sq = 0.0, cost = 0.0;
  int64_t dof = 0, bad = -1;
  cba_rel_out out = {red.data(), w.data(), f.data(), &sigma0_sq, &dof, &cost, &bad};
  expect(rh_observation_reliability(&d, &out) == CBA_OK, "the call succeeds");
  expect(dof == 2 * n_obs - (ncp + 3 * n_points) + 7 && sigma0_sq > 0.0 && cost > 0.0 && bad == 0, "dof, sigma0, cost and no uncontrolled row");
  double sum_r = 0.0;
  bool in_range = true, w_ok = true;
  for (int64_t o = 0; o < n_obs; ++o) {
    const double ru = red[(size_t)o * 3], ruv = red[(size_t)o * 3 + 1], rv = red[(size_t)o * 3 + 2];
    sum_r += ru + rv;
    in_range = in_range && ru > -1e-9 && ru < 1.0 + 1e-9 && rv > -1e-9 && rv < 1.0 + 1e-9 && ru * rv - ruv * ruv > -1e-9;
    for (int j = 0; j < 2; ++j)
      w_ok = w_ok && std::fabs(w[(size_t)o * 2 + j] - f[(size_t)o * 2 + j] / std::sqrt(sigma0_sq * red[(size_t)o * 3 + 2 * j])) <= 1e-12 * std::fabs(w[(size_t)o * 2 + j]);
  }
  expect(std::fabs(sum_r - (double)dof) <= 1e-9 * (double)dof, "the redundancy numbers sum to the degrees of freedom");
  expect(in_range, "every block is positive semi-definite with a diagonal in [0, 1]");
  expect(w_ok, "w = f / (sigma0 sqrt(r))");
  cba_rel_out none = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  expect(rh_observation_reliability(&d, &none) == CBA_OK, "every output is optional");
  std::vector<double> kept = red;
  obs_pt[3] = (int32_t)n_points;
  expect(rh_observation_reliability(&d, &out) == CBA_ERR_INVALID, "a point index out of range is refused");
  obs_pt[3] = 0;
  nparams[0] = 7;
  expect(rh_observation_reliability(&d, &out) == CBA_ERR_INVALID, "seven parameters are refused");
  expect(kept == red, "a refused call writes nothing");
  expect(std::isnan(rh_w(1.0, REL_R_TINY, 1.0)) && std::isnan(rh_w(1.0, -0.5, 1.0)) && std::isnan(rh_w(1.0, std::nan(""), 1.0)), "w is NaN for an uncontrolled row");
  expect(rh_w(3.0, 4.0, 0.5) == 6.0 && rh_w(1.0, 0.25, 1.0) == 2.0, "r is clamped to 1 for the square root");
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
