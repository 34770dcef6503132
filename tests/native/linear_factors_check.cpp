// The no-residual form of project_factors (caliscope_amd/csrc/ba_math.h: what k_tprep and k_jv evaluate under a linear loss) against the full
// one — TEST INFRASTRUCTURE, built by g++ in tests/test_linear_factors.py.  G, Yr, Aint and B have to come out bit for bit: pinhole and
// fisheye rows, six and nine parameters, points off and ON the optical axis (the fisheye model's r = 0 branch).
#include <cmath>
#include <cstdio>
#include <cstring>

#include "ba_math.h"

static int failures = 0;

static void check(const char* what, const cba::CamTab& tab, const double* X) {
  double e[2], G[2][3], Yr[3], Aint[2][3], B[2][3];
  double G2[2][3], Yr2[3], Aint2[2][3], B2[2][3];
  std::memset(G2, 0xff, sizeof G2); std::memset(Yr2, 0xff, sizeof Yr2); std::memset(Aint2, 0xff, sizeof Aint2); std::memset(B2, 0xff, sizeof B2);
  cba::project_factors(tab, X[0], X[1], X[2], 321.5, 207.25, e, G, Yr, Aint, B);
  cba::project_factors(tab, X[0], X[1], X[2], G2, Yr2, Aint2, B2);
  const bool same = !std::memcmp(G, G2, sizeof G) && !std::memcmp(Yr, Yr2, sizeof Yr) && !std::memcmp(Aint, Aint2, sizeof Aint) && !std::memcmp(B, B2, sizeof B);
  bool finite = true;
  for (int r = 0; r < 2; ++r)
    for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(G[r][k]) && std::isfinite(B[r][k]) && std::isfinite(Aint[r][k]);
  // (the case must exercise something: a live G, and live intrinsic columns exactly for nine parameters off the axis)
  const bool live = G[0][0] != 0.0 && G[1][1] != 0.0;
  std::printf("%-34s %s\n", what, same && finite && live ? "bit-equal" : "DIFFERENT");
  if (!(same && finite && live)) ++failures;
}

int main() {
  // rotation vector, translation, (scale, k1, k2) of a nine-parameter camera
  const double x_cam[cba::MAX_NC] = {0.31, -0.42, 0.17, 0.05, -0.08, 2.4, 1.013, -0.21, 0.07};
  const double x_small[cba::MAX_NC] = {1e-6, -2e-6, 3e-6, 0.0, 0.0, 2.0, 0.99, 0.02, -0.01};  // (the series branch of cam_prepare)
  const double cc_pin[9] = {905.3, 911.7, 640.2, 355.9, -0.23, 0.09, 0.0011, -0.0007, -0.013};
  const double cc_fish[9] = {512.4, 509.8, 318.1, 242.6, 0.031, -0.012, 0.0042, -0.0009, 0.0};
  const double X_off[3] = {0.37, -0.22, 0.81};
  for (int model = 0; model < 2; ++model)
    for (int np = 6; np <= 9; np += 3) {
      for (int small = 0; small < 2; ++small) {
        cba::CamTab tab;
        cba::cam_prepare(small ? x_small : x_cam, model ? cc_fish : cc_pin, model, np, &tab, 12);
        char name[64];
        std::snprintf(name, sizeof name, "%s np=%d %s", model ? "fisheye" : "pinhole", np, small ? "small-angle" : "general");
        check(name, tab, X_off);
        // a point on the optical axis: X = R^T (0, 0, z) - R^T t, so that x = y = 0 up to rounding; and one exactly there for the identity rotation
        const double z = 1.7, c[3] = {-tab.t[0], -tab.t[1], z - tab.t[2]};
        const double X_axis[3] = {tab.R[0] * c[0] + tab.R[3] * c[1] + tab.R[6] * c[2], tab.R[1] * c[0] + tab.R[4] * c[1] + tab.R[7] * c[2],
                                  tab.R[2] * c[0] + tab.R[5] * c[1] + tab.R[8] * c[2]};
        std::snprintf(name, sizeof name, "%s np=%d %s, axis", model ? "fisheye" : "pinhole", np, small ? "small-angle" : "general");
        check(name, tab, X_axis);
      }
      {
        const double x_id[cba::MAX_NC] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.03, -0.02};
        const double X_exact[3] = {0.0, 0.0, 2.5};
        cba::CamTab tab;
        cba::cam_prepare(x_id, model ? cc_fish : cc_pin, model, np, &tab, 0);
        char name[64];
        std::snprintf(name, sizeof name, "%s np=%d identity, exact axis", model ? "fisheye" : "pinhole", np);
        check(name, tab, X_exact);
      }
    }
  if (failures) { std::printf("%d case(s) failed\n", failures); return 1; }
  std::printf("all checks passed\n");
  return 0;
}
