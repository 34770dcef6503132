// CPU harness around the three routines of caliscope_amd/csrc/ba_math.h behind cba_triangulate (tan_portable, undistort_one, sym4_null_vector), the
// loop of k_triangulate (cba_kernels.h) over a cba_triangulate_desc — TEST INFRASTRUCTURE, built by g++ in
// tests/triangulation_native.py.  g++ does not contract r0 r0' + r1 r1' into fused multiply-adds as hipcc does in k_triangulate: the undistorted
// coordinates equal the device's bit for bit, the points agree to rounding.  It is not a CPU fallback: nothing in caliscope_amd/ loads it.
#include <cstdint>
#include <limits>

#include "../../include/caliscope_ba.h"
#include "ba_math.h"

using namespace cba;

extern "C" {

void th_tan_portable(const double* x, int64_t n, double* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = tan_portable(x[i]);
}

// uv, out: [n][2]; in9: fx fy cx cy d0..d4 of the one camera
void th_undistort(int model, const double* in9, const double* uv, int64_t n, int f32, double* out) {
  for (int64_t i = 0; i < n; ++i) undistort_one(model, in9, uv[2 * i], uv[2 * i + 1], f32, &out[2 * i], &out[2 * i + 1]);
}

// M: [n][4][4] symmetric (left as it is); w: [n][4]
void th_sym4_null_vector(const double* M, int64_t n, double* w) {
  for (int64_t q = 0; q < n; ++q) {
    double A[4][4];
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) A[r][c] = M[16 * q + 4 * r + c];
    sym4_null_vector(A, w + 4 * q);
  }
}

// k_triangulate, one point after the other.  xyz [n_points][3]; und [n_obs][2] or NULL.  The tables are taken as they come (cba_triangulate checks them).
void th_triangulate(const cba_triangulate_desc* d, double* xyz, double* und) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int64_t q = 0; q < d->n_points; ++q) {
    const int64_t a = d->pt_start[q], b = d->pt_start[q + 1];
    double M[4][4] = {};
    for (int64_t i = a; i < b; ++i) {
      const int cam = d->obs_cam[i];
      double x = d->obs_xy[2 * i], y = d->obs_xy[2 * i + 1];
      if (d->cam_intr) undistort_one(d->cam_model[cam], d->cam_intr + 9 * cam, x, y, d->float32_io ? 1 : 0, &x, &y);
      if (und) { und[2 * i] = x; und[2 * i + 1] = y; }
      const double* P = d->cam_P + 12 * cam;
      double r0[4], r1[4];
      for (int c = 0; c < 4; ++c) { r0[c] = x * P[8 + c] - P[c]; r1[c] = y * P[8 + c] - P[4 + c]; }
      for (int r = 0; r < 4; ++r)
        for (int c = r; c < 4; ++c) M[r][c] += r0[r] * r0[c] + r1[r] * r1[c];
    }
    if (b - a < 2) { xyz[3 * q] = xyz[3 * q + 1] = xyz[3 * q + 2] = nan; continue; }
    for (int r = 1; r < 4; ++r)
      for (int c = 0; c < r; ++c) M[r][c] = M[c][r];
    double w[4];
    sym4_null_vector(M, w);
    for (int k = 0; k < 3; ++k) xyz[3 * q + k] = w[k] / w[3];
  }
}

}  // extern "C"
