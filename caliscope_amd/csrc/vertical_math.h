// Arithmetic, pixel-chunk plan and host-side checks of cba_vertical_fit (include/caliscope_vertical.h): the 2-DOF Levenberg-Marquardt
// fit of a camera's gravity direction to the four perspective fields of a frame (up x/y, up confidence, latitude, latitude
// confidence), the reference's estimators/vertical_solver.py::fit_gravity.  Compiled by hipcc into the kernels of vertical_lib.hip
// and by g++ into tests/native/vertical_harness.cpp, which walks the same chunks, lanes and waves serially on the CPU.
//
// One pass per step.  The reference evaluates its residual / Jacobian routines three times per step; here one pass over the pixels
// at the current gravity vector g gives everything the step needs.  The Jacobian of a pixel's rendered fields with respect to the
// tangent step is A T: A is 2 x 3 for the up field (d normalise(g_xy - g_z uv) / d g) and the pixel ray for the sine of the latitude,
// T the 3 x 2 tangent basis at g.  T does not depend on the pixel, so the pass accumulates in gravity-vector coordinates: the two
// costs, the 3-gradient A^T w r and the six entries of the symmetric 3 x 3 Hessian A^T w A: VERT_NSUM = 11 sums.  The update projects
// them with T^T g and T^T H T (vert_project).  The pass at the new vector gives the new cost (the stop test and the damping update)
// and the next step's system; the pass at the final vector is projected with j_roll_pitch for the uncertainty.
//
// Summation order (fixed, so a fit does not depend on what else is in the batch and two runs agree bit for bit).  The pixels of a
// fit are cut into chunks of VERT_CHUNK_PIXELS, counted from the fit's own first pixel.  Within a chunk thread t of VERT_BLOCK takes
// pixels t, t + VERT_BLOCK, .. in that order; the 64 lanes of a wave are folded with offsets 32, 16, .. 1 (lane l += lane l + offset),
// the waves are added in index order, and the update adds the chunks in index order.
//
// Every clamp and epsilon is the reference's: max(norm, 1e-12) for the normalised up vector, max(norm, 1e-6) inside the Jacobian,
// the sine clipped to +-(1 - 1e-6), Huber on x / scale^2 with sqrt(x + 1e-8), weight floor FLT_EPSILON, loss scales 1e-2, costs as
// means over the pixels, damping max(diag * lambda, 1e-6), every step accepted, lambda x10 / x0.1 clipped to [1e-6, 1e2], stop on
// |dcost| <= 1e-8 + 1e-8 |prev|.  Full-precision divide and square root throughout.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#ifndef CBA_HD
#if defined(__HIPCC__)
#define CBA_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define CBA_HD inline
#endif
#endif

namespace cba {

constexpr int VERT_CHUNK_PIXELS = 4096;  // pixels of one partial workgroup; fixed, so the summation order of a fit is a function of its shape alone
constexpr int VERT_BLOCK = 256;          // threads of a partial workgroup: 16 pixels per thread in a full chunk
constexpr int VERT_WAVE = 64;
constexpr int VERT_NSUM = 11;            // up cost, latitude cost, gradient (3), Hessian 00 01 02 11 12 22
constexpr int VERT_MAX_SIDE = 32768;     // height and width limit: h * w stays below 2^31
constexpr int VERT_MAX_STEPS = 10000;

constexpr double VERT_INITIAL_LAMBDA = 0.1, VERT_LAMBDA_MIN = 1e-6, VERT_LAMBDA_MAX = 1e2;
constexpr double VERT_STOP_ATOL = 1e-8, VERT_STOP_RTOL = 1e-8;
constexpr double VERT_LOSS_SCALE2 = 1e-2 * 1e-2;  // up and latitude loss scale, squared

enum { VERT_OK = 0, VERT_NONFINITE = 1, VERT_SINGULAR = 2 };  // per-fit status

// State of one fit between passes, and its result.  out: roll, pitch, roll / pitch / gravity uncertainty, initial cost, final cost,
// stop_step (as a double).
struct VertState {
  double vec[3];
  double lambda;
  double prev_cost;
  double out[8];
  int32_t done;
  int32_t stop_step;
  int32_t status;
  int32_t pad;
};

CBA_HD int64_t vert_n_chunks(int64_t n_pixels) { return (n_pixels + VERT_CHUNK_PIXELS - 1) / VERT_CHUNK_PIXELS; }

CBA_HD bool vert_finite(double v) { return v - v == 0.0; }

// Huber loss and weight on an already-squared cost, pre-divided by scale^2 and the loss multiplied back.
CBA_HD void vert_scaled_huber(double squared, double& loss, double& weight) {
  const double x = squared / VERT_LOSS_SCALE2;
  const double sqrt_x = sqrt(x + 1e-8);
  const double inv = 1.0 / sqrt_x;
  const bool inlier = x <= 1.0;
  loss = (inlier ? x : 2.0 * sqrt_x - 1.0) * VERT_LOSS_SCALE2;
  weight = inlier ? 1.0 : (inv > (double)FLT_EPSILON ? inv : (double)FLT_EPSILON);
}

// The 11 terms of pixel p (row-major, p = y * width + x) of a height x width frame at gravity vector vec, added to acc.
// tux, tuy: target up vector; cu: its confidence; tsl: sine of the target latitude; cl: its confidence.
CBA_HD void vert_pixel(int32_t height, int32_t width, double fx, double fy, int64_t p, double tux, double tuy, double cu, double tsl, double cl,
                       const double* vec, double* acc) {
  const int64_t py_i = p / width, px_i = p - py_i * width;
  const double u = ((double)px_i - (double)width / 2.0) / fx;
  const double v = ((double)py_i - (double)height / 2.0) / fy;
  const double rn = sqrt(u * u + v * v + 1.0);
  const double rx = u / rn, ry = v / rn, rz = 1.0 / rn;
  const double a = vec[0], b = vec[1], c = vec[2];
  // up field: the image-plane projection of world up, normalised
  const double qx = a - c * u, qy = b - c * v;
  const double n = sqrt(qx * qx + qy * qy);
  const double nn = n > 1e-12 ? n : 1e-12;
  const double ex = tux - qx / nn, ey = tuy - qy / nn;
  // latitude: sine space
  double sl = rx * a + ry * b + rz * c;
  const double lim = 1.0 - 1e-6;
  sl = sl < -lim ? -lim : (sl > lim ? lim : sl);
  const double el = tsl - sl;
  double up_loss, up_w, lat_loss, lat_w;
  vert_scaled_huber(ex * ex + ey * ey, up_loss, up_w);
  vert_scaled_huber(el * el, lat_loss, lat_w);
  acc[0] += up_loss * cu;
  acc[1] += lat_loss * cl;
  up_w *= cu;
  lat_w *= cl;
  // A = d normalise(q) / d q  *  d q / d (a, b, c),  d q / d (a, b, c) = [[1, 0, -u], [0, 1, -v]]
  const double nj = n > 1e-6 ? n : 1e-6;
  const double nj3 = nj * nj * nj;
  const double j00 = 1.0 / nj - qx * qx / nj3, j01 = -(qx * qy) / nj3, j11 = 1.0 / nj - qy * qy / nj3;
  const double a02 = -(j00 * u + j01 * v), a12 = -(j01 * u + j11 * v);
  acc[2] += up_w * (j00 * ex + j01 * ey) + lat_w * rx * el;
  acc[3] += up_w * (j01 * ex + j11 * ey) + lat_w * ry * el;
  acc[4] += up_w * (a02 * ex + a12 * ey) + lat_w * rz * el;
  acc[5] += up_w * (j00 * j00 + j01 * j01) + lat_w * rx * rx;
  acc[6] += up_w * (j00 * j01 + j01 * j11) + lat_w * rx * ry;
  acc[7] += up_w * (j00 * a02 + j01 * a12) + lat_w * rx * rz;
  acc[8] += up_w * (j01 * j01 + j11 * j11) + lat_w * ry * ry;
  acc[9] += up_w * (j01 * a02 + j11 * a12) + lat_w * ry * rz;
  acc[10] += up_w * (a02 * a02 + a12 * a12) + lat_w * rz * rz;
}

// ---- the serial update ------------------------------------------------------------------------------------------------------------

CBA_HD void vert_gravity_vec(double roll, double pitch, double* vec) {
  vec[0] = -sin(roll) * cos(pitch);
  vec[1] = -cos(roll) * cos(pitch);
  vec[2] = sin(pitch);
}

CBA_HD void vert_roll_pitch(const double* vec, double& roll, double& pitch) {
  const double eps = 1e-4;
  const double x = vec[0], y = vec[1], z = vec[2];
  const double zc = z < -1.0 ? -1.0 : (z > 1.0 ? 1.0 : z);
  pitch = asin(zc);
  const double rem = 1.0 - z * z;
  double s = -x / (sqrt(rem > 0.0 ? rem : 0.0) + eps);
  s = s < -1.0 ? -1.0 : (s > 1.0 ? 1.0 : s);
  roll = asin(s);
  if (y >= 0.0) {  // upside-down camera: reflect and offset
    const double sign = x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0);
    roll = -roll - 3.141592653589793 * sign;
  }
}

// v (v[2] = 1) and beta with (I - beta v v^T) x = |x| e_3; last-element pivot
CBA_HD void vert_householder(const double* x, double* v, double& beta, double& norm) {
  double sigma = x[0] * x[0] + x[1] * x[1];
  norm = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  sigma = sigma > 1e-7 ? sigma : 1e-7;
  const double vp = x[2] < 0.0 ? x[2] - norm : -sigma / (x[2] + norm);
  beta = 2.0 * vp * vp / (sigma + vp * vp);
  v[0] = x[0] / vp;
  v[1] = x[1] / vp;
  v[2] = 1.0;
}

// x <- exponential map of the tangent step delta, rotated to x
CBA_HD void vert_spherical_plus(double* x, const double* delta) {
  const double nd = sqrt(delta[0] * delta[0] + delta[1] * delta[1]);
  const double sinc = nd < 1e-7 ? 1.0 : sin(nd) / nd;
  const double e[3] = {sinc * delta[0], sinc * delta[1], cos(nd)};
  double v[3], beta, norm;
  vert_householder(x, v, beta, norm);
  const double k = beta * (v[0] * e[0] + v[1] * e[1] + v[2] * e[2]);
  for (int i = 0; i < 3; ++i) x[i] = norm * (e[i] - v[i] * k);
}

// T[3][2]: the tangent basis at x, the first two columns of the Householder reflection
CBA_HD void vert_spherical_j_plus(const double* x, double T[3][2]) {
  double v[3], beta, norm;
  vert_householder(x, v, beta, norm);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 2; ++j) T[i][j] = (i == j ? 1.0 : 0.0) - beta * v[i] * v[j];
}

// T[3][2]: d vec / d (roll, pitch)
CBA_HD void vert_j_roll_pitch(const double* vec, double T[3][2]) {
  double roll, pitch;
  vert_roll_pitch(vec, roll, pitch);
  const double sr = sin(roll), cr = cos(roll), sp = sin(pitch), cp = cos(pitch);
  T[0][0] = -cr * cp; T[0][1] = sr * sp;
  T[1][0] = sr * cp;  T[1][1] = cr * sp;
  T[2][0] = 0.0;      T[2][1] = cp;
}

// g2 = T^T g, H2 = T^T H T (h00 h01 h11) from the sums in gravity-vector coordinates (s[2..4] gradient, s[5..10] Hessian)
CBA_HD void vert_project(const double* s, const double T[3][2], double* g2, double* h2) {
  const double H[3][3] = {{s[5], s[6], s[7]}, {s[6], s[8], s[9]}, {s[7], s[9], s[10]}};
  double HT[3][2];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 2; ++j) HT[i][j] = H[i][0] * T[0][j] + H[i][1] * T[1][j] + H[i][2] * T[2][j];
  for (int j = 0; j < 2; ++j) g2[j] = T[0][j] * s[2] + T[1][j] * s[3] + T[2][j] * s[4];
  h2[0] = T[0][0] * HT[0][0] + T[1][0] * HT[1][0] + T[2][0] * HT[2][0];
  h2[1] = T[0][0] * HT[0][1] + T[1][0] * HT[1][1] + T[2][0] * HT[2][1];
  h2[2] = T[0][1] * HT[0][1] + T[1][1] * HT[1][1] + T[2][1] * HT[2][1];
}

// [[a00, a01], [a10, a11]] x = b by elimination with row pivoting (the order of a general LU solve); false: a pivot is exactly zero
CBA_HD bool vert_solve2(double a00, double a01, double a10, double a11, double b0, double b1, double& x0, double& x1) {
  if (fabs(a00) < fabs(a10)) {
    double t = a00; a00 = a10; a10 = t;
    t = a01; a01 = a11; a11 = t;
    t = b0; b0 = b1; b1 = t;
  }
  if (a00 == 0.0) return false;
  const double l = a10 / a00;
  const double u11 = a11 - l * a01;
  if (u11 == 0.0) return false;
  x1 = (b1 - l * b0) / u11;
  x0 = (b0 - a01 * x1) / a00;
  return true;
}

CBA_HD void vert_state_init(VertState& st, int32_t num_steps) {
  vert_gravity_vec(0.0, 0.0, st.vec);
  st.lambda = VERT_INITIAL_LAMBDA;
  st.prev_cost = 0.0;
  for (int k = 0; k < 8; ++k) st.out[k] = 0.0;
  st.done = 0;
  st.stop_step = num_steps;
  st.status = VERT_OK;
  st.pad = 0;
}

// The result of a fit from the sums of the pass at its final vector.
CBA_HD void vert_finish(VertState& st, const double* s, double cost) {
  double T[3][2], g2[2], h[3];
  vert_j_roll_pitch(st.vec, T);
  vert_project(s, T, g2, h);
  double c00 = 0.0, c10 = 0.0, c01 = 0.0, c11 = 0.0;
  bool ok = vert_finite(h[0]) && vert_finite(h[1]) && vert_finite(h[2]);
  ok = ok && vert_solve2(h[0], h[1], h[1], h[2], 1.0, 0.0, c00, c10) && vert_solve2(h[0], h[1], h[1], h[2], 0.0, 1.0, c01, c11);
  ok = ok && vert_finite(c00) && vert_finite(c10) && vert_finite(c11);
  st.done = 1;
  st.out[7] = (double)st.stop_step;
  if (!ok) {
    st.status = VERT_SINGULAR;
    return;
  }
  // largest eigenvalue of the symmetric [[c00, c10], [c10, c11]]
  const double half = 0.5 * (c00 - c11);
  const double top = 0.5 * (c00 + c11) + sqrt(half * half + c10 * c10);
  vert_roll_pitch(st.vec, st.out[0], st.out[1]);
  st.out[2] = sqrt(c00 > 0.0 ? c00 : 0.0);
  st.out[3] = sqrt(c11 > 0.0 ? c11 : 0.0);
  st.out[4] = sqrt(top > 0.0 ? top : 0.0);
  st.out[6] = cost;
}

// What follows pass number `pass` (0 .. num_steps) of a fit that is not done: s are the 11 sums over its n_pixels pixels at st.vec.
CBA_HD void vert_update(VertState& st, const double* s, int64_t n_pixels, int32_t pass, int32_t num_steps) {
  const double cost = s[0] / (double)n_pixels + s[1] / (double)n_pixels;
  if (pass == 0) {
    st.out[5] = cost;
    if (!vert_finite(cost)) {
      st.status = VERT_NONFINITE;
      st.done = 1;
      st.out[7] = (double)st.stop_step;
      return;
    }
    st.prev_cost = cost;
  } else {
    double lam = st.lambda * (cost > st.prev_cost ? 10.0 : 0.1);
    st.lambda = lam < VERT_LAMBDA_MIN ? VERT_LAMBDA_MIN : (lam > VERT_LAMBDA_MAX ? VERT_LAMBDA_MAX : lam);
    if (fabs(cost - st.prev_cost) <= VERT_STOP_ATOL + VERT_STOP_RTOL * fabs(st.prev_cost)) {
      st.stop_step = pass < st.stop_step ? pass : st.stop_step;
      vert_finish(st, s, cost);
      return;
    }
    st.prev_cost = cost;
  }
  if (pass >= num_steps) {  // budget reached
    vert_finish(st, s, cost);
    return;
  }
  double T[3][2], g2[2], h[3], delta[2] = {0.0, 0.0};
  vert_spherical_j_plus(st.vec, T);
  vert_project(s, T, g2, h);
  const double d0 = h[0] * st.lambda, d1 = h[2] * st.lambda;
  // NaN goes through like numpy.maximum
  const double damp0 = d0 > 1e-6 || d0 != d0 ? d0 : 1e-6, damp1 = d1 > 1e-6 || d1 != d1 ? d1 : 1e-6;
  if (!vert_solve2(h[0] + damp0, h[1], h[1], h[2] + damp1, g2[0], g2[1], delta[0], delta[1])) delta[0] = delta[1] = 0.0;
  vert_spherical_plus(st.vec, delta);  // every step is accepted
}

// One wave's fold: lane l += lane l + offset for offsets 32 .. 1; the sum ends in lane 0.  The serial form the harness runs.
inline double vert_fold_wave_serial(double* lane) {
  for (int off = VERT_WAVE / 2; off > 0; off >>= 1)
    for (int l = 0; l < off; ++l) lane[l] += lane[l + off];
  return lane[0];
}

}  // namespace cba

// ---- host side: the checks the entry point makes before anything is launched ----------------------------------------------------
#include <string>

namespace cba {

// 0, or the negative code the call returns with `msg` set (-1 CBA_ERR_INVALID)
inline int vert_validate(int32_t n_fits, int32_t num_steps, int64_t n_pixels, const int32_t* height, const int32_t* width, const double* focal_x,
                         const double* focal_y, const int64_t* offset, const void* const* planes, int32_t is_f32, std::string& msg) {
  const std::string what = "cba_vertical_fit: ";
  if (n_fits < 0 || num_steps < 0 || n_pixels < 0) { msg = what + "negative size"; return -1; }
  if (num_steps > VERT_MAX_STEPS) { msg = what + "num_steps " + std::to_string(num_steps) + " above " + std::to_string(VERT_MAX_STEPS); return -1; }
  if (is_f32 != 0 && is_f32 != 1) { msg = what + "is_f32 must be 0 or 1"; return -1; }
  if (n_fits == 0) return 0;
  if (!height || !width || !focal_x || !focal_y || !offset || !planes) { msg = what + "null argument"; return -1; }
  for (int k = 0; k < 5; ++k)
    if (!planes[k]) { msg = what + "null argument"; return -1; }
  for (int32_t f = 0; f < n_fits; ++f) {
    const std::string fit = what + "fit " + std::to_string(f) + ": ";
    if (height[f] < 2 || width[f] < 2 || height[f] > VERT_MAX_SIDE || width[f] > VERT_MAX_SIDE) {
      msg = fit + "shape " + std::to_string(height[f]) + " x " + std::to_string(width[f]) + " outside [2, " + std::to_string(VERT_MAX_SIDE) + "]";
      return -1;
    }
    if (!(focal_x[f] > 0.0) || !(focal_y[f] > 0.0) || !vert_finite(focal_x[f]) || !vert_finite(focal_y[f])) {
      msg = fit + "focal lengths must be positive and finite";
      return -1;
    }
    const int64_t n = (int64_t)height[f] * width[f];
    if (offset[f] < 0 || offset[f] > n_pixels || n > n_pixels - offset[f]) {
      msg = fit + "pixels [" + std::to_string(offset[f]) + ", " + std::to_string(offset[f]) + " + " + std::to_string(n) + ") outside the planes of " +
            std::to_string(n_pixels);
      return -1;
    }
  }
  return 0;
}

}  // namespace cba
