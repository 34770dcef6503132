// Per-view camera-from-board pose (PnP) and two-view stereo reprojection error: the arithmetic of the pose bootstrap
// (caliscope_amd/pose_network.py), host + device inline functions.  hipcc compiles it into the kernels of pose_lib.hip
// (one thread per view, one workgroup per camera pair); g++ compiles it into tests/native/pnp_harness.cpp.
//
// One view = n object points X_i (obj_loc, NaN z read as 0) and their undistorted normalised image points u_i (K = I).
// With f32 set both are rounded to float32 first, as the float32 cv2 calls of the reference see them.
//
//   planar      max(z) - min(z) < 1e-6, needs min_points (>= 4 for the homography)
//               1. centre + scale object and image points, homography by DLT with h33 = 1 (8 x 8 normal equations)
//               2. the two IPPE rotations at the board centre (Collins & Bartoli, IJCV 2014): with v the image ray of the
//                  centre, Rv a rotation taking e_z to v, J the homography's 2 x 2 Jacobian there and B = [I2 | -v_xy],
//                  (B Rv)_{:,:2} R~_{:2,:2} = t_z J, so R~_{:2,:2} = A / sigma_max(A) with A = (B Rv)_{:,:2}^{-1} J; the third
//                  row of R~'s first two columns is fixed up to one common sign: those are the two candidates, R = Rv R~
//               3. t of each candidate by linear least squares (3 x 3), then both refined; the lower cost is kept
//   non-planar  needs max(min_points, 6)
//               1. DLT on centred, scaled object points with P34 = 1 (the centroid depth fixed: 11 x 11 normal equations)
//               2. the 3 x 3 block projected onto SO(3) (scaled Newton iteration of the polar factor, sign so that
//                  det > 0), t = p4 / scale
//               3. refined
//   refinement  Levenberg-Marquardt on the normalised reprojection error, left axis-angle increment R <- exp(w) R,
//               t <- t + dt, Marquardt damping mu diag(J^T J), 6 x 6 Cholesky.  Stopping rule: an accepted step with
//               |dw|_inf <= 1e-13 and |dt|_inf <= 1e-13 (1 + |t|_inf), or the damping exceeds 1e16 (no step lowers the
//               cost at this precision), or PNP_LM_MAX_ITER iterations (accepted or not); then at most PNP_POLISH_ITER undamped
//               Gauss-Newton steps while each is less than half the one before (the cost cannot resolve the last ~sqrt(eps)).
//
// Result: R (row-major), t, rmse = sqrt(mean |u_i - proj(R X_i + t)|^2) at the final pose, status PNP_OK / PNP_TOO_FEW /
// PNP_FAILED (singular normal equations, collinear points, degenerate homography Jacobian, non-finite result).  A view
// that is not PNP_OK returns R = I, t = 0, rmse = 0: no NaN leaves this file.
//
// Only small solves: packed Cholesky of 3, 6, 8 and 11 unknowns, fully unrolled (compile-time indices), so that the
// device build keeps every matrix in registers and needs no scratch (pose_lib.hip: -Rpass-analysis=kernel-resource-usage).
#pragma once
#include "ba_math.h"

// No fused multiply-add contraction in this file: the device then rounds as the g++ build does (x86-64 without -mfma), so the
// kernel and tests/native/pnp_harness.cpp take the same path through the iterations.
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace cba {

constexpr int PNP_OK = 0;
constexpr int PNP_TOO_FEW = 1;
constexpr int PNP_FAILED = 2;
constexpr int PNP_LM_MAX_ITER = 60;
constexpr int PNP_POLISH_ITER = 6;
constexpr double PNP_PLANAR_TOL = 1e-6;

// In-place Cholesky solve of a symmetric positive definite N x N system, A packed lower (row r: entries (r, 0..r) at
// r (r + 1) / 2), b -> x.  False when a pivot is not safely positive (relative to its diagonal).
template <int N>
CBA_HD bool chol_solve(double* A, double* b) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const int jj = j * (j + 1) / 2;
    double d = A[jj + j];
    const double d0 = d;
#pragma unroll
    for (int k = 0; k < j; ++k) d -= A[jj + k] * A[jj + k];
    if (!(d > 1e-13 * d0) || !(d0 > 0.0)) return false;
    const double inv = 1.0 / sqrt(d);
    A[jj + j] = inv;  // reciprocal diagonal
#pragma unroll
    for (int i = j + 1; i < N; ++i) {
      const int ii = i * (i + 1) / 2;
      double s = A[ii + j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= A[ii + k] * A[jj + k];
      A[ii + j] = s * inv;
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {  // L y = b
    const int ii = i * (i + 1) / 2;
    double s = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= A[ii + k] * b[k];
    b[i] = s * A[ii + i];
  }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {  // L^T x = y
    double s = b[i];
#pragma unroll
    for (int k = i + 1; k < N; ++k) s -= A[k * (k + 1) / 2 + i] * b[k];
    b[i] = s * A[i * (i + 1) / 2 + i];
  }
  return true;
}

// A += w r r^T (packed lower), b += w r y
template <int N>
CBA_HD void normal_add(double* A, double* b, const double* r, double y) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int k = 0; k <= i; ++k) A[i * (i + 1) / 2 + k] += r[i] * r[k];
    b[i] += r[i] * y;
  }
}

// finite <=> exponent bits not all set (a bit test: `v - v == 0` is not one once the compiler fuses it with the product that made v)
CBA_HD bool pnp_finite(double v) {
  uint64_t b;
  __builtin_memcpy(&b, &v, sizeof b);
  return ((b >> 52) & 0x7ff) != 0x7ff;
}

// One view's point i, rounded to float32 when f32: object point (NaN z -> 0) and normalised image point.
CBA_HD void pnp_load(const double* obj, const double* uv, int i, int f32, double* X, double* u) {
  X[0] = obj[3 * i];
  X[1] = obj[3 * i + 1];
  const double z = obj[3 * i + 2];
  X[2] = (z == z) ? z : 0.0;
  u[0] = uv[2 * i];
  u[1] = uv[2 * i + 1];
  if (f32) {
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = (double)(float)X[k];
    u[0] = (double)(float)u[0];
    u[1] = (double)(float)u[1];
  }
}

// E = exp([w]x) (Rodrigues, series near 0)
CBA_HD void rot_exp(const double* w, double* E) {
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double s, c;  // sin(th)/th, (1 - cos(th))/th^2
  if (th2 < 1e-8) {
    s = 1.0 - th2 / 6.0 + th2 * th2 / 120.0;
    c = 0.5 - th2 / 24.0 + th2 * th2 / 720.0;
  } else {
    const double th = sqrt(th2);
    s = sin(th) / th;
    c = (1.0 - cos(th)) / th2;
  }
  E[0] = 1.0 - c * (w[1] * w[1] + w[2] * w[2]); E[1] = -s * w[2] + c * w[0] * w[1];      E[2] = s * w[1] + c * w[0] * w[2];
  E[3] = s * w[2] + c * w[0] * w[1];      E[4] = 1.0 - c * (w[0] * w[0] + w[2] * w[2]); E[5] = -s * w[0] + c * w[1] * w[2];
  E[6] = -s * w[1] + c * w[0] * w[2];     E[7] = s * w[0] + c * w[1] * w[2];      E[8] = 1.0 - c * (w[0] * w[0] + w[1] * w[1]);
}

CBA_HD void mat3_mul(const double* A, const double* B, double* C) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}

// cost = sum |u - proj(R (X - c) + t)|^2 over the view; with want_normal also J^T J (packed 6 x 6) and J^T r
// (parameters: left rotation increment w, then t).  Non-finite cost when a point projects from depth 0.
template <bool want_normal>
CBA_HD double pnp_cost(const double* obj, const double* uv, int n, int f32, const double* cen, const double* R, const double* t,
                       double* JtJ, double* Jtr) {
  if (want_normal) {
#pragma unroll
    for (int k = 0; k < 21; ++k) JtJ[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) Jtr[k] = 0.0;
  }
  double cost = 0.0;
  for (int i = 0; i < n; ++i) {
    double X[3], u[2];
    pnp_load(obj, uv, i, f32, X, u);
    X[0] -= cen[0]; X[1] -= cen[1]; X[2] -= cen[2];
    const double a0 = R[0] * X[0] + R[1] * X[1] + R[2] * X[2];
    const double a1 = R[3] * X[0] + R[4] * X[1] + R[5] * X[2];
    const double a2 = R[6] * X[0] + R[7] * X[1] + R[8] * X[2];
    const double x = a0 + t[0], y = a1 + t[1], z = a2 + t[2];
    const double iz = 1.0 / z;
    const double px = x * iz, py = y * iz;
    const double rx = px - u[0], ry = py - u[1];
    cost += rx * rx + ry * ry;
    if (want_normal) {
      // d(px, py)/d(x, y, z) = iz [1 0 -px; 0 1 -py];  d(x, y, z)/dw = -[a]x ;  d/dt = I
      double jx[6], jy[6];
      // -[a]x = [0 a2 -a1; -a2 0 a0; a1 -a0 0]
      jx[0] = iz * (-px * a1);           jy[0] = iz * (-a2 - py * a1);
      jx[1] = iz * (a2 + px * a0);       jy[1] = iz * (py * a0);
      jx[2] = iz * (-a1);                jy[2] = iz * (a0);
      jx[3] = iz;                        jy[3] = 0.0;
      jx[4] = 0.0;                       jy[4] = iz;
      jx[5] = -iz * px;                  jy[5] = -iz * py;
#pragma unroll
      for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = 0; c <= r; ++c) JtJ[r * (r + 1) / 2 + c] += jx[r] * jx[c] + jy[r] * jy[c];
        Jtr[r] += jx[r] * rx + jy[r] * ry;
      }
    }
  }
  return cost;
}

// Levenberg-Marquardt from (R, t) (pose of the centred object); returns the final cost (non-finite: failed).
CBA_HD double pnp_refine(const double* obj, const double* uv, int n, int f32, const double* cen, double* R, double* t) {
  double JtJ[21], Jtr[6];
  double cost = pnp_cost<true>(obj, uv, n, f32, cen, R, t, JtJ, Jtr);
  if (!pnp_finite(cost)) return cost;
  double mu = 1e-3;
  for (int it = 0; it < PNP_LM_MAX_ITER; ++it) {
    double A[21], d[6];
    double dmax = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) dmax = fmax(dmax, JtJ[k * (k + 1) / 2 + k]);
#pragma unroll
    for (int k = 0; k < 21; ++k) A[k] = JtJ[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      A[k * (k + 1) / 2 + k] += mu * fmax(JtJ[k * (k + 1) / 2 + k], 1e-12 * dmax);
      d[k] = -Jtr[k];
    }
    bool ok = chol_solve<6>(A, d);
    if (ok) {
      double E[9], Rn[9], tn[3];
      rot_exp(d, E);
      mat3_mul(E, R, Rn);
      tn[0] = t[0] + d[3]; tn[1] = t[1] + d[4]; tn[2] = t[2] + d[5];
      double JtJn[21], Jtrn[6];
      const double cn = pnp_cost<true>(obj, uv, n, f32, cen, Rn, tn, JtJn, Jtrn);
      if (pnp_finite(cn) && cn < cost) {
        const double tabs = fmax(fabs(t[0]), fmax(fabs(t[1]), fabs(t[2])));
        const bool small = fmax(fabs(d[0]), fmax(fabs(d[1]), fabs(d[2]))) <= 1e-13 &&
                           fmax(fabs(d[3]), fmax(fabs(d[4]), fabs(d[5]))) <= 1e-13 * (1.0 + tabs);
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = Rn[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = tn[k];
#pragma unroll
        for (int k = 0; k < 21; ++k) JtJ[k] = JtJn[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) Jtr[k] = Jtrn[k];
        cost = cn;
        mu = fmax(mu * 0.1, 1e-15);
        if (small) break;
        continue;
      }
    }
    mu *= 10.0;
    if (mu > 1e16) break;
  }
  // Gauss-Newton polish: next to the minimum the cost changes by less than its own rounding, so the acceptance test above
  // stops ~sqrt(eps) away from it; the gradient still resolves it.  Undamped steps while they shrink at least twofold and
  // the cost stays within 1e-10 of the best: the iterate settles where the normal equations put the minimum (~cond(J) eps).
  double prev = 1e300;
  for (int it = 0; it < PNP_POLISH_ITER; ++it) {
    double A[21], d[6];
#pragma unroll
    for (int k = 0; k < 21; ++k) A[k] = JtJ[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) d[k] = -Jtr[k];
    if (!chol_solve<6>(A, d)) break;
    double dn = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) dn = fmax(dn, fabs(d[k]));
    if (!(dn < 0.5 * prev) || dn == 0.0) break;
    double E[9], Rn[9], tn[3], JtJn[21], Jtrn[6];
    rot_exp(d, E);
    mat3_mul(E, R, Rn);
    tn[0] = t[0] + d[3]; tn[1] = t[1] + d[4]; tn[2] = t[2] + d[5];
    const double cn = pnp_cost<true>(obj, uv, n, f32, cen, Rn, tn, JtJn, Jtrn);
    if (!pnp_finite(cn) || cn > cost * (1.0 + 1e-10)) break;
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = Rn[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = tn[k];
#pragma unroll
    for (int k = 0; k < 21; ++k) JtJ[k] = JtJn[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) Jtr[k] = Jtrn[k];
    cost = cn < cost ? cn : cost;
    prev = dn;
  }
  return cost;
}

// t minimising the algebraic error sum |B(u_i) (R (X_i - c) + t)|^2 for a fixed R (B(u) = [1 0 -u; 0 1 -v]).
CBA_HD bool pnp_translation(const double* obj, const double* uv, int n, int f32, const double* cen, const double* R, double* t) {
  double A[6] = {0, 0, 0, 0, 0, 0};
  double b[3] = {0, 0, 0};
  for (int i = 0; i < n; ++i) {
    double X[3], u[2];
    pnp_load(obj, uv, i, f32, X, u);
    X[0] -= cen[0]; X[1] -= cen[1]; X[2] -= cen[2];
    const double a0 = R[0] * X[0] + R[1] * X[1] + R[2] * X[2];
    const double a1 = R[3] * X[0] + R[4] * X[1] + R[5] * X[2];
    const double a2 = R[6] * X[0] + R[7] * X[1] + R[8] * X[2];
    const double r0[3] = {1.0, 0.0, -u[0]}, r1[3] = {0.0, 1.0, -u[1]};
    normal_add<3>(A, b, r0, u[0] * a2 - a0);
    normal_add<3>(A, b, r1, u[1] * a2 - a1);
  }
  if (!chol_solve<3>(A, b)) return false;
  t[0] = b[0]; t[1] = b[1]; t[2] = b[2];
  return pnp_finite(t[0]) && pnp_finite(t[1]) && pnp_finite(t[2]);
}

// The two DLT rows of one correspondence (x, y) -> (u, v) of a homography with h33 = 1, added to the packed 8 x 8 normal equations
// A and their right-hand side h (pnp_planar_init; the start of the homography fit of frame_select_math.h).
CBA_HD void homog_dlt_add(double* A, double* h, double x, double y, double u, double v) {
  const double ru[8] = {x, y, 1.0, 0.0, 0.0, 0.0, -u * x, -u * y};
  const double rv[8] = {0.0, 0.0, 0.0, x, y, 1.0, -v * x, -v * y};
  normal_add<8>(A, h, ru, u);
  normal_add<8>(A, h, rv, v);
}

// Planar initial rotations (IPPE) from the homography of the centred board; false when the homography is degenerate.
CBA_HD bool pnp_planar_init(const double* obj, const double* uv, int n, int f32, const double* cen, const double* im_c, double s_o,
                            double s_i, double* R1, double* R2) {
  double A[36], h[8];
#pragma unroll
  for (int k = 0; k < 36; ++k) A[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k) h[k] = 0.0;
  const double io = 1.0 / s_o, ii = 1.0 / s_i;
  for (int i = 0; i < n; ++i) {
    double X[3], u[2];
    pnp_load(obj, uv, i, f32, X, u);
    const double x = (X[0] - cen[0]) * io, y = (X[1] - cen[1]) * io;
    const double uu = (u[0] - im_c[0]) * ii, vv = (u[1] - im_c[1]) * ii;
    homog_dlt_add(A, h, x, y, uu, vv);
  }
  if (!chol_solve<8>(A, h)) return false;
  // H = Ti^-1 Hn So with So = diag(1/s_o, 1/s_o, 1), Ti^-1 = [s_i 0 cx; 0 s_i cy; 0 0 1]: H22 = 1
  const double g0 = h[6] * io, g1 = h[7] * io;  // third row (g0, g1, 1)
  const double H00 = (s_i * h[0] * io) + im_c[0] * g0, H01 = (s_i * h[1] * io) + im_c[0] * g1, H02 = s_i * h[2] + im_c[0];
  const double H10 = (s_i * h[3] * io) + im_c[1] * g0, H11 = (s_i * h[4] * io) + im_c[1] * g1, H12 = s_i * h[5] + im_c[1];
  const double p = H02, q = H12;  // image of the board centre
  const double j00 = H00 - g0 * p, j01 = H01 - g1 * p, j10 = H10 - g0 * q, j11 = H11 - g1 * q;
  // Rv: the smallest rotation taking e_z to nv = (p, q, 1) / |.|
  const double nn = 1.0 / sqrt(p * p + q * q + 1.0);
  const double n0 = p * nn, n1 = q * nn, c = nn;
  const double k = 1.0 / (1.0 + c);
  // axis a = e_z x nv = (-n1, n0, 0): Rv = I + [a]x + (a a^T - |a|^2 I) / (1 + c)
  const double s2 = n0 * n0 + n1 * n1;
  double Rv[9];
  Rv[0] = 1.0 + (n1 * n1 - s2) * k; Rv[1] = -n0 * n1 * k;           Rv[2] = n0;
  Rv[3] = -n0 * n1 * k;           Rv[4] = 1.0 + (n0 * n0 - s2) * k; Rv[5] = n1;
  Rv[6] = -n0;                    Rv[7] = -n1;                    Rv[8] = 1.0 - s2 * k;
  // Bm = ([1 0 -p; 0 1 -q] Rv)[:, :2]
  const double b00 = Rv[0] - p * Rv[6], b01 = Rv[1] - p * Rv[7];
  const double b10 = Rv[3] - q * Rv[6], b11 = Rv[4] - q * Rv[7];
  const double det = b00 * b11 - b01 * b10;
  if (!(fabs(det) > 1e-14)) return false;
  const double id = 1.0 / det;
  const double a00 = id * (b11 * j00 - b01 * j10), a01 = id * (b11 * j01 - b01 * j11);
  const double a10 = id * (-b10 * j00 + b00 * j10), a11 = id * (-b10 * j01 + b00 * j11);
  // largest singular value of A
  const double m00 = a00 * a00 + a10 * a10, m01 = a00 * a01 + a10 * a11, m11 = a01 * a01 + a11 * a11;
  const double gam2 = 0.5 * (m00 + m11 + sqrt((m00 - m11) * (m00 - m11) + 4.0 * m01 * m01));
  if (!(gam2 > 1e-24) || !pnp_finite(gam2)) return false;
  const double ig = 1.0 / sqrt(gam2);
  const double c00 = a00 * ig, c01 = a01 * ig, c10 = a10 * ig, c11 = a11 * ig;
  const double e0 = sqrt(fmax(0.0, 1.0 - c00 * c00 - c10 * c10));
  double e1 = sqrt(fmax(0.0, 1.0 - c01 * c01 - c11 * c11));
  if (c00 * c01 + c10 * c11 > 0.0) e1 = -e1;  // columns orthogonal: e0 e1 = -(c00 c01 + c10 c11)
#pragma unroll
  for (int sgn = 0; sgn < 2; ++sgn) {
    const double f0 = sgn ? -e0 : e0, f1 = sgn ? -e1 : e1;
    // R~ = [col0 col1 col0 x col1], col0 = (c00, c10, f0), col1 = (c01, c11, f1)
    const double Rt[9] = {c00, c01, c10 * f1 - f0 * c11,
                          c10, c11, f0 * c01 - c00 * f1,
                          f0,  f1,  c00 * c11 - c10 * c01};
    mat3_mul(Rv, Rt, sgn ? R2 : R1);
  }
  return true;
}

CBA_HD double det3(const double* M) {
  return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

CBA_HD bool pnp_dlt_finish(double* A, double* p, double s_o, double* R, double* t);

// Non-planar initial pose by DLT (P34 = 1 on the centred, scaled object points); false when degenerate.
CBA_HD bool pnp_dlt_init(const double* obj, const double* uv, int n, int f32, const double* cen, double s_o, double* R, double* t) {
  double A[66], p[11];
#pragma unroll
  for (int k = 0; k < 66; ++k) A[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 11; ++k) p[k] = 0.0;
  const double io = 1.0 / s_o;
  for (int i = 0; i < n; ++i) {
    double X[3], u[2];
    pnp_load(obj, uv, i, f32, X, u);
    const double x = (X[0] - cen[0]) * io, y = (X[1] - cen[1]) * io, z = (X[2] - cen[2]) * io;
    const double ru[11] = {x, y, z, 1.0, 0.0, 0.0, 0.0, 0.0, -u[0] * x, -u[0] * y, -u[0] * z};
    const double rv[11] = {0.0, 0.0, 0.0, 0.0, x, y, z, 1.0, -u[1] * x, -u[1] * y, -u[1] * z};
    normal_add<11>(A, p, ru, u[0]);
    normal_add<11>(A, p, rv, u[1]);
  }
  return pnp_dlt_finish(A, p, s_o, R, t);
}

// The rest of pnp_dlt_init from its accumulated 11 x 11 normal equations (packed lower A, right-hand side p; both overwritten):
// solve, project the 3 x 3 block onto SO(3), t = p4 / scale.  Also the last step of a resection hypothesis (epipolar_math.h).
CBA_HD bool pnp_dlt_finish(double* A, double* p, double s_o, double* R, double* t) {
  const double io = 1.0 / s_o;
  if (!chol_solve<11>(A, p)) return false;
  double M[9] = {p[0] * io, p[1] * io, p[2] * io, p[4] * io, p[5] * io, p[6] * io, p[8] * io, p[9] * io, p[10] * io};
  double p4[3] = {p[3], p[7], 1.0};
  double dm = det3(M);
  if (!(fabs(dm) > 0.0) || !pnp_finite(dm)) return false;
  if (dm < 0.0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) M[k] = -M[k];
    p4[0] = -p4[0]; p4[1] = -p4[1]; p4[2] = -p4[2];
    dm = -dm;
  }
  // polar factor by the scaled Newton iteration Y <- (g Y + Y^-T / g) / 2, g = |det Y|^(-1/3)
  double Y[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) Y[k] = M[k];
  for (int it = 0; it < 30; ++it) {
    const double dy = det3(Y);
    if (!(dy > 0.0) || !pnp_finite(dy)) return false;
    const double g = 1.0 / cbrt(dy);
    const double idg = 1.0 / (dy * g);
    // Y^-T = cofactor(Y) / det
    const double C[9] = {Y[4] * Y[8] - Y[5] * Y[7], Y[5] * Y[6] - Y[3] * Y[8], Y[3] * Y[7] - Y[4] * Y[6],
                         Y[2] * Y[7] - Y[1] * Y[8], Y[0] * Y[8] - Y[2] * Y[6], Y[1] * Y[6] - Y[0] * Y[7],
                         Y[1] * Y[5] - Y[2] * Y[4], Y[2] * Y[3] - Y[0] * Y[5], Y[0] * Y[4] - Y[1] * Y[3]};
    double change = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const double yn = 0.5 * (g * Y[k] + C[k] * idg);
      change = fmax(change, fabs(yn - Y[k]));
      Y[k] = yn;
    }
    if (change <= 1e-15) break;
  }
  double scale = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) scale += Y[k] * M[k];
  scale *= 1.0 / 3.0;
  if (!(scale > 0.0) || !pnp_finite(scale)) return false;
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = Y[k];
  t[0] = p4[0] / scale; t[1] = p4[1] / scale; t[2] = p4[2] / scale;
  return true;
}

CBA_HD int pnp_fail(double* R, double* t, double* rmse, int status) {
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
  t[0] = t[1] = t[2] = 0.0;
  *rmse = 0.0;
  return status;
}

// The pose of one view (obj: n x 3, uv: n x 2 normalised); returns the status.
CBA_HD int pnp_view(const double* obj, const double* uv, int n, int min_points, int f32, double* R, double* t, double* rmse) {
  if (n <= 0) return pnp_fail(R, t, rmse, PNP_TOO_FEW);
  double cen[3] = {0, 0, 0}, im_c[2] = {0, 0};
  double zmin = 0.0, zmax = 0.0;
  for (int i = 0; i < n; ++i) {
    double X[3], u[2];
    pnp_load(obj, uv, i, f32, X, u);
    cen[0] += X[0]; cen[1] += X[1]; cen[2] += X[2];
    im_c[0] += u[0]; im_c[1] += u[1];
    zmin = (i == 0) ? X[2] : fmin(zmin, X[2]);
    zmax = (i == 0) ? X[2] : fmax(zmax, X[2]);
  }
  const bool planar = zmax - zmin < PNP_PLANAR_TOL;
  const int floor_n = planar ? min_points : (min_points > 6 ? min_points : 6);
  if (n < floor_n) return pnp_fail(R, t, rmse, PNP_TOO_FEW);
  const double inv_n = 1.0 / n;
  cen[0] *= inv_n; cen[1] *= inv_n; cen[2] *= inv_n;
  im_c[0] *= inv_n; im_c[1] *= inv_n;
  double s_o = 0.0, s_i = 0.0;  // mean distances from the centroids
  for (int i = 0; i < n; ++i) {
    double X[3], u[2];
    pnp_load(obj, uv, i, f32, X, u);
    const double dx = X[0] - cen[0], dy = X[1] - cen[1], dz = X[2] - cen[2];
    s_o += sqrt(dx * dx + dy * dy + dz * dz);
    s_i += sqrt((u[0] - im_c[0]) * (u[0] - im_c[0]) + (u[1] - im_c[1]) * (u[1] - im_c[1]));
  }
  s_o *= inv_n;
  s_i *= inv_n;
  if (!(s_o > 0.0) || !(s_i > 0.0) || !pnp_finite(s_o) || !pnp_finite(s_i)) return pnp_fail(R, t, rmse, PNP_FAILED);
  double cost;
  if (planar) {
    double R1[9], R2[9], t1[3], t2[3];
    if (!pnp_planar_init(obj, uv, n, f32, cen, im_c, s_o, s_i, R1, R2)) return pnp_fail(R, t, rmse, PNP_FAILED);
    const bool ok1 = pnp_translation(obj, uv, n, f32, cen, R1, t1);
    const bool ok2 = pnp_translation(obj, uv, n, f32, cen, R2, t2);
    double c1 = ok1 ? pnp_refine(obj, uv, n, f32, cen, R1, t1) : 0.0;
    double c2 = ok2 ? pnp_refine(obj, uv, n, f32, cen, R2, t2) : 0.0;
    const bool v1 = ok1 && pnp_finite(c1), v2 = ok2 && pnp_finite(c2);
    if (!v1 && !v2) return pnp_fail(R, t, rmse, PNP_FAILED);
    const bool take2 = v2 && (!v1 || c2 < c1);
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = take2 ? R2[k] : R1[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = take2 ? t2[k] : t1[k];
    cost = take2 ? c2 : c1;
  } else {
    if (!pnp_dlt_init(obj, uv, n, f32, cen, s_o, R, t)) return pnp_fail(R, t, rmse, PNP_FAILED);
    cost = pnp_refine(obj, uv, n, f32, cen, R, t);
  }
  // back to the board's own origin: R (X - c) + tc = R X + (tc - R c)
  const double tc0 = t[0], tc1 = t[1], tc2 = t[2];
  t[0] = tc0 - (R[0] * cen[0] + R[1] * cen[1] + R[2] * cen[2]);
  t[1] = tc1 - (R[3] * cen[0] + R[4] * cen[1] + R[5] * cen[2]);
  t[2] = tc2 - (R[6] * cen[0] + R[7] * cen[1] + R[8] * cen[2]);
  const double zero[3] = {0.0, 0.0, 0.0};
  double dummy[27];
  const double c_final = pnp_cost<false>(obj, uv, n, f32, zero, R, t, dummy, dummy);
  bool fin = pnp_finite(cost) && pnp_finite(c_final);
#pragma unroll
  for (int k = 0; k < 9; ++k) fin = fin && pnp_finite(R[k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) fin = fin && pnp_finite(t[k]);
  if (!fin) return pnp_fail(R, t, rmse, PNP_FAILED);
  *rmse = sqrt(c_final * inv_n);
  return PNP_OK;
}

CBA_HD void two_view_dlt(const double* rt, double xa, double ya, double xb, double yb, double* w);

// Squared two-view reprojection error of one common observation: DLT with camera A at [I | 0] and B at [R | t] (rt: R
// row-major, then t), the null vector of the 4 x 4 normal matrix as cba_triangulate forms it, then reprojection into both.
// Returns |a - proj_A(X)|^2 + |b - proj_B(X)|^2.
CBA_HD double pair_obs_sq(const double* rt, double xa, double ya, double xb, double yb) {
  double w[4];
  two_view_dlt(rt, xa, ya, xb, yb, w);
  const double X = w[0] / w[3], Y = w[1] / w[3], Z = w[2] / w[3];
  const double ex = xa - X / Z, ey = ya - Y / Z;
  const double bx = rt[0] * X + rt[1] * Y + rt[2] * Z + rt[9];
  const double by = rt[3] * X + rt[4] * Y + rt[5] * Z + rt[10];
  const double bz = rt[6] * X + rt[7] * Y + rt[8] * Z + rt[11];
  const double fx = xb - bx / bz, fy = yb - by / bz;
  return ex * ex + ey * ey + fx * fx + fy * fy;
}

// The homogeneous two-view DLT point of one correspondence (A at [I | 0], B at [R | t]): the null vector w[4] of the 4 x 4
// normal matrix, as cba_triangulate forms it (pair_obs_sq; the cheirality test and the scaffold cloud of epipolar_math.h).
CBA_HD void two_view_dlt(const double* rt, double xa, double ya, double xb, double yb, double* w) {
  double M[4][4];
  const double ra0[4] = {-1.0, 0.0, xa, 0.0}, ra1[4] = {0.0, -1.0, ya, 0.0};
  double rb0[4], rb1[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const double p0 = c < 3 ? rt[c] : rt[9], p1 = c < 3 ? rt[3 + c] : rt[10], p2 = c < 3 ? rt[6 + c] : rt[11];
    rb0[c] = xb * p2 - p0;
    rb1[c] = yb * p2 - p1;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = r; c < 4; ++c) M[r][c] = ra0[r] * ra0[c] + ra1[r] * ra1[c] + rb0[r] * rb0[c] + rb1[r] * rb1[c];
#pragma unroll
  for (int r = 1; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < r; ++c) M[r][c] = M[c][r];
  sym4_null_vector(M, w);
}

}  // namespace cba
