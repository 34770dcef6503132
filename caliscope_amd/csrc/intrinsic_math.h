// Intrinsic calibration of one camera from its board views: the arithmetic of caliscope_amd/calibrate_intrinsics.py, host + device
// inline functions.  hipcc compiles it into k_intrinsics of pose_lib.hip (one workgroup per camera); g++ compiles it into
// tests/native/intrinsic_harness.cpp.
//
//   unknowns    pinhole fx fy cx cy k1 k2 p1 p2 k3 (NI = 9), fisheye fx fy cx cy k1 k2 k3 k4 (NI = 8), skew fixed at 0; and one
//               pose per usable view, moved by the left axis-angle increment of pnp_math.h: R <- exp(w) R, t <- t + dt.
//   cost        sum over views and corners of |proj(intr, R X + t) - pixel|^2 in PIXELS.
//   start       intr_start: pinhole f = max(w, h), c = ((w - 1)/2, (h - 1)/2); fisheye f = max(w, h) / pi, c = (w/2 - 0.5,
//               h/2 - 0.5); zero coefficients (or the caller's values).  View poses: pnp_view on the pixels undistorted with the
//               start intrinsics.  intr_view_screen leaves a view out (PNP_TOO_FEW / PNP_FAILED) when its PnP did, when a
//               fisheye corner lies beyond INTR_MAX_THETA_D under the start intrinsics (the undistortion clips at 90 degrees),
//               or when a corner is not in front of the camera at the start pose; such a view never enters the solve.
//   step        Levenberg-Marquardt, Marquardt damping mu diag(J^T J).  The normal equations are an arrowhead: per view A_v
//               (6 x 6), B_v (6 x NI), g_v; shared C (NI x NI), g_c.  intr_view_reduce linearises one view, factors the damped
//               A_v = L L^T, adds C_v - Z^T Z and g_cv - Z^T L^-1 g_v (Z = L^-1 B_v) to the caller's partial of the reduced system
//               and keeps A_v^-1 g_v, A_v^-1 B_v in the view's work row; intr_solve_reduced solves the NI x NI system (Jacobi-scaled,
//               chol_solve<NI>); intr_view_trial back-substitutes the view's step and evaluates the trial cost.  No
//               per-observation Jacobian is stored.  A step is accepted when the true cost falls.
//   stopping    an accepted step below 1e-14 relative, a cost that no longer changes by more than 1e-13 of itself (or by more than
//               rounding leaves of it), damping above
//               1e16, or max_iter linearisations; then at most INTR_POLISH_ITER undamped Gauss-Newton steps while each is less
//               than half the one before (as pnp_refine: the cost cannot resolve the last ~sqrt(eps), the gradient can).
//   statuses    INTR_OK / INTR_TOO_FEW (fewer than INTR_MIN_VIEWS usable views or fewer than NI + 6 views residuals) /
//               INTR_FAILED (no solvable reduced system at the start, non-finite result).  A camera that is not INTR_OK keeps
//               the start intrinsics and rmse 0, and its views the poses at which the solve stopped (the start poses when it never stepped):
//               no NaN leaves this file.
//
// intr_calibrate is a template over a SUM FUNCTOR that owns the views of one camera (the pattern of epi_refine):
//   screen(in0, out[2])        screens every view, returns {usable views, their corners}
//   reduce(in, mu, out[NSUM])  the reduced system at (in, poses): packed NI x NI, right-hand side, cost
//   trial(in_new, di, out[2])  back-substitution into the trial poses; {trial cost, squared pose step}
//   accept()                   trial poses -> poses
//   finish(in, ok)             per-view outputs
// Every thread of a workgroup calls it with the same arguments and gets the same sums: the host functor loops over views in the
// order of the device's fixed reduction tree (EPI_REDUCE_NT "threads", thread t takes views t, t + NT, ...).
//
// Work row of a view (INTR_WORK doubles): [0, 12) pose R row-major then t; [12, 24) trial pose; [24, 30) A_v^-1 g_v;
// [30, 30 + 6 NI) A_v^-1 B_v, column c at 30 + 6 c.
#pragma once
#include "epipolar_math.h"

// no contraction, as pnp_math.h: the device then rounds as the g++ build does
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace cba {

constexpr int INTR_OK = 0;
constexpr int INTR_TOO_FEW = 1;
constexpr int INTR_FAILED = 2;
constexpr int INTR_LM_MAX_ITER = 100;  // default of max_iter
constexpr int INTR_POLISH_ITER = 8;
constexpr int INTR_MIN_VIEWS = 3;
constexpr int INTR_MIN_POINTS = 4;          // corners per view (the reference's MIN_CORNERS_PER_FRAME)
constexpr double INTR_MAX_THETA_D = 1.5;    // rad; fisheye corners beyond it at the start leave the view out
constexpr int INTR_WORK = 30 + 6 * 9;
constexpr double INTR_BAD_COST = 1e300;     // a corner behind the camera: no such trial is accepted

template <int MODEL>
struct IntrDim {
  static constexpr int NI = MODEL == MODEL_FISHEYE4 ? 8 : 9;
  static constexpr int NP = NI * (NI + 1) / 2;
  static constexpr int NSUM = NP + NI + 1;
};
constexpr int INTR_NSUM_MAX = IntrDim<MODEL_PINHOLE_BC5>::NSUM;  // 55

// start intrinsics (fx fy cx cy d0..d4) from the image size
CBA_HD void intr_start(int model, double width, double height, double* in9) {
  const double m = width > height ? width : height;
#pragma unroll
  for (int k = 0; k < 9; ++k) in9[k] = 0.0;
  if (model == MODEL_FISHEYE4) {
    in9[0] = in9[1] = m / 3.141592653589793;
    in9[2] = 0.5 * width - 0.5;
    in9[3] = 0.5 * height - 0.5;
  } else {
    in9[0] = in9[1] = m;
    in9[2] = (width - 1.0) * 0.5;
    in9[3] = (height - 1.0) * 0.5;
  }
}

// N x N Cholesky in the packed layout of chol_solve, split into its three parts for several right-hand sides
template <int N>
CBA_HD bool chol_factor(double* A) {
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
  return true;
}
template <int N>
CBA_HD void chol_fwd(const double* L, double* b) {  // b <- L^-1 b
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int ii = i * (i + 1) / 2;
    double s = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= L[ii + k] * b[k];
    b[i] = s * L[ii + i];
  }
}
template <int N>
CBA_HD void chol_bwd(const double* L, double* b) {  // b <- L^-T b
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    double s = b[i];
#pragma unroll
    for (int k = i + 1; k < N; ++k) s -= L[k * (k + 1) / 2 + i] * b[k];
    b[i] = s * L[i * (i + 1) / 2 + i];
  }
}

// structural zeros of the intrinsic rows of a corner: ix = (xd, 0, 1, 0, k...), iy = (0, yd, 0, 1, k...)
CBA_HD constexpr bool intr_zx(int c) { return c == 1 || c == 3; }
CBA_HD constexpr bool intr_zy(int c) { return c == 0 || c == 2; }

// One corner of a view, rounded to float32 when f32: object point (NaN z -> 0) and pixel.  Selected by value, as ba_math.h advises
// (pnp_load stores under an `if`).
CBA_HD void intr_load(const double* obj, const double* xy, int i, int f32, double* X, double* u) {
  const double x = obj[3 * i], y = obj[3 * i + 1], z0 = obj[3 * i + 2], px = xy[2 * i], py = xy[2 * i + 1];
  const double z = (z0 == z0) ? z0 : 0.0;
  X[0] = f32 ? (double)(float)x : x;
  X[1] = f32 ? (double)(float)y : y;
  X[2] = f32 ? (double)(float)z : z;
  u[0] = f32 ? (double)(float)px : px;
  u[1] = f32 ? (double)(float)py : py;
}

// One corner: residual e = proj - pixel (pixels); with JAC the rows of its Jacobian: jx, jy [6] (pose: w then t), ix, iy [NI]
// (columns fx fy cx cy k...: those of oracle/camera_model.py).  False when the corner is not in front of the camera.
template <int MODEL, bool JAC>
CBA_HD bool intr_point(const double* in, const double* R, const double* t, const double* X, const double* u, double* e, double* jx,
                       double* jy, double* ix, double* iy) {
  const double fx = in[0], fy = in[1], cx = in[2], cy = in[3];
  const double a0 = R[0] * X[0] + R[1] * X[1] + R[2] * X[2];
  const double a1 = R[3] * X[0] + R[4] * X[1] + R[5] * X[2];
  const double a2 = R[6] * X[0] + R[7] * X[1] + R[8] * X[2];
  const double zc = a2 + t[2];
  const double iz = 1.0 / zc;
  const double x = (a0 + t[0]) * iz, y = (a1 + t[1]) * iz;
  const double r2 = x * x + y * y;
  double xd, yd, dxx = 1.0, dxy = 0.0, dyy = 1.0;
  if (MODEL == MODEL_PINHOLE_BC5) {
    const double k1 = in[4], k2 = in[5], p1 = in[6], p2 = in[7], k3 = in[8];
    const double r4 = r2 * r2, r6 = r4 * r2;
    const double cd = 1.0 + k1 * r2 + k2 * r4 + k3 * r6;
    const double b1 = 2.0 * x * y, b2 = r2 + 2.0 * x * x, b3 = r2 + 2.0 * y * y;
    xd = x * cd + p1 * b1 + p2 * b2;
    yd = y * cd + p1 * b3 + p2 * b1;
    if (JAC) {
      const double dcd = k1 + 2.0 * k2 * r2 + 3.0 * k3 * r4;
      dxx = cd + 2.0 * x * x * dcd + 2.0 * p1 * y + 6.0 * p2 * x;
      dxy = 2.0 * x * y * dcd + 2.0 * p1 * x + 2.0 * p2 * y;
      dyy = cd + 2.0 * y * y * dcd + 6.0 * p1 * y + 2.0 * p2 * x;
      ix[4] = fx * x * r2; iy[4] = fy * y * r2;
      ix[5] = fx * x * r4; iy[5] = fy * y * r4;
      ix[6] = fx * b1;     iy[6] = fy * b3;
      ix[7] = fx * b2;     iy[7] = fy * b1;
      ix[8] = fx * x * r6; iy[8] = fy * y * r6;
    }
  } else {
    const double r = sqrt(r2);
    double cd = 1.0;
    if (r > 1e-8) {
      const double th = atan(r), th2 = th * th;
      const double th3 = th * th2, th5 = th3 * th2, th7 = th5 * th2, th9 = th7 * th2;
      const double thd = th + in[4] * th3 + in[5] * th5 + in[6] * th7 + in[7] * th9;
      const double inv_r = 1.0 / r;
      cd = thd * inv_r;
      if (JAC) {
        const double dthd = 1.0 + 3.0 * in[4] * th2 + 5.0 * in[5] * th2 * th2 + 7.0 * in[6] * th2 * th2 * th2 + 9.0 * in[7] * th2 * th2 * th2 * th2;
        const double gg = (dthd / (1.0 + r2) * r - thd) * inv_r * inv_r * inv_r;  // d cd / dr / r
        dxx = cd + x * x * gg;
        dxy = x * y * gg;
        dyy = cd + y * y * gg;
        ix[4] = fx * x * (th3 * inv_r); iy[4] = fy * y * (th3 * inv_r);
        ix[5] = fx * x * (th5 * inv_r); iy[5] = fy * y * (th5 * inv_r);
        ix[6] = fx * x * (th7 * inv_r); iy[6] = fy * y * (th7 * inv_r);
        ix[7] = fx * x * (th9 * inv_r); iy[7] = fy * y * (th9 * inv_r);
      }
    } else if (JAC) {
#pragma unroll
      for (int k = 4; k < 8; ++k) ix[k] = iy[k] = 0.0;
    }
    xd = x * cd;
    yd = y * cd;
  }
  e[0] = (fx * xd + cx) - u[0];
  e[1] = (fy * yd + cy) - u[1];
  if (JAC) {
    ix[0] = xd;  iy[0] = 0.0;
    ix[1] = 0.0; iy[1] = yd;
    ix[2] = 1.0; iy[2] = 0.0;
    ix[3] = 0.0; iy[3] = 1.0;
    // G = d(pixel)/dX_c; dX_c/dw = -[a]x = [0 a2 -a1; -a2 0 a0; a1 -a0 0]; dX_c/dt = I
    const double g00 = fx * dxx * iz, g01 = fx * dxy * iz, g02 = -(g00 * x + g01 * y);
    const double g10 = fy * dxy * iz, g11 = fy * dyy * iz, g12 = -(g10 * x + g11 * y);
    jx[0] = g02 * a1 - g01 * a2; jy[0] = g12 * a1 - g11 * a2;
    jx[1] = g00 * a2 - g02 * a0; jy[1] = g10 * a2 - g12 * a0;
    jx[2] = g01 * a0 - g00 * a1; jy[2] = g11 * a0 - g10 * a1;
    jx[3] = g00; jy[3] = g10;
    jx[4] = g01; jy[4] = g11;
    jx[5] = g02; jy[5] = g12;
  }
  return zc > 1e-9;
}

// sum |e|^2 of a view at (in, R, t); INTR_BAD_COST when a corner is not in front or the sum is not finite
template <int MODEL>
CBA_HD double intr_view_cost(const double* in, const double* R, const double* t, const double* obj, const double* xy, int n, int f32) {
  double cost = 0.0;
  bool ok = true;
  for (int i = 0; i < n; ++i) {
    double X[3], u[2], e[2];
    intr_load(obj, xy, i, f32, X, u);
    ok = intr_point<MODEL, false>(in, R, t, X, u, e, nullptr, nullptr, nullptr, nullptr) && ok;
    cost += e[0] * e[0] + e[1] * e[1];
  }
  return (ok && pnp_finite(cost)) ? cost : INTR_BAD_COST;
}

// Screening of one view before the solve: `pose` is pnp_view's result on the pixels undistorted with the start intrinsics in0,
// pnp_status its status.  Copies the pose into the work row; returns the view's status.
template <int MODEL>
CBA_HD int intr_view_screen(const double* in0, const double* obj, const double* xy, int n, int f32, int pnp_status, const double* pose,
                            double* w) {
#pragma unroll
  for (int k = 0; k < 12; ++k) w[k] = w[12 + k] = (k % 4 == 0 && k < 9) ? 1.0 : 0.0;
#pragma unroll
  for (int k = 24; k < INTR_WORK; ++k) w[k] = 0.0;
  if (n < INTR_MIN_POINTS) return PNP_TOO_FEW;
  if (pnp_status != PNP_OK) return pnp_status;
  bool ok = true;
  for (int i = 0; i < n; ++i) {
    double X[3], u[2];
    intr_load(obj, xy, i, f32, X, u);
    ok = ok && pnp_finite(u[0]) && pnp_finite(u[1]);
    if (MODEL == MODEL_FISHEYE4) {
      const double x0 = (u[0] - in0[2]) / in0[0], y0 = (u[1] - in0[3]) / in0[1];
      ok = ok && (x0 * x0 + y0 * y0 <= INTR_MAX_THETA_D * INTR_MAX_THETA_D);
    }
    const double zc = pose[6] * X[0] + pose[7] * X[1] + pose[8] * X[2] + pose[11];
    ok = ok && (zc > 1e-9);
  }
  if (!ok) return PNP_FAILED;
#pragma unroll
  for (int k = 0; k < 12; ++k) w[k] = w[12 + k] = pose[k];
  return PNP_OK;
}

// Linearisation and elimination of one view at (in, its pose) with damping mu; acc[NSUM] += the view's part of the reduced system.
template <int MODEL>
CBA_HD void intr_view_reduce(const double* in, double mu, const double* obj, const double* xy, int n, int f32, double* w, double* acc) {
  constexpr int NI = IntrDim<MODEL>::NI, NP = IntrDim<MODEL>::NP;
  double R[9], t[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = w[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = w[9 + k];
  // Two passes over the view's corners, so that neither keeps more accumulators in flight than the VALU registers hold (one
  // pass with A, B, g and the 55 partial sums together went through AGPR copies for every update and spilled to scratch):
  // first the intrinsics block C_v, g_cv straight into the partial, then the pose blocks.
  double cost = 0.0;
  bool ok = true;
  for (int i = 0; i < n; ++i) {
    double X[3], u[2], e[2], jx[6], jy[6], ix[NI], iy[NI];
    intr_load(obj, xy, i, f32, X, u);
    ok = intr_point<MODEL, true>(in, R, t, X, u, e, jx, jy, ix, iy) && ok;
    cost += e[0] * e[0] + e[1] * e[1];
    // (columns fx fy cx cy have structural zeros, intr_zx / intr_zy: written out, because x * 0.0 may not be folded away)
#pragma unroll
    for (int r = 0; r < NI; ++r) {
#pragma unroll
      for (int c = 0; c < r; ++c) {
        const bool hx = !intr_zx(r) && !intr_zx(c), hy = !intr_zy(r) && !intr_zy(c);
        if (hx && hy) acc[r * (r + 1) / 2 + c] += ix[r] * ix[c] + iy[r] * iy[c];
        else if (hx) acc[r * (r + 1) / 2 + c] += ix[r] * ix[c];
        else if (hy) acc[r * (r + 1) / 2 + c] += iy[r] * iy[c];
      }
      const double s = intr_zx(r) ? iy[r] * iy[r] : intr_zy(r) ? ix[r] * ix[r] : ix[r] * ix[r] + iy[r] * iy[r];
      acc[r * (r + 1) / 2 + r] += s + mu * s;  // Marquardt damping of C, term by term: the sum is linear in it
      acc[NP + r] += intr_zx(r) ? iy[r] * e[1] : intr_zy(r) ? ix[r] * e[0] : ix[r] * e[0] + iy[r] * e[1];
    }
  }
  double A[21], B[6 * NI], g[6];
#pragma unroll
  for (int k = 0; k < 21; ++k) A[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 6 * NI; ++k) B[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) g[k] = 0.0;
  for (int i = 0; i < n; ++i) {
    double X[3], u[2], e[2], jx[6], jy[6], ix[NI], iy[NI];
    intr_load(obj, xy, i, f32, X, u);
    intr_point<MODEL, true>(in, R, t, X, u, e, jx, jy, ix, iy);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
      for (int c = 0; c <= r; ++c) A[r * (r + 1) / 2 + c] += jx[r] * jx[c] + jy[r] * jy[c];
      g[r] += jx[r] * e[0] + jy[r] * e[1];
    }
#pragma unroll
    for (int c = 0; c < NI; ++c) {
#pragma unroll
      for (int r = 0; r < 6; ++r) B[c * 6 + r] += intr_zx(c) ? jy[r] * iy[c] : intr_zy(c) ? jx[r] * ix[c] : jx[r] * ix[c] + jy[r] * iy[c];
    }
  }
  double dmax = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) dmax = fmax(dmax, A[k * (k + 1) / 2 + k]);
#pragma unroll
  for (int k = 0; k < 6; ++k) A[k * (k + 1) / 2 + k] += mu * fmax(A[k * (k + 1) / 2 + k], 1e-12 * dmax);
  ok = ok && pnp_finite(cost) && chol_factor<6>(A);
  if (!ok) {
    // no elimination: a non-finite cost tells the caller that this linearisation cannot be used
#pragma unroll
    for (int k = 24; k < 30 + 6 * NI; ++k) w[k] = 0.0;
    acc[NP + NI] += __builtin_nan("");
    return;
  }
  chol_fwd<6>(A, g);
#pragma unroll
  for (int c = 0; c < NI; ++c) chol_fwd<6>(A, B + 6 * c);
#pragma unroll
  for (int r = 0; r < NI; ++r) {
#pragma unroll
    for (int c = 0; c <= r; ++c) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) s += B[r * 6 + k] * B[c * 6 + k];
      acc[r * (r + 1) / 2 + c] -= s;
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) s += B[r * 6 + k] * g[k];
    acc[NP + r] -= s;
  }
  chol_bwd<6>(A, g);
#pragma unroll
  for (int k = 0; k < 6; ++k) w[24 + k] = g[k];
#pragma unroll
  for (int c = 0; c < NI; ++c) {
    chol_bwd<6>(A, B + 6 * c);
#pragma unroll
    for (int k = 0; k < 6; ++k) w[30 + 6 * c + k] = B[6 * c + k];
  }
  acc[NP + NI] += cost;
}

// The step of the intrinsics from the summed reduced system: (D S D) z = -D r with D = diag(S)^-1/2, di = D z.
template <int MODEL>
CBA_HD bool intr_solve_reduced(const double* acc, double* di) {
  constexpr int NI = IntrDim<MODEL>::NI, NP = IntrDim<MODEL>::NP;
  double S[NP], sc[NI];
  bool ok = pnp_finite(acc[NP + NI]);
#pragma unroll
  for (int k = 0; k < NI; ++k) {
    const double d = acc[k * (k + 1) / 2 + k];
    ok = ok && (d > 0.0) && pnp_finite(d);
    sc[k] = 1.0 / sqrt(ok ? d : 1.0);
  }
  if (!ok) return false;
#pragma unroll
  for (int r = 0; r < NI; ++r) {
#pragma unroll
    for (int c = 0; c <= r; ++c) S[r * (r + 1) / 2 + c] = acc[r * (r + 1) / 2 + c] * sc[r] * sc[c];
    di[r] = -acc[NP + r] * sc[r];
  }
  if (!chol_solve<NI>(S, di)) return false;
#pragma unroll
  for (int k = 0; k < NI; ++k) {
    di[k] *= sc[k];
    ok = ok && pnp_finite(di[k]);
  }
  return ok;
}

// Back-substitution of one view for the intrinsics step di, the trial pose into the work row, the trial cost at in_new.
// acc[0] += cost, acc[1] += |dw|^2 + |dt|^2 / (1 + |t|_inf)^2.
template <int MODEL>
CBA_HD void intr_view_trial(const double* in_new, const double* di, const double* obj, const double* xy, int n, int f32, double* w,
                            double* acc) {
  constexpr int NI = IntrDim<MODEL>::NI;
  double d[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    double s = -w[24 + k];
#pragma unroll
    for (int c = 0; c < NI; ++c) s -= w[30 + 6 * c + k] * di[c];
    d[k] = s;
  }
  double R[9], E[9], Rn[9], tn[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = w[k];
  rot_exp(d, E);
  mat3_mul(E, R, Rn);
  // one Newton step towards the nearest rotation, Rn <- Rn (3 I - Rn^T Rn) / 2: the products of many steps drift off SO(3) by an ulp
  // each, which no later step can undo (1e-15 in R is 5e-13 px)
  {
    double Q[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        Q[3 * r + c] = (r == c ? 3.0 : 0.0) - (Rn[r] * Rn[c] + Rn[3 + r] * Rn[3 + c] + Rn[6 + r] * Rn[6 + c]);
    mat3_mul(Rn, Q, E);
#pragma unroll
    for (int k = 0; k < 9; ++k) Rn[k] = 0.5 * E[k];
  }
  const double tabs = fmax(fabs(w[9]), fmax(fabs(w[10]), fabs(w[11])));
#pragma unroll
  for (int k = 0; k < 3; ++k) tn[k] = w[9 + k] + d[3 + k];
#pragma unroll
  for (int k = 0; k < 9; ++k) w[12 + k] = Rn[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) w[21 + k] = tn[k];
  acc[0] += intr_view_cost<MODEL>(in_new, Rn, tn, obj, xy, n, f32);
  const double it = 1.0 / (1.0 + tabs);
  acc[1] += d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + (d[3] * d[3] + d[4] * d[4] + d[5] * d[5]) * it * it;
}

CBA_HD void intr_view_accept(double* w) {
#pragma unroll
  for (int k = 0; k < 12; ++k) w[k] = w[12 + k];
}

// Outputs of one view after the solve: pose and rmse = sqrt(sum |e|^2 / n) at the final intrinsics (a view that was left out:
// I, 0, rmse 0; a camera that is not INTR_OK: the pose at which its solve stopped, rmse 0).
template <int MODEL>
CBA_HD void intr_view_finish(const double* in, bool cam_ok, const double* obj, const double* xy, int n, int f32, int view_status,
                             const double* w, double* pose_out, double* rmse_out) {
#pragma unroll
  for (int k = 0; k < 12; ++k) pose_out[k] = w[k];
  double r = 0.0;
  if (cam_ok && view_status == PNP_OK) {
    const double c = intr_view_cost<MODEL>(in, w, w + 9, obj, xy, n, f32);
    r = (c < INTR_BAD_COST) ? sqrt(c / (double)n) : 0.0;
  }
  *rmse_out = r;
}

// One step of the solve from the summed reduced system `acc`: the trial at in + di.  Returns false when there is none.
template <int MODEL, class Sum>
CBA_HD bool intr_try(Sum& sum, const double* in, const double* acc, double* in_new, double* tr, double* rel) {
  constexpr int NI = IntrDim<MODEL>::NI;
  double di[NI];
  if (!intr_solve_reduced<MODEL>(acc, di)) return false;
  double m = 0.0;
#pragma unroll
  for (int k = 0; k < NI; ++k) {
    in_new[k] = in[k] + di[k];
    m = fmax(m, fabs(di[k]) / (1.0 + fabs(in[k])));
  }
  tr[0] = tr[1] = 0.0;
  sum.trial(in_new, di, tr);
  *rel = fmax(m, sqrt(tr[1]));
  return true;
}

// The calibration of one camera.  in[9]: the start intrinsics, replaced by the result when the status is INTR_OK.
template <int MODEL, class Sum>
CBA_HD int intr_calibrate(Sum& sum, double* in9, int max_iter, double* rmse, int* iters) {
  constexpr int NI = IntrDim<MODEL>::NI, NP = IntrDim<MODEL>::NP, NSUM = IntrDim<MODEL>::NSUM;
  *rmse = 0.0;
  *iters = 0;
  double cnt[2];
  sum.screen(in9, cnt);
  const double n_views = cnt[0], n_pts = cnt[1];
  int status = INTR_OK;
  if (n_views < (double)INTR_MIN_VIEWS || 2.0 * n_pts < (double)NI + 6.0 * n_views) status = INTR_TOO_FEW;
  double in[NI], cost = 0.0;
#pragma unroll
  for (int k = 0; k < NI; ++k) in[k] = in9[k];
  if (status == INTR_OK) {
    if (max_iter <= 0) max_iter = INTR_LM_MAX_ITER;
    double acc[NSUM], in_new[NI], tr[2], rel;
    double mu = 1e-3;
    bool have_cost = false, stepped = false;
    // what rounding alone leaves of the cost (pixel coordinates of magnitude fx + cx + cy, a few ulp each): below it a change of the
    // cost carries no information, which matters on noise-free data only
    const double px_eps = 4.0 * EPS_F64 * (fabs(in[0]) + fabs(in[2]) + fabs(in[3]));
    const double floor_c = 2.0 * n_pts * px_eps * px_eps;
    int it = 0;
    for (; it < max_iter; ++it) {
      sum.reduce(in, mu, acc);
      if (!have_cost) {
        cost = acc[NP + NI];
        if (!pnp_finite(cost)) break;  // (FAILED below: nothing was ever solved)
        have_cost = true;
      }
      if (intr_try<MODEL>(sum, in, acc, in_new, tr, &rel)) {
        const double cn = tr[0];
        if (cn < INTR_BAD_COST && cn < cost) {
          const bool flat = cost - cn <= 1e-13 * cost + floor_c;
          sum.accept();
#pragma unroll
          for (int k = 0; k < NI; ++k) in[k] = in_new[k];
          cost = cn;
          stepped = true;
          mu = fmax(mu * 0.1, 1e-15);
          if (rel <= 1e-14 || flat) { ++it; break; }
          continue;
        }
        if (stepped && cn < INTR_BAD_COST && cn - cost <= 1e-13 * cost + floor_c) { ++it; break; }  // at the cost's resolution
      }
      mu *= 10.0;
      if (mu > 1e16) { ++it; break; }
    }
    if (!stepped) status = INTR_FAILED;
    double prev = 1e300;
    for (int p = 0; p < INTR_POLISH_ITER && status == INTR_OK; ++p, ++it) {
      sum.reduce(in, 0.0, acc);
      if (!intr_try<MODEL>(sum, in, acc, in_new, tr, &rel)) break;
      if (!(rel < 0.5 * prev) || rel == 0.0) break;
      const double cn = tr[0];
      if (!(cn < INTR_BAD_COST) || cn > cost * (1.0 + 1e-10) + floor_c) break;
      sum.accept();
#pragma unroll
      for (int k = 0; k < NI; ++k) in[k] = in_new[k];
      cost = cn;  // (the cost AT the accepted iterate, also where it sits a rounding above the one before)
      prev = rel;
    }
    *iters = it;
    bool fin = pnp_finite(cost);
#pragma unroll
    for (int k = 0; k < NI; ++k) fin = fin && pnp_finite(in[k]);
    if (status == INTR_OK && (!fin || !(in[0] > 0.0) || !(in[1] > 0.0))) status = INTR_FAILED;
  }
  if (status == INTR_OK) {
#pragma unroll
    for (int k = 0; k < NI; ++k) in9[k] = in[k];
    *rmse = sqrt(cost / n_pts);
  }
  sum.finish(in9, status == INTR_OK);
  return status;
}

}  // namespace cba
