// Essential-matrix RANSAC of camera pairs and RANSAC resection of cameras against a point cloud: the arithmetic of the
// epipolar pose bootstrap (caliscope_amd/epipolar_pose.py), host + device inline functions.  hipcc compiles it into the
// kernels of pose_lib.hip; g++ compiles it into tests/native/epipolar_harness.cpp.  Plain per-thread FP64, small matrices
// fully unrolled (compile-time indices), so that the device build keeps them in registers and needs no scratch.
//
// Correspondence i of a pair: normalised, undistorted points a = (xa, ya, 1) in camera A and b = (xb, yb, 1) in camera B;
// x_b^T E x_a = 0 for E = [t]x R when X_B = R X_A + t.
//
//   sampler       counter-based: draw d of hypothesis h of job j is splitmix64 of (seed, j, h, d), taken modulo n; a repeated
//                 index is drawn again (at most EPI_MAX_DRAWS times per index, then the smallest unused index)
//   minimal E     linear 8-point fit on Hartley-normalised points: the null vector of the 8 x 9 system by Householder QR of
//                 its transpose, back to camera coordinates, then the
//                 projection onto the essential manifold U diag(1, 1, 0) V^T (V from a 3 x 3 Jacobi eigen-solve of E^T E)
//   inlier test   squared Sampson distance (x_b^T E x_a)^2 / (|(E x_a)_12|^2 + |(E^T x_b)_12|^2) <= thr^2 (cv2's rule)
//   pose from E   the four (R, t) of E (R = U W V^T or U W^T V^T, t = +-u3, in that order); the candidate with the most inliers
//                 that triangulate with depth in (0, 50) in both views (recoverPose's distanceThresh) wins, the lowest index on ties
//   refinement    Levenberg-Marquardt on the Sampson residuals of the inliers, 5 parameters: R <- exp(w) R and t on S^2
//                 through a 2-D tangent basis, then (local optimisation) the inliers of the refined pose and another
//                 refinement while their count grows, at most EPI_LO_ROUNDS times; sums over the inliers come from a `Sum` object (a workgroup reduction on the
//                 device, the same fixed tree emulated on the host), so both builds take the same path through the iterations
//   conditioning  sigma_2 / sigma_1 of the linear fit on the final inliers (before the manifold projection): the null vector of
//                 their 9 x 9 normal matrix by inverse iteration started at the refined E
//   resection     6-point DLT hypotheses (pnp_math.h pnp_dlt_finish), inlier test |u - proj(R X + t)|^2 <= thr^2 with positive
//                 depth, then pnp_refine's Levenberg-Marquardt + Gauss-Newton polish restated over `Sum`
#pragma once
#include "pnp_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace cba {

constexpr int EPI_OK = 0;
constexpr int EPI_TOO_FEW = 1;
constexpr int EPI_FAILED = 2;
constexpr int EPI_SAMPLE = 8;          // essential hypothesis sample
constexpr int RES_SAMPLE = 6;          // resection hypothesis sample
constexpr int EPI_MAX_DRAWS = 64;      // draws per sample index before the deterministic fallback
constexpr double EPI_DIST_THRESH = 50.0;
constexpr int EPI_LM_MAX_ITER = 60;
constexpr int EPI_LO_ROUNDS = 8;       // local optimisation: re-flag and refine while the inlier count grows
constexpr int EPI_NSUM = 21;           // 5 x 5 packed J^T J, J^T r, cost
constexpr int RES_NSUM = 28;           // 6 x 6 packed J^T J, J^T r, cost
constexpr int EPI_LIN_NSUM = 45;       // 9 x 9 packed normal matrix of the linear fit

CBA_HD uint64_t splitmix64(uint64_t x) {
  x += 0x9e3779b97f4a7c15ULL;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
  return x ^ (x >> 31);
}

CBA_HD uint64_t epi_draw(uint64_t seed, int64_t job, int64_t h, int64_t d) {
  return splitmix64(seed + splitmix64((uint64_t)job + splitmix64((uint64_t)h + splitmix64((uint64_t)d))));
}

// K distinct indices in [0, n) (n >= K) for hypothesis h of job `job`
template <int K>
CBA_HD void sample_distinct(uint64_t seed, int64_t job, int64_t h, int64_t n, int64_t* idx) {
  int64_t d = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    int64_t cand = 0;
    bool dup = true;
    for (int a = 0; a < EPI_MAX_DRAWS && dup; ++a) {
      cand = (int64_t)(epi_draw(seed, job, h, d++) % (uint64_t)n);
      dup = false;
#pragma unroll
      for (int j = 0; j < k; ++j) dup = dup || idx[j] == cand;
    }
    if (dup) {
      cand = 0;
      for (;;) {
        bool used = false;
#pragma unroll
        for (int j = 0; j < k; ++j) used = used || idx[j] == cand;
        if (!used) break;
        ++cand;
      }
    }
    idx[k] = cand;
  }
}

// squared Sampson distance; +huge for a zero gradient (E = 0 marks an invalid hypothesis)
CBA_HD double epi_sampson(const double* E, double xa, double ya, double xb, double yb) {
  const double ex0 = E[0] * xa + E[1] * ya + E[2];
  const double ex1 = E[3] * xa + E[4] * ya + E[5];
  const double ex2 = E[6] * xa + E[7] * ya + E[8];
  const double et0 = E[0] * xb + E[3] * yb + E[6];
  const double et1 = E[1] * xb + E[4] * yb + E[7];
  const double num = xb * ex0 + yb * ex1 + ex2;
  const double d2 = ex0 * ex0 + ex1 * ex1 + et0 * et0 + et1 * et1;
  if (!(d2 > 0.0)) return 1e300;
  return num * num / d2;
}

CBA_HD void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

CBA_HD bool normalize3(double* v) {
  const double n2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
  if (!(n2 > 0.0) || !pnp_finite(n2)) return false;
  const double inv = 1.0 / sqrt(n2);
  v[0] *= inv; v[1] *= inv; v[2] *= inv;
  return true;
}

// Eigen-decomposition of a symmetric 3 x 3 by cyclic Jacobi: lam descending, V columns the eigenvectors.
CBA_HD void sym3_eigen(double (&A)[3][3], double* lam, double (&V)[3][3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) V[r][c] = (r == c) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 16; ++sweep) {
    const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
    const double diag = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
    if (off <= 1e-34 * diag) break;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = p + 1; q < 3; ++q) {
        const double apq = A[p][q];
        if (apq != 0.0) {
          const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
          const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const double akp = A[k][p], akq = A[k][q];
            A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
            const double vkp = V[k][p], vkq = V[k][q];
            V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
          }
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const double apk = A[p][k], aqk = A[q][k];
            A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
          }
        }
      }
  }
  lam[0] = A[0][0]; lam[1] = A[1][1]; lam[2] = A[2][2];
  // sort descending by compare-exchange of (0,1), (0,2), (1,2): columns move with their eigenvalue
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = p + 1; q < 3; ++q)
      if (lam[q] > lam[p]) {
        const double tl = lam[p]; lam[p] = lam[q]; lam[q] = tl;
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double tv = V[k][p]; V[k][p] = V[k][q]; V[k][q] = tv; }
      }
}

// The right-handed frame of E: E ~ U diag(s1, s2, s3) V^T with u3 = u1 x u2, v3 = v1 x v2 (det U = det V = 1), u = columns.
// lam: the eigenvalues of E^T E (descending).  False when E has rank < 2.
CBA_HD bool essential_frame(const double* E, double* U, double* V, double* lam) {
  double S[3][3], W[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) S[r][c] = E[r] * E[c] + E[3 + r] * E[3 + c] + E[6 + r] * E[6 + c];
  sym3_eigen(S, lam, W);
  if (!(lam[0] > 0.0) || !pnp_finite(lam[0]) || !(lam[1] > 1e-20 * lam[0])) return false;
  double v0[3] = {W[0][0], W[1][0], W[2][0]}, v1[3] = {W[0][1], W[1][1], W[2][1]}, v2[3];
  double u0[3], u1[3], u2[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    u0[r] = E[3 * r] * v0[0] + E[3 * r + 1] * v0[1] + E[3 * r + 2] * v0[2];
    u1[r] = E[3 * r] * v1[0] + E[3 * r + 1] * v1[1] + E[3 * r + 2] * v1[2];
  }
  if (!normalize3(u0)) return false;
  const double d = u0[0] * u1[0] + u0[1] * u1[1] + u0[2] * u1[2];
  u1[0] -= d * u0[0]; u1[1] -= d * u0[1]; u1[2] -= d * u0[2];
  if (!normalize3(u1)) return false;
  cross3(u0, u1, u2);
  cross3(v0, v1, v2);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    U[3 * r] = u0[r]; U[3 * r + 1] = u1[r]; U[3 * r + 2] = u2[r];
    V[3 * r] = v0[r]; V[3 * r + 1] = v1[r]; V[3 * r + 2] = v2[r];
  }
  return true;
}

// E <- u1 v1^T + u2 v2^T (the nearest matrix with singular values (1, 1, 0) up to scale); cond = sigma_2 / sigma_1 before.
CBA_HD bool essential_project(double* E, double* cond) {
  double U[9], V[9], lam[3];
  if (!essential_frame(E, U, V, lam)) {
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = 0.0;
    *cond = 0.0;
    return false;
  }
  *cond = sqrt(fmax(lam[1], 0.0) / lam[0]);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) E[3 * r + c] = U[3 * r] * V[3 * c] + U[3 * r + 1] * V[3 * c + 1];
  return true;
}

// One row of the linear system x_b^T E x_a = 0 in the unknowns E (row-major)
CBA_HD void epi_row(double xa, double ya, double xb, double yb, double* a) {
  a[0] = xb * xa; a[1] = xb * ya; a[2] = xb;
  a[3] = yb * xa; a[4] = yb * ya; a[5] = yb;
  a[6] = xa;      a[7] = ya;      a[8] = 1.0;
}

// Linear 8-point fit (c[k] = xa, ya, xb, yb of sample k) on Hartley-normalised points (each view centred, mean distance
// sqrt(2)): the null vector of the 8 x 9 system by Householder QR of its transpose, x = H1 ... H8 e9, then
// E = T_b^T E' T_a back in normalised camera coordinates.  Unit norm.  False when not finite.
CBA_HD bool essential_8pt(const double (&c)[EPI_SAMPLE][4], double* E) {
  double m[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 8; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] += c[k][j];
#pragma unroll
  for (int j = 0; j < 4; ++j) m[j] *= 0.125;
  double da = 0.0, db = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    da += sqrt((c[k][0] - m[0]) * (c[k][0] - m[0]) + (c[k][1] - m[1]) * (c[k][1] - m[1]));
    db += sqrt((c[k][2] - m[2]) * (c[k][2] - m[2]) + (c[k][3] - m[3]) * (c[k][3] - m[3]));
  }
  if (!(da > 0.0) || !(db > 0.0)) return false;
  const double sa = 8.0 * 1.4142135623730951 / da, sb = 8.0 * 1.4142135623730951 / db;
  double M[9][8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    double a[9];
    epi_row(sa * (c[k][0] - m[0]), sa * (c[k][1] - m[1]), sb * (c[k][2] - m[2]), sb * (c[k][3] - m[3]), a);
#pragma unroll
    for (int r = 0; r < 9; ++r) M[r][k] = a[r];
  }
  double beta[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    double n2 = 0.0;
#pragma unroll
    for (int r = k; r < 9; ++r) n2 += M[r][k] * M[r][k];
    const double nrm = sqrt(n2);
    const double alpha = M[k][k] >= 0.0 ? -nrm : nrm;
    M[k][k] -= alpha;  // Householder vector v in column k, rows k..8
    double vv = 0.0;
#pragma unroll
    for (int r = k; r < 9; ++r) vv += M[r][k] * M[r][k];
    beta[k] = vv > 0.0 ? 2.0 / vv : 0.0;
#pragma unroll
    for (int cc = k + 1; cc < 8; ++cc) {
      double s = 0.0;
#pragma unroll
      for (int r = k; r < 9; ++r) s += M[r][k] * M[r][cc];
      s *= beta[k];
#pragma unroll
      for (int r = k; r < 9; ++r) M[r][cc] -= s * M[r][k];
    }
  }
  double x[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) x[r] = (r == 8) ? 1.0 : 0.0;
#pragma unroll
  for (int k = 7; k >= 0; --k) {
    double s = 0.0;
#pragma unroll
    for (int r = k; r < 9; ++r) s += M[r][k] * x[r];
    s *= beta[k];
#pragma unroll
    for (int r = k; r < 9; ++r) x[r] -= s * M[r][k];
  }
  // E = T_b^T E' T_a, T = [s 0 -s m0; 0 s -s m1; 0 0 1]
  double P[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    P[3 * r] = x[3 * r] * sa;
    P[3 * r + 1] = x[3 * r + 1] * sa;
    P[3 * r + 2] = x[3 * r + 2] - x[3 * r] * sa * m[0] - x[3 * r + 1] * sa * m[1];
  }
#pragma unroll
  for (int cc = 0; cc < 3; ++cc) {
    x[cc] = sb * P[cc];
    x[3 + cc] = sb * P[3 + cc];
    x[6 + cc] = P[6 + cc] - sb * m[2] * P[cc] - sb * m[3] * P[3 + cc];
  }
  double n2 = 0.0;
#pragma unroll
  for (int r = 0; r < 9; ++r) n2 += x[r] * x[r];
  if (!(n2 > 0.0) || !pnp_finite(n2)) return false;
  const double inv = 1.0 / sqrt(n2);
#pragma unroll
  for (int r = 0; r < 9; ++r) E[r] = x[r] * inv;
  return true;
}

// The hypothesis of an 8-point sample: linear fit projected onto the manifold (E = 0 when degenerate).
CBA_HD void essential_hypothesis(const double (&c)[EPI_SAMPLE][4], double* E) {
  double cond;
  if (!essential_8pt(c, E)) {
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = 0.0;
    return;
  }
  essential_project(E, &cond);
}

// The four (R, t) of E, candidate k: R = U W V^T (k even) or U W^T V^T (k odd), t = u3 (k < 2) or -u3.  rt: R row-major, t.
CBA_HD bool essential_candidates(const double* E, double (&rt)[4][12]) {
  double U[9], V[9], lam[3];
  if (!essential_frame(E, U, V, lam)) return false;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      // U W = [u2, -u1, u3], U W^T = [-u2, u1, u3]
      const double a = U[3 * r + 1] * V[3 * c] - U[3 * r] * V[3 * c + 1] + U[3 * r + 2] * V[3 * c + 2];
      const double b = -U[3 * r + 1] * V[3 * c] + U[3 * r] * V[3 * c + 1] + U[3 * r + 2] * V[3 * c + 2];
      rt[0][3 * r + c] = a; rt[2][3 * r + c] = a;
      rt[1][3 * r + c] = b; rt[3][3 * r + c] = b;
    }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    rt[0][9 + r] = U[3 * r + 2]; rt[1][9 + r] = U[3 * r + 2];
    rt[2][9 + r] = -U[3 * r + 2]; rt[3][9 + r] = -U[3 * r + 2];
  }
  return true;
}

// recoverPose's test of one correspondence under (R, t): the two-view point has 0 < depth < 50 in both views.
// w: the homogeneous point.
CBA_HD bool epi_in_front(const double* rt, double xa, double ya, double xb, double yb, double* w) {
  two_view_dlt(rt, xa, ya, xb, yb, w);
  if (!(w[2] * w[3] > 0.0)) return false;
  const double X = w[0] / w[3], Y = w[1] / w[3], Z = w[2] / w[3];
  if (!(Z < EPI_DIST_THRESH)) return false;
  const double zb = rt[6] * X + rt[7] * Y + rt[8] * Z + rt[11];
  return zb > 0.0 && zb < EPI_DIST_THRESH;
}

// E = [t]x R
CBA_HD void essential_from_pose(const double* R, const double* t, double* E) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    E[c] = t[1] * R[6 + c] - t[2] * R[3 + c];
    E[3 + c] = t[2] * R[c] - t[0] * R[6 + c];
    E[6 + c] = t[0] * R[3 + c] - t[1] * R[c];
  }
}

// Tangent basis (b1, b2) of S^2 at unit t: b1 = t x e / |.| with e the axis least aligned with t, b2 = t x b1.
CBA_HD void sphere_basis(const double* t, double* b1, double* b2) {
  const double a0 = fabs(t[0]), a1 = fabs(t[1]), a2 = fabs(t[2]);
  const double e[3] = {(a0 <= a1 && a0 <= a2) ? 1.0 : 0.0, (!(a0 <= a1 && a0 <= a2) && a1 <= a2) ? 1.0 : 0.0,
                       (!(a0 <= a1 && a0 <= a2) && !(a1 <= a2)) ? 1.0 : 0.0};
  cross3(t, e, b1);
  normalize3(b1);
  cross3(t, b1, b2);
}

// The derivatives of E = [t]x R by the 5 parameters at (R, t): dE[k] for the left rotation increment w_k (k < 3) and the
// tangent step along b_{k-2} (k >= 3).
CBA_HD void essential_jacobian(const double* R, const double* t, double (&dE)[5][9]) {
  double b1[3], b2[3];
  sphere_basis(t, b1, b2);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    // [e_k]x R, then [t]x of that
    double ek[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
    double G[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      G[c] = ek[1] * R[6 + c] - ek[2] * R[3 + c];
      G[3 + c] = ek[2] * R[c] - ek[0] * R[6 + c];
      G[6 + c] = ek[0] * R[3 + c] - ek[1] * R[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      dE[k][c] = t[1] * G[6 + c] - t[2] * G[3 + c];
      dE[k][3 + c] = t[2] * G[c] - t[0] * G[6 + c];
      dE[k][6 + c] = t[0] * G[3 + c] - t[1] * G[c];
    }
  }
  essential_from_pose(R, b1, dE[3]);
  essential_from_pose(R, b2, dE[4]);
}

// acc[0..14] += J^T J (packed 5 x 5), acc[15..19] += J^T r, acc[20] += r^2 for the Sampson residual r = N / sqrt(D2) of one
// correspondence.
CBA_HD void epi_sampson_normal(const double* E, const double (&dE)[5][9], double xa, double ya, double xb, double yb, double* acc) {
  const double ex0 = E[0] * xa + E[1] * ya + E[2];
  const double ex1 = E[3] * xa + E[4] * ya + E[5];
  const double ex2 = E[6] * xa + E[7] * ya + E[8];
  const double et0 = E[0] * xb + E[3] * yb + E[6];
  const double et1 = E[1] * xb + E[4] * yb + E[7];
  const double num = xb * ex0 + yb * ex1 + ex2;
  const double d2 = ex0 * ex0 + ex1 * ex1 + et0 * et0 + et1 * et1;
  if (!(d2 > 0.0)) return;
  const double dd = sqrt(d2);
  const double r = num / dd;
  const double xav[3] = {xa, ya, 1.0}, xbv[3] = {xb, yb, 1.0};
  const double exv[3] = {ex0, ex1, 0.0}, etv[3] = {et0, et1, 0.0};
  // dr/dE_mn = (xb_m xa_n - r (ex_m xa_n [m<2] + et_n xb_m [n<2]) / D) / D
  double g[5] = {0, 0, 0, 0, 0};
  const double id = 1.0 / dd;
#pragma unroll
  for (int m = 0; m < 3; ++m)
#pragma unroll
    for (int n = 0; n < 3; ++n) {
      const double dr = (xbv[m] * xav[n] - r * (exv[m] * xav[n] + etv[n] * xbv[m]) * id) * id;
#pragma unroll
      for (int k = 0; k < 5; ++k) g[k] += dr * dE[k][3 * m + n];
    }
#pragma unroll
  for (int i = 0; i < 5; ++i) {
#pragma unroll
    for (int k = 0; k <= i; ++k) acc[i * (i + 1) / 2 + k] += g[i] * g[k];
    acc[15 + i] += g[i] * r;
  }
  acc[20] += r * r;
}

// acc[0..44] += a a^T (packed 9 x 9) for the linear-fit row a of one correspondence
CBA_HD void epi_linear_normal(double xa, double ya, double xb, double yb, double* acc) {
  double a[9];
  epi_row(xa, ya, xb, yb, a);
#pragma unroll
  for (int i = 0; i < 9; ++i)
#pragma unroll
    for (int k = 0; k <= i; ++k) acc[i * (i + 1) / 2 + k] += a[i] * a[k];
}

// Levenberg-Marquardt on the Sampson residuals.  sum(R, t, acc) fills acc[EPI_NSUM] with the sums of epi_sampson_normal over
// the inliers at (R, t) (every thread of a workgroup calls it with the same arguments and gets the same sums).  Returns the
// final cost (non-finite: failed); R, t (unit) updated in place.
template <class Sum>
CBA_HD double epi_refine(Sum& sum, double* R, double* t) {
  double acc[EPI_NSUM];
  sum(R, t, acc);
  double cost = acc[20];
  if (!pnp_finite(cost)) return cost;
  double mu = 1e-3;
  for (int it = 0; it < EPI_LM_MAX_ITER; ++it) {
    double A[15], d[5];
    double dmax = 0.0;
#pragma unroll
    for (int k = 0; k < 5; ++k) dmax = fmax(dmax, acc[k * (k + 1) / 2 + k]);
#pragma unroll
    for (int k = 0; k < 15; ++k) A[k] = acc[k];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      A[k * (k + 1) / 2 + k] += mu * fmax(acc[k * (k + 1) / 2 + k], 1e-12 * dmax);
      d[k] = -acc[15 + k];
    }
    if (chol_solve<5>(A, d)) {
      double b1[3], b2[3], Ex[9], Rn[9], tn[3];
      sphere_basis(t, b1, b2);
      rot_exp(d, Ex);
      mat3_mul(Ex, R, Rn);
#pragma unroll
      for (int k = 0; k < 3; ++k) tn[k] = t[k] + d[3] * b1[k] + d[4] * b2[k];
      double accn[EPI_NSUM];
      const bool okn = normalize3(tn);
      if (okn) sum(Rn, tn, accn);
      const double cn = okn ? accn[20] : cost;
      if (okn && pnp_finite(cn) && cn < cost) {
        const bool small = fmax(fabs(d[0]), fmax(fabs(d[1]), fabs(d[2]))) <= 1e-13 && fmax(fabs(d[3]), fabs(d[4])) <= 1e-13;
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = Rn[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = tn[k];
#pragma unroll
        for (int k = 0; k < EPI_NSUM; ++k) acc[k] = accn[k];
        cost = cn;
        mu = fmax(mu * 0.1, 1e-15);
        if (small) break;
        continue;
      }
    }
    mu *= 10.0;
    if (mu > 1e16) break;
  }
  return cost;
}

// sigma_2 / sigma_1 of the null vector of the packed 9 x 9 normal matrix N (overwritten), by inverse iteration from E0.
CBA_HD double epi_conditioning(const double* N, const double* E0) {
  double x[9];
  double dmax = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) { x[k] = E0[k]; dmax = fmax(dmax, N[k * (k + 1) / 2 + k]); }
  if (!(dmax > 0.0) || !pnp_finite(dmax)) return 0.0;
  for (int it = 0; it < 4; ++it) {
    double A[45];
#pragma unroll
    for (int k = 0; k < 45; ++k) A[k] = N[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) A[k * (k + 1) / 2 + k] += 1e-9 * dmax;
    if (!chol_solve<9>(A, x)) return 0.0;
    double n2 = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) n2 += x[k] * x[k];
    if (!(n2 > 0.0) || !pnp_finite(n2)) return 0.0;
    const double inv = 1.0 / sqrt(n2);
#pragma unroll
    for (int k = 0; k < 9; ++k) x[k] *= inv;
  }
  double U[9], V[9], lam[3];
  if (!essential_frame(x, U, V, lam)) return 0.0;
  return sqrt(fmax(lam[1], 0.0) / lam[0]);
}

// ---- resection -------------------------------------------------------------------------------------------------------------

// |u - proj(R X + t)|^2, +huge when the point is not in front of the camera
CBA_HD double res_err2(const double* R, const double* t, const double* X, double u, double v) {
  const double x = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0];
  const double y = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1];
  const double z = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
  if (!(z > 0.0)) return 1e300;
  const double iz = 1.0 / z;
  const double rx = x * iz - u, ry = y * iz - v;
  return rx * rx + ry * ry;
}

// |u - proj(R X + t)| whatever the depth (the error the score takes its median of)
CBA_HD double res_err(const double* R, const double* t, const double* X, double u, double v) {
  const double x = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0];
  const double y = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1];
  const double z = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
  const double rx = x / z - u, ry = y / z - v;
  return sqrt(rx * rx + ry * ry);
}

// The hypothesis of a 6-point sample (P[k] = X, Y, Z, u, v): DLT on the centred, scaled sample, pose of the original points.
CBA_HD bool res_hypothesis(const double (&P)[RES_SAMPLE][5], double* R, double* t) {
  double cen[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < RES_SAMPLE; ++k) { cen[0] += P[k][0]; cen[1] += P[k][1]; cen[2] += P[k][2]; }
  const double inv_n = 1.0 / RES_SAMPLE;
  cen[0] *= inv_n; cen[1] *= inv_n; cen[2] *= inv_n;
  double s_o = 0.0;
#pragma unroll
  for (int k = 0; k < RES_SAMPLE; ++k) {
    const double dx = P[k][0] - cen[0], dy = P[k][1] - cen[1], dz = P[k][2] - cen[2];
    s_o += sqrt(dx * dx + dy * dy + dz * dz);
  }
  s_o *= inv_n;
  if (!(s_o > 0.0) || !pnp_finite(s_o)) return false;
  double A[66], p[11];
#pragma unroll
  for (int k = 0; k < 66; ++k) A[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 11; ++k) p[k] = 0.0;
  const double io = 1.0 / s_o;
#pragma unroll
  for (int k = 0; k < RES_SAMPLE; ++k) {
    const double x = (P[k][0] - cen[0]) * io, y = (P[k][1] - cen[1]) * io, z = (P[k][2] - cen[2]) * io;
    const double u = P[k][3], v = P[k][4];
    const double ru[11] = {x, y, z, 1.0, 0.0, 0.0, 0.0, 0.0, -u * x, -u * y, -u * z};
    const double rv[11] = {0.0, 0.0, 0.0, 0.0, x, y, z, 1.0, -v * x, -v * y, -v * z};
    normal_add<11>(A, p, ru, u);
    normal_add<11>(A, p, rv, v);
  }
  if (!pnp_dlt_finish(A, p, s_o, R, t)) return false;
  const double tc0 = t[0], tc1 = t[1], tc2 = t[2];
  t[0] = tc0 - (R[0] * cen[0] + R[1] * cen[1] + R[2] * cen[2]);
  t[1] = tc1 - (R[3] * cen[0] + R[4] * cen[1] + R[5] * cen[2]);
  t[2] = tc2 - (R[6] * cen[0] + R[7] * cen[1] + R[8] * cen[2]);
  bool fin = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) fin = fin && pnp_finite(R[k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) fin = fin && pnp_finite(t[k]);
  return fin;
}

// acc[0..20] += J^T J (packed 6 x 6), acc[21..26] += J^T r, acc[27] += |r|^2: pnp_cost's terms for one point (no centring)
CBA_HD void res_point_normal(const double* R, const double* t, const double* X, double u, double v, double* acc) {
  const double a0 = R[0] * X[0] + R[1] * X[1] + R[2] * X[2];
  const double a1 = R[3] * X[0] + R[4] * X[1] + R[5] * X[2];
  const double a2 = R[6] * X[0] + R[7] * X[1] + R[8] * X[2];
  const double x = a0 + t[0], y = a1 + t[1], z = a2 + t[2];
  const double iz = 1.0 / z;
  const double px = x * iz, py = y * iz;
  const double rx = px - u, ry = py - v;
  double jx[6], jy[6];
  jx[0] = iz * (-px * a1);           jy[0] = iz * (-a2 - py * a1);
  jx[1] = iz * (a2 + px * a0);       jy[1] = iz * (py * a0);
  jx[2] = iz * (-a1);                jy[2] = iz * (a0);
  jx[3] = iz;                        jy[3] = 0.0;
  jx[4] = 0.0;                       jy[4] = iz;
  jx[5] = -iz * px;                  jy[5] = -iz * py;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
#pragma unroll
    for (int c = 0; c <= r; ++c) acc[r * (r + 1) / 2 + c] += jx[r] * jx[c] + jy[r] * jy[c];
    acc[21 + r] += jx[r] * rx + jy[r] * ry;
  }
  acc[27] += rx * rx + ry * ry;
}

// pnp_refine over `Sum` (acc[RES_NSUM] of res_point_normal over the inliers at (R, t)): Levenberg-Marquardt, then the
// Gauss-Newton polish.  Returns the final cost (non-finite: failed).
template <class Sum>
CBA_HD double res_refine(Sum& sum, double* R, double* t) {
  double acc[RES_NSUM];
  sum(R, t, acc);
  double cost = acc[27];
  if (!pnp_finite(cost)) return cost;
  double mu = 1e-3;
  for (int it = 0; it < PNP_LM_MAX_ITER; ++it) {
    double A[21], d[6];
    double dmax = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) dmax = fmax(dmax, acc[k * (k + 1) / 2 + k]);
#pragma unroll
    for (int k = 0; k < 21; ++k) A[k] = acc[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      A[k * (k + 1) / 2 + k] += mu * fmax(acc[k * (k + 1) / 2 + k], 1e-12 * dmax);
      d[k] = -acc[21 + k];
    }
    if (chol_solve<6>(A, d)) {
      double Ex[9], Rn[9], tn[3], accn[RES_NSUM];
      rot_exp(d, Ex);
      mat3_mul(Ex, R, Rn);
      tn[0] = t[0] + d[3]; tn[1] = t[1] + d[4]; tn[2] = t[2] + d[5];
      sum(Rn, tn, accn);
      const double cn = accn[27];
      if (pnp_finite(cn) && cn < cost) {
        const double tabs = fmax(fabs(t[0]), fmax(fabs(t[1]), fabs(t[2])));
        const bool small = fmax(fabs(d[0]), fmax(fabs(d[1]), fabs(d[2]))) <= 1e-13 &&
                           fmax(fabs(d[3]), fmax(fabs(d[4]), fabs(d[5]))) <= 1e-13 * (1.0 + tabs);
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = Rn[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = tn[k];
#pragma unroll
        for (int k = 0; k < RES_NSUM; ++k) acc[k] = accn[k];
        cost = cn;
        mu = fmax(mu * 0.1, 1e-15);
        if (small) break;
        continue;
      }
    }
    mu *= 10.0;
    if (mu > 1e16) break;
  }
  double prev = 1e300;
  for (int it = 0; it < PNP_POLISH_ITER; ++it) {
    double A[21], d[6];
#pragma unroll
    for (int k = 0; k < 21; ++k) A[k] = acc[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) d[k] = -acc[21 + k];
    if (!chol_solve<6>(A, d)) break;
    double dn = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) dn = fmax(dn, fabs(d[k]));
    if (!(dn < 0.5 * prev) || dn == 0.0) break;
    double Ex[9], Rn[9], tn[3], accn[RES_NSUM];
    rot_exp(d, Ex);
    mat3_mul(Ex, R, Rn);
    tn[0] = t[0] + d[3]; tn[1] = t[1] + d[4]; tn[2] = t[2] + d[5];
    sum(Rn, tn, accn);
    const double cn = accn[27];
    if (!pnp_finite(cn) || cn > cost * (1.0 + 1e-10)) break;
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = Rn[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = tn[k];
#pragma unroll
    for (int k = 0; k < RES_NSUM; ++k) acc[k] = accn[k];
    cost = cn < cost ? cn : cost;
    prev = dn;
  }
  return cost;
}

// The fixed reduction tree both builds use for a workgroup of NT threads (NT a power of two): thread `tid` sums items
// tid, tid + NT, ... in order; then part[t] += part[t + s] for s = NT/2, NT/4, ..., 1.
constexpr int EPI_REDUCE_NT = 128;

}  // namespace cba
