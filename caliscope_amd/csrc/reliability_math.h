// Per-element arithmetic of cba_observation_reliability (include/caliscope/reliability.h): the pieces of the 2 x 2 block
//     P_oo = J_o (J^T J)^- J_o^T = B_o (V_i^-1 + Q_i) B_o^T + A_o C_aa A_o^T - A_o G_o B_o^T - (A_o G_o B_o^T)^T
// of one observation o (camera a, point i), its redundancy block R_oo = I - P_oo and the standardised residuals.  Notation of
// covariance_math.h; Q_i = sum_b Y_b^T G_b, G_o = sum_b' C_{a,cam(b')} Y_b' (b, b' over the observations of point i).  J (J^T J)^- J^T is
// the same for every generalised inverse, so the gauge terms E, F, Z of the point covariance do not appear.  G_o is formed row by row:
// row r needs the nine-wide pieces of row (off_a + r) of C at the cameras of the point, and contributes Y_o[r]^T g to Q_i,
// A_o[:, r] g to A_o G_o and A_o[:, r] (C_aa A_o^T)[r] to A_o C_aa A_o^T.  Compiled by hipcc into reliability_lib.hip and by g++ into
// tests/native/reliability_harness.cpp.  Loops have constant bounds and static indices (nothing here may live in scratch memory).
#pragma once
#include "covariance_math.h"
#include "../../include/caliscope/reliability.h"

namespace cba {

constexpr double REL_R_TINY = 1e-10;  // a row with r_j at or below this is uncontrolled: its w is NaN
constexpr int REL_GROUP = 16;         // lanes of k_rel_point that share one observation (one per row of G_o, nine of them live)

// g += (row piece of C at camera b') Y_b': crow the np_b entries of the row, Yb 9 x 3 row-major
CBA_HD void rel_row_times_y(const double* crow, int np_b, const double* Yb, double* g) {
#pragma unroll
  for (int c = 0; c < MAX_NC; ++c) {
    const double cv = c < np_b ? crow[c] : 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) g[q] += cv * Yb[3 * c + q];
  }
}

// h = (row piece of C at the observation's own camera) A_o^T
CBA_HD void rel_row_times_a(const double* crow, int np_a, const double (*A)[MAX_NC], double* h) {
  h[0] = 0.0; h[1] = 0.0;
#pragma unroll
  for (int c = 0; c < MAX_NC; ++c) {
    const double cv = c < np_a ? crow[c] : 0.0;
    h[0] += cv * A[0][c];
    h[1] += cv * A[1][c];
  }
}

// column r of A, picked with static indices
CBA_HD void rel_a_column(const double (*A)[MAX_NC], int r, double* a) {
  a[0] = 0.0; a[1] = 0.0;
#pragma unroll
  for (int c = 0; c < MAX_NC; ++c)
    if (c == r) { a[0] = A[0][c]; a[1] = A[1][c]; }
}

// What row r of G_o adds to the sums: Q (3 x 3, row-major) += Y_o[r]^T g; M (2 x 3) += A_o[:, r] g; S (uu, uv + vu, vv) += A_o[:, r] h
CBA_HD void rel_row_terms(const double* a, const double* yr, const double* g, const double* h, double* Q, double* M, double* S) {
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int q = 0; q < 3; ++q) Q[3 * p + q] += yr[p] * g[q];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int q = 0; q < 3; ++q) M[3 * j + q] += a[j] * g[q];
  S[0] += a[0] * h[0];
  S[1] += a[0] * h[1] + a[1] * h[0];
  S[2] += a[1] * h[1];
}

// the camera part of P_oo (uu, uv, vv): A C_aa A^T - M B^T - (M B^T)^T with M = A_o G_o
CBA_HD void rel_camera_part(const double* S, const double* M, const double (*B)[3], double* T) {
  double MB[2][2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int m = 0; m < 2; ++m) MB[j][m] = M[3 * j] * B[m][0] + M[3 * j + 1] * B[m][1] + M[3 * j + 2] * B[m][2];
  T[0] = S[0] - 2.0 * MB[0][0];
  T[1] = 0.5 * S[1] - (MB[0][1] + MB[1][0]);
  T[2] = S[2] - 2.0 * MB[1][1];
}

// standardised residual of one row: NaN for an uncontrolled row, r clamped to [0, 1] for the square root only
CBA_HD double rel_w(double f_scaled, double r, double sigma0) {
  if (!(r > REL_R_TINY)) return __builtin_nan("");
  const double rc = r > 1.0 ? 1.0 : r;
  return f_scaled / (sigma0 * sqrt(rc));
}

// The point part B_o (V^-1 + sym Q) B_o^T added to the camera part T, R_oo = I - P_oo (uu, uv, vv; not clamped) and the two w.
// Returns the number of uncontrolled rows (0, 1 or 2).
CBA_HD int rel_finish(const double (*B)[3], const double* Vi, const double* Q, const double* T, double sigma0, const double* f_scaled, double* R, double* w) {
  double K[3][3], BK[2][3];
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int q = 0; q < 3; ++q) K[p][q] = cov_sym3(Vi, p, q) + 0.5 * (Q[3 * p + q] + Q[3 * q + p]);
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int q = 0; q < 3; ++q) BK[j][q] = B[j][0] * K[0][q] + B[j][1] * K[1][q] + B[j][2] * K[2][q];
  const double p00 = BK[0][0] * B[0][0] + BK[0][1] * B[0][1] + BK[0][2] * B[0][2];
  const double p01 = BK[0][0] * B[1][0] + BK[0][1] * B[1][1] + BK[0][2] * B[1][2];
  const double p11 = BK[1][0] * B[1][0] + BK[1][1] * B[1][1] + BK[1][2] * B[1][2];
  R[0] = 1.0 - (p00 + T[0]);
  R[1] = -(p01 + T[1]);
  R[2] = 1.0 - (p11 + T[2]);
  w[0] = rel_w(f_scaled[0], R[0], sigma0);
  w[1] = rel_w(f_scaled[1], R[2], sigma0);
  return (R[0] > REL_R_TINY ? 0 : 1) + (R[2] > REL_R_TINY ? 0 : 1);
}

}  // namespace cba
