// Per-element arithmetic of cba_observation_reliability_constrained (include/caliscope/reliability_constrained.h): the diagonal of the
// projector P = J G^- J^T of a problem WITH rigid-distance rows, G^- = [[C, -C Y], [-Y^T C, V~^-1 + Y^T C Y]] (a generalised inverse of
// J^T J: the gauge terms E, F, Z do not appear, as in reliability_math.h).  Notation of covariance_constraint_math.h: X = L^-1 of a
// component's V~_k (packed lower triangle), Y_c = W_c,k V~_k^-1 stored per (constrained point, component camera) entry as a 9 x 3 block,
// a constraint row c_j = sum_s coef[s] (e_loc[s] (x) u).
//   observation o (camera a) of a constrained point i:  P_oo = B_o([V~_k^-1]_ii + Q_i)B_o^T + A_o C_aa A_o^T - sym(A_o G_e(a) B_o^T),
//       G_e = sum_e' C_{cam(e),cam(e')} Yc[e'],  Q_i = sum_e Yc[e]^T G_e  (e, e' over the entries of point i);
//   constraint row j of component k:  P_jj = |X c_j^T|^2 + sum_cc' v_c^T C_cc' v_c',  v_c = Y_c c_j^T.
// Compiled by hipcc into covariance_lib.hip (rel_con_x_row: k_unc_component) and reliability_lib.hip, and by g++ into
// tests/native/reliability_constrained_harness.cpp.  Loops have constant bounds and static indices (nothing here may live in scratch memory).
#pragma once
#include "covariance_constraint_math.h"
#include "reliability_math.h"
#include "../../include/caliscope/reliability_constrained.h"

namespace cba {

// entry i of q = X c_j^T: loc[8] the slots' points as positions in the component, coef[8], u[3] as cov_con_row leaves them
CBA_HD double rel_con_x_row(const double* X, int i, const int32_t* loc, const double* coef, const double* u) {
  const double* x = X + cov_tri(i, 0);
  double q = 0.0;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    if (coef[s] != 0.0) {
      const int c0 = 3 * loc[s];
#pragma unroll
      for (int a = 0; a < 3; ++a)
        if (c0 + a <= i) q += coef[s] * x[c0 + a] * u[a];
    }
  }
  return q;
}

// entry r of v_c = Y_c c_j^T for the c-th camera of the component: e0[s] the first entry of slot s's point
CBA_HD double rel_con_v_entry(const double* Yc, const int64_t* e0, int c, int r, const double* coef, const double* u) {
  double v = 0.0;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    if (coef[s] != 0.0) {
      const double* y = Yc + (e0[s] + c) * (3 * MAX_NC) + 3 * r;
      v += coef[s] * (y[0] * u[0] + y[1] * u[1] + y[2] * u[2]);
    }
  }
  return v;
}

// (row piece of C at camera c') v_c': crow the np_b entries of the row, one double at a time (rows of C start at multiples of three doubles)
CBA_HD double rel_con_row_dot(const double* crow, int np_b, const double* vb) {
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < MAX_NC; ++c) s += c < np_b ? crow[c] * vb[c] : 0.0;
  return s;
}

// the scaled residual f~ of a constraint row (cov_con_row's residual through robust_one)
CBA_HD double rel_con_residual(const double* points, const int32_t* pt, double dist, double weight, int loss, double f_scale) {
  double a[3] = {0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int64_t pa = pt[s], pb = pt[4 + s];
#pragma unroll
    for (int k = 0; k < 3; ++k) { a[k] += points[3 * pa + k]; b[k] += points[3 * pb + k]; }
  }
  double n2 = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) { const double dl = 0.25 * (a[k] - b[k]); n2 += dl * dl; }
  double js, rs;
  robust_one(loss, f_scale, (sqrt(n2) - dist) * weight, &js, &rs);
  return rs;
}

// What row r of G_e adds to Q_i (3 x 3, row-major): Yc[e][r]^T g
CBA_HD void rel_con_q_terms(const double* yr, const double* g, double* Q) {
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int q = 0; q < 3; ++q) Q[3 * p + q] += yr[p] * g[q];
}

// What row r of G_e(a) adds to the camera part of an observation: M (2 x 3) += A_o[:, r] g; S (uu, uv + vu, vv) += A_o[:, r] h
CBA_HD void rel_con_obs_terms(const double* a, const double* g, const double* h, double* M, double* S) {
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int q = 0; q < 3; ++q) M[3 * j + q] += a[j] * g[q];
  S[0] += a[0] * h[0];
  S[1] += a[0] * h[1] + a[1] * h[0];
  S[2] += a[1] * h[1];
}

// r_j = 1 - (s_j + v^T C v) (not clamped) and w_j of a constraint row; returns 1 for an uncontrolled row
CBA_HD int rel_con_finish(double s, double quad, double f_scaled, double sigma0, double* r, double* w) {
  *r = 1.0 - (s + quad);
  *w = rel_w(f_scaled, *r, sigma0);
  return *r > REL_R_TINY ? 0 : 1;
}

}  // namespace cba
