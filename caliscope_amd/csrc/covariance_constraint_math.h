// Per-element arithmetic of the constraint rows and of the per-component dense blocks of cba_parameter_covariance_constrained
// (include/caliscope/uncertainty_constrained.h).  Compiled by hipcc into covariance_lib.hip, where the loops over the elements are spread
// over the threads of a workgroup, and by g++ into tests/native/covariance_constrained_harness.cpp, where they run one after the other.
//
// A component of m points has the symmetric n x n matrix V~_k, n = 3 m, kept as its packed lower triangle: entry (i, j), j <= i, at
// cov_tri(i, j).  It is factored in place (V~_k = L L^T), L is inverted in place (X = L^-1, lower), and everything after that is a product
// with X: V~_k^-1 = X^T X, so Z = X^T (X Np), Y_c^T = X^T (X W_c^T) and [V~_k^-1]_ii = (X^T X)_ii.  Loops have constant bounds and static
// indices wherever an array could otherwise live in scratch memory on the device.
#pragma once
#include <cmath>
#include <cstdint>

#include "ba_math.h"
#include "covariance_math.h"

namespace cba {

// One constraint row r = weight (|| mean X[a] - mean X[b] || - distance) at `points` ([n_points][3]), `pt` its eight point indices (a then b):
// the residual goes through robust_one like every row of the solver (cba_set_constraints).  u[3] = weight * row scale * unit vector; coef[s]
// is the signed multiplicity of slot s's point among the eight slots in quarters (+ for a, - for b), given to the FIRST slot that names the
// point and zero for the others, so the Jacobian row is sum_s coef[s] (e_pt[s] (x) u).  Coincident endpoints: unit = 0 (the solver's
// subgradient), a zero Jacobian row.  Returns rho (cost = 0.5 sum).
CBA_HD double cov_con_row(const double* points, const int32_t* pt, double dist, double weight, int loss, double f_scale, double* u, double* coef) {
  double a[3] = {0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int64_t pa = pt[s], pb = pt[4 + s];
#pragma unroll
    for (int k = 0; k < 3; ++k) { a[k] += points[3 * pa + k]; b[k] += points[3 * pb + k]; }
  }
  double dlt[3], n2 = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) { dlt[k] = 0.25 * (a[k] - b[k]); n2 += dlt[k] * dlt[k]; }
  const double nrm = sqrt(n2);
  const double inv = nrm > 0.0 ? 1.0 / nrm : 0.0;
  double js, rs;
  const double rho = robust_one(loss, f_scale, (nrm - dist) * weight, &js, &rs);
  const double w = weight * js;
#pragma unroll
  for (int k = 0; k < 3; ++k) u[k] = dlt[k] * inv * w;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    bool first = true;
    double mult = 0.0;
#pragma unroll
    for (int s2 = 0; s2 < 8; ++s2)
      if (pt[s2] == pt[s]) { if (s2 < s) first = false; mult += (s2 < 4) ? 0.25 : -0.25; }
    coef[s] = first ? mult : 0.0;
  }
  return rho;
}

// position of entry (i, j), j <= i, in a packed lower triangle
CBA_HD int cov_tri(int i, int j) { return i * (i + 1) / 2 + j; }

// a pivot of V~_k against the diagonal entry it started from (chol3's rule)
CBA_HD bool cov_con_pivot_ok(double d, double d0) { return d > 16.0 * EPS_F64 * d0 && d < 1.7e308; }

// (X R)[i][col] for X lower (packed) and R row-major with `ld` columns
CBA_HD double cov_tri_lower_dot(const double* X, int i, const double* R, int ld, int col) {
  double s = 0.0;
  const double* x = X + cov_tri(i, 0);
  for (int t = 0; t <= i; ++t) s += x[t] * R[t * ld + col];
  return s;
}

// (X^T P)[j][col] for X lower (packed, n rows) and P row-major with `ld` columns
CBA_HD double cov_tri_upper_dot(const double* X, int n, int j, const double* P, int ld, int col) {
  double s = 0.0;
  for (int t = j; t < n; ++t) s += X[cov_tri(t, j)] * P[t * ld + col];
  return s;
}

// (X^T X)[i][j] for X lower (packed, n rows)
CBA_HD double cov_tri_gram(const double* X, int n, int i, int j) {
  double s = 0.0;
  for (int t = (i > j ? i : j); t < n; ++t) s += X[cov_tri(t, i)] * X[cov_tri(t, j)];
  return s;
}

// entry i > j of column j of X = L^-1 once the columns behind j are inverted in place: -(sum_{t = j + 1 .. i} X[i][t] col[t]) / L[j][j], with
// col[t] = L[t][j] saved before the column is overwritten
CBA_HD double cov_tri_inverse_entry(const double* X, int i, int j, const double* col, double xjj) {
  double s = 0.0;
  const double* x = X + cov_tri(i, 0);
  for (int t = j + 1; t <= i; ++t) s += x[t] * col[t];
  return -s * xjj;
}

// (a, b), a <= b, of entry e of a symmetric 3 x 3 stored xx xy xz yy yz zz
CBA_HD int cov_sym3_row(int e) { return e < 3 ? 0 : (e < 5 ? 1 : 2); }
CBA_HD int cov_sym3_col(int e) { return e < 3 ? e : (e < 5 ? e - 2 : 2); }

// ---- host only: the serial forms of what a workgroup does with barriers --------------------------------------------------------------

// V~_k = L L^T in place; false when a pivot is not safely positive.  diag0: the n diagonal entries before the factorisation.
inline bool cov_tri_cholesky(double* V, int n, const double* diag0) {
  for (int j = 0; j < n; ++j) {
    const double d = V[cov_tri(j, j)];
    if (!cov_con_pivot_ok(d, diag0[j])) return false;
    const double ljj = std::sqrt(d);
    V[cov_tri(j, j)] = ljj;
    for (int i = j + 1; i < n; ++i) V[cov_tri(i, j)] /= ljj;
    for (int i = j + 1; i < n; ++i)
      for (int c = j + 1; c <= i; ++c) V[cov_tri(i, c)] -= V[cov_tri(i, j)] * V[cov_tri(c, j)];
  }
  return true;
}

// X = L^-1 in place, from the last column to the first; col: n doubles of work space
inline void cov_tri_invert(double* L, int n, double* col) {
  for (int j = n - 1; j >= 0; --j) {
    const double xjj = 1.0 / L[cov_tri(j, j)];
    for (int i = j + 1; i < n; ++i) col[i] = L[cov_tri(i, j)];
    for (int i = j + 1; i < n; ++i) L[cov_tri(i, j)] = cov_tri_inverse_entry(L, i, j, col, xjj);
    L[cov_tri(j, j)] = xjj;
  }
}

}  // namespace cba
