// Per-element arithmetic and host-side checks of cba_parameter_covariance (include/caliscope/uncertainty.h): the gauge columns of a
// camera and of a point, the Jacobian products of one observation, the 3 x 3 pieces of one point, and on the host the validation with
// the point-sorted order, the inverse of the 7 x 7 gauge matrix D, the rank-7 terms of the point formula, the refusal texts and the
// camera outputs.  Compiled by hipcc into covariance_lib.hip and by g++ into tests/native/covariance_replay.h (the harnesses of the tests).
//
// Notation (header): H = J^T J = [[U, W], [W^T, V]], N = [Nc; Np] with J N = 0, D = Np^T V^-1 Np, B = Nc - W V^-1 Np,
// St = U - W V^-1 W^T + B D^-1 B^T, C = St^-1, Z_i = V_i^-1 Np_i, Y_a = W_a V_i^-1 (camera block of observation a, 9 x 3),
// E = C B D^-1 (ncp x 7), F = D^-1 (B^T C B) D^-1 - D^-1, and
//     pinv(H)_pp,i = V_i^-1 + Z_i F Z_i^T + sum_ab Y_a^T C_ab Y_b + sum_a (Y_a^T E_a Z_i^T + Z_i E_a^T Y_a).
// Every camera is handled nine wide: a six-parameter camera has zero columns 6..8 in A, so zero rows in W_a, Y_a and Nc; loops have
// constant bounds and static indices (nothing here may live in scratch memory on the device).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "ba_math.h"
#include "../../include/caliscope/uncertainty.h"

namespace cba {

constexpr int COV_GAUGE = 7;          // translation (3), rotation (3), scale
constexpr int COV_BLOCK = 256;        // threads of the per-camera, per-observation and reduction kernels
constexpr int COV_POINT_THREADS = 64; // one wave per point
constexpr int COV_MAX_NCP = 1152;     // the blocked Cholesky's limit (csrc/cba_kernels.h)
// A pivot of the Jacobi-scaled St (unit diagonal) or D at or below this is "not safely positive": the inverse would have no correct digit.
constexpr double COV_PIVOT_TINY = 1e-13;
// Points of one connected component of the constraint graph (cba_parameter_covariance_constrained): the component's V~ lives in LDS as a
// packed lower triangle, 162 * 163 / 2 doubles = 105.6 KB of the 160 KiB a workgroup has.  54 is the inner-corner count of a 10 x 7 board.
constexpr int COV_COMPONENT_CAP = 54;
constexpr int COV_GAUGE_RIGID = 6;    // translation (3), rotation (3): the gauge of a problem with distance rows (they fix the scale)

// inverse of a row-major 3 x 3 by the adjugate; false when the determinant vanishes
CBA_HD bool cov_inv3(const double* m, double* o) {
  const double c0 = m[4] * m[8] - m[5] * m[7], c1 = m[5] * m[6] - m[3] * m[8], c2 = m[3] * m[7] - m[4] * m[6];
  const double det = m[0] * c0 + m[1] * c1 + m[2] * c2;
  if (!(fabs(det) > 0.0)) return false;
  const double id = 1.0 / det;
  o[0] = c0 * id; o[1] = (m[2] * m[7] - m[1] * m[8]) * id; o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
  o[3] = c1 * id; o[4] = (m[0] * m[8] - m[2] * m[6]) * id; o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
  o[6] = c2 * id; o[7] = (m[1] * m[6] - m[0] * m[7]) * id; o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
  return true;
}

// Gauge rows of a camera, N[9][7]: rvec rows -Jl^-1 R in the rotation columns; tvec rows -R in the translation columns and t in the
// scale column; intrinsics (and the rows 6..8 of a six-parameter camera) zero.
// (G = 6: without the scale column)
template <int G> CBA_HD void cov_gauge_cam(const CamTab& c, double (*N)[G]) {
  double Ji[9];
  if (!cov_inv3(c.Jl, Ji)) {  // (Jl is singular at |rvec| = 2 pi only: outside the rvec range of a pose)
#pragma unroll
    for (int i = 0; i < 9; ++i) Ji[i] = (i % 4 == 0) ? 1.0 : 0.0;
  }
#pragma unroll
  for (int r = 0; r < 9; ++r)
#pragma unroll
    for (int j = 0; j < G; ++j) N[r][j] = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      N[r][3 + j] = -(Ji[3 * r] * c.R[j] + Ji[3 * r + 1] * c.R[3 + j] + Ji[3 * r + 2] * c.R[6 + j]);
      N[3 + r][j] = -c.R[3 * r + j];
    }
#pragma unroll
  for (int r = 0; r < 3; ++r)
    if (G > 6) N[3 + r][G - 1] = c.t[r];
}

// Gauge rows of a point, N[3][7] = [I | -[X]x | X]
template <int G> CBA_HD void cov_gauge_point(double X, double Y, double Z, double (*N)[G]) {
  N[0][0] = 1.0; N[0][1] = 0.0; N[0][2] = 0.0; N[0][3] = 0.0; N[0][4] = Z;   N[0][5] = -Y;
  N[1][0] = 0.0; N[1][1] = 1.0; N[1][2] = 0.0; N[1][3] = -Z;  N[1][4] = 0.0; N[1][5] = X;
  N[2][0] = 0.0; N[2][1] = 0.0; N[2][2] = 1.0; N[2][3] = Y;   N[2][4] = -X;  N[2][5] = 0.0;
  if (G > 6) { N[0][G - 1] = X; N[1][G - 1] = Y; N[2][G - 1] = Z; }
}

// One observation: residual and Jacobian blocks (project_full), both rows scaled for the robust loss (robust_one per scalar residual,
// as scipy does).  A is nine wide with zeros behind the camera's parameters.  Returns rho0 + rho1 (cost = 0.5 sum).  `r_scaled`, when
// given, receives the two residuals as scipy scales them for the loss (the residuals themselves for the linear loss).
CBA_HD double cov_obs_jacobian(const CamTab& c, const double* X, const double* uv, int loss, double f_scale, double (*A)[MAX_NC], double (*B)[3],
                               double* r_scaled = nullptr) {
  double e[2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int k = 0; k < MAX_NC; ++k) A[r][k] = 0.0;
  project_full(c, X[0], X[1], X[2], uv[0], uv[1], e, A, B);
  double rho = 0.0;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    double js, rs;
    rho += robust_one(loss, f_scale, e[r], &js, &rs);
    if (r_scaled) r_scaled[r] = rs;
#pragma unroll
    for (int k = 0; k < MAX_NC; ++k) A[r][k] *= js;
#pragma unroll
    for (int k = 0; k < 3; ++k) B[r][k] *= js;
  }
  return rho;
}

// W block A^T B (9 x 3, row-major) and B^T B (xx xy xz yy yz zz) of one observation
CBA_HD void cov_obs_products(const double (*A)[MAX_NC], const double (*B)[3], double* Wb, double* Vo) {
#pragma unroll
  for (int r = 0; r < MAX_NC; ++r)
#pragma unroll
    for (int q = 0; q < 3; ++q) Wb[3 * r + q] = A[0][r] * B[0][q] + A[1][r] * B[1][q];
  Vo[0] = B[0][0] * B[0][0] + B[1][0] * B[1][0]; Vo[1] = B[0][0] * B[0][1] + B[1][0] * B[1][1]; Vo[2] = B[0][0] * B[0][2] + B[1][0] * B[1][2];
  Vo[3] = B[0][1] * B[0][1] + B[1][1] * B[1][1]; Vo[4] = B[0][1] * B[0][2] + B[1][1] * B[1][2]; Vo[5] = B[0][2] * B[0][2] + B[1][2] * B[1][2];
}

// entry (p, q) of a symmetric 3 x 3 stored as xx xy xz yy yz zz
CBA_HD double cov_sym3(const double* s, int p, int q) {
  const int lo = p < q ? p : q, hi = p < q ? q : p;
  return s[lo == 0 ? hi : (lo == 1 ? 2 + hi : 5)];
}

// V^-1 (xx xy xz yy yz zz) of a point from the sum V of its observations' B^T B; false when a pivot is not safely positive (chol3)
CBA_HD bool cov_point_vinv(const double* V, double* Vi) {
  double L[6];
  if (!chol3(V, L)) return false;
  double col[3][3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double e[3] = {j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0};
    double y[3];
    chol3_fwd(L, e, y);
    chol3_bwd(L, y, col[j]);
  }
  Vi[0] = col[0][0]; Vi[1] = col[1][0]; Vi[2] = col[2][0]; Vi[3] = col[1][1]; Vi[4] = col[2][1]; Vi[5] = col[2][2];
  return true;
}

// Z = V^-1 Np (3 x 7) of a point
template <int G> CBA_HD void cov_point_z(const double* Vi, const double* X, double (*Z)[G]) {
  double N[3][G];
  cov_gauge_point(X[0], X[1], X[2], N);
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int j = 0; j < G; ++j) Z[p][j] = cov_sym3(Vi, p, 0) * N[0][j] + cov_sym3(Vi, p, 1) * N[1][j] + cov_sym3(Vi, p, 2) * N[2][j];
}

// the dense part of a point's covariance: V^-1 + Z F Z^T (xx xy xz yy yz zz); F row-major G x G, symmetric
template <int G> CBA_HD void cov_point_base(const double* Vi, const double (*Z)[G], const double* F, double* P) {
  double ZF[3][G];
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int k = 0; k < G; ++k) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < G; ++j) s += Z[p][j] * F[j * G + k];
      ZF[p][k] = s;
    }
  int e = 0;
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int q = p; q < 3; ++q) {
      double s = Vi[e];
#pragma unroll
      for (int k = 0; k < G; ++k) s += ZF[p][k] * Z[q][k];
      P[e++] = s;
    }
}

// ---- host only -------------------------------------------------------------------------------------------------------------------

struct CovPlan {
  std::vector<int64_t> order;     // observations sorted by (point, input position), or by (point, camera, uv, input position): cov_validate
  std::vector<int64_t> pt_start;  // [n_points + 1] into the sorted observations
  std::vector<int32_t> cam_off;   // [n_cams + 1] first parameter of a camera; cam_off[n_cams] = ncp
  int64_t dof = 0;
  int32_t ncp() const { return cam_off.back(); }
};

// Every check of the header, and the plan.  0 or a CBA_ERR_* with `msg` naming the offender (`call`: the entry point the message starts with).
// `canonical`: the observations of a point are ordered by (camera, bits of u, bits of v, input position) instead of by input position alone,
// so that the sorted table, and with CBA_DETERMINISTIC=1 every bit computed from it, does not depend on the order of the caller's rows.
// With constraint rows (covariance_constraint_plan.h): `gauge` = 6, `in_row[p]` != 0 for a point some row of positive weight names (it needs
// no second observation: its component determines it) and `n_con` such rows, which count in the degrees of freedom.
inline int cov_validate(const cba_cov_desc* d, CovPlan& plan, std::string& msg, const char* call = "cba_parameter_covariance", bool canonical = false,
                        int gauge = COV_GAUGE, const uint8_t* in_row = nullptr, int64_t n_con = 0) {
  const std::string what = std::string(call) + ": ";
  auto fail = [&](int code, const std::string& m) { msg = what + m; return code; };
  if (d->n_cams <= 0) return fail(CBA_ERR_INVALID, "n_cams must be positive, got " + std::to_string(d->n_cams));
  if (d->n_points <= 0 || d->n_points > INT32_MAX) return fail(CBA_ERR_INVALID, "n_points must be in [1, 2^31), got " + std::to_string(d->n_points));
  if (d->n_obs <= 0) return fail(CBA_ERR_INVALID, "n_obs must be positive, got " + std::to_string(d->n_obs) + ": no observations, no covariance");
  if (!d->cam_model || !d->cam_nparams || !d->cam_const || !d->cam_x || !d->points || !d->obs_cam || !d->obs_pt || !d->obs_uv)
    return fail(CBA_ERR_INVALID, "null input array");
  if (d->loss < LOSS_LINEAR || d->loss > LOSS_ARCTAN) return fail(CBA_ERR_INVALID, "unknown loss " + std::to_string(d->loss));
  if (d->loss != LOSS_LINEAR && !(d->f_scale > 0.0)) return fail(CBA_ERR_INVALID, "f_scale must be positive for a robust loss");
  plan.cam_off.assign((size_t)d->n_cams + 1, 0);
  for (int32_t c = 0; c < d->n_cams; ++c) {
    const int32_t np = d->cam_nparams[c];
    if (np != 6 && np != 9) return fail(CBA_ERR_INVALID, "camera " + std::to_string(c) + ": cam_nparams must be 6 or 9, got " + std::to_string(np));
    if (d->cam_model[c] != MODEL_PINHOLE_BC5 && d->cam_model[c] != MODEL_FISHEYE4)
      return fail(CBA_ERR_INVALID, "camera " + std::to_string(c) + ": unknown model " + std::to_string(d->cam_model[c]));
    if (np == 9 && d->cam_model[c] == MODEL_FISHEYE4) return fail(CBA_ERR_UNSUPPORTED, "camera " + std::to_string(c) + ": a fisheye camera has no free intrinsics (9 parameters)");
    plan.cam_off[(size_t)c + 1] = plan.cam_off[(size_t)c] + np;
  }
  if (plan.ncp() > COV_MAX_NCP) return fail(CBA_ERR_UNSUPPORTED, std::to_string(plan.ncp()) + " camera parameters: the dense factorisation handles " + std::to_string(COV_MAX_NCP));
  std::vector<int64_t> cam_rows((size_t)d->n_cams, 0);
  plan.pt_start.assign((size_t)d->n_points + 1, 0);
  for (int64_t o = 0; o < d->n_obs; ++o) {
    const int32_t c = d->obs_cam[o], p = d->obs_pt[o];
    if (c < 0 || c >= d->n_cams) return fail(CBA_ERR_INVALID, "observation " + std::to_string(o) + ": camera index " + std::to_string(c) + " out of range");
    if (p < 0 || p >= d->n_points) return fail(CBA_ERR_INVALID, "observation " + std::to_string(o) + ": point index " + std::to_string(p) + " out of range");
    ++cam_rows[(size_t)c];
    ++plan.pt_start[(size_t)p + 1];
  }
  for (int32_t c = 0; c < d->n_cams; ++c)
    if (cam_rows[(size_t)c] == 0) return fail(CBA_ERR_INVALID, "camera " + std::to_string(c) + " has no observation");
  for (int64_t p = 0; p < d->n_points; ++p)
    if (plan.pt_start[(size_t)p + 1] < 2 && !(in_row && in_row[(size_t)p])) return fail(CBA_ERR_INVALID, "point " + std::to_string(p) + " has " + std::to_string(plan.pt_start[(size_t)p + 1]) + " observation(s): two are needed");
  plan.dof = 2 * d->n_obs - ((int64_t)plan.ncp() + 3 * d->n_points) + gauge + n_con;
  if (plan.dof <= 0)
    return fail(CBA_ERR_INVALID, std::string(n_con ? "dof = 2 n_obs + n_con - n_params + " : "dof = 2 n_obs - n_params + ") + std::to_string(gauge) + " = " +
                                     std::to_string(plan.dof) + " is not positive");
  for (int64_t p = 0; p < d->n_points; ++p) plan.pt_start[(size_t)p + 1] += plan.pt_start[(size_t)p];
  std::vector<int64_t> next(plan.pt_start.begin(), plan.pt_start.end() - 1);
  plan.order.resize((size_t)d->n_obs);
  for (int64_t o = 0; o < d->n_obs; ++o) plan.order[(size_t)next[(size_t)d->obs_pt[o]]++] = o;
  if (canonical) {
    const auto bits = [&](int64_t o, int j) { uint64_t b; std::memcpy(&b, d->obs_uv + 2 * o + j, sizeof b); return b; };
    const auto before = [&](int64_t a, int64_t b) {
      if (d->obs_cam[a] != d->obs_cam[b]) return d->obs_cam[a] < d->obs_cam[b];
      if (bits(a, 0) != bits(b, 0)) return bits(a, 0) < bits(b, 0);
      if (bits(a, 1) != bits(b, 1)) return bits(a, 1) < bits(b, 1);
      return a < b;
    };
    for (int64_t p = 0; p < d->n_points; ++p) {
      const auto first = plan.order.begin() + plan.pt_start[(size_t)p], last = plan.order.begin() + plan.pt_start[(size_t)p + 1];
      if (!std::is_sorted(first, last, before)) std::sort(first, last, before);  // (rows grouped by point and camera arrive sorted)
    }
  }
  return CBA_OK;
}

// The numeric refusals of the calls, each text once: the library and the host replay of the tests (tests/native/covariance_replay.h) say
// them through these, and the CPU and GPU tests match on them.  `what`: the entry point the message starts with.
inline std::string cov_msg_point(const std::string& what, int64_t p) {
  return what + ": point " + std::to_string(p) + ": its observations do not determine it (rays parallel or not finite)";
}
inline std::string cov_msg_gauge(const std::string& what, int gauge) {
  return what + ": the points do not fix the " + (gauge == COV_GAUGE ? "seven" : "six") + " gauge directions (all on one line, or not finite)";
}
inline std::string cov_msg_not_pd(const std::string& what) {
  return what + ": the reduced camera system is not positive definite beyond the gauge (a pivot is not safely positive): "
                "the scene does not determine every camera parameter";
}
inline std::string cov_msg_not_finite(const std::string& what, const char* which) {  // which: "point" or "camera"
  return what + ": a " + which + " covariance is not finite";
}

// The camera outputs and the scalars of a call from C = St^-1 (n x n, both triangles): sigma0^2 C into cam_cov_full, its diagonal blocks
// zero-padded to nine wide into cam_cov.  A NULL output is left out.
inline void cov_write_outputs(const CovPlan& plan, const std::vector<double>& C, double sigma0_sq, double cost, cba_cov_out* out) {
  const int32_t n_cams = (int32_t)plan.cam_off.size() - 1, ncp = plan.ncp();
  if (out->cam_cov_full)
    for (size_t i = 0; i < C.size(); ++i) out->cam_cov_full[i] = sigma0_sq * C[i];
  if (out->cam_cov)
    for (int32_t c = 0; c < n_cams; ++c) {
      const int32_t off = plan.cam_off[(size_t)c], np = plan.cam_off[(size_t)c + 1] - off;
      for (int r = 0; r < MAX_NC; ++r)
        for (int q = 0; q < MAX_NC; ++q)
          out->cam_cov[((size_t)c * MAX_NC + r) * MAX_NC + q] = (r < np && q < np) ? sigma0_sq * C[(size_t)(off + r) * ncp + off + q] : 0.0;
    }
  if (out->sigma0_sq) *out->sigma0_sq = sigma0_sq;
  if (out->dof) *out->dof = plan.dof;
  if (out->cost) *out->cost = cost;
}

// In-place inverse of a symmetric positive definite n x n (row-major, both triangles) by Cholesky after a symmetric Jacobi scaling;
// false when a diagonal entry or a scaled pivot is not above COV_PIVOT_TINY.  (D on the host of the device call; St too in the harness.)
inline bool cov_spd_inverse(std::vector<double>& M, int n) {
  std::vector<double> s((size_t)n), L((size_t)n * n, 0.0), X((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) {
    const double dgl = M[(size_t)i * n + i];
    if (!(dgl > 0.0) || !std::isfinite(dgl)) return false;
    s[(size_t)i] = 1.0 / std::sqrt(dgl);
  }
  for (int j = 0; j < n; ++j) {
    double dj = M[(size_t)j * n + j] * s[(size_t)j] * s[(size_t)j];
    for (int t = 0; t < j; ++t) dj -= L[(size_t)j * n + t] * L[(size_t)j * n + t];
    if (!(dj > COV_PIVOT_TINY) || !std::isfinite(dj)) return false;
    const double ljj = std::sqrt(dj);
    L[(size_t)j * n + j] = ljj;
    for (int i = j + 1; i < n; ++i) {
      double v = M[(size_t)i * n + j] * s[(size_t)i] * s[(size_t)j];
      for (int t = 0; t < j; ++t) v -= L[(size_t)i * n + t] * L[(size_t)j * n + t];
      L[(size_t)i * n + j] = v / ljj;
    }
  }
  for (int c = 0; c < n; ++c)  // X = L^-1, column by column
    for (int i = c; i < n; ++i) {
      double v = i == c ? 1.0 : 0.0;
      for (int t = c; t < i; ++t) v -= L[(size_t)i * n + t] * X[(size_t)t * n + c];
      X[(size_t)i * n + c] = v / L[(size_t)i * n + i];
    }
  for (int i = 0; i < n; ++i)
    for (int j = i; j < n; ++j) {
      double v = 0.0;
      for (int t = j; t < n; ++t) v += X[(size_t)t * n + i] * X[(size_t)t * n + j];
      v *= s[(size_t)i] * s[(size_t)j];
      M[(size_t)i * n + j] = v;
      M[(size_t)j * n + i] = v;
    }
  return true;
}

// E = C B D^-1 (n x G) and F = D^-1 (B^T C B) D^-1 - D^-1 (G x G) from C (n x n), B (n x G), D^-1 (G x G), all row-major; G the gauge width
template <int G = COV_GAUGE>
inline void cov_gauge_terms(int n, const double* C, const double* B, const double* Dinv, std::vector<double>& E, std::vector<double>& F) {
  std::vector<double> CB((size_t)n * G, 0.0);
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < n; ++c) {
      const double v = C[(size_t)r * n + c];
      for (int j = 0; j < G; ++j) CB[(size_t)r * G + j] += v * B[(size_t)c * G + j];
    }
  double M[G][G] = {}, MD[G][G] = {};
  for (int r = 0; r < n; ++r)
    for (int j = 0; j < G; ++j)
      for (int k = 0; k < G; ++k) M[j][k] += B[(size_t)r * G + j] * CB[(size_t)r * G + k];
  E.assign((size_t)n * G, 0.0);
  for (int r = 0; r < n; ++r)
    for (int j = 0; j < G; ++j)
      for (int k = 0; k < G; ++k) E[(size_t)r * G + k] += CB[(size_t)r * G + j] * Dinv[j * G + k];
  for (int j = 0; j < G; ++j)
    for (int k = 0; k < G; ++k)
      for (int m = 0; m < G; ++m) MD[j][k] += 0.5 * (M[j][m] + M[m][j]) * Dinv[m * G + k];
  F.assign((size_t)G * G, 0.0);
  for (int j = 0; j < G; ++j)
    for (int k = 0; k < G; ++k) {
      double v = -Dinv[j * G + k];
      for (int m = 0; m < G; ++m) v += Dinv[j * G + m] * MD[m][k];
      F[(size_t)j * G + k] = v;
    }
  for (int j = 0; j < G; ++j)  // symmetric to the bit
    for (int k = j + 1; k < G; ++k) F[(size_t)j * G + k] = F[(size_t)k * G + j] = 0.5 * (F[(size_t)j * G + k] + F[(size_t)k * G + j]);
}

}  // namespace cba
