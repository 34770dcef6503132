// The steps of cba_observation_reliability_constrained behind C = St^-1, serially on the host — TEST INFRASTRUCTURE, plain C++17 (g++), beside
// covariance_replay.h (which it leaves as it is and whose CovReplay it reads).  It mirrors rel_outputs of caliscope_amd/csrc/reliability_lib.hip with
// the per-element arithmetic the library uses (reliability_math.h, reliability_constraint_math.h): k_rel_point on the points in no row,
// k_rel_con_point on the points of the components, k_rel_con_rows on the constraint rows.  What the device keeps from k_unc_con_rows and
// k_unc_component (u, coef, and s_j = |X c_j^T|^2 formed while X is in LDS) is recomputed here with cov_con_row, cov_tri_cholesky and
// cov_tri_invert: CovReplay does not hold them.  It is not a CPU fallback: nothing in caliscope_amd/ includes it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "covariance_replay.h"
#include "reliability_constraint_math.h"

namespace cba {

// con == nullptr: the unconstrained call (every point through k_rel_point).  n_con: the caller's rows.  0 or a CBA_ERR_* with `error` set;
// nothing is written before the last check.
inline int rel_con_replay(const cba_cov_desc* d, const CovConPlan* con, const CovReplay& rp, const std::string& what, std::string& error, const cba_rel_out* out,
                          int64_t n_con, const cba_rel_con_out* con_out) {
  constexpr int WB = 3 * MAX_NC;
  const CovPlan& plan = rp.plan;
  const std::vector<CamTab>& tab = rp.tab;
  const std::vector<int32_t>& cam_sorted = rp.cam_sorted;
  const std::vector<double> &Y = rp.Y, &Yc = rp.Yc, &Vinv = rp.Vinv, &C = rp.C;
  const int32_t ncp = plan.ncp();
  const int64_t n_obs = d->n_obs, n_points = d->n_points;
  for (double v : C)
    if (!std::isfinite(v)) { error = cov_msg_not_finite(what, "camera"); return CBA_ERR_NUMERIC; }
  const double sigma0 = std::sqrt(rp.sigma0_sq);
  std::vector<double> red((size_t)n_obs * 3), w((size_t)n_obs * 2), f((size_t)n_obs * 2);
  int64_t bad = 0, bad_con = 0;
  auto cam_range = [&](int32_t cam, int32_t& off, int32_t& np) { off = plan.cam_off[(size_t)cam]; np = plan.cam_off[(size_t)cam + 1] - off; };
  for (int64_t p = 0; p < n_points; ++p) {
    const int64_t s = plan.pt_start[(size_t)p], k = plan.pt_start[(size_t)p + 1] - s;
    const double* X = d->points + 3 * (size_t)p;
    double Q[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (!(con && con->in_row[(size_t)p])) {  // k_rel_point
      for (int64_t b = 0; b < k; ++b) {
        const int64_t o = plan.order[(size_t)(s + b)];
        int32_t off, np;
        const int32_t cam = cam_sorted[(size_t)(s + b)];
        cam_range(cam, off, np);
        double A[2][MAX_NC], Bo[2][3], M[6] = {0, 0, 0, 0, 0, 0}, S[3] = {0, 0, 0}, T[3];
        cov_obs_jacobian(tab[(size_t)cam], X, d->obs_uv + 2 * (size_t)o, d->loss, d->f_scale, A, Bo);
        for (int r = 0; r < np; ++r) {
          const double* crow = &C[(size_t)(off + r) * ncp];
          double g[3] = {0, 0, 0}, h[2], a[2];
          for (int64_t bp = 0; bp < k; ++bp) {
            int32_t off_b, np_b;
            cam_range(cam_sorted[(size_t)(s + bp)], off_b, np_b);
            rel_row_times_y(crow + off_b, np_b, &Y[(size_t)(s + bp) * WB], g);
          }
          rel_row_times_a(crow + off, np, A, h);
          rel_a_column(A, r, a);
          rel_row_terms(a, &Y[(size_t)(s + b) * WB + 3 * r], g, h, Q, M, S);
        }
        rel_camera_part(S, M, Bo, T);
        for (int e = 0; e < 3; ++e) red[(size_t)o * 3 + e] = T[e];
      }
      for (int64_t b = 0; b < k; ++b) {
        const int64_t o = plan.order[(size_t)(s + b)];
        double A[2][MAX_NC], Bo[2][3];
        cov_obs_jacobian(tab[(size_t)cam_sorted[(size_t)(s + b)]], X, d->obs_uv + 2 * (size_t)o, d->loss, d->f_scale, A, Bo, &f[(size_t)o * 2]);
        const double T[3] = {red[(size_t)o * 3], red[(size_t)o * 3 + 1], red[(size_t)o * 3 + 2]};
        bad += rel_finish(Bo, &Vinv[(size_t)p * 6], Q, T, sigma0, &f[(size_t)o * 2], &red[(size_t)o * 3], &w[(size_t)o * 2]);
      }
      continue;
    }
    // k_rel_con_point
    const int64_t es = con->entry_start[(size_t)p];
    const int n_e = (int)(con->entry_start[(size_t)p + 1] - es);
    std::vector<double> Gs((size_t)n_e * WB, 0.0);
    for (int e = 0; e < n_e; ++e) {
      int32_t off, np;
      cam_range(con->entry_cam[(size_t)(es + e)], off, np);
      for (int r = 0; r < np; ++r) {
        const double* crow = &C[(size_t)(off + r) * ncp];
        double g[3] = {0, 0, 0};
        for (int ep = 0; ep < n_e; ++ep) {
          int32_t off_b, np_b;
          cam_range(con->entry_cam[(size_t)(es + ep)], off_b, np_b);
          rel_row_times_y(crow + off_b, np_b, &Yc[(size_t)(es + ep) * WB], g);
        }
        rel_con_q_terms(&Yc[(size_t)(es + e) * WB + 3 * r], g, Q);
        for (int q = 0; q < 3; ++q) Gs[(size_t)e * WB + 3 * r + q] = g[q];
      }
    }
    for (int64_t b = 0; b < k; ++b) {
      const int64_t o = plan.order[(size_t)(s + b)];
      const int32_t cam = cam_sorted[(size_t)(s + b)];
      int32_t off, np;
      cam_range(cam, off, np);
      double A[2][MAX_NC], Bo[2][3], M[6] = {0, 0, 0, 0, 0, 0}, S[3] = {0, 0, 0}, T[3];
      cov_obs_jacobian(tab[(size_t)cam], X, d->obs_uv + 2 * (size_t)o, d->loss, d->f_scale, A, Bo, &f[(size_t)o * 2]);
      int lo = 0, hi = n_e - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (con->entry_cam[(size_t)(es + mid)] < cam) lo = mid + 1; else hi = mid;
      }
      for (int r = 0; r < np; ++r) {
        double h[2], a[2];
        rel_row_times_a(&C[(size_t)(off + r) * ncp + off], np, A, h);
        rel_a_column(A, r, a);
        rel_con_obs_terms(a, &Gs[(size_t)lo * WB + 3 * r], h, M, S);
      }
      rel_camera_part(S, M, Bo, T);
      bad += rel_finish(Bo, &Vinv[(size_t)p * 6], Q, T, sigma0, &f[(size_t)o * 2], &red[(size_t)o * 3], &w[(size_t)o * 2]);
    }
  }
  for (double v : red)
    if (!std::isfinite(v)) { error = what + ": a redundancy number is not finite"; return CBA_ERR_NUMERIC; }
  // k_rel_con_rows, with u, coef and X of every component formed again
  std::vector<double> cr((size_t)n_con, std::nan("")), cw((size_t)n_con, std::nan("")), cf((size_t)n_con, std::nan(""));
  if (con) {
    std::vector<double> Vobs((size_t)n_obs * 6);
    for (int64_t i = 0; i < n_obs; ++i) {
      const int64_t o = plan.order[(size_t)i];
      double A[2][MAX_NC], Bo[2][3], Wb[WB];
      cov_obs_jacobian(tab[(size_t)cam_sorted[(size_t)i]], d->points + 3 * (size_t)d->obs_pt[o], d->obs_uv + 2 * (size_t)o, d->loss, d->f_scale, A, Bo);
      cov_obs_products(A, Bo, Wb, &Vobs[(size_t)i * 6]);
    }
    for (int32_t k = 0; k < con->n_comp; ++k) {
      const int64_t p0 = con->comp_pt[(size_t)k], r0 = con->comp_row[(size_t)k], r1 = con->comp_row[(size_t)k + 1];
      const int m = (int)(con->comp_pt[(size_t)k + 1] - p0), n = 3 * m;
      const int32_t* pts = &con->pts[(size_t)p0];
      std::vector<double> Vt((size_t)n * (n + 1) / 2, 0.0), col((size_t)n), diag0((size_t)n), row_u((size_t)(r1 - r0) * 3), row_coef((size_t)(r1 - r0) * 8);
      for (int i = 0; i < m; ++i) {
        double V[6] = {0, 0, 0, 0, 0, 0};
        for (int64_t a = plan.pt_start[(size_t)pts[i]]; a < plan.pt_start[(size_t)pts[i] + 1]; ++a)
          for (int e = 0; e < 6; ++e) V[e] += Vobs[(size_t)a * 6 + e];
        for (int e = 0; e < 6; ++e) Vt[(size_t)cov_tri(3 * i + cov_sym3_col(e), 3 * i + cov_sym3_row(e))] = V[e];
      }
      for (int64_t r = r0; r < r1; ++r) {
        double* u = &row_u[(size_t)(r - r0) * 3];
        double* coef = &row_coef[(size_t)(r - r0) * 8];
        cov_con_row(d->points, &con->row_pt[(size_t)r * 8], con->row_dist[(size_t)r], con->row_weight[(size_t)r], d->loss, d->f_scale, u, coef);
        for (int s = 0; s < 8; ++s)
          for (int s2 = 0; s2 < 8; ++s2) {
            const double cc = coef[s] * coef[s2];
            if (cc == 0.0) continue;
            const int ri = 3 * con->row_loc[(size_t)r * 8 + s], rj = 3 * con->row_loc[(size_t)r * 8 + s2];
            for (int a = 0; a < 3; ++a)
              for (int b = 0; b < 3; ++b)
                if (ri + a >= rj + b) Vt[(size_t)cov_tri(ri + a, rj + b)] += cc * u[a] * u[b];
          }
      }
      for (int i = 0; i < n; ++i) diag0[(size_t)i] = Vt[(size_t)cov_tri(i, i)];
      if (!cov_tri_cholesky(Vt.data(), n, diag0.data())) { error = cov_con_msg_component(what, pts[0]); return CBA_ERR_NUMERIC; }
      cov_tri_invert(Vt.data(), n, col.data());
      const int64_t q0 = con->comp_cam[(size_t)k];
      const int nc = (int)(con->comp_cam[(size_t)k + 1] - q0);
      std::vector<double> v((size_t)MAX_NC * nc);
      for (int64_t r = r0; r < r1; ++r) {
        const double* u = &row_u[(size_t)(r - r0) * 3];
        const double* coef = &row_coef[(size_t)(r - r0) * 8];
        const int32_t* pt = &con->row_pt[(size_t)r * 8];
        double s_j = 0.0;
        for (int i = 0; i < n; ++i) {
          const double q = rel_con_x_row(Vt.data(), i, &con->row_loc[(size_t)r * 8], coef, u);
          s_j += q * q;
        }
        int64_t e0[8];
        for (int s = 0; s < 8; ++s) e0[s] = con->entry_start[(size_t)pt[s]];
        for (int it = 0; it < MAX_NC * nc; ++it) v[(size_t)it] = rel_con_v_entry(Yc.data(), e0, it / MAX_NC, it % MAX_NC, coef, u);
        double quad = 0.0;
        for (int it = 0; it < MAX_NC * nc; ++it) {
          const int c = it / MAX_NC, rr = it % MAX_NC;
          int32_t off, np;
          cam_range(con->cams[(size_t)(q0 + c)], off, np);
          if (rr >= np) continue;
          const double* crow = &C[(size_t)(off + rr) * ncp];
          double tsum = 0.0;
          for (int c2 = 0; c2 < nc; ++c2) {
            int32_t off_b, np_b;
            cam_range(con->cams[(size_t)(q0 + c2)], off_b, np_b);
            tsum += rel_con_row_dot(crow + off_b, np_b, &v[(size_t)MAX_NC * c2]);
          }
          quad += v[(size_t)it] * tsum;
        }
        const size_t dst = (size_t)con->row_src[(size_t)r];
        cf[dst] = rel_con_residual(d->points, pt, con->row_dist[(size_t)r], con->row_weight[(size_t)r], d->loss, d->f_scale);
        bad_con += rel_con_finish(s_j, quad, cf[dst], sigma0, &cr[dst], &cw[dst]);
        if (!std::isfinite(cr[dst])) { error = what + ": a redundancy number is not finite"; return CBA_ERR_NUMERIC; }
      }
    }
  }
  if (out) {
    if (out->redundancy) std::copy(red.begin(), red.end(), out->redundancy);
    if (out->w) std::copy(w.begin(), w.end(), out->w);
    if (out->residual) std::copy(f.begin(), f.end(), out->residual);
    if (out->sigma0_sq) *out->sigma0_sq = rp.sigma0_sq;
    if (out->dof) *out->dof = plan.dof;
    if (out->cost) *out->cost = rp.cost;
    if (out->n_uncontrolled) *out->n_uncontrolled = bad;
  }
  if (con_out) {
    if (con_out->redundancy) std::copy(cr.begin(), cr.end(), con_out->redundancy);
    if (con_out->w) std::copy(cw.begin(), cw.end(), con_out->w);
    if (con_out->residual) std::copy(cf.begin(), cf.end(), con_out->residual);
    if (con_out->n_uncontrolled) *con_out->n_uncontrolled = bad_con;
  }
  return CBA_OK;
}

}  // namespace cba
