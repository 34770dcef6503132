// The one serial replay of the covariance pipeline on the host — TEST INFRASTRUCTURE, plain C++17 (g++), included by the three harnesses
// beside it: covariance_harness.cpp, reliability_harness.cpp and covariance_constrained_harness.cpp.  It mirrors cov_pipeline_run<G> /
// cov_outputs<G> of caliscope_amd/csrc/covariance_lib.hip with the host plan, the checks, the refusal texts and the per-element arithmetic
// the library uses (covariance_math.h, covariance_constraint_math.h, covariance_constraint_plan.h); what the kernels spread over threads
// runs serially here (observation after observation, point after point, component after component) and the dense factor and inverse of
// the device (k_chol_step, k_unc_ttt) are cov_spd_inverse.  Every sum has ONE order, so the same input gives the same bytes whichever
// harness asks, and a call without a constraint row of positive weight is the unconstrained call by construction.  It is not a CPU
// fallback: nothing in caliscope_amd/ includes it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "ba_math.h"
#include "covariance_math.h"
#include "covariance_constraint_math.h"
#include "covariance_constraint_plan.h"

namespace cba {

// What CovPipeline hands to `finish`, on the host
struct CovReplay {
  CovPlan plan;
  std::vector<CamTab> tab;          // [n_cams]
  std::vector<int32_t> cam_sorted;  // [n_obs] camera of a sorted position
  std::vector<double> Y;            // [n_obs][27] Y_a = W_a V^-1, sorted order (the points in no row)
  std::vector<double> Yc;           // [entries][27] Y_c[:, i] of a constrained point and a camera of its component
  std::vector<double> Vinv;         // [n_points][6]
  std::vector<double> Z;            // [n_points][3][G]
  std::vector<double> B;            // [ncp][G]
  std::vector<double> Dinv;         // [G][G]
  std::vector<double> C;            // [ncp][ncp] St^-1, both triangles
  double sigma0_sq = 0.0, cost = 0.0;
};

// Everything up to C = St^-1 with G gauge columns.  `con` (G = 6): the components of the constraint rows (cov_con_components, at least one row),
// its tables are completed here; nullptr (G = 7): none.  `canonical` is cov_validate's.  0, or a CBA_ERR_* with `error` set.
template <int G>
int cov_replay(const cba_cov_desc* d, CovConPlan* con, bool canonical, const std::string& what, std::string& error, CovReplay& out) {
  CovPlan& plan = out.plan;
  const int rc = cov_validate(d, plan, error, what.c_str(), canonical, G, con ? con->in_row.data() : nullptr, con ? con->n_rows : 0);
  if (rc) return rc;
  if (con && cov_fixed_order_requested()) {
    error = cov_con_msg_fixed_order(what);
    return CBA_ERR_UNSUPPORTED;
  }
  constexpr int WB = 3 * MAX_NC;
  const int32_t n_cams = d->n_cams, ncp = plan.ncp();
  const int64_t n_obs = d->n_obs, n_points = d->n_points;
  if (con) cov_con_tables(plan, d->obs_cam, n_cams, n_points, *con);
  // k_unc_cam
  std::vector<CamTab>& tab = out.tab;
  std::vector<double>& B = out.B;
  tab.assign((size_t)n_cams, CamTab());
  B.assign((size_t)ncp * G, 0.0);
  for (int32_t c = 0; c < n_cams; ++c) {
    const int32_t off = plan.cam_off[(size_t)c], np = plan.cam_off[(size_t)c + 1] - off;
    double xc[MAX_NC] = {0};
    for (int i = 0; i < np; ++i) xc[i] = d->cam_x[(size_t)c * MAX_NC + i];
    cam_prepare(xc, d->cam_const + (size_t)c * CAM_CONST_STRIDE, d->cam_model[c], np, &tab[(size_t)c], off);
    double N[MAX_NC][G];
    cov_gauge_cam(tab[(size_t)c], N);
    for (int r = 0; r < np; ++r)
      for (int j = 0; j < G; ++j) B[(size_t)(off + r) * G + j] = N[r][j];
  }
  // k_unc_obs
  std::vector<double> Wblk((size_t)n_obs * WB), Vobs((size_t)n_obs * 6), U((size_t)n_cams * MAX_NC * MAX_NC, 0.0);
  std::vector<double>& Y = out.Y;
  std::vector<int32_t>& cam_sorted = out.cam_sorted;
  Y.assign((size_t)n_obs * WB, 0.0);
  cam_sorted.assign((size_t)n_obs, 0);
  double cost = 0.0;
  for (int64_t i = 0; i < n_obs; ++i) {
    const int64_t o = plan.order[(size_t)i];
    const int32_t cam = d->obs_cam[o];
    double A[2][MAX_NC], Bo[2][3];
    cost += 0.5 * cov_obs_jacobian(tab[(size_t)cam], d->points + 3 * (size_t)d->obs_pt[o], d->obs_uv + 2 * (size_t)o, d->loss, d->f_scale, A, Bo);
    cov_obs_products(A, Bo, &Wblk[(size_t)i * WB], &Vobs[(size_t)i * 6]);
    cam_sorted[(size_t)i] = cam;
    for (int r = 0; r < MAX_NC; ++r)
      for (int q = r; q < MAX_NC; ++q) U[((size_t)cam * MAX_NC + r) * MAX_NC + q] += A[0][r] * A[0][q] + A[1][r] * A[1][q];
  }
  // k_unc_con_rows
  std::vector<double> row_u, row_coef;
  if (con) {
    row_u.resize((size_t)con->n_rows * 3); row_coef.resize((size_t)con->n_rows * 8);
    for (int64_t r = 0; r < con->n_rows; ++r)
      cost += 0.5 * cov_con_row(d->points, &con->row_pt[(size_t)r * 8], con->row_dist[(size_t)r], con->row_weight[(size_t)r], d->loss, d->f_scale, &row_u[(size_t)r * 3],
                                &row_coef[(size_t)r * 8]);
  }
  // k_unc_point (the points in no row), k_unc_d
  std::vector<double>& Vinv = out.Vinv;
  std::vector<double>& Zall = out.Z;
  std::vector<double>& D = out.Dinv;
  std::vector<double> St((size_t)ncp * ncp, 0.0);
  Vinv.assign((size_t)n_points * 6, 0.0);
  Zall.assign((size_t)n_points * 3 * G, 0.0);
  D.assign((size_t)G * G, 0.0);
  const int64_t n_free = con ? (int64_t)con->free_pts.size() : n_points;
  for (int64_t f = 0; f < n_free; ++f) {
    const int64_t p = con ? (int64_t)con->free_pts[(size_t)f] : f;
    const int64_t s = plan.pt_start[(size_t)p], k = plan.pt_start[(size_t)p + 1] - s;
    double V[6] = {0, 0, 0, 0, 0, 0};
    for (int64_t a = 0; a < k; ++a)
      for (int e = 0; e < 6; ++e) V[e] += Vobs[(size_t)(s + a) * 6 + e];
    double* Vi = &Vinv[(size_t)p * 6];
    if (!cov_point_vinv(V, Vi)) {
      error = cov_msg_point(what, p);
      return CBA_ERR_NUMERIC;
    }
    double (*Z)[G] = reinterpret_cast<double (*)[G]>(&Zall[(size_t)p * 3 * G]);
    cov_point_z(Vi, d->points + 3 * (size_t)p, Z);
    double N[3][G];
    cov_gauge_point(d->points[3 * p], d->points[3 * p + 1], d->points[3 * p + 2], N);
    for (int j = 0; j < G; ++j)
      for (int m = j; m < G; ++m) D[(size_t)j * G + m] += N[0][j] * Z[0][m] + N[1][j] * Z[1][m] + N[2][j] * Z[2][m];
    for (int64_t a = 0; a < k; ++a) {
      const double* w = &Wblk[(size_t)(s + a) * WB];
      double* y = &Y[(size_t)(s + a) * WB];
      const int32_t off = plan.cam_off[(size_t)cam_sorted[(size_t)(s + a)]], np = plan.cam_off[(size_t)cam_sorted[(size_t)(s + a)] + 1] - off;
      for (int r = 0; r < MAX_NC; ++r) {
        for (int q = 0; q < 3; ++q) y[3 * r + q] = w[3 * r] * cov_sym3(Vi, 0, q) + w[3 * r + 1] * cov_sym3(Vi, 1, q) + w[3 * r + 2] * cov_sym3(Vi, 2, q);
        if (r < np)
          for (int j = 0; j < G; ++j) B[(size_t)(off + r) * G + j] -= w[3 * r] * Z[0][j] + w[3 * r + 1] * Z[1][j] + w[3 * r + 2] * Z[2][j];
      }
    }
    for (int64_t a = 0; a < k; ++a)
      for (int64_t b = 0; b < k; ++b) {
        const int32_t ca = cam_sorted[(size_t)(s + a)], cb = cam_sorted[(size_t)(s + b)];
        const int32_t off_a = plan.cam_off[(size_t)ca], np_a = plan.cam_off[(size_t)ca + 1] - off_a;
        const int32_t off_b = plan.cam_off[(size_t)cb], np_b = plan.cam_off[(size_t)cb + 1] - off_b;
        for (int r = 0; r < np_a; ++r)
          for (int c = 0; c < np_b; ++c) {
            if (off_a + r > off_b + c) continue;
            const double* y = &Y[(size_t)(s + a) * WB + 3 * r];
            const double* w = &Wblk[(size_t)(s + b) * WB + 3 * c];
            St[(size_t)(off_a + r) * ncp + off_b + c] -= y[0] * w[0] + y[1] * w[1] + y[2] * w[2];
          }
      }
  }
  // k_unc_component
  std::vector<double>& Yc = out.Yc;
  Yc.clear();
  if (con) {
    Yc.assign((size_t)con->n_entries() * WB, 0.0);
    for (int32_t k = 0; k < con->n_comp; ++k) {
      const int64_t p0 = con->comp_pt[(size_t)k];
      const int m = (int)(con->comp_pt[(size_t)k + 1] - p0), n = 3 * m;
      const int32_t* pts = &con->pts[(size_t)p0];
      std::vector<double> Vt((size_t)n * (n + 1) / 2, 0.0), pa((size_t)n * MAX_NC), pb((size_t)n * MAX_NC), Zs((size_t)n * G), col((size_t)n), diag0((size_t)n);
      for (int i = 0; i < m; ++i) {
        const int64_t p = pts[i];
        double V[6] = {0, 0, 0, 0, 0, 0};
        for (int64_t a = plan.pt_start[(size_t)p]; a < plan.pt_start[(size_t)p + 1]; ++a)
          for (int e = 0; e < 6; ++e) V[e] += Vobs[(size_t)a * 6 + e];
        for (int e = 0; e < 6; ++e) Vt[(size_t)cov_tri(3 * i + cov_sym3_col(e), 3 * i + cov_sym3_row(e))] = V[e];
      }
      for (int64_t r = con->comp_row[(size_t)k]; r < con->comp_row[(size_t)k + 1]; ++r)
        for (int s = 0; s < 8; ++s)
          for (int s2 = 0; s2 < 8; ++s2) {
            const double cc = row_coef[(size_t)r * 8 + s] * row_coef[(size_t)r * 8 + s2];
            if (cc == 0.0) continue;
            const int ri = 3 * con->row_loc[(size_t)r * 8 + s], rj = 3 * con->row_loc[(size_t)r * 8 + s2];
            for (int a = 0; a < 3; ++a)
              for (int b = 0; b < 3; ++b)
                if (ri + a >= rj + b) Vt[(size_t)cov_tri(ri + a, rj + b)] += cc * row_u[(size_t)r * 3 + a] * row_u[(size_t)r * 3 + b];
          }
      for (int i = 0; i < n; ++i) diag0[(size_t)i] = Vt[(size_t)cov_tri(i, i)];
      if (!cov_tri_cholesky(Vt.data(), n, diag0.data())) {
        error = cov_con_msg_component(what, pts[0]);
        return CBA_ERR_NUMERIC;
      }
      cov_tri_invert(Vt.data(), n, col.data());
      for (int i = 0; i < m; ++i) {
        double N[3][G];
        cov_gauge_point(d->points[3 * (size_t)pts[i]], d->points[3 * (size_t)pts[i] + 1], d->points[3 * (size_t)pts[i] + 2], N);
        for (int a = 0; a < 3; ++a)
          for (int j = 0; j < G; ++j) pa[(size_t)(3 * i + a) * G + j] = N[a][j];
      }
      for (int it = 0; it < n * G; ++it) pb[(size_t)it] = cov_tri_lower_dot(Vt.data(), it / G, pa.data(), G, it % G);
      for (int it = 0; it < n * G; ++it) {
        const int i = it / G, j = it % G;
        Zs[(size_t)it] = cov_tri_upper_dot(Vt.data(), n, i, pb.data(), G, j);
        Zall[(size_t)pts[i / 3] * 3 * G + (size_t)(i % 3) * G + j] = Zs[(size_t)it];
      }
      for (int i = 0; i < m; ++i) {
        for (int e = 0; e < 6; ++e) Vinv[(size_t)pts[i] * 6 + e] = cov_tri_gram(Vt.data(), n, 3 * i + cov_sym3_row(e), 3 * i + cov_sym3_col(e));
        const double* Np = &pa[(size_t)3 * i * G];  // (still the gauge rows)
        const double* Z = &Zs[(size_t)3 * i * G];
        for (int j = 0; j < G; ++j)
          for (int mm = j; mm < G; ++mm) D[(size_t)j * G + mm] += Np[j] * Z[mm] + Np[G + j] * Z[G + mm] + Np[2 * G + j] * Z[2 * G + mm];
      }
      const int64_t q0 = con->comp_cam[(size_t)k];
      const int nc = (int)(con->comp_cam[(size_t)k + 1] - q0);
      for (int cc = 0; cc < nc; ++cc) {
        const int32_t cam = con->cams[(size_t)(q0 + cc)], off = plan.cam_off[(size_t)cam], np = plan.cam_off[(size_t)cam + 1] - off;
        std::fill(pa.begin(), pa.end(), 0.0);
        for (int64_t a = con->cc_obs[(size_t)(q0 + cc)]; a < con->cc_obs[(size_t)(q0 + cc) + 1]; ++a)
          for (int e = 0; e < WB; ++e) pa[(size_t)(3 * con->obs_loc[(size_t)a] + e % 3) * MAX_NC + e / 3] += Wblk[(size_t)con->obs_pos[(size_t)a] * WB + e];
        for (int it = 0; it < n * MAX_NC; ++it) pb[(size_t)it] = cov_tri_lower_dot(Vt.data(), it / MAX_NC, pa.data(), MAX_NC, it % MAX_NC);
        for (int r = 0; r < np; ++r)
          for (int j = 0; j < G; ++j) {
            double v = 0.0;
            for (int i = 0; i < n; ++i) v += pa[(size_t)i * MAX_NC + r] * Zs[(size_t)i * G + j];
            B[(size_t)(off + r) * G + j] += -v;
          }
        for (int it = 0; it < n * MAX_NC; ++it) {
          const int i = it / MAX_NC, r = it % MAX_NC;
          const double y = cov_tri_upper_dot(Vt.data(), n, i, pb.data(), MAX_NC, r);
          pa[(size_t)it] = y;
          Yc[(size_t)(con->entry_start[(size_t)pts[i / 3]] + cc) * WB + 3 * r + (i % 3)] = y;
        }
        for (int c2 = cc; c2 < nc; ++c2) {
          const int32_t cam_b = con->cams[(size_t)(q0 + c2)], off_b = plan.cam_off[(size_t)cam_b], np_b = plan.cam_off[(size_t)cam_b + 1] - off_b;
          for (int r = 0; r < np; ++r)
            for (int c = 0; c < np_b; ++c) {
              if (off + r > off_b + c) continue;
              double v = 0.0;
              for (int64_t a = con->cc_obs[(size_t)(q0 + c2)]; a < con->cc_obs[(size_t)(q0 + c2) + 1]; ++a) {
                const double* w = &Wblk[(size_t)con->obs_pos[(size_t)a] * WB + 3 * c];
                const double* y = &pa[(size_t)3 * con->obs_loc[(size_t)a] * MAX_NC + r];
                v += y[0] * w[0] + y[MAX_NC] * w[1] + y[2 * MAX_NC] * w[2];
              }
              St[(size_t)(off + r) * ncp + off_b + c] += -v;
            }
        }
      }
    }
  }
  for (int j = 0; j < G; ++j)
    for (int m = j + 1; m < G; ++m) D[(size_t)m * G + j] = D[(size_t)j * G + m];
  if (!std::isfinite(cost) || !cov_spd_inverse(D, G)) {
    error = cov_msg_gauge(what, G);
    return CBA_ERR_NUMERIC;
  }
  out.cost = cost;
  out.sigma0_sq = 2.0 * cost / (double)plan.dof;
  // k_unc_assemble, the factorisation and k_unc_ttt
  for (int32_t row = 0; row < ncp; ++row)
    for (int32_t col = row; col < ncp; ++col) {
      double v = St[(size_t)row * ncp + col];
      int32_t cr = 0, cc = 0;
      while (plan.cam_off[(size_t)cr + 1] <= row) ++cr;
      while (plan.cam_off[(size_t)cc + 1] <= col) ++cc;
      if (cr == cc) v += U[((size_t)cr * MAX_NC + (row - plan.cam_off[(size_t)cr])) * MAX_NC + (col - plan.cam_off[(size_t)cr])];
      for (int j = 0; j < G; ++j) {
        double sdb = 0.0;
        for (int m = 0; m < G; ++m) sdb += D[(size_t)j * G + m] * B[(size_t)col * G + m];
        v += B[(size_t)row * G + j] * sdb;
      }
      St[(size_t)row * ncp + col] = v;
      St[(size_t)col * ncp + row] = v;
    }
  if (!cov_spd_inverse(St, ncp)) {
    error = cov_msg_not_pd(what);
    return CBA_ERR_NUMERIC;
  }
  out.C = std::move(St);
  return CBA_OK;
}

// cov_outputs<G> of covariance_lib.hip: the point blocks (k_unc_point_cov: a free point's terms are its observations, a constrained point's
// the (camera, Y block) entries of its component), the checks of the results and the caller's arrays, written only when every check has passed.
template <int G>
int cov_replay_outputs(const cba_cov_desc* d, const CovConPlan* con, const CovReplay& rp, const std::string& what, std::string& error, cba_cov_out* out) {
  constexpr int WB = 3 * MAX_NC;
  const CovPlan& plan = rp.plan;
  const int32_t ncp = plan.ncp();
  const int64_t n_points = d->n_points;
  const std::vector<double>& C = rp.C;
  std::vector<double> point_cov;
  if (out->point_cov) {
    std::vector<double> E, F;
    cov_gauge_terms<G>(ncp, C.data(), rp.B.data(), rp.Dinv.data(), E, F);
    point_cov.resize((size_t)n_points * 6);
    for (int64_t p = 0; p < n_points; ++p) {
      const bool in_row = con && con->in_row[(size_t)p];
      const int64_t s = in_row ? con->entry_start[(size_t)p] : plan.pt_start[(size_t)p];
      const int64_t k = (in_row ? con->entry_start[(size_t)p + 1] : plan.pt_start[(size_t)p + 1]) - s;
      const int32_t* cams = in_row ? con->entry_cam.data() : rp.cam_sorted.data();
      const double* Yb = in_row ? rp.Yc.data() : rp.Y.data();
      const double (*Z)[G] = reinterpret_cast<const double (*)[G]>(&rp.Z[(size_t)p * 3 * G]);
      double full[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
      for (int64_t a = 0; a < k; ++a) {
        const int32_t ca = cams[(size_t)(s + a)], off_a = plan.cam_off[(size_t)ca], np_a = plan.cam_off[(size_t)ca + 1] - off_a;
        const double* ya = &Yb[(size_t)(s + a) * WB];
        for (int64_t b = 0; b < k; ++b) {
          const int32_t cb = cams[(size_t)(s + b)], off_b = plan.cam_off[(size_t)cb], np_b = plan.cam_off[(size_t)cb + 1] - off_b;
          const double* yb = &Yb[(size_t)(s + b) * WB];
          for (int r = 0; r < np_a; ++r) {
            double t3[3] = {0, 0, 0};
            for (int c = 0; c < np_b; ++c)
              for (int q = 0; q < 3; ++q) t3[q] += C[(size_t)(off_a + r) * ncp + off_b + c] * yb[3 * c + q];
            for (int pp = 0; pp < 3; ++pp)
              for (int q = 0; q < 3; ++q) full[pp][q] += ya[3 * r + pp] * t3[q];
          }
        }
        for (int r = 0; r < np_a; ++r) {
          double t3[3] = {0, 0, 0};
          for (int j = 0; j < G; ++j)
            for (int q = 0; q < 3; ++q) t3[q] += E[(size_t)(off_a + r) * G + j] * Z[q][j];
          for (int pp = 0; pp < 3; ++pp)
            for (int q = 0; q < 3; ++q) full[pp][q] += 2.0 * ya[3 * r + pp] * t3[q];
        }
      }
      double P[6];
      cov_point_base(&rp.Vinv[(size_t)p * 6], Z, F.data(), P);
      int e = 0;
      for (int pp = 0; pp < 3; ++pp)
        for (int q = pp; q < 3; ++q) {
          point_cov[(size_t)p * 6 + e] = rp.sigma0_sq * (P[e] + 0.5 * (full[pp][q] + full[q][pp]));
          ++e;
        }
    }
    for (double v : point_cov)
      if (!std::isfinite(v)) { error = cov_msg_not_finite(what, "point"); return CBA_ERR_NUMERIC; }
  }
  for (double v : C)
    if (!std::isfinite(v)) { error = cov_msg_not_finite(what, "camera"); return CBA_ERR_NUMERIC; }
  if (out->point_cov) std::copy(point_cov.begin(), point_cov.end(), out->point_cov);
  cov_write_outputs(plan, C, rp.sigma0_sq, rp.cost, out);
  return CBA_OK;
}

}  // namespace cba
