// The thread body and the host-side checks of k_traj_refine / cba_reconstruct_trajectories_refined
// (include/caliscope/trajectory_refine.h, where the mathematics and the constants below are stated).  Compiled by hipcc into the
// kernel of trajectory_lib.hip and by g++ into tests/native/trajectory_refine_harness.cpp, which runs the same routine slot by slot.
//
// Registers only: X, H, g, the cost and lambda are named scalars, whatever a view contributes is consumed inside the camera loop,
// and the set of views in use lives in the global grid view_state[c][s] (one byte per cell) — nothing is indexed by the camera
// loop's counter but the wave-uniform camera tables and the grids.  Lanes finish after different numbers of evaluations: every loop
// runs to its cap under a per-lane flag, and the camera loop is never left early.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/caliscope/trajectory_refine.h"
#include "trajectory_math.h"

namespace cba {

constexpr double REFINE_LAMBDA0 = 1e-3, REFINE_LAMBDA_DOWN = 0.1, REFINE_LAMBDA_UP = 10.0, REFINE_LAMBDA_MIN = 1e-15;
constexpr double REFINE_XTOL = 1e-9;   // a proposed step of ||delta|| <= XTOL (XTOL + ||X||) ends the round
constexpr double REFINE_GTOL = 1e-4;   // ||g||_inf, px^2 / m
constexpr int REFINE_NO_POINT = 0, REFINE_CONVERGED = 1, REFINE_ITERATION_CAP = 2, REFINE_KEPT_DLT = 3;
constexpr int VIEW_NONE = 0, VIEW_USED = 1, VIEW_REJECTED = 2;

CBA_HD bool refine_finite(double v) { return v - v == 0.0; }

// What one pass over the cameras leaves: cost, normal equations (upper triangle), gradient, and of the views in use the number, the
// sum and the largest of d_c^2 with the camera that has it (the lowest rank on a tie).  ok: every view in front, cost finite.
struct RefineEval {
  double F, h00, h01, h02, h11, h12, h22, g0, g1, g2, sum_d2, max_d2;
  int32_t worst, views;
  bool ok;
};

CBA_HD void traj_refine_eval(int32_t n_cams, int64_t n_slots, int64_t s, const int32_t* cam_model, const double* cam_intr, const double* cam_P,
                             const double* xy, const uint8_t* view_state, int loss, double f_scale, double X, double Y, double Z, RefineEval& o) {
  o.F = o.h00 = o.h01 = o.h02 = o.h11 = o.h12 = o.h22 = o.g0 = o.g1 = o.g2 = o.sum_d2 = 0.0;
  o.max_d2 = -1.0;
  o.worst = -1;
  o.views = 0;
  o.ok = true;
  for (int32_t cam = 0; cam < n_cams; ++cam) {
    const int64_t cell = (int64_t)cam * n_slots + s;
    if (view_state[cell] != VIEW_USED) continue;
    const double u = xy[2 * cell], v = xy[2 * cell + 1];
    const double* P = cam_P + 12 * cam;
    const double* in = cam_intr + 9 * cam;
    const double Xc = P[3] + P[0] * X + P[1] * Y + P[2] * Z;
    const double Yc = P[7] + P[4] * X + P[5] * Y + P[6] * Z;
    const double Zc = P[11] + P[8] * X + P[9] * Y + P[10] * Z;
    ++o.views;
    if (!(Zc > 0.0)) { o.ok = false; continue; }
    const double iz = 1.0 / Zc, x = Xc * iz, y = Yc * iz;
    Lens L;
    if (cam_model[cam] != MODEL_PINHOLE_BC5) lens_fisheye(in + 4, x, y, &L); else lens_pinhole(in + 4, x, y, &L);
    const double e0 = (in[2] - u) + in[0] * L.xd, e1 = (in[3] - v) + in[1] * L.yd;
    // d(pixel)/dX_c (2 x 3), then the point block B = G R
    const double a00 = in[0] * L.dxx * iz, a01 = in[0] * L.dxy * iz, a02 = -(a00 * x + a01 * y);
    const double a10 = in[1] * L.dyx * iz, a11 = in[1] * L.dyy * iz, a12 = -(a10 * x + a11 * y);
    // scipy's treatment of each scalar residual gives the cost and rho' e (= row scale x scaled residual), hence F and g as scipy has
    // them.  The rows of H are weighted by rho' alone: scipy's second-order term 2 rho'' e^2 takes the whole of rho' away wherever
    // the loss is linear in |e|, and at a DLT point dragged by an outlier that is every row (H = 2^-52 J^T J: eighteen refused steps).
    double js0, js1, r0, r1;
    o.F += 0.5 * robust_one(loss, f_scale, e0, &js0, &r0);
    o.F += 0.5 * robust_one(loss, f_scale, e1, &js1, &r1);
    const double q0 = js0 * r0, q1 = js1 * r1;                           // rho' e
    const double w0 = e0 != 0.0 ? q0 / e0 : 1.0, w1 = e1 != 0.0 ? q1 / e1 : 1.0;  // rho'
    const double b00 = a00 * P[0] + a01 * P[4] + a02 * P[8], b01 = a00 * P[1] + a01 * P[5] + a02 * P[9], b02 = a00 * P[2] + a01 * P[6] + a02 * P[10];
    const double b10 = a10 * P[0] + a11 * P[4] + a12 * P[8], b11 = a10 * P[1] + a11 * P[5] + a12 * P[9], b12 = a10 * P[2] + a11 * P[6] + a12 * P[10];
    o.h00 += w0 * b00 * b00 + w1 * b10 * b10;
    o.h01 += w0 * b00 * b01 + w1 * b10 * b11;
    o.h02 += w0 * b00 * b02 + w1 * b10 * b12;
    o.h11 += w0 * b01 * b01 + w1 * b11 * b11;
    o.h12 += w0 * b01 * b02 + w1 * b11 * b12;
    o.h22 += w0 * b02 * b02 + w1 * b12 * b12;
    o.g0 += b00 * q0 + b10 * q1;
    o.g1 += b01 * q0 + b11 * q1;
    o.g2 += b02 * q0 + b12 * q1;
    const double d2 = e0 * e0 + e1 * e1;
    o.sum_d2 += d2;
    if (d2 > o.max_d2) { o.max_d2 = d2; o.worst = cam; }
  }
  o.ok = o.ok && refine_finite(o.F);
}

// k_traj_refine, slot s.  xyz[s] holds the DLT point on entry and the refined point on return; valid is only read.
CBA_HD void traj_refine_slot(int32_t n_cams, int64_t n_slots, int64_t s, const uint8_t* cam_posed, const int32_t* cam_model, const double* cam_intr,
                             const double* cam_P, const double* xy, int loss, double f_scale, int max_iter, double reject_px, int max_reject,
                             int min_views, const uint8_t* valid, double* xyz, uint8_t* view_state, int32_t* views, double* rms_px, double* max_px,
                             int32_t* iterations, uint8_t* status) {
  const bool live = valid[s] == 1;
  int32_t active = 0;
  for (int32_t cam = 0; cam < n_cams; ++cam) {
    const int64_t cell = (int64_t)cam * n_slots + s;
    const bool used = live && cam_posed[cam] && !traj_is_nan(xy[2 * cell]);
    view_state[cell] = used ? VIEW_USED : VIEW_NONE;
    active += used ? 1 : 0;
  }
  if (!live) {
    views[s] = 0;
    rms_px[s] = max_px[s] = traj_nan();
    iterations[s] = 0;
    status[s] = REFINE_NO_POINT;
    return;
  }
  double X = xyz[3 * s], Y = xyz[3 * s + 1], Z = xyz[3 * s + 2];
  RefineEval cur, tri;
  cur.sum_d2 = cur.max_d2 = traj_nan();
  cur.views = active;
  cur.worst = -1;
  int32_t evals = 0;
  int st = REFINE_CONVERGED;
  bool finished = false;
  const int rounds = reject_px > 0.0 ? max_reject : 0;
  for (int round = 0; round <= rounds; ++round) {
    double lam = REFINE_LAMBDA0;
    bool done = finished;
    for (int k = 0; k < max_iter; ++k) {
      if (done) continue;
      double d0 = 0.0, d1 = 0.0, d2 = 0.0;
      if (k > 0) {
        const double A[6] = {cur.h00 * (1.0 + lam), cur.h01, cur.h02, cur.h11 * (1.0 + lam), cur.h12, cur.h22 * (1.0 + lam)};
        const double rhs[3] = {-cur.g0, -cur.g1, -cur.g2};
        double Lf[6], w[3], d[3];
        if (!chol3(A, Lf)) { lam *= REFINE_LAMBDA_UP; continue; }  // (no evaluation is spent on it)
        chol3_fwd(Lf, rhs, w);
        chol3_bwd(Lf, w, d);
        d0 = d[0]; d1 = d[1]; d2 = d[2];
        if (!(sqrt(d0 * d0 + d1 * d1 + d2 * d2) > REFINE_XTOL * (REFINE_XTOL + sqrt(X * X + Y * Y + Z * Z)))) {
          done = true;
          st = REFINE_CONVERGED;
          continue;
        }
      }
      traj_refine_eval(n_cams, n_slots, s, cam_model, cam_intr, cam_P, xy, view_state, loss, f_scale, X + d0, Y + d1, Z + d2, tri);
      ++evals;
      if (k == 0) {
        if (!tri.ok) {  // (round 0: the DLT point itself cannot be evaluated)
          done = finished = true;
          if (round == 0) st = REFINE_KEPT_DLT;
          continue;
        }
        cur = tri;
      } else if (tri.ok && tri.F < cur.F) {
        X += d0; Y += d1; Z += d2;
        cur = tri;
        lam = lam * REFINE_LAMBDA_DOWN > REFINE_LAMBDA_MIN ? lam * REFINE_LAMBDA_DOWN : REFINE_LAMBDA_MIN;
      } else {
        lam *= REFINE_LAMBDA_UP;
        continue;
      }
      const double g_inf = fmax(fabs(cur.g0), fmax(fabs(cur.g1), fabs(cur.g2)));
      if (g_inf <= REFINE_GTOL) { done = true; st = REFINE_CONVERGED; }
    }
    if (finished) continue;
    if (!done) st = REFINE_ITERATION_CAP;
    const bool drop = round < rounds && cur.worst >= 0 && cur.max_d2 > reject_px * reject_px && cur.views - 1 >= min_views;
    if (drop) view_state[(int64_t)cur.worst * n_slots + s] = VIEW_REJECTED;
    finished = !drop;
  }
  if (st != REFINE_KEPT_DLT) {
    xyz[3 * s] = X;
    xyz[3 * s + 1] = Y;
    xyz[3 * s + 2] = Z;
  }
  views[s] = cur.views;
  rms_px[s] = st != REFINE_KEPT_DLT ? sqrt(cur.sum_d2 / (double)cur.views) : traj_nan();
  max_px[s] = st != REFINE_KEPT_DLT ? sqrt(cur.max_d2) : traj_nan();
  iterations[s] = evals;
  status[s] = (uint8_t)st;
}

}  // namespace cba

// ---- host side: the checks of the refinement ---------------------------------------------------------------------------------------
#include <string>

namespace cba {

// bytes of the device buffers the refinement adds: view_state, and views, rms_px, max_px, iterations, status per slot
inline double traj_refine_device_bytes(const cba_traj_desc* d) {
  const double slots = (double)d->n_frames * (double)d->n_traj;
  return (double)d->n_cams * slots + slots * 25.0;
}

// 0, or -1 (CBA_ERR_INVALID) with `msg` naming the field
inline int traj_refine_validate(const cba_traj_refine* r, std::string& msg) {
  const std::string what = "cba_reconstruct_trajectories_refined: ";
  if (!r) { msg = what + "refine: null argument"; return -1; }
  if (r->loss < LOSS_LINEAR || r->loss > LOSS_ARCTAN) { msg = what + "loss: unknown loss " + std::to_string(r->loss); return -1; }
  if (!std::isfinite(r->f_scale)) { msg = what + "f_scale is not finite"; return -1; }
  if (r->loss != LOSS_LINEAR && !(r->f_scale > 0.0)) { msg = what + "f_scale must be positive with a robust loss, got " + std::to_string(r->f_scale); return -1; }
  if (r->max_iter < 1) { msg = what + "max_iter must be at least 1, got " + std::to_string(r->max_iter); return -1; }
  if (!std::isfinite(r->reject_px) || r->reject_px < 0.0) { msg = what + "reject_px must be finite and not negative, got " + std::to_string(r->reject_px); return -1; }
  if (r->min_views < 2) { msg = what + "min_views must be at least 2, got " + std::to_string(r->min_views); return -1; }
  if (r->max_reject < 0) { msg = what + "max_reject must not be negative, got " + std::to_string(r->max_reject); return -1; }
  return 0;
}

// traj_validate, the checks above, and the memory check with the refinement's buffers counted.  memory <= 0: not checked.
inline int traj_refined_validate(const cba_traj_desc* d, const cba_traj_refine* r, double memory, std::string& msg) {
  int rc = traj_validate(d, 0.0, msg);
  if (rc) return rc;
  rc = traj_refine_validate(r, msg);
  if (rc) return rc;
  const double bytes = traj_device_bytes(d) + traj_refine_device_bytes(d);
  if (d->n_rows > 0 && memory > 0.0 && bytes > memory) {
    msg = "cba_reconstruct_trajectories_refined: the grid of " + std::to_string(d->n_cams) + " cameras x " + std::to_string(d->n_frames) +
          " frames x " + std::to_string(d->n_traj) + " trajectories needs " + std::to_string((long long)bytes) + " bytes of device memory, " +
          std::to_string((long long)memory) + " are available";
    return -4;
  }
  return 0;
}

}  // namespace cba
