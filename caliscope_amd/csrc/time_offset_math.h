// The thread bodies, the one-workgroup solve, the host-side checks and the host's driver of cba_estimate_time_offsets
// (include/caliscope/time_offsets.h, where the model, the algorithm and the constants below are stated).  Compiled by hipcc into the
// kernels and the entry point of time_offset_lib.hip and by g++ into tests/native/time_offset_harness.cpp, which runs the same
// routines slot by slot and the driver as it is.
//
// Registers only in the per-slot bodies: X, V, H, g and the factor are named scalars, whatever a view contributes is consumed inside
// the camera loop, and what is indexed by the camera loop's counter (q_c, d_c, b_c) leaves the thread through `emit` inside the loop.
// The camera loop is never left early and runs for every lane of a wave, live or not: `emit` reduces over the wave.
//
// Columns.  The posed cameras are numbered 0 .. n_cols - 1 in ascending order (cam_col[c], -1: unposed); offsets, steps and the
// rows and columns of the Gram matrix are indexed by column.  The column of the reference camera holds q_n = L^-1 g.
//
// Q[(3 col + k) ld + s], k < 3, ld = n_slots rounded up to SYNC_GRAM_CHUNK: neighbouring threads store neighbouring doubles, and
// k_sync_gram reads whole chunks without a bound (the pad is zero).
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/caliscope/time_offsets.h"
#include "trajectory_refine_math.h"

namespace cba {

constexpr int SYNC_BLOCK = 256;          // threads of a workgroup, every kernel
constexpr int SYNC_GRAM_CHUNK = 256;     // slots of a chunk of k_sync_gram
constexpr int SYNC_GRAM_GROUPS = 512;    // most workgroups of k_sync_gram: one partial each
constexpr int SYNC_LD = CBA_OFFSET_MAX_CAMS;  // row length of a partial, of S and of the inverse of its factor
constexpr double SYNC_RESOLVE = 1e-10;   // a trial is kept when F(trial) <= F + RESOLVE (1 + F)
constexpr double SYNC_PRED_ROW = 1e-18;  // px^2 per row: a round ends after a kept step predicted to lower F by no more
constexpr int SYNC_MAX_HALVINGS = 10;
constexpr double SYNC_TOL_FRACTION = 1e-6;

CBA_HD double sync_inf() { return __builtin_huge_val(); }

// pixel of the point (px, py, pz) in camera (P, in, model); false: behind the camera
CBA_HD bool sync_project(const double* P, const double* in, int model, double px, double py, double pz, double* u, double* v) {
  const double Xc = P[3] + P[0] * px + P[1] * py + P[2] * pz;
  const double Yc = P[7] + P[4] * px + P[5] * py + P[6] * pz;
  const double Zc = P[11] + P[8] * px + P[9] * py + P[10] * pz;
  if (!(Zc > 0.0)) { *u = *v = traj_nan(); return false; }
  const double iz = 1.0 / Zc, x = Xc * iz, y = Yc * iz;
  Lens L;
  if (model != MODEL_PINHOLE_BC5) lens_fisheye(in + 4, x, y, &L); else lens_pinhole(in + 4, x, y, &L);
  *u = in[2] + in[0] * L.xd;
  *v = in[3] + in[1] * L.yd;
  return true;
}

// One view at the point X + V lag: residual r = pi - u, B = d pi / dX (2 x 3), a = B V, the IRLS weight and rho.
struct SyncView {
  double e0, e1, b00, b01, b02, b10, b11, b12, a0, a1, w, rho;
};

CBA_HD void sync_view(const double* P, const double* in, int model, double u, double v, double X, double Y, double Z, double Vx, double Vy, double Vz,
                      double lag, double huber, SyncView& o) {
  const double px = X + Vx * lag, py = Y + Vy * lag, pz = Z + Vz * lag;
  const double Xc = P[3] + P[0] * px + P[1] * py + P[2] * pz;
  const double Yc = P[7] + P[4] * px + P[5] * py + P[6] * pz;
  const double Zc = P[11] + P[8] * px + P[9] * py + P[10] * pz;
  const bool front = Zc > 0.0;
  const double iz = front ? 1.0 / Zc : 0.0, x = Xc * iz, y = Yc * iz;
  Lens L;
  if (model != MODEL_PINHOLE_BC5) lens_fisheye(in + 4, x, y, &L); else lens_pinhole(in + 4, x, y, &L);
  o.e0 = (in[2] - u) + in[0] * L.xd;
  o.e1 = (in[3] - v) + in[1] * L.yd;
  const double a00 = in[0] * L.dxx * iz, a01 = in[0] * L.dxy * iz, a02 = -(a00 * x + a01 * y);
  const double a10 = in[1] * L.dyx * iz, a11 = in[1] * L.dyy * iz, a12 = -(a10 * x + a11 * y);
  o.b00 = a00 * P[0] + a01 * P[4] + a02 * P[8]; o.b01 = a00 * P[1] + a01 * P[5] + a02 * P[9]; o.b02 = a00 * P[2] + a01 * P[6] + a02 * P[10];
  o.b10 = a10 * P[0] + a11 * P[4] + a12 * P[8]; o.b11 = a10 * P[1] + a11 * P[5] + a12 * P[9]; o.b12 = a10 * P[2] + a11 * P[6] + a12 * P[10];
  o.a0 = o.b00 * Vx + o.b01 * Vy + o.b02 * Vz;
  o.a1 = o.b10 * Vx + o.b11 * Vy + o.b12 * Vz;
  const double r2 = o.e0 * o.e0 + o.e1 * o.e1, r = sqrt(r2);
  const bool outside = huber > 0.0 && r > huber;
  o.w = outside ? huber / r : 1.0;
  o.rho = outside ? huber * (2.0 * r - huber) : r2;
  if (!front) o.rho = sync_inf();  // (the trial is refused)
}

CBA_HD double sync_clamp(double v, double limit) { return v > limit ? limit : (v < -limit ? -limit : v); }

// What k_sync_build reads beside the grids.
struct SyncBuildArgs {
  int32_t n_cams, n_cols, ref_col;
  int64_t n_slots, n_traj, ld;
  const int32_t* cam_col;
  const int32_t* cam_model;
  const double* cam_intr;
  const double* cam_P;
  const double* xy;
  const double* ft;
  const double* frame_time;
  const uint8_t* valid;
  const double* X0;
  const double* dX;
  const double* V;
  const double* delta0;  // [n_cols]
  const double* ddelta;  // [n_cols]
  double alpha, max_offset, huber;
};

// k_sync_build, slot s (live: s < n_slots; a lane beyond takes part in `emit` with zeros).  Evaluates at X0 + alpha dX and
// delta0 + alpha ddelta.  Pass 1: H, g, the slot's part of F (returned), the factor to Lbuf[k ld + s].  Pass 2: emit(col, q, d, b)
// once per posed camera, ascending, q = L^-1 E_c (zero without a view), for the reference column q = L^-1 g, and writes Q.
template <class Emit>
CBA_HD double sync_build_slot(const SyncBuildArgs& A, int64_t s, bool live, double* Q, double* Lbuf, Emit&& emit) {
  const bool has = live && A.valid[s] != 0;
  const int64_t sl = live ? s : 0;
  double X = 0.0, Y = 0.0, Z = 0.0, Vx = 0.0, Vy = 0.0, Vz = 0.0, tau = 0.0;
  if (has) {
    X = A.X0[3 * s]; Y = A.X0[3 * s + 1]; Z = A.X0[3 * s + 2];
    if (A.alpha != 0.0) { X += A.alpha * A.dX[3 * s]; Y += A.alpha * A.dX[3 * s + 1]; Z += A.alpha * A.dX[3 * s + 2]; }
    Vx = A.V[3 * s]; Vy = A.V[3 * s + 1]; Vz = A.V[3 * s + 2];
    tau = A.frame_time[s / A.n_traj];
  }
  double F = 0.0, h00 = 0.0, h01 = 0.0, h02 = 0.0, h11 = 0.0, h12 = 0.0, h22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
  for (int32_t cam = 0; cam < A.n_cams; ++cam) {
    const int32_t col = A.cam_col[cam];
    if (col < 0) continue;  // (uniform)
    const int64_t cell = (int64_t)cam * A.n_slots + sl;
    const double u = has ? A.xy[2 * cell] : traj_nan();
    if (traj_is_nan(u)) continue;
    const double delta = sync_clamp(A.delta0[col] + A.alpha * A.ddelta[col], A.max_offset);
    SyncView w;
    sync_view(A.cam_P + 12 * cam, A.cam_intr + 9 * cam, A.cam_model[cam], u, A.xy[2 * cell + 1], X, Y, Z, Vx, Vy, Vz, A.ft[cell] - tau + delta, A.huber, w);
    F += 0.5 * w.rho;
    h00 += w.w * (w.b00 * w.b00 + w.b10 * w.b10);
    h01 += w.w * (w.b00 * w.b01 + w.b10 * w.b11);
    h02 += w.w * (w.b00 * w.b02 + w.b10 * w.b12);
    h11 += w.w * (w.b01 * w.b01 + w.b11 * w.b11);
    h12 += w.w * (w.b01 * w.b02 + w.b11 * w.b12);
    h22 += w.w * (w.b02 * w.b02 + w.b12 * w.b12);
    g0 += w.w * (w.b00 * w.e0 + w.b10 * w.e1);
    g1 += w.w * (w.b01 * w.e0 + w.b11 * w.e1);
    g2 += w.w * (w.b02 * w.e0 + w.b12 * w.e1);
  }
  // a slot without a point, or whose H has no factor, contributes nothing to the system and gets no step: L = 0
  const double Hm[6] = {h00, h01, h02, h11, h12, h22};
  double Lf[6];
  const bool ok = has && chol3(Hm, Lf);
  if (!ok) Lf[0] = Lf[1] = Lf[2] = Lf[3] = Lf[4] = Lf[5] = 0.0;
  if (live) {
    Lbuf[s] = Lf[0]; Lbuf[A.ld + s] = Lf[1]; Lbuf[2 * A.ld + s] = Lf[2];
    Lbuf[3 * A.ld + s] = Lf[3]; Lbuf[4 * A.ld + s] = Lf[4]; Lbuf[5 * A.ld + s] = Lf[5];
  }
  const double gv[3] = {g0, g1, g2};
  double qn[3];
  chol3_fwd(Lf, gv, qn);
  for (int32_t cam = 0; cam < A.n_cams; ++cam) {
    const int32_t col = A.cam_col[cam];
    if (col < 0) continue;  // (uniform)
    const int64_t cell = (int64_t)cam * A.n_slots + sl;
    const double u = has ? A.xy[2 * cell] : traj_nan();
    double q[3] = {0.0, 0.0, 0.0}, dc = 0.0, bc = 0.0;
    if (!traj_is_nan(u)) {
      const double delta = sync_clamp(A.delta0[col] + A.alpha * A.ddelta[col], A.max_offset);
      SyncView w;
      sync_view(A.cam_P + 12 * cam, A.cam_intr + 9 * cam, A.cam_model[cam], u, A.xy[2 * cell + 1], X, Y, Z, Vx, Vy, Vz, A.ft[cell] - tau + delta, A.huber, w);
      const double E[3] = {w.w * (w.b00 * w.a0 + w.b10 * w.a1), w.w * (w.b01 * w.a0 + w.b11 * w.a1), w.w * (w.b02 * w.a0 + w.b12 * w.a1)};
      chol3_fwd(Lf, E, q);
      dc = w.w * (w.a0 * w.a0 + w.a1 * w.a1);
      bc = w.w * (w.a0 * w.e0 + w.a1 * w.e1);
    }
    if (col == A.ref_col) { q[0] = qn[0]; q[1] = qn[1]; q[2] = qn[2]; dc = bc = 0.0; }  // (uniform)
    if (live) {
      Q[(3 * (int64_t)col) * A.ld + s] = q[0];
      Q[(3 * (int64_t)col + 1) * A.ld + s] = q[1];
      Q[(3 * (int64_t)col + 2) * A.ld + s] = q[2];
    }
    emit(col, dc, bc);
  }
  return F;
}

// k_sync_update, slot s: the kept trial becomes the point (alpha != 0), then the step of the system k_sync_build left:
// dX = -L^-T (q_n + sum q_c d_c) over the columns but the reference's; d is zero for a fixed camera.
CBA_HD void sync_update_slot(int32_t n_cols, int32_t ref_col, int64_t ld, int64_t s, const double* Q, const double* Lbuf, const double* dnew, double alpha,
                             double* X0, double* dX) {
  if (alpha != 0.0) {
    X0[3 * s] += alpha * dX[3 * s];
    X0[3 * s + 1] += alpha * dX[3 * s + 1];
    X0[3 * s + 2] += alpha * dX[3 * s + 2];
  }
  double z[3] = {Q[(3 * (int64_t)ref_col) * ld + s], Q[(3 * (int64_t)ref_col + 1) * ld + s], Q[(3 * (int64_t)ref_col + 2) * ld + s]};
  for (int32_t col = 0; col < n_cols; ++col) {
    if (col == ref_col) continue;
    const double dc = dnew[col];
    z[0] += Q[(3 * (int64_t)col) * ld + s] * dc;
    z[1] += Q[(3 * (int64_t)col + 1) * ld + s] * dc;
    z[2] += Q[(3 * (int64_t)col + 2) * ld + s] * dc;
  }
  const double Lf[6] = {Lbuf[s], Lbuf[ld + s], Lbuf[2 * ld + s], Lbuf[3 * ld + s], Lbuf[4 * ld + s], Lbuf[5 * ld + s]};
  double d[3];
  chol3_bwd(Lf, z, d);
  dX[3 * s] = -d[0];
  dX[3 * s + 1] = -d[1];
  dX[3 * s + 2] = -d[2];
}

// the columns' part of k_sync_update (block 0): the kept trial's offsets, then the new step
CBA_HD void sync_update_col(int32_t col, double alpha, double max_offset, const double* dnew, double* delta0, double* ddelta) {
  if (alpha != 0.0) delta0[col] = sync_clamp(delta0[col] + alpha * ddelta[col], max_offset);
  ddelta[col] = dnew[col];
}

// k_sync_velocity, slot s: the central difference over the nearest slots with a point before and after, both within `gap` frames.
CBA_HD void sync_velocity_slot(int64_t n_frames, int64_t n_traj, int64_t s, int gap, const uint8_t* valid, const double* X, const double* frame_time,
                               double* V, uint8_t* moving) {
  const int64_t f = s / n_traj;
  int64_t before = -1, after = -1;
  for (int k = 1; k <= gap; ++k) {
    if (before < 0 && f - k >= 0 && valid[s - k * n_traj]) before = s - k * n_traj;
    if (after < 0 && f + k < n_frames && valid[s + k * n_traj]) after = s + k * n_traj;
  }
  double v0 = 0.0, v1 = 0.0, v2 = 0.0;
  if (valid[s] && before >= 0 && after >= 0) {
    const double dt = frame_time[after / n_traj] - frame_time[before / n_traj];
    v0 = (X[3 * after] - X[3 * before]) / dt;
    v1 = (X[3 * after + 1] - X[3 * before + 1]) / dt;
    v2 = (X[3 * after + 2] - X[3 * before + 2]) / dt;
  }
  V[3 * s] = v0; V[3 * s + 1] = v1; V[3 * s + 2] = v2;
  if (moving) moving[s] = (v0 != 0.0 || v1 != 0.0 || v2 != 0.0) ? 1 : 0;
}

// k_sync_rows, row i of camera c.  final false: the squared residual at the synchronous start (X, no lag), whether the row is in use and
// whether its slot moves.  final true: the squared residual at X + V lag, and the compensated pixel and the flag of the row.
CBA_HD void sync_row(bool final, int64_t i, int32_t c, int32_t col, int64_t n_traj, const int32_t* cam_model, const double* cam_intr, const double* cam_P,
                     const int64_t* row_slot, const double* row_xy, const double* row_time, const double* frame_time, const uint8_t* valid,
                     const uint8_t* moving, const double* X, const double* V, const double* delta0, double* out_xy, uint8_t* out_used, double* e2,
                     int64_t* used, int64_t* moves) {
  const int64_t s = row_slot[i];
  const double u = row_xy[2 * i], v = row_xy[2 * i + 1];
  const bool in_use = col >= 0 && valid[s] != 0;
  *e2 = 0.0;
  *used = in_use ? 1 : 0;
  *moves = in_use && moving[s] ? 1 : 0;
  double cu = u, cv = v;
  if (in_use) {
    const double* P = cam_P + 12 * c;
    const double* in = cam_intr + 9 * c;
    double pu, pv;
    sync_project(P, in, cam_model[c], X[3 * s], X[3 * s + 1], X[3 * s + 2], &pu, &pv);
    if (final) {
      const double lag = row_time[i] - frame_time[s / n_traj] + delta0[col];
      double mu, mv;
      sync_project(P, in, cam_model[c], X[3 * s] + V[3 * s] * lag, X[3 * s + 1] + V[3 * s + 1] * lag, X[3 * s + 2] + V[3 * s + 2] * lag, &mu, &mv);
      cu = u - (mu - pu);
      cv = v - (mv - pv);
      pu = mu; pv = mv;
    }
    *e2 = (pu - u) * (pu - u) + (pv - v) * (pv - v);
  }
  if (final) {
    out_xy[2 * i] = cu;
    out_xy[2 * i + 1] = cv;
    out_used[i] = in_use ? 1 : 0;
  }
}

// What k_sync_reduce_solve reads and writes.
struct SyncSolveArgs {
  int32_t n_cols, ref_col, n_groups;
  int64_t n_waves;
  const double* partial;    // [n_groups][SYNC_LD][SYNC_LD], entries (i, j) with i <= j < n_cols
  const double* Fw;         // [n_waves]
  const double* Dw;         // [n_waves][n_cols]
  const double* bw;         // [n_waves][n_cols]
  const uint8_t* free_col;  // [n_cols]
  double* dnew;             // [n_cols] the step, 0 for a fixed column
  double* sinv;             // [n_cols] (S^-1)_cc, NaN for a fixed column
  double* scal;             // [4] F, predicted decrease, max |step|, 1: S has a factor
};

#if defined(__HIP_DEVICE_COMPILE__)
#define SYNC_BARRIER() __syncthreads()
#else
#define SYNC_BARRIER() ((void)0)
#endif

// k_sync_reduce_solve as thread t of NT (the host: t = 0, NT = 1).  Sm, Ym: SYNC_LD x SYNC_LD doubles; vec: 3 SYNC_LD doubles;
// idx: SYNC_LD + 2 ints.  Every sum over partials runs in index order within one thread.
CBA_HD void sync_reduce_solve(int t, int NT, const SyncSolveArgs& A, double* Sm, double* Ym, double* vec, int* idx) {
  double* rhs = vec;
  double* diag = vec + SYNC_LD;
  double* y = vec + 2 * SYNC_LD;
  int* nf_p = idx + SYNC_LD;
  int* ok_p = idx + SYNC_LD + 1;
  {  // F: thread t adds the waves t, t + NT, .. in ascending order, thread 0 the NT sums
    double acc = 0.0;
    for (int64_t w = t; w < A.n_waves; w += NT) acc += A.Fw[w];
    Ym[t] = acc;
  }
  if (t == 0) {
    int n = 0;
    for (int32_t col = 0; col < A.n_cols; ++col)
      if (A.free_col[col]) idx[n++] = col;
    *nf_p = n;
    *ok_p = 1;
  }
  SYNC_BARRIER();
  const int nf = *nf_p;
  double F = 0.0, qnqn = 0.0;
  if (t == 0) {
    for (int i = 0; i < NT; ++i) F += Ym[i];
    for (int32_t g = 0; g < A.n_groups; ++g) qnqn += A.partial[((int64_t)g * SYNC_LD + A.ref_col) * SYNC_LD + A.ref_col];
  }
  SYNC_BARRIER();  // (Ym is free again)
  for (int e = t; e < nf * nf; e += NT) {
    const int a = e / nf, b = e % nf;
    if (a > b) continue;
    const int64_t at = (int64_t)idx[a] * SYNC_LD + idx[b];  // (idx ascends: an entry of the upper triangle)
    double sum = 0.0;
    for (int32_t g = 0; g < A.n_groups; ++g) sum += A.partial[(int64_t)g * SYNC_LD * SYNC_LD + at];
    Sm[a * SYNC_LD + b] = -sum;
    Sm[b * SYNC_LD + a] = -sum;
  }
  for (int a = t; a < nf; a += NT) {
    const int32_t col = idx[a];
    const int32_t lo = col < A.ref_col ? col : A.ref_col, hi = col < A.ref_col ? A.ref_col : col;
    double D = 0.0, b = 0.0, cross = 0.0;
    for (int64_t w = 0; w < A.n_waves; ++w) { D += A.Dw[w * A.n_cols + col]; b += A.bw[w * A.n_cols + col]; }
    for (int32_t g = 0; g < A.n_groups; ++g) cross += A.partial[((int64_t)g * SYNC_LD + lo) * SYNC_LD + hi];
    diag[a] = D;
    rhs[a] = b - cross;
  }
  SYNC_BARRIER();
  for (int a = t; a < nf; a += NT) Sm[a * SYNC_LD + a] += diag[a];
  // Cholesky in place, lower triangle, column by column
  for (int k = 0; k < nf; ++k) {
    SYNC_BARRIER();
    if (t == 0) {
      const double piv = Sm[k * SYNC_LD + k];
      const bool good = piv > 16.0 * EPS_F64 * diag[k];
      if (!good) *ok_p = 0;
      Sm[k * SYNC_LD + k] = good ? sqrt(piv) : 1.0;
    }
    SYNC_BARRIER();
    const double lkk = Sm[k * SYNC_LD + k];
    for (int i = k + 1 + t; i < nf; i += NT) Sm[i * SYNC_LD + k] /= lkk;
    SYNC_BARRIER();
    const int m = nf - k - 1;
    for (int e = t; e < m * m; e += NT) {
      const int i = k + 1 + e / m, j = k + 1 + e % m;
      if (j <= i) Sm[i * SYNC_LD + j] -= Sm[i * SYNC_LD + k] * Sm[j * SYNC_LD + k];
    }
  }
  SYNC_BARRIER();
  const bool ok = *ok_p != 0;
  // column a of the inverse of the factor into row a of Ym; (S^-1)_aa is its squared length
  for (int a = t; a < nf; a += NT) {
    double* x = Ym + a * SYNC_LD;
    double len2 = 0.0;
    for (int i = a; i < nf; ++i) {
      double v = i == a ? 1.0 : 0.0;
      for (int k = a; k < i; ++k) v -= Sm[i * SYNC_LD + k] * x[k];
      x[i] = v / Sm[i * SYNC_LD + i];
      len2 += x[i] * x[i];
    }
    A.sinv[idx[a]] = ok ? len2 : traj_nan();
  }
  for (int32_t col = t; col < A.n_cols; col += NT)
    if (!A.free_col[col]) { A.dnew[col] = 0.0; A.sinv[col] = traj_nan(); }
  if (t == 0) {
    double yy = 0.0, step = 0.0;
    for (int i = 0; i < nf; ++i) {  // L y = rhs
      double v = rhs[i];
      for (int k = 0; k < i; ++k) v -= Sm[i * SYNC_LD + k] * y[k];
      y[i] = v / Sm[i * SYNC_LD + i];
      yy += y[i] * y[i];
    }
    for (int i = nf - 1; i >= 0; --i) {  // L^T d = -y
      double v = -y[i];
      for (int k = i + 1; k < nf; ++k) v -= Sm[k * SYNC_LD + i] * A.dnew[idx[k]];
      const double d = ok ? v / Sm[i * SYNC_LD + i] : 0.0;
      A.dnew[idx[i]] = d;
      step = fmax(step, fabs(d));
    }
    A.scal[0] = F;
    A.scal[1] = 0.5 * (qnqn + (ok ? yy : 0.0));
    A.scal[2] = step;
    A.scal[3] = ok ? 1.0 : 0.0;
  }
}

}  // namespace cba

// ---- host side: the checks of a call, its plan and the driver -------------------------------------------------------------------------
#include <algorithm>
#include <string>
#include <vector>

namespace cba {

struct SyncPlan {
  int32_t n_cols = 0, ref_col = -1, ref_cam = -1;
  int64_t ld = 0, n_waves = 0, n_chunks = 0;
  int32_t n_groups = 0;
  std::vector<int32_t> cam_col, col_cam;
  std::vector<int64_t> cam_row_start;  // [n_cams + 1]
  std::vector<double> tau;             // [n_frames] the host's k_traj_frame_time: the same additions in the same order
  double interval = 0.0, max_offset = 0.0, tol = 0.0;
};

// bytes of the device buffers of a call: the grids and the rows of the reconstruction, the per-slot state (X, dX, V, L, valid,
// moving), Q and the partial sums
inline double sync_device_bytes(const cba_traj_desc* d, const SyncPlan& p) {
  const double slots = (double)d->n_frames * (double)d->n_traj, cams = (double)d->n_cams, ld = (double)p.ld;
  return cams * slots * 24.0 + slots * 74.0 + ld * 48.0 + ld * 24.0 * (double)p.n_cols + (double)d->n_frames * 8.0 + (double)d->n_rows * 53.0 +
         cams * 300.0 + (double)p.n_waves * (8.0 + 16.0 * (double)p.n_cols) + (double)p.n_groups * 8.0 * SYNC_LD * SYNC_LD;
}

// 0, or -1 / -4 with `msg` set; fills `plan`.  *launch false: the call returns without a launch.  memory <= 0: not checked.
inline int sync_validate(const cba_traj_desc* d, const cba_time_offset_options* o, double memory, SyncPlan& plan, std::string& msg, bool* launch) {
  const std::string what = "cba_estimate_time_offsets: ";
  *launch = false;
  plan = SyncPlan();
  int rc = traj_validate(d, 0.0, msg);
  if (rc) return rc;
  if (!o) { msg = what + "options: null argument"; return -1; }
  if (d->xy_gap != 0) { msg = what + "xy_gap must be 0, got " + std::to_string(d->xy_gap) + " (this call fills no holes)"; return -1; }
  if (d->xyz_gap != 0) { msg = what + "xyz_gap must be 0, got " + std::to_string(d->xyz_gap) + " (this call fills no holes)"; return -1; }
  if (d->filter_b) { msg = what + "a filter in the descriptor (this call does not smooth)"; return -1; }
  if (!std::isfinite(o->huber_px) || o->huber_px < 0.0) { msg = what + "huber_px must be finite and not negative, got " + std::to_string(o->huber_px); return -1; }
  if (!std::isfinite(o->max_offset) || o->max_offset < 0.0) { msg = what + "max_offset must be finite and not negative, got " + std::to_string(o->max_offset); return -1; }
  if (!std::isfinite(o->tol) || o->tol < 0.0) { msg = what + "tol must be finite and not negative, got " + std::to_string(o->tol); return -1; }
  if (o->max_neighbour_gap < 1) { msg = what + "max_neighbour_gap must be at least 1, got " + std::to_string(o->max_neighbour_gap); return -1; }
  if (o->min_rows < 1) { msg = what + "min_rows must be at least 1, got " + std::to_string(o->min_rows); return -1; }
  if (o->max_rounds < 1) { msg = what + "max_rounds must be at least 1, got " + std::to_string(o->max_rounds); return -1; }
  if (o->reference_cam < -1 || o->reference_cam >= d->n_cams) {
    if (d->n_rows == 0 && o->reference_cam >= 0) { msg = what + "reference camera " + std::to_string(o->reference_cam) + " has no rows"; return -1; }
    msg = what + "reference camera " + std::to_string(o->reference_cam) + " out of range [0, " + std::to_string(d->n_cams) + ")";
    return -1;
  }
  if (d->n_rows == 0) {
    if (o->reference_cam >= 0) { msg = what + "reference camera " + std::to_string(o->reference_cam) + " has no rows"; return -1; }
    return 0;
  }
  const int32_t n_cams = d->n_cams;
  const int64_t n_frames = d->n_frames, n_traj = d->n_traj, n_slots = n_frames * n_traj;
  plan.cam_col.assign((size_t)n_cams, -1);
  for (int32_t c = 0; c < n_cams; ++c)
    if (d->cam_posed[c]) { plan.cam_col[(size_t)c] = plan.n_cols++; plan.col_cam.push_back(c); }
  plan.cam_row_start.assign((size_t)n_cams + 1, 0);
  plan.tau.assign((size_t)n_frames, 0.0);
  std::vector<int64_t> count((size_t)n_frames, 0);
  for (int64_t i = 0; i < d->n_rows; ++i) {  // (rows ascend in (camera, trajectory): per frame the order of k_traj_frame_time)
    if (!std::isfinite(d->row_time[i])) { msg = what + "row " + std::to_string(i) + ": row_time is not finite"; return -1; }
    const int64_t f = d->row_slot[i] / n_traj;
    plan.tau[(size_t)f] += d->row_time[i];
    ++count[(size_t)f];
    ++plan.cam_row_start[(size_t)d->row_cam[i] + 1];
  }
  for (int32_t c = 0; c < n_cams; ++c) plan.cam_row_start[(size_t)c + 1] += plan.cam_row_start[(size_t)c];
  std::vector<double> steps;
  int64_t last = -1;
  for (int64_t f = 0; f < n_frames; ++f) {
    if (!count[(size_t)f]) { plan.tau[(size_t)f] = traj_nan(); continue; }
    plan.tau[(size_t)f] /= (double)count[(size_t)f];
    if (last >= 0) {
      if (!(plan.tau[(size_t)f] > plan.tau[(size_t)last])) {
        msg = what + "frame " + std::to_string(f) + ": its mean time " + std::to_string(plan.tau[(size_t)f]) + " does not lie after that of frame " +
              std::to_string(last) + ", " + std::to_string(plan.tau[(size_t)last]);
        return -1;
      }
      steps.push_back((plan.tau[(size_t)f] - plan.tau[(size_t)last]) / (double)(f - last));
    }
    last = f;
  }
  const auto has_rows = [&](int32_t c) { return plan.cam_row_start[(size_t)c + 1] > plan.cam_row_start[(size_t)c]; };
  if (o->reference_cam >= 0) {
    if (!d->cam_posed[o->reference_cam]) { msg = what + "reference camera " + std::to_string(o->reference_cam) + " is unposed"; return -1; }
    if (!has_rows(o->reference_cam)) { msg = what + "reference camera " + std::to_string(o->reference_cam) + " has no rows"; return -1; }
    plan.ref_cam = o->reference_cam;
  } else {
    for (int32_t c = 0; c < n_cams && plan.ref_cam < 0; ++c)
      if (d->cam_posed[c] && has_rows(c)) plan.ref_cam = c;
    if (plan.ref_cam < 0) return 0;  // no posed camera with rows: nothing to estimate
  }
  plan.ref_col = plan.cam_col[(size_t)plan.ref_cam];
  if (plan.n_cols > CBA_OFFSET_MAX_CAMS) {
    msg = what + std::to_string(plan.n_cols) + " posed cameras: at most " + std::to_string(CBA_OFFSET_MAX_CAMS) + " are supported";
    return -4;
  }
  if (steps.empty()) {
    if (!(o->max_offset > 0.0) || !(o->tol > 0.0)) {
      msg = what + "one frame with rows: no frame interval to derive max_offset and tol from";
      return -1;
    }
  } else {
    std::nth_element(steps.begin(), steps.begin() + (steps.size() - 1) / 2, steps.end());  // the lower median
    plan.interval = steps[(steps.size() - 1) / 2];
  }
  plan.max_offset = o->max_offset > 0.0 ? o->max_offset : plan.interval;
  plan.tol = o->tol > 0.0 ? o->tol : SYNC_TOL_FRACTION * plan.interval;
  plan.n_chunks = (n_slots + SYNC_GRAM_CHUNK - 1) / SYNC_GRAM_CHUNK;
  plan.ld = plan.n_chunks * SYNC_GRAM_CHUNK;
  plan.n_waves = plan.ld / 64;
  plan.n_groups = (int32_t)std::min<int64_t>(plan.n_chunks, SYNC_GRAM_GROUPS);
  const double bytes = sync_device_bytes(d, plan);
  if (memory > 0.0 && bytes > memory) {
    msg = what + "the grid of " + std::to_string(n_cams) + " cameras x " + std::to_string(n_frames) + " frames x " + std::to_string(n_traj) +
          " trajectories needs " + std::to_string((long long)bytes) + " bytes of device memory (" + std::to_string(24 * plan.n_cols) +
          " per slot for the " + std::to_string(plan.n_cols) + " columns of Q), " + std::to_string((long long)memory) + " are available";
    return -4;
  }
  *launch = true;
  return 0;
}

// what a call without a launch returns
inline void sync_nothing(const cba_traj_desc* d, const SyncPlan& plan, cba_time_offset_out* o) {
  const double nan = traj_nan();
  const int64_t n_slots = d->n_frames * d->n_traj;
  for (int32_t c = 0; c < d->n_cams; ++c) {
    if (o->offsets) o->offsets[c] = nan;
    if (o->sigma) o->sigma[c] = nan;
    if (o->status) o->status[c] = CBA_OFFSET_NONE;
    if (o->rms_before) o->rms_before[c] = nan;
    if (o->rms_after) o->rms_after[c] = nan;
    if (o->rows) o->rows[c] = 0;
  }
  if (o->sigma0_px) *o->sigma0_px = nan;
  if (o->rounds) *o->rounds = 0;
  if (o->converged) *o->converged = 0;
  for (int64_t s = 0; s < n_slots; ++s) {
    if (o->xyz) o->xyz[3 * s] = o->xyz[3 * s + 1] = o->xyz[3 * s + 2] = nan;
    if (o->valid) o->valid[s] = 0;
    if (o->velocity) o->velocity[3 * s] = o->velocity[3 * s + 1] = o->velocity[3 * s + 2] = 0.0;
  }
  for (int64_t f = 0; f < d->n_frames; ++f)
    if (o->frame_time) o->frame_time[f] = plan.tau.empty() ? nan : plan.tau[(size_t)f];
  for (int64_t i = 0; i < d->n_rows; ++i) {
    if (o->row_xy) { o->row_xy[2 * i] = d->row_xy[2 * i]; o->row_xy[2 * i + 1] = d->row_xy[2 * i + 1]; }
    if (o->row_used) o->row_used[i] = 0;
  }
}

struct SyncScalars { double F, pred, step, ok; };

// The rounds and the safeguarded Gauss-Newton of a call on a backend `be` (the device: time_offset_lib.hip; the g++ build:
// tests/native/time_offset_harness.cpp), which holds the state and has
//     bool velocity(bool first)   V from the current points (first: also the moving flags the fixed set is decided with)
//     bool rows(bool final)       the pass over the rows: before (sums, counts, the fixed set) or after (sums, pixels)
//     bool eval(double alpha, SyncScalars&)   build, Gram matrix, reduce and solve at point + alpha step; reads the four scalars
//     bool step(double alpha)     the trial at alpha becomes the point (alpha == 0: the point stays), the solved step the step
//     bool offsets(double* by_col)            reads the offsets of the point
//     bool set_offsets(const double* by_col)  writes them
// each false on a failure of the device, which ends the call.  The state starts at the DLT points with V = 0, offsets 0 and every
// column fixed.  Leaves rounds, converged and the F of the end; eval(0) is the last evaluation, so the backend's S^-1 is that of
// the end.  sync_inner is one safeguarded Gauss-Newton run with V frozen; n_rows scales the floor of the predicted decrease.
template <class Backend>
inline bool sync_inner(Backend& be, double pred_floor) {
  SyncScalars sc;
  double alpha = 0.0, F = 0.0, pending = 0.0;
  int halvings = 0;
  for (int it = 0; it < CBA_OFFSET_MAX_INNER; ++it) {
    if (!be.eval(alpha, sc)) return false;
    const bool keep = alpha == 0.0 || (sc.F - sc.F == 0.0 && sc.F <= F + SYNC_RESOLVE * (1.0 + F));
    if (!keep) {
      alpha *= 0.5;
      if (++halvings > SYNC_MAX_HALVINGS) break;  // (the point stays where it is)
      continue;
    }
    const bool last = alpha != 0.0 && pending <= pred_floor;
    if (!be.step(alpha)) return false;
    F = sc.F;
    pending = sc.pred;
    alpha = 1.0;
    halvings = 0;
    if (last || sc.ok == 0.0) break;
  }
  return true;
}

template <class Backend>
inline bool sync_drive(Backend& be, const SyncPlan& plan, int64_t n_rows, int max_rounds, int32_t* rounds, uint8_t* converged, double* F_end) {
  *rounds = 0;
  *converged = 0;
  const double pred_floor = SYNC_PRED_ROW * (double)n_rows;
  // the synchronous start: V = 0 and every offset fixed, the points alone from the DLT to the minimum of the reprojection error
  if (!sync_inner(be, pred_floor)) return false;
  if (!be.velocity(true) || !be.rows(false)) return false;
  std::vector<double> prev((size_t)plan.n_cols, 0.0), now((size_t)plan.n_cols, 0.0);
  SyncScalars sc;
  for (int round = 0; round < max_rounds; ++round) {
    if (round > 0 && !be.velocity(false)) return false;
    if (!sync_inner(be, pred_floor)) return false;
    if (!be.offsets(now.data())) return false;
    double change = 0.0;
    for (int32_t c = 0; c < plan.n_cols; ++c) change = std::max(change, std::fabs(now[(size_t)c] - prev[(size_t)c]));
    prev = now;
    *rounds = round + 1;
    if (change < plan.tol) { *converged = 1; break; }
  }
  // an offset below tol is not told from zero by the rounds' own criterion: it is zero, so that the rows of cameras that are
  // synchronous come back as they went in
  bool snapped = false;
  for (int32_t c = 0; c < plan.n_cols; ++c)
    if (now[(size_t)c] != 0.0 && std::fabs(now[(size_t)c]) < plan.tol) { now[(size_t)c] = 0.0; snapped = true; }
  if (snapped && !be.set_offsets(now.data())) return false;
  if (!be.eval(0.0, sc)) return false;
  *F_end = sc.F;
  return be.rows(true);
}

// The per-camera results from what the backend read back at the end, by column: offsets, (S^-1)_cc, the fixed set, and by camera the
// sums of squares and the counts of the two row passes.  n_points: slots with a point.
inline void sync_report(const cba_traj_desc* d, const SyncPlan& plan, const double* delta, const double* sinv, const uint8_t* free_col,
                        const double* e2_before, const double* e2_after, const int64_t* used, int64_t n_points, double F_end, cba_time_offset_out* o) {
  const double nan = traj_nan();
  int64_t rows = 0, n_free = 0;
  for (int32_t c = 0; c < d->n_cams; ++c) rows += used[c];
  for (int32_t k = 0; k < plan.n_cols; ++k) n_free += free_col[k] ? 1 : 0;
  const int64_t dof = 2 * rows - 3 * n_points - n_free;
  const double sigma0 = dof > 0 ? std::sqrt(2.0 * F_end / (double)dof) : nan;
  if (o->sigma0_px) *o->sigma0_px = sigma0;
  for (int32_t c = 0; c < d->n_cams; ++c) {
    const int32_t k = plan.cam_col[(size_t)c];
    uint8_t st = CBA_OFFSET_NONE;
    double off = nan, sg = nan;
    if (k >= 0 && used[c] > 0) {
      if (k == plan.ref_col) { st = CBA_OFFSET_REFERENCE; off = 0.0; sg = 0.0; }
      else if (!free_col[k]) st = CBA_OFFSET_UNDETERMINED;
      else {
        off = delta[k];
        sg = sigma0 * std::sqrt(sinv[k]);
        st = std::fabs(off) >= plan.max_offset ? CBA_OFFSET_AT_LIMIT : CBA_OFFSET_ESTIMATED;
      }
    }
    if (o->offsets) o->offsets[c] = off;
    if (o->sigma) o->sigma[c] = sg;
    if (o->status) o->status[c] = st;
    if (o->rows) o->rows[c] = k >= 0 ? used[c] : 0;
    if (o->rms_before) o->rms_before[c] = k >= 0 && used[c] > 0 ? std::sqrt(e2_before[c] / (double)used[c]) : nan;
    if (o->rms_after) o->rms_after[c] = k >= 0 && used[c] > 0 ? std::sqrt(e2_after[c] / (double)used[c]) : nan;
  }
}

}  // namespace cba
