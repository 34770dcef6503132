// Arithmetic of cba_adjust_skeleton (include/caliscope/trajectory_skeleton.h, where the mathematics is stated).  Compiled by hipcc into
// skeleton_lib.hip and by g++ into tests/native/trajectory_skeleton_harness.cpp.
//
// skel_adjust_group is what one workgroup of k_skel_adjust does for one (frame, component): thread t of NT runs it, SKEL_BARRIER() between
// the phases.  Every loop over elements is `for (i = t; i < n; i += NT)` and every sum over points is partial per point and added by thread
// 0 in ascending order, so the host's serial form is the same function with t = 0, NT = 1 and no barrier: the same operations in the same
// order.  The lengths (k_skel_length) share skel_pair and skel_length_lane; the select has a host-only serial form, skel_lower_median.
// Arrays indexed at run time live in LDS (SkelLds), never in registers: no scratch.
#pragma once
#include <cmath>
#include <cstdint>

#include "ba_math.h"
#include "covariance_constraint_math.h"
#include "trajectory_smooth_math.h"
#include "../../include/caliscope/trajectory_skeleton.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define SKEL_BARRIER() __syncthreads()
#else
#define SKEL_BARRIER() ((void)0)
#endif

namespace cba {

constexpr int SKEL_MAX_POINTS = CBA_SKELETON_MAX_POINTS;
constexpr int SKEL_LEN_THREADS = 256;  // lanes of the fixed-order sums of k_skel_length (and its workgroup)
constexpr int SKEL_PASS_BLOCK = 256;
constexpr uint8_t SKEL_SLOT_NONE = 0, SKEL_SLOT_ADJUSTED = 1, SKEL_SLOT_INACTIVE = 2, SKEL_SLOT_FAILED = 3;
constexpr uint8_t SKEL_COMP_NONE = 0, SKEL_COMP_CONVERGED = 1, SKEL_COMP_MAX_ITER = 2, SKEL_COMP_FAILED = 3;
constexpr double SKEL_LAMBDA_FIRST = 1e-4, SKEL_LAMBDA_UP = 10.0, SKEL_LAMBDA_DOWN = 0.1;
constexpr double SKEL_MAD_SCALE = 1.4826;
constexpr double SKEL_RESOLVE = 1e-10;  // the share of 1 + F below which a change of F is not told from its rounding

CBA_HD bool skel_finite(double v) { return v - v == 0.0; }

// the tables of the components, built by the host (skel_plan) and read by k_skel_adjust
struct SkelTables {
  const int32_t* comp_pt;    // [n_comp + 1] into pts
  const int32_t* pts;        // trajectories of a component, ascending
  const int32_t* comp_seg;   // [n_comp + 1] into segs
  const int32_t* segs;       // segments of a component, ascending
  const int32_t* seg_loc;    // [n_seg][2] places of a and b in their component
  const int32_t* inc_start;  // [len(pts) + 1] into inc: the segments incident to a point
  const int32_t* inc;        // ascending segment index
};

struct SkelOut {
  double *pos, *pos_cov;
  uint8_t* status;
  double *len_before, *w_before, *len_after, *chi2;
  int32_t *rows, *iterations;
  uint8_t* comp_status;
};

// doubles of LDS a component of m points takes; the int tables follow
CBA_HD int skel_lds_doubles(int m) {
  const int n = 3 * m;
  return n * (n + 1) / 2 + 7 * n + 6 * m + 8;
}
CBA_HD int skel_lds_bytes(int m) { return skel_lds_doubles(m) * 8 + (3 * m + 2) * 4; }

struct SkelLds {
  double *Vt, *g, *dl, *X, *Xt, *Z, *diag0, *col, *Ri, *scal;  // scal: F, F trial, decrement, F at Z
  int32_t *meas, *loc, *rowsa;
  CBA_HD explicit SkelLds(double* base, int m) {
    const int n = 3 * m;
    Vt = base; g = Vt + n * (n + 1) / 2; dl = g + n; X = dl + n; Xt = X + n; Z = Xt + n; diag0 = Z + n; col = diag0 + n; Ri = col + n;
    scal = Ri + 6 * m;
    meas = (int32_t*)(scal + 8); loc = meas + m; rowsa = loc + m;
  }
};

// |a - b| and u = (a - b) / |a - b| (0 for coincident ends)
// (no contraction to fused multiply-adds: the median of the lengths is the same bits on the device, on the host and in numpy)
CBA_HD double skel_unit(const double* a, const double* b, double* u) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
  const double d = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
  const double inv = d > 0.0 ? 1.0 / d : 0.0;
  u[0] = d0 * inv; u[1] = d1 * inv; u[2] = d2 * inv;
  return d;
}

// u^T (Ra + Rb) u of symmetric 3 x 3 rows xx xy xz yy yz zz
CBA_HD double skel_quad2(const double* Ra, const double* Rb, const double* u) {
  const double xx = Ra[0] + Rb[0], xy = Ra[1] + Rb[1], xz = Ra[2] + Rb[2], yy = Ra[3] + Rb[3], yz = Ra[4] + Rb[4], zz = Ra[5] + Rb[5];
  return u[0] * (xx * u[0] + 2.0 * (xy * u[1] + xz * u[2])) + u[1] * (yy * u[1] + 2.0 * yz * u[2]) + u[2] * zz * u[2];
}

// d_f and its variance for the slots sa, sb of one frame; false when an end is not measured
CBA_HD bool skel_pair(int64_t sa, int64_t sb, const double* xyz, const double* meas_cov, const uint8_t* measured, double* d, double* var) {
  if (measured[sa] != 1 || measured[sb] != 1) return false;
  double u[3];
  *d = skel_unit(xyz + 3 * sa, xyz + 3 * sb, u);
  const double* Ra = meas_cov + 6 * sa;
  const double* Rb = meas_cov + 6 * sb;
  *var = *d > 0.0 ? skel_quad2(Ra, Rb, u) : (Ra[0] + Rb[0] + Ra[3] + Rb[3] + Ra[5] + Rb[5]) / 3.0;
  return true;
}

// whether a frame's d takes part in the mean
CBA_HD bool skel_keep(double d, double med, double mad, double trim) {
  return mad == 0.0 ? d == med : fabs(d - med) <= trim * SKEL_MAD_SCALE * mad;
}

// lane t's share of sum(d / v), sum(1 / v) of segment (a, b): the frames t, t + SKEL_LEN_THREADS, .. in ascending order
CBA_HD void skel_length_lane(int t, int64_t n_frames, int64_t n_traj, int32_t a, int32_t b, const double* xyz, const double* meas_cov,
                             const uint8_t* measured, double med, double mad, double trim, double* num, double* den) {
  double sn = 0.0, sd = 0.0;
  for (int64_t f = t; f < n_frames; f += SKEL_LEN_THREADS) {
    double d, v;
    if (!skel_pair(f * n_traj + a, f * n_traj + b, xyz, meas_cov, measured, &d, &v) || !skel_keep(d, med, mad, trim)) continue;
    const double w = 1.0 / v;
    sn += d * w;
    sd += w;
  }
  *num = sn;
  *den = sd;
}

// bit pattern of a non-negative double: ascending as the doubles
CBA_HD uint64_t skel_bits(double v) {
  uint64_t b;
  __builtin_memcpy(&b, &v, sizeof b);
  return b;
}
CBA_HD double skel_from_bits(uint64_t b) {
  double v;
  __builtin_memcpy(&v, &b, sizeof v);
  return v;
}

// whether segment s = (place a, place b) of the component is active: both ends measured in the frame, a finite length
CBA_HD bool skel_active(const int32_t* meas, int a, int b, double length) { return meas[a] && meas[b] && skel_finite(length); }

// F's share of unknown point i (place in the component), at the iterate P ([n], by unknown): its own term and the terms of the active
// segments whose first end it is
CBA_HD double skel_F_point(int i, int64_t p0, const SkelTables& T, const SkelLds& S, const double* P, const double* length, const double* sigma) {
  const int q = S.loc[i];
  const double e0 = P[3 * q] - S.Z[3 * q], e1 = P[3 * q + 1] - S.Z[3 * q + 1], e2 = P[3 * q + 2] - S.Z[3 * q + 2];
  const double* R = S.Ri + 6 * q;
  double val = e0 * (R[0] * e0 + 2.0 * (R[1] * e1 + R[2] * e2)) + e1 * (R[3] * e1 + 2.0 * R[4] * e2) + e2 * R[5] * e2;
  for (int32_t c = T.inc_start[p0 + i]; c < T.inc_start[p0 + i + 1]; ++c) {
    const int32_t s = T.inc[c];
    const int a = T.seg_loc[2 * s], b = T.seg_loc[2 * s + 1];
    if (a != i || !skel_active(S.meas, a, b, length[s])) continue;
    double u[3];
    const double r = (skel_unit(P + 3 * S.loc[a], P + 3 * S.loc[b], u) - length[s]) / sigma[s];
    val += r * r;
  }
  return val;
}

// F at P into S.scal[slot]: partial per point into S.col, added by thread 0 in ascending order.  Ends with a barrier.
CBA_HD void skel_F(int t, int NT, int m, int mf, int64_t p0, const SkelTables& T, const SkelLds& S, const double* P, const double* length,
                   const double* sigma, int slot) {
  for (int i = t; i < m; i += NT)
    if (S.loc[i] >= 0) S.col[S.loc[i]] = skel_F_point(i, p0, T, S, P, length, sigma);
  SKEL_BARRIER();
  if (t == 0) {
    double F = 0.0;
    for (int q = 0; q < mf; ++q) F += S.col[q];
    S.scal[slot] = F;
  }
  SKEL_BARRIER();
}

// N (packed lower triangle, lambda diag(N) added) and g at S.X; S.diag0 the diagonal before the damping.  Ends with a barrier.
CBA_HD void skel_assemble(int t, int NT, int m, int mf, int64_t p0, int32_t s0, int n_cs, const SkelTables& T, const SkelLds& S, const double* length,
                          const double* sigma, double lambda) {
  const int n = 3 * mf, ntri = n * (n + 1) / 2;
  for (int e = t; e < ntri; e += NT) S.Vt[e] = 0.0;
  SKEL_BARRIER();
  for (int i = t; i < m; i += NT) {
    const int q = S.loc[i];
    if (q < 0) continue;
    const double* R = S.Ri + 6 * q;
    const double e0 = S.X[3 * q] - S.Z[3 * q], e1 = S.X[3 * q + 1] - S.Z[3 * q + 1], e2 = S.X[3 * q + 2] - S.Z[3 * q + 2];
    double b0 = R[0], b1 = R[1], b2 = R[2], b3 = R[3], b4 = R[4], b5 = R[5];
    double g0 = R[0] * e0 + R[1] * e1 + R[2] * e2, g1 = R[1] * e0 + R[3] * e1 + R[4] * e2, g2 = R[2] * e0 + R[4] * e1 + R[5] * e2;
    for (int32_t c = T.inc_start[p0 + i]; c < T.inc_start[p0 + i + 1]; ++c) {
      const int32_t s = T.inc[c];
      const int a = T.seg_loc[2 * s], b = T.seg_loc[2 * s + 1];
      if (!skel_active(S.meas, a, b, length[s])) continue;
      double u[3];
      const double d = skel_unit(S.X + 3 * S.loc[a], S.X + 3 * S.loc[b], u);
      const double w = 1.0 / (sigma[s] * sigma[s]);
      const double wr = (a == i ? w : -w) * (d - length[s]);
      b0 += w * u[0] * u[0]; b1 += w * u[0] * u[1]; b2 += w * u[0] * u[2];
      b3 += w * u[1] * u[1]; b4 += w * u[1] * u[2]; b5 += w * u[2] * u[2];
      g0 += wr * u[0]; g1 += wr * u[1]; g2 += wr * u[2];
    }
    const int r = 3 * q;
    S.Vt[cov_tri(r, r)] = b0;
    S.Vt[cov_tri(r + 1, r)] = b1; S.Vt[cov_tri(r + 1, r + 1)] = b3;
    S.Vt[cov_tri(r + 2, r)] = b2; S.Vt[cov_tri(r + 2, r + 1)] = b4; S.Vt[cov_tri(r + 2, r + 2)] = b5;
    S.g[r] = g0; S.g[r + 1] = g1; S.g[r + 2] = g2;
  }
  for (int e = t; e < n_cs; e += NT) {
    const int32_t s = T.segs[s0 + e];
    const int a = T.seg_loc[2 * s], b = T.seg_loc[2 * s + 1];
    if (!skel_active(S.meas, a, b, length[s])) continue;
    double u[3];
    skel_unit(S.X + 3 * S.loc[a], S.X + 3 * S.loc[b], u);
    const double w = -1.0 / (sigma[s] * sigma[s]);
    const int hi = 3 * (S.loc[a] > S.loc[b] ? S.loc[a] : S.loc[b]), lo = 3 * (S.loc[a] > S.loc[b] ? S.loc[b] : S.loc[a]);
    S.Vt[cov_tri(hi, lo)] = w * u[0] * u[0]; S.Vt[cov_tri(hi, lo + 1)] = w * u[0] * u[1]; S.Vt[cov_tri(hi, lo + 2)] = w * u[0] * u[2];
    S.Vt[cov_tri(hi + 1, lo)] = w * u[1] * u[0]; S.Vt[cov_tri(hi + 1, lo + 1)] = w * u[1] * u[1]; S.Vt[cov_tri(hi + 1, lo + 2)] = w * u[1] * u[2];
    S.Vt[cov_tri(hi + 2, lo)] = w * u[2] * u[0]; S.Vt[cov_tri(hi + 2, lo + 1)] = w * u[2] * u[1]; S.Vt[cov_tri(hi + 2, lo + 2)] = w * u[2] * u[2];
  }
  SKEL_BARRIER();
  for (int i = t; i < n; i += NT) {
    const double d = S.Vt[cov_tri(i, i)];
    S.diag0[i] = d;
    S.Vt[cov_tri(i, i)] = d + lambda * d;
  }
  SKEL_BARRIER();
}

// Vt = L in place (right-looking, three barriers a column).  false, for every thread alike, when a pivot is not safely positive.
CBA_HD bool skel_factor(int t, int NT, int n, const SkelLds& S) {
  const int CW = NT >= 16 ? 16 : 1, RW = NT / CW;
  for (int j = 0; j < n; ++j) {
    const double d = S.Vt[cov_tri(j, j)];
    if (!cov_con_pivot_ok(d, S.diag0[j])) return false;
    const double ljj = sqrt(d);
    SKEL_BARRIER();  // (every thread has read the pivot)
    for (int i = j + t; i < n; i += NT) S.Vt[cov_tri(i, j)] = i == j ? ljj : S.Vt[cov_tri(i, j)] / ljj;
    SKEL_BARRIER();
    for (int i = j + 1 + t / CW; i < n; i += RW) {
      const double lij = S.Vt[cov_tri(i, j)];
      for (int c = j + 1 + t % CW; c <= i; c += CW) S.Vt[cov_tri(i, c)] -= lij * S.Vt[cov_tri(c, j)];
    }
    SKEL_BARRIER();
  }
  return true;
}

// dl = -(L L^T)^-1 g: column-oriented forward and backward substitution, two barriers a column each.  Ends with a barrier.
CBA_HD void skel_solve(int t, int NT, int n, const SkelLds& S) {
  for (int i = t; i < n; i += NT) S.dl[i] = -S.g[i];
  SKEL_BARRIER();
  for (int j = 0; j < n; ++j) {
    const double y = S.dl[j] / S.Vt[cov_tri(j, j)];
    SKEL_BARRIER();  // (every thread has read dl[j])
    if (t == 0) S.dl[j] = y;
    for (int i = j + 1 + t; i < n; i += NT) S.dl[i] -= S.Vt[cov_tri(i, j)] * y;
    SKEL_BARRIER();
  }
  for (int j = n - 1; j >= 0; --j) {
    const double x = S.dl[j] / S.Vt[cov_tri(j, j)];
    SKEL_BARRIER();
    if (t == 0) S.dl[j] = x;
    for (int i = t; i < j; i += NT) S.dl[i] -= S.Vt[cov_tri(j, i)] * x;
    SKEL_BARRIER();
  }
}

// One (frame f, component k).  lds: skel_lds_bytes(m) bytes, 8-aligned.
CBA_HD void skel_adjust_group(int t, int NT, int64_t f, int32_t k, int32_t n_comp, int64_t n_traj, int64_t n_seg, const double* xyz,
                              const double* meas_cov, const uint8_t* measured, const double* length, const double* sigma, int max_iter, double tol,
                              const SkelTables& T, const SkelOut& O, double* lds) {
  const int64_t p0 = T.comp_pt[k];
  const int m = (int)(T.comp_pt[k + 1] - p0);
  const int32_t s0 = T.comp_seg[k];
  const int n_cs = T.comp_seg[k + 1] - s0;
  const int32_t* pts = T.pts + p0;
  const SkelLds S(lds, m);
  const int64_t slot0 = f * n_traj, cell = f * n_comp + k;
  // the unknowns of the frame
  for (int i = t; i < m; i += NT) S.meas[i] = measured[slot0 + pts[i]] == 1 ? 1 : 0;
  SKEL_BARRIER();
  for (int i = t; i < m; i += NT) {
    int any = 0, first = 0;
    for (int32_t c = T.inc_start[p0 + i]; c < T.inc_start[p0 + i + 1]; ++c) {
      const int32_t s = T.inc[c];
      const int a = T.seg_loc[2 * s], b = T.seg_loc[2 * s + 1];
      if (!skel_active(S.meas, a, b, length[s])) continue;
      any = 1;
      first += a == i ? 1 : 0;
    }
    S.loc[i] = any ? 0 : -1;
    S.rowsa[i] = first;
  }
  SKEL_BARRIER();
  if (t == 0) {
    int c = 0, rows = 0;
    for (int i = 0; i < m; ++i) {
      rows += S.rowsa[i];
      if (S.loc[i] == 0) S.loc[i] = c++;
    }
    S.rowsa[m] = c;
    S.rowsa[m + 1] = rows;
  }
  SKEL_BARRIER();
  const int mf = S.rowsa[m], rows = S.rowsa[m + 1], n = 3 * mf;
  if (mf == 0) {  // (uniform)
    if (t == 0) { O.chi2[cell] = 0.0; O.rows[cell] = 0; O.iterations[cell] = 0; O.comp_status[cell] = SKEL_COMP_NONE; }
    return;
  }
  for (int i = t; i < m; i += NT) {
    const int q = S.loc[i];
    if (q < 0) continue;
    const int64_t s = slot0 + pts[i];
    for (int c = 0; c < 3; ++c) S.Z[3 * q + c] = S.X[3 * q + c] = xyz[3 * s + c];
    if (!smooth_inv3(meas_cov + 6 * s, S.Ri + 6 * q))  // (the checks refuse such a slot)
      for (int c = 0; c < 6; ++c) S.Ri[6 * q + c] = traj_nan();
  }
  SKEL_BARRIER();
  for (int e = t; e < n_cs; e += NT) {
    const int32_t s = T.segs[s0 + e];
    const int a = T.seg_loc[2 * s], b = T.seg_loc[2 * s + 1];
    if (!skel_active(S.meas, a, b, length[s])) continue;
    double u[3];
    const double d = skel_unit(S.Z + 3 * S.loc[a], S.Z + 3 * S.loc[b], u);
    const double var = skel_quad2(meas_cov + 6 * (slot0 + pts[a]), meas_cov + 6 * (slot0 + pts[b]), u);
    O.len_before[f * n_seg + s] = d;
    O.w_before[f * n_seg + s] = (d - length[s]) / sqrt(sigma[s] * sigma[s] + var);
  }
  skel_F(t, NT, m, mf, p0, T, S, S.X, length, sigma, 0);
  if (t == 0) S.scal[3] = S.scal[0];
  double lambda = 0.0;
  int iters = 0, status = SKEL_COMP_MAX_ITER;
  while (iters < max_iter) {
    skel_assemble(t, NT, m, mf, p0, s0, n_cs, T, S, length, sigma, lambda);
    ++iters;
    bool lower = false;
    double dec = 0.0;
    if (skel_factor(t, NT, n, S)) {
      skel_solve(t, NT, n, S);
      for (int q = t; q < mf; q += NT) {
        S.col[q] = -(S.g[3 * q] * S.dl[3 * q] + S.g[3 * q + 1] * S.dl[3 * q + 1] + S.g[3 * q + 2] * S.dl[3 * q + 2]);
        for (int c = 0; c < 3; ++c) S.Xt[3 * q + c] = S.X[3 * q + c] + S.dl[3 * q + c];
      }
      SKEL_BARRIER();
      if (t == 0) {
        double s = 0.0;
        for (int q = 0; q < mf; ++q) s += S.col[q];
        S.scal[2] = s;
      }
      SKEL_BARRIER();
      skel_F(t, NT, m, mf, p0, T, S, S.Xt, length, sigma, 1);
      dec = S.scal[2];
      const double res = SKEL_RESOLVE * (1.0 + S.scal[0]);
      lower = S.scal[1] <= S.scal[0] || (dec <= res && S.scal[1] <= S.scal[0] + res);
    }
    SKEL_BARRIER();  // (every thread has read the scalars)
    if (lower) {
      for (int i = t; i < n; i += NT) S.X[i] = S.Xt[i];
      if (t == 0) S.scal[0] = S.scal[1];
      const bool undamped = lambda == 0.0;
      lambda = lambda * SKEL_LAMBDA_DOWN < SKEL_LAMBDA_FIRST ? 0.0 : lambda * SKEL_LAMBDA_DOWN;
      SKEL_BARRIER();
      if (undamped && dec <= tol * tol) { status = SKEL_COMP_CONVERGED; break; }
    } else {
      lambda = lambda == 0.0 ? SKEL_LAMBDA_FIRST : lambda * SKEL_LAMBDA_UP;
    }
  }
  // the covariance: one undamped factorisation at the result, inverted in place
  skel_assemble(t, NT, m, mf, p0, s0, n_cs, T, S, length, sigma, 0.0);
  const bool ok = skel_factor(t, NT, n, S);
  SKEL_BARRIER();
  if (ok) {
    for (int j = n - 1; j >= 0; --j) {
      const double xjj = 1.0 / S.Vt[cov_tri(j, j)];
      for (int i = j + 1 + t; i < n; i += NT) S.col[i] = S.Vt[cov_tri(i, j)];
      SKEL_BARRIER();
      for (int i = j + t; i < n; i += NT) S.Vt[cov_tri(i, j)] = i == j ? xjj : cov_tri_inverse_entry(S.Vt, i, j, S.col, xjj);
      SKEL_BARRIER();
    }
  }
  for (int it = t; it < m * 6; it += NT) {
    const int i = it / 6, e = it % 6, q = S.loc[i];
    if (q < 0) continue;
    if (ok) O.pos_cov[(slot0 + pts[i]) * 6 + e] = cov_tri_gram(S.Vt, n, 3 * q + cov_sym3_row(e), 3 * q + cov_sym3_col(e));
    if (ok && e < 3) O.pos[(slot0 + pts[i]) * 3 + e] = S.X[3 * q + e];
    if (e == 0) O.status[slot0 + pts[i]] = ok ? SKEL_SLOT_ADJUSTED : SKEL_SLOT_FAILED;
  }
  for (int e = t; e < n_cs; e += NT) {
    const int32_t s = T.segs[s0 + e];
    const int a = T.seg_loc[2 * s], b = T.seg_loc[2 * s + 1];
    if (!skel_active(S.meas, a, b, length[s])) continue;
    double u[3];
    const double* P = ok ? S.X : S.Z;
    O.len_after[f * n_seg + s] = skel_unit(P + 3 * S.loc[a], P + 3 * S.loc[b], u);
  }
  if (t == 0) {
    O.chi2[cell] = ok ? S.scal[0] : S.scal[3];
    O.rows[cell] = rows;
    O.iterations[cell] = iters;
    O.comp_status[cell] = ok ? status : SKEL_COMP_FAILED;
  }
}

// what k_skel_pass writes for slot s before the adjustment: the input's bytes where measured, NaN elsewhere
CBA_HD void skel_pass_slot(int64_t s, const double* xyz, const double* meas_cov, const uint8_t* measured, double* pos, double* pos_cov, uint8_t* status) {
  const bool m = measured[s] == 1;
  const double nan = traj_nan();
  for (int c = 0; c < 3; ++c) pos[3 * s + c] = m ? xyz[3 * s + c] : nan;
  for (int c = 0; c < 6; ++c) pos_cov[6 * s + c] = m ? meas_cov[6 * s + c] : nan;
  status[s] = m ? SKEL_SLOT_INACTIVE : SKEL_SLOT_NONE;
}

}  // namespace cba

// ---- host side: the components, the checks, the serial forms -------------------------------------------------------------------------
#include <algorithm>
#include <numeric>
#include <string>
#include <utility>
#include <vector>

namespace cba {

struct SkelPlan {
  int32_t n_comp = 0, max_m = 0;
  std::vector<int32_t> traj_comp, comp_pt, pts, comp_seg, segs, seg_loc, inc_start, inc;
  SkelTables tables() const { return {comp_pt.data(), pts.data(), comp_seg.data(), segs.data(), seg_loc.data(), inc_start.data(), inc.data()}; }
};

// The components of the segment graph, numbered by their smallest trajectory, and the tables of k_skel_adjust.  0, or -1 / -4 with `msg`.
inline int skel_plan(const std::string& what, int64_t n_traj, int64_t n_seg, const int32_t* seg_traj, SkelPlan& P, std::string& msg) {
  if (n_traj < 0 || n_seg < 0) { msg = what + "negative size"; return -1; }
  if (n_traj > 0x7fffffff || n_seg > 0x3fffffff) { msg = what + "more trajectories or segments than 32-bit tables index"; return -4; }
  if (n_seg > 0 && !seg_traj) { msg = what + "seg_traj: null argument"; return -1; }
  std::vector<std::pair<int64_t, int64_t>> keys((size_t)n_seg);
  for (int64_t s = 0; s < n_seg; ++s) {
    const int64_t a = seg_traj[2 * s], b = seg_traj[2 * s + 1];
    if (a < 0 || a >= n_traj || b < 0 || b >= n_traj) {
      msg = what + "segment " + std::to_string(s) + ": trajectory " + std::to_string(a < 0 || a >= n_traj ? a : b) + " out of range (n_traj " +
            std::to_string(n_traj) + ")";
      return -1;
    }
    if (a == b) { msg = what + "segment " + std::to_string(s) + ": both ends are trajectory " + std::to_string(a); return -1; }
    keys[(size_t)s] = {std::min(a, b) * n_traj + std::max(a, b), s};
  }
  std::sort(keys.begin(), keys.end());
  for (size_t i = 1; i < keys.size(); ++i)
    if (keys[i].first == keys[i - 1].first) {
      msg = what + "segment " + std::to_string(keys[i].second) + " repeats the pair of segment " + std::to_string(keys[i - 1].second);
      return -1;
    }
  std::vector<int32_t> root((size_t)n_traj), degree((size_t)n_traj, 0);
  std::iota(root.begin(), root.end(), 0);
  auto find = [&](int32_t x) {
    while (root[(size_t)x] != x) x = root[(size_t)x] = root[(size_t)root[(size_t)x]];
    return x;
  };
  for (int64_t s = 0; s < n_seg; ++s) {
    const int32_t a = find(seg_traj[2 * s]), b = find(seg_traj[2 * s + 1]);
    root[(size_t)std::max(a, b)] = std::min(a, b);  // (the root of a component is its smallest trajectory)
    ++degree[(size_t)seg_traj[2 * s]];
    ++degree[(size_t)seg_traj[2 * s + 1]];
  }
  P = SkelPlan();
  P.traj_comp.assign((size_t)n_traj, -1);
  std::vector<int32_t> size;
  for (int64_t j = 0; j < n_traj; ++j) {
    if (!degree[(size_t)j]) continue;
    const int32_t r = find((int32_t)j);
    if (r == j) { P.traj_comp[(size_t)j] = P.n_comp++; size.push_back(0); }
    else P.traj_comp[(size_t)j] = P.traj_comp[(size_t)r];
    ++size[(size_t)P.traj_comp[(size_t)j]];
  }
  for (int64_t j = 0; j < n_traj; ++j) {
    const int32_t k = P.traj_comp[(size_t)j];
    if (k >= 0 && find((int32_t)j) == j && size[(size_t)k] > SKEL_MAX_POINTS) {
      msg = what + "the component of trajectory " + std::to_string(j) + " has " + std::to_string(size[(size_t)k]) + " trajectories, at most " +
            std::to_string(SKEL_MAX_POINTS) + " are supported (one workgroup factors a component in LDS)";
      return -4;
    }
  }
  P.comp_pt.assign((size_t)P.n_comp + 1, 0);
  P.comp_seg.assign((size_t)P.n_comp + 1, 0);
  for (int32_t k = 0; k < P.n_comp; ++k) {
    P.comp_pt[(size_t)k + 1] = P.comp_pt[(size_t)k] + size[(size_t)k];
    P.max_m = std::max(P.max_m, size[(size_t)k]);
  }
  for (int64_t s = 0; s < n_seg; ++s) ++P.comp_seg[(size_t)P.traj_comp[(size_t)seg_traj[2 * s]] + 1];
  for (int32_t k = 0; k < P.n_comp; ++k) P.comp_seg[(size_t)k + 1] += P.comp_seg[(size_t)k];
  std::vector<int32_t> place((size_t)n_traj, -1), fill_pt(P.comp_pt.begin(), P.comp_pt.end() - 1), fill_seg(P.comp_seg.begin(), P.comp_seg.end() - 1);
  P.pts.assign((size_t)P.comp_pt.back(), 0);
  for (int64_t j = 0; j < n_traj; ++j) {
    const int32_t k = P.traj_comp[(size_t)j];
    if (k < 0) continue;
    place[(size_t)j] = fill_pt[(size_t)k] - P.comp_pt[(size_t)k];
    P.pts[(size_t)fill_pt[(size_t)k]++] = (int32_t)j;
  }
  P.segs.assign((size_t)n_seg, 0);
  P.seg_loc.assign((size_t)n_seg * 2, 0);
  P.inc_start.assign(P.pts.size() + 1, 0);
  for (int64_t s = 0; s < n_seg; ++s) {
    const int32_t a = seg_traj[2 * s], b = seg_traj[2 * s + 1], k = P.traj_comp[(size_t)a];
    P.segs[(size_t)fill_seg[(size_t)k]++] = (int32_t)s;
    P.seg_loc[(size_t)(2 * s)] = place[(size_t)a];
    P.seg_loc[(size_t)(2 * s + 1)] = place[(size_t)b];
    ++P.inc_start[(size_t)(P.comp_pt[(size_t)k] + place[(size_t)a]) + 1];
    ++P.inc_start[(size_t)(P.comp_pt[(size_t)k] + place[(size_t)b]) + 1];
  }
  for (size_t i = 0; i + 1 < P.inc_start.size(); ++i) P.inc_start[i + 1] += P.inc_start[i];
  std::vector<int32_t> fill_inc(P.inc_start.begin(), P.inc_start.end() - 1);
  P.inc.assign((size_t)n_seg * 2, 0);
  for (int64_t s = 0; s < n_seg; ++s)
    for (int e = 0; e < 2; ++e) {
      const int32_t j = seg_traj[2 * s + e];
      P.inc[(size_t)fill_inc[(size_t)(P.comp_pt[(size_t)P.traj_comp[(size_t)j]] + place[(size_t)j])]++] = (int32_t)s;
    }
  return 0;
}

constexpr double SKEL_SLOT_BYTES = 24.0 + 48.0 + 1.0 + 24.0 + 48.0 + 1.0 + 8.0;  // (with 8 for the tables a trajectory takes: never less than they do)
constexpr double SKEL_FRAME_SEG_BYTES = 32.0, SKEL_FRAME_COMP_BYTES = 17.0;

inline double skel_device_bytes(double n_frames, double n_traj, double n_seg, double n_comp) {
  return n_frames * (n_traj * SKEL_SLOT_BYTES + n_seg * SKEL_FRAME_SEG_BYTES + n_comp * SKEL_FRAME_COMP_BYTES) + n_seg * 64.0;
}

// cba_adjust_skeleton: 0, or -1 (CBA_ERR_INVALID) / -4 (CBA_ERR_UNSUPPORTED) with `msg` naming the offender.  memory <= 0: not checked.
// *launch: whether there is anything to launch.
inline int skel_validate(const cba_skeleton_desc* d, double memory, SkelPlan& P, std::string& msg, bool* launch) {
  const std::string what = "cba_adjust_skeleton: ";
  *launch = false;
  if (!d) { msg = what + "null argument"; return -1; }
  if (d->n_frames < 0 || d->n_traj < 0 || d->n_seg < 0) { msg = what + "negative size"; return -1; }
  const struct { const char* name; double v; } reals[2] = {{"trim", d->trim}, {"tol", d->tol}};
  for (const auto& r : reals)
    if (!std::isfinite(r.v) || !(r.v > 0.0)) { msg = what + r.name + " must be finite and positive, got " + std::to_string(r.v); return -1; }
  if (d->max_iter < 1) { msg = what + "max_iter must be at least 1, got " + std::to_string(d->max_iter); return -1; }
  if ((double)d->n_frames * (double)d->n_traj >= 9.0e15 || (double)d->n_frames * (double)d->n_seg >= 9.0e15) { msg = what + "grid too large to index"; return -4; }
  if (d->n_seg > 0 && (!d->seg_traj || !d->seg_length || !d->seg_sigma)) { msg = what + "null argument"; return -1; }
  int rc = skel_plan(what, d->n_traj, d->n_seg, d->seg_traj, P, msg);
  if (rc) return rc;
  for (int64_t s = 0; s < d->n_seg; ++s) {
    if (!std::isfinite(d->seg_sigma[s]) || !(d->seg_sigma[s] > 0.0)) {
      msg = what + "segment " + std::to_string(s) + ": seg_sigma must be finite and positive, got " + std::to_string(d->seg_sigma[s]);
      return -1;
    }
    const double L = d->seg_length[s];
    if (!std::isnan(L) && (!std::isfinite(L) || !(L > 0.0))) {
      msg = what + "segment " + std::to_string(s) + ": a given seg_length must be finite and positive, got " + std::to_string(L);
      return -1;
    }
  }
  const int64_t n_slots = d->n_frames * d->n_traj;
  if (n_slots == 0) return 0;
  if (!d->xyz || !d->meas_cov || !d->measured) { msg = what + "null argument"; return -1; }
  bool any = false;
  for (int64_t s = 0; s < n_slots; ++s) {
    if (d->measured[s] != 1) continue;
    any = true;
    const double* z = d->xyz + 3 * s;
    const double* R = d->meas_cov + 6 * s;
    if (!std::isfinite(z[0]) || !std::isfinite(z[1]) || !std::isfinite(z[2])) { msg = what + "slot " + std::to_string(s) + ": xyz is not finite"; return -1; }
    double L[6];
    bool finite = true;
    for (int i = 0; i < 6; ++i) finite = finite && std::isfinite(R[i]);
    if (!finite) { msg = what + "slot " + std::to_string(s) + ": meas_cov is not finite"; return -1; }
    if (!chol3(R, L)) { msg = what + "slot " + std::to_string(s) + ": meas_cov is not positive definite (chol3 finds no positive pivots)"; return -1; }
  }
  *launch = any && d->n_seg > 0;
  const double bytes = skel_device_bytes((double)d->n_frames, (double)d->n_traj, (double)d->n_seg, (double)P.n_comp);
  if (*launch && memory > 0.0 && bytes > memory) {
    msg = what + "the grid of " + std::to_string(d->n_frames) + " frames x " + std::to_string(d->n_traj) + " trajectories with " +
          std::to_string(d->n_seg) + " segments in " + std::to_string(P.n_comp) + " components needs " + std::to_string((long long)bytes) +
          " bytes of device memory (" + std::to_string((int)SKEL_SLOT_BYTES) + " per slot, " + std::to_string((int)SKEL_FRAME_SEG_BYTES) +
          " per (frame, segment), " + std::to_string((int)SKEL_FRAME_COMP_BYTES) + " per (frame, component)), " + std::to_string((long long)memory) +
          " are available";
    return -4;
  }
  return 0;
}

// what a call returns before any kernel has run, and all of it when nothing is launched: the slots pass through, a given length is reported
inline void skel_nothing(const cba_skeleton_desc* d, int32_t n_comp, cba_skeleton_out* o) {
  const double nan = traj_nan();
  const int64_t n_slots = d->n_frames * d->n_traj;
  for (int64_t s = 0; s < n_slots; ++s) {
    const bool m = d->measured[s] == 1;
    for (int c = 0; c < 3; ++c) if (o->pos) o->pos[3 * s + c] = m ? d->xyz[3 * s + c] : nan;
    for (int c = 0; c < 6; ++c) if (o->pos_cov) o->pos_cov[6 * s + c] = m ? d->meas_cov[6 * s + c] : nan;
    if (o->status) o->status[s] = m ? SKEL_SLOT_INACTIVE : SKEL_SLOT_NONE;
  }
  for (int64_t s = 0; s < d->n_seg; ++s) {
    if (o->length) o->length[s] = d->seg_length[s];
    if (o->med) o->med[s] = nan;
    if (o->mad) o->mad[s] = nan;
    if (o->frames) o->frames[s] = 0;
  }
  for (int64_t i = 0; i < d->n_frames * d->n_seg; ++i) {
    if (o->len_before) o->len_before[i] = nan;
    if (o->w_before) o->w_before[i] = nan;
    if (o->len_after) o->len_after[i] = nan;
  }
  for (int64_t i = 0; i < d->n_frames * n_comp; ++i) {
    if (o->chi2) o->chi2[i] = 0.0;
    if (o->rows) o->rows[i] = 0;
    if (o->iterations) o->iterations[i] = 0;
    if (o->comp_status) o->comp_status[i] = SKEL_COMP_NONE;
  }
}

// host only: the lower median (rank floor((n - 1) / 2)) of v, which it reorders; NaN for none
inline double skel_lower_median(std::vector<double>& v) {
  if (v.empty()) return traj_nan();
  const size_t k = (v.size() - 1) / 2;
  std::nth_element(v.begin(), v.begin() + (std::ptrdiff_t)k, v.end());
  return v[k];
}

// host only: k_skel_length for segment s, serial
inline void skel_length_host(const cba_skeleton_desc* D, int64_t s, double* length, double* med, double* mad, int64_t* frames) {
  const int32_t a = D->seg_traj[2 * s], b = D->seg_traj[2 * s + 1];
  std::vector<double> d;
  for (int64_t f = 0; f < D->n_frames; ++f) {
    double df, v;
    if (skel_pair(f * D->n_traj + a, f * D->n_traj + b, D->xyz, D->meas_cov, D->measured, &df, &v)) d.push_back(df);
  }
  *frames = (int64_t)d.size();
  std::vector<double> w = d;
  *med = skel_lower_median(w);
  for (size_t i = 0; i < d.size(); ++i) w[i] = std::fabs(d[i] - *med);
  *mad = skel_lower_median(w);
  *length = D->seg_length[s];
  if (!std::isnan(*length) || d.empty()) return;
  double num = 0.0, den = 0.0;
  for (int t = 0; t < SKEL_LEN_THREADS; ++t) {
    double pn, pd;
    skel_length_lane(t, D->n_frames, D->n_traj, a, b, D->xyz, D->meas_cov, D->measured, *med, *mad, D->trim, &pn, &pd);
    num += pn;
    den += pd;
  }
  *length = num / den;
}

}  // namespace cba
