// The thread body and the host-side checks of k_traj_smooth / cba_smooth_trajectories / cba_reconstruct_trajectories_smoothed
// (include/caliscope/trajectory_smoother.h, where the model, the recursion and its limits are stated).  Compiled by hipcc into the
// kernel of trajectory_lib.hip and by g++ into tests/native/trajectory_smooth_harness.cpp, which runs the same routine trajectory by
// trajectory.
//
// Registers only.  The covariance P = [[A, B], [B^T, C]] is held as A (6, xx xy xz yy yz zz), B (9, row-major: cov(p_i, v_j)) and
// C (6), the adjoint Lambda likewise; every index is a compile-time constant after unrolling (sym3 folds).  One thread runs a
// trajectory forward and backward: a serial recurrence, so what is tuned here is the latency of a step (loads of the next frame in
// flight during the arithmetic of this one), not throughput.
//
// Scratch.  park[c * n_slots + s], c < SMOOTH_PARK: lanes of a wave are neighbouring trajectories of one frame, so every access is to
// consecutive doubles.  Rows 0..26 (filtered x, A, B, C) are written for every frame of the span, rows 27..44 (u, S^-1, N) for the
// measured ones after f0 alone, and read back under the same conditions.  status doubles as the measured flag of the backward pass:
// the forward pass writes 1 at a measured frame, SMOOTH_AFTER_FILLABLE at one that ends a hole of at most max_gap frames, and the
// backward pass replaces both by the status of the call.  pos, vel, pos_cov, vel_cov and nis are NaN and status 0 before the thread
// runs (the caller's memset): the thread writes the rows that have a result and no others.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/caliscope/trajectory_smoother.h"
#include "trajectory_cov_math.h"

namespace cba {

constexpr int SMOOTH_NONE = 0, SMOOTH_MEASURED = 1, SMOOTH_INTERPOLATED = 2;
constexpr int SMOOTH_AFTER_FILLABLE = 3;  // between the passes only
constexpr int SMOOTH_PARK = 45;           // doubles parked per slot
constexpr int PARK_X = 0, PARK_A = 6, PARK_B = 12, PARK_C = 21, PARK_U = 27, PARK_SI = 30, PARK_N = 36;

// entry (i, j) of a symmetric 3 x 3 held as xx xy xz yy yz zz
constexpr int sym3(int i, int j) { return i <= j ? (i == 0 ? j : i + j + 1) : (j == 0 ? i : i + j + 1); }

struct SmoothModel {
  double dt, qpp, qpv, qvv, sv2;  // Q = [[qpp I, qpv I], [qpv I, qvv I]], sv2 = velocity_prior_std^2
  int32_t max_gap;
};

inline SmoothModel smooth_model(double fps, double accel_density, double velocity_prior_std, int32_t max_gap) {
  const double dt = 1.0 / fps, q2 = accel_density * accel_density;
  return SmoothModel{dt, q2 * dt * dt * dt / 3.0, q2 * dt * dt / 2.0, q2 * dt, velocity_prior_std * velocity_prior_std, max_gap};
}

#if defined(__HIPCC__)
#define CBA_UNROLL _Pragma("unroll")
#else
#define CBA_UNROLL
#endif

// S^-1 of a symmetric 3 x 3; false when chol3 finds a pivot that is not safely positive
CBA_HD bool smooth_inv3(const double* S, double* Si) {
  double L[6], w[3], I0[3], I1[3], I2[3];
  if (!chol3(S, L)) return false;
  const double e0[3] = {1.0, 0.0, 0.0}, e1[3] = {0.0, 1.0, 0.0}, e2[3] = {0.0, 0.0, 1.0};
  chol3_fwd(L, e0, w); chol3_bwd(L, w, I0);
  chol3_fwd(L, e1, w); chol3_bwd(L, w, I1);
  chol3_fwd(L, e2, w); chol3_bwd(L, w, I2);
  Si[0] = I0[0]; Si[1] = 0.5 * (I0[1] + I1[0]); Si[2] = 0.5 * (I0[2] + I2[0]);
  Si[3] = I1[1]; Si[4] = 0.5 * (I1[2] + I2[1]); Si[5] = I2[2];
  return true;
}

// x <- F x, P <- F P F^T + Q
CBA_HD void smooth_predict(const SmoothModel& m, double* x, double* A, double* B, double* C) {
  const double dt = m.dt, dt2 = m.dt * m.dt;
  CBA_UNROLL
  for (int i = 0; i < 3; ++i) x[i] += dt * x[3 + i];
  CBA_UNROLL
  for (int i = 0; i < 3; ++i) {
    CBA_UNROLL
    for (int j = i; j < 3; ++j) A[sym3(i, j)] += dt * (B[3 * i + j] + B[3 * j + i]) + dt2 * C[sym3(i, j)] + (i == j ? m.qpp : 0.0);
  }
  CBA_UNROLL
  for (int i = 0; i < 3; ++i) {
    CBA_UNROLL
    for (int j = 0; j < 3; ++j) B[3 * i + j] += dt * C[sym3(i, j)] + (i == j ? m.qpv : 0.0);
  }
  C[0] += m.qvv; C[3] += m.qvv; C[5] += m.qvv;
}

// The measurement z with covariance R at a predicted pair: the filtered pair in place, u = S^-1 y, S^-1, N = -S^-1 B and the nis.
// false, and nothing is changed, when S has no positive pivots (it has them whenever R has: A is positive semi-definite).
CBA_HD bool smooth_update(const double* z, const double* R, double* x, double* A, double* B, double* C, double* u, double* Si, double* N,
                          double* nis) {
  double S[6], y[3], M[9];
  CBA_UNROLL
  for (int i = 0; i < 6; ++i) S[i] = A[i] + R[i];
  if (!smooth_inv3(S, Si)) return false;
  CBA_UNROLL
  for (int i = 0; i < 3; ++i) y[i] = z[i] - x[i];
  CBA_UNROLL
  for (int i = 0; i < 3; ++i) u[i] = Si[sym3(i, 0)] * y[0] + Si[sym3(i, 1)] * y[1] + Si[sym3(i, 2)] * y[2];
  *nis = y[0] * u[0] + y[1] * u[1] + y[2] * u[2];
  CBA_UNROLL
  for (int i = 0; i < 3; ++i) {
    x[i] += A[sym3(i, 0)] * u[0] + A[sym3(i, 1)] * u[1] + A[sym3(i, 2)] * u[2];
    x[3 + i] += B[i] * u[0] + B[3 + i] * u[1] + B[6 + i] * u[2];
  }
  // M = S^-1 R (so that I - K H = [[M^T, 0], [N^T, I]]), N = -S^-1 B
  CBA_UNROLL
  for (int i = 0; i < 3; ++i) {
    CBA_UNROLL
    for (int j = 0; j < 3; ++j) {
      M[3 * i + j] = Si[sym3(i, 0)] * R[sym3(0, j)] + Si[sym3(i, 1)] * R[sym3(1, j)] + Si[sym3(i, 2)] * R[sym3(2, j)];
      N[3 * i + j] = -(Si[sym3(i, 0)] * B[j] + Si[sym3(i, 1)] * B[3 + j] + Si[sym3(i, 2)] * B[6 + j]);
    }
  }
  // C - B^T S^-1 B, M^T B, and M^T A with the two halves of its rounding averaged
  double nA[6], nB[9];
  CBA_UNROLL
  for (int i = 0; i < 3; ++i) {
    CBA_UNROLL
    for (int j = i; j < 3; ++j) {
      C[sym3(i, j)] += B[i] * N[j] + B[3 + i] * N[3 + j] + B[6 + i] * N[6 + j];
      const double ij = M[i] * A[sym3(0, j)] + M[3 + i] * A[sym3(1, j)] + M[6 + i] * A[sym3(2, j)];
      const double ji = M[j] * A[sym3(0, i)] + M[3 + j] * A[sym3(1, i)] + M[6 + j] * A[sym3(2, i)];
      nA[sym3(i, j)] = 0.5 * (ij + ji);
    }
    CBA_UNROLL
    for (int j = 0; j < 3; ++j) nB[3 * i + j] = M[i] * B[j] + M[3 + i] * B[3 + j] + M[6 + i] * B[6 + j];
  }
  CBA_UNROLL
  for (int i = 0; i < 6; ++i) A[i] = nA[i];
  CBA_UNROLL
  for (int i = 0; i < 9; ++i) B[i] = nB[i];
  return true;
}

// what the forward pass reads of a frame
struct SmoothSample {
  double z[3], R[6];
  bool measured;
};

CBA_HD SmoothSample smooth_load_sample(int64_t s, const double* xyz, const double* meas_cov, const uint8_t* measured) {
  SmoothSample m;
  CBA_UNROLL
  for (int i = 0; i < 3; ++i) m.z[i] = xyz[3 * s + i];
  CBA_UNROLL
  for (int i = 0; i < 6; ++i) m.R[i] = meas_cov[6 * s + i];
  m.measured = measured[s] == 1;
  return m;
}

// what the backward pass reads of a frame (u, Si, N hold what the scratch held at a frame that parked none: they are not used there)
struct SmoothParked {
  double x[6], A[6], B[9], C[6], u[3], Si[6], N[9], R[6];
  int flag;
};

CBA_HD SmoothParked smooth_load_parked(int64_t n_slots, int64_t s, const double* park, const double* meas_cov, const uint8_t* status) {
  SmoothParked p;
  const double* at = park + s;
  CBA_UNROLL
  for (int i = 0; i < 6; ++i) p.x[i] = at[(PARK_X + i) * n_slots];
  CBA_UNROLL
  for (int i = 0; i < 6; ++i) p.A[i] = at[(PARK_A + i) * n_slots];
  CBA_UNROLL
  for (int i = 0; i < 9; ++i) p.B[i] = at[(PARK_B + i) * n_slots];
  CBA_UNROLL
  for (int i = 0; i < 6; ++i) p.C[i] = at[(PARK_C + i) * n_slots];
  CBA_UNROLL
  for (int i = 0; i < 3; ++i) p.u[i] = at[(PARK_U + i) * n_slots];
  CBA_UNROLL
  for (int i = 0; i < 6; ++i) p.Si[i] = at[(PARK_SI + i) * n_slots];
  CBA_UNROLL
  for (int i = 0; i < 9; ++i) p.N[i] = at[(PARK_N + i) * n_slots];
  CBA_UNROLL
  for (int i = 0; i < 6; ++i) p.R[i] = meas_cov[6 * s + i];
  p.flag = status[s];
  return p;
}

CBA_HD void smooth_park_state(int64_t n_slots, int64_t s, const double* x, const double* A, const double* B, const double* C, double* park) {
  double* at = park + s;
  CBA_UNROLL
  for (int i = 0; i < 6; ++i) at[(PARK_X + i) * n_slots] = x[i];
  CBA_UNROLL
  for (int i = 0; i < 6; ++i) at[(PARK_A + i) * n_slots] = A[i];
  CBA_UNROLL
  for (int i = 0; i < 9; ++i) at[(PARK_B + i) * n_slots] = B[i];
  CBA_UNROLL
  for (int i = 0; i < 6; ++i) at[(PARK_C + i) * n_slots] = C[i];
}

// smoothed x = x - P lambda and the position and velocity blocks of P - P Lambda P, stored as the row of slot s
CBA_HD void smooth_store(int64_t s, const SmoothParked& p, const double* lam, const double* LA, const double* LB, const double* LC, int status,
                         double* pos, double* vel, double* pos_cov, double* vel_cov, uint8_t* out_status) {
  const double *A = p.A, *B = p.B, *C = p.C;
  CBA_UNROLL
  for (int i = 0; i < 3; ++i) {
    pos[3 * s + i] = p.x[i] - (A[sym3(i, 0)] * lam[0] + A[sym3(i, 1)] * lam[1] + A[sym3(i, 2)] * lam[2] + B[3 * i] * lam[3] + B[3 * i + 1] * lam[4] +
                               B[3 * i + 2] * lam[5]);
    vel[3 * s + i] = p.x[3 + i] - (B[i] * lam[0] + B[3 + i] * lam[1] + B[6 + i] * lam[2] + C[sym3(i, 0)] * lam[3] + C[sym3(i, 1)] * lam[4] +
                                   C[sym3(i, 2)] * lam[5]);
  }
  // U = Lambda P: U11 = LA A + LB B^T, U21 = LB^T A + LC B^T, U12 = LA B + LB C, U22 = LB^T B + LC C
  double U11[9], U21[9], U12[9], U22[9];
  CBA_UNROLL
  for (int i = 0; i < 3; ++i) {
    CBA_UNROLL
    for (int j = 0; j < 3; ++j) {
      double a = 0.0, b = 0.0, c = 0.0, d = 0.0;
      CBA_UNROLL
      for (int k = 0; k < 3; ++k) {
        a += LA[sym3(i, k)] * A[sym3(k, j)] + LB[3 * i + k] * B[3 * j + k];
        b += LB[3 * k + i] * A[sym3(k, j)] + LC[sym3(i, k)] * B[3 * j + k];
        c += LA[sym3(i, k)] * B[3 * k + j] + LB[3 * i + k] * C[sym3(k, j)];
        d += LB[3 * k + i] * B[3 * k + j] + LC[sym3(i, k)] * C[sym3(k, j)];
      }
      U11[3 * i + j] = a; U21[3 * i + j] = b; U12[3 * i + j] = c; U22[3 * i + j] = d;
    }
  }
  CBA_UNROLL
  for (int i = 0; i < 3; ++i) {
    CBA_UNROLL
    for (int j = i; j < 3; ++j) {
      double pp = 0.0, vv = 0.0;
      CBA_UNROLL
      for (int k = 0; k < 3; ++k) {
        pp += A[sym3(i, k)] * U11[3 * k + j] + B[3 * i + k] * U21[3 * k + j];
        vv += B[3 * k + i] * U12[3 * k + j] + C[sym3(i, k)] * U22[3 * k + j];
      }
      pos_cov[6 * s + sym3(i, j)] = A[sym3(i, j)] - pp;
      vel_cov[6 * s + sym3(i, j)] = C[sym3(i, j)] - vv;
    }
  }
  out_status[s] = (uint8_t)status;
}

// lambda <- G lambda - H^T u, Lambda <- G Lambda G^T + H^T S^-1 H with G = (I - K H)^T = [[M, N], [0, I]], M = S^-1 R:
// Lambda_pp <- T1 M^T + T2 N^T + S^-1, Lambda_pv <- T2, Lambda_vv stays, with T1 = M LA + N LB^T and T2 = M LB + N LC
CBA_HD void smooth_adjoint_measurement(const SmoothParked& p, double* lam, double* LA, double* LB, const double* LC) {
  double M[9], T1[9], T2[9], lp[3];
  const double* N = p.N;
  CBA_UNROLL
  for (int i = 0; i < 3; ++i) {
    CBA_UNROLL
    for (int j = 0; j < 3; ++j) M[3 * i + j] = p.Si[sym3(i, 0)] * p.R[sym3(0, j)] + p.Si[sym3(i, 1)] * p.R[sym3(1, j)] + p.Si[sym3(i, 2)] * p.R[sym3(2, j)];
  }
  CBA_UNROLL
  for (int i = 0; i < 3; ++i)
    lp[i] = M[3 * i] * lam[0] + M[3 * i + 1] * lam[1] + M[3 * i + 2] * lam[2] + N[3 * i] * lam[3] + N[3 * i + 1] * lam[4] + N[3 * i + 2] * lam[5] - p.u[i];
  lam[0] = lp[0]; lam[1] = lp[1]; lam[2] = lp[2];
  CBA_UNROLL
  for (int i = 0; i < 3; ++i) {
    CBA_UNROLL
    for (int j = 0; j < 3; ++j) {
      double a = 0.0, b = 0.0;
      CBA_UNROLL
      for (int k = 0; k < 3; ++k) {
        a += M[3 * i + k] * LA[sym3(k, j)] + N[3 * i + k] * LB[3 * j + k];
        b += M[3 * i + k] * LB[3 * k + j] + N[3 * i + k] * LC[sym3(k, j)];
      }
      T1[3 * i + j] = a; T2[3 * i + j] = b;
    }
  }
  CBA_UNROLL
  for (int i = 0; i < 3; ++i) {
    CBA_UNROLL
    for (int j = i; j < 3; ++j) {
      double a = p.Si[sym3(i, j)];
      CBA_UNROLL
      for (int k = 0; k < 3; ++k) a += T1[3 * i + k] * M[3 * j + k] + T2[3 * i + k] * N[3 * j + k];
      LA[sym3(i, j)] = a;
    }
  }
  CBA_UNROLL
  for (int i = 0; i < 9; ++i) LB[i] = T2[i];
}

// lambda <- F^T lambda, Lambda <- F^T Lambda F
CBA_HD void smooth_adjoint_step(const SmoothModel& m, double* lam, const double* LA, double* LB, double* LC) {
  const double dt = m.dt, dt2 = m.dt * m.dt;
  CBA_UNROLL
  for (int i = 0; i < 3; ++i) lam[3 + i] += dt * lam[i];
  CBA_UNROLL
  for (int i = 0; i < 3; ++i) {
    CBA_UNROLL
    for (int j = i; j < 3; ++j) LC[sym3(i, j)] += dt * (LB[3 * i + j] + LB[3 * j + i]) + dt2 * LA[sym3(i, j)];
  }
  CBA_UNROLL
  for (int i = 0; i < 3; ++i) {
    CBA_UNROLL
    for (int j = 0; j < 3; ++j) LB[3 * i + j] += dt * LA[sym3(i, j)];
  }
}

// k_traj_smooth, trajectory j.  measured[s] == 1: the slot has the sample xyz[s] with covariance meas_cov[s] (neither is used
// elsewhere).  park: SMOOTH_PARK n_slots doubles.  The six outputs are NaN / 0 before the call.
CBA_HD void traj_smooth_thread(int64_t n_frames, int64_t n_traj, int64_t j, const double* xyz, const double* meas_cov, const uint8_t* measured,
                               const SmoothModel& m, double* park, double* pos, double* vel, double* pos_cov, double* vel_cov, double* nis,
                               uint8_t* status) {
  const int64_t n_slots = n_frames * n_traj;
  int64_t f0 = -1, f1 = -1;
  for (int64_t f = 0; f < n_frames; ++f)
    if (measured[f * n_traj + j] == 1) {
      if (f0 < 0) f0 = f;
      f1 = f;
    }
  if (f0 < 0) return;
  // forward
  double x[6], A[6], B[9], C[6];
  {
    const SmoothSample first = smooth_load_sample(f0 * n_traj + j, xyz, meas_cov, measured);
    CBA_UNROLL
    for (int i = 0; i < 3; ++i) { x[i] = first.z[i]; x[3 + i] = 0.0; }
    CBA_UNROLL
    for (int i = 0; i < 6; ++i) { A[i] = first.R[i]; C[i] = 0.0; }
    CBA_UNROLL
    for (int i = 0; i < 9; ++i) B[i] = 0.0;
    C[0] = C[3] = C[5] = m.sv2;
    smooth_park_state(n_slots, f0 * n_traj + j, x, A, B, C, park);
    status[f0 * n_traj + j] = SMOOTH_MEASURED;
  }
  int64_t run = 0;  // unmeasured frames since the last measured one
  SmoothSample next = smooth_load_sample((f0 < f1 ? f0 + 1 : f1) * n_traj + j, xyz, meas_cov, measured);
  for (int64_t f = f0 + 1; f <= f1; ++f) {
    const int64_t s = f * n_traj + j;
    const SmoothSample cur = next;
    next = smooth_load_sample((f < f1 ? f + 1 : f1) * n_traj + j, xyz, meas_cov, measured);  // in flight during the step
    smooth_predict(m, x, A, B, C);
    double u[3], Si[6], N[9], q;
    if (cur.measured && smooth_update(cur.z, cur.R, x, A, B, C, u, Si, N, &q)) {
      double* at = park + s;
      CBA_UNROLL
      for (int i = 0; i < 3; ++i) at[(PARK_U + i) * n_slots] = u[i];
      CBA_UNROLL
      for (int i = 0; i < 6; ++i) at[(PARK_SI + i) * n_slots] = Si[i];
      CBA_UNROLL
      for (int i = 0; i < 9; ++i) at[(PARK_N + i) * n_slots] = N[i];
      nis[s] = q;
      status[s] = run > 0 && run <= (int64_t)m.max_gap ? SMOOTH_AFTER_FILLABLE : SMOOTH_MEASURED;
      run = 0;
    } else {
      ++run;  // (a sample whose S has no positive pivots is passed over like a hole; valid input has none)
    }
    smooth_park_state(n_slots, s, x, A, B, C, park);
  }
  // backward
  double lam[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, LA[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, LC[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double LB[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool fill = false;  // the unmeasured frames below the last measured one passed belong to a hole of at most max_gap frames
  SmoothParked back = smooth_load_parked(n_slots, f1 * n_traj + j, park, meas_cov, status);
  for (int64_t f = f1; f >= f0; --f) {
    const int64_t s = f * n_traj + j;
    const SmoothParked cur = back;
    back = smooth_load_parked(n_slots, (f > f0 ? f - 1 : f0) * n_traj + j, park, meas_cov, status);  // in flight during the step
    const bool meas = cur.flag != SMOOTH_NONE;
    const int st = meas ? SMOOTH_MEASURED : (fill ? SMOOTH_INTERPOLATED : SMOOTH_NONE);
    if (st != SMOOTH_NONE) smooth_store(s, cur, lam, LA, LB, LC, st, pos, vel, pos_cov, vel_cov, status);
    if (meas) {
      fill = cur.flag == SMOOTH_AFTER_FILLABLE;
      if (f > f0) smooth_adjoint_measurement(cur, lam, LA, LB, LC);
    }
    smooth_adjoint_step(m, lam, LA, LB, LC);
  }
}

}  // namespace cba

// ---- host side: sizes and the checks of the two calls ------------------------------------------------------------------------------
#include <string>

namespace cba {

// bytes per slot the smoother adds to a call: meas_cov 48, the six outputs 153, the parked rows 360
constexpr double SMOOTH_SLOT_BYTES = 48.0 + 153.0 + 8.0 * SMOOTH_PARK;

inline double traj_smooth_device_bytes(double n_frames, double n_traj, bool standalone) {
  return n_frames * n_traj * (SMOOTH_SLOT_BYTES + (standalone ? 25.0 : 0.0));  // (+ xyz 24, measured 1)
}

// fps, accel_density, velocity_prior_std finite and positive, max_gap >= 0; -1 with the field named
inline int traj_smoother_validate(const std::string& what, double fps, double accel_density, double velocity_prior_std, int32_t max_gap,
                                  std::string& msg) {
  const struct { const char* name; double v; } reals[3] = {{"fps", fps}, {"accel_density", accel_density}, {"velocity_prior_std", velocity_prior_std}};
  for (const auto& r : reals)
    if (!std::isfinite(r.v) || !(r.v > 0.0)) { msg = what + r.name + " must be finite and positive, got " + std::to_string(r.v); return -1; }
  if (max_gap < 0) { msg = what + "max_gap must not be negative, got " + std::to_string(max_gap); return -1; }
  return 0;
}

// cba_smooth_trajectories: 0, or -1 (CBA_ERR_INVALID) / -4 (CBA_ERR_UNSUPPORTED) with `msg` naming the field or the slot.
// memory <= 0: not checked.  *any_measured: whether there is anything to launch.
inline int traj_smooth_validate(const cba_smooth_desc* d, double memory, std::string& msg, bool* any_measured) {
  const std::string what = "cba_smooth_trajectories: ";
  *any_measured = false;
  if (!d) { msg = what + "null argument"; return -1; }
  if (d->n_frames < 0 || d->n_traj < 0) { msg = what + "negative size"; return -1; }
  const int rc = traj_smoother_validate(what, d->fps, d->accel_density, d->velocity_prior_std, d->max_gap, msg);
  if (rc) return rc;
  if ((double)d->n_frames * (double)d->n_traj >= 9.0e15) { msg = what + "grid too large to index"; return -4; }
  const int64_t n_slots = d->n_frames * d->n_traj;
  if (n_slots == 0) return 0;
  if (!d->xyz || !d->meas_cov || !d->measured) { msg = what + "null argument"; return -1; }
  for (int64_t s = 0; s < n_slots; ++s) {
    if (d->measured[s] != 1) continue;
    *any_measured = true;
    const double* z = d->xyz + 3 * s;
    const double* R = d->meas_cov + 6 * s;
    if (!std::isfinite(z[0]) || !std::isfinite(z[1]) || !std::isfinite(z[2])) { msg = what + "slot " + std::to_string(s) + ": xyz is not finite"; return -1; }
    double L[6];
    bool finite = true;
    for (int i = 0; i < 6; ++i) finite = finite && std::isfinite(R[i]);
    if (!finite) { msg = what + "slot " + std::to_string(s) + ": meas_cov is not finite"; return -1; }
    if (!chol3(R, L)) { msg = what + "slot " + std::to_string(s) + ": meas_cov is not positive definite (chol3 finds no positive pivots)"; return -1; }
  }
  const double bytes = traj_smooth_device_bytes((double)d->n_frames, (double)d->n_traj, true);
  if (*any_measured && memory > 0.0 && bytes > memory) {
    msg = what + "the grid of " + std::to_string(d->n_frames) + " frames x " + std::to_string(d->n_traj) + " trajectories needs " +
          std::to_string((long long)bytes) + " bytes of device memory, " + std::to_string((long long)memory) + " are available";
    return -4;
  }
  return 0;
}

// cba_reconstruct_trajectories_smoothed: the checks of the uncertain call, those of the model, the refusal of a second fill or filter,
// and the memory check with all buffers counted.  memory <= 0: not checked.
inline int traj_smoothed_validate(const cba_traj_desc* d, const cba_traj_refine* r, const cba_traj_uncertainty* u, const cba_traj_cov_out* o,
                                  const cba_traj_smoother* sm, const cba_traj_smooth_out* so, double memory, std::string& msg) {
  const std::string what = "cba_reconstruct_trajectories_smoothed: ";
  if (!u || !o) { msg = what + "uncertainty: null argument (the smoother weights a sample by its covariance)"; return -1; }
  if (!sm || !so) { msg = what + "smoother: null argument"; return -1; }
  int rc = traj_uncertain_validate(d, r, u, o, 0.0, msg);
  if (rc) return rc;
  rc = traj_smoother_validate(what, sm->fps, sm->accel_density, sm->velocity_prior_std, sm->max_gap, msg);
  if (rc) return rc;
  if (d->xyz_gap > 0) { msg = what + "xyz_gap " + std::to_string(d->xyz_gap) + " with the smoother: it fills the holes itself (max_gap)"; return -1; }
  if (d->filter_b) { msg = what + "a Butterworth filter with the smoother: one call smooths once"; return -1; }
  const double bytes = traj_device_bytes(d) + (r ? traj_refine_device_bytes(d) : 0.0) + traj_cov_device_bytes(d, u, o) +
                       traj_smooth_device_bytes((double)d->n_frames, (double)d->n_traj, false);
  if (d->n_rows > 0 && memory > 0.0 && bytes > memory) {
    msg = what + "the grid of " + std::to_string(d->n_cams) + " cameras x " + std::to_string(d->n_frames) + " frames x " + std::to_string(d->n_traj) +
          " trajectories with its covariances and the smoother needs " + std::to_string((long long)bytes) + " bytes of device memory, " +
          std::to_string((long long)memory) + " are available";
    return -4;
  }
  return 0;
}

}  // namespace cba
