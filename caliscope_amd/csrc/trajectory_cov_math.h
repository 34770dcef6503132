// The thread body and the host-side checks of k_traj_cov / cba_reconstruct_trajectories_uncertain
// (include/caliscope/trajectory_uncertainty.h, where the mathematics and its limits are stated).  Compiled by hipcc into the kernel of
// trajectory_lib.hip and by g++ into tests/native/trajectory_cov_harness.cpp, which runs the same routine slot by slot.
//
// Registers only.  V, its Cholesky factor, the gain M_c (3 x 9), the Jacobians of the second camera and the sums are small arrays whose every index
// is a compile-time constant after unrolling; nothing is indexed by a camera counter but the wave-uniform tables (CamTab, width,
// offset, cam_cov) and the grids.  Both camera loops run on wave-uniform counters: a lane that does not use a camera carries a
// zero gain through it, and a camera that no lane of the wave uses is skipped (traj_cov_any), so a large rig whose landmarks are
// seen by a few cameras each does not pay n_cams^2 per wave.  cam_cov is read inside the blocks of the two cameras alone: the
// rows and columns 6..8 under the (uniform) width of their camera.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/caliscope/trajectory_uncertainty.h"
#include "trajectory_refine_math.h"

namespace cba {

constexpr int COV_NO_POINT = 0, COV_OK = 1, COV_NOT_COMPUTABLE = 2;
constexpr int TRAJ_COV_LDS_CAMS = 128;  // camera tables staged in LDS up to here (48 KiB); above, uniform global loads

// does any lane of the wave set the flag?  (the harness runs one slot at a time)
CBA_HD bool traj_cov_any(bool flag) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ballot(flag ? 1 : 0) != 0;
#else
  return flag;
#endif
}

// Is camera c a view in use of slot s?  view_state: the refinement's grid, or null in the plain call (the posed cameras with a cell).
CBA_HD bool traj_cov_uses(int32_t c, int64_t n_slots, int64_t s, bool live, const uint8_t* cam_posed, const double* xy, const uint8_t* view_state) {
  const int64_t cell = (int64_t)c * n_slots + s;
  if (!live) return false;
  return view_state ? view_state[cell] == VIEW_USED : (cam_posed[c] != 0 && !traj_is_nan(xy[2 * cell]));
}

// B (2 x 3) and A (2 x 9) of one camera at X in pixels (project_full's times fx0; the intrinsic columns of a 6-wide camera zero),
// and the depth.  Nothing is selected here: a lane that does not use the camera gets numbers it throws away.
CBA_HD double traj_cov_jacobians(const CamTab& t, double X, double Y, double Z, double (*A)[MAX_NC], double (*B)[3]) {
  double e[2];
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int j = 0; j < MAX_NC; ++j) A[0][j] = A[1][j] = 0.0;
  project_full(t, X, Y, Z, 0.0, 0.0, e, A, B);
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int r = 0; r < 2; ++r) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < MAX_NC; ++j) A[r][j] *= t.fx0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 3; ++j) B[r][j] *= t.fx0;
  }
  return t.t[2] + t.R[6] * X + t.R[7] * Y + t.R[8] * Z;
}

// column j of M = V^-1 B^T A (3 x 9) of one camera, L the factor of V; zero for a lane that does not use the camera
CBA_HD void traj_cov_gain_column(const double (*A)[MAX_NC], const double (*B)[3], bool used, const double* L, int j, double* m) {
  const double rhs[3] = {B[0][0] * A[0][j] + B[1][0] * A[1][j], B[0][1] * A[0][j] + B[1][1] * A[1][j], B[0][2] * A[0][j] + B[1][2] * A[1][j]};
  double w[3], x[3];
  chol3_fwd(L, rhs, w);
  chol3_bwd(L, w, x);
  m[0] = used ? x[0] : 0.0;
  m[1] = used ? x[1] : 0.0;
  m[2] = used ? x[2] : 0.0;
}

// W (3 x 3) = Mc S M2^T, S the block of cam_cov at rows off_c.. (width np_c) and columns off_2.. (width np_2).  Mc is held; M2 is
// recomputed a column at a time from the second camera's A and B (27 registers less than holding it), or, DIAG, is Mc itself.
// Every address is wave-uniform and inside the block: rows and columns 6..8 are read for a 9-wide camera only (the gains there
// are zero otherwise).
template <bool DIAG>
CBA_HD void traj_cov_pair(const double (*Mc)[MAX_NC], const double (*A2)[MAX_NC], const double (*B2)[3], bool used_2, const double* L,
                          const double* cam_cov, int64_t ncp, int64_t off_c, bool wide_c, int64_t off_2, bool wide_2, double (*W)[3]) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < 3; ++i) W[i][0] = W[i][1] = W[i][2] = 0.0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int l = 0; l < MAX_NC; ++l) {
    if (l >= 6 && !wide_2) continue;
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < MAX_NC; ++k) {
      if (k >= 6 && !wide_c) continue;
      const double sv = cam_cov[(off_c + k) * ncp + off_2 + l];
      t0 += Mc[0][k] * sv;
      t1 += Mc[1][k] * sv;
      t2 += Mc[2][k] * sv;
    }
    double m[3];
    if constexpr (DIAG) { m[0] = Mc[0][l]; m[1] = Mc[1][l]; m[2] = Mc[2][l]; }
    else traj_cov_gain_column(A2, B2, used_2, L, l, m);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 3; ++j) {
      W[0][j] += t0 * m[j];
      W[1][j] += t1 * m[j];
      W[2][j] += t2 * m[j];
    }
  }
}

CBA_HD void traj_cov_store(int64_t s, const double* total, const double* calib, const double* noise, int status, double* cov, double* cov_calib,
                           uint8_t* cov_status, double* meas_cov) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < 6; ++i) {
    cov[6 * s + i] = total[i];
    if (cov_calib) cov_calib[6 * s + i] = calib[i];
    if (meas_cov) meas_cov[6 * s + i] = noise[i];
  }
  cov_status[s] = (uint8_t)status;
}

// k_traj_cov, slot s.  tabs: the CamTab of every camera (LDS or global); cam_np[c]: 6 or 9, 0 for a camera that takes no part;
// cam_off[c]: its first row in cam_cov or -1; cam_cov null: the noise term alone (cam_off is not read, cov_calib gets NaN).
// valid and xyz are those of the call at this point: the refined (or the DLT) points, before the 3-D fill.  meas_cov (the smoothed
// call; null: the stores of the uncertain call and no others) takes the noise term alone, before the calibration term is added.
CBA_HD void traj_cov_slot(int32_t n_cams, int64_t n_slots, int64_t s, const CamTab* tabs, const int32_t* cam_np, const int64_t* cam_off,
                          const double* cam_cov, int64_t ncp, double sigma_px, const uint8_t* cam_posed, const double* xy, const uint8_t* view_state,
                          const uint8_t* valid, const double* xyz, double* cov, double* cov_calib, uint8_t* cov_status,
                          double* meas_cov = nullptr) {
  const double nan = traj_nan();
  const double none[6] = {nan, nan, nan, nan, nan, nan};
  const bool live = valid[s] == 1;
  const double X = xyz[3 * s], Y = xyz[3 * s + 1], Z = xyz[3 * s + 2];
  // pass 1: V = sum B^T B over the views in use (xx xy xz yy yz zz), every one of them in front of its camera
  double V[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool front = true;
  for (int32_t c = 0; c < n_cams; ++c) {
    if (cam_np[c] == 0) continue;
    const bool used = traj_cov_uses(c, n_slots, s, live, cam_posed, xy, view_state);
    if (!traj_cov_any(used)) continue;
    double A[2][MAX_NC], B[2][3];
    const double Zc = traj_cov_jacobians(tabs[c], X, Y, Z, A, B);
    front = front && (!used || Zc > 0.0);
    const double b00 = used ? B[0][0] : 0.0, b01 = used ? B[0][1] : 0.0, b02 = used ? B[0][2] : 0.0;
    const double b10 = used ? B[1][0] : 0.0, b11 = used ? B[1][1] : 0.0, b12 = used ? B[1][2] : 0.0;
    V[0] += b00 * b00 + b10 * b10;
    V[1] += b00 * b01 + b10 * b11;
    V[2] += b00 * b02 + b10 * b12;
    V[3] += b01 * b01 + b11 * b11;
    V[4] += b01 * b02 + b11 * b12;
    V[5] += b02 * b02 + b12 * b12;
  }
  double L[6];
  if (!live || !front || !chol3(V, L)) {
    traj_cov_store(s, none, none, none, live ? COV_NOT_COMPUTABLE : COV_NO_POINT, cov, cov_calib, cov_status, meas_cov);
    return;
  }
  // pass 2: sum over the pairs c' <= c of M_c S[c, c'] M_c'^T, with its transpose for c' < c
  double calib[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (cam_cov) {
    for (int32_t c = 0; c < n_cams; ++c) {
      const int32_t np_c = cam_np[c];
      if (np_c == 0) continue;
      const int64_t off_c = cam_off[c];
      if (off_c < 0) continue;
      const bool used_c = traj_cov_uses(c, n_slots, s, true, cam_posed, xy, view_state);
      if (!traj_cov_any(used_c)) continue;
      double Mc[3][MAX_NC], A2[2][MAX_NC], B2[2][3], W[3][3];
      traj_cov_jacobians(tabs[c], X, Y, Z, A2, B2);
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int j = 0; j < MAX_NC; ++j) {
        double m[3];
        traj_cov_gain_column(A2, B2, used_c, L, j, m);
        Mc[0][j] = m[0]; Mc[1][j] = m[1]; Mc[2][j] = m[2];
      }
      for (int32_t c2 = 0; c2 < c; ++c2) {
        const int32_t np_2 = cam_np[c2];
        if (np_2 == 0) continue;
        const int64_t off_2 = cam_off[c2];
        if (off_2 < 0) continue;
        const bool used_2 = traj_cov_uses(c2, n_slots, s, true, cam_posed, xy, view_state);
        if (!traj_cov_any(used_c && used_2)) continue;
        traj_cov_jacobians(tabs[c2], X, Y, Z, A2, B2);
        traj_cov_pair<false>(Mc, A2, B2, used_2, L, cam_cov, ncp, off_c, np_c == 9, off_2, np_2 == 9, W);
        calib[0] += 2.0 * W[0][0];
        calib[1] += W[0][1] + W[1][0];
        calib[2] += W[0][2] + W[2][0];
        calib[3] += 2.0 * W[1][1];
        calib[4] += W[1][2] + W[2][1];
        calib[5] += 2.0 * W[2][2];
      }
      traj_cov_pair<true>(Mc, A2, B2, true, L, cam_cov, ncp, off_c, np_c == 9, off_c, np_c == 9, W);
      calib[0] += W[0][0];
      calib[1] += 0.5 * (W[0][1] + W[1][0]);
      calib[2] += 0.5 * (W[0][2] + W[2][0]);
      calib[3] += W[1][1];
      calib[4] += 0.5 * (W[1][2] + W[2][1]);
      calib[5] += W[2][2];
    }
  }
  // the noise term last (nothing of it is live across the pair pass): V^-1, column by column
  double I0[3], I1[3], I2[3], w[3];
  const double e0[3] = {1.0, 0.0, 0.0}, e1[3] = {0.0, 1.0, 0.0}, e2[3] = {0.0, 0.0, 1.0};
  chol3_fwd(L, e0, w); chol3_bwd(L, w, I0);
  chol3_fwd(L, e1, w); chol3_bwd(L, w, I1);
  chol3_fwd(L, e2, w); chol3_bwd(L, w, I2);
  const double s2 = sigma_px * sigma_px;
  const double noise[6] = {s2 * I0[0], s2 * 0.5 * (I0[1] + I1[0]), s2 * 0.5 * (I0[2] + I2[0]), s2 * I1[1], s2 * 0.5 * (I1[2] + I2[1]), s2 * I2[2]};
  double total[6], sum = 0.0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < 6; ++i) {
    total[i] = noise[i] + calib[i];
    sum += total[i];
  }
  if (!refine_finite(sum)) {  // (a NaN row never goes out as "ok")
    traj_cov_store(s, none, none, none, COV_NOT_COMPUTABLE, cov, cov_calib, cov_status, meas_cov);
    return;
  }
  traj_cov_store(s, total, cam_cov ? calib : none, noise, COV_OK, cov, cov_calib, cov_status, meas_cov);
}

// after k_traj_fill3d: a cell the 3-D fill added has no covariance of its own (its row is NaN already: it had no point)
CBA_HD void traj_cov_mark_filled(int64_t s, const uint8_t* valid, uint8_t* cov_status) {
  if (valid[s] == 2) cov_status[s] = COV_NOT_COMPUTABLE;
}

}  // namespace cba

// ---- host side: the tables and the checks of the call ------------------------------------------------------------------------------
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

namespace cba {

// bytes of the device buffers the covariance adds: cov and cov_status per slot, cov_calib where it is returned, CamTab + width +
// offset per camera, cam_cov
inline double traj_cov_device_bytes(const cba_traj_desc* d, const cba_traj_uncertainty* u, const cba_traj_cov_out* o) {
  const double slots = (double)d->n_frames * (double)d->n_traj;
  double bytes = slots * 49.0 + (double)d->n_cams * 396.0;
  if (u->cam_cov) bytes += (double)u->ncp * (double)u->ncp * 8.0;
  if (o->cov_calib) bytes += slots * 48.0;
  return bytes;
}

// 0, or -1 (CBA_ERR_INVALID) / -4 (CBA_ERR_UNSUPPORTED) with `msg` naming the field.  d has passed traj_validate.
inline int traj_cov_validate(const cba_traj_desc* d, const cba_traj_uncertainty* u, const cba_traj_cov_out* o, std::string& msg) {
  const std::string what = "cba_reconstruct_trajectories_uncertain: ";
  if (!u || !o) { msg = what + "uncertainty: null argument"; return -1; }
  if (!std::isfinite(u->sigma_px) || !(u->sigma_px > 0.0)) { msg = what + "sigma_px must be finite and positive, got " + std::to_string(u->sigma_px); return -1; }
  if (d->n_rows == 0) return 0;
  if (!u->cam_nparams || !u->cam_const || !u->cam_x || (u->cam_cov && !u->cam_offset)) { msg = what + "uncertainty: null argument"; return -1; }
  for (int32_t c = 0; c < d->n_cams; ++c) {
    if (!d->cam_posed[c]) continue;
    const int32_t np = u->cam_nparams[c];
    if (np != 6 && np != 9) { msg = what + "camera " + std::to_string(c) + ": cam_nparams must be 6 or 9, got " + std::to_string(np); return -1; }
    if (np == 9 && d->cam_model[c] == MODEL_FISHEYE4) {
      msg = what + "camera " + std::to_string(c) + ": cam_nparams: a fisheye camera has no free intrinsics (9 parameters)";
      return -4;
    }
  }
  if (!u->cam_cov) return 0;
  if (u->ncp < 0) { msg = what + "ncp must not be negative, got " + std::to_string(u->ncp); return -1; }
  std::vector<std::pair<int64_t, int32_t>> blocks;  // (offset, camera)
  for (int32_t c = 0; c < d->n_cams; ++c) {
    if (!d->cam_posed[c]) continue;
    const int64_t off = u->cam_offset[c], np = u->cam_nparams[c];
    if (off == -1) continue;
    if (off < -1 || off > u->ncp - np) {
      msg = what + "camera " + std::to_string(c) + ": cam_offset " + std::to_string(off) + " puts its " + std::to_string(np) + " rows outside [0, " +
            std::to_string(u->ncp) + ")";
      return -1;
    }
    blocks.emplace_back(off, c);
  }
  std::sort(blocks.begin(), blocks.end());
  for (size_t i = 1; i < blocks.size(); ++i)
    if (blocks[i - 1].first + u->cam_nparams[blocks[i - 1].second] > blocks[i].first) {
      msg = what + "camera " + std::to_string(blocks[i].second) + ": cam_offset " + std::to_string(blocks[i].first) + " overlaps the rows of camera " +
            std::to_string(blocks[i - 1].second);
      return -1;
    }
  const int64_t n = u->ncp;
  double top = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    for (int64_t j = 0; j < n; ++j)
      if (!std::isfinite(u->cam_cov[i * n + j])) { msg = what + "cam_cov[" + std::to_string(i) + "][" + std::to_string(j) + "] is not finite"; return -1; }
    top = std::max(top, std::fabs(u->cam_cov[i * n + i]));
  }
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = 0; j < i; ++j)
      if (std::fabs(u->cam_cov[i * n + j] - u->cam_cov[j * n + i]) > 1e-12 * top) {
        msg = what + "cam_cov is not symmetric at [" + std::to_string(i) + "][" + std::to_string(j) + "]";
        return -1;
      }
  return 0;
}

// The checks of the call it extends (refine null: the plain one), those above, and the memory check with all buffers counted.
// memory <= 0: not checked.
inline int traj_uncertain_validate(const cba_traj_desc* d, const cba_traj_refine* r, const cba_traj_uncertainty* u, const cba_traj_cov_out* o,
                                   double memory, std::string& msg) {
  int rc = traj_validate(d, 0.0, msg);
  if (rc) return rc;
  if (r && (rc = traj_refine_validate(r, msg))) return rc;
  rc = traj_cov_validate(d, u, o, msg);
  if (rc) return rc;
  const double bytes = traj_device_bytes(d) + (r ? traj_refine_device_bytes(d) : 0.0) + traj_cov_device_bytes(d, u, o);
  if (d->n_rows > 0 && memory > 0.0 && bytes > memory) {
    msg = "cba_reconstruct_trajectories_uncertain: the grid of " + std::to_string(d->n_cams) + " cameras x " + std::to_string(d->n_frames) +
          " frames x " + std::to_string(d->n_traj) + " trajectories with its covariances needs " + std::to_string((long long)bytes) +
          " bytes of device memory, " + std::to_string((long long)memory) + " are available";
    return -4;
  }
  return 0;
}

// What k_traj_cov reads per camera, from a description that has passed the checks: cam_prepare of the posed cameras (an unposed one:
// zeros, width 0), and the offsets (-1 throughout without cam_cov).
inline void traj_cov_tables(const cba_traj_desc* d, const cba_traj_uncertainty* u, std::vector<CamTab>& tabs, std::vector<int32_t>& np,
                            std::vector<int64_t>& off) {
  const size_t n = (size_t)d->n_cams;
  tabs.assign(n, CamTab{});
  np.assign(n, 0);
  off.assign(n, -1);
  for (size_t c = 0; c < n; ++c) {
    if (!d->cam_posed[c]) continue;
    np[c] = u->cam_nparams[c];
    if (u->cam_cov) off[c] = u->cam_offset[c];
    cam_prepare(u->cam_x + 9 * c, u->cam_const + CAM_CONST_STRIDE * c, d->cam_model[c], np[c], &tabs[c]);
  }
}

}  // namespace cba
