// CPU harness around caliscope_amd/csrc/trajectory_smooth_math.h with trajectory_cov_math.h, trajectory_refine_math.h and
// trajectory_math.h — TEST INFRASTRUCTURE (built by g++ in tests/trajectory_smooth_native.py).  It evaluates cba_smooth_trajectories and
// cba_reconstruct_trajectories_smoothed with the checks and the per-thread routines that trajectory_lib.hip uses, the kernels' threads
// one after the other in index order.  It is not a CPU fallback: nothing in caliscope_amd/ loads it.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "trajectory_smooth_math.h"

using namespace cba;

namespace {
std::string g_error;

// k_traj_smooth over all trajectories on host arrays, into the buffers of `o` that are given (the others into temporaries)
void smooth_all(int64_t n_frames, int64_t n_traj, const double* xyz, const double* meas_cov, const uint8_t* measured, const SmoothModel& model,
                cba_traj_smooth_out* o) {
  const size_t n = (size_t)(n_frames * n_traj);
  const double nan = traj_nan();
  std::vector<double> pos(n * 3, nan), vel(n * 3, nan), pos_cov(n * 6, nan), vel_cov(n * 6, nan), nis(n, nan), park(n * SMOOTH_PARK, nan);
  std::vector<uint8_t> status(n, 0);
  for (int64_t j = 0; j < n_traj; ++j)
    traj_smooth_thread(n_frames, n_traj, j, xyz, meas_cov, measured, model, park.data(), pos.data(), vel.data(), pos_cov.data(), vel_cov.data(),
                       nis.data(), status.data());
  if (o->pos) std::memcpy(o->pos, pos.data(), pos.size() * sizeof(double));
  if (o->vel) std::memcpy(o->vel, vel.data(), vel.size() * sizeof(double));
  if (o->pos_cov) std::memcpy(o->pos_cov, pos_cov.data(), pos_cov.size() * sizeof(double));
  if (o->vel_cov) std::memcpy(o->vel_cov, vel_cov.data(), vel_cov.size() * sizeof(double));
  if (o->nis) std::memcpy(o->nis, nis.data(), nis.size() * sizeof(double));
  if (o->status) std::memcpy(o->status, status.data(), status.size());
}
}  // namespace

extern "C" {

const char* tsh_last_error() { return g_error.c_str(); }

// cba_smooth_trajectories on the host: 0, -1 (invalid) or -4 (unsupported) with tsh_last_error() set
int tsh_smooth_trajectories(const cba_smooth_desc* d, cba_traj_smooth_out* out) {
  if (!d || !out) { g_error = "cba_smooth_trajectories: null argument"; return -1; }
  bool any = false;
  const int rc = traj_smooth_validate(d, (double)d->memory_limit, g_error, &any);
  if (rc) return rc;
  // (without a measured slot no thread writes anything: the rows stay NaN / 0 as the call returns them without a launch)
  smooth_all(d->n_frames, d->n_traj, d->xyz, d->meas_cov, d->measured, smooth_model(d->fps, d->accel_density, d->velocity_prior_std, d->max_gap), out);
  return 0;
}

// the thread body alone, no check in front: for arrays the device was given
void tsh_smooth_threads(const cba_smooth_desc* d, cba_traj_smooth_out* out) {
  smooth_all(d->n_frames, d->n_traj, d->xyz, d->meas_cov, d->measured, smooth_model(d->fps, d->accel_density, d->velocity_prior_std, d->max_gap), out);
}

// cba_reconstruct_trajectories_smoothed on the host.  r and q null: the plain call; otherwise every pointer of `q` must be given.  Every
// pointer of `co` but cov_calib must be given.
int tsh_reconstruct_trajectories_smoothed(const cba_traj_desc* d, const cba_traj_refine* r, const cba_traj_uncertainty* u, const cba_traj_smoother* sm,
                                          cba_traj_out* out, cba_traj_quality* q, cba_traj_cov_out* co, cba_traj_smooth_out* so) {
  const std::string what = "cba_reconstruct_trajectories_smoothed";
  if (!d || !out) { g_error = what + ": null argument"; return -1; }
  if (!u || !co) { g_error = what + ": uncertainty: null argument (the smoother weights a sample by its covariance)"; return -1; }
  if (!sm || !so) { g_error = what + ": smoother: null argument"; return -1; }
  if ((r == nullptr) != (q == nullptr)) { g_error = what + ": quality goes with refine, and with it alone"; return -1; }
  const int rc = traj_smoothed_validate(d, r, u, co, sm, so, (double)d->memory_limit, g_error);
  if (rc) return rc;
  const int32_t n_cams = d->n_cams;
  const int64_t n_frames = d->n_frames, n_traj = d->n_traj, n_slots = n_frames * n_traj;
  const size_t cells = (size_t)n_cams * (size_t)n_slots;
  const double nan = traj_nan();
  std::vector<double> xy(cells * 2, nan), ft(cells, nan), frame((size_t)n_frames, nan), xyz((size_t)n_slots * 3, nan), time((size_t)n_slots, nan);
  std::vector<double> meas((size_t)n_slots * 6, nan);
  std::vector<uint8_t> valid((size_t)n_slots, 0);
  if (q) {
    std::memset(q->view_state, 0, cells);
    for (int64_t s = 0; s < n_slots; ++s) {
      q->views[s] = q->iterations[s] = 0;
      q->rms_px[s] = q->max_px[s] = nan;
      q->status[s] = 0;
    }
  }
  for (int64_t s = 0; s < n_slots; ++s) {
    for (int i = 0; i < 6; ++i) {
      co->cov[6 * s + i] = nan;
      if (co->cov_calib) co->cov_calib[6 * s + i] = nan;
    }
    co->cov_status[s] = COV_NO_POINT;
  }
  if (d->n_rows > 0) {
    for (int64_t i = 0; i < d->n_rows; ++i)
      traj_fill2d_row(d->n_rows, n_traj, n_slots, i, d->row_cam, d->row_slot, d->row_xy, d->row_time, d->xy_gap, xy.data(), ft.data());
    for (int64_t f = 0; f < n_frames; ++f) frame[(size_t)f] = traj_frame_mean(n_cams, n_traj, n_slots, f, ft.data());
    for (int64_t s = 0; s < n_slots; ++s) {
      const int views = traj_triangulate_slot(n_cams, n_slots, s, d->cam_posed, d->cam_model, d->cam_intr, d->cam_P, xy.data(), d->float32_io ? 1 : 0,
                                              &xyz[(size_t)s * 3]);
      valid[(size_t)s] = views >= 2 ? 1 : 0;
      time[(size_t)s] = views >= 2 ? frame[(size_t)(s / n_traj)] : nan;
    }
    for (int64_t s = 0; r && s < n_slots; ++s)
      traj_refine_slot(n_cams, n_slots, s, d->cam_posed, d->cam_model, d->cam_intr, d->cam_P, xy.data(), r->loss, r->f_scale, r->max_iter, r->reject_px,
                       r->max_reject, r->min_views, valid.data(), xyz.data(), q->view_state, q->views, q->rms_px, q->max_px, q->iterations, q->status);
    std::vector<CamTab> tabs;
    std::vector<int32_t> cam_np;
    std::vector<int64_t> cam_off;
    traj_cov_tables(d, u, tabs, cam_np, cam_off);
    for (int64_t s = 0; s < n_slots; ++s)
      traj_cov_slot(n_cams, n_slots, s, tabs.data(), cam_np.data(), cam_off.data(), u->cam_cov, u->cam_cov ? u->ncp : 0, u->sigma_px, d->cam_posed,
                    xy.data(), q ? q->view_state : nullptr, valid.data(), xyz.data(), co->cov, co->cov_calib, co->cov_status, meas.data());
  }
  // (the rows without a result stay NaN / 0, with or without rows in the call)
  smooth_all(n_frames, n_traj, xyz.data(), meas.data(), co->cov_status, smooth_model(sm->fps, sm->accel_density, sm->velocity_prior_std, sm->max_gap), so);
  if (so->meas_cov) std::memcpy(so->meas_cov, meas.data(), meas.size() * sizeof(double));
  if (out->xyz) std::memcpy(out->xyz, xyz.data(), xyz.size() * sizeof(double));
  if (out->valid) std::memcpy(out->valid, valid.data(), valid.size());
  if (out->slot_time) std::memcpy(out->slot_time, time.data(), time.size() * sizeof(double));
  if (out->frame_time) std::memcpy(out->frame_time, frame.data(), frame.size() * sizeof(double));
  if (out->xy_filled) std::memcpy(out->xy_filled, xy.data(), xy.size() * sizeof(double));
  if (out->ft_filled) std::memcpy(out->ft_filled, ft.data(), ft.size() * sizeof(double));
  return 0;
}

}
