// CPU harness around caliscope_amd/csrc/trajectory_cov_math.h, trajectory_refine_math.h and trajectory_math.h — TEST INFRASTRUCTURE
// (built by g++ in tests/trajectory_cov_native.py).  It evaluates cba_reconstruct_trajectories_uncertain with the checks, the table
// preparation and the per-thread routines that trajectory_lib.hip uses, the kernels' threads one after the other in index order (a
// "wave" is one slot here).  It is not a CPU fallback: nothing in caliscope_amd/ loads it.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "trajectory_cov_math.h"

using namespace cba;

namespace {
std::string g_error;
}

extern "C" {

const char* tch_last_error() { return g_error.c_str(); }

// k_traj_cov alone: the threads of all slots on grids given by hand (xy[n_cams][n_slots][2], xyz[n_slots][3], valid[n_slots] as they
// are in front of the 3-D fill; view_state[n_cams][n_slots] or null for the plain call), the tables prepared as the call prepares
// them.  No host check stands in front.
void tch_cov_grid(int32_t n_cams, int64_t n_slots, const uint8_t* cam_posed, const int32_t* cam_model, const cba_traj_uncertainty* u, const double* xy,
                  const uint8_t* view_state, const uint8_t* valid, const double* xyz, cba_traj_cov_out* co) {
  cba_traj_desc d{};
  d.n_cams = n_cams;
  d.cam_posed = cam_posed;
  d.cam_model = cam_model;
  std::vector<CamTab> tabs;
  std::vector<int32_t> cam_np;
  std::vector<int64_t> cam_off;
  traj_cov_tables(&d, u, tabs, cam_np, cam_off);
  for (int64_t s = 0; s < n_slots; ++s)
    traj_cov_slot(n_cams, n_slots, s, tabs.data(), cam_np.data(), cam_off.data(), u->cam_cov, u->cam_cov ? u->ncp : 0, u->sigma_px, cam_posed, xy,
                  view_state, valid, xyz, co->cov, co->cov_calib, co->cov_status);
}

// cba_reconstruct_trajectories_uncertain on the host: 0, -1 (invalid) or -4 (unsupported) with tch_last_error() set.  r and q null:
// the plain call; otherwise every pointer of `q` must be given.  Every pointer of `co` but cov_calib must be given.
int tch_reconstruct_trajectories_uncertain(const cba_traj_desc* d, const cba_traj_refine* r, const cba_traj_uncertainty* u, cba_traj_out* out,
                                           cba_traj_quality* q, cba_traj_cov_out* co) {
  const std::string what = "cba_reconstruct_trajectories_uncertain";
  if (!d || !out || !u || !co) { g_error = what + ": null argument"; return -1; }
  if ((r == nullptr) != (q == nullptr)) { g_error = what + ": quality goes with refine, and with it alone"; return -1; }
  const int rc = traj_uncertain_validate(d, r, u, co, (double)d->memory_limit, g_error);
  if (rc) return rc;
  const int32_t n_cams = d->n_cams;
  const int64_t n_frames = d->n_frames, n_traj = d->n_traj, n_slots = n_frames * n_traj;
  const size_t cells = (size_t)n_cams * (size_t)n_slots;
  const double nan = traj_nan();
  std::vector<double> xy(cells * 2, nan), ft(cells, nan), frame((size_t)n_frames, nan), xyz((size_t)n_slots * 3, nan), time((size_t)n_slots, nan);
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
                    xy.data(), q ? q->view_state : nullptr, valid.data(), xyz.data(), co->cov, co->cov_calib, co->cov_status);
    for (int64_t s = 0; s < n_slots; ++s) traj_fill3d_cell(n_frames, n_traj, s, d->xyz_gap, valid.data(), xyz.data(), time.data());
    for (int64_t s = 0; d->xyz_gap > 0 && s < n_slots; ++s) traj_cov_mark_filled(s, valid.data(), co->cov_status);
    if (d->filter_b) {
      std::vector<double> scratch((size_t)(n_frames + 2 * traj_pad(d->filter_order)) * (size_t)n_traj * 3, 0.0);
      for (int64_t t = 0; t < 3 * n_traj; ++t)
        traj_filtfilt_thread(n_frames, n_traj, t, d->filter_order, d->filter_b, d->filter_a, d->filter_zi, valid.data(), xyz.data(), scratch.data());
    }
  }
  if (out->xyz) std::memcpy(out->xyz, xyz.data(), xyz.size() * sizeof(double));
  if (out->valid) std::memcpy(out->valid, valid.data(), valid.size());
  if (out->slot_time) std::memcpy(out->slot_time, time.data(), time.size() * sizeof(double));
  if (out->frame_time) std::memcpy(out->frame_time, frame.data(), frame.size() * sizeof(double));
  if (out->xy_filled) std::memcpy(out->xy_filled, xy.data(), xy.size() * sizeof(double));
  if (out->ft_filled) std::memcpy(out->ft_filled, ft.data(), ft.size() * sizeof(double));
  return 0;
}

}
