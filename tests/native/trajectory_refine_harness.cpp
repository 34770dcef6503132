// CPU harness around caliscope_amd/csrc/trajectory_refine_math.h and trajectory_math.h — TEST INFRASTRUCTURE (built by g++ in
// tests/trajectory_refine_native.py).  It evaluates cba_reconstruct_trajectories_refined with the checks and the per-thread routines
// that trajectory_lib.hip uses, the kernels' threads one after the other in index order, and k_traj_refine alone on a grid given by
// hand.  It is not a CPU fallback: nothing in caliscope_amd/ loads it.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "trajectory_refine_math.h"

using namespace cba;

namespace {
std::string g_error;
}

extern "C" {

const char* trh_last_error() { return g_error.c_str(); }

// k_traj_refine alone: the threads of all slots on the given grids (xy[n_cams][n_slots][2], xyz[n_slots][3] in place), with the options
// handed to the routine as they are — no host check stands in front (min_views = 1 gets through).
void trh_refine_grid(int32_t n_cams, int64_t n_slots, const uint8_t* cam_posed, const int32_t* cam_model, const double* cam_intr, const double* cam_P,
                     const double* xy, const cba_traj_refine* r, const uint8_t* valid, double* xyz, cba_traj_quality* q) {
  for (int64_t s = 0; s < n_slots; ++s)
    traj_refine_slot(n_cams, n_slots, s, cam_posed, cam_model, cam_intr, cam_P, xy, r->loss, r->f_scale, r->max_iter, r->reject_px, r->max_reject,
                     r->min_views, valid, xyz, q->view_state, q->views, q->rms_px, q->max_px, q->iterations, q->status);
}

// cba_reconstruct_trajectories_refined on the host: 0, -1 (invalid) or -4 (unsupported) with trh_last_error() set.  Every pointer of
// `q` must be given.
int trh_reconstruct_trajectories_refined(const cba_traj_desc* d, const cba_traj_refine* r, cba_traj_out* out, cba_traj_quality* q) {
  if (!d || !out || !q) { g_error = "cba_reconstruct_trajectories_refined: null argument"; return -1; }
  const int rc = traj_refined_validate(d, r, (double)d->memory_limit, g_error);
  if (rc) return rc;
  const int32_t n_cams = d->n_cams;
  const int64_t n_frames = d->n_frames, n_traj = d->n_traj, n_slots = n_frames * n_traj;
  const size_t cells = (size_t)n_cams * (size_t)n_slots;
  const double nan = traj_nan();
  std::vector<double> xy(cells * 2, nan), ft(cells, nan), frame((size_t)n_frames, nan), xyz((size_t)n_slots * 3, nan), time((size_t)n_slots, nan);
  std::vector<uint8_t> valid((size_t)n_slots, 0);
  std::memset(q->view_state, 0, cells);
  for (int64_t s = 0; s < n_slots; ++s) {
    q->views[s] = q->iterations[s] = 0;
    q->rms_px[s] = q->max_px[s] = nan;
    q->status[s] = 0;
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
    trh_refine_grid(n_cams, n_slots, d->cam_posed, d->cam_model, d->cam_intr, d->cam_P, xy.data(), r, valid.data(), xyz.data(), q);
    for (int64_t s = 0; s < n_slots; ++s) traj_fill3d_cell(n_frames, n_traj, s, d->xyz_gap, valid.data(), xyz.data(), time.data());
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
