// CPU harness around caliscope_amd/csrc/trajectory_math.h — TEST INFRASTRUCTURE (built by g++ in tests/trajectory_native.py).
// It evaluates cba_reconstruct_trajectories with the checks and the per-thread routines that trajectory_lib.hip uses; the kernels'
// threads run one after the other in index order, so that the non-GPU suite can check the fills and the filter against pandas and
// scipy and drive caliscope_amd.reconstruction through its `_solver` hook.  The triangulation is the same routine built without
// fused multiply-adds: its points differ from the device's in the last bits.  It is not a CPU fallback: nothing in caliscope_amd/
// loads it.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "trajectory_math.h"

using namespace cba;

namespace {
std::string g_error;
}

extern "C" {

const char* th_last_error() { return g_error.c_str(); }

double th_lerp(double left, double right, int64_t i, int64_t k) { return traj_lerp(left, right, i, k); }

// scipy.signal.filtfilt(b, a, x) of one signal of n samples (n > 3 (order + 1)) by traj_filtfilt_thread: a grid of one trajectory
// whose x coordinate is the signal; returns 0, or -1 when the routine leaves the signal alone
int th_filtfilt(const double* x, int64_t n, int order, const double* b, const double* a, const double* zi, double* y) {
  std::vector<double> xyz((size_t)n * 3, 0.0), scratch((size_t)(n + 2 * traj_pad(order)) * 3, 0.0);
  std::vector<uint8_t> valid((size_t)n, 1);
  for (int64_t i = 0; i < n; ++i) xyz[(size_t)i * 3] = x[i];
  traj_filtfilt_thread(n, 1, 0, order, b, a, zi, valid.data(), xyz.data(), scratch.data());
  for (int64_t i = 0; i < n; ++i) y[i] = xyz[(size_t)i * 3];
  return n <= 3 * (int64_t)order || n <= traj_pad(order) ? -1 : 0;
}

// The 3-D stages alone on a given dense grid (xyz[n_slots][3], time[n_slots], valid[n_slots], all in place): k_traj_fill3d, then
// k_traj_filtfilt when b is given.
void th_world_stages(int64_t n_frames, int64_t n_traj, int xyz_gap, int order, const double* b, const double* a, const double* zi, uint8_t* valid,
                     double* xyz, double* time) {
  const int64_t n_slots = n_frames * n_traj;
  for (int64_t s = 0; s < n_slots; ++s) traj_fill3d_cell(n_frames, n_traj, s, xyz_gap, valid, xyz, time);
  if (!b) return;
  std::vector<double> scratch((size_t)(n_frames + 2 * traj_pad(order)) * (size_t)n_traj * 3, 0.0);
  for (int64_t t = 0; t < 3 * n_traj; ++t) traj_filtfilt_thread(n_frames, n_traj, t, order, b, a, zi, valid, xyz, scratch.data());
}

// cba_reconstruct_trajectories on the host: 0, -1 (invalid) or -4 (unsupported) with th_last_error() set
int th_reconstruct_trajectories(const cba_traj_desc* d, cba_traj_out* out) {
  if (!d || !out) { g_error = "cba_reconstruct_trajectories: null argument"; return -1; }
  const int rc = traj_validate(d, (double)d->memory_limit, g_error);
  if (rc) return rc;
  const int32_t n_cams = d->n_cams;
  const int64_t n_frames = d->n_frames, n_traj = d->n_traj, n_slots = n_frames * n_traj;
  const size_t cells = (size_t)n_cams * (size_t)n_slots;
  const double nan = traj_nan();
  std::vector<double> xy(cells * 2, nan), ft(cells, nan), frame((size_t)n_frames, nan), xyz((size_t)n_slots * 3, nan), time((size_t)n_slots, nan);
  std::vector<uint8_t> valid((size_t)n_slots, 0);
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
    th_world_stages(n_frames, n_traj, d->xyz_gap, d->filter_order, d->filter_b, d->filter_a, d->filter_zi, valid.data(), xyz.data(), time.data());
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
