// CPU harness around caliscope_amd/csrc/pnp_math.h — TEST INFRASTRUCTURE (built by g++ in tests/pnp_native.py).
// It runs the per-view PnP and the pair RMSE of the pose bootstrap with the arithmetic the kernels of pose_lib.hip inline,
// so that the non-GPU suite can check them against scipy and drive caliscope_amd/pose_network.py through its `_pnp` hook.
// It is not a CPU fallback: nothing in caliscope_amd/ loads it.
#include <cstdint>

#include "pnp_math.h"

extern "C" {

// one view, normalised image points: R_out [9] row-major, t_out [3]
int ph_pnp_view(const double* obj, const double* uv, int n, int min_points, int f32, double* R_out, double* t_out, double* rmse) {
  return cba::pnp_view(obj, uv, n, min_points, f32, R_out, t_out, rmse);
}

// what cba_pose_pnp_batch computes, view after view: undistortion with the view's camera, then pnp_view
void ph_pnp_batch(int64_t n_views, const int64_t* view_start, const int32_t* view_cam, const int32_t* cam_model, const double* cam_intr,
                  const double* obs_xy, const double* obs_obj, int min_points, int f32, double* und, double* pose_out, double* rmse_out,
                  int32_t* status_out) {
  for (int64_t v = 0; v < n_views; ++v) {
    const int64_t a = view_start[v], b = view_start[v + 1];
    const int c = view_cam[v];
    for (int64_t i = a; i < b; ++i) cba::undistort_one(cam_model[c], cam_intr + 9 * c, obs_xy[2 * i], obs_xy[2 * i + 1], f32, &und[2 * i], &und[2 * i + 1]);
    status_out[v] = cba::pnp_view(obs_obj + 3 * a, und + 2 * a, (int)(b - a), min_points, f32, pose_out + 12 * v, pose_out + 12 * v + 9, rmse_out + v);
  }
}

// what cba_pose_pair_rmse computes (summed in observation order here)
void ph_pair_rmse(int64_t n_pairs, const double* pair_pose, const int64_t* pair_start, const double* obs_a, const double* obs_b, double* rmse_out,
                  int64_t* count_out) {
  for (int64_t p = 0; p < n_pairs; ++p) {
    const int64_t a = pair_start[p], b = pair_start[p + 1];
    double s = 0.0;
    for (int64_t i = a; i < b; ++i) s += cba::pair_obs_sq(pair_pose + 12 * p, obs_a[2 * i], obs_a[2 * i + 1], obs_b[2 * i], obs_b[2 * i + 1]);
    count_out[p] = b - a;
    rmse_out[p] = (b > a) ? sqrt(s / (2.0 * (double)(b - a))) : 0.0;
  }
}

}
