// CPU harness around caliscope_amd/csrc/intrinsic_math.h — TEST INFRASTRUCTURE (built by g++ in tests/intrinsic_native.py).
// It runs the intrinsic calibration with the arithmetic k_intrinsics of pose_lib.hip inlines, views summed in the order of the
// kernel's reduction tree, so that the non-GPU suite can check it against scipy and drive caliscope_amd/calibrate_intrinsics.py
// through its `_solver` hook.  It is not a CPU fallback: nothing in caliscope_amd/ loads it.
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#include "intrinsic_math.h"

using namespace cba;

namespace {

constexpr int NT = EPI_REDUCE_NT;

// the functor of intr_calibrate over the views of one camera; "thread" tid takes views tid, tid + NT, ... of the camera's list
template <int MODEL>
struct IntrSumHost {
  const int64_t* views; int64_t nv;
  const int64_t* view_start; const double* xy; const double* obj; int f32;
  const double* pnp_pose; const int32_t* pnp_status;
  double* work; int32_t* vstat; double* pose_out; double* view_rmse;

  template <int K, class Item>
  void tree(Item item, double* out) {
    std::vector<double> part((size_t)NT * K, 0.0);
    for (int tid = 0; tid < NT; ++tid)
      for (int64_t q = tid; q < nv; q += NT) item(views[q], &part[(size_t)tid * K]);
    for (int st = NT / 2; st > 0; st >>= 1)
      for (int tid = 0; tid < st; ++tid)
        for (int k = 0; k < K; ++k) part[(size_t)tid * K + k] += part[(size_t)(tid + st) * K + k];
    for (int k = 0; k < K; ++k) out[k] = part[k];
  }
  int n_of(int64_t v) const { return (int)(view_start[v + 1] - view_start[v]); }
  const double* o(int64_t v) const { return obj + 3 * view_start[v]; }
  const double* p(int64_t v) const { return xy + 2 * view_start[v]; }

  void screen(const double* in0, double* out) {
    tree<2>([&](int64_t v, double* acc) {
      const int st = intr_view_screen<MODEL>(in0, o(v), p(v), n_of(v), f32, pnp_status[v], pnp_pose + 12 * v, work + v * INTR_WORK);
      vstat[v] = st;
      if (st == PNP_OK) { acc[0] += 1.0; acc[1] += (double)n_of(v); }
    }, out);
  }
  void reduce(const double* in, double mu, double* out) {
    tree<IntrDim<MODEL>::NSUM>([&](int64_t v, double* acc) {
      if (vstat[v] == PNP_OK) intr_view_reduce<MODEL>(in, mu, o(v), p(v), n_of(v), f32, work + v * INTR_WORK, acc);
    }, out);
  }
  void trial(const double* in_new, const double* di, double* out) {
    tree<2>([&](int64_t v, double* acc) {
      if (vstat[v] == PNP_OK) intr_view_trial<MODEL>(in_new, di, o(v), p(v), n_of(v), f32, work + v * INTR_WORK, acc);
    }, out);
  }
  void accept() {
    for (int64_t q = 0; q < nv; ++q)
      if (vstat[views[q]] == PNP_OK) intr_view_accept(work + views[q] * INTR_WORK);
  }
  void finish(const double* in, bool ok) {
    for (int64_t q = 0; q < nv; ++q) {
      const int64_t v = views[q];
      intr_view_finish<MODEL>(in, ok, o(v), p(v), n_of(v), f32, vstat[v], work + v * INTR_WORK, pose_out + 12 * v, view_rmse + v);
    }
  }
};

}  // namespace

extern "C" {

int ih_work_stride() { return INTR_WORK; }

void ih_start(int model, double width, double height, double* in9) { intr_start(model, width, height, in9); }

// residual and Jacobian of one corner: e[2], J[2][6 + NI] (pose columns w, t first, then the intrinsics); returns "in front"
int ih_point(int model, const double* in, const double* R, const double* t, const double* X, const double* u, double* e, double* J) {
  double jx[6], jy[6], ix[9], iy[9];
  const int ni = model == MODEL_FISHEYE4 ? 8 : 9;
  const bool front = model == MODEL_FISHEYE4 ? intr_point<MODEL_FISHEYE4, true>(in, R, t, X, u, e, jx, jy, ix, iy)
                                              : intr_point<MODEL_PINHOLE_BC5, true>(in, R, t, X, u, e, jx, jy, ix, iy);
  for (int k = 0; k < 6; ++k) { J[k] = jx[k]; J[6 + ni + k] = jy[k]; }
  for (int k = 0; k < ni; ++k) { J[6 + k] = ix[k]; J[6 + ni + 6 + k] = iy[k]; }
  return front ? 1 : 0;
}

// what cba_pose_intrinsics_batch computes, camera after camera (cam_start: [n_cams][9] or null; a row whose fx is not > 0 takes
// the default start)
void ih_intrinsics_batch(int32_t n_cams, const int32_t* cam_model, const double* cam_size, const double* cam_start, int64_t n_views,
                         const int64_t* view_start, const int32_t* view_cam, const double* obs_xy, const double* obs_obj, int f32,
                         int max_iter, double* intr_out, double* rmse_out, int32_t* status_out, int32_t* iters_out, double* pose_out,
                         double* view_rmse_out, int32_t* view_status_out) {
  const int64_t n_obs = n_views > 0 ? view_start[n_views] : 0;
  std::vector<double> start((size_t)n_cams * 9), und((size_t)n_obs * 2), pnp_pose((size_t)n_views * 12), pnp_rmse(n_views),
      work((size_t)n_views * INTR_WORK, 0.0);
  std::vector<int32_t> pnp_status(n_views);
  for (int c = 0; c < n_cams; ++c) {
    if (cam_start && cam_start[9 * c] > 0.0) std::copy(cam_start + 9 * c, cam_start + 9 * c + 9, start.begin() + 9 * c);
    else intr_start(cam_model[c], cam_size[2 * c], cam_size[2 * c + 1], &start[9 * c]);
  }
  for (int64_t v = 0; v < n_views; ++v) {
    const int64_t a = view_start[v], b = view_start[v + 1];
    const int c = view_cam[v];
    for (int64_t i = a; i < b; ++i) undistort_one(cam_model[c], &start[9 * c], obs_xy[2 * i], obs_xy[2 * i + 1], f32, &und[2 * i], &und[2 * i + 1]);
    pnp_status[v] = pnp_view(obs_obj + 3 * a, und.data() + 2 * a, (int)(b - a), INTR_MIN_POINTS, f32, &pnp_pose[12 * v], &pnp_pose[12 * v + 9], &pnp_rmse[v]);
  }
  // views by corner count (stable), then the list of each camera
  std::vector<int64_t> order(n_views);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return view_start[x + 1] - view_start[x] < view_start[y + 1] - view_start[y]; });
  for (int c = 0; c < n_cams; ++c) {
    std::vector<int64_t> mine;
    for (int64_t v : order)
      if (view_cam[v] == c) mine.push_back(v);
    double in9[9];
    std::copy(start.begin() + 9 * c, start.begin() + 9 * c + 9, in9);
    int it = 0;
    if (cam_model[c] == MODEL_FISHEYE4) {
      IntrSumHost<MODEL_FISHEYE4> sum{mine.data(), (int64_t)mine.size(), view_start, obs_xy, obs_obj, f32, pnp_pose.data(), pnp_status.data(),
                                      work.data(), view_status_out, pose_out, view_rmse_out};
      status_out[c] = intr_calibrate<MODEL_FISHEYE4>(sum, in9, max_iter, rmse_out + c, &it);
    } else {
      IntrSumHost<MODEL_PINHOLE_BC5> sum{mine.data(), (int64_t)mine.size(), view_start, obs_xy, obs_obj, f32, pnp_pose.data(), pnp_status.data(),
                                         work.data(), view_status_out, pose_out, view_rmse_out};
      status_out[c] = intr_calibrate<MODEL_PINHOLE_BC5>(sum, in9, max_iter, rmse_out + c, &it);
    }
    iters_out[c] = it;
    std::copy(in9, in9 + 9, intr_out + 9 * c);
  }
}

}
