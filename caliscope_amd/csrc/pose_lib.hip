// Pose-bootstrap kernels of libcaliscope_ba.so (C ABI: include/caliscope_pose.h).  The arithmetic is pnp_math.h; this file
// holds the two launches and their host side.
//
//   k_pose_pnp        one thread per board view: undistort the view's observations (ba_math.h undistort_one, the routine
//                     of cba_triangulate) into a device buffer, then pnp_view on them.  Threads take views in the order
//                     `order` gives (views sorted by point count on the host), so that the lanes of a wave run loops of
//                     similar length; results are written at the view's own index.
//   k_pose_pair_rmse  one 256-thread workgroup per camera pair: each thread sums pair_obs_sq over a strided slice of the
//                     pair's observations, then a fixed shuffle + LDS tree: deterministic, no atomics.
//
// Both kernels are FP64 VALU with per-thread matrices of at most 66 doubles (the 11 x 11 DLT normal matrix), fully
// unrolled so that they stay in registers: hipcc -Rpass-analysis=kernel-resource-usage reports ScratchSize 0 for both.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/caliscope_pose.h"
#include "pnp_math.h"

using namespace cba;

namespace {

constexpr int POSE_BLOCK = 64;   // one wave: views differ in cost, small groups keep the tail short
constexpr int PAIR_BLOCK = 256;

__global__ void __launch_bounds__(POSE_BLOCK)
k_pose_pnp(long n_views, const long* __restrict__ order, const long* __restrict__ view_start, const int* __restrict__ view_cam,
           const int* __restrict__ cam_model, const double* __restrict__ cam_intr, const double* __restrict__ obs_xy,
           const double* __restrict__ obs_obj, int min_points, int f32, double* __restrict__ und, double* __restrict__ pose,
           double* __restrict__ rmse, int* __restrict__ status) {
  const long q = (long)blockIdx.x * POSE_BLOCK + threadIdx.x;
  if (q >= n_views) return;
  const long v = order[q];
  const long a = view_start[v], b = view_start[v + 1];
  const int c = view_cam[v];
  const int model = cam_model[c];
  const double* in9 = cam_intr + 9 * c;
  for (long i = a; i < b; ++i) {
    double x, y;
    undistort_one(model, in9, obs_xy[2 * i], obs_xy[2 * i + 1], f32, &x, &y);
    und[2 * i] = x;
    und[2 * i + 1] = y;
  }
  double R[9], t[3], r;
  const int st = pnp_view(obs_obj + 3 * a, und + 2 * a, (int)(b - a), min_points, f32, R, t, &r);
#pragma unroll
  for (int k = 0; k < 9; ++k) pose[12 * v + k] = R[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) pose[12 * v + 9 + k] = t[k];
  rmse[v] = r;
  status[v] = st;
}

__global__ void __launch_bounds__(PAIR_BLOCK)
k_pose_pair_rmse(const double* __restrict__ pair_pose, const long* __restrict__ pair_start, const double* __restrict__ obs_a,
                 const double* __restrict__ obs_b, double* __restrict__ rmse, long* __restrict__ count) {
  __shared__ double part[PAIR_BLOCK / 64];
  const long p = blockIdx.x;
  const long a = pair_start[p], b = pair_start[p + 1];
  double rt[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) rt[k] = pair_pose[12 * p + k];
  double s = 0.0;
  for (long i = a + threadIdx.x; i < b; i += PAIR_BLOCK) s += pair_obs_sq(rt, obs_a[2 * i], obs_a[2 * i + 1], obs_b[2 * i], obs_b[2 * i + 1]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < PAIR_BLOCK / 64; ++w) tot += part[w];
    const long m = b - a;
    rmse[p] = m > 0 ? sqrt(tot / (2.0 * (double)m)) : 0.0;
    count[p] = m;
  }
}

int err(int code, const std::string& msg) { return cba_set_error(code, msg.c_str()); }  // returns `code`

// device buffers of one call, freed on every path
struct Buffers {
  std::vector<void*> p;
  ~Buffers() { for (void* b : p) (void)hipFree(b); }
  int up(const void* src, size_t bytes, void** dst) {
    void* ptr = nullptr;
    if (hipMalloc(&ptr, std::max<size_t>(bytes, 8)) != hipSuccess) return CBA_ERR_HIP;
    p.push_back(ptr);
    if (src && bytes && hipMemcpy(ptr, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return CBA_ERR_HIP;
    *dst = ptr;
    return CBA_OK;
  }
};

int select_device(int32_t device, const char* what) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return err(CBA_ERR_NO_DEVICE, std::string(what) + ": no HIP device");
  if (device < 0 || device >= ndev) return err(CBA_ERR_INVALID, std::string(what) + ": device " + std::to_string(device) + " of " + std::to_string(ndev));
  if (hipSetDevice(device) != hipSuccess) return err(CBA_ERR_HIP, std::string(what) + ": hipSetDevice failed");
  return CBA_OK;
}

}  // namespace

extern "C" {

int cba_pose_pnp_batch(const cba_pose_pnp_desc* d, int32_t device, double* pose_out, double* rmse_out, int32_t* status_out,
                       double* undistorted_out) {
  const char* what = "cba_pose_pnp_batch";
  if (!d || !pose_out || !rmse_out || !status_out) return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  if (d->n_views < 0 || d->n_cams <= 0 || !d->cam_model || !d->cam_intr || (d->n_views > 0 && (!d->view_start || !d->view_cam || !d->obs_xy || !d->obs_obj)))
    return err(CBA_ERR_INVALID, std::string(what) + ": bad descriptor");
  if (d->n_views == 0) return CBA_OK;
  // bounds of everything the kernel indexes, checked on the host before anything reaches the device
  if (d->view_start[0] != 0) return err(CBA_ERR_INVALID, std::string(what) + ": view_start[0] != 0");
  for (int64_t v = 0; v < d->n_views; ++v) {
    if (d->view_start[v + 1] < d->view_start[v]) return err(CBA_ERR_INVALID, std::string(what) + ": view_start decreases at view " + std::to_string(v));
    if (d->view_start[v + 1] - d->view_start[v] > (int64_t)1 << 30) return err(CBA_ERR_INVALID, std::string(what) + ": view too large");
    if (d->view_cam[v] < 0 || d->view_cam[v] >= d->n_cams) return err(CBA_ERR_INVALID, std::string(what) + ": view_cam out of range at view " + std::to_string(v));
  }
  for (int32_t c = 0; c < d->n_cams; ++c)
    if (d->cam_model[c] != 0 && d->cam_model[c] != 1) return err(CBA_ERR_INVALID, std::string(what) + ": unknown camera model");
  int rc = select_device(device, what);
  if (rc) return rc;
  const int64_t n_views = d->n_views, n_obs = d->view_start[n_views];
  // views by point count (stable: equal counts keep their order)
  std::vector<int64_t> order(n_views);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
    return d->view_start[x + 1] - d->view_start[x] < d->view_start[y + 1] - d->view_start[y];
  });
  Buffers buf;
  void *dord = nullptr, *dvs = nullptr, *dvc = nullptr, *dmodel = nullptr, *dintr = nullptr, *dxy = nullptr, *dobj = nullptr, *dund = nullptr,
       *dpose = nullptr, *drmse = nullptr, *dst = nullptr;
  rc = buf.up(order.data(), (size_t)n_views * sizeof(int64_t), &dord);
  if (!rc) rc = buf.up(d->view_start, (size_t)(n_views + 1) * sizeof(int64_t), &dvs);
  if (!rc) rc = buf.up(d->view_cam, (size_t)n_views * sizeof(int32_t), &dvc);
  if (!rc) rc = buf.up(d->cam_model, (size_t)d->n_cams * sizeof(int32_t), &dmodel);
  if (!rc) rc = buf.up(d->cam_intr, (size_t)d->n_cams * 9 * sizeof(double), &dintr);
  if (!rc) rc = buf.up(d->obs_xy, (size_t)n_obs * 2 * sizeof(double), &dxy);
  if (!rc) rc = buf.up(d->obs_obj, (size_t)n_obs * 3 * sizeof(double), &dobj);
  if (!rc) rc = buf.up(nullptr, (size_t)n_obs * 2 * sizeof(double), &dund);
  if (!rc) rc = buf.up(nullptr, (size_t)n_views * 12 * sizeof(double), &dpose);
  if (!rc) rc = buf.up(nullptr, (size_t)n_views * sizeof(double), &drmse);
  if (!rc) rc = buf.up(nullptr, (size_t)n_views * sizeof(int32_t), &dst);
  if (rc) return err(CBA_ERR_HIP, std::string(what) + ": device allocation / upload failed");
  static_assert(sizeof(long) == sizeof(int64_t), "CSR offsets are passed as long");
  const int grid = (int)((n_views + POSE_BLOCK - 1) / POSE_BLOCK);
  hipLaunchKernelGGL(k_pose_pnp, dim3(grid), dim3(POSE_BLOCK), 0, 0, (long)n_views, (const long*)dord, (const long*)dvs, (const int*)dvc,
                     (const int*)dmodel, (const double*)dintr, (const double*)dxy, (const double*)dobj, (int)d->min_points,
                     d->float32_io ? 1 : 0, (double*)dund, (double*)dpose, (double*)drmse, (int*)dst);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpy(pose_out, dpose, (size_t)n_views * 12 * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(rmse_out, drmse, (size_t)n_views * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(status_out, dst, (size_t)n_views * sizeof(int32_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess && undistorted_out) e = hipMemcpy(undistorted_out, dund, (size_t)n_obs * 2 * sizeof(double), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return err(CBA_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
  return CBA_OK;
}

int cba_pose_pair_rmse(const cba_pose_pair_desc* d, int32_t device, double* rmse_out, int64_t* count_out) {
  const char* what = "cba_pose_pair_rmse";
  if (!d || !rmse_out || !count_out) return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  if (d->n_pairs < 0 || (d->n_pairs > 0 && (!d->pair_pose || !d->pair_start || !d->obs_a || !d->obs_b)))
    return err(CBA_ERR_INVALID, std::string(what) + ": bad descriptor");
  if (d->n_pairs == 0) return CBA_OK;
  if (d->pair_start[0] != 0) return err(CBA_ERR_INVALID, std::string(what) + ": pair_start[0] != 0");
  for (int64_t p = 0; p < d->n_pairs; ++p)
    if (d->pair_start[p + 1] < d->pair_start[p]) return err(CBA_ERR_INVALID, std::string(what) + ": pair_start decreases at pair " + std::to_string(p));
  if (d->n_pairs > 0x7fffffff) return err(CBA_ERR_INVALID, std::string(what) + ": too many pairs");
  int rc = select_device(device, what);
  if (rc) return rc;
  const int64_t n_pairs = d->n_pairs, n_obs = d->pair_start[n_pairs];
  Buffers buf;
  void *dpose = nullptr, *dps = nullptr, *da = nullptr, *db = nullptr, *drmse = nullptr, *dcount = nullptr;
  rc = buf.up(d->pair_pose, (size_t)n_pairs * 12 * sizeof(double), &dpose);
  if (!rc) rc = buf.up(d->pair_start, (size_t)(n_pairs + 1) * sizeof(int64_t), &dps);
  if (!rc) rc = buf.up(d->obs_a, (size_t)n_obs * 2 * sizeof(double), &da);
  if (!rc) rc = buf.up(d->obs_b, (size_t)n_obs * 2 * sizeof(double), &db);
  if (!rc) rc = buf.up(nullptr, (size_t)n_pairs * sizeof(double), &drmse);
  if (!rc) rc = buf.up(nullptr, (size_t)n_pairs * sizeof(int64_t), &dcount);
  if (rc) return err(CBA_ERR_HIP, std::string(what) + ": device allocation / upload failed");
  hipLaunchKernelGGL(k_pose_pair_rmse, dim3((unsigned)n_pairs), dim3(PAIR_BLOCK), 0, 0, (const double*)dpose, (const long*)dps,
                     (const double*)da, (const double*)db, (double*)drmse, (long*)dcount);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpy(rmse_out, drmse, (size_t)n_pairs * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(count_out, dcount, (size_t)n_pairs * sizeof(int64_t), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return err(CBA_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
  return CBA_OK;
}

}  // extern "C"
