// cba_reconstruct_trajectories of libcaliscope_ba.so (C ABI: include/caliscope_trajectory.h): the 2-D tracks of a whole recording
// to filled, triangulated, filled and smoothed 3-D trajectories on one dense grid; and cba_reconstruct_trajectories_refined
// (include/caliscope/trajectory_refine.h), the same call with the robust reprojection refinement of every point in between; and
// cba_reconstruct_trajectories_uncertain (include/caliscope/trajectory_uncertainty.h), either of them with the 3-D covariance of
// every sample; and cba_reconstruct_trajectories_smoothed and cba_smooth_trajectories (include/caliscope/trajectory_smoother.h), the
// covariance-weighted fixed-interval smoother behind the uncertain call and on its own.  What a thread does, and the checks, are
// trajectory_math.h, trajectory_refine_math.h, trajectory_cov_math.h and trajectory_smooth_math.h (shared with
// tests/native/trajectory_harness.cpp, trajectory_refine_harness.cpp, trajectory_cov_harness.cpp and trajectory_smooth_harness.cpp);
// this file holds the kernels and the entry points.
//
//   k_traj_fill2d       one thread per uploaded row (sorted by camera, trajectory, frame): the row's cell of xy[c][s][2] / ft[c][s],
//                       and the first min(hole, xy_gap) cells of the hole between it and the next row of its track.  Holes of
//                       different rows are disjoint and no row lies in a hole (the checks refuse duplicates), so nothing is
//                       written twice.  Both grids are NaN (all bits set) before it runs.
//   k_traj_frame_time   one thread per frame: mean of the times of the frame in a fixed order.
//   k_traj_triangulate  one thread per slot s = f * n_traj + j; neighbouring threads read neighbouring cells of every camera's grid.
//   k_traj_refine       (refined call only) one thread per slot, the same access pattern as k_traj_triangulate: Levenberg-Marquardt on the
//                       slot's point in registers, the views in use in the byte grid view_state[c][s].
//   k_traj_cov          (uncertain call only) one thread per slot, the same access pattern again: V = sum B^T B over the views in use,
//                       its Cholesky factor, then the camera pairs of the calibration term on wave-uniform counters.  The camera
//                       tables are staged in LDS up to TRAJ_COV_LDS_CAMS cameras (STAGE), read from global memory above.
//                       No scratch in either form; as compiled for gfx950 the staged form takes 256 VGPRs and 4 AGPRs (one wave
//                       per SIMD: the table rows it reads from LDS sit in VGPRs), the global form 249 VGPRs (two waves per SIMD:
//                       its rows are scalar loads).  NOISE (smoothed call only): the noise term also goes to a buffer of its own.
//   k_traj_fill3d       one thread per slot, in place (see traj_fill3d_cell for why that is safe).
//   k_traj_cov_filled   (uncertain call with xyz_gap only) one thread per slot: cov_status 2 for the cells the 3-D fill added.
//   k_traj_filtfilt     one thread per (trajectory, coordinate); thread t reads xyz[f][t] and its scratch column scratch[e][t], so
//                       a wave's loads and stores are contiguous.
//   k_traj_smooth       (smoothed calls only) one thread per trajectory: the Kalman filter forward and the modified Bryson-Frazier
//                       pass backward over the frames of its span, 6-state, everything in registers, what the backward pass needs
//                       parked component-major in park[45][n_slots].  A serial recurrence like k_traj_filtfilt: latency, not
//                       throughput; the loads of the next frame are issued before the arithmetic of the current one.
//
// Null stream throughout: the launches of a call run in the order they were issued.  Nothing is added with atomics.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "trajectory_math.h"
#include "trajectory_refine_math.h"
#include "trajectory_cov_math.h"
#include "trajectory_smooth_math.h"
#include "device_call.h"

using namespace cba;

namespace {

__global__ void __launch_bounds__(TRAJ_BLOCK)
k_traj_fill2d(int64_t n_rows, int64_t n_traj, int64_t n_slots, const int32_t* __restrict__ row_cam, const int64_t* __restrict__ row_slot,
              const double* __restrict__ row_xy, const double* __restrict__ row_time, int max_gap, double* __restrict__ xy, double* __restrict__ ft) {
  const int64_t i = (int64_t)blockIdx.x * TRAJ_BLOCK + threadIdx.x;
  if (i >= n_rows) return;
  traj_fill2d_row(n_rows, n_traj, n_slots, i, row_cam, row_slot, row_xy, row_time, max_gap, xy, ft);
}

__global__ void __launch_bounds__(TRAJ_BLOCK)
k_traj_frame_time(int32_t n_cams, int64_t n_frames, int64_t n_traj, int64_t n_slots, const double* __restrict__ ft, double* __restrict__ frame_time) {
  const int64_t f = (int64_t)blockIdx.x * TRAJ_BLOCK + threadIdx.x;
  if (f >= n_frames) return;
  frame_time[f] = traj_frame_mean(n_cams, n_traj, n_slots, f, ft);
}

__global__ void __launch_bounds__(TRAJ_BLOCK)
k_traj_triangulate(int32_t n_cams, int64_t n_traj, int64_t n_slots, const uint8_t* __restrict__ cam_posed, const int32_t* __restrict__ cam_model,
                   const double* __restrict__ cam_intr, const double* __restrict__ cam_P, const double* __restrict__ xy,
                   const double* __restrict__ frame_time, int f32, double* __restrict__ xyz, uint8_t* __restrict__ valid, double* __restrict__ time) {
  const int64_t s = (int64_t)blockIdx.x * TRAJ_BLOCK + threadIdx.x;
  if (s >= n_slots) return;
  double p[3];
  const int views = traj_triangulate_slot(n_cams, n_slots, s, cam_posed, cam_model, cam_intr, cam_P, xy, f32, p);
  xyz[3 * s] = p[0];
  xyz[3 * s + 1] = p[1];
  xyz[3 * s + 2] = p[2];
  valid[s] = views >= 2 ? 1 : 0;
  time[s] = views >= 2 ? frame_time[s / n_traj] : traj_nan();
}

__global__ void __launch_bounds__(TRAJ_BLOCK)
k_traj_refine(int32_t n_cams, int64_t n_slots, const uint8_t* __restrict__ cam_posed, const int32_t* __restrict__ cam_model,
              const double* __restrict__ cam_intr, const double* __restrict__ cam_P, const double* __restrict__ xy, int loss, double f_scale,
              int max_iter, double reject_px, int max_reject, int min_views, const uint8_t* __restrict__ valid, double* __restrict__ xyz,
              uint8_t* view_state, int32_t* __restrict__ views, double* __restrict__ rms_px, double* __restrict__ max_px,
              int32_t* __restrict__ iterations, uint8_t* __restrict__ status) {
  const int64_t s = (int64_t)blockIdx.x * TRAJ_BLOCK + threadIdx.x;
  if (s >= n_slots) return;
  traj_refine_slot(n_cams, n_slots, s, cam_posed, cam_model, cam_intr, cam_P, xy, loss, f_scale, max_iter, reject_px, max_reject, min_views, valid,
                   xyz, view_state, views, rms_px, max_px, iterations, status);
}

template <bool STAGE, bool NOISE>
__global__ void __launch_bounds__(TRAJ_BLOCK)
k_traj_cov(int32_t n_cams, int64_t n_slots, const double* __restrict__ cam_tab, const int32_t* __restrict__ cam_np, const int64_t* __restrict__ cam_off,
           const double* __restrict__ cam_cov, int64_t ncp, double sigma_px, const uint8_t* __restrict__ cam_posed, const double* __restrict__ xy,
           const uint8_t* __restrict__ view_state, const uint8_t* __restrict__ valid, const double* __restrict__ xyz, double* __restrict__ cov,
           double* __restrict__ cov_calib, uint8_t* __restrict__ cov_status, double* __restrict__ meas_cov) {
  extern __shared__ __attribute__((aligned(16))) double s_tab[];
  const CamTab* tabs = (const CamTab*)cam_tab;
  if constexpr (STAGE) {
    for (int32_t i = threadIdx.x; i < n_cams * CAMTAB_DOUBLES; i += TRAJ_BLOCK) s_tab[i] = cam_tab[i];
    __syncthreads();
    tabs = (const CamTab*)s_tab;
  }
  const int64_t s = (int64_t)blockIdx.x * TRAJ_BLOCK + threadIdx.x;
  if (s >= n_slots) return;
  traj_cov_slot(n_cams, n_slots, s, tabs, cam_np, cam_off, cam_cov, ncp, sigma_px, cam_posed, xy, view_state, valid, xyz, cov, cov_calib, cov_status,
                NOISE ? meas_cov : nullptr);
}

__global__ void __launch_bounds__(TRAJ_BLOCK)
k_traj_cov_filled(int64_t n_slots, const uint8_t* __restrict__ valid, uint8_t* __restrict__ cov_status) {
  const int64_t s = (int64_t)blockIdx.x * TRAJ_BLOCK + threadIdx.x;
  if (s >= n_slots) return;
  traj_cov_mark_filled(s, valid, cov_status);
}

__global__ void __launch_bounds__(TRAJ_BLOCK)
k_traj_fill3d(int64_t n_frames, int64_t n_traj, int64_t n_slots, int max_gap, uint8_t* valid, double* xyz, double* time) {
  const int64_t s = (int64_t)blockIdx.x * TRAJ_BLOCK + threadIdx.x;
  if (s >= n_slots) return;
  traj_fill3d_cell(n_frames, n_traj, s, max_gap, valid, xyz, time);
}

__global__ void __launch_bounds__(TRAJ_BLOCK)
k_traj_filtfilt(int64_t n_frames, int64_t n_traj, int order, const double* __restrict__ b, const double* __restrict__ a, const double* __restrict__ zi,
                const uint8_t* __restrict__ valid, double* xyz, double* scratch) {
  const int64_t t = (int64_t)blockIdx.x * TRAJ_BLOCK + threadIdx.x;
  if (t >= 3 * n_traj) return;
  traj_filtfilt_thread(n_frames, n_traj, t, order, b, a, zi, valid, xyz, scratch);
}

__global__ void __launch_bounds__(TRAJ_BLOCK)
k_traj_smooth(int64_t n_frames, int64_t n_traj, const double* __restrict__ xyz, const double* __restrict__ meas_cov, const uint8_t* __restrict__ measured,
              SmoothModel model, double* __restrict__ park, double* __restrict__ pos, double* __restrict__ vel, double* __restrict__ pos_cov,
              double* __restrict__ vel_cov, double* __restrict__ nis, uint8_t* status) {
  const int64_t j = (int64_t)blockIdx.x * TRAJ_BLOCK + threadIdx.x;
  if (j >= n_traj) return;
  traj_smooth_thread(n_frames, n_traj, j, xyz, meas_cov, measured, model, park, pos, vel, pos_cov, vel_cov, nis, status);
}

unsigned blocks(int64_t n) { return (unsigned)((n + TRAJ_BLOCK - 1) / TRAJ_BLOCK); }

// The checks of a call and its memory check against `memory` (<= 0: not checked)
int validate(const cba_traj_desc* d, bool refined, const cba_traj_refine* r, const cba_traj_uncertainty* u, const cba_traj_cov_out* co,
             const cba_traj_smoother* sm, const cba_traj_smooth_out* so, double memory, std::string& msg) {
  if (sm) return traj_smoothed_validate(d, refined ? r : nullptr, u, co, sm, so, memory, msg);
  if (u) return traj_uncertain_validate(d, refined ? r : nullptr, u, co, memory, msg);
  return refined ? traj_refined_validate(d, r, memory, msg) : traj_validate(d, memory, msg);
}

// The device buffers of the smoother's results, NaN / status 0 until k_traj_smooth writes a row, and its scratch.
struct SmoothBuffers {
  double *pos = nullptr, *vel = nullptr, *pos_cov = nullptr, *vel_cov = nullptr, *nis = nullptr, *park = nullptr;
  uint8_t* status = nullptr;

  void make(Buffers& buf, int64_t n_slots) {
    pos = buf.make<double>(n_slots, 3);
    vel = buf.make<double>(n_slots, 3);
    pos_cov = buf.make<double>(n_slots, 6);
    vel_cov = buf.make<double>(n_slots, 6);
    nis = buf.make<double>(n_slots);
    status = buf.make<uint8_t>(n_slots);
    park = buf.make<double>(SMOOTH_PARK, n_slots);
  }
  // (all bits set is a NaN)
  void clear(Buffers& buf, int64_t n_slots) {
    const size_t n = (size_t)n_slots;
    buf.check(hipMemsetAsync(pos, 0xff, n * 3 * sizeof(double), 0));
    if (!buf.status()) buf.check(hipMemsetAsync(vel, 0xff, n * 3 * sizeof(double), 0));
    if (!buf.status()) buf.check(hipMemsetAsync(pos_cov, 0xff, n * 6 * sizeof(double), 0));
    if (!buf.status()) buf.check(hipMemsetAsync(vel_cov, 0xff, n * 6 * sizeof(double), 0));
    if (!buf.status()) buf.check(hipMemsetAsync(nis, 0xff, n * sizeof(double), 0));
    if (!buf.status()) buf.check(hipMemsetAsync(status, 0, n, 0));
  }
  void launch(int64_t n_frames, int64_t n_traj, const double* xyz, const double* meas_cov, const uint8_t* measured, const SmoothModel& model) {
    hipLaunchKernelGGL(k_traj_smooth, dim3(blocks(n_traj)), dim3(TRAJ_BLOCK), 0, 0, n_frames, n_traj, xyz, meas_cov, measured, model, park, pos, vel,
                       pos_cov, vel_cov, nis, status);
  }
  void out(Buffers& buf, int64_t n_slots, cba_traj_smooth_out* o) const {
    buf.out(o->pos, pos, n_slots, 3);
    buf.out(o->vel, vel, n_slots, 3);
    buf.out(o->pos_cov, pos_cov, n_slots, 6);
    buf.out(o->vel_cov, vel_cov, n_slots, 6);
    buf.out(o->nis, nis, n_slots);
    buf.out(o->status, status, n_slots);
  }
};

// what a call without a launch returns; meas_cov too where the call has one
void smooth_nothing(int64_t n_slots, cba_traj_smooth_out* o, bool with_meas_cov) {
  const double nan = traj_nan();
  for (int64_t s = 0; s < n_slots; ++s) {
    for (int i = 0; i < 3; ++i) {
      if (o->pos) o->pos[3 * s + i] = nan;
      if (o->vel) o->vel[3 * s + i] = nan;
    }
    for (int i = 0; i < 6; ++i) {
      if (o->pos_cov) o->pos_cov[6 * s + i] = nan;
      if (o->vel_cov) o->vel_cov[6 * s + i] = nan;
      if (with_meas_cov && o->meas_cov) o->meas_cov[6 * s + i] = nan;
    }
    if (o->nis) o->nis[s] = nan;
    if (o->status) o->status[s] = SMOOTH_NONE;
  }
}

// The entry points of the reconstruction.  refined: r and q belong to the call (r is checked, not assumed); otherwise nothing of the refinement is
// checked, allocated or launched.  u and co: the uncertain call; null, nothing of the covariance is checked, allocated or launched.
// sm and so: the smoothed call (with u and co); null, nothing of the smoother is checked, allocated or launched.
int reconstruct(const char* what, const cba_traj_desc* d, bool refined, const cba_traj_refine* r, int32_t device, cba_traj_out* out,
                cba_traj_quality* q, const cba_traj_uncertainty* u = nullptr, cba_traj_cov_out* co = nullptr, const cba_traj_smoother* sm = nullptr,
                cba_traj_smooth_out* so = nullptr) {
  if (!d || !out || (refined && !q)) return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  // everything that does not need the device first: the sizes, the filter, every index the kernels use
  std::string msg;
  // (memory_limit 0: the free memory is asked for below)
  int rc = validate(d, refined, r, u, co, sm, so, (double)d->memory_limit, msg);
  if (rc) return err(rc, msg);
  const int32_t n_cams = d->n_cams;
  const int64_t n_frames = d->n_frames, n_traj = d->n_traj, n_rows = d->n_rows, n_slots = n_frames * n_traj;
  if (n_rows == 0) {
    const double nan = traj_nan();
    for (int64_t s = 0; s < n_slots; ++s) {
      if (out->xyz) out->xyz[3 * s] = out->xyz[3 * s + 1] = out->xyz[3 * s + 2] = nan;
      if (out->valid) out->valid[s] = 0;
      if (out->slot_time) out->slot_time[s] = nan;
    }
    for (int64_t f = 0; f < n_frames; ++f)
      if (out->frame_time) out->frame_time[f] = nan;
    for (int64_t i = 0; i < (int64_t)n_cams * n_slots; ++i) {
      if (out->xy_filled) out->xy_filled[2 * i] = out->xy_filled[2 * i + 1] = nan;
      if (out->ft_filled) out->ft_filled[i] = nan;
      if (refined && q->view_state) q->view_state[i] = VIEW_NONE;
    }
    for (int64_t s = 0; refined && s < n_slots; ++s) {
      if (q->views) q->views[s] = 0;
      if (q->rms_px) q->rms_px[s] = nan;
      if (q->max_px) q->max_px[s] = nan;
      if (q->iterations) q->iterations[s] = 0;
      if (q->status) q->status[s] = REFINE_NO_POINT;
    }
    for (int64_t s = 0; u && s < n_slots; ++s) {
      for (int i = 0; i < 6; ++i) {
        if (co->cov) co->cov[6 * s + i] = nan;
        if (co->cov_calib) co->cov_calib[6 * s + i] = nan;
      }
      if (co->cov_status) co->cov_status[s] = COV_NO_POINT;
    }
    if (sm) smooth_nothing(n_slots, so, true);
    return CBA_OK;
  }
  rc = select_device(device, what);
  if (rc) return rc;
  double memory = (double)d->memory_limit;
  if (d->memory_limit <= 0) {
    size_t free_bytes = 0, total_bytes = 0;
    if (hipMemGetInfo(&free_bytes, &total_bytes) != hipSuccess) return err(CBA_ERR_HIP, std::string(what) + ": hipMemGetInfo failed");
    memory = (double)free_bytes;
  }
  if (traj_device_bytes(d) + (refined ? traj_refine_device_bytes(d) : 0.0) + (u ? traj_cov_device_bytes(d, u, co) : 0.0) +
          (sm ? traj_smooth_device_bytes((double)n_frames, (double)n_traj, false) : 0.0) > memory) {
    rc = validate(d, refined, r, u, co, sm, so, memory, msg);  // (puts the message together)
    return err(rc ? rc : CBA_ERR_UNSUPPORTED, msg);
  }
  if (n_slots > (int64_t)0x7fffffff * TRAJ_BLOCK || n_rows > (int64_t)0x7fffffff * TRAJ_BLOCK)
    return err(CBA_ERR_UNSUPPORTED, std::string(what) + ": more workgroups than one launch takes");

  Buffers buf;
  const uint8_t* dposed = buf.in(d->cam_posed, n_cams);
  const int32_t* dmodel = buf.in(d->cam_model, n_cams);
  const double* dintr = buf.in(d->cam_intr, n_cams, 9);
  const double* dP = buf.in(d->cam_P, n_cams, 12);
  const int32_t* drcam = buf.in(d->row_cam, n_rows);
  const int64_t* drslot = buf.in(d->row_slot, n_rows);
  const double* drxy = buf.in(d->row_xy, n_rows, 2);
  const double* drt = buf.in(d->row_time, n_rows);
  double* dxy = buf.make<double>(n_cams, n_slots, 2);
  double* dft = buf.make<double>(n_cams, n_slots);
  double* dframe = buf.make<double>(n_frames);
  double* dxyz = buf.make<double>(n_slots, 3);
  uint8_t* dvalid = buf.make<uint8_t>(n_slots);
  double* dtime = buf.make<double>(n_slots);
  // without a filter its four buffers stay null
  const int order = d->filter_b ? d->filter_order : 0;
  const double* db = d->filter_b ? buf.in(d->filter_b, order + 1) : nullptr;
  const double* da = d->filter_b ? buf.in(d->filter_a, order + 1) : nullptr;
  const double* dzi = d->filter_b ? buf.in(d->filter_zi, order) : nullptr;
  double* dscratch = d->filter_b ? buf.make<double>(n_frames + 2 * traj_pad(order), n_traj, 3) : nullptr;
  // without the refinement its six buffers stay null
  uint8_t* dstate = refined ? buf.make<uint8_t>(n_cams, n_slots) : nullptr;
  int32_t* dviews = refined ? buf.make<int32_t>(n_slots) : nullptr;
  double* drms = refined ? buf.make<double>(n_slots) : nullptr;
  double* dmax = refined ? buf.make<double>(n_slots) : nullptr;
  int32_t* diter = refined ? buf.make<int32_t>(n_slots) : nullptr;
  uint8_t* dstatus = refined ? buf.make<uint8_t>(n_slots) : nullptr;
  // without the covariance its eight buffers stay null
  std::vector<CamTab> tabs;
  std::vector<int32_t> cam_np;
  std::vector<int64_t> cam_off;
  if (u) traj_cov_tables(d, u, tabs, cam_np, cam_off);
  const double* dtab = u ? buf.in((const double*)tabs.data(), n_cams, CAMTAB_DOUBLES) : nullptr;
  const int32_t* dnp = u ? buf.in(cam_np.data(), n_cams) : nullptr;
  const int64_t* doff = u ? buf.in(cam_off.data(), n_cams) : nullptr;
  const double* dcamcov = u && u->cam_cov ? buf.in(u->cam_cov, u->ncp, u->ncp) : nullptr;
  double* dcov = u ? buf.make<double>(n_slots, 6) : nullptr;
  double* dcalib = u && co->cov_calib ? buf.make<double>(n_slots, 6) : nullptr;
  uint8_t* dcstat = u ? buf.make<uint8_t>(n_slots) : nullptr;
  // without the smoother its eight buffers stay null
  double* dmeas = sm ? buf.make<double>(n_slots, 6) : nullptr;
  SmoothBuffers smooth;
  if (sm) smooth.make(buf, n_slots);
  if (buf.status()) return buf.result(what);

  // all bits set is a NaN: "no row here"
  const size_t cells = (size_t)n_cams * (size_t)n_slots;
  buf.check(hipMemsetAsync(dxy, 0xff, cells * 2 * sizeof(double), 0));
  if (!buf.status()) buf.check(hipMemsetAsync(dft, 0xff, cells * sizeof(double), 0));
  if (buf.status()) return buf.result(what);
  hipLaunchKernelGGL(k_traj_fill2d, dim3(blocks(n_rows)), dim3(TRAJ_BLOCK), 0, 0, n_rows, n_traj, n_slots, drcam, drslot, drxy, drt, (int)d->xy_gap, dxy, dft);
  hipLaunchKernelGGL(k_traj_frame_time, dim3(blocks(n_frames)), dim3(TRAJ_BLOCK), 0, 0, n_cams, n_frames, n_traj, n_slots, dft, dframe);
  hipLaunchKernelGGL(k_traj_triangulate, dim3(blocks(n_slots)), dim3(TRAJ_BLOCK), 0, 0, n_cams, n_traj, n_slots, dposed, dmodel, dintr, dP, dxy,
                     dframe, d->float32_io ? 1 : 0, dxyz, dvalid, dtime);
  if (refined)  // (writes every cell of its six buffers)
    hipLaunchKernelGGL(k_traj_refine, dim3(blocks(n_slots)), dim3(TRAJ_BLOCK), 0, 0, n_cams, n_slots, dposed, dmodel, dintr, dP, dxy, (int)r->loss,
                       r->f_scale, (int)r->max_iter, r->reject_px, (int)r->max_reject, (int)r->min_views, dvalid, dxyz, dstate, dviews, drms, dmax,
                       diter, dstatus);
  if (u) {  // (writes every cell of its buffers)
    const int64_t camcov_rows = u->cam_cov ? u->ncp : 0;
    const bool stage = n_cams <= TRAJ_COV_LDS_CAMS;
    const auto kernel = stage ? (sm ? k_traj_cov<true, true> : k_traj_cov<true, false>) : (sm ? k_traj_cov<false, true> : k_traj_cov<false, false>);
    hipLaunchKernelGGL(kernel, dim3(blocks(n_slots)), dim3(TRAJ_BLOCK), stage ? (size_t)n_cams * sizeof(CamTab) : 0, 0, n_cams, n_slots, dtab, dnp, doff,
                       dcamcov, camcov_rows, u->sigma_px, dposed, dxy, dstate, dvalid, dxyz, dcov, dcalib, dcstat, dmeas);
  }
  if (sm) {  // (xyz_gap and the filter are refused with it: xyz and cov_status are those k_traj_cov saw and wrote)
    smooth.clear(buf, n_slots);
    if (buf.status()) return buf.result(what);
    smooth.launch(n_frames, n_traj, dxyz, dmeas, dcstat, smooth_model(sm->fps, sm->accel_density, sm->velocity_prior_std, sm->max_gap));
  }
  if (d->xyz_gap > 0)
    hipLaunchKernelGGL(k_traj_fill3d, dim3(blocks(n_slots)), dim3(TRAJ_BLOCK), 0, 0, n_frames, n_traj, n_slots, (int)d->xyz_gap, dvalid, dxyz, dtime);
  if (u && d->xyz_gap > 0)
    hipLaunchKernelGGL(k_traj_cov_filled, dim3(blocks(n_slots)), dim3(TRAJ_BLOCK), 0, 0, n_slots, dvalid, dcstat);
  if (d->filter_b)
    hipLaunchKernelGGL(k_traj_filtfilt, dim3(blocks(3 * n_traj)), dim3(TRAJ_BLOCK), 0, 0, n_frames, n_traj, order, db, da, dzi, dvalid, dxyz,
                       dscratch);
  buf.check(hipGetLastError());
  buf.out(out->xyz, dxyz, n_slots, 3);
  buf.out(out->valid, dvalid, n_slots);
  buf.out(out->slot_time, dtime, n_slots);
  buf.out(out->frame_time, dframe, n_frames);
  buf.out(out->xy_filled, dxy, n_cams, n_slots, 2);
  buf.out(out->ft_filled, dft, n_cams, n_slots);
  if (refined) {
    buf.out(q->views, dviews, n_slots);
    buf.out(q->rms_px, drms, n_slots);
    buf.out(q->max_px, dmax, n_slots);
    buf.out(q->iterations, diter, n_slots);
    buf.out(q->status, dstatus, n_slots);
    buf.out(q->view_state, dstate, n_cams, n_slots);
  }
  if (u) {
    buf.out(co->cov, dcov, n_slots, 6);
    buf.out(co->cov_calib, dcalib, n_slots, 6);
    buf.out(co->cov_status, dcstat, n_slots);
  }
  if (sm) {
    smooth.out(buf, n_slots, so);
    buf.out(so->meas_cov, dmeas, n_slots, 6);
  }
  if (!buf.status()) buf.check(hipDeviceSynchronize());
  return buf.result(what);
}

}  // namespace

extern "C" int cba_reconstruct_trajectories(const cba_traj_desc* d, int32_t device, cba_traj_out* out) {
  return reconstruct("cba_reconstruct_trajectories", d, false, nullptr, device, out, nullptr);
}

extern "C" int cba_reconstruct_trajectories_refined(const cba_traj_desc* d, const cba_traj_refine* refine, int32_t device, cba_traj_out* out,
                                                    cba_traj_quality* quality) {
  return reconstruct("cba_reconstruct_trajectories_refined", d, true, refine, device, out, quality);
}

extern "C" int cba_reconstruct_trajectories_uncertain(const cba_traj_desc* d, const cba_traj_refine* refine, const cba_traj_uncertainty* uncertainty,
                                                      int32_t device, cba_traj_out* out, cba_traj_quality* quality, cba_traj_cov_out* cov_out) {
  const char* what = "cba_reconstruct_trajectories_uncertain";
  if (!uncertainty || !cov_out) return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  if ((refine == nullptr) != (quality == nullptr)) return err(CBA_ERR_INVALID, std::string(what) + ": quality goes with refine, and with it alone");
  return reconstruct(what, d, refine != nullptr, refine, device, out, quality, uncertainty, cov_out);
}

extern "C" int cba_reconstruct_trajectories_smoothed(const cba_traj_desc* d, const cba_traj_refine* refine, const cba_traj_uncertainty* uncertainty,
                                                     const cba_traj_smoother* smoother, int32_t device, cba_traj_out* out, cba_traj_quality* quality,
                                                     cba_traj_cov_out* cov_out, cba_traj_smooth_out* smooth_out) {
  const char* what = "cba_reconstruct_trajectories_smoothed";
  if (!uncertainty || !cov_out) return err(CBA_ERR_INVALID, std::string(what) + ": uncertainty: null argument (the smoother weights a sample by its covariance)");
  if (!smoother || !smooth_out) return err(CBA_ERR_INVALID, std::string(what) + ": smoother: null argument");
  if ((refine == nullptr) != (quality == nullptr)) return err(CBA_ERR_INVALID, std::string(what) + ": quality goes with refine, and with it alone");
  return reconstruct(what, d, refine != nullptr, refine, device, out, quality, uncertainty, cov_out, smoother, smooth_out);
}

extern "C" int cba_smooth_trajectories(const cba_smooth_desc* d, int32_t device, cba_traj_smooth_out* out) {
  const char* what = "cba_smooth_trajectories";
  if (!d || !out) return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  std::string msg;
  bool any = false;
  int rc = traj_smooth_validate(d, (double)d->memory_limit, msg, &any);
  if (rc) return err(rc, msg);
  const int64_t n_frames = d->n_frames, n_traj = d->n_traj, n_slots = n_frames * n_traj;
  if (!any) {
    smooth_nothing(n_slots, out, false);
    return CBA_OK;
  }
  rc = select_device(device, what);
  if (rc) return rc;
  if (d->memory_limit <= 0) {
    size_t free_bytes = 0, total_bytes = 0;
    if (hipMemGetInfo(&free_bytes, &total_bytes) != hipSuccess) return err(CBA_ERR_HIP, std::string(what) + ": hipMemGetInfo failed");
    rc = traj_smooth_validate(d, (double)free_bytes, msg, &any);
    if (rc) return err(rc, msg);
  }
  if (n_traj > (int64_t)0x7fffffff * TRAJ_BLOCK) return err(CBA_ERR_UNSUPPORTED, std::string(what) + ": more workgroups than one launch takes");
  Buffers buf;
  const double* dxyz = buf.in(d->xyz, n_slots, 3);
  const double* dmeas = buf.in(d->meas_cov, n_slots, 6);
  const uint8_t* dflag = buf.in(d->measured, n_slots);
  SmoothBuffers smooth;
  smooth.make(buf, n_slots);
  if (buf.status()) return buf.result(what);
  smooth.clear(buf, n_slots);
  if (buf.status()) return buf.result(what);
  smooth.launch(n_frames, n_traj, dxyz, dmeas, dflag, smooth_model(d->fps, d->accel_density, d->velocity_prior_std, d->max_gap));
  buf.check(hipGetLastError());
  smooth.out(buf, n_slots, out);
  if (!buf.status()) buf.check(hipDeviceSynchronize());
  return buf.result(what);
}
