// cba_reconstruct_trajectories of libcaliscope_ba.so (C ABI: include/caliscope_trajectory.h): the 2-D tracks of a whole recording
// to filled, triangulated, filled and smoothed 3-D trajectories on one dense grid; and cba_reconstruct_trajectories_refined
// (include/caliscope/trajectory_refine.h), the same call with the robust reprojection refinement of every point in between; and
// cba_reconstruct_trajectories_uncertain (include/caliscope/trajectory_uncertainty.h), either of them with the 3-D covariance of
// every sample.  What a thread does, and the checks, are trajectory_math.h, trajectory_refine_math.h and trajectory_cov_math.h
// (shared with tests/native/trajectory_harness.cpp, trajectory_refine_harness.cpp and trajectory_cov_harness.cpp); this file holds
// the kernels and the entry points.
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
//                       its rows are scalar loads).
//   k_traj_fill3d       one thread per slot, in place (see traj_fill3d_cell for why that is safe).
//   k_traj_cov_filled   (uncertain call with xyz_gap only) one thread per slot: cov_status 2 for the cells the 3-D fill added.
//   k_traj_filtfilt     one thread per (trajectory, coordinate); thread t reads xyz[f][t] and its scratch column scratch[e][t], so
//                       a wave's loads and stores are contiguous.
//
// Null stream throughout: the launches of a call run in the order they were issued.  Nothing is added with atomics.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "trajectory_math.h"
#include "trajectory_refine_math.h"
#include "trajectory_cov_math.h"
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

template <bool STAGE>
__global__ void __launch_bounds__(TRAJ_BLOCK)
k_traj_cov(int32_t n_cams, int64_t n_slots, const double* __restrict__ cam_tab, const int32_t* __restrict__ cam_np, const int64_t* __restrict__ cam_off,
           const double* __restrict__ cam_cov, int64_t ncp, double sigma_px, const uint8_t* __restrict__ cam_posed, const double* __restrict__ xy,
           const uint8_t* __restrict__ view_state, const uint8_t* __restrict__ valid, const double* __restrict__ xyz, double* __restrict__ cov,
           double* __restrict__ cov_calib, uint8_t* __restrict__ cov_status) {
  extern __shared__ __attribute__((aligned(16))) double s_tab[];
  const CamTab* tabs = (const CamTab*)cam_tab;
  if constexpr (STAGE) {
    for (int32_t i = threadIdx.x; i < n_cams * CAMTAB_DOUBLES; i += TRAJ_BLOCK) s_tab[i] = cam_tab[i];
    __syncthreads();
    tabs = (const CamTab*)s_tab;
  }
  const int64_t s = (int64_t)blockIdx.x * TRAJ_BLOCK + threadIdx.x;
  if (s >= n_slots) return;
  traj_cov_slot(n_cams, n_slots, s, tabs, cam_np, cam_off, cam_cov, ncp, sigma_px, cam_posed, xy, view_state, valid, xyz, cov, cov_calib, cov_status);
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

unsigned blocks(int64_t n) { return (unsigned)((n + TRAJ_BLOCK - 1) / TRAJ_BLOCK); }

// The checks of a call and its memory check against `memory` (<= 0: not checked)
int validate(const cba_traj_desc* d, bool refined, const cba_traj_refine* r, const cba_traj_uncertainty* u, const cba_traj_cov_out* co, double memory,
             std::string& msg) {
  if (u) return traj_uncertain_validate(d, refined ? r : nullptr, u, co, memory, msg);
  return refined ? traj_refined_validate(d, r, memory, msg) : traj_validate(d, memory, msg);
}

// The three entry points.  refined: r and q belong to the call (r is checked, not assumed); otherwise nothing of the refinement is
// checked, allocated or launched.  u and co: the uncertain call; null, nothing of the covariance is checked, allocated or launched.
int reconstruct(const char* what, const cba_traj_desc* d, bool refined, const cba_traj_refine* r, int32_t device, cba_traj_out* out,
                cba_traj_quality* q, const cba_traj_uncertainty* u = nullptr, cba_traj_cov_out* co = nullptr) {
  if (!d || !out || (refined && !q)) return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  // everything that does not need the device first: the sizes, the filter, every index the kernels use
  std::string msg;
  // (memory_limit 0: the free memory is asked for below)
  int rc = validate(d, refined, r, u, co, (double)d->memory_limit, msg);
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
  if (traj_device_bytes(d) + (refined ? traj_refine_device_bytes(d) : 0.0) + (u ? traj_cov_device_bytes(d, u, co) : 0.0) > memory) {
    rc = validate(d, refined, r, u, co, memory, msg);  // (puts the message together)
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
    if (n_cams <= TRAJ_COV_LDS_CAMS)
      hipLaunchKernelGGL(k_traj_cov<true>, dim3(blocks(n_slots)), dim3(TRAJ_BLOCK), (size_t)n_cams * sizeof(CamTab), 0, n_cams, n_slots, dtab, dnp, doff,
                         dcamcov, camcov_rows, u->sigma_px, dposed, dxy, dstate, dvalid, dxyz, dcov, dcalib, dcstat);
    else
      hipLaunchKernelGGL(k_traj_cov<false>, dim3(blocks(n_slots)), dim3(TRAJ_BLOCK), 0, 0, n_cams, n_slots, dtab, dnp, doff, dcamcov, camcov_rows,
                         u->sigma_px, dposed, dxy, dstate, dvalid, dxyz, dcov, dcalib, dcstat);
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
