// cba_reprojection_filter of libcaliscope_ba.so (C ABI: include/caliscope_report.h): pixel errors of every observation, their sums
// per camera and per group, and the keep mask of the percentile / absolute outlier filter with its safety floor.  Keys, the select
// step, the percentile and the checks are report_math.h (shared with tests/native/report_harness.cpp); this file holds the kernels
// and the entry point.
//
//   k_rep_cam_prep  one thread per camera: the CamTab of ba_math.h from the pose and the locked intrinsics.
//   k_rep_error     a workgroup of REP_BLOCK threads per REP_TILE observations: project_residual, pixels = residual x fx, err =
//                   sqrt(ex^2 + ey^2) (or err_in).  err^2 is added per camera and per group to partials in LDS (REP_LDS_SUMS
//                   entries each; beyond, straight to global memory), the overall sum per wave by shuffles; per workgroup one
//                   global add per destination that it touched.  The camera tables are read from LDS while REP_LDS_CAMS hold
//                   them, through the vector cache beyond.
//   k_rep_hist      one select pass: every observation looks at the queries of its segment and adds one to hist[query][digit]
//                   where its high bits equal the query's prefix; histograms in LDS per workgroup while REP_LDS_QUERIES hold
//                   them ("overall" puts every observation on the same two histograms), flushed with 64-bit integer atomics.
//   k_rep_refine    one thread per query: rep_refine on its histogram, new prefix and rank, histogram cleared for the next pass.
//                   Histograms never travel to the host.
//   k_rep_mask      keep = err <= threshold[camera], kept counts per camera (LDS partials as above).
//
// Null stream throughout.  The host reads back: the non-finite count after the error kernel, the keys the queries found after a
// select round (a few bytes per segment: the interpolation is host arithmetic), and the kept counts after a mask.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ba_math.h"
#include "report_math.h"
#include "device_call.h"

using namespace cba;

namespace {

typedef unsigned long long u64;

__global__ void __launch_bounds__(REP_BLOCK)
k_rep_cam_prep(int32_t n_cams, const int32_t* __restrict__ cam_model, const double* __restrict__ cam_const, const double* __restrict__ cam_pose,
               double* __restrict__ tab) {
  const int32_t c = blockIdx.x * REP_BLOCK + threadIdx.x;
  if (c >= n_cams) return;
  double xc[MAX_NC];
#pragma unroll
  for (int i = 0; i < MAX_NC; ++i) xc[i] = i < 6 ? cam_pose[(int64_t)c * 6 + i] : 0.0;  // locked intrinsics: six parameters
  CamTab t;
  cam_prepare(xc, cam_const + (int64_t)c * CAM_CONST_STRIDE, cam_model[c], 6, &t, 0);
  const double* src = reinterpret_cast<const double*>(&t);
#pragma unroll
  for (int i = 0; i < CAMTAB_DOUBLES; ++i) tab[(int64_t)c * CAMTAB_DOUBLES + i] = src[i];
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;  // lane 0 holds the sum
}

template <bool TAB_LDS>
__global__ void __launch_bounds__(REP_BLOCK)
k_rep_error(int64_t n_obs, int32_t n_cams, int32_t n_groups, const double* __restrict__ tab, const double* __restrict__ points,
            const int32_t* __restrict__ obs_cam, const int32_t* __restrict__ obs_pt, const double* __restrict__ obs_uv,
            const int32_t* __restrict__ obs_group, const double* __restrict__ err_in, double* __restrict__ err_xy, double* __restrict__ err,
            double* __restrict__ cam_sumsq, u64* __restrict__ cam_count, double* __restrict__ group_sumsq, u64* __restrict__ group_count,
            double* __restrict__ overall, u64* __restrict__ nonfinite) {
  __shared__ double sh_tab[TAB_LDS ? REP_LDS_CAMS * CAMTAB_DOUBLES : 1];
  __shared__ double sh_cam_sum[REP_LDS_SUMS];
  __shared__ double sh_grp_sum[REP_LDS_SUMS];
  __shared__ unsigned sh_cam_cnt[REP_LDS_SUMS];
  __shared__ unsigned sh_grp_cnt[REP_LDS_SUMS];
  __shared__ double sh_total;
  __shared__ unsigned sh_bad;
  const int t = threadIdx.x;
  const bool cam_lds = n_cams <= REP_LDS_SUMS;
  const bool grp_lds = obs_group != nullptr && n_groups <= REP_LDS_SUMS;
  if (TAB_LDS)
    for (int i = t; i < n_cams * CAMTAB_DOUBLES; i += REP_BLOCK) sh_tab[i] = tab[i];
  if (cam_lds)
    for (int i = t; i < n_cams; i += REP_BLOCK) { sh_cam_sum[i] = 0.0; sh_cam_cnt[i] = 0u; }
  if (grp_lds)
    for (int i = t; i < n_groups; i += REP_BLOCK) { sh_grp_sum[i] = 0.0; sh_grp_cnt[i] = 0u; }
  if (t == 0) { sh_total = 0.0; sh_bad = 0u; }
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * REP_TILE;
  double total = 0.0;
  unsigned bad = 0u;
  for (int k = 0; k < REP_TILE / REP_BLOCK; ++k) {
    const int64_t o = base + (int64_t)k * REP_BLOCK + t;
    if (o >= n_obs) break;
    const int32_t cam = obs_cam[o];
    double e;
    if (err_in) {
      e = err_in[o];
    } else {
      const CamTab& c = TAB_LDS ? reinterpret_cast<const CamTab*>(sh_tab)[cam] : reinterpret_cast<const CamTab*>(tab)[cam];
      const int64_t p = obs_pt[o];
      double r[2];
      project_residual(c, points[3 * p], points[3 * p + 1], points[3 * p + 2], obs_uv[2 * o], obs_uv[2 * o + 1], r);
      const double ex = r[0] * c.fx0, ey = r[1] * c.fx0;
      e = sqrt(ex * ex + ey * ey);
      if (err_xy) { err_xy[2 * o] = ex; err_xy[2 * o + 1] = ey; }
    }
    err[o] = e;
    const double sq = e * e;
    total += sq;
    if (!rep_finite(e)) ++bad;
    if (cam_lds) { atomicAdd(&sh_cam_sum[cam], sq); atomicAdd(&sh_cam_cnt[cam], 1u); }
    else { atomicAdd(&cam_sumsq[cam], sq); atomicAdd(&cam_count[cam], (u64)1); }
    if (obs_group) {
      const int32_t g = obs_group[o];
      if (grp_lds) { atomicAdd(&sh_grp_sum[g], sq); atomicAdd(&sh_grp_cnt[g], 1u); }
      else { atomicAdd(&group_sumsq[g], sq); atomicAdd(&group_count[g], (u64)1); }
    }
  }
  total = wave_sum(total);
  if ((t & 63) == 0) atomicAdd(&sh_total, total);
  if (bad) atomicAdd(&sh_bad, bad);
  __syncthreads();
  if (cam_lds)
    for (int i = t; i < n_cams; i += REP_BLOCK)
      if (sh_cam_cnt[i]) { atomicAdd(&cam_sumsq[i], sh_cam_sum[i]); atomicAdd(&cam_count[i], (u64)sh_cam_cnt[i]); }
  if (grp_lds)
    for (int i = t; i < n_groups; i += REP_BLOCK)
      if (sh_grp_cnt[i]) { atomicAdd(&group_sumsq[i], sh_grp_sum[i]); atomicAdd(&group_count[i], (u64)sh_grp_cnt[i]); }
  if (t == 0) {
    atomicAdd(overall, sh_total);
    if (sh_bad) atomicAdd(nonfinite, (u64)sh_bad);
  }
}

// cam_qfirst == nullptr: the "overall" segment, every observation belongs to the queries 0 .. per_seg-1
__global__ void __launch_bounds__(REP_BLOCK)
k_rep_hist(int64_t n_obs, const double* __restrict__ err, const int32_t* __restrict__ obs_cam, const int32_t* __restrict__ cam_qfirst, int32_t per_seg,
           int32_t n_queries, int pass, const u64* __restrict__ q_prefix, u64* __restrict__ hist) {
  __shared__ unsigned sh_hist[REP_LDS_QUERIES * REP_RADIX];
  const int t = threadIdx.x;
  const bool lds = n_queries <= REP_LDS_QUERIES;
  if (lds) {
    for (int i = t; i < n_queries * REP_RADIX; i += REP_BLOCK) sh_hist[i] = 0u;
    __syncthreads();
  }
  const int64_t base = (int64_t)blockIdx.x * REP_TILE;
  for (int k = 0; k < REP_TILE / REP_BLOCK; ++k) {
    const int64_t o = base + (int64_t)k * REP_BLOCK + t;
    if (o >= n_obs) break;
    const int32_t first = cam_qfirst ? cam_qfirst[obs_cam[o]] : 0;
    if (first < 0) continue;
    const uint64_t key = rep_key(err[o]);
    const int digit = rep_digit(key, pass);
    for (int32_t j = 0; j < per_seg; ++j) {
      const int32_t q = first + j;
      if (!rep_matches(key, q_prefix[q], pass)) continue;
      if (lds) atomicAdd(&sh_hist[q * REP_RADIX + digit], 1u);
      else atomicAdd(&hist[(int64_t)q * REP_RADIX + digit], (u64)1);
    }
  }
  if (lds) {
    __syncthreads();
    for (int i = t; i < n_queries * REP_RADIX; i += REP_BLOCK)
      if (sh_hist[i]) atomicAdd(&hist[i], (u64)sh_hist[i]);
  }
}

__global__ void __launch_bounds__(REP_BLOCK)
k_rep_refine(int32_t n_queries, u64* __restrict__ q_prefix, int64_t* __restrict__ q_rank, u64* __restrict__ hist) {
  const int32_t q = blockIdx.x * REP_BLOCK + threadIdx.x;
  if (q >= n_queries) return;
  u64* h = hist + (int64_t)q * REP_RADIX;
  int digit;
  int64_t rank;
  rep_refine(h, q_rank[q], digit, rank);
  q_rank[q] = rank;
  q_prefix[q] = (q_prefix[q] << REP_DIGIT_BITS) | (u64)digit;
  for (int d = 0; d < REP_RADIX; ++d) h[d] = 0;
}

__global__ void __launch_bounds__(REP_BLOCK)
k_rep_mask(int64_t n_obs, int32_t n_cams, const double* __restrict__ err, const int32_t* __restrict__ obs_cam, const double* __restrict__ threshold,
           uint8_t* __restrict__ keep, u64* __restrict__ cam_kept) {
  __shared__ unsigned sh_cnt[REP_LDS_SUMS];
  const int t = threadIdx.x;
  const bool lds = n_cams <= REP_LDS_SUMS;
  if (lds) {
    for (int i = t; i < n_cams; i += REP_BLOCK) sh_cnt[i] = 0u;
    __syncthreads();
  }
  const int64_t base = (int64_t)blockIdx.x * REP_TILE;
  for (int k = 0; k < REP_TILE / REP_BLOCK; ++k) {
    const int64_t o = base + (int64_t)k * REP_BLOCK + t;
    if (o >= n_obs) break;
    const int32_t cam = obs_cam[o];
    const bool kept = rep_keep(err[o], threshold[cam]);
    keep[o] = kept ? 1 : 0;
    if (kept) {
      if (lds) atomicAdd(&sh_cnt[cam], 1u);
      else atomicAdd(&cam_kept[cam], (u64)1);
    }
  }
  if (lds) {
    __syncthreads();
    for (int i = t; i < n_cams; i += REP_BLOCK)
      if (sh_cnt[i]) atomicAdd(&cam_kept[i], (u64)sh_cnt[i]);
  }
}

// One select round on the device: q.rank -> the keys of those order statistics in `found`.
hipError_t select_round(const RepQueries& q, int64_t n_obs, const double* derr, const int32_t* dcam, int32_t* dqfirst, u64* dprefix, int64_t* drank,
                        u64* dhist, std::vector<uint64_t>& found) {
  const int32_t nq = q.n();
  found.assign((size_t)nq, 0);
  if (nq == 0) return hipSuccess;
  hipError_t e = hipMemcpy(drank, q.rank.data(), (size_t)nq * sizeof(int64_t), hipMemcpyHostToDevice);
  if (e == hipSuccess && !q.cam_qfirst.empty()) e = hipMemcpy(dqfirst, q.cam_qfirst.data(), q.cam_qfirst.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemsetAsync(dprefix, 0, (size_t)nq * sizeof(u64), 0);
  if (e == hipSuccess) e = hipMemsetAsync(dhist, 0, (size_t)nq * REP_RADIX * sizeof(u64), 0);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)((n_obs + REP_TILE - 1) / REP_TILE)), qgrid((unsigned)((nq + REP_BLOCK - 1) / REP_BLOCK));
  for (int pass = 0; pass < REP_PASSES; ++pass) {
    hipLaunchKernelGGL(k_rep_hist, grid, dim3(REP_BLOCK), 0, 0, n_obs, derr, dcam, q.cam_qfirst.empty() ? (const int32_t*)nullptr : dqfirst, q.per_seg, nq,
                       pass, (const u64*)dprefix, dhist);
    hipLaunchKernelGGL(k_rep_refine, qgrid, dim3(REP_BLOCK), 0, 0, nq, dprefix, drank, dhist);
  }
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpy(found.data(), dprefix, (size_t)nq * sizeof(u64), hipMemcpyDeviceToHost);
  return e;
}

hipError_t mask_round(int64_t n_obs, int32_t n_cams, const double* derr, const int32_t* dcam, const std::vector<double>& thr, double* dthr, uint8_t* dkeep,
                      u64* dkept, std::vector<int64_t>& kept) {
  hipError_t e = hipMemcpy(dthr, thr.data(), (size_t)n_cams * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemsetAsync(dkept, 0, (size_t)n_cams * sizeof(u64), 0);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_rep_mask, dim3((unsigned)((n_obs + REP_TILE - 1) / REP_TILE)), dim3(REP_BLOCK), 0, 0, n_obs, n_cams, derr, dcam, dthr,
                     dkeep, dkept);
  e = hipGetLastError();
  kept.assign((size_t)n_cams, 0);
  if (e == hipSuccess) e = hipMemcpy(kept.data(), dkept, (size_t)n_cams * sizeof(u64), hipMemcpyDeviceToHost);
  return e;
}

}  // namespace

extern "C" int cba_reprojection_filter(const cba_report_desc* d, int32_t device, cba_report_out* out) {
  const char* what = "cba_reprojection_filter";
  if (!d || !out) return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  // every index the kernels use, checked on the host before anything reaches the device
  std::string msg;
  std::vector<int64_t> cam_rows;
  int rc = rep_validate(d, cam_rows, msg);
  if (rc) return err(rc, msg);
  const int32_t n_cams = d->n_cams, n_groups = d->obs_group ? d->n_groups : 0;
  const int64_t n_obs = d->n_obs;
  const bool filter = d->mode != CBA_REPORT_STATS;
  if (n_obs == 0 || n_cams == 0) {
    for (int32_t c = 0; c < n_cams; ++c) {
      if (out->cam_sumsq) out->cam_sumsq[c] = 0.0;
      if (out->cam_count) out->cam_count[c] = 0;
      if (filter && out->cam_threshold) out->cam_threshold[c] = d->mode == CBA_REPORT_ABSOLUTE ? d->value : rep_inf();
      if (filter && out->cam_kept) out->cam_kept[c] = 0;
    }
    for (int32_t g = 0; g < n_groups; ++g) {
      if (out->group_sumsq) out->group_sumsq[g] = 0.0;
      if (out->group_count) out->group_count[g] = 0;
    }
    if (out->overall_sumsq) *out->overall_sumsq = 0.0;
    if (out->n_nonfinite) *out->n_nonfinite = 0;
    if (filter && out->n_floor_cams) *out->n_floor_cams = 0;
    return CBA_OK;
  }
  rc = select_device(device, what);
  if (rc) return rc;
  Buffers buf;
  // what the chosen path does not read stays null: the kernels branch on that
  const bool project = d->err_in == nullptr;
  const int32_t* dcam = buf.in(d->obs_cam, n_obs);
  const int32_t* dmodel = project ? buf.in(d->cam_model, n_cams) : nullptr;
  const double* dconst = project ? buf.in(d->cam_const, n_cams, CAM_CONST_STRIDE) : nullptr;
  const double* dpose = project ? buf.in(d->cam_pose, n_cams, 6) : nullptr;
  double* dtab = project ? buf.make<double>(n_cams, CAMTAB_DOUBLES) : nullptr;
  const double* dpoints = project ? buf.in(d->points, d->n_points, 3) : nullptr;
  const int32_t* dpt = project ? buf.in(d->obs_pt, n_obs) : nullptr;
  const double* duv = project ? buf.in(d->obs_uv, n_obs, 2) : nullptr;
  double* derr_xy = project && out->err_xy ? buf.make<double>(n_obs, 2) : nullptr;
  const double* derr_in = project ? nullptr : buf.in(d->err_in, n_obs);
  const int32_t* dgroup = d->obs_group ? buf.in(d->obs_group, n_obs) : nullptr;
  double* derr = buf.make<double>(n_obs);
  // the sums of the error kernel in one zeroed block of 8-byte words: camera sums, camera counts, group sums, group counts, overall, non-finite
  const size_t n_sums = 2 * (size_t)n_cams + 2 * (size_t)n_groups + 2;
  u64* dsums = buf.make<u64>(n_sums);
  if (buf.status()) return buf.result(what);
  double* dsums_f64 = (double*)dsums;  // (the sums are doubles, the counts integers, in the same block)
  double* dcam_sum = dsums_f64;
  u64* dcam_cnt = dsums + n_cams;
  double* dgrp_sum = dsums_f64 + 2 * (size_t)n_cams;
  u64* dgrp_cnt = dsums + 2 * (size_t)n_cams + n_groups;
  double* doverall = dsums_f64 + n_sums - 2;
  u64* dbad = dsums + n_sums - 1;
  buf.check(hipMemsetAsync(dsums, 0, n_sums * 8, 0));
  if (buf.status()) return buf.result(what);
  const dim3 grid((unsigned)((n_obs + REP_TILE - 1) / REP_TILE));
  if (project) hipLaunchKernelGGL(k_rep_cam_prep, dim3((unsigned)((n_cams + REP_BLOCK - 1) / REP_BLOCK)), dim3(REP_BLOCK), 0, 0, n_cams, dmodel, dconst, dpose, dtab);
  if (project && n_cams <= REP_LDS_CAMS)
    hipLaunchKernelGGL(k_rep_error<true>, grid, dim3(REP_BLOCK), 0, 0, n_obs, n_cams, n_groups, dtab, dpoints, dcam, dpt, duv, dgroup, derr_in,
                       derr_xy, derr, dcam_sum, dcam_cnt, dgrp_sum, dgrp_cnt, doverall, dbad);
  else
    hipLaunchKernelGGL(k_rep_error<false>, grid, dim3(REP_BLOCK), 0, 0, n_obs, n_cams, n_groups, dtab, dpoints, dcam, dpt, duv, dgroup, derr_in,
                       derr_xy, derr, dcam_sum, dcam_cnt, dgrp_sum, dgrp_cnt, doverall, dbad);
  buf.check(hipGetLastError());
  std::vector<u64> sums(n_sums);
  buf.out(sums.data(), dsums, n_sums);
  if (project) buf.out(out->err_xy, derr_xy, n_obs, 2);
  buf.out(out->err, derr, n_obs);
  if (buf.status()) return buf.result(what);
  for (int32_t c = 0; c < n_cams; ++c) {
    if (out->cam_sumsq) out->cam_sumsq[c] = rep_value(sums[(size_t)c]);
    if (out->cam_count) out->cam_count[c] = (int64_t)sums[(size_t)n_cams + c];
  }
  for (int32_t g = 0; g < n_groups; ++g) {
    if (out->group_sumsq) out->group_sumsq[g] = rep_value(sums[2 * (size_t)n_cams + g]);
    if (out->group_count) out->group_count[g] = (int64_t)sums[2 * (size_t)n_cams + n_groups + g];
  }
  if (out->overall_sumsq) *out->overall_sumsq = rep_value(sums[n_sums - 2]);
  const int64_t n_bad = (int64_t)sums[n_sums - 1];
  if (out->n_nonfinite) *out->n_nonfinite = n_bad;
  if (!filter || n_bad != 0) return CBA_OK;

  // ---- the filter: thresholds (a select round for the percentile), mask, floor round, mask ----
  std::vector<double> thr((size_t)n_cams, d->value);
  RepQueries q;
  if (d->mode == CBA_REPORT_PERCENTILE) q = rep_percentile_queries(cam_rows, n_obs, d->scope, d->value);
  const size_t max_q = std::max<size_t>((size_t)q.n(), (size_t)n_cams);  // the floor round has at most one query per camera
  int32_t* dqfirst = buf.make<int32_t>(n_cams);
  u64* dprefix = buf.make<u64>(max_q);
  int64_t* drank = buf.make<int64_t>(max_q);
  u64* dhist = buf.make<u64>(max_q, REP_RADIX);
  double* dthr = buf.make<double>(n_cams);
  uint8_t* dkeep = buf.make<uint8_t>(n_obs);
  u64* dkept = buf.make<u64>(n_cams);
  if (buf.status()) return buf.result(what);
  std::vector<uint64_t> found;
  std::vector<int64_t> kept;
  if (d->mode == CBA_REPORT_PERCENTILE) {
    buf.check(select_round(q, n_obs, derr, dcam, dqfirst, dprefix, drank, dhist, found));
    if (buf.status()) return buf.result(what);
    rep_percentile_thresholds(q, found, cam_rows, n_obs, d->scope, d->value, thr);
  }
  buf.check(mask_round(n_obs, n_cams, derr, dcam, thr, dthr, dkeep, dkept, kept));
  if (buf.status()) return buf.result(what);
  const RepQueries fq = rep_floor_queries(cam_rows, kept, d->min_per_camera);
  if (fq.n() > 0) {
    buf.check(select_round(fq, n_obs, derr, dcam, dqfirst, dprefix, drank, dhist, found));
    if (buf.status()) return buf.result(what);
    for (int32_t k = 0; k < fq.n(); ++k) thr[(size_t)fq.seg[(size_t)k]] = rep_value(found[(size_t)k]);
    // (the mask of a camera whose threshold did not change comes out as before)
    buf.check(mask_round(n_obs, n_cams, derr, dcam, thr, dthr, dkeep, dkept, kept));
  }
  buf.out(out->keep, dkeep, n_obs);
  if (buf.status()) return buf.result(what);
  for (int32_t c = 0; c < n_cams; ++c) {
    if (out->cam_threshold) out->cam_threshold[c] = thr[(size_t)c];
    if (out->cam_kept) out->cam_kept[c] = kept[(size_t)c];
  }
  if (out->n_floor_cams) *out->n_floor_cams = fq.n();
  return CBA_OK;
}
