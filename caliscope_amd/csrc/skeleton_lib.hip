// cba_adjust_skeleton and cba_skeleton_components of libcaliscope_ba.so (C ABI and mathematics: include/caliscope/trajectory_skeleton.h):
// reconstructed trajectories adjusted to the constant segment lengths of a skeleton, frame by frame, weighted by their covariances.  What a
// thread does, the checks and the host's serial forms are trajectory_skeleton_math.h (shared with
// tests/native/trajectory_skeleton_harness.cpp); this file holds the kernels and the entry points.
//
//   k_skel_pass    one thread per slot: pos, pos_cov and status as they are without an adjustment (the input's bytes, status 2, where
//                  measured; NaN, status 0, elsewhere).  k_skel_adjust overwrites the slots it adjusts.
//   k_skel_length  one workgroup of 256 per segment: d_f of the co-measured frames to dist[s][f] (all bits set elsewhere), the lower median
//                  and the lower median of the absolute deviations by a radix select over the bit patterns, 8 passes of 8 bits, the
//                  histogram of a pass in LDS (integer atomics; the counts do not depend on their order), then the trimmed
//                  inverse-variance mean: lane t adds its frames in ascending order, lane 0 the 256 partial sums.
//   k_skel_adjust  one workgroup per (frame, component): skel_adjust_group.  Dynamic LDS sized by the call's largest component
//                  (skel_lds_bytes: the packed triangle, seven vectors of n, R^-1, the scalars and the int tables; 118 008 bytes at 54
//                  points, above the 64 KiB a kernel gets without hipFuncSetAttribute).  256 threads, measured against 64 below.
//
// As compiled for gfx950 (-O3): k_skel_adjust 87 VGPRs, no AGPRs, dynamic LDS alone; k_skel_length 70 VGPRs and 5 128 bytes of static LDS
// (the histogram 1 024, the partial sums 2 x 2 048, the count); k_skel_pass 16 VGPRs.  No kernel uses scratch.
//
// Null stream throughout: the launches of a call run in the order they were issued.  No floating-point atomics.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "trajectory_skeleton_math.h"
#include "device_call.h"

using namespace cba;

namespace {

__global__ void __launch_bounds__(SKEL_PASS_BLOCK)
k_skel_pass(int64_t n_slots, const double* __restrict__ xyz, const double* __restrict__ meas_cov, const uint8_t* __restrict__ measured,
            double* __restrict__ pos, double* __restrict__ pos_cov, uint8_t* __restrict__ status) {
  const int64_t s = (int64_t)blockIdx.x * SKEL_PASS_BLOCK + threadIdx.x;
  if (s >= n_slots) return;
  skel_pass_slot(s, xyz, meas_cov, measured, pos, pos_cov, status);
}

// The element of rank `rank` among the keys of the frames that have one: key(f) = dist[f] (MAD false) or the bits of |dist[f] - med|.
// hist: 256 counters in LDS.  Uniform: every thread returns the same key.
template <bool MAD>
__device__ uint64_t skel_select(int t, int64_t n_frames, const uint64_t* dist, double med, int64_t rank, uint32_t* hist) {
  uint64_t prefix = 0;
  for (int pass = 7; pass >= 0; --pass) {
    const int shift = 8 * pass;
    hist[t] = 0;
    __syncthreads();
    for (int64_t f = t; f < n_frames; f += SKEL_LEN_THREADS) {
      const uint64_t raw = dist[f];
      if (raw == ~0ull) continue;
      const uint64_t key = MAD ? skel_bits(fabs(skel_from_bits(raw) - med)) : raw;
      if (pass == 7 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(key >> shift) & 255], 1u);
    }
    __syncthreads();
    int64_t below = 0;
    int bin = 0;
    for (; bin < 255; ++bin) {
      const int64_t c = hist[bin];
      if (below + c > rank) break;
      below += c;
    }
    prefix |= (uint64_t)bin << shift;
    rank -= below;
    __syncthreads();  // (every thread has read the histogram)
  }
  return prefix;
}

__global__ void __launch_bounds__(SKEL_LEN_THREADS)
k_skel_length(int64_t n_frames, int64_t n_traj, const int32_t* __restrict__ seg_traj, const double* __restrict__ seg_length, double trim,
              const double* __restrict__ xyz, const double* __restrict__ meas_cov, const uint8_t* __restrict__ measured, uint64_t* dist_all,
              double* __restrict__ length, double* __restrict__ med_out, double* __restrict__ mad_out, int64_t* __restrict__ frames) {
  __shared__ uint32_t hist[256];
  __shared__ double pnum[SKEL_LEN_THREADS], pden[SKEL_LEN_THREADS];
  __shared__ uint32_t total;
  const int64_t s = blockIdx.x;
  const int t = threadIdx.x;
  const int32_t a = seg_traj[2 * s], b = seg_traj[2 * s + 1];
  uint64_t* dist = dist_all + s * n_frames;
  if (t == 0) total = 0;
  __syncthreads();
  uint32_t mine = 0;
  for (int64_t f = t; f < n_frames; f += SKEL_LEN_THREADS) {
    double d, v;
    const bool has = skel_pair(f * n_traj + a, f * n_traj + b, xyz, meas_cov, measured, &d, &v);
    dist[f] = has ? skel_bits(d) : ~0ull;
    mine += has ? 1u : 0u;
  }
  if (mine) atomicAdd(&total, mine);
  __syncthreads();  // (the block's own stores to dist are visible to it behind the barrier)
  const int64_t n = total;
  const double given = seg_length[s];
  if (n == 0) {  // (uniform)
    if (t == 0) { length[s] = given; med_out[s] = traj_nan(); mad_out[s] = traj_nan(); frames[s] = 0; }
    return;
  }
  const double med = skel_from_bits(skel_select<false>(t, n_frames, dist, 0.0, (n - 1) / 2, hist));
  const double mad = skel_from_bits(skel_select<true>(t, n_frames, dist, med, (n - 1) / 2, hist));
  double num = 0.0, den = 0.0;
  if (given != given) skel_length_lane(t, n_frames, n_traj, a, b, xyz, meas_cov, measured, med, mad, trim, &num, &den);
  pnum[t] = num;
  pden[t] = den;
  __syncthreads();
  if (t == 0) {
    double sn = 0.0, sd = 0.0;
    for (int i = 0; i < SKEL_LEN_THREADS; ++i) { sn += pnum[i]; sd += pden[i]; }
    length[s] = given != given ? sn / sd : given;
    med_out[s] = med;
    mad_out[s] = mad;
    frames[s] = n;
  }
}

// 256 threads: 74.6 ms against 130.5 ms with one wave of 64 for the whole call at 20 000 frames of one 33-point component on an MI355X
// (DESIGN.md); the two sizes return the same bytes, every sum being in an order that does not depend on the size.
constexpr int SKEL_ADJUST_THREADS = 256;
__global__ void __launch_bounds__(SKEL_ADJUST_THREADS)
k_skel_adjust(int32_t n_comp, int64_t n_traj, int64_t n_seg, const double* __restrict__ xyz, const double* __restrict__ meas_cov,
              const uint8_t* __restrict__ measured, const double* __restrict__ length, const double* __restrict__ sigma, int max_iter, double tol,
              SkelTables T, SkelOut O) {
  extern __shared__ __attribute__((aligned(16))) double skel_lds[];
  const int64_t cell = blockIdx.x;
  skel_adjust_group((int)threadIdx.x, SKEL_ADJUST_THREADS, cell / n_comp, (int32_t)(cell % n_comp), n_comp, n_traj, n_seg, xyz, meas_cov, measured, length,
                    sigma, max_iter, tol, T, O, skel_lds);
}

}  // namespace

extern "C" int64_t cba_skeleton_components(const cba_skeleton_desc* d, int32_t* traj_comp) {
  const std::string what = "cba_skeleton_components: ";
  if (!d || (!traj_comp && d->n_traj > 0)) return err(CBA_ERR_INVALID, what + "null argument");
  SkelPlan plan;
  std::string msg;
  const int rc = skel_plan(what, d->n_traj, d->n_seg, d->seg_traj, plan, msg);
  if (rc) return err(rc, msg);
  for (int64_t j = 0; j < d->n_traj; ++j) traj_comp[j] = plan.traj_comp[(size_t)j];
  return plan.n_comp;
}

extern "C" int cba_adjust_skeleton(const cba_skeleton_desc* d, int32_t device, cba_skeleton_out* out) {
  const char* what = "cba_adjust_skeleton";
  if (!d || !out) return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  SkelPlan plan;
  std::string msg;
  bool launch = false;
  int rc = skel_validate(d, (double)d->memory_limit, plan, msg, &launch);
  if (rc) return err(rc, msg);
  if (!launch) {
    skel_nothing(d, plan.n_comp, out);
    return CBA_OK;
  }
  rc = select_device(device, what);
  if (rc) return rc;
  if (d->memory_limit <= 0) {
    size_t free_bytes = 0, total_bytes = 0;
    if (hipMemGetInfo(&free_bytes, &total_bytes) != hipSuccess) return err(CBA_ERR_HIP, std::string(what) + ": hipMemGetInfo failed");
    rc = skel_validate(d, (double)free_bytes, plan, msg, &launch);
    if (rc) return err(rc, msg);
  }
  const int64_t n_frames = d->n_frames, n_traj = d->n_traj, n_seg = d->n_seg, n_slots = n_frames * n_traj;
  const int32_t n_comp = plan.n_comp;
  if (n_slots > (int64_t)0x7fffffff * SKEL_PASS_BLOCK || n_frames * n_comp > 0x7fffffff || n_seg > 0x7fffffff)
    return err(CBA_ERR_UNSUPPORTED, std::string(what) + ": more workgroups than one launch takes");
  const size_t lds = (size_t)skel_lds_bytes(plan.max_m);

  Buffers buf;
  const double* dxyz = buf.in(d->xyz, n_slots, 3);
  const double* dmeas = buf.in(d->meas_cov, n_slots, 6);
  const uint8_t* dflag = buf.in(d->measured, n_slots);
  const int32_t* dseg = buf.in(d->seg_traj, n_seg, 2);
  const double* dgiven = buf.in(d->seg_length, n_seg);
  const double* dsigma = buf.in(d->seg_sigma, n_seg);
  SkelTables T;
  T.comp_pt = buf.in(plan.comp_pt.data(), plan.comp_pt.size());
  T.pts = buf.in(plan.pts.data(), plan.pts.size());
  T.comp_seg = buf.in(plan.comp_seg.data(), plan.comp_seg.size());
  T.segs = buf.in(plan.segs.data(), plan.segs.size());
  T.seg_loc = buf.in(plan.seg_loc.data(), plan.seg_loc.size());
  T.inc_start = buf.in(plan.inc_start.data(), plan.inc_start.size());
  T.inc = buf.in(plan.inc.data(), plan.inc.size());
  SkelOut O;
  O.pos = buf.make<double>(n_slots, 3);
  O.pos_cov = buf.make<double>(n_slots, 6);
  O.status = buf.make<uint8_t>(n_slots);
  O.len_before = buf.make<double>(n_frames, n_seg);
  O.w_before = buf.make<double>(n_frames, n_seg);
  O.len_after = buf.make<double>(n_frames, n_seg);
  O.chi2 = buf.make<double>(n_frames, n_comp);
  O.rows = buf.make<int32_t>(n_frames, n_comp);
  O.iterations = buf.make<int32_t>(n_frames, n_comp);
  O.comp_status = buf.make<uint8_t>(n_frames, n_comp);
  uint64_t* ddist = buf.make<uint64_t>(n_seg, n_frames);
  double* dlength = buf.make<double>(n_seg);
  double* dmed = buf.make<double>(n_seg);
  double* dmad = buf.make<double>(n_seg);
  int64_t* dframes = buf.make<int64_t>(n_seg);
  if (buf.status()) return buf.result(what);

  // all bits set is a NaN: "the segment is inactive here"
  const size_t fs = (size_t)n_frames * (size_t)n_seg;
  buf.check(hipMemsetAsync(O.len_before, 0xff, fs * sizeof(double), 0));
  if (!buf.status()) buf.check(hipMemsetAsync(O.w_before, 0xff, fs * sizeof(double), 0));
  if (!buf.status()) buf.check(hipMemsetAsync(O.len_after, 0xff, fs * sizeof(double), 0));
  if (!buf.status()) buf.check(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_skel_adjust), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if (buf.status()) return buf.result(what);
  hipLaunchKernelGGL(k_skel_pass, dim3((unsigned)((n_slots + SKEL_PASS_BLOCK - 1) / SKEL_PASS_BLOCK)), dim3(SKEL_PASS_BLOCK), 0, 0, n_slots, dxyz, dmeas,
                     dflag, O.pos, O.pos_cov, O.status);
  hipLaunchKernelGGL(k_skel_length, dim3((unsigned)n_seg), dim3(SKEL_LEN_THREADS), 0, 0, n_frames, n_traj, dseg, dgiven, d->trim, dxyz, dmeas, dflag, ddist,
                     dlength, dmed, dmad, dframes);
  hipLaunchKernelGGL(k_skel_adjust, dim3((unsigned)(n_frames * n_comp)), dim3(SKEL_ADJUST_THREADS), lds, 0, n_comp, n_traj, n_seg, dxyz, dmeas, dflag, (const double*)dlength,
                     dsigma, (int)d->max_iter, d->tol, T, O);
  buf.check(hipGetLastError());
  buf.out(out->pos, (const double*)O.pos, n_slots, 3);
  buf.out(out->pos_cov, (const double*)O.pos_cov, n_slots, 6);
  buf.out(out->status, (const uint8_t*)O.status, n_slots);
  buf.out(out->length, (const double*)dlength, n_seg);
  buf.out(out->med, (const double*)dmed, n_seg);
  buf.out(out->mad, (const double*)dmad, n_seg);
  buf.out(out->frames, (const int64_t*)dframes, n_seg);
  buf.out(out->len_before, (const double*)O.len_before, n_frames, n_seg);
  buf.out(out->w_before, (const double*)O.w_before, n_frames, n_seg);
  buf.out(out->len_after, (const double*)O.len_after, n_frames, n_seg);
  buf.out(out->chi2, (const double*)O.chi2, n_frames, n_comp);
  buf.out(out->rows, (const int32_t*)O.rows, n_frames, n_comp);
  buf.out(out->iterations, (const int32_t*)O.iterations, n_frames, n_comp);
  buf.out(out->comp_status, (const uint8_t*)O.comp_status, n_frames, n_comp);
  if (!buf.status()) buf.check(hipDeviceSynchronize());
  return buf.result(what);
}
