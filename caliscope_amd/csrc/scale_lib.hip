// cba_scale_errors of libcaliscope_ba.so (C ABI: include/caliscope_ba.h): all pairwise distance errors of every rigid-object
// group of a capture volume, reduced to eight numbers per group.  The arithmetic, the lane-to-pair mapping and the binning of the
// groups are scale_math.h (shared with tests/native/scale_harness.cpp); this file holds the two kernels and their launch
// (cba_scale_launch); the entry point itself, with the input checks and the binning, is plain C++ in cba_solve.cpp.
//
//   k_scale_small      one thread per group of at most SCALE_SMALL_MAX = 12 entries (66 pairs), 64 groups per workgroup, groups
//                      handed out sorted by entry count so that the lanes of a wave run loops of the same length.  Markers of 4
//                      corners have 6 pairs each: anything wider than a lane per marker idles most of a wave.
//   k_scale_group<CAP> one 256-thread workgroup per group of 13 entries or more.  The six coordinates of every entry are staged in
//                      LDS as six arrays of CAP doubles (CAP = 128: 6 KiB, boards up to 128 corners; CAP = 1024: 48 KiB, up to
//                      1024 corners, 3 workgroups per CU), lanes stride over the pairs (scale_lane_first / scale_lane_next: integer
//                      steps, no pair-number formula).  A lane reads entry i (the same or a neighbouring address across the wave:
//                      a broadcast) and entry j (consecutive doubles across the lanes of a row: every bank once per 32 lanes).
//                      CAP = 0 is the same kernel for groups above 1024 entries, up to SCALE_MAX_GROUP = 32 768: no stage, the
//                      coordinates are gathered through the cache.
//
// Sums run in a fixed order: a lane's pairs in its own order, then shuffle-down 32, 16, .. 1 inside each wave, then the four waves
// in sequence through LDS.  No atomics: two runs return the same bits.  One upload per input array, the launches (at most four,
// into disjoint rows of the output) on the null stream, one copy-back; no host synchronisation in between.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/caliscope_ba.h"
#include "device_call.h"
#include "scale_math.h"

using namespace cba;

static_assert(CBA_SCALE_NSTAT == SCALE_NSTAT, "header and arithmetic disagree on the statistics per group");

namespace {

__global__ void __launch_bounds__(SCALE_SMALL_BLOCK)
k_scale_small(int64_t n_list, const int64_t* __restrict__ list, const int64_t* __restrict__ group_start,
              const int64_t* __restrict__ ent_world, const double* __restrict__ ent_obj, const double* __restrict__ world,
              double* __restrict__ stats) {
  const int64_t q = (int64_t)blockIdx.x * SCALE_SMALL_BLOCK + threadIdx.x;
  if (q >= n_list) return;
  const int64_t g = list[q];
  const int64_t a = group_start[g];
  scale_group_serial(world, ent_world + a, ent_obj + 3 * a, (int)(group_start[g + 1] - a), stats + SCALE_NSTAT * g);
}

template <int CAP>
__global__ void __launch_bounds__(SCALE_BLOCK)
k_scale_group(const int64_t* __restrict__ list, const int64_t* __restrict__ group_start, const int64_t* __restrict__ ent_world,
              const double* __restrict__ ent_obj, const double* __restrict__ world, double* __restrict__ stats) {
  __shared__ double stage[CAP > 0 ? 6 * CAP : 1];
  __shared__ double red[(SCALE_BLOCK / 64) * 7];
  const int64_t g = list[blockIdx.x];
  const int64_t a = group_start[g];
  const int n = (int)(group_start[g + 1] - a);  // 13 <= n <= CAP (or SCALE_MAX_GROUP): the host's binning
  const int64_t* __restrict__ ew = ent_world + a;
  const double* __restrict__ eo = ent_obj + 3 * a;
  const int t = threadIdx.x;
  double cx = 0.0, cy = 0.0, cz = 0.0;
  for (int e = t; e < n; e += SCALE_BLOCK) {
    const double* w = world + 3 * ew[e];
    const double x = w[0], y = w[1], z = w[2];
    cx += x; cy += y; cz += z;
    if (CAP > 0) {
      stage[e] = x; stage[CAP + e] = y; stage[2 * CAP + e] = z;
      stage[3 * CAP + e] = eo[3 * e]; stage[4 * CAP + e] = eo[3 * e + 1]; stage[5 * CAP + e] = eo[3 * e + 2];
    }
  }
  if (CAP > 0) __syncthreads();
  ScaleAcc acc;
  scale_acc_zero(acc);
  int i, j;
  bool more = scale_lane_first(n, t, i, j);
  while (more) {
    if (CAP > 0) {
      scale_pair(acc, stage[i], stage[CAP + i], stage[2 * CAP + i], stage[j], stage[CAP + j], stage[2 * CAP + j],
                 stage[3 * CAP + i], stage[4 * CAP + i], stage[5 * CAP + i], stage[3 * CAP + j], stage[4 * CAP + j], stage[5 * CAP + j]);
    } else {
      const double* wi = world + 3 * ew[i];
      const double* wj = world + 3 * ew[j];
      scale_pair(acc, wi[0], wi[1], wi[2], wj[0], wj[1], wj[2], eo[3 * i], eo[3 * i + 1], eo[3 * i + 2], eo[3 * j], eo[3 * j + 1],
                 eo[3 * j + 2]);
    }
    more = scale_lane_next(n, SCALE_BLOCK, i, j);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ScaleAcc b;
    b.s1 = __shfl_down(acc.s1, o, 64);
    b.s2 = __shfl_down(acc.s2, o, 64);
    b.mx = __shfl_down(acc.mx, o, 64);
    b.dref = __shfl_down(acc.dref, o, 64);
    scale_acc_merge(acc, b);
    cx += __shfl_down(cx, o, 64);
    cy += __shfl_down(cy, o, 64);
    cz += __shfl_down(cz, o, 64);
  }
  if ((t & 63) == 0) {
    double* r = red + (t >> 6) * 7;
    r[0] = acc.s1; r[1] = acc.s2; r[2] = acc.mx; r[3] = acc.dref; r[4] = cx; r[5] = cy; r[6] = cz;
  }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int w = 1; w < SCALE_BLOCK / 64; ++w) {
      const double* r = red + w * 7;
      ScaleAcc b{r[0], r[1], r[2], r[3]};
      scale_acc_merge(acc, b);
      cx += r[4]; cy += r[5]; cz += r[6];
    }
    scale_write(stats + SCALE_NSTAT * g, acc, cx, cy, cz, n);
  }
}

}  // namespace

// The device half of cba_scale_errors: the caller (cba_solve.cpp) has checked every index and binned the groups.
extern "C" int cba_scale_launch(const cba_scale_desc* d, int32_t device, const int64_t* list, const int64_t* counts, double* stats_out) {
  const char* what = "cba_scale_errors";
  const int64_t n_groups = d->n_groups, n_ent = d->group_start[n_groups];
  int rc = select_device(device, what);
  if (rc) return rc;
  Buffers buf;
  const int64_t* l = buf.in(list, n_groups);
  const int64_t* dgs = buf.in(d->group_start, n_groups + 1);
  const int64_t* dew = buf.in(d->ent_world, n_ent);
  const double* deo = buf.in(d->ent_obj, n_ent, 3);
  const double* dworld = buf.in(d->world_xyz, d->n_world, 3);
  double* dstats = buf.make<double>(n_groups, SCALE_NSTAT);
  if (buf.status()) return buf.result(what);
  const int64_t n_small = counts[0], n_a = counts[1], n_b = counts[2], n_c = counts[3];
  if (n_small)
    hipLaunchKernelGGL(k_scale_small, dim3((unsigned)((n_small + SCALE_SMALL_BLOCK - 1) / SCALE_SMALL_BLOCK)), dim3(SCALE_SMALL_BLOCK), 0, 0, n_small, l, dgs, dew,
                       deo, dworld, dstats);
  if (n_a) hipLaunchKernelGGL(k_scale_group<SCALE_LDS_SMALL>, dim3((unsigned)n_a), dim3(SCALE_BLOCK), 0, 0, l + n_small, dgs, dew, deo, dworld, dstats);
  if (n_b) hipLaunchKernelGGL(k_scale_group<SCALE_LDS_LARGE>, dim3((unsigned)n_b), dim3(SCALE_BLOCK), 0, 0, l + n_small + n_a, dgs, dew, deo, dworld, dstats);
  if (n_c) hipLaunchKernelGGL(k_scale_group<0>, dim3((unsigned)n_c), dim3(SCALE_BLOCK), 0, 0, l + n_small + n_a + n_b, dgs, dew, deo, dworld, dstats);
  buf.check(hipGetLastError());
  buf.out(stats_out, dstats, n_groups, SCALE_NSTAT);
  return buf.result(what);
}
