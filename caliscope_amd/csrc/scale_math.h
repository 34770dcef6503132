// Arithmetic, lane-to-pair mapping and host-side binning of cba_scale_errors (include/caliscope_ba.h): for every group of
// (world point, object point) entries the errors  err = |w_i - w_j| - |o_i - o_j|  over all pairs i < j, reduced to eight numbers.
// Compiled by hipcc into the kernels of scale_lib.hip and the entry point in cba_solve.cpp, and by g++ into tests/native/scale_harness.cpp, which walks the same pairs in
// the same order on the CPU.
//
// Per pair: plain FP64, a distance is sqrt(dx dx + dy dy + dz dz) in that order, no contraction (as undistort_one of ba_math.h): the
// device and the g++ build differ only where their square roots do.
//
// Which lane takes which pair.  There is no "pair number -> (i, j)" formula (a square root of the pair number is not exact in FP64
// for large groups, and one in FP32 is wrong from a few thousand entries on).  Pairs are ordered row by row, (0,1) (0,2) .. (0,n-1)
// (1,2) ..; lane t of T starts `t` pairs after (0,1) and then moves T pairs on each time, by integer additions and a carry loop
// that walks to the next row while the column is past the end (scale_lane_first / scale_lane_next).  Every quantity is an index
// below n or below n + T: exact in int32 for every n the call accepts.  A lane's carry loop runs at most n times over the whole
// group, next to its n (n - 1) / (2 T) pairs.
//
// SCALE_MAX_GROUP = 32 768 entries (536 854 528 pairs) is the largest group the call takes; CBA_ERR_UNSUPPORTED beyond.  The
// mapping itself is exact up to n + T < 2^31; the limit is set by time (one workgroup works through a group; at the 0.7 G pairs/s a
// workgroup was measured at on staged 600-corner boards the largest group takes of the order of a second) and keeps every pair count
// far below 2^53, so that it is exact as a double.
//
// Binning (scale_plan, on the host), by entry count n of the group:
//   n <= SCALE_SMALL_MAX (12, 66 pairs)   one thread per group, groups handed to lanes sorted by n.  A 4-corner marker has 6 pairs:
//                                         a workgroup, even a wave, per marker would idle 58 of 64 lanes; 250 000 markers are 3 900
//                                         full waves this way.  At 12 entries a thread runs 66 pairs in sequence, the length of the
//                                         longest loop a 256-lane workgroup runs on a 180-corner board.
//   n <= SCALE_LDS_SMALL (128)            one 256-thread workgroup per group, six coordinates per entry staged in 6 KiB of LDS:
//                                         boards of 13 .. 128 corners, 78 .. 8 128 pairs; 26 workgroups fit a CU's LDS, so occupancy
//                                         is bounded by waves, not LDS.
//   n <= SCALE_LDS_LARGE (1024)           the same kernel with a 48 KiB stage (3 workgroups per CU): up to 523 776 pairs per group,
//                                         2 046 per lane, each pair two LDS reads of 24 bytes instead of two gathers.
//   n <= SCALE_MAX_GROUP                  the same kernel without a stage: coordinates are gathered through the cache.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SCALE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SCALE_HD inline
#endif

namespace cba {

constexpr int SCALE_NSTAT = 8;
constexpr int SCALE_BLOCK = 256;          // threads of the workgroup path
constexpr int SCALE_SMALL_BLOCK = 64;     // threads (= groups) per workgroup of the thread-per-group path
constexpr int SCALE_SMALL_MAX = 12;
constexpr int SCALE_LDS_SMALL = 128;
constexpr int SCALE_LDS_LARGE = 1024;
constexpr int SCALE_MAX_GROUP = 32768;

// running statistics of one lane: sum err, sum err^2, max |err|, max true distance
struct ScaleAcc {
  double s1, s2, mx, dref;
};

SCALE_HD void scale_acc_zero(ScaleAcc& a) { a.s1 = 0.0; a.s2 = 0.0; a.mx = 0.0; a.dref = 0.0; }

SCALE_HD double scale_dist(double ax, double ay, double az, double bx, double by, double bz) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double dx = ax - bx, dy = ay - by, dz = az - bz;
  return sqrt(dx * dx + dy * dy + dz * dz);
}

// one pair: w* measured (world) points, o* true (object) points
SCALE_HD void scale_pair(ScaleAcc& a, double wix, double wiy, double wiz, double wjx, double wjy, double wjz, double oix, double oiy,
                         double oiz, double ojx, double ojy, double ojz) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double dt = scale_dist(oix, oiy, oiz, ojx, ojy, ojz);
  const double e = scale_dist(wix, wiy, wiz, wjx, wjy, wjz) - dt;
  a.s1 += e;
  a.s2 += e * e;
  const double ae = fabs(e);
  a.mx = ae > a.mx ? ae : a.mx;
  a.dref = dt > a.dref ? dt : a.dref;
}

// a += b, the step of the reduction trees
SCALE_HD void scale_acc_merge(ScaleAcc& a, const ScaleAcc& b) {
  a.s1 += b.s1;
  a.s2 += b.s2;
  a.mx = b.mx > a.mx ? b.mx : a.mx;
  a.dref = b.dref > a.dref ? b.dref : a.dref;
}

// first pair (i, j) of lane t in a group of n >= 2 entries; false when the lane has none
SCALE_HD bool scale_lane_first(int n, int t, int& i, int& j) {
  i = 0;
  j = 1 + t;
  while (j >= n) {
    ++i;
    if (i >= n - 1) return false;
    j = j - n + i + 1;
  }
  return true;
}

// the pair `stride` pairs after (i, j); false past the last pair
SCALE_HD bool scale_lane_next(int n, int stride, int& i, int& j) {
  j += stride;
  while (j >= n) {
    ++i;
    if (i >= n - 1) return false;
    j = j - n + i + 1;
  }
  return true;
}

// the eight numbers of a group from its reduced statistics and coordinate sums
SCALE_HD void scale_write(double* out, const ScaleAcc& a, double cx, double cy, double cz, int n) {
  out[0] = a.s1;
  out[1] = a.s2;
  out[2] = a.mx;
  out[3] = a.dref;
  out[4] = cx / (double)n;
  out[5] = cy / (double)n;
  out[6] = cz / (double)n;
  out[7] = (double)(((int64_t)n * (int64_t)(n - 1)) / 2);
}

// a whole group on one thread (the path of n <= SCALE_SMALL_MAX; also n < 2: zeros)
SCALE_HD void scale_group_serial(const double* __restrict__ world, const int64_t* __restrict__ ew, const double* __restrict__ eo, int n,
                                 double* __restrict__ out) {
  if (n < 2) {
    for (int k = 0; k < SCALE_NSTAT; ++k) out[k] = 0.0;
    return;
  }
  ScaleAcc a;
  scale_acc_zero(a);
  double cx = 0.0, cy = 0.0, cz = 0.0;
  for (int i = 0; i < n; ++i) {
    const double* wi = world + 3 * ew[i];
    const double wix = wi[0], wiy = wi[1], wiz = wi[2];
    const double oix = eo[3 * i], oiy = eo[3 * i + 1], oiz = eo[3 * i + 2];
    cx += wix; cy += wiy; cz += wiz;
    for (int j = i + 1; j < n; ++j) {
      const double* wj = world + 3 * ew[j];
      scale_pair(a, wix, wiy, wiz, wj[0], wj[1], wj[2], oix, oiy, oiz, eo[3 * j], eo[3 * j + 1], eo[3 * j + 2]);
    }
  }
  scale_write(out, a, cx, cy, cz, n);
}

}  // namespace cba

// ---- host side: checks and binning -------------------------------------------------------------------------------------------
#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

namespace cba {

// Which groups go where.  small: groups of n <= SCALE_SMALL_MAX sorted by n (stable), one per thread.  lds_small / lds_large /
// direct: the workgroup path by stage size, each list largest group first (stable) so that the long ones start early.
struct ScalePlan {
  std::vector<int64_t> small, lds_small, lds_large, direct;
};

// 0, or the negative code the call returns with `msg` set (-1 CBA_ERR_INVALID, -4 CBA_ERR_UNSUPPORTED)
inline int scale_plan(int64_t n_world, int64_t n_groups, const int64_t* group_start, const int64_t* ent_world, ScalePlan& plan,
                      std::string& msg) {
  if (group_start[0] != 0) { msg = "cba_scale_errors: group_start[0] != 0"; return -1; }
  for (int64_t g = 0; g < n_groups; ++g)
    if (group_start[g + 1] < group_start[g]) { msg = "cba_scale_errors: group_start decreases at group " + std::to_string(g); return -1; }
  const int64_t n_ent = group_start[n_groups];
  for (int64_t e = 0; e < n_ent; ++e)
    if (ent_world[e] < 0 || ent_world[e] >= n_world) {
      msg = "cba_scale_errors: entry " + std::to_string(e) + ": world row " + std::to_string(ent_world[e]) + " out of range [0, " +
            std::to_string(n_world) + ")";
      return -1;
    }
  for (int64_t g = 0; g < n_groups; ++g) {
    const int64_t n = group_start[g + 1] - group_start[g];
    if (n > SCALE_MAX_GROUP) {
      msg = "cba_scale_errors: group " + std::to_string(g) + " has " + std::to_string(n) + " entries; at most " +
            std::to_string(SCALE_MAX_GROUP) + " are supported";
      return -4;
    }
    (n <= SCALE_SMALL_MAX ? plan.small : n <= SCALE_LDS_SMALL ? plan.lds_small : n <= SCALE_LDS_LARGE ? plan.lds_large : plan.direct).push_back(g);
  }
  auto size_of = [&](int64_t g) { return group_start[g + 1] - group_start[g]; };
  std::stable_sort(plan.small.begin(), plan.small.end(), [&](int64_t a, int64_t b) { return size_of(a) < size_of(b); });
  for (auto* v : {&plan.lds_small, &plan.lds_large, &plan.direct})
    std::stable_sort(v->begin(), v->end(), [&](int64_t a, int64_t b) { return size_of(a) > size_of(b); });
  return 0;
}

}  // namespace cba

// The device half of cba_scale_errors (scale_lib.hip): upload, launches, copy-back.  `list`: the group indices of the four bins one
// after the other (small | lds_small | lds_large | direct), `counts[4]` their lengths; every index has been checked.  The host half
// (cba_solve.cpp, plain C++) is also part of builds without device code, where this symbol is absent: hence weak.
#ifdef CALISCOPE_BA_H  // (the two halves include the public header first; the test harness of the arithmetic does not need it)
extern "C" int cba_scale_launch(const cba_scale_desc* d, int32_t device, const int64_t* list, const int64_t* counts, double* stats_out)
    __attribute__((weak));
#endif
