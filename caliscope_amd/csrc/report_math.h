// Order keys, the radix select, the percentile of numpy's default method and the host-side checks of cba_reprojection_filter
// (include/caliscope_report.h).  Compiled by hipcc into the kernels and the entry point of report_lib.hip, and by g++ into
// tests/native/report_harness.cpp, which runs the same select, mask and floor logic in loops on the CPU.
//
// Keys.  A reprojection error is a non-negative finite double: its bit pattern, read as an unsigned 64-bit integer, orders like its
// value (rep_key; the sign bit is cleared, so that -0.0 is 0.0).  The k-th smallest error of a segment (a camera, or everything)
// is found most significant digit first: per pass every observation of the segment whose high bits equal the digits chosen so far
// (rep_matches) adds one to the histogram bin of its next digit (rep_digit), and rep_refine picks the bin that holds the rank and
// reduces the rank by the bins before it.  After REP_PASSES = 64 / REP_DIGIT_BITS passes the chosen digits are the key of the
// order statistic: bit-exact, whatever the order in which the observations arrived.
//
// Queries.  A select query is (segment, rank).  The percentile needs two per segment (the ranks either side of the virtual index,
// rep_rank_plan), the safety floor one per camera below it.  The histogram kernel keeps the histograms of up to REP_LDS_QUERIES
// queries in LDS per workgroup (REP_RADIX 32-bit bins each) and adds straight to global memory beyond.
//
// Threshold.  rep_interpolate restates numpy's `linear` method; it runs on the host between launches, and its product goes through
// a volatile so that no compiler contracts it into the sum (hipcc contracts by default, on the host too).
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/caliscope_report.h"

#ifndef CBA_HD
#if defined(__HIPCC__)
#define CBA_HD __host__ __device__ __forceinline__
#else
#define CBA_HD inline
#endif
#endif

namespace cba {

constexpr int REP_DIGIT_BITS = 8;
constexpr int REP_RADIX = 1 << REP_DIGIT_BITS;
constexpr int REP_PASSES = 64 / REP_DIGIT_BITS;
constexpr int REP_BLOCK = 256;        // threads of a workgroup
constexpr int REP_TILE = 1024;        // observations of a workgroup (REP_TILE / REP_BLOCK per thread, a block apart)
constexpr int REP_LDS_QUERIES = 32;   // select queries whose histograms a workgroup keeps in LDS (32 KiB)
constexpr int REP_LDS_CAMS = 64;      // cameras whose prepared tables the error kernel keeps in LDS (24 KiB)
constexpr int REP_LDS_SUMS = 1024;    // cameras, and groups, whose partial sums a workgroup keeps in LDS (12 KiB each)

CBA_HD uint64_t rep_key(double e) {
  uint64_t k;
  __builtin_memcpy(&k, &e, sizeof k);
  return k & 0x7fffffffffffffffull;
}

CBA_HD double rep_value(uint64_t key) {
  double e;
  __builtin_memcpy(&e, &key, sizeof e);
  return e;
}

CBA_HD int rep_shift(int pass) { return 64 - REP_DIGIT_BITS * (pass + 1); }
CBA_HD int rep_digit(uint64_t key, int pass) { return (int)((key >> rep_shift(pass)) & (uint64_t)(REP_RADIX - 1)); }
// `prefix`: the digits chosen in passes 0 .. pass-1, the first one highest
CBA_HD bool rep_matches(uint64_t key, uint64_t prefix, int pass) { return pass == 0 || (key >> (rep_shift(pass) + REP_DIGIT_BITS)) == prefix; }

// One refinement step: the bin that holds `rank` (0-based among the observations counted in `hist`) and the rank within it.  An
// empty histogram (a query nobody matched) leaves digit REP_RADIX - 1 and a rank nobody reads.
CBA_HD void rep_refine(const unsigned long long* hist, int64_t rank, int& digit, int64_t& new_rank) {
  // no early exit: the loads of the bins do not wait for each other
  int64_t before = 0, chosen_before = 0;
  int chosen = REP_RADIX - 1;
  bool found = false;
#if defined(__HIPCC__)
#pragma unroll 16
#endif
  for (int d = 0; d < REP_RADIX; ++d) {
    const int64_t h = (int64_t)hist[d];
    const bool hit = !found && rank < before + h;
    chosen = hit ? d : chosen;
    chosen_before = hit ? before : chosen_before;
    found = found || hit;
    before += h;
  }
  digit = chosen;
  new_rank = rank - chosen_before;
}

CBA_HD bool rep_keep(double e, double threshold) { return e <= threshold; }
CBA_HD bool rep_finite(double e) { return (rep_key(e) >> 52) != 0x7ffull; }

}  // namespace cba

// ---- host side: the rank plan, the interpolation, the checks and the query lists of a call ----------------------------------------
#include <limits>
#include <string>
#include <vector>

namespace cba {

// numpy.percentile(x, 100 - percentile), method "linear", of n values: ranks lo <= hi in the sorted segment and the weight g
struct RepRankPlan {
  int64_t lo, hi;
  double g;
};

inline RepRankPlan rep_rank_plan(int64_t n, double percentile) {
  const double q = 100.0 - percentile;
  const double v = (double)(n - 1) * (q / 100.0);
  double fl = std::floor(v);
  RepRankPlan p;
  p.g = v - fl;
  if (fl < 0.0) fl = 0.0;
  if (fl > (double)(n - 1)) fl = (double)(n - 1);
  p.lo = (int64_t)fl;
  p.hi = p.lo + 1 < n - 1 ? p.lo + 1 : n - 1;
  if (p.hi < p.lo) p.hi = p.lo;
  return p;
}

// a = s[lo], b = s[hi]: a + (b - a) g, b - (b - a)(1 - g) from g = 0.5 on, a where b == a; every product rounded before it is added
inline double rep_interpolate(double a, double b, double g) {
  volatile double d = b - a;
  if (d == 0.0) return a;
  if (g >= 0.5) {
    volatile double w = 1.0 - g;
    volatile double prod = d * w;
    return b - prod;
  }
  volatile double prod = d * g;
  return a + prod;
}

inline double rep_inf() { return std::numeric_limits<double>::infinity(); }

// 0, or CBA_ERR_INVALID with `msg` set; cam_rows[c] = observations of camera c
inline int rep_validate(const cba_report_desc* d, std::vector<int64_t>& cam_rows, std::string& msg) {
  const std::string what = "cba_reprojection_filter: ";
  if (!d) { msg = what + "null argument"; return -1; }
  if (d->n_cams < 0 || d->n_points < 0 || d->n_obs < 0 || d->n_groups < 0) { msg = what + "negative size"; return -1; }
  if (d->mode != CBA_REPORT_STATS && d->mode != CBA_REPORT_PERCENTILE && d->mode != CBA_REPORT_ABSOLUTE) {
    msg = what + "unknown mode " + std::to_string(d->mode);
    return -1;
  }
  if (d->mode != CBA_REPORT_STATS) {
    if (d->min_per_camera < 1) { msg = what + "min_per_camera must be >= 1, got " + std::to_string(d->min_per_camera); return -1; }
    if (d->mode == CBA_REPORT_PERCENTILE) {
      if (!(d->value > 0.0 && d->value <= 100.0)) { msg = what + "percentile must be in (0, 100]"; return -1; }
      if (d->scope != CBA_REPORT_PER_CAMERA && d->scope != CBA_REPORT_OVERALL) { msg = what + "unknown scope " + std::to_string(d->scope); return -1; }
    } else if (!(d->value > 0.0)) {
      msg = what + "max_pixels must be positive";
      return -1;
    }
  }
  cam_rows.assign((size_t)d->n_cams, 0);
  if (d->n_obs == 0) return 0;
  if (!d->obs_cam) { msg = what + "null argument"; return -1; }
  if (!d->err_in && (!d->obs_pt || !d->obs_uv || (d->n_cams > 0 && (!d->cam_model || !d->cam_const || !d->cam_pose)) || (d->n_points > 0 && !d->points))) {
    msg = what + "null argument";
    return -1;
  }
  if (!d->err_in)
    for (int32_t c = 0; c < d->n_cams; ++c)
      if (d->cam_model[c] != 0 && d->cam_model[c] != 1) {
        msg = what + "camera " + std::to_string(c) + ": unknown model " + std::to_string(d->cam_model[c]);
        return -1;
      }
  // (the message is put together only for the observation that fails: the loop runs over millions of rows)
  const auto where = [&](int64_t o) { return what + "observation " + std::to_string(o) + ": "; };
  const bool project = d->err_in == nullptr;
  for (int64_t o = 0; o < d->n_obs; ++o) {
    const int32_t cam = d->obs_cam[o];
    if (cam < 0 || cam >= d->n_cams) {
      msg = where(o) + "camera " + std::to_string(cam) + " out of range [0, " + std::to_string(d->n_cams) + ")";
      return -1;
    }
    if (project && (d->obs_pt[o] < 0 || d->obs_pt[o] >= d->n_points)) {
      msg = where(o) + "point " + std::to_string(d->obs_pt[o]) + " out of range [0, " + std::to_string(d->n_points) + ")";
      return -1;
    }
    if (d->obs_group && (d->obs_group[o] < 0 || d->obs_group[o] >= d->n_groups)) {
      msg = where(o) + "group " + std::to_string(d->obs_group[o]) + " out of range [0, " + std::to_string(d->n_groups) + ")";
      return -1;
    }
    if (!project && !(rep_finite(d->err_in[o]) && d->err_in[o] >= 0.0)) {
      msg = where(o) + "error " + std::to_string(d->err_in[o]) + " is not a finite non-negative number";
      return -1;
    }
    ++cam_rows[(size_t)cam];
  }
  return 0;
}

// The select queries of one round: rank[q] within segment seg[q]; cam_qfirst[c] = first query of camera c or -1 (empty for the
// "overall" scope, where every observation belongs to the queries 0 .. per_seg-1).
struct RepQueries {
  std::vector<int64_t> rank;
  std::vector<int32_t> seg;
  std::vector<int32_t> cam_qfirst;
  int32_t per_seg = 0;
  int32_t n() const { return (int32_t)rank.size(); }
};

// two queries (ranks lo, hi) per segment with rows
inline RepQueries rep_percentile_queries(const std::vector<int64_t>& cam_rows, int64_t n_obs, int32_t scope, double percentile) {
  RepQueries q;
  q.per_seg = 2;
  if (scope == CBA_REPORT_OVERALL) {
    const RepRankPlan p = rep_rank_plan(n_obs, percentile);
    q.rank = {p.lo, p.hi};
    q.seg = {-1, -1};
    return q;
  }
  q.cam_qfirst.assign(cam_rows.size(), -1);
  for (size_t c = 0; c < cam_rows.size(); ++c) {
    if (cam_rows[c] == 0) continue;
    const RepRankPlan p = rep_rank_plan(cam_rows[c], percentile);
    q.cam_qfirst[c] = q.n();
    q.rank.push_back(p.lo); q.rank.push_back(p.hi);
    q.seg.push_back((int32_t)c); q.seg.push_back((int32_t)c);
  }
  return q;
}

// thresholds per camera from the keys the queries of rep_percentile_queries found
inline void rep_percentile_thresholds(const RepQueries& q, const std::vector<uint64_t>& found, const std::vector<int64_t>& cam_rows, int64_t n_obs,
                                      int32_t scope, double percentile, std::vector<double>& thr) {
  thr.assign(cam_rows.size(), rep_inf());
  if (scope == CBA_REPORT_OVERALL) {
    const double t = rep_interpolate(rep_value(found[0]), rep_value(found[1]), rep_rank_plan(n_obs, percentile).g);
    for (double& v : thr) v = t;
    return;
  }
  for (size_t c = 0; c < cam_rows.size(); ++c) {
    const int32_t f = q.cam_qfirst[c];
    if (f >= 0) thr[c] = rep_interpolate(rep_value(found[(size_t)f]), rep_value(found[(size_t)f + 1]), rep_rank_plan(cam_rows[c], percentile).g);
  }
}

// one query (rank r - 1, r = min(min_per_camera, rows)) per camera that kept fewer than r
inline RepQueries rep_floor_queries(const std::vector<int64_t>& cam_rows, const std::vector<int64_t>& cam_kept, int64_t min_per_camera) {
  RepQueries q;
  q.per_seg = 1;
  q.cam_qfirst.assign(cam_rows.size(), -1);
  for (size_t c = 0; c < cam_rows.size(); ++c) {
    const int64_t r = min_per_camera < cam_rows[c] ? min_per_camera : cam_rows[c];
    if (cam_kept[c] >= r) continue;
    q.cam_qfirst[c] = q.n();
    q.rank.push_back(r - 1);
    q.seg.push_back((int32_t)c);
  }
  return q;
}

}  // namespace cba
