// CPU harness around caliscope_amd/csrc/report_math.h — TEST INFRASTRUCTURE (built by g++ in tests/report_native.py).
// It evaluates cba_reprojection_filter with the checks, the keys, the select step, the percentile and the query lists that
// report_lib.hip uses; the kernels' work runs serially (tile after tile, a tile's histograms kept apart and flushed as a workgroup
// does), so that the non-GPU suite can check it against a sort-based brute force and drive CaptureVolume.filter_outliers and
// reprojection_summary through their `_solver` hook.  It is not a CPU fallback: nothing in caliscope_amd/ loads it.
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "ba_math.h"
#include "report_math.h"

using namespace cba;

namespace {
std::string g_error;

// k_rep_hist + k_rep_refine, REP_PASSES times
void select_round(const RepQueries& q, int64_t n_obs, const double* err, const int32_t* obs_cam, std::vector<uint64_t>& found) {
  const int32_t nq = q.n();
  found.assign((size_t)nq, 0);
  if (nq == 0) return;
  std::vector<int64_t> rank = q.rank;
  std::vector<unsigned long long> hist((size_t)nq * REP_RADIX, 0);
  const bool lds = nq <= REP_LDS_QUERIES;
  std::vector<unsigned> tile_hist(lds ? (size_t)nq * REP_RADIX : 0);
  for (int pass = 0; pass < REP_PASSES; ++pass) {
    for (int64_t base = 0; base < n_obs; base += REP_TILE) {
      std::fill(tile_hist.begin(), tile_hist.end(), 0u);
      const int64_t end = base + REP_TILE < n_obs ? base + REP_TILE : n_obs;
      for (int64_t o = base; o < end; ++o) {
        const int32_t first = q.cam_qfirst.empty() ? 0 : q.cam_qfirst[(size_t)obs_cam[o]];
        if (first < 0) continue;
        const uint64_t key = rep_key(err[o]);
        const int digit = rep_digit(key, pass);
        for (int32_t j = 0; j < q.per_seg; ++j) {
          const int32_t k = first + j;
          if (!rep_matches(key, found[(size_t)k], pass)) continue;
          if (lds) ++tile_hist[(size_t)k * REP_RADIX + digit];
          else ++hist[(size_t)k * REP_RADIX + digit];
        }
      }
      for (size_t i = 0; i < tile_hist.size(); ++i) hist[i] += tile_hist[i];
    }
    for (int32_t k = 0; k < nq; ++k) {
      int digit;
      int64_t r;
      rep_refine(hist.data() + (size_t)k * REP_RADIX, rank[(size_t)k], digit, r);
      rank[(size_t)k] = r;
      found[(size_t)k] = (found[(size_t)k] << REP_DIGIT_BITS) | (uint64_t)digit;
      std::fill(hist.begin() + (size_t)k * REP_RADIX, hist.begin() + (size_t)(k + 1) * REP_RADIX, 0ull);
    }
  }
}

// k_rep_mask
void mask_round(int64_t n_obs, const double* err, const int32_t* obs_cam, const std::vector<double>& thr, std::vector<uint8_t>& keep, std::vector<int64_t>& kept) {
  std::fill(kept.begin(), kept.end(), (int64_t)0);
  for (int64_t o = 0; o < n_obs; ++o) {
    const bool k = rep_keep(err[o], thr[(size_t)obs_cam[o]]);
    keep[(size_t)o] = k ? 1 : 0;
    if (k) ++kept[(size_t)obs_cam[o]];
  }
}
}  // namespace

extern "C" {

const char* rh_last_error() { return g_error.c_str(); }

// REP_DIGIT_BITS, REP_RADIX, REP_PASSES, REP_BLOCK, REP_TILE, REP_LDS_QUERIES, REP_LDS_CAMS, REP_LDS_SUMS
void rh_constants(int32_t* out) {
  out[0] = REP_DIGIT_BITS; out[1] = REP_RADIX; out[2] = REP_PASSES; out[3] = REP_BLOCK; out[4] = REP_TILE; out[5] = REP_LDS_QUERIES;
  out[6] = REP_LDS_CAMS; out[7] = REP_LDS_SUMS;
}

double rh_interpolate(double a, double b, double g) { return rep_interpolate(a, b, g); }

void rh_rank_plan(int64_t n, double percentile, int64_t* lo_hi, double* g) {
  const RepRankPlan p = rep_rank_plan(n, percentile);
  lo_hi[0] = p.lo; lo_hi[1] = p.hi; *g = p.g;
}

// the rank-th smallest (0-based) of x[n] by the select
double rh_select(const double* x, int64_t n, int64_t rank) {
  RepQueries q;
  q.per_seg = 1;
  q.rank = {rank};
  q.seg = {-1};
  std::vector<uint64_t> found;
  select_round(q, n, x, nullptr, found);
  return rep_value(found[0]);
}

// numpy.percentile(x, 100 - percentile) by two select queries and rep_interpolate
double rh_percentile(const double* x, int64_t n, double percentile) {
  const std::vector<int64_t> none;
  const RepQueries q = rep_percentile_queries(none, n, CBA_REPORT_OVERALL, percentile);
  std::vector<uint64_t> found;
  select_round(q, n, x, nullptr, found);
  return rep_interpolate(rep_value(found[0]), rep_value(found[1]), rep_rank_plan(n, percentile).g);
}

// cba_reprojection_filter on the host: 0 or -1 (invalid) with rh_last_error() set
int rh_reprojection_filter(const cba_report_desc* d, cba_report_out* out) {
  if (!d || !out) { g_error = "cba_reprojection_filter: null argument"; return -1; }
  std::vector<int64_t> cam_rows;
  const int rc = rep_validate(d, cam_rows, g_error);
  if (rc) return rc;
  const int32_t n_cams = d->n_cams, n_groups = d->obs_group ? d->n_groups : 0;
  const int64_t n_obs = d->n_obs;
  const bool filter = d->mode != CBA_REPORT_STATS;
  // k_rep_cam_prep, k_rep_error
  std::vector<CamTab> tab;
  if (!d->err_in && n_obs > 0) {
    tab.resize((size_t)n_cams);
    for (int32_t c = 0; c < n_cams; ++c) {
      double xc[MAX_NC] = {0};
      for (int i = 0; i < 6; ++i) xc[i] = d->cam_pose[(size_t)c * 6 + i];
      cam_prepare(xc, d->cam_const + (size_t)c * CAM_CONST_STRIDE, d->cam_model[c], 6, &tab[(size_t)c], 0);
    }
  }
  std::vector<double> err((size_t)n_obs), cam_sum((size_t)n_cams, 0.0), grp_sum((size_t)n_groups, 0.0);
  std::vector<int64_t> cam_cnt((size_t)n_cams, 0), grp_cnt((size_t)n_groups, 0);
  double total = 0.0;
  int64_t n_bad = 0;
  for (int64_t o = 0; o < n_obs; ++o) {
    double e;
    if (d->err_in) {
      e = d->err_in[o];
    } else {
      const CamTab& c = tab[(size_t)d->obs_cam[o]];
      const int64_t p = d->obs_pt[o];
      double r[2];
      project_residual(c, d->points[3 * p], d->points[3 * p + 1], d->points[3 * p + 2], d->obs_uv[2 * o], d->obs_uv[2 * o + 1], r);
      const double ex = r[0] * c.fx0, ey = r[1] * c.fx0;
      e = std::sqrt(ex * ex + ey * ey);
      if (out->err_xy) { out->err_xy[2 * o] = ex; out->err_xy[2 * o + 1] = ey; }
    }
    err[(size_t)o] = e;
    if (out->err) out->err[o] = e;
    const double sq = e * e;
    total += sq;
    if (!rep_finite(e)) ++n_bad;
    cam_sum[(size_t)d->obs_cam[o]] += sq; ++cam_cnt[(size_t)d->obs_cam[o]];
    if (d->obs_group) { grp_sum[(size_t)d->obs_group[o]] += sq; ++grp_cnt[(size_t)d->obs_group[o]]; }
  }
  for (int32_t c = 0; c < n_cams; ++c) {
    if (out->cam_sumsq) out->cam_sumsq[c] = cam_sum[(size_t)c];
    if (out->cam_count) out->cam_count[c] = cam_cnt[(size_t)c];
  }
  for (int32_t g = 0; g < n_groups; ++g) {
    if (out->group_sumsq) out->group_sumsq[g] = grp_sum[(size_t)g];
    if (out->group_count) out->group_count[g] = grp_cnt[(size_t)g];
  }
  if (out->overall_sumsq) *out->overall_sumsq = total;
  if (out->n_nonfinite) *out->n_nonfinite = n_bad;
  if (!filter || n_bad != 0) return 0;
  std::vector<double> thr((size_t)n_cams, d->mode == CBA_REPORT_ABSOLUTE ? d->value : rep_inf());
  std::vector<int64_t> kept((size_t)n_cams, 0);
  std::vector<uint8_t> keep((size_t)n_obs);
  int32_t n_floor = 0;
  if (n_obs > 0 && n_cams > 0) {
    std::vector<uint64_t> found;
    if (d->mode == CBA_REPORT_PERCENTILE) {
      const RepQueries q = rep_percentile_queries(cam_rows, n_obs, d->scope, d->value);
      select_round(q, n_obs, err.data(), d->obs_cam, found);
      rep_percentile_thresholds(q, found, cam_rows, n_obs, d->scope, d->value, thr);
    }
    mask_round(n_obs, err.data(), d->obs_cam, thr, keep, kept);
    const RepQueries fq = rep_floor_queries(cam_rows, kept, d->min_per_camera);
    n_floor = fq.n();
    if (n_floor > 0) {
      select_round(fq, n_obs, err.data(), d->obs_cam, found);
      for (int32_t k = 0; k < n_floor; ++k) thr[(size_t)fq.seg[(size_t)k]] = rep_value(found[(size_t)k]);
      mask_round(n_obs, err.data(), d->obs_cam, thr, keep, kept);
    }
  }
  for (int64_t o = 0; o < n_obs; ++o)
    if (out->keep) out->keep[o] = keep[(size_t)o];
  for (int32_t c = 0; c < n_cams; ++c) {
    if (out->cam_threshold) out->cam_threshold[c] = thr[(size_t)c];
    if (out->cam_kept) out->cam_kept[c] = kept[(size_t)c];
  }
  if (out->n_floor_cams) *out->n_floor_cams = n_floor;
  return 0;
}

}
