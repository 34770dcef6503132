// CPU harness around caliscope_amd/csrc/scale_math.h — TEST INFRASTRUCTURE (built by g++ in tests/scale_native.py).
// It evaluates cba_scale_errors with the arithmetic, the binning and the lane-to-pair mapping the kernels of scale_lib.hip use, every
// sum in the order of the kernels' reduction (a lane's pairs in its own order, shuffle-down tree per wave, the waves in sequence),
// so that the non-GPU suite can check it against scipy and drive the scale report through its `_solver` hook.  It is not a CPU
// fallback: nothing in caliscope_amd/ loads it.
#include <cstdint>
#include <string>
#include <vector>

#include "scale_math.h"

using namespace cba;

namespace {

std::string g_error;

// what k_scale_group computes for one group, lane by lane
void group_by_lanes(const double* world, const int64_t* ew, const double* eo, int n, double* out) {
  constexpr int T = SCALE_BLOCK;
  std::vector<ScaleAcc> acc(T);
  std::vector<double> c(3 * T, 0.0);
  for (int t = 0; t < T; ++t) {
    scale_acc_zero(acc[t]);
    for (int e = t; e < n; e += T)
      for (int k = 0; k < 3; ++k) c[3 * t + k] += world[3 * ew[e] + k];
    int i, j;
    bool more = scale_lane_first(n, t, i, j);
    while (more) {
      const double* wi = world + 3 * ew[i];
      const double* wj = world + 3 * ew[j];
      scale_pair(acc[t], wi[0], wi[1], wi[2], wj[0], wj[1], wj[2], eo[3 * i], eo[3 * i + 1], eo[3 * i + 2], eo[3 * j], eo[3 * j + 1], eo[3 * j + 2]);
      more = scale_lane_next(n, T, i, j);
    }
  }
  for (int w = 0; w < T / 64; ++w)  // shuffle-down 32, 16, .. 1 inside a wave
    for (int o = 32; o > 0; o >>= 1)
      for (int l = 0; l < o; ++l) {
        scale_acc_merge(acc[64 * w + l], acc[64 * w + l + o]);
        for (int k = 0; k < 3; ++k) c[3 * (64 * w + l) + k] += c[3 * (64 * w + l + o) + k];
      }
  for (int w = 1; w < T / 64; ++w) {  // lane 0 adds the other waves in sequence
    scale_acc_merge(acc[0], acc[64 * w]);
    for (int k = 0; k < 3; ++k) c[k] += c[3 * 64 * w + k];
  }
  scale_write(out, acc[0], c[0], c[1], c[2], n);
}

}  // namespace

extern "C" {

const char* sh_last_error() { return g_error.c_str(); }

// SCALE_SMALL_MAX, SCALE_LDS_SMALL, SCALE_LDS_LARGE, SCALE_MAX_GROUP, SCALE_BLOCK, SCALE_NSTAT
void sh_constants(int32_t* out) {
  out[0] = SCALE_SMALL_MAX; out[1] = SCALE_LDS_SMALL; out[2] = SCALE_LDS_LARGE; out[3] = SCALE_MAX_GROUP; out[4] = SCALE_BLOCK; out[5] = SCALE_NSTAT;
}

// the pairs lane `t` of `stride` visits in a group of n entries, in its order; returns how many (at most `cap` are written)
int64_t sh_lane_pairs(int32_t n, int32_t t, int32_t stride, int64_t cap, int32_t* out_i, int32_t* out_j) {
  int64_t k = 0;
  if (n < 2) return 0;
  int i, j;
  bool more = scale_lane_first(n, t, i, j);
  while (more) {
    if (k < cap) { out_i[k] = i; out_j[k] = j; }
    ++k;
    more = scale_lane_next(n, stride, i, j);
  }
  return k;
}

// cba_scale_errors on the host: 0, -1 (invalid) or -4 (unsupported) with sh_last_error() set.  bins_out [n_groups] (or null): the
// path each group took, 0 thread per group, 1 / 2 workgroup with the small / large stage, 3 workgroup without a stage.
int sh_scale_errors(int64_t n_world, const double* world, int64_t n_groups, const int64_t* group_start, const int64_t* ent_world,
                    const double* ent_obj, double* stats_out, int32_t* bins_out) {
  if (n_groups == 0) return 0;
  ScalePlan plan;
  const int rc = scale_plan(n_world, n_groups, group_start, ent_world, plan, g_error);
  if (rc) return rc;
  for (int64_t g : plan.small) {
    const int64_t a = group_start[g];
    scale_group_serial(world, ent_world + a, ent_obj + 3 * a, (int)(group_start[g + 1] - a), stats_out + SCALE_NSTAT * g);
    if (bins_out) bins_out[g] = 0;
  }
  int bin = 1;
  for (const auto* list : {&plan.lds_small, &plan.lds_large, &plan.direct}) {
    for (int64_t g : *list) {
      const int64_t a = group_start[g];
      group_by_lanes(world, ent_world + a, ent_obj + 3 * a, (int)(group_start[g + 1] - a), stats_out + SCALE_NSTAT * g);
      if (bins_out) bins_out[g] = bin;
    }
    ++bin;
  }
  return 0;
}

}
