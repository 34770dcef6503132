// CPU harness around caliscope_amd/csrc/coverage_math.h — TEST INFRASTRUCTURE (built by g++ in tests/coverage_native.py).
// It evaluates cba_coverage_counts with the checks, the bit layout and the enumeration of slabs, tile pairs and word chunks that
// coverage_lib.hip uses, mark and gram run serially (one "thread" after the other, the stage copied with the kernel's padded stride),
// so that the non-GPU suite can check it against a brute force and drive caliscope_amd.coverage_analysis through its `_solver` hook.
// It is not a CPU fallback: nothing in caliscope_amd/ loads it.
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "coverage_math.h"

using namespace cba;

namespace {
std::string g_error;
}

extern "C" {

const char* ch_last_error() { return g_error.c_str(); }

// COV_TILE, COV_BLOCK, COV_STAGE_WORDS, COV_LDS_STRIDE, COV_TARGET_WG, COV_MAX_CAMS
void ch_constants(int32_t* out) {
  out[0] = COV_TILE; out[1] = COV_BLOCK; out[2] = COV_STAGE_WORDS; out[3] = COV_LDS_STRIDE; out[4] = COV_TARGET_WG; out[5] = COV_MAX_CAMS;
}

// n_words, slab_words, n_slabs, stride, chunk_words, n_chunks, n_tiles, n_tile_pairs of a call
void ch_plan(int32_t n_cams, int64_t n_keys, int64_t slab_words, int64_t* out) {
  const CovPlan p = cov_plan(n_cams, n_keys, slab_words);
  out[0] = p.n_words; out[1] = p.slab_words; out[2] = p.n_slabs; out[3] = p.stride; out[4] = p.chunk_words; out[5] = p.n_chunks;
  out[6] = p.n_tiles; out[7] = p.n_tile_pairs;
}

void ch_tile_pair(int64_t p, int32_t n_tiles, int32_t* out) { cov_tile_pair(p, n_tiles, out[0], out[1]); }

// cba_coverage_counts on the host: 0, -1 (invalid) or -4 (unsupported) with ch_last_error() set
int ch_coverage_counts(int32_t n_cams, int64_t n_keys, int64_t n_obs, const int64_t* obs_key, const int32_t* obs_cam, int64_t slab_words,
                       int64_t* counts_out) {
  const int rc = cov_validate(n_cams, n_keys, n_obs, obs_key, obs_cam, slab_words, g_error);
  if (rc) return rc;
  if (n_cams == 0) return 0;
  const int64_t n_counts = (int64_t)n_cams * n_cams;
  for (int64_t e = 0; e < n_counts; ++e) counts_out[e] = 0;
  if (n_obs == 0) return 0;
  const CovPlan plan = cov_plan(n_cams, n_keys, slab_words);
  std::vector<uint64_t> bits((size_t)n_cams * plan.stride);
  std::vector<uint64_t> sa(COV_TILE * COV_LDS_STRIDE), sb(COV_TILE * COV_LDS_STRIDE);
  for (int64_t s = 0; s < plan.n_slabs; ++s) {
    const int64_t w0 = s * plan.slab_words;
    const int64_t w1 = w0 + plan.slab_words < plan.n_words ? w0 + plan.slab_words : plan.n_words;
    std::fill(bits.begin(), bits.end(), (uint64_t)0);
    for (int64_t o = 0; o < n_obs; ++o) {  // k_cov_mark
      int64_t index;
      uint64_t bit;
      if (cov_mark_target(obs_key[o], obs_cam[o], w0, w1, plan.stride, index, bit)) bits[index] |= bit;
    }
    for (int64_t p = 0; p < plan.n_tile_pairs; ++p)  // k_cov_gram: blockIdx.x = p, blockIdx.y = chunk
      for (int64_t chunk = 0; chunk < plan.n_chunks; ++chunk) {
        int32_t I, J;
        cov_tile_pair(p, plan.n_tiles, I, J);
        const int64_t c0 = chunk * plan.chunk_words;
        const int64_t c1 = c0 + plan.chunk_words < plan.stride ? c0 + plan.chunk_words : plan.stride;
        std::vector<int64_t> sum(COV_BLOCK, 0);
        for (int64_t w = c0; w < c1; w += COV_STAGE_WORDS) {
          for (int r = 0; r < COV_TILE; ++r)
            for (int col = 0; col < COV_STAGE_WORDS; ++col) {
              const int32_t ca = I * COV_TILE + r, cb = J * COV_TILE + r;
              sa[r * COV_LDS_STRIDE + col] = ca < n_cams ? bits[(size_t)ca * plan.stride + w + col] : 0;
              sb[r * COV_LDS_STRIDE + col] = cb < n_cams ? bits[(size_t)cb * plan.stride + w + col] : 0;
            }
          for (int t = 0; t < COV_BLOCK; ++t) sum[t] += cov_stage_sum(sa.data(), sb.data(), t / COV_TILE, t % COV_TILE, COV_LDS_STRIDE);
        }
        for (int t = 0; t < COV_BLOCK; ++t) {
          const int32_t i = I * COV_TILE + t / COV_TILE, j = J * COV_TILE + t % COV_TILE;
          if (sum[t] != 0 && i <= j && j < n_cams) counts_out[(int64_t)i * n_cams + j] += sum[t];
        }
      }
  }
  for (int64_t i = 0; i < n_cams; ++i)  // k_cov_mirror
    for (int64_t j = 0; j < i; ++j) counts_out[i * n_cams + j] = counts_out[j * n_cams + i];
  return 0;
}

}
