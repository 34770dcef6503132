// Bit layout, work enumeration and host-side checks of cba_coverage_counts (include/caliscope_coverage.h): counts[i][j] = number of
// observation keys seen by both camera i and camera j, the Gram matrix of the binary table keys x cameras.  Compiled by hipcc into
// the kernels and the entry point of coverage_lib.hip, and by g++ into tests/native/coverage_harness.cpp, which walks the same slabs,
// tile pairs and word chunks serially on the CPU.
//
// Bits.  Camera c owns a row of 64-bit words; key k is bit (k & 63) of word (k >> 6).  The key range is walked in slabs of at most
// `slab_words` words per row (cov_plan): the bit table of a slab holds n_cams rows of `stride` words, stride = slab_words rounded up to
// a multiple of COV_STAGE_WORDS, so that the Gram kernel stages whole word blocks without a column check (the padding stays zero).
//
// Work of the Gram kernel.  Cameras go in tiles of COV_TILE = 16; a workgroup of COV_BLOCK = 256 threads takes one pair of tiles
// (I <= J: upper triangle, cov_tile_pair turns the pair number into (I, J) by integer arithmetic) and one chunk of `chunk_words`
// words of the slab; thread t owns the camera pair (16 I + t / 16, 16 J + t % 16).  The chunk is a multiple of COV_STAGE_WORDS and
// chosen so that tile pairs x chunks reaches COV_TARGET_WG workgroups where the slab is long enough: a 4-camera rig has one tile pair,
// and only the split of the word range fills the chip.
//
// LDS.  A stage is COV_STAGE_WORDS = 64 words of each of the 2 x 16 rows, row stride COV_LDS_STRIDE = 65 words.  In the inner loop
// the 32 lanes of a half-wave read word w of 2 rows of tile I (two addresses, broadcast) and of 16 rows of tile J: row r of J starts at
// dword 130 r, bank 2 r (mod 64) + {0, 1}, so the 16 eight-byte reads fall on 32 different banks.  With a stride of 64 words all 16
// would start in bank 0.
//
// Every sum is an integer: the order of the atomic additions does not matter, two runs return the same matrix.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define CBA_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define CBA_HD inline
#endif

namespace cba {

constexpr int COV_TILE = 16;                  // cameras per tile
constexpr int COV_BLOCK = COV_TILE * COV_TILE;  // threads of a Gram workgroup: one per camera pair of the tile pair
constexpr int COV_STAGE_WORDS = 64;           // words of a row staged in LDS at a time
constexpr int COV_LDS_STRIDE = COV_STAGE_WORDS + 1;
constexpr int COV_MARK_BLOCK = 256;           // threads (= observations) of a mark workgroup
constexpr int COV_TARGET_WG = 1024;           // Gram workgroups to aim for (4 per CU of a 256-CU chip)
constexpr int COV_MAX_CAMS = 32768;           // 2048 tiles, 2 098 176 tile pairs; the matrix alone is 8 GiB there
constexpr int64_t COV_SLAB_BYTES = (int64_t)256 << 20;  // default size of the bit table of one slab

CBA_HD int64_t cov_key_word(int64_t key) { return key >> 6; }
CBA_HD uint64_t cov_key_bit(int64_t key) { return (uint64_t)1 << (key & 63); }
CBA_HD int64_t cov_round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

CBA_HD int cov_popcount(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(v);
#else
  return __builtin_popcountll(v);
#endif
}

// Where an observation goes in the bit table of the slab of words [w0, w1): false when it is skipped (camera -1: outside the
// caller's map; key in another slab), else the word index within the table and the bit.
CBA_HD bool cov_mark_target(int64_t key, int32_t cam, int64_t w0, int64_t w1, int64_t stride, int64_t& index, uint64_t& bit) {
  if (cam < 0) return false;
  const int64_t w = cov_key_word(key);
  if (w < w0 || w >= w1) return false;
  index = (int64_t)cam * stride + (w - w0);
  bit = cov_key_bit(key);
  return true;
}

CBA_HD int32_t cov_n_tiles(int32_t n_cams) { return (n_cams + COV_TILE - 1) / COV_TILE; }
CBA_HD int64_t cov_n_tile_pairs(int32_t n_tiles) { return (int64_t)n_tiles * (n_tiles + 1) / 2; }
// first pair number of tile row I: rows 0 .. I-1 hold n_tiles, n_tiles - 1, .. pairs
CBA_HD int64_t cov_tile_row_start(int32_t I, int32_t n_tiles) { return (int64_t)I * n_tiles - (int64_t)I * (I - 1) / 2; }

// Pair number p (rows (0,0) (0,1) .. (0,n-1) (1,1) ..) -> tiles I <= J.  The square root only proposes a row; the two loops make
// it the row whose range holds p, so the result is exact whatever the rounding of the root.
CBA_HD void cov_tile_pair(int64_t p, int32_t n_tiles, int32_t& I, int32_t& J) {
  const double b = 2.0 * n_tiles + 1.0;
  double disc = b * b - 8.0 * (double)p;
  if (disc < 0.0) disc = 0.0;
  int32_t r = (int32_t)((b - sqrt(disc)) * 0.5);
  if (r < 0) r = 0;
  if (r > n_tiles - 1) r = n_tiles - 1;
  while (r + 1 < n_tiles && cov_tile_row_start(r + 1, n_tiles) <= p) ++r;
  while (r > 0 && cov_tile_row_start(r, n_tiles) > p) --r;
  I = r;
  J = r + (int32_t)(p - cov_tile_row_start(r, n_tiles));
}

// The enumeration of one call: slabs over the words of a row, chunks over the words of a slab, tile pairs over the cameras.
struct CovPlan {
  int64_t n_words;      // ceil(n_keys / 64)
  int64_t slab_words;   // words of a row per slab (the last slab may hold fewer)
  int64_t n_slabs;
  int64_t stride;       // row stride of the bit table, a multiple of COV_STAGE_WORDS
  int64_t chunk_words;  // words of a row per Gram workgroup, a multiple of COV_STAGE_WORDS
  int64_t n_chunks;     // chunks that cover `stride`
  int32_t n_tiles;
  int64_t n_tile_pairs;
};

// `requested` = 0: as many words as keep the table of a slab at COV_SLAB_BYTES (at least one stage).
CBA_HD CovPlan cov_plan(int32_t n_cams, int64_t n_keys, int64_t requested) {
  CovPlan p;
  p.n_words = (n_keys + 63) >> 6;
  p.n_tiles = cov_n_tiles(n_cams);
  p.n_tile_pairs = cov_n_tile_pairs(p.n_tiles);
  int64_t slab = requested;
  if (slab <= 0) {
    slab = COV_SLAB_BYTES / 8 / (n_cams > 0 ? n_cams : 1) / COV_STAGE_WORDS * COV_STAGE_WORDS;
    if (slab < COV_STAGE_WORDS) slab = COV_STAGE_WORDS;
  }
  if (slab > p.n_words) slab = p.n_words;
  if (slab < 1) slab = 1;
  p.slab_words = slab;
  p.n_slabs = (p.n_words + slab - 1) / slab;
  p.stride = cov_round_up(slab, COV_STAGE_WORDS);
  const int64_t pairs = p.n_tile_pairs > 0 ? p.n_tile_pairs : 1;
  const int64_t want = (COV_TARGET_WG + pairs - 1) / pairs;  // chunks that would reach the target
  p.chunk_words = cov_round_up((p.stride + want - 1) / want, COV_STAGE_WORDS);
  p.n_chunks = (p.stride + p.chunk_words - 1) / p.chunk_words;
  return p;
}

// The sum of thread (ti, tj) over one stage: words [0, COV_STAGE_WORDS) of row ti of `a` and row tj of `b`, rows `stride` apart.
CBA_HD int64_t cov_stage_sum(const uint64_t* a, const uint64_t* b, int ti, int tj, int stride) {
  const uint64_t* ra = a + ti * stride;
  const uint64_t* rb = b + tj * stride;
  int s = 0;
#if defined(__HIPCC__)  // eight words in flight: unrolled all the way the kernel takes 179 registers instead of 46
#pragma unroll 8
#endif
  for (int w = 0; w < COV_STAGE_WORDS; ++w) s += cov_popcount(ra[w] & rb[w]);
  return s;
}

}  // namespace cba

// ---- host side: the checks the entry point makes before anything is launched ----------------------------------------------------
#include <string>

namespace cba {

// 0, or the negative code the call returns with `msg` set (-1 CBA_ERR_INVALID, -4 CBA_ERR_UNSUPPORTED)
inline int cov_validate(int32_t n_cams, int64_t n_keys, int64_t n_obs, const int64_t* obs_key, const int32_t* obs_cam, int64_t slab_words,
                        std::string& msg) {
  const std::string what = "cba_coverage_counts: ";
  if (n_cams < 0 || n_keys < 0 || n_obs < 0 || slab_words < 0) { msg = what + "negative size"; return -1; }
  if (n_obs > 0 && (!obs_key || !obs_cam)) { msg = what + "null argument"; return -1; }
  if (n_cams > COV_MAX_CAMS) {
    msg = what + std::to_string(n_cams) + " cameras; at most " + std::to_string(COV_MAX_CAMS) + " are supported";
    return -4;
  }
  for (int64_t o = 0; o < n_obs; ++o) {
    if (obs_cam[o] < -1 || obs_cam[o] >= n_cams) {
      msg = what + "observation " + std::to_string(o) + ": camera " + std::to_string(obs_cam[o]) + " out of range [-1, " + std::to_string(n_cams) + ")";
      return -1;
    }
    if (obs_key[o] < 0 || obs_key[o] >= n_keys) {
      msg = what + "observation " + std::to_string(o) + ": key " + std::to_string(obs_key[o]) + " out of range [0, " + std::to_string(n_keys) + ")";
      return -1;
    }
  }
  return 0;
}

}  // namespace cba
