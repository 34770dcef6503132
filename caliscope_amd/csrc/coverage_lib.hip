// cba_coverage_counts of libcaliscope_ba.so (C ABI: include/caliscope_coverage.h): how many observation keys every pair of cameras
// shares.  The bit layout and the enumeration of slabs, tile pairs and word chunks are coverage_math.h (shared with
// tests/native/coverage_harness.cpp); this file holds the three kernels and the entry point.
//
//   k_cov_mark    one thread per observation: atomicOr of the key's bit into the camera's row of the slab's bit table.  Rows arrive
//                 in any order, repeated rows set the same bit, camera -1 and keys of another slab are skipped.
//   k_cov_gram    one 256-thread workgroup per (pair of 16-camera tiles, upper triangle; chunk of the word range).  Per stage the
//                 64 words of the 2 x 16 rows go to LDS (row stride 65 words: the 16 rows a half-wave reads fall on different
//                 banks), each thread adds popcount(a & b) of its camera pair in a register, and at the end of the chunk adds the
//                 sum once to the 64-bit count of the pair (atomicAdd: chunks and slabs meet there; integers, so no order matters).
//   k_cov_mirror  counts[j][i] = counts[i][j] for i < j, once after the last slab.
//
// One upload per input array; memset, mark and gram per slab on the null stream; one copy-back; no host synchronisation in between.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/caliscope_coverage.h"
#include "coverage_math.h"
#include "device_call.h"

using namespace cba;

namespace {

__global__ void __launch_bounds__(COV_MARK_BLOCK)
k_cov_mark(int64_t n_obs, const int64_t* __restrict__ obs_key, const int32_t* __restrict__ obs_cam, int64_t w0, int64_t w1, int64_t stride,
           unsigned long long* __restrict__ bits) {
  const int64_t o = (int64_t)blockIdx.x * COV_MARK_BLOCK + threadIdx.x;
  if (o >= n_obs) return;
  int64_t index;
  uint64_t bit;
  if (cov_mark_target(obs_key[o], obs_cam[o], w0, w1, stride, index, bit)) atomicOr(bits + index, (unsigned long long)bit);
}

__global__ void __launch_bounds__(COV_BLOCK)
k_cov_gram(int32_t n_cams, int32_t n_tiles, int64_t stride, int64_t chunk_words, const uint64_t* __restrict__ bits,
           unsigned long long* __restrict__ counts) {
  __shared__ uint64_t sa[COV_TILE * COV_LDS_STRIDE];
  __shared__ uint64_t sb[COV_TILE * COV_LDS_STRIDE];
  int32_t I, J;
  cov_tile_pair(blockIdx.x, n_tiles, I, J);
  const int t = threadIdx.x;
  const int ti = t / COV_TILE, tj = t % COV_TILE;
  const int64_t c0 = (int64_t)blockIdx.y * chunk_words;
  const int64_t c1 = c0 + chunk_words < stride ? c0 + chunk_words : stride;  // both multiples of COV_STAGE_WORDS
  int64_t sum = 0;
  for (int64_t w = c0; w < c1; w += COV_STAGE_WORDS) {
    // 16 rows x 64 words per tile: a wave loads one row, 512 contiguous bytes; rows past the last camera read as zero
#pragma unroll
    for (int k = 0; k < COV_TILE * COV_STAGE_WORDS / COV_BLOCK; ++k) {
      const int e = t + k * COV_BLOCK;
      const int r = e / COV_STAGE_WORDS, col = e % COV_STAGE_WORDS;
      const int32_t ca = I * COV_TILE + r, cb = J * COV_TILE + r;
      sa[r * COV_LDS_STRIDE + col] = ca < n_cams ? bits[(int64_t)ca * stride + w + col] : 0;
      sb[r * COV_LDS_STRIDE + col] = cb < n_cams ? bits[(int64_t)cb * stride + w + col] : 0;
    }
    __syncthreads();
    sum += cov_stage_sum(sa, sb, ti, tj, COV_LDS_STRIDE);
    __syncthreads();
  }
  const int32_t i = I * COV_TILE + ti, j = J * COV_TILE + tj;
  if (sum != 0 && i <= j && j < n_cams) atomicAdd(counts + (int64_t)i * n_cams + j, (unsigned long long)sum);
}

__global__ void __launch_bounds__(256)
k_cov_mirror(int32_t n_cams, int64_t* __restrict__ counts) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)n_cams * n_cams) return;
  const int64_t i = e / n_cams, j = e % n_cams;
  if (i > j) counts[e] = counts[j * n_cams + i];
}

}  // namespace

extern "C" int cba_coverage_counts(const cba_coverage_desc* d, int32_t device, int64_t* counts_out) {
  const char* what = "cba_coverage_counts";
  if (!d) return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  // every index the kernels use, checked on the host before anything reaches the device
  std::string msg;
  int rc = cov_validate(d->n_cams, d->n_keys, d->n_obs, d->obs_key, d->obs_cam, d->slab_words, msg);
  if (rc) return err(rc, msg);
  const int32_t n_cams = d->n_cams;
  const int64_t n_obs = d->n_obs;
  if (n_cams == 0) return CBA_OK;
  if (!counts_out) return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  const size_t n_counts = (size_t)n_cams * n_cams;
  if (n_obs == 0) {
    std::fill(counts_out, counts_out + n_counts, (int64_t)0);
    return CBA_OK;
  }
  const CovPlan plan = cov_plan(n_cams, d->n_keys, d->slab_words);
  rc = select_device(device, what);
  if (rc) return rc;
  Buffers buf;
  const int64_t* dkey = buf.in(d->obs_key, n_obs);
  const int32_t* dcam = buf.in(d->obs_cam, n_obs);
  uint64_t* dbits = buf.make<uint64_t>(n_cams, plan.stride);
  int64_t* dcounts = buf.make<int64_t>(n_counts);
  if (buf.status()) return buf.result(what);
  // the 64-bit atomics are declared on unsigned long long: the same words as uint64_t / int64_t under another name
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "bit words and counts are passed as unsigned long long");
  unsigned long long* dbits_atomic = (unsigned long long*)dbits;
  unsigned long long* dcounts_atomic = (unsigned long long*)dcounts;
  const size_t bits_bytes = (size_t)n_cams * (size_t)plan.stride * sizeof(uint64_t);
  hipError_t e = hipMemsetAsync(dcounts, 0, n_counts * sizeof(int64_t), 0);
  const dim3 mark_grid((unsigned)((n_obs + COV_MARK_BLOCK - 1) / COV_MARK_BLOCK));
  const dim3 gram_grid((unsigned)plan.n_tile_pairs, (unsigned)plan.n_chunks);
  for (int64_t s = 0; s < plan.n_slabs && e == hipSuccess; ++s) {
    const int64_t w0 = s * plan.slab_words;
    const int64_t w1 = w0 + plan.slab_words < plan.n_words ? w0 + plan.slab_words : plan.n_words;
    e = hipMemsetAsync(dbits, 0, bits_bytes, 0);
    if (e != hipSuccess) break;
    hipLaunchKernelGGL(k_cov_mark, mark_grid, dim3(COV_MARK_BLOCK), 0, 0, n_obs, dkey, dcam, w0, w1, plan.stride, dbits_atomic);
    hipLaunchKernelGGL(k_cov_gram, gram_grid, dim3(COV_BLOCK), 0, 0, n_cams, plan.n_tiles, plan.stride, plan.chunk_words, dbits, dcounts_atomic);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_cov_mirror, dim3((unsigned)((n_counts + 255) / 256)), dim3(256), 0, 0, n_cams, dcounts);
    e = hipGetLastError();
  }
  buf.check(e);
  buf.out(counts_out, dcounts, n_counts);
  return buf.result(what);
}
