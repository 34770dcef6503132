// Pose-bootstrap kernels of libcaliscope_ba.so (C ABI: include/caliscope_pose.h).  The arithmetic is pnp_math.h; this file
// holds the two launches and their host side.
//
//   k_pose_pnp        one thread per board view: undistort the view's observations (ba_math.h undistort_one, the routine
//                     of cba_triangulate) into a device buffer, then pnp_view on them.  Threads take views in the order
//                     `order` gives (views sorted by point count on the host), so that the lanes of a wave run loops of
//                     similar length; results are written at the view's own index.
//   k_pose_pair_rmse  one 256-thread workgroup per camera pair: each thread sums pair_obs_sq over a strided slice of the
//                     pair's observations, then a fixed shuffle + LDS tree: deterministic, no atomics.
//
// Both kernels are FP64 VALU with per-thread matrices of at most 66 doubles (the 11 x 11 DLT normal matrix), fully
// unrolled so that they stay in registers: hipcc -Rpass-analysis=kernel-resource-usage reports ScratchSize 0 for both.
//
// The epipolar bootstrap (arithmetic: epipolar_math.h) adds two calls of three steps each, RANSAC over many jobs at once:
//
//   k_epi_undistort   one thread per observation row: undistort_one once, however many pairs the row belongs to.
//   k_epi_hyp         one thread per (pair, hypothesis): 8 distinct correspondences from the counter-based sampler, linear
//   k_res_hyp         8-point E projected onto the manifold (9 doubles) / one thread per (job, hypothesis): 6-point DLT pose
//                     (12 doubles).  An invalid hypothesis is all zeros / NaN and scores no inlier.
//   k_score<ESS>      a 2-D grid: x = tiles of SCORE_BLOCK * SCORE_PER_LANE items of one job, y = jobs, so that one large
//                     pair (the 2-camera case) still fills the chip.  Hypotheses are staged in LDS SCORE_CHUNK at a time;
//                     each lane tests its items, each wave counts inliers by ballot + popcount and adds them with one
//                     integer atomic per wave per hypothesis.  Integer sums do not depend on order: counts are deterministic.
//   k_epi_refine      one REFINE_BLOCK workgroup per pair / job: the winner is the maximum count, the lowest hypothesis
//   k_res_refine      on ties; then the inlier flags, cheirality (essential), Levenberg-Marquardt whose normal equations
//                     are summed by a fixed LDS tree (wg_sum: the same order in tests/native/epipolar_harness.cpp), the
//                     final flags, counts, conditioning, two-view points / reprojection errors.
//
// The intrinsic calibration (arithmetic: intrinsic_math.h) is one call of two launches:
//
//   k_pose_pnp        as above, with the START intrinsics of every camera: the start pose of every view.
//   k_intrinsics      one REFINE_BLOCK workgroup per camera, the whole Levenberg-Marquardt loop of intr_calibrate in one launch.
//                     Threads stride over the camera's views (handed out sorted by corner count): a thread linearises a view,
//                     eliminates its 6 x 6 pose block in registers and adds the view's part of the reduced NI x NI system to its
//                     partial; wg_sum of the NI (NI + 1) / 2 + NI + 1 partials in a fixed order; every thread solves the reduced
//                     system redundantly, back-substitutes its own views and evaluates their trial cost.  Per-view pose, trial
//                     pose and the A_v^-1 terms live in a global work array (INTR_WORK doubles per view; each thread touches only
//                     the rows of its own views, so no barrier guards them).  No atomics: bit-identical from run to run.
//
// The frame selection of the intrinsic calibration (arithmetic: frame_select_math.h) is one call of two launches; the per-frame
// features stay on the device between them:
//
//   k_frame_features  one thread per frame, frames handed out sorted by corner count as k_pose_pnp's views: cell mask, pose features,
//                     then the homography of the frame's subrange (8 x 8 normal equations and the Levenberg-Marquardt polish in
//                     registers) and the orientation features read off it.
//   k_frame_select    one SELECT_BLOCK workgroup per camera, fsel_select: threads stride over the camera's frames; every anchor bin
//                     and every greedy round is one value per frame and one workgroup argmax over (value, -frame): shuffles inside
//                     a wave, then LDS across the waves, every thread reads the winner.  The running distance to the nearest
//                     selected frame lives in a device array of n_frames doubles; a frame's entry is only ever touched by the one
//                     thread that strides over it.  No atomics, fixed order: bit-identical from run to run.
//                     k_frame_features: 236 VGPRs, ScratchSize 0 (a trial step evaluates the cost alone, so one normal matrix and
//                     its damped copy are live); k_frame_select: 49 VGPRs, ScratchSize 0.
//
// No host synchronisation inside a call beyond the final copy-back.  The epipolar workgroup kernels keep one LDS reduction buffer
// of EPI_LIN_NSUM x REFINE_BLOCK doubles (46 KiB), k_intrinsics one of INTR_NSUM_MAX x REFINE_BLOCK doubles (55 KiB).  The largest
// per-thread matrices of the bootstrap kernels are the 9 x 8 Householder factor (k_epi_hyp) and the 11 x 11 DLT normal matrix
// (k_res_hyp), fully unrolled: ScratchSize 0 for each of them.  k_intrinsics fills the register file (256 VGPRs + 228 AGPRs, no VGPR
// spill) and has 24 bytes of scratch per lane: one store and two loads per corner in its fisheye instance (the stores of the lens's
// `r > 1e-8` branches, merged into one through a selected address); its pinhole instance has none in the corner loops
// (INTEGRATION.md section 3d).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <numeric>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/caliscope_pose.h"
#include "device_call.h"
#include "epipolar_math.h"
#include "frame_select_math.h"
#include "intrinsic_math.h"

using namespace cba;

// The kernels take CSR offsets and counts as long, the C ABI as int64_t.  Where the two are one type the buffers of a call go to the
// launches as they are; anywhere else this file must not compile.
static_assert(std::is_same<long, int64_t>::value, "CSR offsets are passed as long");

namespace {

constexpr int POSE_BLOCK = 64;   // one wave: views differ in cost, small groups keep the tail short
constexpr int PAIR_BLOCK = 256;

__global__ void __launch_bounds__(POSE_BLOCK)
k_pose_pnp(long n_views, const long* __restrict__ order, const long* __restrict__ view_start, const int* __restrict__ view_cam,
           const int* __restrict__ cam_model, const double* __restrict__ cam_intr, const double* __restrict__ obs_xy,
           const double* __restrict__ obs_obj, int min_points, int f32, double* __restrict__ und, double* __restrict__ pose,
           double* __restrict__ rmse, int* __restrict__ status) {
  const long q = (long)blockIdx.x * POSE_BLOCK + threadIdx.x;
  if (q >= n_views) return;
  const long v = order[q];
  const long a = view_start[v], b = view_start[v + 1];
  const int c = view_cam[v];
  const int model = cam_model[c];
  const double* in9 = cam_intr + 9 * c;
  for (long i = a; i < b; ++i) {
    double x, y;
    undistort_one(model, in9, obs_xy[2 * i], obs_xy[2 * i + 1], f32, &x, &y);
    und[2 * i] = x;
    und[2 * i + 1] = y;
  }
  double R[9], t[3], r;
  const int st = pnp_view(obs_obj + 3 * a, und + 2 * a, (int)(b - a), min_points, f32, R, t, &r);
#pragma unroll
  for (int k = 0; k < 9; ++k) pose[12 * v + k] = R[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) pose[12 * v + 9 + k] = t[k];
  rmse[v] = r;
  status[v] = st;
}

__global__ void __launch_bounds__(PAIR_BLOCK)
k_pose_pair_rmse(const double* __restrict__ pair_pose, const long* __restrict__ pair_start, const double* __restrict__ obs_a,
                 const double* __restrict__ obs_b, double* __restrict__ rmse, long* __restrict__ count) {
  __shared__ double part[PAIR_BLOCK / 64];
  const long p = blockIdx.x;
  const long a = pair_start[p], b = pair_start[p + 1];
  double rt[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) rt[k] = pair_pose[12 * p + k];
  double s = 0.0;
  for (long i = a + threadIdx.x; i < b; i += PAIR_BLOCK) s += pair_obs_sq(rt, obs_a[2 * i], obs_a[2 * i + 1], obs_b[2 * i], obs_b[2 * i + 1]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < PAIR_BLOCK / 64; ++w) tot += part[w];
    const long m = b - a;
    rmse[p] = m > 0 ? sqrt(tot / (2.0 * (double)m)) : 0.0;
    count[p] = m;
  }
}

// ---- epipolar bootstrap ------------------------------------------------------------------------------------------------------

constexpr int HYP_BLOCK = 64;
constexpr int SCORE_BLOCK = 256;
constexpr int SCORE_PER_LANE = 4;
constexpr int SCORE_CHUNK = 128;
constexpr int REFINE_BLOCK = EPI_REDUCE_NT;

__global__ void __launch_bounds__(SCORE_BLOCK)
k_epi_undistort(long n_obs, const int* __restrict__ obs_cam, const int* __restrict__ cam_model, const double* __restrict__ cam_intr,
                const double* __restrict__ obs_xy, int f32, double* __restrict__ und) {
  const long i = (long)blockIdx.x * SCORE_BLOCK + threadIdx.x;
  if (i >= n_obs) return;
  const int c = obs_cam[i];
  double x, y;
  undistort_one(cam_model[c], cam_intr + 9 * c, obs_xy[2 * i], obs_xy[2 * i + 1], f32, &x, &y);
  und[2 * i] = x;
  und[2 * i + 1] = y;
}

__device__ __forceinline__ void epi_corr(const double* __restrict__ und, const long* __restrict__ ca, const long* __restrict__ cb, long i,
                                         double* c) {
  const long a = ca[i], b = cb[i];
  c[0] = und[2 * a]; c[1] = und[2 * a + 1]; c[2] = und[2 * b]; c[3] = und[2 * b + 1];
}

__global__ void __launch_bounds__(HYP_BLOCK)
k_epi_hyp(long n_pairs, int n_hyp, unsigned long long seed, const long* __restrict__ start, const long* __restrict__ ca,
          const long* __restrict__ cb, const double* __restrict__ und, double* __restrict__ hyp) {
  const long q = (long)blockIdx.x * HYP_BLOCK + threadIdx.x;
  if (q >= n_pairs * n_hyp) return;
  const long p = q / n_hyp, h = q - p * n_hyp;
  const long s = start[p], n = start[p + 1] - s;
  double E[9];
  if (n < EPI_SAMPLE) {
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = 0.0;
  } else {
    int64_t idx[EPI_SAMPLE];
    sample_distinct<EPI_SAMPLE>(seed, p, h, n, idx);
    double c[EPI_SAMPLE][4];
#pragma unroll
    for (int k = 0; k < EPI_SAMPLE; ++k) epi_corr(und, ca, cb, s + idx[k], c[k]);
    essential_hypothesis(c, E);
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) hyp[9 * q + k] = E[k];
}

__global__ void __launch_bounds__(HYP_BLOCK)
k_res_hyp(long n_jobs, int n_hyp, int min_points, unsigned long long seed, const long* __restrict__ start, const double* __restrict__ obj,
          const double* __restrict__ uv, double* __restrict__ hyp) {
  const long q = (long)blockIdx.x * HYP_BLOCK + threadIdx.x;
  if (q >= n_jobs * n_hyp) return;
  const long j = q / n_hyp, h = q - j * n_hyp;
  const long s = start[j], n = start[j + 1] - s;
  double R[9], t[3];
  bool ok = false;
  if (n >= RES_SAMPLE && n >= min_points) {
    int64_t idx[RES_SAMPLE];
    sample_distinct<RES_SAMPLE>(seed, j, h, n, idx);
    double P[RES_SAMPLE][5];
#pragma unroll
    for (int k = 0; k < RES_SAMPLE; ++k) {
      const long i = s + idx[k];
      P[k][0] = obj[3 * i]; P[k][1] = obj[3 * i + 1]; P[k][2] = obj[3 * i + 2]; P[k][3] = uv[2 * i]; P[k][4] = uv[2 * i + 1];
    }
    ok = res_hypothesis(P, R, t);
  }
  const double nan = __builtin_nan("");
#pragma unroll
  for (int k = 0; k < 9; ++k) hyp[12 * q + k] = ok ? R[k] : nan;
#pragma unroll
  for (int k = 0; k < 3; ++k) hyp[12 * q + 9 + k] = ok ? t[k] : nan;
}

// ESS: items are correspondences (ca, cb into und), hypotheses E[9]; otherwise items are (obj, uv) points, hypotheses [R | t].
template <bool ESS>
__global__ void __launch_bounds__(SCORE_BLOCK)
k_score(long n_jobs, int n_hyp, const long* __restrict__ start, const long* __restrict__ ca, const long* __restrict__ cb,
        const double* __restrict__ und, const double* __restrict__ obj, const double* __restrict__ uv, const double* __restrict__ thr,
        const double* __restrict__ hyp, unsigned* __restrict__ count) {
  constexpr int HW = ESS ? 9 : 12;
  constexpr int TILE = SCORE_BLOCK * SCORE_PER_LANE;
  __shared__ double sh[SCORE_CHUNK * HW];
  const int tid = threadIdx.x, lane = tid & 63;
  for (long j = blockIdx.y; j < n_jobs; j += gridDim.y) {
    const long s = start[j], e = start[j + 1];
    const long base = s + (long)blockIdx.x * TILE;
    if (base >= e) continue;  // (uniform over the workgroup)
    const double thr2 = thr[j] * thr[j];
    double it[SCORE_PER_LANE][5];
    bool valid[SCORE_PER_LANE];
#pragma unroll
    for (int c = 0; c < SCORE_PER_LANE; ++c) {
      const long i = base + c * SCORE_BLOCK + tid;
      valid[c] = i < e;
      const long ii = valid[c] ? i : s;
      if (ESS) {
        epi_corr(und, ca, cb, ii, it[c]);
        it[c][4] = 0.0;
      } else {
        it[c][0] = obj[3 * ii]; it[c][1] = obj[3 * ii + 1]; it[c][2] = obj[3 * ii + 2]; it[c][3] = uv[2 * ii]; it[c][4] = uv[2 * ii + 1];
      }
    }
    for (int h0 = 0; h0 < n_hyp; h0 += SCORE_CHUNK) {
      const int nh = min(SCORE_CHUNK, n_hyp - h0);
      __syncthreads();
      for (int k = tid; k < nh * HW; k += SCORE_BLOCK) sh[k] = hyp[((long)j * n_hyp + h0) * HW + k];
      __syncthreads();
      for (int h = 0; h < nh; ++h) {
        const double* H = sh + h * HW;
        unsigned cnt = 0;
#pragma unroll
        for (int c = 0; c < SCORE_PER_LANE; ++c) {
          bool in;
          if (ESS) in = valid[c] && epi_sampson(H, it[c][0], it[c][1], it[c][2], it[c][3]) <= thr2;
          else in = valid[c] && res_err2(H, H + 9, it[c], it[c][3], it[c][4]) <= thr2;
          cnt += (unsigned)__popcll(__ballot(in));
        }
        if (lane == 0 && cnt) atomicAdd(&count[(long)j * n_hyp + h0 + h], cnt);
      }
    }
    __syncthreads();
  }
}

// Fixed-order workgroup sum of K values per thread (the tree of epipolar_math.h EPI_REDUCE_NT); every thread gets the result.
template <int K>
__device__ __forceinline__ void wg_sum(const double* acc, double (*red)[REFINE_BLOCK], double* out) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < K; ++k) red[k][tid] = acc[k];
  __syncthreads();
#pragma unroll
  for (int s = REFINE_BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int k = 0; k < K; ++k) red[k][tid] += red[k][tid + s];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < K; ++k) out[k] = red[k][0];
  __syncthreads();
}

// winner: the maximum count, the lowest index on ties
__device__ __forceinline__ int wg_select(const unsigned* count, int n_hyp, unsigned* bc, int* bi, unsigned* best_count) {
  const int tid = threadIdx.x;
  unsigned c = 0;
  int b = -1;
  for (int h = tid; h < n_hyp; h += REFINE_BLOCK)
    if (b < 0 || count[h] > c) { c = count[h]; b = h; }
  bc[tid] = c; bi[tid] = b;
  __syncthreads();
  for (int s = REFINE_BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) {
      const unsigned c2 = bc[tid + s];
      const int b2 = bi[tid + s];
      if (b2 >= 0 && (bi[tid] < 0 || c2 > bc[tid] || (c2 == bc[tid] && b2 < bi[tid]))) { bc[tid] = c2; bi[tid] = b2; }
    }
    __syncthreads();
  }
  const int w = bi[0];
  *best_count = bc[0];
  __syncthreads();
  return w;
}

struct EpiSumDev {
  const double* und; const long* ca; const long* cb; const unsigned char* flag; long s, e;
  double (*red)[REFINE_BLOCK];
  __device__ void operator()(const double* R, const double* t, double* out) {
    double E[9], dE[5][9], acc[EPI_NSUM];
    essential_from_pose(R, t, E);
    essential_jacobian(R, t, dE);
#pragma unroll
    for (int k = 0; k < EPI_NSUM; ++k) acc[k] = 0.0;
    for (long i = s + threadIdx.x; i < e; i += REFINE_BLOCK)
      if (flag[i]) {
        double c[4];
        epi_corr(und, ca, cb, i, c);
        epi_sampson_normal(E, dE, c[0], c[1], c[2], c[3], acc);
      }
    wg_sum<EPI_NSUM>(acc, red, out);
  }
};

__global__ void __launch_bounds__(REFINE_BLOCK)
k_epi_refine(long n_pairs, int n_hyp, const long* __restrict__ start, const long* __restrict__ ca, const long* __restrict__ cb,
             const double* __restrict__ und, const double* __restrict__ thr, const double* __restrict__ hyp, const unsigned* __restrict__ count,
             double* __restrict__ pose, int* __restrict__ status, long* __restrict__ n_inl, long* __restrict__ n_chr, double* __restrict__ cond,
             int* __restrict__ winner, unsigned char* __restrict__ flag, double* __restrict__ xyz) {
  __shared__ double red[EPI_LIN_NSUM][REFINE_BLOCK];
  __shared__ unsigned bc[REFINE_BLOCK];
  __shared__ int bi[REFINE_BLOCK];
  __shared__ unsigned icnt[4];
  const long p = blockIdx.x;
  const int tid = threadIdx.x;
  const long s = start[p], e = start[p + 1];
  const double thr2 = thr[p] * thr[p];
  const double nan = __builtin_nan("");
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
  int st = EPI_OK, w = -1;
  unsigned best = 0;
  if (e - s < EPI_SAMPLE) st = EPI_TOO_FEW;
  if (st == EPI_OK) {
    w = wg_select(count + p * n_hyp, n_hyp, bc, bi, &best);
    if (w < 0 || best < EPI_SAMPLE) st = EPI_FAILED;
  }
  double rt[4][12];
  if (st == EPI_OK) {
    const double* E = hyp + ((long)p * n_hyp + w) * 9;
    if (tid < 4) icnt[tid] = 0;
    // flags of the winner (each thread writes and later reads only its own items)
    for (long i = s + tid; i < e; i += REFINE_BLOCK) {
      double c[4];
      epi_corr(und, ca, cb, i, c);
      flag[i] = epi_sampson(E, c[0], c[1], c[2], c[3]) <= thr2 ? 1 : 0;
    }
    if (!essential_candidates(E, rt)) st = EPI_FAILED;
  }
  if (st == EPI_OK) {
    unsigned mine[4] = {0, 0, 0, 0};
    for (long i = s + tid; i < e; i += REFINE_BLOCK)
      if (flag[i]) {
        double c[4], wv[4];
        epi_corr(und, ca, cb, i, c);
#pragma unroll
        for (int k = 0; k < 4; ++k) mine[k] += epi_in_front(rt[k], c[0], c[1], c[2], c[3], wv) ? 1u : 0u;
      }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) if (mine[k]) atomicAdd(&icnt[k], mine[k]);
    __syncthreads();
    int kb = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k) if (icnt[k] > icnt[kb]) kb = k;
    // (selects, not rt[kb]: a dynamic index would send rt to scratch)
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const double v = kb == 0 ? rt[0][k] : kb == 1 ? rt[1][k] : kb == 2 ? rt[2][k] : rt[3][k];
      if (k < 9) R[k] = v; else t[k - 9] = v;
    }
    EpiSumDev sum{und, ca, cb, flag, s, e, red};
    if (!pnp_finite(epi_refine(sum, R, t))) st = EPI_FAILED;
    unsigned prev = best;
    for (int lo = 0; lo < EPI_LO_ROUNDS && st == EPI_OK; ++lo) {
      double Ec[9];
      essential_from_pose(R, t, Ec);
      __syncthreads();
      if (tid == 0) icnt[0] = 0;
      __syncthreads();
      unsigned m = 0;
      for (long i = s + tid; i < e; i += REFINE_BLOCK) {
        double c[4];
        epi_corr(und, ca, cb, i, c);
        const unsigned char f = epi_sampson(Ec, c[0], c[1], c[2], c[3]) <= thr2 ? 1 : 0;
        flag[i] = f;
        m += f;
      }
      if (m) atomicAdd(&icnt[0], m);
      __syncthreads();
      const unsigned cnt = icnt[0];
      if (cnt <= prev) break;
      prev = cnt;
      if (!pnp_finite(epi_refine(sum, R, t))) st = EPI_FAILED;
    }
  }
  if (st != EPI_OK) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    t[0] = t[1] = t[2] = 0.0;
  }
  // final flags, points, counts (a failed pair: all outliers)
  double Ef[9], rtf[12];
  essential_from_pose(R, t, Ef);
#pragma unroll
  for (int k = 0; k < 9; ++k) rtf[k] = R[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) rtf[9 + k] = t[k];
  __syncthreads();
  if (tid < 2) icnt[tid] = 0;
  __syncthreads();
  unsigned m1 = 0, m2 = 0;
  double lin[EPI_LIN_NSUM];
#pragma unroll
  for (int k = 0; k < EPI_LIN_NSUM; ++k) lin[k] = 0.0;
  for (long i = s + tid; i < e; i += REFINE_BLOCK) {
    double c[4], wv[4];
    epi_corr(und, ca, cb, i, c);
    unsigned char f = 0;
    double X = nan, Y = nan, Z = nan;
    if (st == EPI_OK && epi_sampson(Ef, c[0], c[1], c[2], c[3]) <= thr2) {
      f = 1;
      epi_linear_normal(c[0], c[1], c[2], c[3], lin);
      if (epi_in_front(rtf, c[0], c[1], c[2], c[3], wv)) {
        f = 2;
        if (fabs(wv[3]) > 1e-12) { X = wv[0] / wv[3]; Y = wv[1] / wv[3]; Z = wv[2] / wv[3]; }
      }
    }
    flag[i] = f;
    m1 += f >= 1;
    m2 += f == 2;
    if (xyz) { xyz[3 * i] = X; xyz[3 * i + 1] = Y; xyz[3 * i + 2] = Z; }
  }
  if (m1) atomicAdd(&icnt[0], m1);
  if (m2) atomicAdd(&icnt[1], m2);
  double N[EPI_LIN_NSUM];
  wg_sum<EPI_LIN_NSUM>(lin, red, N);  // (its barriers also publish icnt)
  if (tid == 0) {
    const double cd = st == EPI_OK ? epi_conditioning(N, Ef) : 0.0;
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[12 * p + k] = rtf[k];
    status[p] = st;
    n_inl[p] = icnt[0];
    n_chr[p] = icnt[1];
    cond[p] = cd;
    winner[p] = w;
  }
}

struct ResSumDev {
  const double* obj; const double* uv; const double* Rh; const double* th; double thr2; long s, e;
  double (*red)[REFINE_BLOCK];
  __device__ void operator()(const double* R, const double* t, double* out) {
    double acc[RES_NSUM];
#pragma unroll
    for (int k = 0; k < RES_NSUM; ++k) acc[k] = 0.0;
    for (long i = s + threadIdx.x; i < e; i += REFINE_BLOCK)
      if (res_err2(Rh, th, obj + 3 * i, uv[2 * i], uv[2 * i + 1]) <= thr2) res_point_normal(R, t, obj + 3 * i, uv[2 * i], uv[2 * i + 1], acc);
    wg_sum<RES_NSUM>(acc, red, out);
  }
};

__global__ void __launch_bounds__(REFINE_BLOCK)
k_res_refine(long n_jobs, int n_hyp, int min_points, const long* __restrict__ start, const double* __restrict__ obj, const double* __restrict__ uv,
             const double* __restrict__ thr, const double* __restrict__ hyp, const unsigned* __restrict__ count, double* __restrict__ pose,
             int* __restrict__ status, long* __restrict__ n_inl, int* __restrict__ winner, double* __restrict__ err_out) {
  __shared__ double red[RES_NSUM][REFINE_BLOCK];
  __shared__ unsigned bc[REFINE_BLOCK];
  __shared__ int bi[REFINE_BLOCK];
  __shared__ unsigned icnt;
  const long j = blockIdx.x;
  const int tid = threadIdx.x;
  const long s = start[j], e = start[j + 1];
  const double thr2 = thr[j] * thr[j];
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
  int st = EPI_OK, w = -1;
  unsigned best = 0;
  if (e - s < RES_SAMPLE || e - s < min_points) st = EPI_TOO_FEW;
  if (st == EPI_OK) {
    w = wg_select(count + j * n_hyp, n_hyp, bc, bi, &best);
    if (w < 0 || best < RES_SAMPLE) st = EPI_FAILED;
  }
  if (st == EPI_OK) {
    const double* H = hyp + ((long)j * n_hyp + w) * 12;
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = H[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = H[9 + k];
    ResSumDev sum{obj, uv, H, H + 9, thr2, s, e, red};
    const double cost = res_refine(sum, R, t);
    if (!pnp_finite(cost)) st = EPI_FAILED;
  }
  if (st != EPI_OK) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    t[0] = t[1] = t[2] = 0.0;
  }
  if (tid == 0) icnt = 0;
  __syncthreads();
  unsigned m = 0;
  for (long i = s + tid; i < e; i += REFINE_BLOCK) {
    m += (st == EPI_OK && res_err2(R, t, obj + 3 * i, uv[2 * i], uv[2 * i + 1]) <= thr2) ? 1u : 0u;
    err_out[i] = st == EPI_OK ? res_err(R, t, obj + 3 * i, uv[2 * i], uv[2 * i + 1]) : __builtin_nan("");
  }
  if (m) atomicAdd(&icnt, m);
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) pose[12 * j + k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) pose[12 * j + 9 + k] = t[k];
    status[j] = st;
    n_inl[j] = icnt;
    winner[j] = w;
  }
}

// ---- intrinsic calibration ---------------------------------------------------------------------------------------------------

// The functor of intr_calibrate on the device: the workgroup's threads stride over the camera's views.
template <int MODEL>
struct IntrSumDev {
  const long* views; long nv;
  const long* view_start; const double* xy; const double* obj; int f32;
  const double* pnp_pose; const int* pnp_status;
  double* work; int* vstat; double* pose_out; double* view_rmse;
  double (*red)[REFINE_BLOCK];
  __device__ int n_of(long v) const { return (int)(view_start[v + 1] - view_start[v]); }
  __device__ void screen(const double* in0, double* out) {
    double acc[2] = {0.0, 0.0};
    for (long q = threadIdx.x; q < nv; q += REFINE_BLOCK) {
      const long v = views[q], a = view_start[v];
      const int st = intr_view_screen<MODEL>(in0, obj + 3 * a, xy + 2 * a, n_of(v), f32, pnp_status[v], pnp_pose + 12 * v, work + v * INTR_WORK);
      vstat[v] = st;
      if (st == PNP_OK) { acc[0] += 1.0; acc[1] += (double)n_of(v); }
    }
    wg_sum<2>(acc, red, out);
  }
  __device__ void reduce(const double* in, double mu, double* out) {
    double acc[IntrDim<MODEL>::NSUM];
#pragma unroll
    for (int k = 0; k < IntrDim<MODEL>::NSUM; ++k) acc[k] = 0.0;
    for (long q = threadIdx.x; q < nv; q += REFINE_BLOCK) {
      const long v = views[q], a = view_start[v];
      if (vstat[v] == PNP_OK) intr_view_reduce<MODEL>(in, mu, obj + 3 * a, xy + 2 * a, n_of(v), f32, work + v * INTR_WORK, acc);
    }
    wg_sum<IntrDim<MODEL>::NSUM>(acc, red, out);
  }
  __device__ void trial(const double* in_new, const double* di, double* out) {
    double acc[2] = {0.0, 0.0};
    for (long q = threadIdx.x; q < nv; q += REFINE_BLOCK) {
      const long v = views[q], a = view_start[v];
      if (vstat[v] == PNP_OK) intr_view_trial<MODEL>(in_new, di, obj + 3 * a, xy + 2 * a, n_of(v), f32, work + v * INTR_WORK, acc);
    }
    wg_sum<2>(acc, red, out);
  }
  __device__ void accept() {
    for (long q = threadIdx.x; q < nv; q += REFINE_BLOCK)
      if (vstat[views[q]] == PNP_OK) intr_view_accept(work + views[q] * INTR_WORK);
  }
  __device__ void finish(const double* in, bool ok) {
    for (long q = threadIdx.x; q < nv; q += REFINE_BLOCK) {
      const long v = views[q], a = view_start[v];
      intr_view_finish<MODEL>(in, ok, obj + 3 * a, xy + 2 * a, n_of(v), f32, vstat[v], work + v * INTR_WORK, pose_out + 12 * v, view_rmse + v);
    }
  }
};

__global__ void __launch_bounds__(REFINE_BLOCK)
k_intrinsics(const int* __restrict__ cam_model, const double* __restrict__ cam_start, const long* __restrict__ cam_view_start,
             const long* __restrict__ cam_views, const long* __restrict__ view_start, const double* __restrict__ obs_xy,
             const double* __restrict__ obs_obj, int f32, int max_iter, const double* __restrict__ pnp_pose, const int* __restrict__ pnp_status,
             double* __restrict__ work, double* __restrict__ intr_out, double* __restrict__ rmse_out, int* __restrict__ status_out,
             int* __restrict__ iters_out, double* __restrict__ pose_out, double* __restrict__ view_rmse_out, int* __restrict__ view_status_out) {
  __shared__ double red[INTR_NSUM_MAX][REFINE_BLOCK];
  const int c = blockIdx.x;
  const long vs = cam_view_start[c], nv = cam_view_start[c + 1] - vs;
  double in9[9], rmse;
#pragma unroll
  for (int k = 0; k < 9; ++k) in9[k] = cam_start[9 * c + k];
  int st, it;
  if (cam_model[c] == MODEL_FISHEYE4) {  // (uniform over the workgroup)
    IntrSumDev<MODEL_FISHEYE4> sum{cam_views + vs, nv, view_start, obs_xy, obs_obj, f32, pnp_pose, pnp_status, work, view_status_out, pose_out,
                                   view_rmse_out, red};
    st = intr_calibrate<MODEL_FISHEYE4>(sum, in9, max_iter, &rmse, &it);
  } else {
    IntrSumDev<MODEL_PINHOLE_BC5> sum{cam_views + vs, nv, view_start, obs_xy, obs_obj, f32, pnp_pose, pnp_status, work, view_status_out, pose_out,
                                      view_rmse_out, red};
    st = intr_calibrate<MODEL_PINHOLE_BC5>(sum, in9, max_iter, &rmse, &it);
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) intr_out[9 * c + k] = in9[k];
    rmse_out[c] = rmse;
    status_out[c] = st;
    iters_out[c] = it;
  }
}

// ---- frame selection ---------------------------------------------------------------------------------------------------------

constexpr int FEAT_BLOCK = 64;     // one wave, as POSE_BLOCK: frames differ in cost
constexpr int SELECT_BLOCK = 256;

__global__ void __launch_bounds__(FEAT_BLOCK)
k_frame_features(long n_frames, const long* __restrict__ order, const long* __restrict__ frame_start, const int* __restrict__ frame_cam,
                 const double* __restrict__ cam_size, const long* __restrict__ homog_start, const int* __restrict__ homog_count,
                 const double* __restrict__ obs_xy, const double* __restrict__ obs_obj, int grid, int f32,
                 unsigned long long* __restrict__ mask_out, double* __restrict__ feat_out, double* __restrict__ orient_out,
                 int* __restrict__ status_out, double* __restrict__ rmse_out) {
  const long q = (long)blockIdx.x * FEAT_BLOCK + threadIdx.x;
  if (q >= n_frames) return;
  const long f = order[q];
  const long a = frame_start[f];
  const int n = (int)(frame_start[f + 1] - a);
  const int c = frame_cam[f];
  const double w = cam_size[2 * c], h = cam_size[2 * c + 1];
  mask_out[f] = fsel_coverage(obs_xy + 2 * a, n, w, h, grid);
  double feat[5];
  fsel_pose_features(obs_xy + 2 * a, n, w, h, feat);
#pragma unroll
  for (int k = 0; k < 5; ++k) feat_out[5 * f + k] = feat[k];
  const long ha = homog_start ? homog_start[f] : a;
  const int hn = homog_start ? homog_count[f] : n;
  double o[3], r;
  const int st = fsel_orientation(obs_obj + 2 * ha, obs_xy + 2 * ha, hn, f32, o, &r);
#pragma unroll
  for (int k = 0; k < 3; ++k) orient_out[3 * f + k] = o[k];
  status_out[f] = st;
  rmse_out[f] = r;
}

// workgroup argmax over (value, -frame): every thread gets the winner (-1: no candidate) and its value
__device__ __forceinline__ int wg_argmax(double v, int f, double* sv, int* si, double* best) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double v2 = __shfl_down(v, o, 64);
    const int f2 = __shfl_down(f, o, 64);
    if (fsel_better(v2, f2, v, f)) { v = v2; f = f2; }
  }
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) { sv[tid >> 6] = v; si[tid >> 6] = f; }
  __syncthreads();
  double bv = sv[0];
  int bf = si[0];
#pragma unroll
  for (int k = 1; k < SELECT_BLOCK / 64; ++k)
    if (fsel_better(sv[k], si[k], bv, bf)) { bv = sv[k]; bf = si[k]; }
  __syncthreads();
  *best = bv;
  return bf;
}

// The ops of fsel_select on the device: the workgroup's threads stride over the camera's frames (all arrays start at the camera's
// first frame).
struct FrameSelDev {
  int nf; const long* fstart; int min_corners;
  const unsigned long long* mask; const double* feat; const double* orient;
  uint64_t edge, corner;
  double* dist; int* sel; double* sv; int* si;
  __device__ bool eligible(int f) const { return fstart[f + 1] - fstart[f] >= (long)min_corners; }
  __device__ uint64_t mask_of(int f) const { return mask[f]; }
  __device__ void take(int k, int f) { if (threadIdx.x == 0) sel[k] = f; }
  __device__ int best_in_bin(int b) {
    double bv = 0.0, best;
    int bf = -1;
    for (int f = threadIdx.x; f < nf; f += SELECT_BLOCK)
      if (eligible(f) && fsel_bin(orient + 3 * f) == b && fsel_better(orient[3 * f + 1], f, bv, bf)) { bv = orient[3 * f + 1]; bf = f; }
    return wg_argmax(bv, bf, sv, si, &best);
  }
  __device__ void start(const int* anchors, int na) {
    for (int f = threadIdx.x; f < nf; f += SELECT_BLOCK) dist[f] = fsel_start_dist(feat, f, eligible(f), anchors, na);
  }
  __device__ int best_score(int last, uint64_t covered, bool have, double* score) {
    double bv = 0.0;
    int bf = -1;
    for (int f = threadIdx.x; f < nf; f += SELECT_BLOCK) {
      double m = dist[f], s;
      const bool cand = fsel_round_item(feat, f, last, mask[f], covered, edge, corner, have, &m, &s);
      if (last >= 0) dist[f] = m;
      if (cand && fsel_better(s, f, bv, bf)) { bv = s; bf = f; }
    }
    return wg_argmax(bv, bf, sv, si, score);
  }
};

__global__ void __launch_bounds__(SELECT_BLOCK)
k_frame_select(const long* __restrict__ cam_frame_start, const long* __restrict__ frame_start, const unsigned long long* __restrict__ mask,
               const double* __restrict__ feat, const double* __restrict__ orient, int grid, int min_corners, int target,
               double* __restrict__ dist, int* __restrict__ selected_out, int* __restrict__ n_selected_out, int* __restrict__ n_anchors_out,
               int* __restrict__ bin_mask_out, int* __restrict__ eligible_out) {
  __shared__ double sv[SELECT_BLOCK / 64];
  __shared__ int si[SELECT_BLOCK / 64];
  __shared__ int cnt[SELECT_BLOCK / 64];
  const int c = blockIdx.x;
  const long f0 = cam_frame_start[c];
  const int nf = (int)(cam_frame_start[c + 1] - f0);
  FrameSelDev ops{nf, frame_start + f0, min_corners, mask + f0, feat + 5 * f0, orient + 3 * f0, fsel_edge_mask(grid), fsel_corner_mask(grid),
                  dist + f0, selected_out + (long)c * target, sv, si};
  int n_el = 0;
  for (int f = threadIdx.x; f < nf; f += SELECT_BLOCK) n_el += ops.eligible(f) ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n_el += __shfl_down(n_el, o, 64);
  if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = n_el;
  __syncthreads();
  int na, bins;
  const int n_sel = fsel_select(ops, target, &na, &bins);
  if (threadIdx.x == 0) {
    int tot = 0;
#pragma unroll
    for (int k = 0; k < SELECT_BLOCK / 64; ++k) tot += cnt[k];
    n_selected_out[c] = n_sel;
    n_anchors_out[c] = na;
    bin_mask_out[c] = bins;
    eligible_out[c] = tot;
  }
}

}  // namespace

extern "C" {

int cba_pose_pnp_batch(const cba_pose_pnp_desc* d, int32_t device, double* pose_out, double* rmse_out, int32_t* status_out,
                       double* undistorted_out) {
  const char* what = "cba_pose_pnp_batch";
  if (!d || !pose_out || !rmse_out || !status_out) return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  if (d->n_views < 0 || d->n_cams <= 0 || !d->cam_model || !d->cam_intr || (d->n_views > 0 && (!d->view_start || !d->view_cam || !d->obs_xy || !d->obs_obj)))
    return err(CBA_ERR_INVALID, std::string(what) + ": bad descriptor");
  if (d->n_views == 0) return CBA_OK;
  // bounds of everything the kernel indexes, checked on the host before anything reaches the device
  if (d->view_start[0] != 0) return err(CBA_ERR_INVALID, std::string(what) + ": view_start[0] != 0");
  for (int64_t v = 0; v < d->n_views; ++v) {
    if (d->view_start[v + 1] < d->view_start[v]) return err(CBA_ERR_INVALID, std::string(what) + ": view_start decreases at view " + std::to_string(v));
    if (d->view_start[v + 1] - d->view_start[v] > (int64_t)1 << 30) return err(CBA_ERR_INVALID, std::string(what) + ": view too large");
    if (d->view_cam[v] < 0 || d->view_cam[v] >= d->n_cams) return err(CBA_ERR_INVALID, std::string(what) + ": view_cam out of range at view " + std::to_string(v));
  }
  for (int32_t c = 0; c < d->n_cams; ++c)
    if (d->cam_model[c] != 0 && d->cam_model[c] != 1) return err(CBA_ERR_INVALID, std::string(what) + ": unknown camera model");
  int rc = select_device(device, what);
  if (rc) return rc;
  const int64_t n_views = d->n_views, n_obs = d->view_start[n_views];
  // views by point count (stable: equal counts keep their order)
  std::vector<int64_t> order(n_views);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
    return d->view_start[x + 1] - d->view_start[x] < d->view_start[y + 1] - d->view_start[y];
  });
  Buffers buf;
  const int64_t* dord = buf.in(order.data(), n_views);
  const int64_t* dvs = buf.in(d->view_start, n_views + 1);
  const int32_t* dvc = buf.in(d->view_cam, n_views);
  const int32_t* dmodel = buf.in(d->cam_model, d->n_cams);
  const double* dintr = buf.in(d->cam_intr, d->n_cams, 9);
  const double* dxy = buf.in(d->obs_xy, n_obs, 2);
  const double* dobj = buf.in(d->obs_obj, n_obs, 3);
  double* dund = buf.make<double>(n_obs, 2);
  double* dpose = buf.make<double>(n_views, 12);
  double* drmse = buf.make<double>(n_views);
  int32_t* dst = buf.make<int32_t>(n_views);
  if (buf.status()) return buf.result(what);
  const int grid = (int)((n_views + POSE_BLOCK - 1) / POSE_BLOCK);
  hipLaunchKernelGGL(k_pose_pnp, dim3(grid), dim3(POSE_BLOCK), 0, 0, (long)n_views, dord, dvs, dvc, dmodel, dintr, dxy, dobj, (int)d->min_points,
                     d->float32_io ? 1 : 0, dund, dpose, drmse, dst);
  buf.check(hipGetLastError());
  buf.out(pose_out, dpose, n_views, 12);
  buf.out(rmse_out, drmse, n_views);
  buf.out(status_out, dst, n_views);
  buf.out(undistorted_out, dund, n_obs, 2);
  return buf.result(what);
}

int cba_pose_pair_rmse(const cba_pose_pair_desc* d, int32_t device, double* rmse_out, int64_t* count_out) {
  const char* what = "cba_pose_pair_rmse";
  if (!d || !rmse_out || !count_out) return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  if (d->n_pairs < 0 || (d->n_pairs > 0 && (!d->pair_pose || !d->pair_start || !d->obs_a || !d->obs_b)))
    return err(CBA_ERR_INVALID, std::string(what) + ": bad descriptor");
  if (d->n_pairs == 0) return CBA_OK;
  if (d->pair_start[0] != 0) return err(CBA_ERR_INVALID, std::string(what) + ": pair_start[0] != 0");
  for (int64_t p = 0; p < d->n_pairs; ++p)
    if (d->pair_start[p + 1] < d->pair_start[p]) return err(CBA_ERR_INVALID, std::string(what) + ": pair_start decreases at pair " + std::to_string(p));
  if (d->n_pairs > 0x7fffffff) return err(CBA_ERR_INVALID, std::string(what) + ": too many pairs");
  int rc = select_device(device, what);
  if (rc) return rc;
  const int64_t n_pairs = d->n_pairs, n_obs = d->pair_start[n_pairs];
  Buffers buf;
  const double* dpose = buf.in(d->pair_pose, n_pairs, 12);
  const int64_t* dps = buf.in(d->pair_start, n_pairs + 1);
  const double* da = buf.in(d->obs_a, n_obs, 2);
  const double* db = buf.in(d->obs_b, n_obs, 2);
  double* drmse = buf.make<double>(n_pairs);
  int64_t* dcount = buf.make<int64_t>(n_pairs);
  if (buf.status()) return buf.result(what);
  hipLaunchKernelGGL(k_pose_pair_rmse, dim3((unsigned)n_pairs), dim3(PAIR_BLOCK), 0, 0, dpose, dps, da, db, drmse, dcount);
  buf.check(hipGetLastError());
  buf.out(rmse_out, drmse, n_pairs);
  buf.out(count_out, dcount, n_pairs);
  return buf.result(what);
}

int cba_pose_essential_batch(const cba_pose_essential_desc* d, int32_t device, double* pose_out, int32_t* status_out, int64_t* n_inliers_out,
                             int64_t* n_cheiral_out, double* conditioning_out, int32_t* winner_out, uint8_t* corr_flag_out, double* xyz_out,
                             double* undistorted_out) {
  const char* what = "cba_pose_essential_batch";
  if (!d || !pose_out || !status_out || !n_inliers_out || !n_cheiral_out || !conditioning_out || !corr_flag_out)
    return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  if (d->n_cams <= 0 || !d->cam_model || !d->cam_intr || d->n_obs < 0 || d->n_pairs < 0 || !d->pair_start ||
      (d->n_obs > 0 && (!d->obs_xy || !d->obs_cam)) || (d->n_pairs > 0 && !d->threshold))
    return err(CBA_ERR_INVALID, std::string(what) + ": bad descriptor");
  if (d->n_hyp < 1 || d->n_hyp > (1 << 16)) return err(CBA_ERR_INVALID, std::string(what) + ": n_hyp out of [1, 65536]");
  if (d->n_pairs > 0x7fffffff) return err(CBA_ERR_INVALID, std::string(what) + ": too many pairs");
  // bounds of everything the kernels index, checked on the host before anything reaches the device
  for (int32_t c = 0; c < d->n_cams; ++c)
    if (d->cam_model[c] != 0 && d->cam_model[c] != 1) return err(CBA_ERR_INVALID, std::string(what) + ": unknown camera model");
  for (int64_t i = 0; i < d->n_obs; ++i)
    if (d->obs_cam[i] < 0 || d->obs_cam[i] >= d->n_cams) return err(CBA_ERR_INVALID, std::string(what) + ": obs_cam out of range at row " + std::to_string(i));
  if (d->pair_start[0] != 0) return err(CBA_ERR_INVALID, std::string(what) + ": pair_start[0] != 0");
  for (int64_t p = 0; p < d->n_pairs; ++p) {
    if (d->pair_start[p + 1] < d->pair_start[p]) return err(CBA_ERR_INVALID, std::string(what) + ": pair_start decreases at pair " + std::to_string(p));
    if (!(d->threshold[p] > 0.0) || !pnp_finite(d->threshold[p])) return err(CBA_ERR_INVALID, std::string(what) + ": bad threshold at pair " + std::to_string(p));
  }
  const int64_t n_pairs = d->n_pairs, n_corr = d->pair_start[n_pairs], n_obs = d->n_obs;
  if (n_corr > 0 && (!d->corr_a || !d->corr_b)) return err(CBA_ERR_INVALID, std::string(what) + ": bad descriptor");
  for (int64_t i = 0; i < n_corr; ++i)
    if (d->corr_a[i] < 0 || d->corr_a[i] >= n_obs || d->corr_b[i] < 0 || d->corr_b[i] >= n_obs)
      return err(CBA_ERR_INVALID, std::string(what) + ": correspondence " + std::to_string(i) + " indexes no row");
  int rc = select_device(device, what);
  if (rc) return rc;
  if (n_obs == 0 && n_pairs == 0) return CBA_OK;
  const int n_hyp = d->n_hyp;
  int64_t max_n = 0;
  for (int64_t p = 0; p < n_pairs; ++p) max_n = std::max<int64_t>(max_n, d->pair_start[p + 1] - d->pair_start[p]);
  Buffers buf;
  const int32_t* dmodel = buf.in(d->cam_model, d->n_cams);
  const double* dintr = buf.in(d->cam_intr, d->n_cams, 9);
  const double* dxy = buf.in(d->obs_xy, n_obs, 2);
  const int32_t* dcam = buf.in(d->obs_cam, n_obs);
  double* dund = buf.make<double>(n_obs, 2);
  const int64_t* dps = buf.in(d->pair_start, n_pairs + 1);
  const int64_t* dca = buf.in(d->corr_a, n_corr);
  const int64_t* dcb = buf.in(d->corr_b, n_corr);
  const double* dthr = buf.in(d->threshold, n_pairs);
  double* dhyp = buf.make<double>(n_pairs, n_hyp, 9);
  unsigned* dcount = buf.make<unsigned>(n_pairs, n_hyp);
  double* dpose = buf.make<double>(n_pairs, 12);
  int32_t* dst = buf.make<int32_t>(n_pairs);
  int64_t* dninl = buf.make<int64_t>(n_pairs);
  int64_t* dnchr = buf.make<int64_t>(n_pairs);
  double* dcond = buf.make<double>(n_pairs);
  int32_t* dwin = buf.make<int32_t>(n_pairs);
  uint8_t* dflag = buf.make<uint8_t>(n_corr);
  double* dxyz = xyz_out ? buf.make<double>(n_corr, 3) : nullptr;  // null: k_epi_refine writes no points
  if (buf.status()) return buf.result(what);
  if (n_pairs > 0) buf.check(hipMemset(dcount, 0, (size_t)n_pairs * n_hyp * sizeof(unsigned)));
  if (buf.status()) return buf.result(what);
  if (n_obs > 0)
    hipLaunchKernelGGL(k_epi_undistort, dim3((unsigned)((n_obs + SCORE_BLOCK - 1) / SCORE_BLOCK)), dim3(SCORE_BLOCK), 0, 0, (long)n_obs, dcam, dmodel, dintr, dxy,
                       d->float32_io ? 1 : 0, dund);
  if (n_pairs > 0) {
    const long nq = (long)n_pairs * n_hyp;
    const double* no_f64 = nullptr;
    hipLaunchKernelGGL(k_epi_hyp, dim3((unsigned)((nq + HYP_BLOCK - 1) / HYP_BLOCK)), dim3(HYP_BLOCK), 0, 0, (long)n_pairs, n_hyp,
                       (unsigned long long)d->seed, dps, dca, dcb, dund, dhyp);
    const long tiles = std::max<long>(1, (long)((max_n + SCORE_BLOCK * SCORE_PER_LANE - 1) / (SCORE_BLOCK * SCORE_PER_LANE)));
    hipLaunchKernelGGL(k_score<true>, dim3((unsigned)tiles, (unsigned)std::min<int64_t>(n_pairs, 65535)), dim3(SCORE_BLOCK), 0, 0, (long)n_pairs,
                       n_hyp, dps, dca, dcb, dund, no_f64, no_f64, dthr, dhyp, dcount);
    hipLaunchKernelGGL(k_epi_refine, dim3((unsigned)n_pairs), dim3(REFINE_BLOCK), 0, 0, (long)n_pairs, n_hyp, dps, dca, dcb, dund, dthr,
                       dhyp, dcount, dpose, dst, dninl, dnchr, dcond, dwin, dflag, dxyz);
  }
  buf.check(hipGetLastError());
  if (n_pairs > 0) {
    buf.out(pose_out, dpose, n_pairs, 12);
    buf.out(status_out, dst, n_pairs);
    buf.out(n_inliers_out, dninl, n_pairs);
    buf.out(n_cheiral_out, dnchr, n_pairs);
    buf.out(conditioning_out, dcond, n_pairs);
    buf.out(winner_out, dwin, n_pairs);
    buf.out(corr_flag_out, dflag, n_corr);
    buf.out(xyz_out, dxyz, n_corr, 3);
  }
  buf.out(undistorted_out, dund, n_obs, 2);
  return buf.result(what);
}

int cba_pose_resect_batch(const cba_pose_resect_desc* d, int32_t device, double* pose_out, int32_t* status_out, int64_t* n_inliers_out,
                          int32_t* winner_out, double* err_out) {
  const char* what = "cba_pose_resect_batch";
  if (!d || !pose_out || !status_out || !n_inliers_out || !err_out) return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  if (d->n_jobs < 0 || !d->job_start || (d->n_jobs > 0 && !d->threshold)) return err(CBA_ERR_INVALID, std::string(what) + ": bad descriptor");
  if (d->n_hyp < 1 || d->n_hyp > (1 << 16)) return err(CBA_ERR_INVALID, std::string(what) + ": n_hyp out of [1, 65536]");
  if (d->n_jobs > 0x7fffffff) return err(CBA_ERR_INVALID, std::string(what) + ": too many jobs");
  if (d->job_start[0] != 0) return err(CBA_ERR_INVALID, std::string(what) + ": job_start[0] != 0");
  for (int64_t j = 0; j < d->n_jobs; ++j) {
    if (d->job_start[j + 1] < d->job_start[j]) return err(CBA_ERR_INVALID, std::string(what) + ": job_start decreases at job " + std::to_string(j));
    if (!(d->threshold[j] > 0.0) || !pnp_finite(d->threshold[j])) return err(CBA_ERR_INVALID, std::string(what) + ": bad threshold at job " + std::to_string(j));
  }
  const int64_t n_jobs = d->n_jobs, n = d->job_start[n_jobs];
  if (n > 0 && (!d->obj || !d->uv)) return err(CBA_ERR_INVALID, std::string(what) + ": bad descriptor");
  int rc = select_device(device, what);
  if (rc) return rc;
  if (n_jobs == 0) return CBA_OK;
  const int n_hyp = d->n_hyp;
  int64_t max_n = 0;
  for (int64_t j = 0; j < n_jobs; ++j) max_n = std::max<int64_t>(max_n, d->job_start[j + 1] - d->job_start[j]);
  Buffers buf;
  const int64_t* djs = buf.in(d->job_start, n_jobs + 1);
  const double* dobj = buf.in(d->obj, n, 3);
  const double* duv = buf.in(d->uv, n, 2);
  const double* dthr = buf.in(d->threshold, n_jobs);
  double* dhyp = buf.make<double>(n_jobs, n_hyp, 12);
  unsigned* dcount = buf.make<unsigned>(n_jobs, n_hyp);
  double* dpose = buf.make<double>(n_jobs, 12);
  int32_t* dst = buf.make<int32_t>(n_jobs);
  int64_t* dninl = buf.make<int64_t>(n_jobs);
  int32_t* dwin = buf.make<int32_t>(n_jobs);
  double* derr = buf.make<double>(n);
  if (buf.status()) return buf.result(what);
  buf.check(hipMemset(dcount, 0, (size_t)n_jobs * n_hyp * sizeof(unsigned)));
  if (buf.status()) return buf.result(what);
  const long nq = (long)n_jobs * n_hyp;
  const long* no_i64 = nullptr;
  const double* no_f64 = nullptr;
  hipLaunchKernelGGL(k_res_hyp, dim3((unsigned)((nq + HYP_BLOCK - 1) / HYP_BLOCK)), dim3(HYP_BLOCK), 0, 0, (long)n_jobs, n_hyp, (int)d->min_points,
                     (unsigned long long)d->seed, djs, dobj, duv, dhyp);
  const long tiles = std::max<long>(1, (long)((max_n + SCORE_BLOCK * SCORE_PER_LANE - 1) / (SCORE_BLOCK * SCORE_PER_LANE)));
  hipLaunchKernelGGL(k_score<false>, dim3((unsigned)tiles, (unsigned)std::min<int64_t>(n_jobs, 65535)), dim3(SCORE_BLOCK), 0, 0, (long)n_jobs, n_hyp, djs,
                     no_i64, no_i64, no_f64, dobj, duv, dthr, dhyp, dcount);
  hipLaunchKernelGGL(k_res_refine, dim3((unsigned)n_jobs), dim3(REFINE_BLOCK), 0, 0, (long)n_jobs, n_hyp, (int)d->min_points, djs, dobj, duv, dthr,
                     dhyp, dcount, dpose, dst, dninl, dwin, derr);
  buf.check(hipGetLastError());
  buf.out(pose_out, dpose, n_jobs, 12);
  buf.out(status_out, dst, n_jobs);
  buf.out(n_inliers_out, dninl, n_jobs);
  buf.out(winner_out, dwin, n_jobs);
  buf.out(err_out, derr, n);
  return buf.result(what);
}

int cba_pose_intrinsics_batch(const cba_intrinsics_desc* d, int32_t device, double* intr_out, double* rmse_out, int32_t* status_out,
                              int32_t* iters_out, double* pose_out, double* view_rmse_out, int32_t* view_status_out) {
  const char* what = "cba_pose_intrinsics_batch";
  if (!d || !intr_out || !rmse_out || !status_out) return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  if (d->n_cams <= 0 || !d->cam_model || !d->cam_size || d->n_views < 0 || d->max_iter < 0 ||
      (d->n_views > 0 && (!d->view_start || !d->view_cam || !d->obs_xy || !d->obs_obj || !pose_out || !view_rmse_out || !view_status_out)))
    return err(CBA_ERR_INVALID, std::string(what) + ": bad descriptor");
  // bounds of everything the kernels index, checked on the host before anything reaches the device
  for (int32_t c = 0; c < d->n_cams; ++c) {
    if (d->cam_model[c] != 0 && d->cam_model[c] != 1) return err(CBA_ERR_INVALID, std::string(what) + ": unknown camera model");
    const bool own = d->cam_start && d->cam_start[9 * c] > 0.0;
    if (!own && (!(d->cam_size[2 * c] > 0.0) || !(d->cam_size[2 * c + 1] > 0.0) || !pnp_finite(d->cam_size[2 * c]) || !pnp_finite(d->cam_size[2 * c + 1])))
      return err(CBA_ERR_INVALID, std::string(what) + ": camera " + std::to_string(c) + " has no image size");
    if (own)
      for (int k = 0; k < 9; ++k)
        if (!pnp_finite(d->cam_start[9 * c + k]) || (k == 1 && !(d->cam_start[9 * c + 1] > 0.0)))
          return err(CBA_ERR_INVALID, std::string(what) + ": bad start intrinsics of camera " + std::to_string(c));
  }
  const int64_t n_views = d->n_views;
  if (n_views > 0 && d->view_start[0] != 0) return err(CBA_ERR_INVALID, std::string(what) + ": view_start[0] != 0");
  for (int64_t v = 0; v < n_views; ++v) {
    if (d->view_start[v + 1] < d->view_start[v]) return err(CBA_ERR_INVALID, std::string(what) + ": view_start decreases at view " + std::to_string(v));
    if (d->view_start[v + 1] - d->view_start[v] > (int64_t)1 << 30) return err(CBA_ERR_INVALID, std::string(what) + ": view too large");
    if (d->view_cam[v] < 0 || d->view_cam[v] >= d->n_cams) return err(CBA_ERR_INVALID, std::string(what) + ": view_cam out of range at view " + std::to_string(v));
  }
  int rc = select_device(device, what);
  if (rc) return rc;
  const int32_t n_cams = d->n_cams;
  const int64_t n_obs = n_views > 0 ? d->view_start[n_views] : 0;
  std::vector<double> start((size_t)n_cams * 9);
  for (int32_t c = 0; c < n_cams; ++c) {
    if (d->cam_start && d->cam_start[9 * c] > 0.0) std::copy(d->cam_start + 9 * c, d->cam_start + 9 * c + 9, start.begin() + 9 * c);
    else intr_start(d->cam_model[c], d->cam_size[2 * c], d->cam_size[2 * c + 1], &start[9 * c]);
  }
  // views by corner count (stable), then the list of each camera in that order
  std::vector<int64_t> order(n_views), cam_view_start(n_cams + 1, 0), cam_views(n_views), fill(n_cams, 0);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
    return d->view_start[x + 1] - d->view_start[x] < d->view_start[y + 1] - d->view_start[y];
  });
  for (int64_t v = 0; v < n_views; ++v) ++cam_view_start[d->view_cam[v] + 1];
  for (int32_t c = 0; c < n_cams; ++c) cam_view_start[c + 1] += cam_view_start[c];
  for (int64_t v : order) {
    const int32_t c = d->view_cam[v];
    cam_views[cam_view_start[c] + fill[c]++] = v;
  }
  Buffers buf;
  const int64_t* dord = buf.in(order.data(), n_views);
  const int64_t* dvs = buf.in(d->view_start, n_views > 0 ? n_views + 1 : 0);
  const int32_t* dvc = buf.in(d->view_cam, n_views);
  const int32_t* dmodel = buf.in(d->cam_model, n_cams);
  const double* dstart = buf.in(start.data(), n_cams, 9);
  const double* dxy = buf.in(d->obs_xy, n_obs, 2);
  const double* dobj = buf.in(d->obs_obj, n_obs, 3);
  double* dund = buf.make<double>(n_obs, 2);
  double* dpnp = buf.make<double>(n_views, 12);
  double* dprm = buf.make<double>(n_views);
  int32_t* dpst = buf.make<int32_t>(n_views);
  const int64_t* dcvs = buf.in(cam_view_start.data(), n_cams + 1);
  const int64_t* dcv = buf.in(cam_views.data(), n_views);
  double* dwork = buf.make<double>(n_views, INTR_WORK);
  double* dintr = buf.make<double>(n_cams, 9);
  double* drmse = buf.make<double>(n_cams);
  int32_t* dst = buf.make<int32_t>(n_cams);
  int32_t* dit = buf.make<int32_t>(n_cams);
  double* dpose = buf.make<double>(n_views, 12);
  double* dvr = buf.make<double>(n_views);
  int32_t* dvst = buf.make<int32_t>(n_views);
  if (buf.status()) return buf.result(what);
  const int f32 = d->float32_io ? 1 : 0;
  if (n_views > 0)
    hipLaunchKernelGGL(k_pose_pnp, dim3((unsigned)((n_views + POSE_BLOCK - 1) / POSE_BLOCK)), dim3(POSE_BLOCK), 0, 0, (long)n_views, dord, dvs, dvc, dmodel,
                       dstart, dxy, dobj, (int)INTR_MIN_POINTS, f32, dund, dpnp, dprm, dpst);
  hipLaunchKernelGGL(k_intrinsics, dim3((unsigned)n_cams), dim3(REFINE_BLOCK), 0, 0, dmodel, dstart, dcvs, dcv, dvs, dxy, dobj, f32, (int)d->max_iter,
                     dpnp, dpst, dwork, dintr, drmse, dst, dit, dpose, dvr, dvst);
  buf.check(hipGetLastError());
  buf.out(intr_out, dintr, n_cams, 9);
  buf.out(rmse_out, drmse, n_cams);
  buf.out(status_out, dst, n_cams);
  buf.out(iters_out, dit, n_cams);
  buf.out(pose_out, dpose, n_views, 12);
  buf.out(view_rmse_out, dvr, n_views);
  buf.out(view_status_out, dvst, n_views);
  return buf.result(what);
}

int cba_pose_select_frames(const cba_frame_select_desc* d, int32_t device, uint64_t* cell_mask_out, double* pose_feat_out, double* orient_out,
                           int32_t* homog_status_out, double* homog_rmse_out, int32_t* selected_out, int32_t* n_selected_out,
                           int32_t* n_anchors_out, int32_t* bin_mask_out, int32_t* eligible_out) {
  const char* what = "cba_pose_select_frames";
  if (!d) return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  if (d->n_cams < 0 || d->n_frames < 0 || d->target_count < 1 || d->min_corners < 0 || (!d->homog_start != !d->homog_count))
    return err(CBA_ERR_INVALID, std::string(what) + ": bad descriptor");
  if (d->grid_size < 1 || d->grid_size > FSEL_MAX_GRID)
    return err(CBA_ERR_UNSUPPORTED, std::string(what) + ": grid_size " + std::to_string(d->grid_size) + " outside 1.." + std::to_string(FSEL_MAX_GRID) +
                                        " (the cell mask has 64 bits)");
  const int32_t n_cams = d->n_cams, target = d->target_count;
  const int64_t n_frames = d->n_frames;
  if (n_cams > 0 && (!d->cam_frame_start || !d->cam_size || !selected_out || !n_selected_out || !n_anchors_out || !bin_mask_out || !eligible_out))
    return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  if (n_frames > 0 && (n_cams == 0 || !d->frame_start || !d->obs_xy || !d->obs_obj || !cell_mask_out || !pose_feat_out || !orient_out ||
                       !homog_status_out || !homog_rmse_out))
    return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  if (n_cams == 0) return CBA_OK;
  // bounds of everything the kernels index, checked on the host before anything reaches the device
  if (d->cam_frame_start[0] != 0) return err(CBA_ERR_INVALID, std::string(what) + ": cam_frame_start[0] != 0");
  for (int32_t c = 0; c < n_cams; ++c) {
    if (d->cam_frame_start[c + 1] < d->cam_frame_start[c]) return err(CBA_ERR_INVALID, std::string(what) + ": cam_frame_start decreases at camera " + std::to_string(c));
    if (d->cam_frame_start[c + 1] - d->cam_frame_start[c] > 0x7fffffff) return err(CBA_ERR_INVALID, std::string(what) + ": too many frames of camera " + std::to_string(c));
    const double w = d->cam_size[2 * c], h = d->cam_size[2 * c + 1];
    if (!(w > 0.0) || !(h > 0.0) || !pnp_finite(w) || !pnp_finite(h)) return err(CBA_ERR_INVALID, std::string(what) + ": camera " + std::to_string(c) + " has no image size");
  }
  if (d->cam_frame_start[n_cams] != n_frames) return err(CBA_ERR_INVALID, std::string(what) + ": cam_frame_start does not end at n_frames");
  if ((uint64_t)n_cams * (uint64_t)target > (uint64_t)1 << 40) return err(CBA_ERR_INVALID, std::string(what) + ": n_cams * target_count too large");
  std::fill(selected_out, selected_out + (size_t)n_cams * target, -1);
  if (n_frames == 0) {
    for (int32_t c = 0; c < n_cams; ++c) n_selected_out[c] = n_anchors_out[c] = bin_mask_out[c] = eligible_out[c] = 0;
    return CBA_OK;
  }
  if (d->frame_start[0] != 0) return err(CBA_ERR_INVALID, std::string(what) + ": frame_start[0] != 0");
  for (int64_t f = 0; f < n_frames; ++f) {
    const int64_t a = d->frame_start[f], b = d->frame_start[f + 1];
    if (b < a) return err(CBA_ERR_INVALID, std::string(what) + ": frame_start decreases at frame " + std::to_string(f));
    if (b - a > (int64_t)1 << 30) return err(CBA_ERR_INVALID, std::string(what) + ": frame too large");
    if (d->homog_start && (d->homog_count[f] < 0 || d->homog_start[f] < a || d->homog_start[f] > b || d->homog_count[f] > b - d->homog_start[f]))
      return err(CBA_ERR_INVALID, std::string(what) + ": homography subrange outside frame " + std::to_string(f));
  }
  int rc = select_device(device, what);
  if (rc) return rc;
  const int64_t n_obs = d->frame_start[n_frames];
  // frames by corner count (stable), and the camera of every frame
  std::vector<int64_t> order(n_frames);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
    return d->frame_start[x + 1] - d->frame_start[x] < d->frame_start[y + 1] - d->frame_start[y];
  });
  std::vector<int32_t> frame_cam(n_frames);
  for (int32_t c = 0; c < n_cams; ++c) std::fill(frame_cam.begin() + d->cam_frame_start[c], frame_cam.begin() + d->cam_frame_start[c + 1], c);
  Buffers buf;
  const int64_t* dord = buf.in(order.data(), n_frames);
  const int64_t* dfs = buf.in(d->frame_start, n_frames + 1);
  const int32_t* dfc = buf.in(frame_cam.data(), n_frames);
  const int64_t* dcfs = buf.in(d->cam_frame_start, n_cams + 1);
  const double* dsize = buf.in(d->cam_size, n_cams, 2);
  const int64_t* dhs = d->homog_start ? buf.in(d->homog_start, n_frames) : nullptr;  // null: the homography takes every corner of a frame
  const int32_t* dhc = d->homog_start ? buf.in(d->homog_count, n_frames) : nullptr;
  const double* dxy = buf.in(d->obs_xy, n_obs, 2);
  const double* dobj = buf.in(d->obs_obj, n_obs, 2);
  // the kernels take the cell masks as unsigned long long, the C ABI as uint64_t: the same words under another name
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "cell masks are passed as unsigned long long");
  unsigned long long* dmask = buf.make<unsigned long long>(n_frames);
  double* dfeat = buf.make<double>(n_frames, 5);
  double* dori = buf.make<double>(n_frames, 3);
  int32_t* dhst = buf.make<int32_t>(n_frames);
  double* dhr = buf.make<double>(n_frames);
  double* ddist = buf.make<double>(n_frames);
  int32_t* dsel = buf.in(selected_out, n_cams, target);
  int32_t* dns = buf.make<int32_t>(n_cams);
  int32_t* dna = buf.make<int32_t>(n_cams);
  int32_t* dbm = buf.make<int32_t>(n_cams);
  int32_t* del = buf.make<int32_t>(n_cams);
  if (buf.status()) return buf.result(what);
  hipLaunchKernelGGL(k_frame_features, dim3((unsigned)((n_frames + FEAT_BLOCK - 1) / FEAT_BLOCK)), dim3(FEAT_BLOCK), 0, 0, (long)n_frames, dord, dfs, dfc, dsize,
                     dhs, dhc, dxy, dobj, (int)d->grid_size, d->float32_io ? 1 : 0, dmask, dfeat, dori, dhst, dhr);
  hipLaunchKernelGGL(k_frame_select, dim3((unsigned)n_cams), dim3(SELECT_BLOCK), 0, 0, dcfs, dfs, dmask, dfeat,
                     dori, (int)d->grid_size, (int)d->min_corners, (int)target, ddist, dsel, dns, dna, dbm, del);
  buf.check(hipGetLastError());
  buf.out((unsigned long long*)cell_mask_out, dmask, n_frames);
  buf.out(pose_feat_out, dfeat, n_frames, 5);
  buf.out(orient_out, dori, n_frames, 3);
  buf.out(homog_status_out, dhst, n_frames);
  buf.out(homog_rmse_out, dhr, n_frames);
  buf.out(selected_out, dsel, n_cams, target);
  buf.out(n_selected_out, dns, n_cams);
  buf.out(n_anchors_out, dna, n_cams);
  buf.out(bin_mask_out, dbm, n_cams);
  buf.out(eligible_out, del, n_cams);
  return buf.result(what);
}

}  // extern "C"
