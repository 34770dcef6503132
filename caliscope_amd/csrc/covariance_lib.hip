// cba_parameter_covariance of libcaliscope_ba.so (C ABI: include/caliscope/uncertainty.h): the covariance of every camera's parameters and
// of every point in the inner-constraint gauge, sigma0^2 pinv(J^T J), from the bordered system with points and multipliers eliminated.
// The formulas, the per-element arithmetic, the checks, the refusal texts and the host-side small matrices are covariance_math.h (shared with
// tests/native/covariance_replay.h, the one host replay of this pipeline that the harnesses of the CPU suite run); this file holds the kernels
// and the entry points.  Everything is FP64.
//
//   k_unc_cam        one thread per camera: the CamTab of ba_math.h and the camera's gauge rows, written into B (B starts as Nc).
//   k_unc_obs        one thread per observation, in point order: project_full + robust_one, the W block A^T B and B^T B stored per
//                    observation, A^T A added to U of the camera and rho to the cost (atomics; the cost per wave by shuffles).
//   k_unc_point      one wave per point: V = sum B^T B, V^-1 (chol3), Z = V^-1 Np, Y_a = W_a V^-1 per observation (stored: the point
//                    formula reads them again), -W_a Z into B and -Y_a W_b^T into the dense Schur complement for every ordered pair of the
//                    point's observations whose entry lies in the upper triangle (atomics: a repeated (camera, point) pair simply adds).
//   k_unc_d          D = sum Np^T Z over the points: grid-stride, 28 sums per thread (21 with six columns), per wave by shuffles, then atomics.
//   (host)           D^-1 (7 x 7, cov_spd_inverse) and sigma0^2 between two launches.
//   k_unc_assemble   one thread per entry of the upper triangle: St = U + Schur + B D^-1 B^T, scaled by 1 / sqrt of its diagonal on both
//                    sides, into both triangles of the Cholesky work matrix.
//   k_chol_step      the solver's blocked Cholesky (cba_kernels.h through enqueue_chol_factor of cba_lib.hip): L and T = L^-T.
//   k_unc_pivots     one thread per pivot: a pivot at or below COV_PIVOT_TINY raises the numeric error.
//   k_unc_ttt        C = St^-1 = Ds T T^T Ds by v_mfma_f64_16x16x4: one workgroup per 32 x 32 block of the upper block triangle, four
//                    16 x 16 tiles, depth from the block's column to the end (T is upper triangular); written to both triangles.
//   (host)           E = C B D^-1 and F (cov_gauge_terms: O(ncp^2) flops), the camera outputs sigma0^2 C.
//   k_unc_point_cov  one wave per point: sigma0^2 (V^-1 + Z F Z^T + sum_ab Y_a^T C_ab Y_b + sum_a sym(Y_a^T E_a Z^T)), the k^2 pairs and
//                    the k rank-7 terms spread over the lanes, 3 x 3 sums by shuffles.
//
// CBA_DETERMINISTIC=1 (read per call, as the solver's handles read it when they are made): the sums the kernels above form with FP64 atomics —
// U, the cost, B, the Schur complement and D — are formed in a FIXED order instead, so that two calls return the same bits: the three kernels
// skip their atomics and k_unc_cam_sums (one wave per camera: U and the camera's share of the cost), k_unc_rows (one workgroup per camera: its
// rows of B and of the Schur complement, one thread per entry, points in order) and k_unc_fixed_sums (D and the cost from per-wave rows) take
// their place.  Every entry has ONE owner that adds in observation order; slower (each camera scans all observations), and not the default.
//
// cba_parameter_covariance_constrained (include/caliscope/uncertainty_constrained.h; host plan: covariance_constraint_plan.h, per-element arithmetic:
// covariance_constraint_math.h) adds the solver's rigid-distance rows to J.  They couple the points of a connected component of the constraint graph
// and fix the scale, so V becomes V~ = V + C^T C, block-diagonal per component, and the gauge keeps six columns: the kernels above are templates on
// the gauge width G (7, or 6 with rows), k_unc_point and k_unc_point_cov take the points in no row through a list, and
//   k_unc_con_rows   one thread per row: residual, robust_one, the scaled Jacobian entries on up to eight points, rho into the cost;
//   k_unc_component  one workgroup per component: V~_k in LDS, its Cholesky factor and inverse, Z_k, [V~_k^-1]_ii, per camera Y_c = W_c,k V~_k^-1,
//                    the component's terms of B and of the Schur complement (its comment has the steps);
//   k_unc_point_cov  a second time, on the points of the components: one (camera, Y_c[:, i]) entry per camera of the component in the place of the
//                    point's observations.
// Without a row of positive weight the call is cba_parameter_covariance: G = 7, no list, the launches above and nothing else.
//
// Null stream throughout.  Scaling by sigma0^2 has no kernel of its own: the point kernel applies it, the camera blocks take it on the
// host where they are copied into the caller's arrays.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "ba_math.h"
#include "covariance_math.h"
#include "covariance_constraint_math.h"
#include "covariance_constraint_plan.h"
#include "covariance_pipeline.h"
#include "device_call.h"
#include "reliability_constraint_math.h"
#include "chol_factor.h"
#include "chol_schedule.h"

using namespace cba;

namespace {

typedef double v4f64 __attribute__((ext_vector_type(4)));
enum CovFlag : int { F_POINT = 0, F_DIAG = 1, F_CHOL = 2, F_TINY = 3, F_WHICH = 4, F_COMP = 5, F_COMP_WHICH = 6, N_FLAGS = 8 };

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;  // lane 0 holds the sum
}

template <int G> __global__ void __launch_bounds__(COV_BLOCK)
k_unc_cam(int32_t n_cams, const int32_t* __restrict__ cam_model, const int32_t* __restrict__ cam_off, const double* __restrict__ cam_const,
          const double* __restrict__ cam_x, double* __restrict__ tab, double* __restrict__ B) {
  const int32_t c = blockIdx.x * COV_BLOCK + threadIdx.x;
  if (c >= n_cams) return;
  const int32_t off = cam_off[c], np = cam_off[c + 1] - off;
  double xc[MAX_NC];
#pragma unroll
  for (int i = 0; i < MAX_NC; ++i) xc[i] = cam_x[(int64_t)c * MAX_NC + i];
  CamTab t;
  cam_prepare(xc, cam_const + (int64_t)c * CAM_CONST_STRIDE, cam_model[c], np, &t, off);
  const double* src = reinterpret_cast<const double*>(&t);
#pragma unroll
  for (int i = 0; i < CAMTAB_DOUBLES; ++i) tab[(int64_t)c * CAMTAB_DOUBLES + i] = src[i];
  double N[MAX_NC][G];
  cov_gauge_cam(t, N);
#pragma unroll
  for (int r = 0; r < MAX_NC; ++r)
    if (r < np) {
#pragma unroll
      for (int j = 0; j < G; ++j) B[(int64_t)(off + r) * G + j] = N[r][j];
    }
}

__global__ void __launch_bounds__(COV_BLOCK)
k_unc_obs(int64_t n_obs, const int64_t* __restrict__ order, const int32_t* __restrict__ obs_cam, const int32_t* __restrict__ obs_pt,
          const double* __restrict__ obs_uv, const double* __restrict__ tab, const double* __restrict__ points, int loss, double f_scale,
          double* __restrict__ Wblk, double* __restrict__ Vobs, int32_t* __restrict__ cam_sorted, double* __restrict__ U, double* __restrict__ cost,
          bool fixed_order) {
  const int64_t i = (int64_t)blockIdx.x * COV_BLOCK + threadIdx.x;
  double rho = 0.0;
  if (i < n_obs) {
    const int64_t o = order[i];
    const int32_t cam = obs_cam[o];
    const int64_t p = obs_pt[o];
    const CamTab& c = reinterpret_cast<const CamTab*>(tab)[cam];
    const double X[3] = {points[3 * p], points[3 * p + 1], points[3 * p + 2]};
    const double uv[2] = {obs_uv[2 * o], obs_uv[2 * o + 1]};
    double A[2][MAX_NC], B[2][3], Wb[3 * MAX_NC], Vo[6];
    rho = cov_obs_jacobian(c, X, uv, loss, f_scale, A, B);
    cov_obs_products(A, B, Wb, Vo);
#pragma unroll
    for (int e = 0; e < 3 * MAX_NC; ++e) Wblk[i * (3 * MAX_NC) + e] = Wb[e];
#pragma unroll
    for (int e = 0; e < 6; ++e) Vobs[i * 6 + e] = Vo[e];
    cam_sorted[i] = cam;
    if (fixed_order) return;  // (k_unc_cam_sums forms U and the cost)
    const bool nine = c.nparams == 9.0;
    double* Uc = U + (int64_t)cam * (MAX_NC * MAX_NC);
#pragma unroll
    for (int r = 0; r < MAX_NC; ++r)
#pragma unroll
      for (int q = r; q < MAX_NC; ++q)
        if (q < 6 || nine) atomicAdd(&Uc[r * MAX_NC + q], A[0][r] * A[0][q] + A[1][r] * A[1][q]);
  }
  if (fixed_order) return;
  rho = wave_sum(rho);
  if ((threadIdx.x & 63) == 0 && rho != 0.0) atomicAdd(cost, 0.5 * rho);
}

// fixed order: one wave per camera.  Lane l takes the observations i = l, l + 64, .. (point order) of its camera, the lanes' sums meet in wave_sum's tree.
__global__ void __launch_bounds__(64)
k_unc_cam_sums(int64_t n_obs, const int64_t* __restrict__ order, const int32_t* __restrict__ obs_pt, const double* __restrict__ obs_uv,
               const double* __restrict__ tab, const double* __restrict__ points, int loss, double f_scale, const int32_t* __restrict__ cam_sorted,
               double* __restrict__ U, double* __restrict__ cam_cost) {
  const int32_t cam = blockIdx.x;
  const CamTab& c = reinterpret_cast<const CamTab*>(tab)[cam];
  const bool nine = c.nparams == 9.0;
  double acc[MAX_NC * (MAX_NC + 1) / 2], rho = 0.0;
#pragma unroll
  for (int e = 0; e < MAX_NC * (MAX_NC + 1) / 2; ++e) acc[e] = 0.0;
  for (int64_t i = threadIdx.x; i < n_obs; i += 64) {
    if (cam_sorted[i] != cam) continue;
    const int64_t o = order[i], p = obs_pt[o];
    const double X[3] = {points[3 * p], points[3 * p + 1], points[3 * p + 2]};
    const double uv[2] = {obs_uv[2 * o], obs_uv[2 * o + 1]};
    double A[2][MAX_NC], B[2][3];
    rho += cov_obs_jacobian(c, X, uv, loss, f_scale, A, B);
    int e = 0;
#pragma unroll
    for (int r = 0; r < MAX_NC; ++r)
#pragma unroll
      for (int q = r; q < MAX_NC; ++q) acc[e++] += A[0][r] * A[0][q] + A[1][r] * A[1][q];
  }
  double* Uc = U + (int64_t)cam * (MAX_NC * MAX_NC);
  int e = 0;
#pragma unroll
  for (int r = 0; r < MAX_NC; ++r)
#pragma unroll
    for (int q = r; q < MAX_NC; ++q) {
      const double v = wave_sum(acc[e++]);
      if (threadIdx.x == 0 && (q < 6 || nine)) Uc[r * MAX_NC + q] += v;  // (U is zero on entry; this wave is the entry's only writer)
    }
  rho = wave_sum(rho);
  if (threadIdx.x == 0) cam_cost[cam] = 0.5 * rho;
}

// `list` (a problem with constraint rows): the points in no row, which are the points this kernel takes; nullptr: every point
template <int G> __global__ void __launch_bounds__(COV_POINT_THREADS)
k_unc_point(const int32_t* __restrict__ list, const int64_t* __restrict__ pt_start, const int32_t* __restrict__ cam_sorted, const int32_t* __restrict__ cam_off, int32_t ncp,
            const double* __restrict__ points, const double* __restrict__ Wblk, const double* __restrict__ Vobs, double* __restrict__ Y,
            double* __restrict__ Vinv, double* __restrict__ Zbuf, double* __restrict__ B, double* __restrict__ Sacc, int* __restrict__ flags,
            bool fixed_order) {
  __shared__ double sh_vi[9], sh_z[3 * G];
  const int64_t p = list ? (int64_t)list[blockIdx.x] : (int64_t)blockIdx.x;
  const int t = threadIdx.x;
  const int64_t s = pt_start[p], k = pt_start[p + 1] - s;
  double V[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t a = 0; a < k; ++a) {
#pragma unroll
    for (int e = 0; e < 6; ++e) V[e] += Vobs[(s + a) * 6 + e];
  }
  double Vi[6];
  if (!cov_point_vinv(V, Vi)) {  // (every lane holds the same V: the branch is uniform)
    if (t == 0) { flags[F_POINT] = 1; atomicMax(&flags[F_WHICH], (int)p + 1); }
    return;
  }
  const double X[3] = {points[3 * p], points[3 * p + 1], points[3 * p + 2]};
  double Z[3][G];
  cov_point_z(Vi, X, Z);
  if (t == 0) {
#pragma unroll
    for (int e = 0; e < 6; ++e) Vinv[p * 6 + e] = Vi[e];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) sh_vi[3 * a + b] = cov_sym3(Vi, a, b);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int j = 0; j < G; ++j) { sh_z[a * G + j] = Z[a][j]; Zbuf[p * (3 * G) + a * G + j] = Z[a][j]; }
  }
  __syncthreads();
  constexpr int WB = 3 * MAX_NC;
  for (int64_t it = t; it < k * WB; it += COV_POINT_THREADS) {  // Y_a = W_a V^-1
    const int64_t a = it / WB;
    const int e = (int)(it % WB), r = e / 3, q = e % 3;
    const double* w = Wblk + (s + a) * WB + 3 * r;
    Y[(s + a) * WB + e] = w[0] * sh_vi[q] + w[1] * sh_vi[3 + q] + w[2] * sh_vi[6 + q];
  }
  __syncthreads();  // (Y of this point is read below by other lanes)
  if (fixed_order) return;  // (k_unc_rows forms B and the Schur complement from Y, Z and the W blocks)
  for (int64_t it = t; it < k * (MAX_NC * G); it += COV_POINT_THREADS) {  // B -= W_a Z
    const int64_t a = it / (MAX_NC * G);
    const int e = (int)(it % (MAX_NC * G)), r = e / G, j = e % G;
    const int32_t cam = cam_sorted[s + a], off = cam_off[cam], np = cam_off[cam + 1] - off;
    if (r >= np) continue;
    const double* w = Wblk + (s + a) * WB + 3 * r;
    atomicAdd(&B[(int64_t)(off + r) * G + j], -(w[0] * sh_z[j] + w[1] * sh_z[G + j] + w[2] * sh_z[2 * G + j]));
  }
  constexpr int BLK = MAX_NC * MAX_NC;
  for (int64_t it = t; it < k * k * BLK; it += COV_POINT_THREADS) {  // Schur -= Y_a W_b^T, upper triangle
    const int64_t ab = it / BLK, a = ab / k, b = ab % k;
    const int e = (int)(it % BLK), r = e / MAX_NC, c = e % MAX_NC;
    const int32_t cam_a = cam_sorted[s + a], off_a = cam_off[cam_a], np_a = cam_off[cam_a + 1] - off_a;
    const int32_t cam_b = cam_sorted[s + b], off_b = cam_off[cam_b], np_b = cam_off[cam_b + 1] - off_b;
    const int32_t row = off_a + r, col = off_b + c;
    if (r >= np_a || c >= np_b || row > col) continue;
    const double* y = Y + (s + a) * WB + 3 * r;
    const double* w = Wblk + (s + b) * WB + 3 * c;
    atomicAdd(&Sacc[(int64_t)row * ncp + col], -(y[0] * w[0] + y[1] * w[1] + y[2] * w[2]));
  }
}

// fixed order: one workgroup per camera, which owns the camera's rows of B and of the Schur complement.  Thread e < 63 owns entry (r, j) of the
// B rows, thread 64 + e, e < 81, the entries (r, off_b + c) of the Schur rows for every camera b; each walks the points in order and adds the
// terms of its entries one after the other, so no entry has two writers and a repeated (camera, point) pair simply adds twice.
constexpr int COV_ROWS_THREADS = 192;
__global__ void __launch_bounds__(COV_ROWS_THREADS)
k_unc_rows(int64_t n_points, const int64_t* __restrict__ pt_start, const int32_t* __restrict__ cam_sorted, const int32_t* __restrict__ cam_off, int32_t ncp,
           const double* __restrict__ Wblk, const double* __restrict__ Y, const double* __restrict__ Zbuf, double* __restrict__ B, double* __restrict__ Sacc) {
  constexpr int WB = 3 * MAX_NC;
  const int32_t cam = blockIdx.x, off_a = cam_off[cam], np_a = cam_off[cam + 1] - off_a;
  const int t = threadIdx.x;
  const bool b_role = t < MAX_NC * COV_GAUGE, s_role = t >= 64 && t < 64 + MAX_NC * MAX_NC;
  const int e = b_role ? t : t - 64;
  const int r = b_role ? e / COV_GAUGE : e / MAX_NC, c = b_role ? e % COV_GAUGE : e % MAX_NC;
  if (!(b_role || s_role) || r >= np_a) return;
  for (int64_t p = 0; p < n_points; ++p) {
    const int64_t s = pt_start[p], k = pt_start[p + 1] - s;
    for (int64_t a = 0; a < k; ++a) {
      if (cam_sorted[s + a] != cam) continue;
      if (b_role) {
        const double* w = Wblk + (s + a) * WB + 3 * r;
        const double* z = Zbuf + p * (3 * COV_GAUGE);
        B[(int64_t)(off_a + r) * COV_GAUGE + c] += -(w[0] * z[c] + w[1] * z[COV_GAUGE + c] + w[2] * z[2 * COV_GAUGE + c]);
        continue;
      }
      const double* y = Y + (s + a) * WB + 3 * r;
      for (int64_t b = 0; b < k; ++b) {
        const int32_t cam_b = cam_sorted[s + b], off_b = cam_off[cam_b], np_b = cam_off[cam_b + 1] - off_b;
        const int32_t row = off_a + r, col = off_b + c;
        if (c >= np_b || row > col) continue;
        const double* w = Wblk + (s + b) * WB + 3 * c;
        Sacc[(int64_t)row * ncp + col] += -(y[0] * w[0] + y[1] * w[1] + y[2] * w[2]);
      }
    }
  }
}

// D: with `rows` != nullptr (fixed order) every wave leaves its 28 sums as a row of `rows` for k_unc_fixed_sums instead of adding them to D
constexpr int COV_D_BLOCKS = 256;
template <int G> __global__ void __launch_bounds__(COV_BLOCK)
k_unc_d(int64_t n_points, const double* __restrict__ points, const double* __restrict__ Zbuf, double* __restrict__ D, double* __restrict__ rows) {
  double acc[G * (G + 1) / 2];
#pragma unroll
  for (int e = 0; e < G * (G + 1) / 2; ++e) acc[e] = 0.0;
  for (int64_t p = (int64_t)blockIdx.x * COV_BLOCK + threadIdx.x; p < n_points; p += (int64_t)gridDim.x * COV_BLOCK) {
    double N[3][G], Z[3][G];
    cov_gauge_point(points[3 * p], points[3 * p + 1], points[3 * p + 2], N);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int j = 0; j < G; ++j) Z[a][j] = Zbuf[p * (3 * G) + a * G + j];
    int e = 0;
#pragma unroll
    for (int j = 0; j < G; ++j)
#pragma unroll
      for (int m = j; m < G; ++m) acc[e++] += N[0][j] * Z[0][m] + N[1][j] * Z[1][m] + N[2][j] * Z[2][m];
  }
  int e = 0;
#pragma unroll
  for (int j = 0; j < G; ++j)
#pragma unroll
    for (int m = j; m < G; ++m) {
      const double v = wave_sum(acc[e]);
      if ((threadIdx.x & 63) == 0) {
        if (rows) rows[((int64_t)blockIdx.x * (COV_BLOCK / 64) + (threadIdx.x >> 6)) * (G * (G + 1) / 2) + e] = v; else atomicAdd(&D[j * G + m], v);
      }
      ++e;
    }
}

// fixed order: thread e < COV_D_SUMS (28) adds the waves' rows of D in order, the thread behind them the cameras' shares of the cost
constexpr int COV_D_SUMS = COV_GAUGE * (COV_GAUGE + 1) / 2;  // the upper triangle of D, as k_unc_d<COV_GAUGE> leaves it per wave
__global__ void __launch_bounds__(64)
k_unc_fixed_sums(const double* __restrict__ rows, int n_rows, const double* __restrict__ cam_cost, int32_t n_cams, double* __restrict__ D, double* __restrict__ cost) {
  const int e = threadIdx.x;
  if (e < COV_D_SUMS) {
    double v = 0.0;
    for (int i = 0; i < n_rows; ++i) v += rows[(int64_t)i * COV_D_SUMS + e];
    int j = 0, rest = e;
    while (rest >= COV_GAUGE - j) { rest -= COV_GAUGE - j; ++j; }
    D[j * COV_GAUGE + j + rest] = v;
  } else if (e == COV_D_SUMS) {
    double v = 0.0;
    for (int32_t c = 0; c < n_cams; ++c) v += cam_cost[c];
    *cost = v;
  }
}

// entry (row <= col) of St = U + Schur + B D^-1 B^T
template <int G> __device__ __forceinline__ double st_entry(int row, int col, int32_t ncp, const double* __restrict__ U, const double* __restrict__ Sacc,
                                           const double* __restrict__ B, const double* __restrict__ Dinv, const int32_t* __restrict__ param_cam,
                                           const int32_t* __restrict__ param_loc) {
  double v = Sacc[(int64_t)row * ncp + col];
  if (param_cam[row] == param_cam[col]) v += U[(int64_t)param_cam[row] * (MAX_NC * MAX_NC) + param_loc[row] * MAX_NC + param_loc[col]];
#pragma unroll
  for (int j = 0; j < G; ++j) {
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < G; ++m) s += Dinv[j * G + m] * B[(int64_t)col * G + m];
    v += B[(int64_t)row * G + j] * s;
  }
  return v;
}

template <int G> __global__ void __launch_bounds__(COV_BLOCK)
k_unc_assemble(int32_t ncp, int ldw, const double* __restrict__ U, const double* __restrict__ Sacc, const double* __restrict__ B,
               const double* __restrict__ Dinv, const int32_t* __restrict__ param_cam, const int32_t* __restrict__ param_loc,
               double* __restrict__ W, double* __restrict__ scale, int* __restrict__ flags) {
  const int64_t t = (int64_t)blockIdx.x * COV_BLOCK + threadIdx.x;
  if (t >= (int64_t)ncp * ncp) return;
  const int row = (int)(t / ncp), col = (int)(t % ncp);
  if (col < row) return;
  const double dr = st_entry<G>(row, row, ncp, U, Sacc, B, Dinv, param_cam, param_loc);
  const double dc = st_entry<G>(col, col, ncp, U, Sacc, B, Dinv, param_cam, param_loc);
  double sr = 1.0, sc = 1.0;
  if (dr > 0.0 && dr < 1.7e308) sr = 1.0 / sqrt(dr); else flags[F_DIAG] = 1;
  if (dc > 0.0 && dc < 1.7e308) sc = 1.0 / sqrt(dc); else flags[F_DIAG] = 1;
  const double v = (row == col ? dr : st_entry<G>(row, col, ncp, U, Sacc, B, Dinv, param_cam, param_loc)) * sr * sc;
  W[(int64_t)row * ldw + col] = v;
  W[(int64_t)col * ldw + row] = v;
  if (row == col) scale[row] = sr;
}

__global__ void __launch_bounds__(COV_BLOCK)
k_unc_pivots(int n, int ldw, const double* __restrict__ W, int* __restrict__ flags) {
  const int j = blockIdx.x * COV_BLOCK + threadIdx.x;
  if (j >= n) return;
  const double l = W[(int64_t)j * ldw + j];
  if (!(l * l > COV_PIVOT_TINY) || !(l < 1.7e308)) flags[F_TINY] = 1;
}

// T: (32 blocks) x ldw with ldw = 32 blocks, zero outside the upper triangle of its first n rows and columns: no read needs a bound.
__global__ void __launch_bounds__(256)
k_unc_ttt(int n, int ldw, const double* __restrict__ T, const double* __restrict__ scale, double* __restrict__ C) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj < bi) return;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ti = wv >> 1, tj = wv & 1, lr = lane & 15, kq = 4 * (lane >> 4);
  const double* pa = T + (int64_t)(bi * NB + ti * 16 + lr) * ldw + kq;
  const double* pb = T + (int64_t)(bj * NB + tj * 16 + lr) * ldw + kq;
  v4f64 acc = {0.0, 0.0, 0.0, 0.0};
  // a lane loads 4 consecutive doubles of its row per 16-deep slab; MFMA step t pairs the t-th of each lane's four on both operands: the
  // same permutation of the depth index on both sides, so the sum is unchanged
  for (int q0 = bj * NB; q0 < ldw; q0 += 16) {
    const double2 a0 = *reinterpret_cast<const double2*>(pa + q0), a1 = *reinterpret_cast<const double2*>(pa + q0 + 2);
    const double2 b0 = *reinterpret_cast<const double2*>(pb + q0), b1 = *reinterpret_cast<const double2*>(pb + q0 + 2);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.x, b0.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0.y, b0.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.x, b1.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1.y, b1.y, acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int gi = bi * NB + ti * 16 + (lane >> 4) + 4 * r, gj = bj * NB + tj * 16 + lr;
    if (gi < n && gj < n && gi <= gj) {
      const double v = acc[r] * scale[gi] * scale[gj];
      C[(int64_t)gi * n + gj] = v;
      C[(int64_t)gj * n + gi] = v;
    }
  }
}

// `list` as k_unc_point's.  For the points of a constraint component the same kernel runs on the component's (camera, Y block) entries in the
// place of the point's observations: pt_start, cam_sorted and Y are then the entry tables k_unc_component filled.
template <int G> __global__ void __launch_bounds__(COV_POINT_THREADS)
k_unc_point_cov(const int32_t* __restrict__ list, const int64_t* __restrict__ pt_start, const int32_t* __restrict__ cam_sorted, const int32_t* __restrict__ cam_off, int32_t ncp,
                const double* __restrict__ Y, const double* __restrict__ Vinv, const double* __restrict__ Zbuf, const double* __restrict__ C,
                const double* __restrict__ E, const double* __restrict__ F, double sigma0_sq, double* __restrict__ out) {
  const int64_t p = list ? (int64_t)list[blockIdx.x] : (int64_t)blockIdx.x;
  const int t = threadIdx.x;
  const int64_t s = pt_start[p], k = pt_start[p + 1] - s;
  constexpr int WB = 3 * MAX_NC;
  double Z[3][G];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int j = 0; j < G; ++j) Z[a][j] = Zbuf[p * (3 * G) + a * G + j];
  double full[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  for (int64_t it = t; it < k * k; it += COV_POINT_THREADS) {  // Y_a^T C_ab Y_b
    const int64_t a = it / k, b = it % k;
    const int32_t cam_a = cam_sorted[s + a], off_a = cam_off[cam_a], np_a = cam_off[cam_a + 1] - off_a;
    const int32_t cam_b = cam_sorted[s + b], off_b = cam_off[cam_b], np_b = cam_off[cam_b + 1] - off_b;
    double Yb[WB];
#pragma unroll
    for (int e = 0; e < WB; ++e) Yb[e] = Y[(s + b) * WB + e];
#pragma unroll
    for (int r = 0; r < MAX_NC; ++r) {
      if (r < np_a) {
        const double* crow = C + (int64_t)(off_a + r) * ncp + off_b;
        double t3[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int c = 0; c < MAX_NC; ++c) {
          const double cv = c < np_b ? crow[c] : 0.0;
#pragma unroll
          for (int q = 0; q < 3; ++q) t3[q] += cv * Yb[3 * c + q];
        }
        const double* ya = Y + (s + a) * WB + 3 * r;
#pragma unroll
        for (int pp = 0; pp < 3; ++pp)
#pragma unroll
          for (int q = 0; q < 3; ++q) full[pp][q] += ya[pp] * t3[q];
      }
    }
  }
  for (int64_t a = t; a < k; a += COV_POINT_THREADS) {  // Y_a^T E_a Z^T and its transpose (the sum is symmetrised below: twice the term)
    const int32_t cam_a = cam_sorted[s + a], off_a = cam_off[cam_a], np_a = cam_off[cam_a + 1] - off_a;
#pragma unroll
    for (int r = 0; r < MAX_NC; ++r) {
      if (r < np_a) {
        const double* er = E + (int64_t)(off_a + r) * G;
        double t3[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < G; ++j) {
          const double ev = er[j];
#pragma unroll
          for (int q = 0; q < 3; ++q) t3[q] += ev * Z[q][j];
        }
        const double* ya = Y + (s + a) * WB + 3 * r;
#pragma unroll
        for (int pp = 0; pp < 3; ++pp)
#pragma unroll
          for (int q = 0; q < 3; ++q) full[pp][q] += 2.0 * ya[pp] * t3[q];
      }
    }
  }
#pragma unroll
  for (int pp = 0; pp < 3; ++pp)
#pragma unroll
    for (int q = 0; q < 3; ++q) full[pp][q] = wave_sum(full[pp][q]);
  if (t != 0) return;
  double Vi[6], Fm[G * G], P[6];
#pragma unroll
  for (int e = 0; e < 6; ++e) Vi[e] = Vinv[p * 6 + e];
#pragma unroll
  for (int e = 0; e < G * G; ++e) Fm[e] = F[e];
  cov_point_base(Vi, Z, Fm, P);
  int e = 0;
#pragma unroll
  for (int pp = 0; pp < 3; ++pp)
#pragma unroll
    for (int q = pp; q < 3; ++q) {
      out[p * 6 + e] = sigma0_sq * (P[e] + 0.5 * (full[pp][q] + full[q][pp]));
      ++e;
    }
}

// ---- constraint rows (cba_parameter_covariance_constrained) -------------------------------------------------------------------------------
// What the component kernel walks: the tables of covariance_constraint_plan.h on the device, and the stores it fills.
struct ConDev {
  int64_t n_rows;
  const int32_t* row_pt;      // [n_rows][8]
  const int32_t* row_loc;     // [n_rows][8]
  const double* row_dist;     // [n_rows]
  const double* row_weight;   // [n_rows]
  double* row_u;              // [n_rows][3]   weight * row scale * unit vector (k_unc_con_rows)
  double* row_coef;           // [n_rows][8]   signed multiplicities in quarters (k_unc_con_rows)
  const int64_t* comp_row;    // [n_comp + 1]
  const int64_t* comp_pt;     // [n_comp + 1]
  const int32_t* pts;
  const int64_t* comp_cam;    // [n_comp + 1]
  const int32_t* cams;
  const int64_t* cc_obs;      // [n (component, camera) + 1]
  const int64_t* obs_pos;
  const int32_t* obs_loc;
  const int64_t* entry_start; // [n_points + 1]
  double* Yc;                 // [entries][27] Y_c[:, i] of a constrained point i and a camera c of its component
  double* row_s;              // [n_rows] |X c_j^T|^2 for cba_observation_reliability_constrained, or nullptr: not formed
};

// one thread per kept constraint row: residual, robust scaling, the scaled Jacobian entries (u and the slots' coefficients), rho into the cost
__global__ void __launch_bounds__(COV_BLOCK)
k_unc_con_rows(ConDev cd, const double* __restrict__ points, int loss, double f_scale, double* __restrict__ cost) {
  const int64_t r = (int64_t)blockIdx.x * COV_BLOCK + threadIdx.x;
  double rho = 0.0;
  if (r < cd.n_rows) {
    int32_t pt[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) pt[s] = cd.row_pt[r * 8 + s];
    double u[3], coef[8];
    rho = cov_con_row(points, pt, cd.row_dist[r], cd.row_weight[r], loss, f_scale, u, coef);
#pragma unroll
    for (int k = 0; k < 3; ++k) cd.row_u[r * 3 + k] = u[k];
#pragma unroll
    for (int s = 0; s < 8; ++s) cd.row_coef[r * 8 + s] = coef[s];
  }
  rho = wave_sum(rho);
  if ((threadIdx.x & 63) == 0 && rho != 0.0) atomicAdd(cost, 0.5 * rho);
}

// One workgroup per constraint component k (m points, n = 3 m).  Dynamic LDS (cov_con_lds_doubles of the call's largest component): the packed
// lower triangle Vt of V~_k, two n x 9 panels pa and pb, Z_k (n x 6), a saved column and the diagonal V~_k started with.
//   1. Vt = the points' V_i (their observations' B^T B summed in sorted order) + the rows' outer products (LDS atomics: row after row, any count)
//   2. Vt = L (right-looking Cholesky, three barriers a column), then Vt = X = L^-1 in place from the last column to the first
//   3. Z_k = X^T (X Np) to LDS and to Zbuf, [V~_k^-1]_ii = (X^T X)_ii to Vinv: k_unc_d and k_unc_point_cov read them as they read a free point's
//   4. per camera c that sees the component: pa = W_c,k^T (n x 9, from the stored W blocks), pb = X pa, B_c -= W_c,k Z_k (atomics),
//      pa = Y_c^T = X^T pb to the entry store, Schur(c, c') -= Y_c W_c',k^T for the component's cameras c' >= c, upper triangle: one atomic per
//      entry of a block (the sum over the observations of c' is formed by the entry's thread).
// With cd.row_s (cba_observation_reliability_constrained) between 2. and 3.: a wave per row j, lanes over the entries of q = X c_j^T, s_j = |q|^2 by shuffles.
// A pivot that is not safely positive raises F_COMP with the component's first point; every branch on it is uniform (all threads read the pivot from LDS).
constexpr int COV_COMP_THREADS = 256;
__global__ void __launch_bounds__(COV_COMP_THREADS)
k_unc_component(ConDev cd, const int64_t* __restrict__ pt_start, const int32_t* __restrict__ cam_off, int32_t ncp,
                const double* __restrict__ points, const double* __restrict__ Wblk, const double* __restrict__ Vobs, double* __restrict__ Vinv,
                double* __restrict__ Zbuf, double* __restrict__ B, double* __restrict__ Sacc, int* __restrict__ flags) {
  extern __shared__ double cov_lds[];
  constexpr int G = COV_GAUGE_RIGID, WB = 3 * MAX_NC, NT = COV_COMP_THREADS;
  const int k = blockIdx.x, t = threadIdx.x;
  const int64_t p0 = cd.comp_pt[k];
  const int m = (int)(cd.comp_pt[k + 1] - p0), n = 3 * m, ntri = n * (n + 1) / 2;
  const int32_t* pts = cd.pts + p0;
  double* Vt = cov_lds;
  double* pa = Vt + ntri;
  double* pb = pa + n * MAX_NC;
  double* Zs = pb + n * MAX_NC;
  double* col = Zs + n * G;
  double* diag0 = col + n;
  // 1.
  for (int e = t; e < ntri; e += NT) Vt[e] = 0.0;
  __syncthreads();
  for (int i = t; i < m; i += NT) {
    const int64_t p = pts[i];
    double V[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t a = pt_start[p]; a < pt_start[p + 1]; ++a) {
#pragma unroll
      for (int e = 0; e < 6; ++e) V[e] += Vobs[a * 6 + e];
    }
    const int r = 3 * i;
    Vt[cov_tri(r, r)] = V[0];
    Vt[cov_tri(r + 1, r)] = V[1]; Vt[cov_tri(r + 1, r + 1)] = V[3];
    Vt[cov_tri(r + 2, r)] = V[2]; Vt[cov_tri(r + 2, r + 1)] = V[4]; Vt[cov_tri(r + 2, r + 2)] = V[5];
  }
  __syncthreads();
  const int64_t r0 = cd.comp_row[k], n_rows = cd.comp_row[k + 1] - r0;
  for (int64_t it = t; it < n_rows * 64; it += NT) {
    const int64_t r = r0 + it / 64;
    const int s = (int)(it % 64) / 8, s2 = (int)(it % 8);
    const double cc = cd.row_coef[r * 8 + s] * cd.row_coef[r * 8 + s2];
    if (cc == 0.0) continue;
    const int ri = 3 * cd.row_loc[r * 8 + s], rj = 3 * cd.row_loc[r * 8 + s2];
    const double u0 = cd.row_u[r * 3], u1 = cd.row_u[r * 3 + 1], u2 = cd.row_u[r * 3 + 2];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b)
        if (ri + a >= rj + b) atomicAdd(&Vt[cov_tri(ri + a, rj + b)], cc * (a == 0 ? u0 : (a == 1 ? u1 : u2)) * (b == 0 ? u0 : (b == 1 ? u1 : u2)));
  }
  __syncthreads();
  for (int i = t; i < n; i += NT) diag0[i] = Vt[cov_tri(i, i)];
  __syncthreads();
  // 2.
  for (int j = 0; j < n; ++j) {
    const double d = Vt[cov_tri(j, j)];
    if (!cov_con_pivot_ok(d, diag0[j])) {
      if (t == 0) { flags[F_COMP] = 1; atomicMax(&flags[F_COMP_WHICH], (int)pts[0] + 1); }
      return;
    }
    const double ljj = sqrt(d);
    __syncthreads();  // (every thread has read the pivot)
    for (int i = j + t; i < n; i += NT) Vt[cov_tri(i, j)] = i == j ? ljj : Vt[cov_tri(i, j)] / ljj;
    __syncthreads();
    for (int i = j + 1 + (t >> 4); i < n; i += NT / 16) {
      const double lij = Vt[cov_tri(i, j)];
      for (int c = j + 1 + (t & 15); c <= i; c += 16) Vt[cov_tri(i, c)] -= lij * Vt[cov_tri(c, j)];
    }
    __syncthreads();
  }
  for (int j = n - 1; j >= 0; --j) {
    const double xjj = 1.0 / Vt[cov_tri(j, j)];
    for (int i = j + 1 + t; i < n; i += NT) col[i] = Vt[cov_tri(i, j)];
    __syncthreads();
    for (int i = j + t; i < n; i += NT) Vt[cov_tri(i, j)] = i == j ? xjj : cov_tri_inverse_entry(Vt, i, j, col, xjj);
    __syncthreads();
  }
  if (cd.row_s) {  // (uniform; Vt is X from here to the end)
    for (int64_t r = r0 + (t >> 6); r < r0 + n_rows; r += NT / 64) {
      int32_t loc[8];
      double coef[8];
#pragma unroll
      for (int s = 0; s < 8; ++s) { loc[s] = cd.row_loc[r * 8 + s]; coef[s] = cd.row_coef[r * 8 + s]; }
      const double u[3] = {cd.row_u[r * 3], cd.row_u[r * 3 + 1], cd.row_u[r * 3 + 2]};
      double acc = 0.0;
      for (int i = t & 63; i < n; i += 64) {
        const double q = rel_con_x_row(Vt, i, loc, coef, u);
        acc += q * q;
      }
      acc = wave_sum(acc);
      if ((t & 63) == 0) cd.row_s[r] = acc;
    }
  }
  // 3.
  for (int i = t; i < m; i += NT) {
    const int64_t p = pts[i];
    double N[3][G];
    cov_gauge_point(points[3 * p], points[3 * p + 1], points[3 * p + 2], N);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int j = 0; j < G; ++j) pa[(3 * i + a) * G + j] = N[a][j];
  }
  __syncthreads();
  for (int it = t; it < n * G; it += NT) pb[it] = cov_tri_lower_dot(Vt, it / G, pa, G, it % G);
  __syncthreads();
  for (int it = t; it < n * G; it += NT) {
    const int i = it / G, j = it % G;
    const double z = cov_tri_upper_dot(Vt, n, i, pb, G, j);
    Zs[it] = z;
    Zbuf[(int64_t)pts[i / 3] * (3 * G) + (i % 3) * G + j] = z;
  }
  for (int it = t; it < m * 6; it += NT) {
    const int i = it / 6, e = it % 6;
    Vinv[(int64_t)pts[i] * 6 + e] = cov_tri_gram(Vt, n, 3 * i + cov_sym3_row(e), 3 * i + cov_sym3_col(e));
  }
  __syncthreads();
  // 4.
  const int64_t q0 = cd.comp_cam[k];
  const int nc = (int)(cd.comp_cam[k + 1] - q0);
  for (int cc = 0; cc < nc; ++cc) {
    const int32_t cam = cd.cams[q0 + cc], off = cam_off[cam], np = cam_off[cam + 1] - off;
    const int64_t o0 = cd.cc_obs[q0 + cc], n_o = cd.cc_obs[q0 + cc + 1] - o0;
    for (int it = t; it < n * MAX_NC; it += NT) pa[it] = 0.0;
    __syncthreads();
    for (int64_t it = t; it < n_o * WB; it += NT) {  // (a repeated (camera, point) pair adds twice: atomics)
      const int64_t a = o0 + it / WB;
      const int e = (int)(it % WB), r = e / 3, q = e % 3;
      atomicAdd(&pa[(3 * cd.obs_loc[a] + q) * MAX_NC + r], Wblk[cd.obs_pos[a] * WB + e]);
    }
    __syncthreads();
    for (int it = t; it < n * MAX_NC; it += NT) pb[it] = cov_tri_lower_dot(Vt, it / MAX_NC, pa, MAX_NC, it % MAX_NC);
    for (int it = t; it < np * G; it += NT) {
      const int r = it / G, j = it % G;
      double v = 0.0;
      for (int i = 0; i < n; ++i) v += pa[i * MAX_NC + r] * Zs[i * G + j];
      atomicAdd(&B[(int64_t)(off + r) * G + j], -v);
    }
    __syncthreads();
    for (int it = t; it < n * MAX_NC; it += NT) {
      const int i = it / MAX_NC, r = it % MAX_NC;
      const double y = cov_tri_upper_dot(Vt, n, i, pb, MAX_NC, r);
      pa[it] = y;
      cd.Yc[(cd.entry_start[pts[i / 3]] + cc) * WB + 3 * r + (i % 3)] = y;
    }
    __syncthreads();
    for (int it = t; it < (nc - cc) * (MAX_NC * MAX_NC); it += NT) {
      const int c2 = cc + it / (MAX_NC * MAX_NC), e = it % (MAX_NC * MAX_NC), r = e / MAX_NC, c = e % MAX_NC;
      const int32_t cam_b = cd.cams[q0 + c2], off_b = cam_off[cam_b], np_b = cam_off[cam_b + 1] - off_b;
      const int32_t row = off + r, colm = off_b + c;
      if (r >= np || c >= np_b || row > colm) continue;
      double v = 0.0;
      for (int64_t a = cd.cc_obs[q0 + c2]; a < cd.cc_obs[q0 + c2 + 1]; ++a) {
        const double* w = Wblk + cd.obs_pos[a] * WB + 3 * c;
        const double* y = pa + 3 * cd.obs_loc[a] * MAX_NC + r;
        v += y[0] * w[0] + y[MAX_NC] * w[1] + y[2 * MAX_NC] * w[2];
      }
      atomicAdd(&Sacc[(int64_t)row * ncp + colm], -v);
    }
    __syncthreads();
  }
}

// Everything up to C with G gauge columns.  `con` (G = 6 only): the components of the constraint rows (cov_con_components, at least one row);
// its tables are completed here, once the observations are sorted.  nullptr (G = 7): the launches of the unconstrained call, as they always were.
// `reliability` (with `con`): the caller is cba_observation_reliability_constrained; its stores count in the memory check and k_unc_component leaves row_s.
template <int G>
int cov_pipeline_run(const cba_cov_desc* d, int32_t device, const char* what, bool canonical, CovConPlan* con, const std::function<int(const CovPipeline&)>& finish,
                     bool reliability = false) {
  // every index the kernels use, checked on the host before anything reaches the device
  std::string msg;
  CovPlan plan;
  int rc = cov_validate(d, plan, msg, what, canonical, G, con ? con->in_row.data() : nullptr, con ? con->n_rows : 0);
  if (rc) return err(rc, msg);
  if (con && cov_fixed_order_requested()) return err(CBA_ERR_UNSUPPORTED, cov_con_msg_fixed_order(what));
  rc = select_device(device, what);
  if (rc) return rc;
  const int32_t n_cams = d->n_cams, ncp = plan.ncp();
  const int64_t n_obs = d->n_obs, n_points = d->n_points;
  if (con) {
    cov_con_tables(plan, d->obs_cam, n_cams, n_points, *con);
    size_t free_bytes = 0, total_bytes = 0;
    if (hipMemGetInfo(&free_bytes, &total_bytes) != hipSuccess) return err(CBA_ERR_HIP, std::string(what) + ": hipMemGetInfo failed");
    rc = cov_con_memory_check(cov_con_device_bytes(d, ncp, *con) + (reliability ? cov_con_reliability_bytes(d, *con) : 0.0), (double)free_bytes, msg, what);
    if (rc) return err(rc, msg);
  }
  const int nbk = (ncp + NB - 1) / NB, ldw = nbk * NB;  // the work matrix and T padded to whole blocks: k_unc_ttt reads without bounds
  std::vector<int32_t> param_cam((size_t)ncp), param_loc((size_t)ncp);
  for (int32_t c = 0; c < n_cams; ++c)
    for (int32_t r = plan.cam_off[(size_t)c]; r < plan.cam_off[(size_t)c + 1]; ++r) { param_cam[(size_t)r] = c; param_loc[(size_t)r] = r - plan.cam_off[(size_t)c]; }
  std::vector<double> cam_x((size_t)n_cams * MAX_NC, 0.0);  // (the caller's rows behind a six-parameter camera's pose are not read)
  for (int32_t c = 0; c < n_cams; ++c)
    for (int i = 0; i < d->cam_nparams[c]; ++i) cam_x[(size_t)c * MAX_NC + i] = d->cam_x[(size_t)c * MAX_NC + i];

  Buffers buf;
  const int32_t* dmodel = buf.in(d->cam_model, n_cams);
  const int32_t* dcam_off = buf.in(plan.cam_off.data(), n_cams + 1);
  const double* dconst = buf.in(d->cam_const, n_cams, CAM_CONST_STRIDE);
  const double* dcam_x = buf.in(cam_x.data(), n_cams, MAX_NC);
  const double* dpoints = buf.in(d->points, n_points, 3);
  const int32_t* dobs_cam = buf.in(d->obs_cam, n_obs);
  const int32_t* dobs_pt = buf.in(d->obs_pt, n_obs);
  const double* dobs_uv = buf.in(d->obs_uv, n_obs, 2);
  const int64_t* dorder = buf.in(plan.order.data(), n_obs);
  const int64_t* dpt_start = buf.in(plan.pt_start.data(), n_points + 1);
  const int32_t* dparam_cam = buf.in(param_cam.data(), ncp);
  const int32_t* dparam_loc = buf.in(param_loc.data(), ncp);
  double* dtab = buf.make<double>(n_cams, CAMTAB_DOUBLES);
  double* dWblk = buf.make<double>(n_obs, 3 * MAX_NC);
  double* dVobs = buf.make<double>(n_obs, 6);
  double* dY = buf.make<double>(n_obs, 3 * MAX_NC);
  int32_t* dcam_sorted = buf.make<int32_t>(n_obs);
  double* dVinv = buf.make<double>(n_points, 6);
  double* dZ = buf.make<double>(n_points, 3 * G);
  double* dB = buf.make<double>(ncp, G);
  double* dscale = buf.make<double>(ncp);
  double* dC = buf.make<double>(ncp, ncp);
  const bool fixed_order = !con && cov_fixed_order_requested();  // (as caliscope_amd/engine_cache.py reads it)
  const int64_t d_blocks_all = (n_points + COV_BLOCK - 1) / COV_BLOCK;
  const int d_grid = (int)(d_blocks_all < COV_D_BLOCKS ? d_blocks_all : COV_D_BLOCKS), d_rows = d_grid * (COV_BLOCK / 64);
  double* dD_rows = fixed_order ? buf.make<double>(d_rows, COV_D_SUMS) : nullptr;
  double* dcam_cost = fixed_order ? buf.make<double>(n_cams) : nullptr;
  double* dXinv = buf.make<double>(chol_xinv_blocks(nbk), NB * NB);  // the inverses of the diagonal blocks and the side slots of the early update
  // the tables of the constraint components and what their kernels store
  ConDev cd = {};
  const int32_t* dfree = nullptr;
  const int32_t* dentry_cam = nullptr;
  const int64_t* drow_src = nullptr;
  int64_t n_free = n_points;
  if (con) {
    n_free = (int64_t)con->free_pts.size();
    cd.n_rows = con->n_rows;
    cd.row_pt = buf.in(con->row_pt.data(), con->n_rows, 8);
    cd.row_loc = buf.in(con->row_loc.data(), con->n_rows, 8);
    cd.row_dist = buf.in(con->row_dist.data(), con->n_rows);
    cd.row_weight = buf.in(con->row_weight.data(), con->n_rows);
    cd.row_u = buf.make<double>(con->n_rows, 3);
    cd.row_coef = buf.make<double>(con->n_rows, 8);
    cd.comp_row = buf.in(con->comp_row.data(), con->n_comp + 1);
    cd.comp_pt = buf.in(con->comp_pt.data(), con->n_comp + 1);
    cd.pts = buf.in(con->pts.data(), con->pts.size());
    cd.comp_cam = buf.in(con->comp_cam.data(), con->n_comp + 1);
    cd.cams = buf.in(con->cams.data(), con->cams.size());
    cd.cc_obs = buf.in(con->cc_obs.data(), con->cc_obs.size());
    cd.obs_pos = buf.in(con->obs_pos.data(), con->obs_pos.size());
    cd.obs_loc = buf.in(con->obs_loc.data(), con->obs_loc.size());
    cd.entry_start = buf.in(con->entry_start.data(), n_points + 1);
    cd.Yc = buf.make<double>(con->n_entries(), 3 * MAX_NC);
    dfree = buf.in(con->free_pts.data(), con->free_pts.size());
    dentry_cam = buf.in(con->entry_cam.data(), con->entry_cam.size());
    if (reliability) {
      cd.row_s = buf.make<double>(con->n_rows);
      drow_src = buf.in(con->row_src.data(), con->n_rows);
    }
  }
  // zeroed in one block: the work matrix [ldw + 1][ldw] and T [ldw][ldw] (first: their rows are read sixteen bytes at a time), U [n_cams][81],
  // Schur [ncp][ncp], D [G][G], cost [1], flags
  const size_t n_U = (size_t)n_cams * MAX_NC * MAX_NC, n_S = (size_t)ncp * ncp, n_W = ((size_t)ldw + 1) * ldw, n_T = (size_t)ldw * ldw;
  const size_t n_zero = n_U + n_S + G * G + 1 + n_W + n_T + N_FLAGS;
  double* dzero = buf.make<double>(n_zero);
  if (buf.status()) return buf.result(what);
  double* dW = dzero;
  double* dT = dW + n_W;
  double* dU = dT + n_T;
  double* dSacc = dU + n_U;
  double* dD = dSacc + n_S;
  double* dcost = dD + G * G;
  int* dflags = reinterpret_cast<int*>(dcost + 1);
  buf.check(hipMemsetAsync(dzero, 0, n_zero * sizeof(double), 0));
  if (buf.status()) return buf.result(what);

  const auto blocks = [](int64_t n) { return dim3((unsigned)((n + COV_BLOCK - 1) / COV_BLOCK)); };
  hipLaunchKernelGGL(k_unc_cam<G>, blocks(n_cams), dim3(COV_BLOCK), 0, 0, n_cams, dmodel, dcam_off, dconst, dcam_x, dtab, dB);
  hipLaunchKernelGGL(k_unc_obs, blocks(n_obs), dim3(COV_BLOCK), 0, 0, n_obs, dorder, dobs_cam, dobs_pt, dobs_uv, (const double*)dtab, dpoints, (int)d->loss,
                     d->f_scale, dWblk, dVobs, dcam_sorted, dU, dcost, fixed_order);
  if (fixed_order)
    hipLaunchKernelGGL(k_unc_cam_sums, dim3((unsigned)n_cams), dim3(64), 0, 0, n_obs, dorder, dobs_pt, dobs_uv, (const double*)dtab, dpoints, (int)d->loss, d->f_scale,
                       (const int32_t*)dcam_sorted, dU, dcam_cost);
  if (n_free > 0)  // (n_free == n_points without constraint rows)
    hipLaunchKernelGGL(k_unc_point<G>, dim3((unsigned)n_free), dim3(COV_POINT_THREADS), 0, 0, dfree, dpt_start, (const int32_t*)dcam_sorted, dcam_off, ncp, dpoints,
                       (const double*)dWblk, (const double*)dVobs, dY, dVinv, dZ, dB, dSacc, dflags, fixed_order);
  if constexpr (G == COV_GAUGE) {
    if (fixed_order)  // (a point whose observations do not determine it has raised F_POINT: the call returns below before anything reads these sums)
      hipLaunchKernelGGL(k_unc_rows, dim3((unsigned)n_cams), dim3(COV_ROWS_THREADS), 0, 0, n_points, dpt_start, (const int32_t*)dcam_sorted, dcam_off, ncp,
                         (const double*)dWblk, (const double*)dY, (const double*)dZ, dB, dSacc);
  }
  if (con) {
    const size_t lds = cov_con_lds_doubles(con->max_m) * sizeof(double);
    buf.check(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_unc_component), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (buf.status()) return buf.result(what);
    hipLaunchKernelGGL(k_unc_con_rows, blocks(con->n_rows), dim3(COV_BLOCK), 0, 0, cd, dpoints, (int)d->loss, d->f_scale, dcost);
    hipLaunchKernelGGL(k_unc_component, dim3((unsigned)con->n_comp), dim3(COV_COMP_THREADS), lds, 0, cd, dpt_start, dcam_off, ncp, dpoints, (const double*)dWblk,
                       (const double*)dVobs, dVinv, dZ, dB, dSacc, dflags);
  }
  hipLaunchKernelGGL(k_unc_d<G>, dim3((unsigned)d_grid), dim3(COV_BLOCK), 0, 0, n_points, dpoints, (const double*)dZ, dD, dD_rows);
  if constexpr (G == COV_GAUGE) {
    if (fixed_order)
      hipLaunchKernelGGL(k_unc_fixed_sums, dim3(1), dim3(64), 0, 0, (const double*)dD_rows, d_rows, (const double*)dcam_cost, n_cams, dD, dcost);
  }
  buf.check(hipGetLastError());
  std::vector<double> D(G * G + 1);  // D and the cost behind it
  std::vector<int> flags(N_FLAGS, 0);
  buf.out(D.data(), (const double*)dD, G * G + 1);
  buf.out(flags.data(), (const int*)dflags, N_FLAGS);
  if (buf.status()) return buf.result(what);
  if (flags[F_POINT]) return err(CBA_ERR_NUMERIC, cov_msg_point(what, flags[F_WHICH] - 1));
  if (flags[F_COMP]) return err(CBA_ERR_NUMERIC, cov_con_msg_component(what, flags[F_COMP_WHICH] - 1));
  const double cost = D[G * G];
  D.resize(G * G);
  for (int j = 0; j < G; ++j)
    for (int m = j + 1; m < G; ++m) D[(size_t)m * G + j] = D[(size_t)j * G + m];
  if (!std::isfinite(cost) || !cov_spd_inverse(D, G)) return err(CBA_ERR_NUMERIC, cov_msg_gauge(what, G));
  const double sigma0_sq = 2.0 * cost / (double)plan.dof;
  const double* dDinv = buf.in(D.data(), G * G);
  if (buf.status()) return buf.result(what);

  hipLaunchKernelGGL(k_unc_assemble<G>, blocks((int64_t)ncp * ncp), dim3(COV_BLOCK), 0, 0, ncp, ldw, (const double*)dU, (const double*)dSacc, (const double*)dB, dDinv,
                     dparam_cam, dparam_loc, dW, dscale, dflags);
  enqueue_chol_factor(dW, ncp, ldw, dflags, nullptr, dXinv, dT, chol_early_from_env(), 0, false, false);  // (all launches, none paired: T and L's diagonal are read here)
  hipLaunchKernelGGL(k_unc_pivots, blocks(ncp), dim3(COV_BLOCK), 0, 0, (int)ncp, ldw, (const double*)dW, dflags);
  hipLaunchKernelGGL(k_unc_ttt, dim3((unsigned)nbk, (unsigned)nbk), dim3(256), 0, 0, (int)ncp, ldw, (const double*)dT, (const double*)dscale, dC);
  buf.check(hipGetLastError());
  std::vector<double> C(n_S), B((size_t)ncp * G);
  buf.out(flags.data(), (const int*)dflags, N_FLAGS);
  buf.out(C.data(), (const double*)dC, ncp, ncp);
  buf.out(B.data(), (const double*)dB, ncp, G);
  if (buf.status()) return buf.result(what);
  if (flags[F_DIAG] || flags[F_CHOL] || flags[F_TINY]) return err(CBA_ERR_NUMERIC, cov_msg_not_pd(what));
  const CovPipeline pipe = {&plan, n_cams, ncp, n_obs, n_points, dorder, dpt_start, dcam_sorted, dcam_off, dtab, dpoints, dobs_uv, dY, dVinv, dZ, dC,
                            &C, &B, &D, sigma0_sq, cost, G, dfree, n_free, cd.pts, con ? (int64_t)con->pts.size() : 0, cd.entry_start, dentry_cam, cd.Yc,
                            con, con ? con->n_rows : 0, cd.row_pt, cd.row_u, cd.row_coef, cd.row_dist, cd.row_weight, drow_src, cd.row_s, cd.comp_row, cd.comp_cam, cd.cams};
  return finish(pipe);
}

// The point blocks, the checks of the results and the caller's arrays: what both entry points do with the pipeline's C.
template <int G>
int cov_outputs(const CovPipeline& pipe, const char* what, cba_cov_out* out) {
    const int32_t ncp = pipe.ncp;
    const int64_t n_points = pipe.n_points;
    const std::vector<double>& C = *pipe.C_host;
    const double sigma0_sq = pipe.sigma0_sq;
    Buffers buf;
    std::vector<double> point_cov;
    if (out->point_cov) {
      std::vector<double> E, F;
      cov_gauge_terms<G>(ncp, C.data(), pipe.B_host->data(), pipe.Dinv_host->data(), E, F);
      const double* dE = buf.in(E.data(), ncp, G);
      const double* dF = buf.in(F.data(), G * G);
      double* dout = buf.make<double>(n_points, 6);
      if (buf.status()) return buf.result(what);
      if (pipe.n_free > 0)  // (every point without constraint rows)
        hipLaunchKernelGGL(k_unc_point_cov<G>, dim3((unsigned)pipe.n_free), dim3(COV_POINT_THREADS), 0, 0, pipe.free_list, pipe.pt_start, pipe.cam_sorted, pipe.cam_off,
                           ncp, pipe.Y, pipe.Vinv, pipe.Z, pipe.C, dE, dF, sigma0_sq, dout);
      if (pipe.n_con_pts > 0)  // the points of the components: their entries in the place of observations
        hipLaunchKernelGGL(k_unc_point_cov<G>, dim3((unsigned)pipe.n_con_pts), dim3(COV_POINT_THREADS), 0, 0, pipe.con_list, pipe.entry_start, pipe.entry_cam,
                           pipe.cam_off, ncp, pipe.Yc, pipe.Vinv, pipe.Z, pipe.C, dE, dF, sigma0_sq, dout);
      buf.check(hipGetLastError());
      point_cov.resize((size_t)n_points * 6);
      buf.out(point_cov.data(), (const double*)dout, n_points, 6);
      if (buf.status()) return buf.result(what);
      for (double v : point_cov)
        if (!std::isfinite(v)) return err(CBA_ERR_NUMERIC, cov_msg_not_finite(what, "point"));
    }
    for (double v : C)
      if (!std::isfinite(v)) return err(CBA_ERR_NUMERIC, cov_msg_not_finite(what, "camera"));
    // outputs, written only now: a failed call leaves the caller's arrays alone
    if (out->point_cov) std::copy(point_cov.begin(), point_cov.end(), out->point_cov);
    cov_write_outputs(*pipe.plan, C, sigma0_sq, pipe.cost, out);
    return CBA_OK;
}

}  // namespace

// covariance_pipeline.h: everything up to C, shared with cba_observation_reliability (reliability_lib.hip)
int cba::cov_pipeline(const cba_cov_desc* d, int32_t device, const char* what, bool canonical, const std::function<int(const CovPipeline&)>& finish) {
  return cov_pipeline_run<COV_GAUGE>(d, device, what, canonical, nullptr, finish);
}

// the same with the constraint rows, for cba_observation_reliability_constrained; without a row of positive weight: cov_pipeline itself
int cba::cov_pipeline_constrained(const cba_cov_desc* d, const cba_cov_constraints* constraints, int32_t device, const char* what, bool canonical,
                                  const std::function<int(const CovPipeline&)>& finish) {
  if (d->n_points <= 0 || d->n_points > INT32_MAX) return cov_pipeline(d, device, what, canonical, finish);  // (refused there)
  std::string msg;
  CovConPlan con;
  const int rc = cov_con_components(d->n_points, constraints, con, msg, what);
  if (rc) return err(rc, msg);
  if (con.n_rows == 0) return cov_pipeline(d, device, what, canonical, finish);
  return cov_pipeline_run<COV_GAUGE_RIGID>(d, device, what, canonical, &con, finish, true);
}

extern "C" int cba_parameter_covariance(const cba_cov_desc* d, int32_t device, cba_cov_out* out) {
  const char* what = "cba_parameter_covariance";
  if (!d || !out) return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  return cov_pipeline(d, device, what, false, [&](const CovPipeline& pipe) -> int { return cov_outputs<COV_GAUGE>(pipe, what, out); });
}

// include/caliscope/uncertainty_constrained.h.  Without a row of positive weight: cba_parameter_covariance itself.
extern "C" int cba_parameter_covariance_constrained(const cba_cov_desc* d, const cba_cov_constraints* constraints, int32_t device, cba_cov_out* out) {
  const char* what = "cba_parameter_covariance_constrained";
  if (!d || !out) return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  if (d->n_points <= 0 || d->n_points > INT32_MAX) return cba_parameter_covariance(d, device, out);  // (refused there, by name)
  std::string msg;
  CovConPlan con;
  const int rc = cov_con_components(d->n_points, constraints, con, msg, what);
  if (rc) return err(rc, msg);
  if (con.n_rows == 0) return cba_parameter_covariance(d, device, out);
  return cov_pipeline_run<COV_GAUGE_RIGID>(d, device, what, false, &con, [&](const CovPipeline& pipe) -> int { return cov_outputs<COV_GAUGE_RIGID>(pipe, what, out); });
}
