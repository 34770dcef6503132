// cba_observation_reliability of libcaliscope_ba.so (C ABI: include/caliscope/reliability.h): per observation the 2 x 2 redundancy block
// R_oo = I - J_o (J^T J)^- J_o^T, the standardised residuals w and the scaled residuals.  Everything up to C = St^-1 is cov_pipeline of
// covariance_lib.hip (covariance_pipeline.h); the formulas and the per-element arithmetic are reliability_math.h (shared with
// tests/native/reliability_harness.cpp); this file holds the one kernel behind the pipeline and the entry point.  Everything is FP64.
//
//   k_rel_point   one wave per point.  First the camera part: four observations at a time, sixteen lanes each; lane r < np_a of observation o
//                 forms row r of G_o = sum_b' C_{a,cam(b')} Y_b' (the nine-wide pieces of row off_a + r of C, one per observation of the
//                 point: C stays cache-resident) and row r of C_aa A_o^T, and adds its terms to Q_i (per lane, summed over the wave at the
//                 end), to A_o G_o and to A_o C_aa A_o^T (summed over the sixteen lanes by shuffles); the first lane of the group leaves
//                 A C_aa A^T - sym(A G B^T) in the observation's row of the output.  Then, Q_i known, one lane per observation adds
//                 B_o (V^-1 + Q_i) B_o^T and writes R_oo, w and f~ to the caller's row.  A_o, B_o are recomputed (cov_obs_jacobian), not stored.
//
// No sum crosses a point: no floating-point atomics, the same bits for the same C.  The call asks cov_pipeline for the canonical order of a
// point's observations, so with CBA_DETERMINISTIC=1 a permutation of the caller's rows permutes the outputs and changes no bit.  The count of uncontrolled rows is a per-wave sum and
// one integer atomic; a block that is not finite raises a flag beside it, which the host reads before it copies anything back.  The rows of C start at multiples of three doubles, so its pieces are loaded one double at a time.  Null stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "ba_math.h"
#include "covariance_pipeline.h"
#include "device_call.h"
#include "reliability_math.h"

using namespace cba;

namespace {

static_assert(COV_POINT_THREADS == 64 && COV_POINT_THREADS % REL_GROUP == 0 && MAX_NC <= REL_GROUP, "k_rel_point: one wave, whole groups");
constexpr int REL_GROUPS = COV_POINT_THREADS / REL_GROUP;

__device__ __forceinline__ double group_sum(double v) {  // over the REL_GROUP lanes of a group, in every lane
#pragma unroll
  for (int m = REL_GROUP / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__device__ __forceinline__ double wave_total(double v) {  // over the wave, the same bits in every lane
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return __shfl(v, 0, 64);
}

__global__ void __launch_bounds__(COV_POINT_THREADS)
k_rel_point(const int64_t* __restrict__ pt_start, const int64_t* __restrict__ order, const int32_t* __restrict__ cam_sorted,
            const int32_t* __restrict__ cam_off, int32_t ncp, const double* __restrict__ tab, const double* __restrict__ points,
            const double* __restrict__ obs_uv, int loss, double f_scale, const double* __restrict__ Y, const double* __restrict__ Vinv,
            const double* __restrict__ C, double sigma0, double* out_r, double* __restrict__ out_w, double* __restrict__ out_f,
            unsigned long long* __restrict__ counts) {  // counts[0]: uncontrolled rows, counts[1]: set when an R_oo is not finite
  constexpr int WB = 3 * MAX_NC;
  const int64_t p = blockIdx.x;
  const int t = threadIdx.x, grp = t / REL_GROUP, r = t % REL_GROUP;
  const int64_t s = pt_start[p], k = pt_start[p + 1] - s;
  const double X[3] = {points[3 * p], points[3 * p + 1], points[3 * p + 2]};
  double Q[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t b0 = 0; b0 < k; b0 += REL_GROUPS) {  // (the same trip count in every lane: the shuffles below need the whole wave)
    const int64_t b = b0 + grp;
    double M[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, S[3] = {0.0, 0.0, 0.0};
    double A[2][MAX_NC], B[2][3];
    int64_t o = 0;
    bool row = false;
    if (b < k) {
      o = order[s + b];
      const int32_t cam = cam_sorted[s + b], off = cam_off[cam], np = cam_off[cam + 1] - off;
      row = r < np;
      if (row) {
        const double uv[2] = {obs_uv[2 * o], obs_uv[2 * o + 1]};
        cov_obs_jacobian(reinterpret_cast<const CamTab*>(tab)[cam], X, uv, loss, f_scale, A, B);
        const double* crow = C + (int64_t)(off + r) * ncp;
        double g[3] = {0.0, 0.0, 0.0}, h[2], a[2];
        for (int64_t bp = 0; bp < k; ++bp) {
          const int32_t cam_b = cam_sorted[s + bp], off_b = cam_off[cam_b], np_b = cam_off[cam_b + 1] - off_b;
          rel_row_times_y(crow + off_b, np_b, Y + (s + bp) * WB, g);
        }
        rel_row_times_a(crow + off, np, A, h);
        rel_a_column(A, r, a);
        const double yr[3] = {Y[(s + b) * WB + 3 * r], Y[(s + b) * WB + 3 * r + 1], Y[(s + b) * WB + 3 * r + 2]};
        rel_row_terms(a, yr, g, h, Q, M, S);
      }
    }
#pragma unroll
    for (int e = 0; e < 6; ++e) M[e] = group_sum(M[e]);
#pragma unroll
    for (int e = 0; e < 3; ++e) S[e] = group_sum(S[e]);
    if (row && r == 0) {  // (row 0 exists for every camera: this lane holds B_o)
      double T[3];
      rel_camera_part(S, M, B, T);
#pragma unroll
      for (int e = 0; e < 3; ++e) out_r[3 * o + e] = T[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 9; ++e) Q[e] = wave_total(Q[e]);
  __threadfence_block();
  __syncthreads();  // (the camera parts in out_r are read below by other lanes of this wave)
  double Vi[6];
#pragma unroll
  for (int e = 0; e < 6; ++e) Vi[e] = Vinv[p * 6 + e];
  int bad = 0;
  for (int64_t b = t; b < k; b += COV_POINT_THREADS) {
    const int64_t o = order[s + b];
    const int32_t cam = cam_sorted[s + b];
    const double uv[2] = {obs_uv[2 * o], obs_uv[2 * o + 1]};
    double A[2][MAX_NC], B[2][3], fs[2], R[3], w[2];
    cov_obs_jacobian(reinterpret_cast<const CamTab*>(tab)[cam], X, uv, loss, f_scale, A, B, fs);
    const double T[3] = {out_r[3 * o], out_r[3 * o + 1], out_r[3 * o + 2]};
    bad += rel_finish(B, Vi, Q, T, sigma0, fs, R, w);
    if (!isfinite(R[0] + R[1] + R[2])) counts[1] = 1;
#pragma unroll
    for (int e = 0; e < 3; ++e) out_r[3 * o + e] = R[e];
    out_w[2 * o] = w[0]; out_w[2 * o + 1] = w[1];
    out_f[2 * o] = fs[0]; out_f[2 * o + 1] = fs[1];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, 64);
  if (t == 0 && bad) atomicAdd(&counts[0], (unsigned long long)bad);
}

}  // namespace

extern "C" int cba_observation_reliability(const cba_cov_desc* d, int32_t device, cba_rel_out* out) {
  const char* what = "cba_observation_reliability";
  if (!d || !out) return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  return cov_pipeline(d, device, what, true, [&](const CovPipeline& pipe) -> int {
    for (double v : *pipe.C_host)
      if (!std::isfinite(v)) return err(CBA_ERR_NUMERIC, cov_msg_not_finite(what, "camera"));
    const int64_t n_obs = pipe.n_obs;
    Buffers buf;
    double* dr = buf.make<double>(n_obs, 3);
    double* dw = buf.make<double>(n_obs, 2);
    double* df = buf.make<double>(n_obs, 2);
    unsigned long long* dcounts = buf.make<unsigned long long>(2);
    if (buf.status()) return buf.result(what);
    buf.check(hipMemsetAsync(dcounts, 0, 2 * sizeof(unsigned long long), 0));
    hipLaunchKernelGGL(k_rel_point, dim3((unsigned)pipe.n_points), dim3(COV_POINT_THREADS), 0, 0, pipe.pt_start, pipe.order, pipe.cam_sorted, pipe.cam_off,
                       pipe.ncp, pipe.tab, pipe.points, pipe.obs_uv, (int)d->loss, d->f_scale, pipe.Y, pipe.Vinv, pipe.C, std::sqrt(pipe.sigma0_sq), dr, dw,
                       df, dcounts);
    buf.check(hipGetLastError());
    unsigned long long counts[2] = {0, 0};
    buf.out(counts, (const unsigned long long*)dcounts, 2);
    if (buf.status()) return buf.result(what);
    if (counts[1]) return err(CBA_ERR_NUMERIC, std::string(what) + ": a redundancy number is not finite");
    // outputs, only now and straight into the caller's arrays (seven doubles per observation: no second copy on the host): every check has passed
    buf.out(out->redundancy, (const double*)dr, n_obs, 3);
    buf.out(out->w, (const double*)dw, n_obs, 2);
    buf.out(out->residual, (const double*)df, n_obs, 2);
    if (buf.status()) return buf.result(what);
    if (out->sigma0_sq) *out->sigma0_sq = pipe.sigma0_sq;
    if (out->dof) *out->dof = pipe.plan->dof;
    if (out->cost) *out->cost = pipe.cost;
    if (out->n_uncontrolled) *out->n_uncontrolled = (int64_t)counts[0];
    return CBA_OK;
  });
}
