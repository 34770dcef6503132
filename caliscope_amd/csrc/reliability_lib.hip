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
// cba_observation_reliability_constrained (include/caliscope/reliability_constrained.h; arithmetic: reliability_constraint_math.h) is the same report with the
// rigid-distance rows in J, behind cov_pipeline_constrained (six gauge columns; k_unc_component of covariance_lib.hip also leaves s_j = |X c_j^T|^2):
//   k_rel_point       on the list of the points in no row;
//   k_rel_con_point   one wave per point of a component.  First its (component camera, Yc block) entries, four at a time, sixteen lanes each: lane r of
//                     entry e forms row r of G_e = sum_e' C_{cam(e),cam(e')} Yc[e'], adds Yc[e][r]^T g to Q_i (summed over the wave at the end) and
//                     leaves g in a device store laid out as Yc.  Then the point's observations, four at a time: the entry of the observation's camera
//                     by binary search (the entry cameras ascend), lane r adds A[:, r] g_r and A[:, r] (C_aa A^T)[r], group sums by shuffles, the
//                     first lane of the group finishes the block with [V~_k^-1]_ii + Q_i and writes the caller's row;
//   k_rel_con_rows    one wave per constraint row j: v_c = Y_c c_j^T for the cameras of the row's component into a device buffer (any number of
//                     cameras), then v^T C v with the lanes over the rows of C, r_j = 1 - (s_j + v^T C v), w_j and f~_j into the caller's row.
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
#include "covariance_constraint_plan.h"
#include "reliability_constraint_math.h"
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

// `list` (a problem with constraint rows): the points in no row, which are the points this kernel takes; nullptr: every point
__global__ void __launch_bounds__(COV_POINT_THREADS)
k_rel_point(const int32_t* __restrict__ list, const int64_t* __restrict__ pt_start, const int64_t* __restrict__ order, const int32_t* __restrict__ cam_sorted,
            const int32_t* __restrict__ cam_off, int32_t ncp, const double* __restrict__ tab, const double* __restrict__ points,
            const double* __restrict__ obs_uv, int loss, double f_scale, const double* __restrict__ Y, const double* __restrict__ Vinv,
            const double* __restrict__ C, double sigma0, double* out_r, double* __restrict__ out_w, double* __restrict__ out_f,
            unsigned long long* __restrict__ counts) {  // counts[0]: uncontrolled rows, counts[1]: set when an R_oo is not finite
  constexpr int WB = 3 * MAX_NC;
  const int64_t p = list ? (int64_t)list[blockIdx.x] : (int64_t)blockIdx.x;
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


// The observations of the points of the constraint components.  `Gs` ([entries][27], laid out as Yc) receives the rows of G_e.
__global__ void __launch_bounds__(COV_POINT_THREADS)
k_rel_con_point(const int32_t* __restrict__ list, const int64_t* __restrict__ pt_start, const int64_t* __restrict__ order, const int32_t* __restrict__ cam_sorted,
                const int32_t* __restrict__ cam_off, int32_t ncp, const double* __restrict__ tab, const double* __restrict__ points,
                const double* __restrict__ obs_uv, int loss, double f_scale, const int64_t* __restrict__ entry_start, const int32_t* __restrict__ entry_cam,
                const double* __restrict__ Yc, double* Gs, const double* __restrict__ Vinv, const double* __restrict__ C, double sigma0,
                double* __restrict__ out_r, double* __restrict__ out_w, double* __restrict__ out_f, unsigned long long* __restrict__ counts) {
  constexpr int WB = 3 * MAX_NC;
  const int64_t p = list[blockIdx.x];
  const int t = threadIdx.x, grp = t / REL_GROUP, r = t % REL_GROUP;
  const int64_t es = entry_start[p];
  const int n_e = (int)(entry_start[p + 1] - es);
  double Q[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int e0 = 0; e0 < n_e; e0 += REL_GROUPS) {  // (the same trip count in every lane, as in k_rel_point)
    const int e = e0 + grp;
    if (e < n_e) {
      const int32_t cam = entry_cam[es + e], off = cam_off[cam], np = cam_off[cam + 1] - off;
      if (r < np) {
        const double* crow = C + (int64_t)(off + r) * ncp;
        double g[3] = {0.0, 0.0, 0.0};
        for (int ep = 0; ep < n_e; ++ep) {
          const int32_t cam_b = entry_cam[es + ep], off_b = cam_off[cam_b], np_b = cam_off[cam_b + 1] - off_b;
          rel_row_times_y(crow + off_b, np_b, Yc + (es + ep) * WB, g);
        }
        const double yr[3] = {Yc[(es + e) * WB + 3 * r], Yc[(es + e) * WB + 3 * r + 1], Yc[(es + e) * WB + 3 * r + 2]};
        rel_con_q_terms(yr, g, Q);
#pragma unroll
        for (int q = 0; q < 3; ++q) Gs[(es + e) * WB + 3 * r + q] = g[q];
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 9; ++e) Q[e] = wave_total(Q[e]);
  __threadfence_block();
  __syncthreads();  // (the rows of G_e in Gs are read below by other lanes of this wave)
  double Vi[6];
#pragma unroll
  for (int e = 0; e < 6; ++e) Vi[e] = Vinv[p * 6 + e];
  const double X[3] = {points[3 * p], points[3 * p + 1], points[3 * p + 2]};
  const int64_t s = pt_start[p], k = pt_start[p + 1] - s;
  int bad = 0;
  for (int64_t b0 = 0; b0 < k; b0 += REL_GROUPS) {  // (whole wave in every trip: the shuffles below)
    const int64_t b = b0 + grp;
    double M[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, S[3] = {0.0, 0.0, 0.0};
    double A[2][MAX_NC], B[2][3], fs[2] = {0.0, 0.0};
    int64_t o = 0;
    bool row = false;
    if (b < k) {
      o = order[s + b];
      const int32_t cam = cam_sorted[s + b], off = cam_off[cam], np = cam_off[cam + 1] - off;
      row = r < np;
      if (row) {
        const double uv[2] = {obs_uv[2 * o], obs_uv[2 * o + 1]};
        cov_obs_jacobian(reinterpret_cast<const CamTab*>(tab)[cam], X, uv, loss, f_scale, A, B, fs);
        int lo = 0, hi = n_e - 1;  // (the camera observes the point: it is among the component's cameras)
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (entry_cam[es + mid] < cam) lo = mid + 1; else hi = mid;
        }
        const double* gp = Gs + (es + lo) * WB + 3 * r;
        const double g[3] = {gp[0], gp[1], gp[2]};
        double h[2], a[2];
        rel_row_times_a(C + (int64_t)(off + r) * ncp + off, np, A, h);
        rel_a_column(A, r, a);
        rel_con_obs_terms(a, g, h, M, S);
      }
    }
#pragma unroll
    for (int e = 0; e < 6; ++e) M[e] = group_sum(M[e]);
#pragma unroll
    for (int e = 0; e < 3; ++e) S[e] = group_sum(S[e]);
    if (row && r == 0) {
      double T[3], R[3], w[2];
      rel_camera_part(S, M, B, T);
      bad += rel_finish(B, Vi, Q, T, sigma0, fs, R, w);
      if (!isfinite(R[0] + R[1] + R[2])) counts[1] = 1;
#pragma unroll
      for (int e = 0; e < 3; ++e) out_r[3 * o + e] = R[e];
      out_w[2 * o] = w[0]; out_w[2 * o + 1] = w[1];
      out_f[2 * o] = fs[0]; out_f[2 * o + 1] = fs[1];
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, 64);
  if (t == 0 && bad) atomicAdd(&counts[0], (unsigned long long)bad);
}

// The constraint rows: one wave per kept row j.  `vbuf` ([n_rows][vstride], vstride = 9 x the cameras of the widest component) receives v.
// counts[2]: uncontrolled constraint rows.  out_*: the CALLER's rows (row_src[j]).
__global__ void __launch_bounds__(COV_POINT_THREADS)
k_rel_con_rows(const int32_t* __restrict__ row_pt, const double* __restrict__ row_u, const double* __restrict__ row_coef, const double* __restrict__ row_dist,
               const double* __restrict__ row_weight, const int64_t* __restrict__ row_src, const int32_t* __restrict__ row_comp,
               const double* __restrict__ row_s, const int64_t* __restrict__ comp_cam, const int32_t* __restrict__ cams, const int32_t* __restrict__ cam_off,
               int32_t ncp, const int64_t* __restrict__ entry_start, const double* __restrict__ Yc, const double* __restrict__ C,
               const double* __restrict__ points, int loss, double f_scale, double sigma0, double* vbuf, int64_t vstride, double* __restrict__ out_r,
               double* __restrict__ out_w, double* __restrict__ out_f, unsigned long long* __restrict__ counts) {
  const int64_t j = blockIdx.x;
  const int lane = threadIdx.x;
  int32_t pt[8];
  int64_t e0[8];
  double coef[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) { pt[s] = row_pt[j * 8 + s]; coef[s] = row_coef[j * 8 + s]; e0[s] = entry_start[pt[s]]; }
  const double u[3] = {row_u[j * 3], row_u[j * 3 + 1], row_u[j * 3 + 2]};
  const int32_t k = row_comp[j];
  const int64_t q0 = comp_cam[k];
  const int nc = (int)(comp_cam[k + 1] - q0);
  double* v = vbuf + j * vstride;
  for (int it = lane; it < MAX_NC * nc; it += COV_POINT_THREADS) v[it] = rel_con_v_entry(Yc, e0, it / MAX_NC, it % MAX_NC, coef, u);
  __threadfence_block();
  __syncthreads();  // (v is read below by other lanes of this wave)
  double acc = 0.0;
  for (int it = lane; it < MAX_NC * nc; it += COV_POINT_THREADS) {
    const int c = it / MAX_NC, r = it % MAX_NC;
    const int32_t cam = cams[q0 + c], off = cam_off[cam], np = cam_off[cam + 1] - off;
    if (r >= np) continue;
    const double* crow = C + (int64_t)(off + r) * ncp;
    double tsum = 0.0;
    for (int c2 = 0; c2 < nc; ++c2) {
      const int32_t cam_b = cams[q0 + c2], off_b = cam_off[cam_b], np_b = cam_off[cam_b + 1] - off_b;
      tsum += rel_con_row_dot(crow + off_b, np_b, v + MAX_NC * c2);
    }
    acc += v[it] * tsum;
  }
  acc = wave_total(acc);
  if (lane != 0) return;
  double rr, w;
  const double f = rel_con_residual(points, pt, row_dist[j], row_weight[j], loss, f_scale);
  const int bad = rel_con_finish(row_s[j], acc, f, sigma0, &rr, &w);
  if (!isfinite(rr)) counts[1] = 1;
  const int64_t dst = row_src[j];
  out_r[dst] = rr; out_w[dst] = w; out_f[dst] = f;
  if (bad) atomicAdd(&counts[2], 1ull);
}

// Everything behind C = St^-1 of both entry points.  pipe.con == nullptr: k_rel_point on every point and nothing else.
int rel_outputs(const cba_cov_desc* d, const CovPipeline& pipe, const char* what, const cba_rel_out* out, int64_t n_con, const cba_rel_con_out* con_out) {
  for (double v : *pipe.C_host)
    if (!std::isfinite(v)) return err(CBA_ERR_NUMERIC, cov_msg_not_finite(what, "camera"));
  const int64_t n_obs = pipe.n_obs;
  const CovConPlan* con = pipe.con;
  const double sigma0 = std::sqrt(pipe.sigma0_sq);
  Buffers buf;
  double* dr = buf.make<double>(n_obs, 3);
  double* dw = buf.make<double>(n_obs, 2);
  double* df = buf.make<double>(n_obs, 2);
  unsigned long long* dcounts = buf.make<unsigned long long>(3);
  double *dcr = nullptr, *dcw = nullptr, *dcf = nullptr, *dGs = nullptr, *dv = nullptr;
  const int32_t* drow_comp = nullptr;
  const int64_t vstride = con ? MAX_NC * cov_con_max_cams(*con) : 0;
  if (con) {
    const std::vector<double> nans((size_t)n_con, std::nan(""));  // (a row of weight 0 stays NaN)
    std::vector<int32_t> row_comp((size_t)con->n_rows);
    for (int32_t k = 0; k < con->n_comp; ++k)
      for (int64_t r = con->comp_row[(size_t)k]; r < con->comp_row[(size_t)k + 1]; ++r) row_comp[(size_t)r] = k;
    dcr = buf.in(nans.data(), n_con);
    dcw = buf.in(nans.data(), n_con);
    dcf = buf.in(nans.data(), n_con);
    drow_comp = buf.in(row_comp.data(), con->n_rows);
    dGs = buf.make<double>(con->n_entries(), 3 * MAX_NC);
    dv = buf.make<double>(con->n_rows, vstride);
  }
  if (buf.status()) return buf.result(what);
  buf.check(hipMemsetAsync(dcounts, 0, 3 * sizeof(unsigned long long), 0));
  const int64_t n_list = con ? pipe.n_free : pipe.n_points;
  if (n_list > 0)
    hipLaunchKernelGGL(k_rel_point, dim3((unsigned)n_list), dim3(COV_POINT_THREADS), 0, 0, pipe.free_list, pipe.pt_start, pipe.order, pipe.cam_sorted, pipe.cam_off,
                       pipe.ncp, pipe.tab, pipe.points, pipe.obs_uv, (int)d->loss, d->f_scale, pipe.Y, pipe.Vinv, pipe.C, sigma0, dr, dw, df, dcounts);
  if (con) {
    hipLaunchKernelGGL(k_rel_con_point, dim3((unsigned)pipe.n_con_pts), dim3(COV_POINT_THREADS), 0, 0, pipe.con_list, pipe.pt_start, pipe.order, pipe.cam_sorted,
                       pipe.cam_off, pipe.ncp, pipe.tab, pipe.points, pipe.obs_uv, (int)d->loss, d->f_scale, pipe.entry_start, pipe.entry_cam, pipe.Yc, dGs, pipe.Vinv,
                       pipe.C, sigma0, dr, dw, df, dcounts);
    hipLaunchKernelGGL(k_rel_con_rows, dim3((unsigned)pipe.n_rows), dim3(COV_POINT_THREADS), 0, 0, pipe.row_pt, pipe.row_u, pipe.row_coef, pipe.row_dist,
                       pipe.row_weight, pipe.row_src, drow_comp, pipe.row_s, pipe.comp_cam, pipe.cams, pipe.cam_off, pipe.ncp, pipe.entry_start, pipe.Yc, pipe.C,
                       pipe.points, (int)d->loss, d->f_scale, sigma0, dv, vstride, dcr, dcw, dcf, dcounts);
  }
  buf.check(hipGetLastError());
  unsigned long long counts[3] = {0, 0, 0};
  buf.out(counts, (const unsigned long long*)dcounts, 3);
  if (buf.status()) return buf.result(what);
  if (counts[1]) return err(CBA_ERR_NUMERIC, std::string(what) + ": a redundancy number is not finite");
  // outputs, only now and straight into the caller's arrays (seven doubles per observation: no second copy on the host): every check has passed
  if (out) {
    buf.out(out->redundancy, (const double*)dr, n_obs, 3);
    buf.out(out->w, (const double*)dw, n_obs, 2);
    buf.out(out->residual, (const double*)df, n_obs, 2);
  }
  if (con && con_out) {
    buf.out(con_out->redundancy, (const double*)dcr, n_con);
    buf.out(con_out->w, (const double*)dcw, n_con);
    buf.out(con_out->residual, (const double*)dcf, n_con);
  }
  if (buf.status()) return buf.result(what);
  if (out) {
    if (out->sigma0_sq) *out->sigma0_sq = pipe.sigma0_sq;
    if (out->dof) *out->dof = pipe.plan->dof;
    if (out->cost) *out->cost = pipe.cost;
    if (out->n_uncontrolled) *out->n_uncontrolled = (int64_t)counts[0];
  }
  if (con_out) {
    if (!con)  // no row of positive weight: every row of the caller is NaN
      for (int64_t r = 0; r < n_con; ++r) {
        if (con_out->redundancy) con_out->redundancy[r] = std::nan("");
        if (con_out->w) con_out->w[r] = std::nan("");
        if (con_out->residual) con_out->residual[r] = std::nan("");
      }
    if (con_out->n_uncontrolled) *con_out->n_uncontrolled = (int64_t)counts[2];
  }
  return CBA_OK;
}

}  // namespace

extern "C" int cba_observation_reliability(const cba_cov_desc* d, int32_t device, cba_rel_out* out) {
  const char* what = "cba_observation_reliability";
  if (!d || !out) return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  return cov_pipeline(d, device, what, true, [&](const CovPipeline& pipe) -> int { return rel_outputs(d, pipe, what, out, 0, nullptr); });
}

// include/caliscope/reliability_constrained.h.  Without a row of positive weight: the launches of cba_observation_reliability.
extern "C" int cba_observation_reliability_constrained(const cba_cov_desc* d, const cba_cov_constraints* constraints, int32_t device, cba_rel_out* out,
                                                       cba_rel_con_out* con_out) {
  const char* what = "cba_observation_reliability_constrained";
  if (!d) return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  return cov_pipeline_constrained(d, constraints, device, what, true, [&](const CovPipeline& pipe) -> int {
    const int64_t n_con = constraints && constraints->n_con > 0 ? constraints->n_con : 0;
    return rel_outputs(d, pipe, what, out, n_con, con_out);
  });
}
