// The host planning of a handle's set-up (caliscope_amd/csrc/host_plan.h) behind a flat C interface, compiled by g++: tests/test_setup_plan.py checks
// what it returns against numpy restatements.  Output arrays are sized by the caller for the worst case named at each function.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/caliscope_ba.h"
#include "../../caliscope_amd/csrc/host_plan.h"

static std::string g_error;
static int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_error = buf;
  return code;
}
template <typename V, typename T>
static void copy_out(const V& v, T* out) { std::copy(v.begin(), v.end(), out); }

extern "C" {

const char* sp_last_error() { return g_error.c_str(); }

// host plan -> sorted observations -> point tables, as cba_create chains them.  sorted_cam, sorted_pt [N]; pt_start [P + 1]; chunk_start [N + 2];
// chunk_pts [2 (N + 1)]; heavy, heavy_frag [P]; scalars: n_chunks, max_obs_per_point, n_heavy, has_fragments
int sp_point_tables(int P, long N, const int* obs_pt, const int* obs_cam, int C, int chunk, int heavy_obs, int* sorted_cam, int* sorted_pt, int* pt_start,
                    int* chunk_start, int* chunk_pts, int* heavy, int* heavy_frag, long* scalars) {
  std::vector<int64_t> order(N), pstart((size_t)P + 1), cstart((size_t)N + 2);
  const int64_t nch = host_plan_impl(fail, P, N, obs_pt, obs_cam, C, chunk, order.data(), pstart.data(), cstart.data());
  if (nch < 0) return (int)nch;
  SortedObs obs;
  gather_sorted(N, obs_cam, obs_pt, order.data(), obs);
  PointTables t;
  const int rc = point_tables(fail, P, pstart.data(), nch, cstart.data(), obs.pt.data(), chunk, heavy_obs, t);
  if (rc) return rc;
  copy_out(obs.cam, sorted_cam); copy_out(obs.pt, sorted_pt);
  copy_out(t.pt_start, pt_start); copy_out(t.chunk_start, chunk_start); copy_out(t.chunk_pts, chunk_pts);
  copy_out(t.heavy, heavy); copy_out(t.heavy_frag, heavy_frag);
  scalars[0] = nch; scalars[1] = t.max_obs_per_point; scalars[2] = (long)t.heavy.size(); scalars[3] = t.has_fragments;
  return 0;
}

// perm [n_chunks][chunk], cst [n_chunks][C + 1]
int sp_det_plan(int C, int nct, long n_chunks, const int* chunk_start, const int* sorted_cam, int chunk, int det_round, int block, unsigned char* perm,
                unsigned short* cst, int* det_m) {
  HostDetPlan plan;
  const int rc = det_plan(fail, C, nct, n_chunks, chunk_start, sorted_cam, chunk, det_round, block, plan);
  *det_m = plan.det_m;
  if (rc) return rc;
  copy_out(plan.perm, perm); copy_out(plan.cst, cst);
  return 0;
}

// sc_obs [n_chunks + 1]; sc_p0, sc_np [n_chunks]; cperm [N]; scalars: n_sc, pmax, rounds, greedy
void sp_cs_plan(int enabled, int deterministic, int C, long N, long n_chunks, const int* chunk_start, const int* chunk_pts, const int* sorted_cam,
                long workgroups, long cap, int chunk, int max_pts, int* sc_obs, int* sc_p0, int* sc_np, int* cperm, long* scalars) {
  HostCsPlan plan;
  cs_plan(enabled != 0, deterministic != 0, C, N, n_chunks, chunk_start, chunk_pts, sorted_cam, workgroups, cap, chunk, max_pts, plan);
  scalars[0] = plan.n_sc; scalars[1] = plan.pmax; scalars[2] = plan.rounds; scalars[3] = plan.greedy;
  if (!plan.n_sc) return;
  copy_out(plan.sc_obs, sc_obs); copy_out(plan.sc_p0, sc_p0); copy_out(plan.sc_np, sc_np); copy_out(plan.cperm, cperm);
}

// pt, lp [n_con][8]; order, dist, wgt [n_con]; comp_con, comp_pt, comp_m [n_con + 1]; comp_pts, orphan [8 n_con]; pt_start [P + 1];
// scalars: n_comp, max_m, max_pts, big, points in comp_pts, orphans
int sp_constraint_plan(int P, int ncp, int n_con, const int* groups_a, const int* groups_b, const double* distances, const double* weights, int lds_points,
                       const int* pt_start, int* pt, int* lp, int* order, int* comp_con, int* comp_pt, int* comp_pts, long* comp_m, double* dist, double* wgt,
                       int* orphan, long* scalars) {
  HostConPlan plan;
  const int rc = constraint_plan(fail, P, ncp, n_con, groups_a, groups_b, distances, weights, lds_points, plan);
  if (rc) return rc;
  const std::vector<int> orph = constraint_orphans(plan.comp_pts, pt_start);
  copy_out(plan.pt, pt); copy_out(plan.lp, lp); copy_out(plan.order, order); copy_out(plan.comp_con, comp_con); copy_out(plan.comp_pt, comp_pt);
  copy_out(plan.comp_pts, comp_pts); copy_out(plan.comp_m, comp_m); copy_out(plan.dist, dist); copy_out(plan.wgt, wgt); copy_out(orph, orphan);
  scalars[0] = plan.n_comp; scalars[1] = plan.max_m; scalars[2] = plan.max_pts; scalars[3] = plan.big; scalars[4] = (long)plan.comp_pts.size();
  scalars[5] = (long)orph.size();
  return 0;
}

// the point table of a cba_triangulate_desc: 0, or CBA_ERR_INVALID with sp_last_error() naming the entry
int sp_triangulate_starts_ok(long n_points, const long* pt_start) { return triangulate_starts_ok(fail, n_points, (const int64_t*)pt_start); }

// out: cam, flags, bcam, total, scalars, sequence slot (doubles)
void sp_mail_layout(int ncp, long* out) {
  const MailLayout m(ncp);
  out[0] = (long)m.cam; out[1] = (long)m.flags; out[2] = (long)m.bcam; out[3] = (long)m.total; out[4] = (long)MailLayout::kScalars; out[5] = (long)MailLayout::kSeqSlot;
}

}  // extern "C"
