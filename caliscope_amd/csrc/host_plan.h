// Host-side planning of a handle's set-up, plain C++ (no HIP): everything cba_create and cba_set_constraints decide between their device calls.
//   validate_problem_desc / camera_layout   the checks of a problem description, the layout of the camera block
//   host_plan_impl                          include/caliscope_ba.h: cba_host_plan — stable sort by (world point, camera), first observation of every
//                                           point, chunk table
//   gather_sorted / point_tables            the observations in that order; per-point and per-chunk tables, heavy points
//   det_plan                                fixed-order sums (cba_options.deterministic): per chunk a stable order by camera
//   cs_plan                                 camera-sorted super-chunks of k_build_cs
//   constraint_plan / constraint_orphans    rows of cba_set_constraints grouped by connected component
//   MailLayout                              the mapped host mailbox
//   triangulate_starts_ok                   the point table of a cba_triangulate_desc
// Shared by the device library (cba_lib.hip), the CPU test build of the C ABI (tests/native/cpu_library.cpp) and the CPU harness of the set-up
// (tests/native/setup_harness.cpp, tests/test_setup_plan.py).  The kernel constants a function depends on (CHUNK, HEAVY_OBS, ...) are its arguments;
// `fail(code, fmt, ...)` is the including file's error reporter; include/caliscope_ba.h comes before this file.
#pragma once
#include <algorithm>
#include <cstdint>
#include <thread>
#include <vector>

#include "schur_plan.h"  // usable_cpus, HostVec

// ---- problem description -------------------------------------------------------------------------------------------------------------
template <typename Fail>
static int validate_problem_desc(Fail fail, const cba_problem_desc* d) {
  if (d->n_cams <= 0 || d->n_points <= 0 || d->n_obs <= 0) return fail(CBA_ERR_INVALID, "cba_create: empty problem (cams=%d points=%d obs=%lld)", d->n_cams, d->n_points, (long long)d->n_obs);
  if (d->n_obs >= (1LL << 31)) return fail(CBA_ERR_UNSUPPORTED, "cba_create: more than 2^31 observations");
  if (!d->cam_n_params || !d->cam_model || !d->cam_const || !d->obs_cam || !d->obs_pt || !d->obs_uv) return fail(CBA_ERR_INVALID, "cba_create: null array");
  if (d->loss < CBA_LOSS_LINEAR || d->loss > CBA_LOSS_ARCTAN) return fail(CBA_ERR_INVALID, "cba_create: unknown loss %d", d->loss);
  if (d->loss != CBA_LOSS_LINEAR && !(d->f_scale > 0.0)) return fail(CBA_ERR_INVALID, "cba_create: f_scale must be positive");
  return CBA_OK;
}

// the camera block of the parameter vector: camera c owns np[c] parameters from off[c] on; nct is 9 as soon as one camera has free intrinsics
struct CameraLayout {
  std::vector<int> np, model, off;
  int ncp = 0, nct = 6, ncp_pad = 0;
  std::vector<int> param_cam, param_loc;  // [ncp_pad] camera and index inside the camera of every camera parameter
};
template <typename Fail>
static int camera_layout(Fail fail, const cba_problem_desc* d, CameraLayout& out) {
  const int C = d->n_cams;
  out = CameraLayout{};
  out.np.resize(C); out.model.resize(C); out.off.resize(C);
  for (int c = 0; c < C; ++c) {
    const int np = out.np[c] = d->cam_n_params[c], model = out.model[c] = d->cam_model[c];
    if (np != 6 && np != 9) return fail(CBA_ERR_INVALID, "camera %d: n_params must be 6 or 9, got %d", c, np);
    if (model != CBA_MODEL_PINHOLE_BC5 && model != CBA_MODEL_FISHEYE4) return fail(CBA_ERR_INVALID, "camera %d: unknown model %d", c, model);
    if (model == CBA_MODEL_FISHEYE4 && np != 6) return fail(CBA_ERR_INVALID, "camera %d: fisheye cameras are always locked (6 params)", c);
    if (!(d->cam_const[c * 12] > 0.0)) return fail(CBA_ERR_INVALID, "camera %d: fx_initial must be positive", c);
    out.off[c] = out.ncp; out.ncp += np;
    if (np == 9) out.nct = 9;
  }
  out.ncp_pad = (out.ncp + 31) / 32 * 32;
  out.param_cam.assign(out.ncp_pad, 0); out.param_loc.assign(out.ncp_pad, 0);
  for (int c = 0; c < C; ++c)
    for (int r = 0; r < out.np[c]; ++r) { out.param_cam[out.off[c] + r] = c; out.param_loc[out.off[c] + r] = r; }
  return CBA_OK;
}

// ---- observation order ---------------------------------------------------------------------------------------------------------------
template <typename Fail>
static int64_t host_plan_impl(Fail fail, int32_t n_points, int64_t n_obs, const int32_t* obs_pt, const int32_t* obs_cam, int32_t n_cams,
                      int32_t chunk_cap, int64_t* order_out, int64_t* pt_start_out, int64_t* chunk_start_out) {
  if (n_points < 0 || n_obs < 0 || chunk_cap <= 0 || (n_obs > 0 && !obs_pt)) return fail(CBA_ERR_INVALID, "cba_host_plan: bad arguments");
  // Already in (point, camera) order?  One pass decides (the arrays CaptureVolume hands over after a first optimize() are, and so is anything
  // produced point by point); the two scattering passes below cost ~9 ns per observation.  The pass and, for sorted input, the point table and
  // the identity order are split over a few threads (1M observations: 4 ms on one).
  const bool with_cam = obs_cam && n_cams > 0;
  const int nth = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(16, std::thread::hardware_concurrency()), n_obs / 131072));
  auto slices = [&](auto&& body) {  // body(thread, lo, hi)
    std::vector<std::thread> pool;
    for (int t = 1; t < nth; ++t) pool.emplace_back(body, t, n_obs * t / nth, n_obs * (t + 1) / nth);
    body(0, (int64_t)0, n_obs / nth);
    for (auto& th : pool) th.join();
  };
  std::vector<char> slice_ok((size_t)nth, 1), slice_sorted((size_t)nth, 1);
  slices([&](int t, int64_t lo, int64_t hi) {
    bool ok = true, srt = true;
    for (int64_t i = lo; i < hi; ++i) {
      const int32_t p = obs_pt[i];
      if (p < 0 || p >= n_points || (with_cam && (obs_cam[i] < 0 || obs_cam[i] >= n_cams))) { ok = false; break; }
      if (i > 0 && (p < obs_pt[i - 1] || (p == obs_pt[i - 1] && with_cam && obs_cam[i] < obs_cam[i - 1]))) srt = false;
    }
    slice_ok[(size_t)t] = ok; slice_sorted[(size_t)t] = srt;
  });
  bool sorted = true;
  for (int t = 0; t < nth; ++t) {
    if (!slice_ok[(size_t)t])  // report the first offender, in input order
      for (int64_t i = 0; i < n_obs; ++i) {
        const int32_t p = obs_pt[i];
        if (p < 0 || p >= n_points) return fail(CBA_ERR_INVALID, "observation %lld: world-point index %d out of range", (long long)i, p);
        if (with_cam && (obs_cam[i] < 0 || obs_cam[i] >= n_cams)) return fail(CBA_ERR_INVALID, "observation %lld: camera index %d out of range", (long long)i, obs_cam[i]);
      }
    sorted = sorted && slice_sorted[(size_t)t];
  }
  if (sorted) {
    // first observation of every point straight from the runs of equal indices: thread t fills the entries of the points that BEGIN in its slice
    // (and of the unobserved points in front of them); the identity order on the way
    slices([&](int, int64_t lo, int64_t hi) {
      for (int64_t i = lo; i < hi; ++i) {
        order_out[i] = i;
        const int32_t p = obs_pt[i], prev = i > 0 ? obs_pt[i - 1] : -1;
        for (int32_t q = prev + 1; q <= p; ++q) pt_start_out[q] = i;
      }
    });
    for (int32_t q = (n_obs > 0 ? obs_pt[n_obs - 1] : -1) + 1; q <= n_points; ++q) pt_start_out[q] = n_obs;
  } else {
    // optional first key: camera (stable counting sort), so that the final order is (point, camera, input order)
    std::vector<int64_t> by_cam;
    if (with_cam) {
      std::vector<int64_t> cc((size_t)n_cams + 1, 0);
      for (int64_t i = 0; i < n_obs; ++i) cc[obs_cam[i] + 1]++;
      for (int32_t c = 0; c < n_cams; ++c) cc[c + 1] += cc[c];
      by_cam.resize((size_t)n_obs);
      for (int64_t i = 0; i < n_obs; ++i) by_cam[cc[obs_cam[i]]++] = i;
    }
    std::vector<int64_t> count((size_t)n_points + 1, 0);
    for (int64_t i = 0; i < n_obs; ++i) count[obs_pt[i] + 1]++;
    for (int32_t p = 0; p < n_points; ++p) count[p + 1] += count[p];
    for (int32_t p = 0; p <= n_points; ++p) pt_start_out[p] = count[p];
    std::vector<int64_t> cursor(count.begin(), count.end() - 1);
    for (int64_t q = 0; q < n_obs; ++q) {  // stable counting sort by point
      const int64_t i = by_cam.empty() ? q : by_cam[q];
      order_out[cursor[obs_pt[i]]++] = i;
    }
  }
  int64_t n_chunks = 0;
  int64_t start = 0;
  chunk_start_out[0] = 0;
  for (int32_t p = 0; p < n_points; ++p) {
    const int64_t begin = pt_start_out[p], end = pt_start_out[p + 1];
    if (end - begin > chunk_cap) {
      // a point that does not fit one chunk gets chunks of its own ("fragments" of at most chunk_cap observations)
      if (begin > start) chunk_start_out[++n_chunks] = begin;
      for (int64_t o = begin + chunk_cap; o < end; o += chunk_cap) chunk_start_out[++n_chunks] = o;
      chunk_start_out[++n_chunks] = end;
      start = end;
    } else if (end - start > chunk_cap) {  // close the chunk before this point
      chunk_start_out[++n_chunks] = begin;
      start = begin;
    }
  }
  if (n_obs > start) chunk_start_out[++n_chunks] = n_obs;
  return n_chunks;
}

// body(lo, hi) over the slices of [0, n): on up to 16 host threads, one per `grain` items (the calling thread takes the first slice)
template <typename Body>
static void host_slices(int64_t n, int64_t grain, Body body) {
  const int nth = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(16, cba::usable_cpus()), n / grain));
  std::vector<std::thread> pool;
  for (int t = 1; t < nth; ++t) pool.emplace_back(body, n * t / nth, n * (t + 1) / nth);
  body((int64_t)0, n / nth);
  for (auto& th : pool) th.join();
}

// the caller's observations in the order of host_plan_impl (the coordinates are gathered on the device: k_gather_uv)
struct SortedObs { cba::HostVec<int> cam, pt, order; };
static void gather_sorted(int64_t n_obs, const int32_t* obs_cam, const int32_t* obs_pt, const int64_t* order, SortedObs& out) {
  out.cam.resize(n_obs); out.pt.resize(n_obs); out.order.resize(n_obs);
  host_slices(n_obs, 65536, [&](int64_t lo, int64_t hi) {  // (1M observations: 6 ms on one thread)
    for (int64_t i = lo; i < hi; ++i) {
      const int64_t o = order[i];
      out.cam[i] = obs_cam[o]; out.pt[i] = obs_pt[o]; out.order[i] = (int)o;
    }
  });
}

// ---- point and chunk tables ----------------------------------------------------------------------------------------------------------
struct PointTables {
  std::vector<int> pt_start, chunk_start;  // host_plan_impl's tables as the kernels read them
  std::vector<int> chunk_pts;              // [n_chunks][2] first point and number of points (observed or not) in a chunk's range; -1: a fragment
  int max_obs_per_point = 0;
  std::vector<int> heavy, heavy_frag;      // points with more than heavy_obs observations; 1: with more than a chunk holds
  bool has_fragments = false;              // some chunk is a fragment of a point with more than `chunk` observations
};
template <typename Fail>
static int point_tables(Fail fail, int P, const int64_t* pstart, int64_t n_chunks, const int64_t* cstart, const int* sorted_pt, int chunk, int heavy_obs,
                        PointTables& out) {
  out = PointTables{};
  std::vector<int>&hps = out.pt_start, &hcs = out.chunk_start, &hcp = out.chunk_pts;
  hps.resize((size_t)P + 1); hcs.resize((size_t)n_chunks + 1);
  int maxk = 0;
  for (int q = 0; q <= P; ++q) { hps[q] = (int)pstart[q]; if (q) maxk = std::max<int>(maxk, (int)(pstart[q] - pstart[q - 1])); }
  for (int64_t q = 0; q <= n_chunks; ++q) hcs[q] = (int)cstart[q];
  out.max_obs_per_point = maxk;
  // heavy points (static markers observed again in every frame): per-camera Schur sums instead of observation pairs
  for (int q = 0; q < P && maxk > heavy_obs; ++q)
    if (hps[q + 1] - hps[q] > heavy_obs) { out.heavy.push_back(q); out.heavy_frag.push_back(hps[q + 1] - hps[q] > chunk ? 1 : 0); }
  const long heavy_max = std::max<long>(64, P / 64);
  if ((long)out.heavy.size() > heavy_max) {
    // not a few static points but a dense problem (every point seen by > heavy_obs cameras): the per-point workgroup of
    // k_heavy_schur is the wrong tool; keep the pair plan (a point with more observations in one tile than a chunk holds is refused by the Schur plan)
    if (maxk > chunk) return fail(CBA_ERR_UNSUPPORTED, "%zu world points have more than %d observations (one has %d); at most %ld such points are supported",
                                  out.heavy.size(), heavy_obs, maxk, heavy_max);
    out.heavy.clear(); out.heavy_frag.clear();
  }
  hcp.assign((size_t)std::max<int64_t>(n_chunks, 1) * 2, 0);
  for (int64_t q = 0; q < n_chunks; ++q) {
    const int first = sorted_pt[hcs[q]];
    hcp[2 * q] = first;
    hcp[2 * q + 1] = sorted_pt[hcs[q + 1] - 1] - first + 1;
    if (hps[first + 1] - hps[first] > chunk) { hcp[2 * q + 1] = -1; out.has_fragments = true; }
  }
  return CBA_OK;
}

// ---- fixed-order sums ----------------------------------------------------------------------------------------------------------------
// (k_build / k_tprep, det_round): per chunk the observation order by camera and the camera offsets
struct HostDetPlan {
  int det_m = 0;                     // tasks per thread: 3, 5, 8 or 16
  std::vector<unsigned char> perm;   // [n_chunks][chunk] chunk-local observation indices, sorted by camera
  std::vector<unsigned short> cst;   // [n_chunks][C + 1] offsets into perm
};
template <typename Fail>
static int det_plan(Fail fail, int C, int nct, int64_t n_chunks, const int* chunk_start, const int* sorted_cam, int chunk, int det_round, int block,
                    HostDetPlan& out) {
  const int need = (C * det_round + block - 1) / block;
  // tasks per thread of the fixed-order sums: 3, 5, 8 (<= 227 cameras) and, six-parameter cameras only, 16 (<= 455 by the task count; the LDS copy of
  // the camera table next to k_tprep's staging and parking areas admits 385: configure_kernels reports the bytes beyond that).  Nine-parameter cameras stop at 227: six
  // rounds of 16 running sums are 96 doubles per thread.
  out.det_m = need <= 3 ? 3 : need <= 5 ? 5 : need <= 8 ? 8 : (nct == 6 && need <= 16) ? 16 : -1;
  if (out.det_m < 0) return fail(CBA_ERR_UNSUPPORTED, "deterministic sums support up to %d %s-parameter cameras, the problem has %d",
                                 (nct == 6 ? 16 : 8) * block / det_round, nct == 6 ? "six" : "nine", C);
  out.perm.assign((size_t)std::max<int64_t>(n_chunks, 1) * chunk, 0);
  out.cst.assign((size_t)std::max<int64_t>(n_chunks, 1) * (C + 1), 0);
  for (int64_t c = 0; c < n_chunks; ++c) {
    const int o0 = chunk_start[c], n = chunk_start[c + 1] - o0;
    unsigned short* cs = &out.cst[(size_t)c * (C + 1)];
    for (int k = 0; k < n; ++k) cs[sorted_cam[o0 + k] + 1]++;
    for (int q = 0; q < C; ++q) cs[q + 1] += cs[q];
    std::vector<unsigned short> cur(cs, cs + C);
    for (int k = 0; k < n; ++k) out.perm[(size_t)c * chunk + cur[sorted_cam[o0 + k]]++] = (unsigned char)k;  // stable: observation order inside a camera
  }
  return CBA_OK;
}

// ---- camera-sorted super-chunks ------------------------------------------------------------------------------------------------------
// k_build_cs walks SUPER-CHUNKS: consecutive chunks of at most cap + chunk observations and max_pts points, their observations a second time in
// (super-chunk, camera, point) order.  Not for the fixed-order sums (their own per-chunk order) nor with fragments of points larger than a chunk
// (those add to V / g by global atomics in k_build).
struct HostCsPlan {
  int n_sc = 0;                          // 0: no plan (k_build)
  std::vector<int> sc_obs, sc_p0, sc_np; // [n_sc + 1] first observation, [n_sc] first point and points of every super-chunk
  int pmax = 0;                          // the largest sc_np, padded to 32
  int64_t rounds = 0;                    // super-chunks per workgroup the cut was made for
  bool greedy = false;                   // no cut fitted the caps in eight rounds: filled greedily
  cba::HostVec<int> cperm;               // position in (super-chunk, camera, point) order -> sorted observation (the copy is made on the device: k_cs_fill)
};
namespace cs_detail {
struct Cut {
  const int *hcs, *hcp;
  int64_t n_chunks, cap, chunk, max_pts;
  HostCsPlan& out;
  int raw_pmax = 0;
  void reset() { out.sc_obs.assign(1, 0); out.sc_p0.clear(); out.sc_np.clear(); raw_pmax = 0; }
  int points(int64_t q, int64_t e) const { return hcp[2 * (e - 1)] + hcp[2 * (e - 1) + 1] - hcp[2 * q]; }  // of chunks [q, e)
  void push(int64_t q, int64_t e) {
    out.sc_obs.push_back(hcs[e]); out.sc_p0.push_back(hcp[2 * q]); out.sc_np.push_back(points(q, e));
    raw_pmax = std::max(raw_pmax, out.sc_np.back());
  }
  // exactly min(n_slots, n_chunks) super-chunks, cut k at the chunk boundary nearest to k N / n; false: a cut exceeds the caps
  bool nearest(int64_t N, int64_t n_slots) {
    const int64_t n_target = std::min<int64_t>(std::max<int64_t>(1, n_slots), n_chunks);
    reset();
    int64_t q = 0;
    for (int64_t k = 0; k < n_target && q < n_chunks; ++k) {
      const int64_t goal = (N * (k + 1) + n_target - 1) / n_target;  // observations behind super-chunk k
      int64_t e = q + 1;
      while (e < n_chunks && (k + 1 == n_target || hcs[e + 1] <= goal || (hcs[e] < goal && goal - hcs[e] > hcs[e + 1] - goal))) ++e;  // nearest boundary
      if (k + 1 == n_target) e = n_chunks;
      if (hcs[e] - hcs[q] > cap + chunk || points(q, e) > max_pts) return false;
      push(q, e);
      q = e;
    }
    return q == n_chunks;
  }
  // whole chunks up to N / n_slots observations (at least one chunk) and max_pts points: always fits
  void fill(int64_t N, int64_t n_slots) {
    const int64_t s_target = std::max<int64_t>(chunk, (N + n_slots - 1) / n_slots);
    reset();
    for (int64_t q = 0; q < n_chunks;) {
      int64_t e = q + 1;
      while (e < n_chunks && hcs[e + 1] - hcs[q] <= s_target && hcp[2 * e] + hcp[2 * e + 1] - hcp[2 * q] <= max_pts) ++e;
      push(q, e);
      q = e;
    }
  }
};
}  // namespace cs_detail

// `workgroups`: the persistent workgroups of the launch; `cap`: observations per super-chunk to aim for (a cut may exceed it by one chunk)
static void cs_plan(bool enabled, bool deterministic, int C, int64_t N, int64_t n_chunks, const int* chunk_start, const int* chunk_pts, const int* sorted_cam,
                    int64_t workgroups, int64_t cap, int chunk, int max_pts, HostCsPlan& out) {
  out = HostCsPlan{};
  if (!enabled || deterministic || n_chunks <= 0) return;
  for (int64_t q = 0; q < n_chunks; ++q)
    if (chunk_pts[2 * q + 1] < 0 || chunk_pts[2 * q + 1] > max_pts) return;
  // Size: every workgroup of the launch should get the same number of super-chunks — with 1.3 per workgroup a quarter of the pass is a tail.  The
  // super-chunks are cut at the chunk boundaries nearest to k N / (rounds * workgroups), so that there are EXACTLY rounds * workgroups of them (fewer
  // on a small problem) and workgroup w, which takes super-chunks w, w + grid, ..., gets `rounds` of about the same size.  Filled greedily up to
  // N / (rounds * workgroups) observations, whole chunks leave each a little short of that: cfg4 ended with 1143 super-chunks of 1750 observations
  // for 1024 slots, and 119 of the 512 workgroups walked three of them while the others walked two (device stamps: workgroup lifetimes 42 / 53 / 63 us
  // min / mean / max; cfg5 236 / 273 / 337).  A cut that would exceed the caps (observations, points of the LDS stage) asks for one more round;
  // irregular point sizes end with the greedy fill.
  const int64_t wgs = std::max<int64_t>(1, workgroups);
  cs_detail::Cut cut{chunk_start, chunk_pts, n_chunks, cap, chunk, max_pts, out};
  out.rounds = std::max<int64_t>(1, (N + wgs * cap - 1) / (wgs * cap));
  bool fits = cut.nearest(N, wgs * out.rounds);
  for (int attempt = 1; attempt < 8 && !fits; ++attempt) fits = cut.nearest(N, wgs * ++out.rounds);
  if (!fits) { cut.fill(N, wgs * out.rounds); out.greedy = true; }
  out.n_sc = (int)out.sc_p0.size();
  out.pmax = (cut.raw_pmax + 31) / 32 * 32;
  out.cperm.resize(N);
  host_slices(out.n_sc, 64, [&](int64_t s0, int64_t s1) {
    std::vector<int> start((size_t)C + 1);
    for (int64_t sidx = s0; sidx < s1; ++sidx) {
      const int o0 = out.sc_obs[sidx], o1 = out.sc_obs[sidx + 1];
      std::fill(start.begin(), start.end(), 0);
      for (int i = o0; i < o1; ++i) start[(size_t)sorted_cam[i] + 1]++;
      for (int c = 0; c < C; ++c) start[(size_t)c + 1] += start[c];
      for (int i = o0; i < o1; ++i) out.cperm[o0 + start[sorted_cam[i]]++] = i;  // stable: point order inside a camera
    }
  });
}

// ---- rigid-distance constraint rows --------------------------------------------------------------------------------------------------
// Rows that share a world point are solved together: connected components of the constraint graph (union-find over world points), the rows
// regrouped by component, every point of a component numbered inside it.
struct HostConPlan {
  int n_comp = 0;
  std::vector<int> pt, lp;        // [n_con][8] world point of every group slot (0-3 group a, 4-7 group b) and its index inside the component
  std::vector<int> order;         // [n_con] caller's row of the i-th constraint here
  std::vector<int> comp_con, comp_pt;  // [n_comp + 1] first row and first entry of comp_pts of every component
  std::vector<int> comp_pts;      // world points, component by component, in the order the rows name them
  std::vector<long> comp_m;       // [n_comp + 1] running sum of m^2 (m: rows of a component)
  std::vector<double> dist, wgt;  // [n_con] in the order here
  long max_m = 0;
  int max_pts = 0;
  bool big = false;               // a component has more points than the LDS of the constraint kernels holds: their factors live in global scratch
};
template <typename Fail>
static int constraint_plan(Fail fail, int P, int ncp, int n_con, const int32_t* groups_a, const int32_t* groups_b, const double* distances,
                           const double* weights, int lds_points, HostConPlan& out) {
  out = HostConPlan{};
  for (long e = 0; e < (long)n_con * 4; ++e)
    if (groups_a[e] < 0 || groups_a[e] >= P || groups_b[e] < 0 || groups_b[e] >= P)
      return fail(CBA_ERR_INVALID, "cba_set_constraints: point index out of range in constraint %ld", e / 4);
  auto slot = [&](int c, int s) { return (s < 4) ? groups_a[4 * c + s] : groups_b[4 * c + s - 4]; };
  std::vector<int> parent(P);
  for (int q = 0; q < P; ++q) parent[q] = q;
  auto find = [&](int a) { while (parent[a] != a) { parent[a] = parent[parent[a]]; a = parent[a]; } return a; };
  for (int c = 0; c < n_con; ++c) {
    const int r0 = find(groups_a[4 * c]);
    for (int s = 0; s < 8; ++s) {
      const int r = find(slot(c, s));
      if (r != r0) parent[r] = r0;
    }
  }
  std::vector<int> comp_of_root(P, -1), con_comp(n_con);
  int K = 0;
  for (int c = 0; c < n_con; ++c) {
    const int r = find(groups_a[4 * c]);
    if (comp_of_root[r] < 0) comp_of_root[r] = K++;
    con_comp[c] = comp_of_root[r];
  }
  out.n_comp = K;
  out.comp_con.assign(K + 1, 0); out.order.resize(n_con);
  for (int c = 0; c < n_con; ++c) out.comp_con[con_comp[c] + 1]++;
  for (int k = 0; k < K; ++k) out.comp_con[k + 1] += out.comp_con[k];
  {
    std::vector<int> cur(out.comp_con.begin(), out.comp_con.end() - 1);
    for (int c = 0; c < n_con; ++c) out.order[cur[con_comp[c]]++] = c;
  }
  out.pt.resize((size_t)n_con * 8); out.lp.resize((size_t)n_con * 8); out.comp_pt.assign(K + 1, 0);
  out.dist.resize(n_con); out.wgt.resize(n_con); out.comp_m.assign(K + 1, 0);
  std::vector<int> local(P, -1);
  std::vector<int>& comp_pts = out.comp_pts;
  for (int k = 0; k < K; ++k) {
    const int first = (int)comp_pts.size();
    for (int i = out.comp_con[k]; i < out.comp_con[k + 1]; ++i) {
      const int c = out.order[i];
      out.dist[i] = distances[c]; out.wgt[i] = weights[c];
      for (int s = 0; s < 8; ++s) {
        const int q = slot(c, s);
        if (local[q] < 0) { local[q] = (int)comp_pts.size() - first; comp_pts.push_back(q); }
        out.pt[(size_t)i * 8 + s] = q; out.lp[(size_t)i * 8 + s] = local[q];
      }
    }
    for (size_t j = first; j < comp_pts.size(); ++j) local[comp_pts[j]] = -1;
    out.comp_pt[k + 1] = (int)comp_pts.size();
    const long m = out.comp_con[k + 1] - out.comp_con[k];
    out.comp_m[k + 1] = out.comp_m[k] + m * m;
    out.max_m = std::max(out.max_m, m);
    out.max_pts = std::max(out.max_pts, (int)comp_pts.size() - first);
  }
  out.big = out.max_pts > lds_points;
  // memory of the Woodbury correction: M (sum of m^2 over the components) and G (n_con x (ncp + 1)), doubles
  if (out.comp_m[K] > (1L << 28) || (long)n_con * (ncp + 1) > (1L << 29))
    return fail(CBA_ERR_UNSUPPORTED, "cba_set_constraints: the constraint rows need %.1f GB for the per-component matrices (sum of m^2 = %ld) and %.1f GB for their "
                "camera coupling (%d rows x %d camera parameters); the limits are 2 GB and 4 GB - use fewer rows per object and frame (DESIGN.md 2.2)",
                out.comp_m[K] * 8e-9, out.comp_m[K], (double)n_con * (ncp + 1) * 8e-9, n_con, ncp);
  return CBA_OK;
}
// constrained points that no observation sees: the build writes neither their V nor their g_p, the back-substitution not their step
static std::vector<int> constraint_orphans(const std::vector<int>& comp_pts, const int* pt_start) {
  std::vector<int> orphan;
  for (const int q : comp_pts)
    if (pt_start[(size_t)q + 1] == pt_start[q]) orphan.push_back(q);
  return orphan;
}

// ---- mapped host mailbox -------------------------------------------------------------------------------------------------------------
// One mapped allocation, offsets in doubles: scalars (k_publish; slot kSeqSlot is the sequence word the host spins on) | camera blocks of up to
// three vectors + a sequence word | flags (4 ints) | the four camera blocks a bounded fused iteration sends with its packet
struct MailLayout {
  static constexpr size_t kScalars = 64, kSeqSlot = 63;
  size_t cam, flags, bcam, total;
  explicit MailLayout(int ncp) : cam(kScalars), flags(cam + (size_t)3 * ncp + 8), bcam(flags + 2), total(bcam + (size_t)4 * ncp) {}
};

// ---- cba_triangulate -----------------------------------------------------------------------------------------------------------------
// k_triangulate reads obs_cam and obs_xy at [pt_start[q], pt_start[q + 1]) and the call sizes its copies by pt_start[n_points]: the table starts at 0
// and never decreases (so that every entry lies in [0, pt_start[n_points]]).  n_points > 0.
template <typename Fail>
static int triangulate_starts_ok(Fail fail, int64_t n_points, const int64_t* pt_start) {
  if (pt_start[0] != 0) return fail(CBA_ERR_INVALID, "cba_triangulate: pt_start[0] is %lld, not 0", (long long)pt_start[0]);
  for (int64_t q = 0; q < n_points; ++q)
    if (pt_start[q + 1] < pt_start[q])
      return fail(CBA_ERR_INVALID, "cba_triangulate: pt_start[%lld] = %lld is below pt_start[%lld] = %lld", (long long)(q + 1), (long long)pt_start[q + 1],
                  (long long)q, (long long)pt_start[q]);
  return CBA_OK;
}
