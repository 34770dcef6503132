// Kernel variants and LDS layouts of the bundle-adjustment engine, plain C++ (no HIP): what has to agree between a kernel's carve-up of its
// dynamic LDS, the byte count of its launch and the routes cba_create chooses — written once.
//   CostLds / BuildLds / BuildCsLds / JvLds / TprepLds / BacksubLds / SmallSolveLds
//                               one struct per kernel family: the offset of every region and bytes().  The kernel (cba_kernels.h) takes its
//                               pointers from the struct, the host (cba_lib.hip) the launch's LDS size and the ceiling it raises.
//   BsrCfg                      the same for k_backsub_rec
//   *_lds_bytes                 kernels with a single region
//   KernelRoutes / kernel_routes
//                               which variant of every family a handle runs: camera table in LDS or global, the build route, the
//                               back-substitution, and the refusal of a rig no route holds.  Filled once by cba_create; the launch sites and
//                               cba_get_info read it.
// Offsets are in doubles from the start of the dynamic LDS; the int tables of the fixed-order variants lie behind the doubles, their offsets are
// in bytes.  Shared by the kernels, the device library and the CPU harness tests/native/kernel_plan_harness.cpp (tests/test_kernel_plan.py).
#pragma once
#include <algorithm>
#include <cstddef>

#include "ba_math.h"        // CBA_HD
#include "chol_schedule.h"  // NB

namespace cba {

// The sizes the layouts are written with.  cba_kernels.h keeps BLOCK, CHUNK and DET_ROUND under their own names, where the kernels and the set-up
// plan's test (tests/test_setup_plan.py reads them out of that file) look for them, and asserts that they are these.
namespace dims {
constexpr int BLOCK = 256;     // threads of a workgroup of the per-observation kernels
constexpr int CHUNK = 256;     // observations of a chunk at most
constexpr int DET_ROUND = 9;   // fixed-order sums: values per observation and round
}  // namespace dims
constexpr int WAVE = 64;

// LDS copy of the camera table.  Rows are padded to 49 doubles: with the natural stride of 48 doubles
// (96 dwords == 32 mod 64 banks) the lanes of a wave, each reading the same field of a different camera,
// would land on two bank pairs (32-way conflict); an odd stride spreads 32 cameras over all bank pairs.
constexpr int CAMTAB_LIVE = 36;               // doubles of a CamTab row in use (everything up to and including pad[0], the camera's parameter offset)
constexpr int CAMTAB_LDS = CAMTAB_LIVE + 1;    // 37 (odd): the padding stays in HBM (49 doubles per camera cost k_build / k_tprep their third workgroup per CU)

template <int NC> struct UPack {
  static constexpr int TRI = NC * (NC + 1) / 2;
  static constexpr int STRIDE = TRI + NC;  // upper triangle + gradient
  CBA_HD static constexpr int idx(int r, int c) { return r * NC - r * (r - 1) / 2 + (c - r); }
};

constexpr int DET_LD = dims::CHUNK + 1;         // row stride of the parking area (odd: the nine rows of a task group hit nine banks)

// sizes of a Schur record (cba_kernels.h describes the record above k_tprep)
template <int NC> struct SchurRec {
  static constexpr int NVAL = (NC == 9) ? 21 : 10;        // doubles that carry data
  static constexpr int NPH = (NVAL + 1) / 2;              // 16-byte pieces that carry data: 5 / 11
  static constexpr int LST = (NPH & 1) ? NPH : NPH + 1;   // record stride in LDS, 16-byte pieces, odd: 5 / 11 (bank spread)
  static constexpr int REC = 2 * LST;                     // record stride in LDS, doubles: 10 / 22
  // record stride in HBM, doubles: the pieces that carry data, 10 / 22 (80 / 176 bytes).  (128-byte records, one line each, were measured on the
  // twelve-double form: the pair kernel's issue phase shrank by 7 %, k_tprep grew by as much, and the pass moved 1.15 GB instead of 0.93 GB through HBM.)
  static constexpr int HREC = 2 * NPH;
  static constexpr int STAGE = (HREC / 2) | 1;            // k_tprep's transposing LDS stage: record stride in pieces, odd (bank spread)
  // waves of a k_tprep workgroup that stage at the same time.  NC = 9: two, in two turns — with a stage for all four (45 KB) next to the camera
  // table the kernel had 92 KB of LDS and ran one workgroup per CU
  static constexpr int STAGE_WAVES = (NC == 9) ? 2 : 4;
};
static_assert(SchurRec<6>::REC == 10 && SchurRec<6>::LST == 5 && SchurRec<6>::HREC == 10 && SchurRec<6>::STAGE == 5 && SchurRec<9>::REC == 22 &&
                  SchurRec<9>::LST == 11,
              "record sizes");

constexpr int SMALL_N = 96;            // k_small_solve: camera parameters at most
constexpr int SMALL_LD = SMALL_N + 1;  // odd row stride

// ---- LDS layouts -----------------------------------------------------------------------------------------------------------------------
constexpr int LDS_RED = 8;  // doubles kept for block_sum / block_max (dims::BLOCK / WAVE are used)
// doubles of the LDS copy of the camera table; CAMG variants read the table through the vector cache and keep none
CBA_HD int camtab_lds(int n_cams, bool camg) { return camg ? 0 : n_cams * CAMTAB_LDS; }

struct CostLds {  // k_cost<WRITE_R, CAMG>
  int tab, red, end;
  CBA_HD CostLds(int n_cams, bool camg) : tab(0), red(camtab_lds(n_cams, camg)), end(red + LDS_RED) {}
  CBA_HD size_t bytes() const { return (size_t)end * 8; }
};

// k_build<NC, DETM, CAMG>.  U: the packed camera blocks; det (DETM > 0): the parking area of det_round in their place, and behind the doubles the
// chunk's camera order, perm[dims::CHUNK] and cs[n_cams + 1] (ints; offsets in bytes).  The fixed-order sums keep the camera table in LDS (!(det && camg)).
template <int NC> struct BuildLds {
  int tab, U, pt, red, end;  // pt: [9][dims::CHUNK]
  int perm, cs;
  size_t total;
  CBA_HD BuildLds(int n_cams, bool det, bool camg)
      : tab(0), U(camtab_lds(n_cams, camg)), pt(U + (det ? dims::DET_ROUND * DET_LD : n_cams * UPack<NC>::STRIDE)), red(pt + 9 * dims::CHUNK), end(red + LDS_RED),
        perm(end * 8), cs(perm + dims::CHUNK * 4), total(det ? (size_t)cs + ((size_t)n_cams + 1) * 4 : (size_t)end * 8) {}
  CBA_HD size_t bytes() const { return total; }
};

// k_build_cs<NC, CAMG, UGLOB, TRIAL>; pmax: CsPlan::pmax, the row stride of the per-point arrays.  UGLOB: the blocks are one global copy, none in LDS.
template <int NC> struct BuildCsLds {
  int tab, U, vg, x, red, end;  // vg: [9][pmax], x: [3][pmax]
  CBA_HD BuildCsLds(int n_cams, int pmax, bool camg, bool uglob)
      : tab(0), U(camtab_lds(n_cams, camg)), vg(U + (uglob ? 0 : n_cams * UPack<NC>::STRIDE)), x(vg + 9 * pmax), red(x + 3 * pmax), end(red + LDS_RED) {}
  CBA_HD size_t bytes() const { return (size_t)end * 8; }
};

struct JvLds {  // k_jv<NC, NV, CAMG, LIN>
  int tab, v, red, end;  // v: [nv][ncp_pad]
  CBA_HD JvLds(int n_cams, int ncp_pad, int nv, bool camg) : tab(0), v(camtab_lds(n_cams, camg)), red(v + nv * ncp_pad), end(red + LDS_RED) {}
  CBA_HD size_t bytes() const { return (size_t)end * 8; }
};

// k_tprep<NC, DETM, CAMG, LINF, LIN>.  stage: the record transpose, [STAGE_WAVES][WAVE * STAGE] 16-byte pieces (read as double2: at the front).
// b: the rhs sums, ncp_pad; det: the parking area of det_round in their place, then perm and cs as in BuildLds.
template <int NC> struct TprepLds {
  int stage, tab, b, end;
  int perm, cs;
  size_t total;
  CBA_HD TprepLds(int n_cams, int ncp_pad, bool det, bool camg)
      : stage(0), tab(SchurRec<NC>::STAGE_WAVES * WAVE * SchurRec<NC>::STAGE * 2), b(tab + camtab_lds(n_cams, camg)),
        end(b + (det ? dims::DET_ROUND * DET_LD : ncp_pad)), perm(end * 8), cs(perm + dims::CHUNK * 4),
        total(det ? (size_t)cs + ((size_t)n_cams + 1) * 4 : (size_t)end * 8) {}
  CBA_HD size_t bytes() const { return total; }
};

struct BacksubLds {  // k_backsub<NC, CAMG, SCAL>
  int tab, dc, pt, end;  // dc: ncp_pad, pt: [3][dims::CHUNK]
  CBA_HD BacksubLds(int n_cams, int ncp_pad, bool camg) : tab(0), dc(camtab_lds(n_cams, camg)), pt(dc + ncp_pad), end(pt + 3 * dims::CHUNK) {}
  CBA_HD size_t bytes() const { return (size_t)end * 8; }
};

// k_backsub_rec<NC, SCAL>
constexpr int BSR_PT = 3 * dims::CHUNK;  // doubles of one buffer of per-observation terms
template <int NC> struct BsrCfg {
  static constexpr int NP = SchurRec<NC>::NPH;       // 16-byte pieces of a record in HBM (5 / 11)
  static constexpr int CS = (NC == 9) ? 9 : 8;       // doubles of a camera's entry: its step (w, dt [, di]); six parameters: and t0, t1
  static constexpr int CSS = CS;                     // its stride in LDS (an odd stride would spread the banks; 40 000 bytes per workgroup let four share a CU)
  static constexpr int REC = 0, PT = dims::BLOCK * NP * 2, STEP = PT + 2 * BSR_PT;  // records (read as double2), [2][3][dims::CHUNK], [n_cams][CSS]
  static constexpr size_t lds_bytes(int n_cams) { return ((size_t)dims::BLOCK * NP * 2 + 2 * BSR_PT + (size_t)n_cams * CSS + 8) * sizeof(double); }
};

// k_small_solve: W [SMALL_N + 1][SMALL_LD] (S, then rhs^T), D [2 NB][NB + 1] (chol_factor_block's block), X [nbk][NB][NB + 1] (inverses of the
// diagonal blocks), y [SMALL_N]; behind the doubles the ints pc[SMALL_N], pl[SMALL_N] (bytes)
struct SmallSolveLds {
  static constexpr int W = 0, D = (SMALL_N + 1) * SMALL_LD, X = D + 2 * NB * (NB + 1), y = X + (SMALL_N + NB - 1) / NB * NB * (NB + 1), end = y + SMALL_N;
  static constexpr int pc = end * 8, pl = pc + SMALL_N * 4;
  static constexpr size_t bytes() { return (size_t)pl + SMALL_N * 4; }
};

// kernels with one region
CBA_HD size_t heavy_schur_lds_bytes(int ncp) { return (size_t)ncp * 3 * sizeof(double) + (size_t)ncp * sizeof(int); }  // k_heavy_schur
CBA_HD size_t chol_apply_lds_bytes(int n) { return (size_t)n * 8; }                                                    // k_chol_apply: y[n]
CBA_HD size_t step_cam_lds_bytes(int ncp_pad) { return (size_t)ncp_pad * sizeof(double); }                             // k_step_cam: the trial point's cameras
CBA_HD size_t con_backsub_small_lds_bytes(int max_np, int max_m) { return (size_t)(9 * max_np + 2 * max_m) * sizeof(double); }  // k_con_backsub_small

// ---- routes ----------------------------------------------------------------------------------------------------------------------------
constexpr size_t LDS_MAX = 160 * 1024;     // of a workgroup: beyond, no launch
constexpr size_t LDS_HALF = 80 * 1024;     // two workgroups per CU
constexpr size_t LDS_TAB_MAX = 150 * 1024; // the camera table stays in LDS while its largest neighbour fits this next to it
constexpr const char* LDS_REFUSAL = "kernel needs %zu bytes of LDS (> 160 KiB)";

struct KernelRoutes {
  // The camera table in LDS (296 B per camera) next to the largest other LDS user: beyond the budget every per-observation kernel switches to
  // its CAMG variant (table through the vector cache).  What then bounds the camera count is the per-camera accumulators of the linearisation
  // (nc (nc + 3) / 2 doubles per camera in LDS: ~650 six-parameter or ~320 nine-parameter cameras).  CBA_CAMTAB_GLOBAL=0/1 forces the choice (tests).
  bool tab_global = false;
  bool build_cs = false;       // the build runs over camera-sorted super-chunks (k_build_cs), not point by point (k_build)
  // k_build<NC, 0, true> reads the camera table from global memory: chosen when the table is what keeps a second workgroup off the CU, and when
  // table + accumulators exceed the LDS; CBA_BUILD_CAMG=0/1 forces the choice
  bool build_pt_camg = false;
  bool build_cs_camg = false;  // k_build_cs keeps the camera table in LDS while that leaves room for two workgroups per CU
  // beyond ~650 six- / ~320 nine-parameter cameras the packed camera blocks do not fit the LDS: one global copy, FP64 global atomics (k_build_cs<.., UGLOB>)
  bool build_uglob = false;
  // back-substitution from the T records: whenever no chunk is a fragment of a very large point (those add their sums by atomics in k_backsub) and the
  // per-camera step entries fit the LDS next to the record buffer (~2400 six- / ~1000 nine-parameter cameras); CBA_BACKSUB_REC=0: the old kernel (A/B).
  // Nine-parameter cameras keep k_backsub unless CBA_BACKSUB_REC=1: their records are 176 bytes, and streaming them costs more than linearising again
  // (cfg5, round 6: 394 us against 326; six-parameter cameras, cfg4: 48 against 64)
  bool backsub_rec = false;
  size_t refused_bytes = 0;    // != 0: a kernel of the chosen routes needs this much LDS, more than LDS_MAX (LDS_REFUSAL)
  bool build_camg() const { return build_cs ? build_cs_camg : build_pt_camg; }  // of the build kernel that runs
};

// A switch is -1 (not set), 0 or 1: the caller parses the environment.  n_sc, pmax: the camera-sorted plan (n_sc == 0: none).
template <int NC>
inline KernelRoutes kernel_routes_nc(int C, int ncp_pad, int det_m, int n_heavy, int n_sc, int pmax, bool eval_only, bool has_fragments,
                                     int camtab_global_switch, int build_camg_switch, int backsub_rec_switch) {
  KernelRoutes r;
  const bool det = det_m != 0;
  {
    const size_t worst = std::max(std::max(JvLds(C, ncp_pad, 2, false).bytes(), BacksubLds(C, ncp_pad, false).bytes()), TprepLds<NC>(C, ncp_pad, det, false).bytes());
    r.tab_global = !det && worst > LDS_TAB_MAX;  // (the linearisation has its own switch: build_pt_camg)
    if (camtab_global_switch >= 0) r.tab_global = camtab_global_switch != 0 && !det;
  }
  {
    const size_t with_tab = BuildLds<NC>(C, false, false).bytes(), without = BuildLds<NC>(C, false, true).bytes();
    if (r.tab_global) r.build_pt_camg = true;
    else if (build_camg_switch >= 0) r.build_pt_camg = build_camg_switch != 0 && !det;
    // (a second workgroup per CU when the table is what keeps it off; no choice at all when table + accumulators exceed the LDS)
    else r.build_pt_camg = !det && ((with_tab > LDS_HALF && without <= LDS_HALF) || with_tab > LDS_MAX);
  }
  r.build_cs = n_sc && !det && !n_heavy;
  if (r.build_cs) {
    r.build_uglob = BuildCsLds<NC>(C, pmax, true, false).bytes() > LDS_MAX;  // (then build_cs_camg holds as well: the table adds to what does not fit)
    r.build_cs_camg = r.tab_global || BuildCsLds<NC>(C, pmax, false, false).bytes() > LDS_HALF;
  }
  r.backsub_rec = (NC == 6 || backsub_rec_switch == 1) && !eval_only && !has_fragments && BsrCfg<NC>::lds_bytes(C) <= LDS_TAB_MAX && backsub_rec_switch != 0;
  // what the handle launches with (configure_kernels raises the ceilings in this order): the first that does not fit is reported
  const size_t need[] = {CostLds(C, r.tab_global).bytes(),
                         r.build_cs ? BuildCsLds<NC>(C, pmax, r.build_cs_camg, r.build_uglob).bytes() : 0,
                         // (the point-ordered kernel keeps the packed blocks in LDS: not made ready with that many cameras)
                         r.build_uglob ? 0 : BuildLds<NC>(C, det, r.build_pt_camg).bytes(),
                         det ? TprepLds<NC>(C, ncp_pad, true, false).bytes() : 0,
                         JvLds(C, ncp_pad, 1, r.tab_global).bytes(), JvLds(C, ncp_pad, 2, r.tab_global).bytes(),
                         TprepLds<NC>(C, ncp_pad, det, r.tab_global).bytes(), BacksubLds(C, ncp_pad, r.tab_global).bytes()};
  for (size_t b : need)
    if (b > LDS_MAX && !r.refused_bytes) r.refused_bytes = b;
  return r;
}
inline KernelRoutes kernel_routes(int C, int nct, int ncp_pad, int det_m, int n_heavy, int n_sc, int pmax, bool eval_only, bool has_fragments,
                                  int camtab_global_switch, int build_camg_switch, int backsub_rec_switch) {
  return nct == 9 ? kernel_routes_nc<9>(C, ncp_pad, det_m, n_heavy, n_sc, pmax, eval_only, has_fragments, camtab_global_switch, build_camg_switch, backsub_rec_switch)
                  : kernel_routes_nc<6>(C, ncp_pad, det_m, n_heavy, n_sc, pmax, eval_only, has_fragments, camtab_global_switch, build_camg_switch, backsub_rec_switch);
}

}  // namespace cba
