// The LDS layouts and the routes of the kernels (caliscope_amd/csrc/kernel_plan.h) behind a flat C interface, compiled by g++:
// tests/test_kernel_plan.py checks what they return against Python restatements of the byte formulas and of the route rules.
#include <cstdio>

#include "../../caliscope_amd/csrc/kernel_plan.h"

using namespace cba;

namespace {
constexpr int ROW = 8;  // boundaries per layout at most
enum Family { COST = 0, BUILD, BUILD_CS, JV, TPREP, BACKSUB, BACKSUB_REC, SMALL_SOLVE };
enum Flag { CAMG = 1, DET = 2, UGLOB = 4 };

// region boundaries in bytes, first to last; returns how many
template <int NC>
int boundaries(int family, int C, int ncp_pad, int pmax, int nv, int flags, long* o, long* bytes) {
  const bool camg = flags & CAMG, det = flags & DET, uglob = flags & UGLOB;
  int k = 0;
  auto d = [&](int doubles) { o[k++] = 8L * doubles; };
  auto b = [&](long at) { o[k++] = at; };
  switch (family) {
    case COST: { const CostLds L(C, camg); d(L.tab); d(L.red); d(L.end); *bytes = (long)L.bytes(); break; }
    case BUILD: {
      const BuildLds<NC> L(C, det, camg);
      d(L.tab); d(L.U); d(L.pt); d(L.red); d(L.end);
      if (det) { b(L.perm); b(L.cs); b((long)L.total); }  // (perm starts where the doubles end: an empty region between them)
      *bytes = (long)L.bytes();
      break;
    }
    case BUILD_CS: { const BuildCsLds<NC> L(C, pmax, camg, uglob); d(L.tab); d(L.U); d(L.vg); d(L.x); d(L.red); d(L.end); *bytes = (long)L.bytes(); break; }
    case JV: { const JvLds L(C, ncp_pad, nv, camg); d(L.tab); d(L.v); d(L.red); d(L.end); *bytes = (long)L.bytes(); break; }
    case TPREP: {
      const TprepLds<NC> L(C, ncp_pad, det, camg);
      d(L.stage); d(L.tab); d(L.b); d(L.end);
      if (det) { b(L.perm); b(L.cs); b((long)L.total); }
      *bytes = (long)L.bytes();
      break;
    }
    case BACKSUB: { const BacksubLds L(C, ncp_pad, camg); d(L.tab); d(L.dc); d(L.pt); d(L.end); *bytes = (long)L.bytes(); break; }
    case BACKSUB_REC: {
      using Cfg = BsrCfg<NC>;
      d(Cfg::REC); d(Cfg::PT); d(Cfg::STEP); d(Cfg::STEP + C * Cfg::CSS); d(Cfg::STEP + C * Cfg::CSS + 8);  // (eight doubles to spare)
      *bytes = (long)Cfg::lds_bytes(C);
      break;
    }
    case SMALL_SOLVE: {
      using L = SmallSolveLds;
      d(L::W); d(L::D); d(L::X); d(L::y); b(L::pc); b(L::pl); b((long)L::bytes());
      *bytes = (long)L::bytes();
      break;
    }
    default: return -1;
  }
  return k;
}
}  // namespace

extern "C" {

// n layouts of one family (camera counts C[i], camera blocks ncp_pad[i]): out[i][ROW] the region boundaries in bytes, bytes_out[i] = bytes().
// Returns the number of boundaries of a row.
int kp_layout(int family, int nc, int n, const int* C, const int* ncp_pad, int pmax, int nv, int flags, long* out, long* bytes_out) {
  int k = -1;
  for (int i = 0; i < n; ++i)
    k = nc == 9 ? boundaries<9>(family, C[i], ncp_pad[i], pmax, nv, flags, out + (long)i * ROW, bytes_out + i)
                : boundaries<6>(family, C[i], ncp_pad[i], pmax, nv, flags, out + (long)i * ROW, bytes_out + i);
  return k;
}

// the kernels with one region: heavy_schur(a), chol_apply(a), step_cam(a), con_backsub_small(a, b)
void kp_single(int a, int b, long* out) {
  out[0] = (long)heavy_schur_lds_bytes(a); out[1] = (long)chol_apply_lds_bytes(a); out[2] = (long)step_cam_lds_bytes(a); out[3] = (long)con_backsub_small_lds_bytes(a, b);
}

// routes of n handles; bits_out: 1 tab_global, 2 build_cs, 4 build_pt_camg, 8 build_cs_camg, 16 build_uglob, 32 backsub_rec, 64 build_camg()
void kp_routes(int n, const int* C, int nct, const int* ncp_pad, int det_m, int n_heavy, int n_sc, int pmax, int eval_only, int has_fragments, int camtab_global_switch,
               int build_camg_switch, int backsub_rec_switch, int* bits_out, long* refused_out) {
  for (int i = 0; i < n; ++i) {
    const KernelRoutes r = kernel_routes(C[i], nct, ncp_pad[i], det_m, n_heavy, n_sc, pmax, eval_only != 0, has_fragments != 0, camtab_global_switch,
                                         build_camg_switch, backsub_rec_switch);
    bits_out[i] = (r.tab_global ? 1 : 0) | (r.build_cs ? 2 : 0) | (r.build_pt_camg ? 4 : 0) | (r.build_cs_camg ? 8 : 0) | (r.build_uglob ? 16 : 0) |
                  (r.backsub_rec ? 32 : 0) | (r.build_camg() ? 64 : 0);
    refused_out[i] = (long)r.refused_bytes;
  }
}

int kp_refusal(long bytes, char* buf, int size) { return snprintf(buf, (size_t)size, LDS_REFUSAL, (size_t)bytes); }

}  // extern "C"
