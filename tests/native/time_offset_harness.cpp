// CPU harness around caliscope_amd/csrc/time_offset_math.h — TEST INFRASTRUCTURE (built by g++ in tests/time_offset_native.py).  It
// evaluates cba_estimate_time_offsets with the checks, the driver of the rounds (sync_drive) and the routines that time_offset_lib.hip
// uses: the per-slot bodies in loops, the workgroup of k_sync_reduce_solve as one thread of one (t = 0, NT = 1), the Gram matrix and
// the wave sums as plain loops in ascending order (one partial, one "wave" per 64 slots).  It is not a CPU fallback: nothing in
// caliscope_amd/ loads it.
#include <cstdint>
#include <string>
#include <vector>

#include "time_offset_math.h"

using namespace cba;

namespace {
std::string g_error;

struct HostBackend {
  const cba_traj_desc* d;
  const cba_time_offset_options* o;
  const SyncPlan& plan;
  int64_t n_slots;
  std::vector<double> xy, ft, frame, X0, dX, V, L, Q, Fw, Dw, bw, partial, delta0, ddelta, dnew, sinv, e2_before, e2_after, out_xy;
  std::vector<uint8_t> valid, moving, free_col, out_used;
  std::vector<int64_t> used;
  double scal[4];

  HostBackend(const cba_traj_desc* d_, const cba_time_offset_options* o_, const SyncPlan& p) : d(d_), o(o_), plan(p), n_slots(d_->n_frames * d_->n_traj) {
    const size_t cells = (size_t)d->n_cams * (size_t)n_slots, nc = (size_t)plan.n_cols;
    xy.assign(2 * cells, traj_nan());
    ft.assign(cells, traj_nan());
    frame.assign((size_t)d->n_frames, 0.0);
    X0.assign(3 * (size_t)n_slots, 0.0);
    dX.assign(3 * (size_t)n_slots, 0.0);
    V.assign(3 * (size_t)n_slots, 0.0);
    valid.assign((size_t)n_slots, 0);
    moving.assign((size_t)n_slots, 0);
    L.assign(6 * (size_t)plan.ld, 0.0);
    Q.assign(3 * nc * (size_t)plan.ld, 0.0);
    Fw.assign((size_t)plan.n_waves, 0.0);
    Dw.assign((size_t)plan.n_waves * nc, 0.0);
    bw.assign((size_t)plan.n_waves * nc, 0.0);
    partial.assign((size_t)SYNC_LD * SYNC_LD, 0.0);
    delta0.assign(nc, 0.0); ddelta.assign(nc, 0.0); dnew.assign(nc, 0.0); sinv.assign(nc, 0.0);
    free_col.assign(nc, 0);
    e2_before.assign((size_t)d->n_cams, 0.0); e2_after.assign((size_t)d->n_cams, 0.0);
    used.assign((size_t)d->n_cams, 0);
    out_xy.assign(2 * (size_t)d->n_rows, 0.0);
    out_used.assign((size_t)d->n_rows, 0);
    for (int64_t i = 0; i < d->n_rows; ++i)
      traj_fill2d_row(d->n_rows, d->n_traj, n_slots, i, d->row_cam, d->row_slot, d->row_xy, d->row_time, 0, xy.data(), ft.data());
    for (int64_t f = 0; f < d->n_frames; ++f) frame[(size_t)f] = traj_frame_mean(d->n_cams, d->n_traj, n_slots, f, ft.data());
    for (int64_t s = 0; s < n_slots; ++s)
      valid[(size_t)s] = traj_triangulate_slot(d->n_cams, n_slots, s, d->cam_posed, d->cam_model, d->cam_intr, d->cam_P, xy.data(), d->float32_io ? 1 : 0,
                                               X0.data() + 3 * s) >= 2 ? 1 : 0;
  }

  bool velocity(bool first) {
    for (int64_t s = 0; s < n_slots; ++s)
      sync_velocity_slot(d->n_frames, d->n_traj, s, o->max_neighbour_gap, valid.data(), X0.data(), frame.data(), V.data(), first ? moving.data() : nullptr);
    return true;
  }
  bool rows(bool final) {
    std::vector<double>& e2 = final ? e2_after : e2_before;
    for (int32_t c = 0; c < d->n_cams; ++c) {
      const int32_t col = plan.cam_col[(size_t)c];
      double sum = 0.0;
      int64_t n = 0, m = 0;
      for (int64_t i = plan.cam_row_start[(size_t)c]; i < plan.cam_row_start[(size_t)c + 1]; ++i) {
        double e;
        int64_t u, mv;
        sync_row(final, i, c, col, d->n_traj, d->cam_model, d->cam_intr, d->cam_P, d->row_slot, d->row_xy, d->row_time, frame.data(), valid.data(),
                 moving.data(), X0.data(), V.data(), delta0.data(), out_xy.data(), out_used.data(), &e, &u, &mv);
        sum += e; n += u; m += mv;
      }
      e2[(size_t)c] = sum;
      if (!final) {
        used[(size_t)c] = n;
        if (col >= 0) free_col[(size_t)col] = col != plan.ref_col && m >= (int64_t)o->min_rows ? 1 : 0;
      }
    }
    return true;
  }
  bool eval(double alpha, SyncScalars& sc) {
    const int32_t nc = plan.n_cols;
    const SyncBuildArgs B{d->n_cams, nc, plan.ref_col, n_slots, d->n_traj, plan.ld, plan.cam_col.data(), d->cam_model, d->cam_intr, d->cam_P, xy.data(),
                          ft.data(), frame.data(), valid.data(), X0.data(), dX.data(), V.data(), delta0.data(), ddelta.data(), alpha, plan.max_offset,
                          o->huber_px};
    std::fill(Fw.begin(), Fw.end(), 0.0);
    std::fill(Dw.begin(), Dw.end(), 0.0);
    std::fill(bw.begin(), bw.end(), 0.0);
    for (int64_t s = 0; s < n_slots; ++s) {
      const int64_t wave = s >> 6;
      Fw[(size_t)wave] += sync_build_slot(B, s, true, Q.data(), L.data(), [&](int32_t col, double dc, double bc) {
        Dw[(size_t)(wave * nc + col)] += dc;
        bw[(size_t)(wave * nc + col)] += bc;
      });
    }
    for (int32_t i = 0; i < nc; ++i)
      for (int32_t j = i; j < nc; ++j) {
        double sum = 0.0;
        for (int64_t s = 0; s < n_slots; ++s)
          for (int k = 0; k < 3; ++k) sum += Q[(size_t)((3 * (int64_t)i + k) * plan.ld + s)] * Q[(size_t)((3 * (int64_t)j + k) * plan.ld + s)];
        partial[(size_t)(i * SYNC_LD + j)] = sum;
      }
    const SyncSolveArgs S{nc, plan.ref_col, 1, plan.n_waves, partial.data(), Fw.data(), Dw.data(), bw.data(), free_col.data(), dnew.data(), sinv.data(), scal};
    std::vector<double> Sm((size_t)SYNC_LD * SYNC_LD), Ym((size_t)SYNC_LD * SYNC_LD), vec(3 * SYNC_LD);
    std::vector<int> idx(SYNC_LD + 2);
    sync_reduce_solve(0, 1, S, Sm.data(), Ym.data(), vec.data(), idx.data());
    sc.F = scal[0]; sc.pred = scal[1]; sc.step = scal[2]; sc.ok = scal[3];
    return true;
  }
  bool step(double alpha) {
    for (int32_t col = 0; col < plan.n_cols; ++col) sync_update_col(col, alpha, plan.max_offset, dnew.data(), delta0.data(), ddelta.data());
    for (int64_t s = 0; s < n_slots; ++s) sync_update_slot(plan.n_cols, plan.ref_col, plan.ld, s, Q.data(), L.data(), dnew.data(), alpha, X0.data(), dX.data());
    return true;
  }
  bool offsets(double* by_col) {
    for (int32_t col = 0; col < plan.n_cols; ++col) by_col[col] = delta0[(size_t)col];
    return true;
  }
  bool set_offsets(const double* by_col) {
    for (int32_t col = 0; col < plan.n_cols; ++col) delta0[(size_t)col] = by_col[col];
    return true;
  }
};
}  // namespace

extern "C" {

const char* toh_last_error() { return g_error.c_str(); }

// cba_estimate_time_offsets on the host: 0, -1 (invalid) or -4 (unsupported) with toh_last_error() set
int toh_estimate_time_offsets(const cba_traj_desc* d, const cba_time_offset_options* o, cba_time_offset_out* out) {
  if (!d || !o || !out) { g_error = "cba_estimate_time_offsets: null argument"; return -1; }
  SyncPlan plan;
  bool launch = false;
  const int rc = sync_validate(d, o, (double)d->memory_limit, plan, g_error, &launch);
  if (rc) return rc;
  if (!launch) { sync_nothing(d, plan, out); return 0; }
  HostBackend be(d, o, plan);
  int32_t rounds = 0;
  uint8_t converged = 0;
  double F_end = 0.0;
  sync_drive(be, plan, d->n_rows, (int)o->max_rounds, &rounds, &converged, &F_end);
  int64_t n_points = 0;
  for (int64_t s = 0; s < be.n_slots; ++s) {
    n_points += be.valid[(size_t)s] ? 1 : 0;
    if (out->valid) out->valid[s] = be.valid[(size_t)s];
    for (int k = 0; k < 3; ++k) {
      if (out->xyz) out->xyz[3 * s + k] = be.X0[(size_t)(3 * s + k)];
      if (out->velocity) out->velocity[3 * s + k] = be.V[(size_t)(3 * s + k)];
    }
  }
  for (int64_t f = 0; f < d->n_frames; ++f)
    if (out->frame_time) out->frame_time[f] = be.frame[(size_t)f];
  for (int64_t i = 0; i < d->n_rows; ++i) {
    if (out->row_xy) { out->row_xy[2 * i] = be.out_xy[(size_t)(2 * i)]; out->row_xy[2 * i + 1] = be.out_xy[(size_t)(2 * i + 1)]; }
    if (out->row_used) out->row_used[i] = be.out_used[(size_t)i];
  }
  sync_report(d, plan, be.delta0.data(), be.sinv.data(), be.free_col.data(), be.e2_before.data(), be.e2_after.data(), be.used.data(), n_points, F_end, out);
  if (out->rounds) *out->rounds = rounds;
  if (out->converged) *out->converged = converged;
  return 0;
}

}
