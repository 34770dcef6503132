// cba_estimate_time_offsets of libcaliscope_ba.so (C ABI, model and algorithm: include/caliscope/time_offsets.h): the time offset of
// every posed camera against a reference camera, the trajectories at the nominal frame times and the motion-compensated pixel of every
// row.  What a thread does, the one-workgroup solve, the checks and the host's driver of the rounds are time_offset_math.h (shared with
// tests/native/time_offset_harness.cpp); this file holds the kernels, the device backend of the driver and the entry point.
//
//   k_sync_scatter, k_sync_frame_time, k_sync_triangulate
//                        the fill-free grid, tau_f and the DLT start: the thread bodies of trajectory_math.h.
//   k_sync_velocity      one thread per slot: V of the round, and in the first round the moving flag.
//   k_sync_build         one thread per slot, the access pattern of k_traj_refine (neighbouring threads read neighbouring cells of each
//                        camera's grid), two passes over the cameras, no early exit and no lane leaves: pass 1 gives H, g, the cost and
//                        the factor L, pass 2 stores q_c = L^-1 E_c per posed camera (q_n = L^-1 g in the reference camera's column)
//                        to Q[(3 col + k) ld + s], so a wave's stores are contiguous, and reduces d_c, b_c and the cost over the wave
//                        by a butterfly of shuffles (a fixed tree): one partial per wave.
//   k_sync_gram          G = Q^T Q with v_mfma_f64_16x16x4: wave w of a workgroup holds tile row w of the 4 x 4 grid of 16 x 16 tiles
//                        (the upper block triangle), workgroup g adds the chunks g, g + groups, .. of 256 slots in ascending order
//                        and writes one partial.  A lane loads 4 consecutive slots of its column (32 bytes); MFMA step m pairs
//                        the m-th of each lane's four on both operands, the same permutation of the depth on both sides.
//   k_sync_reduce_solve  one workgroup: the partials in index order, the fixed columns dropped, S = D - G and its Cholesky factor in
//                        LDS (S and the inverse of the factor, 2 x 32 KiB, dynamic), the step, (S^-1)_cc and the four scalars the
//                        host reads.
//   k_sync_update        one thread per slot: the kept trial becomes the point, then dX = -L^-T (q_n + Q d); block 0 also moves the
//                        offsets.
//   k_sync_rows          one workgroup per camera over its rows (they are contiguous): the sum of squared residuals, the counts and,
//                        at the end, the compensated pixels; thread t adds its rows in ascending order, thread 0 the 256 sums.
//
// Chunk and workgroup size were not chosen by measurement: 256 slots is the block of the per-slot kernels, so a wave's partial of
// k_sync_build and a chunk of k_sync_gram cover whole blocks.  No kernel uses scratch.
//
// Null stream throughout: the launches of a call run in the order they were issued.  No floating-point atomics.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "time_offset_math.h"
#include "device_call.h"

using namespace cba;

namespace {

typedef double v4f64 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(SYNC_BLOCK)
k_sync_scatter(int64_t n_rows, int64_t n_traj, int64_t n_slots, const int32_t* __restrict__ row_cam, const int64_t* __restrict__ row_slot,
               const double* __restrict__ row_xy, const double* __restrict__ row_time, double* __restrict__ xy, double* __restrict__ ft) {
  const int64_t i = (int64_t)blockIdx.x * SYNC_BLOCK + threadIdx.x;
  if (i >= n_rows) return;
  traj_fill2d_row(n_rows, n_traj, n_slots, i, row_cam, row_slot, row_xy, row_time, 0, xy, ft);
}

__global__ void __launch_bounds__(SYNC_BLOCK)
k_sync_frame_time(int32_t n_cams, int64_t n_frames, int64_t n_traj, int64_t n_slots, const double* __restrict__ ft, double* __restrict__ frame_time) {
  const int64_t f = (int64_t)blockIdx.x * SYNC_BLOCK + threadIdx.x;
  if (f >= n_frames) return;
  frame_time[f] = traj_frame_mean(n_cams, n_traj, n_slots, f, ft);
}

__global__ void __launch_bounds__(SYNC_BLOCK)
k_sync_triangulate(int32_t n_cams, int64_t n_slots, const uint8_t* __restrict__ cam_posed, const int32_t* __restrict__ cam_model,
                   const double* __restrict__ cam_intr, const double* __restrict__ cam_P, const double* __restrict__ xy, int f32,
                   double* __restrict__ xyz, uint8_t* __restrict__ valid) {
  const int64_t s = (int64_t)blockIdx.x * SYNC_BLOCK + threadIdx.x;
  if (s >= n_slots) return;
  double p[3];
  const int views = traj_triangulate_slot(n_cams, n_slots, s, cam_posed, cam_model, cam_intr, cam_P, xy, f32, p);
  xyz[3 * s] = p[0];
  xyz[3 * s + 1] = p[1];
  xyz[3 * s + 2] = p[2];
  valid[s] = views >= 2 ? 1 : 0;
}

__global__ void __launch_bounds__(SYNC_BLOCK)
k_sync_velocity(int64_t n_frames, int64_t n_traj, int64_t n_slots, int gap, const uint8_t* __restrict__ valid, const double* __restrict__ X,
                const double* __restrict__ frame_time, double* __restrict__ V, uint8_t* __restrict__ moving) {
  const int64_t s = (int64_t)blockIdx.x * SYNC_BLOCK + threadIdx.x;
  if (s >= n_slots) return;
  sync_velocity_slot(n_frames, n_traj, s, gap, valid, X, frame_time, V, moving);
}

// the sum over the 64 lanes of a wave, the same tree on every lane
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// grid: ld / SYNC_BLOCK blocks, so that every wave is whole
__global__ void __launch_bounds__(SYNC_BLOCK)
k_sync_build(SyncBuildArgs A, double* __restrict__ Q, double* __restrict__ Lbuf, double* __restrict__ Fw, double* __restrict__ Dw, double* __restrict__ bw) {
  const int64_t s = (int64_t)blockIdx.x * SYNC_BLOCK + threadIdx.x;
  const int64_t wave = s >> 6;
  const bool first = (threadIdx.x & 63) == 0;
  const int32_t n_cols = A.n_cols;
  const double F = sync_build_slot(A, s, s < A.n_slots, Q, Lbuf, [&](int32_t col, double dc, double bc) {
    dc = wave_sum(dc);
    bc = wave_sum(bc);
    if (first) { Dw[wave * n_cols + col] = dc; bw[wave * n_cols + col] = bc; }
  });
  const double Fs = wave_sum(F);
  if (first) Fw[wave] = Fs;
}

// one depth slab of 16 slots into one tile: MFMA step m pairs the m-th of each lane's four doubles
__device__ __forceinline__ void gram_tile(bool on, int cb, int32_t n_cols, const double* __restrict__ Q, int64_t row, const double4& a, v4f64& acc) {
  if (!on) return;  // (uniform over the wave)
  const double4 b = cb < n_cols ? *reinterpret_cast<const double4*>(Q + row) : make_double4(0.0, 0.0, 0.0, 0.0);
  acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a.z, b.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a.w, b.w, acc, 0, 0, 0);
}

__device__ __forceinline__ void gram_store(bool on, double* __restrict__ out, int ti, int tj, int kq, int lr, const v4f64& acc) {
  if (!on) return;
  out[(ti * 16 + kq) * SYNC_LD + tj * 16 + lr] = acc[0];
  out[(ti * 16 + kq + 4) * SYNC_LD + tj * 16 + lr] = acc[1];
  out[(ti * 16 + kq + 8) * SYNC_LD + tj * 16 + lr] = acc[2];
  out[(ti * 16 + kq + 12) * SYNC_LD + tj * 16 + lr] = acc[3];
}

__global__ void __launch_bounds__(SYNC_BLOCK)
k_sync_gram(int32_t n_cols, int64_t ld, int64_t n_chunks, const double* __restrict__ Q, double* __restrict__ partial) {
  const int ti = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, kq = lane >> 4;
  const int nt = (n_cols + 15) >> 4;
  if (ti >= nt) return;  // (a whole wave; the kernel has no barrier)
  v4f64 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = acc0, acc2 = acc0, acc3 = acc0;
  const bool on0 = ti <= 0 && 0 < nt, on1 = ti <= 1 && 1 < nt, on2 = ti <= 2 && 2 < nt, on3 = ti <= 3 && 3 < nt;
  const int ca = ti * 16 + lr;
  for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    for (int k = 0; k < 3; ++k) {
      for (int step = 0; step < SYNC_GRAM_CHUNK / 16; ++step) {
        const int64_t s = chunk * SYNC_GRAM_CHUNK + step * 16 + 4 * kq;  // (< ld; the pad is zero)
        const double4 a = ca < n_cols ? *reinterpret_cast<const double4*>(Q + (3 * (int64_t)ca + k) * ld + s) : make_double4(0.0, 0.0, 0.0, 0.0);
        gram_tile(on0, lr, n_cols, Q, (3 * (int64_t)lr + k) * ld + s, a, acc0);
        gram_tile(on1, 16 + lr, n_cols, Q, (3 * (int64_t)(16 + lr) + k) * ld + s, a, acc1);
        gram_tile(on2, 32 + lr, n_cols, Q, (3 * (int64_t)(32 + lr) + k) * ld + s, a, acc2);
        gram_tile(on3, 48 + lr, n_cols, Q, (3 * (int64_t)(48 + lr) + k) * ld + s, a, acc3);
      }
    }
  }
  double* out = partial + (int64_t)blockIdx.x * SYNC_LD * SYNC_LD;
  gram_store(on0, out, ti, 0, kq, lr, acc0);
  gram_store(on1, out, ti, 1, kq, lr, acc1);
  gram_store(on2, out, ti, 2, kq, lr, acc2);
  gram_store(on3, out, ti, 3, kq, lr, acc3);
}

constexpr size_t SYNC_SOLVE_LDS = (2 * SYNC_LD * SYNC_LD + 3 * SYNC_LD) * sizeof(double) + (SYNC_LD + 2) * sizeof(int);

__global__ void __launch_bounds__(SYNC_BLOCK)
k_sync_reduce_solve(SyncSolveArgs A) {
  extern __shared__ __attribute__((aligned(16))) double sync_lds[];
  double* Sm = sync_lds;
  double* Ym = Sm + SYNC_LD * SYNC_LD;
  double* vec = Ym + SYNC_LD * SYNC_LD;
  int* idx = reinterpret_cast<int*>(vec + 3 * SYNC_LD);
  sync_reduce_solve((int)threadIdx.x, SYNC_BLOCK, A, Sm, Ym, vec, idx);
}

__global__ void __launch_bounds__(SYNC_BLOCK)
k_sync_update(int32_t n_cols, int32_t ref_col, int64_t n_slots, int64_t ld, const double* __restrict__ Q, const double* __restrict__ Lbuf,
              const double* __restrict__ dnew, double alpha, double max_offset, double* __restrict__ X0, double* __restrict__ dX, double* __restrict__ delta0,
              double* __restrict__ ddelta) {
  const int64_t s = (int64_t)blockIdx.x * SYNC_BLOCK + threadIdx.x;
  if (blockIdx.x == 0 && (int32_t)threadIdx.x < n_cols) sync_update_col((int32_t)threadIdx.x, alpha, max_offset, dnew, delta0, ddelta);
  if (s >= n_slots) return;
  sync_update_slot(n_cols, ref_col, ld, s, Q, Lbuf, dnew, alpha, X0, dX);
}

struct SyncRowArgs {
  int64_t n_traj;
  int32_t ref_col, min_rows;
  const int32_t* cam_col;
  const int64_t* cam_row_start;
  const int32_t* cam_model;
  const double* cam_intr;
  const double* cam_P;
  const int64_t* row_slot;
  const double* row_xy;
  const double* row_time;
  const double* frame_time;
  const uint8_t* valid;
  const uint8_t* moving;
  const double* X;
  const double* V;
  const double* delta0;
  double* out_xy;
  uint8_t* out_used;
  double* e2;         // [n_cams] of this pass
  int64_t* used;      // [n_cams] (first pass)
  uint8_t* free_col;  // [n_cols] (first pass)
};

template <bool FINAL>
__global__ void __launch_bounds__(SYNC_BLOCK)
k_sync_rows(SyncRowArgs A) {
  __shared__ double s_e2[SYNC_BLOCK];
  __shared__ int64_t s_used[SYNC_BLOCK], s_moves[SYNC_BLOCK];
  const int32_t c = blockIdx.x, col = A.cam_col[c];
  const int t = threadIdx.x;
  double e2 = 0.0;
  int64_t used = 0, moves = 0;
  for (int64_t i = A.cam_row_start[c] + t; i < A.cam_row_start[c + 1]; i += SYNC_BLOCK) {
    double e;
    int64_t u, m;
    sync_row(FINAL, i, c, col, A.n_traj, A.cam_model, A.cam_intr, A.cam_P, A.row_slot, A.row_xy, A.row_time, A.frame_time, A.valid, A.moving, A.X, A.V,
             A.delta0, A.out_xy, A.out_used, &e, &u, &m);
    e2 += e;
    used += u;
    moves += m;
  }
  s_e2[t] = e2;
  s_used[t] = used;
  s_moves[t] = moves;
  __syncthreads();
  if (t != 0) return;
  e2 = 0.0;
  used = moves = 0;
  for (int i = 0; i < SYNC_BLOCK; ++i) { e2 += s_e2[i]; used += s_used[i]; moves += s_moves[i]; }
  A.e2[c] = e2;
  if (!FINAL) {
    A.used[c] = used;
    if (col >= 0) A.free_col[col] = col != A.ref_col && moves >= (int64_t)A.min_rows ? 1 : 0;
  }
}

unsigned blocks(int64_t n) { return (unsigned)((n + SYNC_BLOCK - 1) / SYNC_BLOCK); }

// The device behind sync_drive: the buffers of the state and the launches of one evaluation.
struct DeviceBackend {
  Buffers& buf;
  const SyncPlan& plan;
  int32_t n_cams;
  int64_t n_frames, n_traj, n_slots;
  int gap;
  SyncBuildArgs B;
  SyncSolveArgs S;
  SyncRowArgs R;
  double *Q, *Lbuf, *X0, *dX, *V, *delta0, *ddelta, *e2_before, *e2_after;
  uint8_t* moving;

  bool good() {
    buf.check(hipGetLastError());
    return !buf.status();
  }
  bool velocity(bool first) {
    hipLaunchKernelGGL(k_sync_velocity, dim3(blocks(n_slots)), dim3(SYNC_BLOCK), 0, 0, n_frames, n_traj, n_slots, gap, B.valid, (const double*)X0,
                       B.frame_time, V, first ? moving : (uint8_t*)nullptr);
    return good();
  }
  bool rows(bool final) {
    R.e2 = final ? e2_after : e2_before;
    if (final) hipLaunchKernelGGL(k_sync_rows<true>, dim3((unsigned)n_cams), dim3(SYNC_BLOCK), 0, 0, R);
    else hipLaunchKernelGGL(k_sync_rows<false>, dim3((unsigned)n_cams), dim3(SYNC_BLOCK), 0, 0, R);
    return good();
  }
  bool eval(double alpha, SyncScalars& sc) {
    B.alpha = alpha;
    hipLaunchKernelGGL(k_sync_build, dim3((unsigned)plan.n_chunks), dim3(SYNC_BLOCK), 0, 0, B, Q, Lbuf, (double*)S.Fw, (double*)S.Dw, (double*)S.bw);
    hipLaunchKernelGGL(k_sync_gram, dim3((unsigned)plan.n_groups), dim3(SYNC_BLOCK), 0, 0, plan.n_cols, plan.ld, plan.n_chunks, (const double*)Q,
                       (double*)S.partial);
    hipLaunchKernelGGL(k_sync_reduce_solve, dim3(1), dim3(SYNC_BLOCK), SYNC_SOLVE_LDS, 0, S);
    if (!good()) return false;
    double h[4];
    buf.out(h, (const double*)S.scal, 4);  // (waits for the launches)
    sc.F = h[0]; sc.pred = h[1]; sc.step = h[2]; sc.ok = h[3];
    return !buf.status();
  }
  bool step(double alpha) {
    hipLaunchKernelGGL(k_sync_update, dim3(blocks(n_slots)), dim3(SYNC_BLOCK), 0, 0, plan.n_cols, plan.ref_col, n_slots, plan.ld, (const double*)Q,
                       (const double*)Lbuf, (const double*)S.dnew, alpha, plan.max_offset, X0, dX, delta0, ddelta);
    return good();
  }
  bool offsets(double* by_col) {
    buf.out(by_col, (const double*)delta0, plan.n_cols);
    return !buf.status();
  }
  bool set_offsets(const double* by_col) {
    if (!buf.status()) buf.check(hipMemcpy(delta0, by_col, (size_t)plan.n_cols * sizeof(double), hipMemcpyHostToDevice));
    return !buf.status();
  }
};

}  // namespace

extern "C" int cba_estimate_time_offsets(const cba_traj_desc* d, const cba_time_offset_options* o, int32_t device, cba_time_offset_out* out) {
  const char* what = "cba_estimate_time_offsets";
  if (!d || !o || !out) return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  // everything that does not need the device first
  SyncPlan plan;
  std::string msg;
  bool launch = false;
  int rc = sync_validate(d, o, (double)d->memory_limit, plan, msg, &launch);
  if (rc) return err(rc, msg);
  if (!launch) {
    sync_nothing(d, plan, out);
    return CBA_OK;
  }
  rc = select_device(device, what);
  if (rc) return rc;
  if (d->memory_limit <= 0) {
    size_t free_bytes = 0, total_bytes = 0;
    if (hipMemGetInfo(&free_bytes, &total_bytes) != hipSuccess) return err(CBA_ERR_HIP, std::string(what) + ": hipMemGetInfo failed");
    rc = sync_validate(d, o, (double)free_bytes, plan, msg, &launch);
    if (rc) return err(rc, msg);
  }
  const int32_t n_cams = d->n_cams, n_cols = plan.n_cols;
  const int64_t n_frames = d->n_frames, n_traj = d->n_traj, n_rows = d->n_rows, n_slots = n_frames * n_traj, ld = plan.ld;
  if (plan.n_chunks > (int64_t)0x7fffffff || n_rows > (int64_t)0x7fffffff * SYNC_BLOCK)
    return err(CBA_ERR_UNSUPPORTED, std::string(what) + ": more workgroups than one launch takes");

  Buffers buf;
  const uint8_t* dposed = buf.in(d->cam_posed, n_cams);
  const int32_t* dmodel = buf.in(d->cam_model, n_cams);
  const double* dintr = buf.in(d->cam_intr, n_cams, 9);
  const double* dP = buf.in(d->cam_P, n_cams, 12);
  const int32_t* dcol = buf.in(plan.cam_col.data(), n_cams);
  const int64_t* dstart = buf.in(plan.cam_row_start.data(), n_cams + 1);
  const int32_t* drcam = buf.in(d->row_cam, n_rows);
  const int64_t* drslot = buf.in(d->row_slot, n_rows);
  const double* drxy = buf.in(d->row_xy, n_rows, 2);
  const double* drt = buf.in(d->row_time, n_rows);
  double* dxy = buf.make<double>(n_cams, n_slots, 2);
  double* dft = buf.make<double>(n_cams, n_slots);
  double* dframe = buf.make<double>(n_frames);
  uint8_t* dvalid = buf.make<uint8_t>(n_slots);
  uint8_t* dmoving = buf.make<uint8_t>(n_slots);
  double* dX0 = buf.make<double>(n_slots, 3);
  double* ddX = buf.make<double>(n_slots, 3);
  double* dV = buf.make<double>(n_slots, 3);
  double* dL = buf.make<double>(6, ld);
  double* dQ = buf.make<double>(3 * (int64_t)n_cols, ld);
  double* dFw = buf.make<double>(plan.n_waves);
  double* dDw = buf.make<double>(plan.n_waves, n_cols);
  double* dbw = buf.make<double>(plan.n_waves, n_cols);
  double* dpartial = buf.make<double>(plan.n_groups, SYNC_LD, SYNC_LD);
  uint8_t* dfree = buf.make<uint8_t>(n_cols);
  double* ddelta0 = buf.make<double>(n_cols);
  double* dddelta = buf.make<double>(n_cols);
  double* ddnew = buf.make<double>(n_cols);
  double* dsinv = buf.make<double>(n_cols);
  double* dscal = buf.make<double>(4);
  double* de2b = buf.make<double>(n_cams);
  double* de2a = buf.make<double>(n_cams);
  int64_t* dused = buf.make<int64_t>(n_cams);
  double* doutxy = buf.make<double>(n_rows, 2);
  uint8_t* doutused = buf.make<uint8_t>(n_rows);
  if (buf.status()) return buf.result(what);

  // all bits set is a NaN: "no row here"; Q's pad beyond n_slots stays zero, as the state the first evaluation does not write
  const size_t cells = (size_t)n_cams * (size_t)n_slots;
  buf.check(hipMemsetAsync(dxy, 0xff, cells * 2 * sizeof(double), 0));
  if (!buf.status()) buf.check(hipMemsetAsync(dft, 0xff, cells * sizeof(double), 0));
  if (!buf.status()) buf.check(hipMemsetAsync(dQ, 0, (size_t)3 * n_cols * ld * sizeof(double), 0));
  if (!buf.status()) buf.check(hipMemsetAsync(ddX, 0, (size_t)n_slots * 3 * sizeof(double), 0));
  if (!buf.status()) buf.check(hipMemsetAsync(dV, 0, (size_t)n_slots * 3 * sizeof(double), 0));
  if (!buf.status()) buf.check(hipMemsetAsync(dfree, 0, (size_t)n_cols, 0));
  if (!buf.status()) buf.check(hipMemsetAsync(ddelta0, 0, (size_t)n_cols * sizeof(double), 0));
  if (!buf.status()) buf.check(hipMemsetAsync(dddelta, 0, (size_t)n_cols * sizeof(double), 0));
  if (!buf.status())
    buf.check(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sync_reduce_solve), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SYNC_SOLVE_LDS));
  if (buf.status()) return buf.result(what);
  hipLaunchKernelGGL(k_sync_scatter, dim3(blocks(n_rows)), dim3(SYNC_BLOCK), 0, 0, n_rows, n_traj, n_slots, drcam, drslot, drxy, drt, dxy, dft);
  hipLaunchKernelGGL(k_sync_frame_time, dim3(blocks(n_frames)), dim3(SYNC_BLOCK), 0, 0, n_cams, n_frames, n_traj, n_slots, (const double*)dft, dframe);
  hipLaunchKernelGGL(k_sync_triangulate, dim3(blocks(n_slots)), dim3(SYNC_BLOCK), 0, 0, n_cams, n_slots, dposed, dmodel, dintr, dP, (const double*)dxy,
                     d->float32_io ? 1 : 0, dX0, dvalid);

  DeviceBackend be{buf, plan, n_cams, n_frames, n_traj, n_slots, (int)o->max_neighbour_gap};
  be.B = SyncBuildArgs{n_cams, n_cols, plan.ref_col, n_slots, n_traj, ld, dcol, dmodel, dintr, dP, dxy, dft, dframe, dvalid, dX0, ddX, dV, ddelta0, dddelta,
                       0.0, plan.max_offset, o->huber_px};
  be.S = SyncSolveArgs{n_cols, plan.ref_col, plan.n_groups, plan.n_waves, dpartial, dFw, dDw, dbw, dfree, ddnew, dsinv, dscal};
  be.R = SyncRowArgs{n_traj, plan.ref_col, o->min_rows, dcol, dstart, dmodel, dintr, dP, drslot, drxy, drt, dframe, dvalid, dmoving, dX0, dV, ddelta0,
                     doutxy, doutused, de2b, dused, dfree};
  be.Q = dQ; be.Lbuf = dL; be.X0 = dX0; be.dX = ddX; be.V = dV; be.delta0 = ddelta0; be.ddelta = dddelta; be.e2_before = de2b; be.e2_after = de2a;
  be.moving = dmoving;
  int32_t rounds = 0;
  uint8_t converged = 0;
  double F_end = 0.0;
  if (!sync_drive(be, plan, n_rows, (int)o->max_rounds, &rounds, &converged, &F_end)) return buf.result(what);

  std::vector<double> delta((size_t)n_cols), sinv((size_t)n_cols), e2b((size_t)n_cams), e2a((size_t)n_cams);
  std::vector<uint8_t> free_col((size_t)n_cols), valid((size_t)n_slots);
  std::vector<int64_t> used((size_t)n_cams);
  buf.out(delta.data(), (const double*)ddelta0, n_cols);
  buf.out(sinv.data(), (const double*)dsinv, n_cols);
  buf.out(free_col.data(), (const uint8_t*)dfree, n_cols);
  buf.out(e2b.data(), (const double*)de2b, n_cams);
  buf.out(e2a.data(), (const double*)de2a, n_cams);
  buf.out(used.data(), (const int64_t*)dused, n_cams);
  buf.out(valid.data(), (const uint8_t*)dvalid, n_slots);
  buf.out(out->xyz, (const double*)dX0, n_slots, 3);
  buf.out(out->velocity, (const double*)dV, n_slots, 3);
  buf.out(out->frame_time, (const double*)dframe, n_frames);
  buf.out(out->row_xy, (const double*)doutxy, n_rows, 2);
  buf.out(out->row_used, (const uint8_t*)doutused, n_rows);
  if (!buf.status()) buf.check(hipDeviceSynchronize());
  if (buf.status()) return buf.result(what);
  int64_t n_points = 0;
  for (int64_t s = 0; s < n_slots; ++s) {
    n_points += valid[(size_t)s] ? 1 : 0;
    if (out->valid) out->valid[s] = valid[(size_t)s];
  }
  sync_report(d, plan, delta.data(), sinv.data(), free_col.data(), e2b.data(), e2a.data(), used.data(), n_points, F_end, out);
  if (out->rounds) *out->rounds = rounds;
  if (out->converged) *out->converged = converged;
  return CBA_OK;
}
