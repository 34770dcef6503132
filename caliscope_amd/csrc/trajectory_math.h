// The per-thread work and the host-side checks of cba_reconstruct_trajectories (include/caliscope_trajectory.h).  Compiled by hipcc
// into the kernels and the entry point of trajectory_lib.hip, and by g++ into tests/native/trajectory_harness.cpp, which runs the
// same routines in loops on the CPU.
//
// Grid.  slot s = f * n_traj + j; xy[c][s][2] and ft[c][s] hold NaN where camera c has no row; xyz[s][3], time[s] and valid[s] are
// the 3-D side.  valid: 0 nothing, 1 triangulated, 2 filled by the 3-D fill.
//
// Arithmetic.  The straight line of the two fills (traj_lerp) and the filter recurrence (traj_lfilter_step) are written in the order
// of pandas' / scipy's own arithmetic and compiled without contraction, so that hipcc and g++ return the bits of the host chain.
// traj_triangulate_slot is the body of k_triangulate (cba_kernels.h) over the grid, with the fused multiply-adds of that kernel's
// build written out (see there).
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/caliscope_trajectory.h"
#include "ba_math.h"

namespace cba {

constexpr int TRAJ_BLOCK = 256;  // threads of a workgroup, every kernel

CBA_HD double traj_nan() {
  const uint64_t bits = 0x7ff8000000000000ull;
  double v;
  __builtin_memcpy(&v, &bits, sizeof v);
  return v;
}

CBA_HD bool traj_is_nan(double v) { return v != v; }

// cell i (1..k) of a hole of which k cells are filled: k + 1 equal steps from the left neighbour to the right one
CBA_HD double traj_lerp(double left, double right, int64_t i, int64_t k) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double frac = (double)i / ((double)k + 1.0);
  const double step = (right - left) * frac;
  return left + step;
}

// k_traj_fill2d, row i: the row's own cell, then the hole between it and the next row of its track
CBA_HD void traj_fill2d_row(int64_t n_rows, int64_t n_traj, int64_t n_slots, int64_t i, const int32_t* row_cam, const int64_t* row_slot,
                            const double* row_xy, const double* row_time, int max_gap, double* xy, double* ft) {
  const int32_t c = row_cam[i];
  const int64_t s = row_slot[i], base = (int64_t)c * n_slots;
  const double x = row_xy[2 * i], y = row_xy[2 * i + 1], t = row_time[i];
  xy[2 * (base + s)] = x;
  xy[2 * (base + s) + 1] = y;
  ft[base + s] = t;
  if (max_gap <= 0 || i + 1 >= n_rows || row_cam[i + 1] != c) return;
  const int64_t s2 = row_slot[i + 1];
  if (s2 % n_traj != s % n_traj) return;
  const int64_t gap = (s2 - s) / n_traj - 1;  // the checks of the call made it >= 0
  if (gap <= 0) return;
  const int64_t k = gap < (int64_t)max_gap ? gap : (int64_t)max_gap;
  const double x2 = row_xy[2 * (i + 1)], y2 = row_xy[2 * (i + 1) + 1], t2 = row_time[i + 1];
  for (int64_t q = 1; q <= k; ++q) {
    const int64_t cell = base + s + q * n_traj;  // frame + q < frame of the next row <= n_frames - 1
    xy[2 * cell] = traj_lerp(x, x2, q, k);
    xy[2 * cell + 1] = traj_lerp(y, y2, q, k);
    ft[cell] = traj_lerp(t, t2, q, k);
  }
}

// k_traj_frame_time, frame f: mean of the times that are there, cameras ascending, trajectories ascending within a camera
CBA_HD double traj_frame_mean(int32_t n_cams, int64_t n_traj, int64_t n_slots, int64_t f, const double* ft) {
  double sum = 0.0;
  int64_t count = 0;
  for (int32_t c = 0; c < n_cams; ++c) {
    const double* row = ft + (int64_t)c * n_slots + f * n_traj;
    for (int64_t j = 0; j < n_traj; ++j) {
      const double v = row[j];
      if (!traj_is_nan(v)) { sum += v; ++count; }
    }
  }
  return count > 0 ? sum / (double)count : traj_nan();
}

// k_traj_triangulate, slot s: the loop of k_triangulate over the posed cameras that have a cell there.  Returns the views.
// k_triangulate is compiled with contraction, and which of the two products of r0 r0' + r1 r1' ends up inside the fused
// multiply-add is the compiler's choice per expression (it was not the same choice here as there).  So the rows and the sums are
// written out the way that kernel is compiled — r = fma(x, P2, -P0), M += fma(r0, r0', r1 r1') — and nothing else is contracted.
CBA_HD int traj_triangulate_slot(int32_t n_cams, int64_t n_slots, int64_t s, const uint8_t* cam_posed, const int32_t* cam_model,
                                 const double* cam_intr, const double* cam_P, const double* xy, int f32, double* out3) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double M[4][4];
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int r = 0; r < 4; ++r)
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int c = 0; c < 4; ++c) M[r][c] = 0.0;
  int views = 0;
  for (int32_t cam = 0; cam < n_cams; ++cam) {
    if (!cam_posed[cam]) continue;
    const int64_t cell = (int64_t)cam * n_slots + s;
    double x = xy[2 * cell], y = xy[2 * cell + 1];
    if (traj_is_nan(x)) continue;
    ++views;
    undistort_one(cam_model[cam], cam_intr + 9 * cam, x, y, f32, &x, &y);
    const double* P = cam_P + 12 * cam;
    double r0[4], r1[4];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int c = 0; c < 4; ++c) { r0[c] = fma(x, P[8 + c], -P[c]); r1[c] = fma(y, P[8 + c], -P[4 + c]); }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int r = 0; r < 4; ++r)
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int c = r; c < 4; ++c) {
        const double inner = r1[r] * r1[c];
        M[r][c] = M[r][c] + fma(r0[r], r0[c], inner);
      }
  }
  if (views < 2) { out3[0] = out3[1] = out3[2] = traj_nan(); return views; }
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int r = 1; r < 4; ++r)
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int c = 0; c < r; ++c) M[r][c] = M[c][r];
  double w[4];
  sym4_null_vector(M, w);
  out3[0] = w[0] / w[3];
  out3[1] = w[1] / w[3];
  out3[2] = w[2] / w[3];
  return views;
}

// k_traj_fill3d, slot s.  In place: a cell is an owner, a walk's end or a line's end only while valid == 1, and the kernel never
// gives or takes that value (filled cells get 2); only the owner of a hole writes inside it, and a walk stops at the first cell
// with valid == 1, so it never enters another owner's hole.  The walk ends at n_frames.
CBA_HD void traj_fill3d_cell(int64_t n_frames, int64_t n_traj, int64_t s, int max_gap, uint8_t* valid, double* xyz, double* time) {
  if (max_gap <= 0 || valid[s] != 1) return;
  const int64_t f = s / n_traj;
  int64_t r = f + 1;
  while (r < n_frames && valid[s + (r - f) * n_traj] != 1) ++r;
  if (r >= n_frames || r == f + 1) return;  // the trajectory ends here, or there is no hole
  const int64_t gap = r - f - 1, k = gap < (int64_t)max_gap ? gap : (int64_t)max_gap, right = s + (r - f) * n_traj;
  for (int64_t q = 1; q <= k; ++q) {
    const int64_t cell = s + q * n_traj;
    for (int d = 0; d < 3; ++d) xyz[3 * cell + d] = traj_lerp(xyz[3 * s + d], xyz[3 * right + d], q, k);
    time[cell] = traj_lerp(time[s], time[right], q, k);
    valid[cell] = 2;
  }
}

// One step of scipy's lfilter (direct form II transposed): y = z0 + b0 x; z_i = z_{i+1} + x b_{i+1} - y a_{i+1}; the last state
// without a successor.  b and a hold CBA_TRAJ_MAX_ORDER + 1 entries, z CBA_TRAJ_MAX_ORDER; fixed trip counts and selects keep the
// state in registers on the device.
CBA_HD double traj_lfilter_step(int order, const double* b, const double* a, double* z, double x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double y = z[0] + b[0] * x;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < CBA_TRAJ_MAX_ORDER; ++i) {
    const double xb = x * b[i + 1], ya = y * a[i + 1];
    const double next = z[i + 1 < CBA_TRAJ_MAX_ORDER ? i + 1 : i];  // (not read for the last state)
    const double mid = next + xb - ya, last = xb - ya;
    z[i] = i < order - 1 ? mid : (i == order - 1 ? last : z[i]);
  }
  return y;
}

CBA_HD double traj_odd_reflect(double end, double v) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double twice = 2.0 * end;
  return twice - v;
}

// k_traj_filtfilt, thread t = 3 j + coordinate of n_threads = 3 n_traj: scipy.signal.filtfilt(b, a, x) with its defaults over the
// cells of trajectory j that hold a point, in frame order.  buf: the thread's column of the scratch array, element e at
// buf[e * n_threads]; it takes the extended signal (n + 2 pad entries, pad = 3 (order + 1)) and is filtered in place, forward then
// backward.  n <= 3 order: nothing is done.  (n <= pad does not get here: the checks of the call refuse it.)
CBA_HD void traj_filtfilt_thread(int64_t n_frames, int64_t n_traj, int64_t t, int order, const double* b_in, const double* a_in,
                                 const double* zi_in, const uint8_t* valid, double* xyz, double* scratch) {
  const int64_t n_threads = 3 * n_traj, j = t / 3;
  const int64_t pad = 3 * ((int64_t)order + 1);
  double* buf = scratch + t;
  double* col = xyz + t;  // coordinate of frame f: col[f * n_threads]
  int64_t n = 0;
  for (int64_t f = 0; f < n_frames; ++f)
    if (valid[f * n_traj + j]) { buf[(pad + n) * n_threads] = col[f * n_threads]; ++n; }
  if (n <= 3 * (int64_t)order || n <= pad) return;
  double b[CBA_TRAJ_MAX_ORDER + 1], a[CBA_TRAJ_MAX_ORDER + 1], zi[CBA_TRAJ_MAX_ORDER], z[CBA_TRAJ_MAX_ORDER];
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i <= CBA_TRAJ_MAX_ORDER; ++i) { b[i] = i <= order ? b_in[i] : 0.0; a[i] = i <= order ? a_in[i] : 0.0; }
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < CBA_TRAJ_MAX_ORDER; ++i) zi[i] = i < order ? zi_in[i] : 0.0;
  // odd extension: 2 x[0] - x[pad], .., 2 x[0] - x[1] | x | 2 x[n-1] - x[n-2], .., 2 x[n-1] - x[n-1-pad]
  const double first = buf[pad * n_threads], last = buf[(pad + n - 1) * n_threads];
  for (int64_t e = 0; e < pad; ++e) {
    buf[e * n_threads] = traj_odd_reflect(first, buf[(pad + pad - e) * n_threads]);
    buf[(pad + n + e) * n_threads] = traj_odd_reflect(last, buf[(pad + n - 2 - e) * n_threads]);
  }
  const int64_t m = n + 2 * pad;
  {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double x0 = buf[0];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < CBA_TRAJ_MAX_ORDER; ++i) z[i] = zi[i] * x0;
  }
  for (int64_t e = 0; e < m; ++e) buf[e * n_threads] = traj_lfilter_step(order, b, a, z, buf[e * n_threads]);
  {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double y0 = buf[(m - 1) * n_threads];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < CBA_TRAJ_MAX_ORDER; ++i) z[i] = zi[i] * y0;
  }
  for (int64_t e = m - 1; e >= 0; --e) buf[e * n_threads] = traj_lfilter_step(order, b, a, z, buf[e * n_threads]);
  int64_t q = 0;
  for (int64_t f = 0; f < n_frames; ++f)
    if (valid[f * n_traj + j]) { col[f * n_threads] = buf[(pad + q) * n_threads]; ++q; }
}

}  // namespace cba

// ---- host side: sizes and the checks of a call -----------------------------------------------------------------------------------
#include <string>
#include <vector>

namespace cba {

inline int64_t traj_pad(int order) { return 3 * ((int64_t)order + 1); }

// bytes of the device buffers of a call
inline double traj_device_bytes(const cba_traj_desc* d) {
  const double slots = (double)d->n_frames * (double)d->n_traj, cams = (double)d->n_cams;
  double bytes = cams * slots * 24.0 + slots * 33.0 + (double)d->n_frames * 8.0 + (double)d->n_rows * 36.0 + cams * 200.0;
  if (d->filter_b) bytes += ((double)d->n_frames + 2.0 * (double)traj_pad(d->filter_order)) * (double)d->n_traj * 24.0;
  return bytes;
}

// Cells per trajectory that reach the filter, from the rows alone: posed views per slot after the 2-D fill, slots with two or more,
// and what the 3-D fill adds between them.  Returns the first trajectory with 3 order < n <= 3 (order + 1), or -1.
inline int64_t traj_unfilterable(const cba_traj_desc* d, int64_t* n_found) {
  const int64_t n_traj = d->n_traj, n_slots = d->n_frames * n_traj;
  std::vector<uint8_t> views((size_t)n_slots, 0);
  const auto bump = [&](int64_t s) { if (views[(size_t)s] < 2) ++views[(size_t)s]; };
  for (int64_t i = 0; i < d->n_rows; ++i) {
    const int32_t c = d->row_cam[i];
    if (!d->cam_posed[c]) continue;
    const int64_t s = d->row_slot[i];
    bump(s);
    if (d->xy_gap <= 0 || i + 1 >= d->n_rows || d->row_cam[i + 1] != c) continue;
    const int64_t s2 = d->row_slot[i + 1];
    if (s2 % n_traj != s % n_traj) continue;
    const int64_t gap = (s2 - s) / n_traj - 1, k = gap < (int64_t)d->xy_gap ? gap : (int64_t)d->xy_gap;
    for (int64_t q = 1; q <= k; ++q) bump(s + q * n_traj);
  }
  std::vector<int64_t> count((size_t)n_traj, 0), last((size_t)n_traj, -1);
  for (int64_t f = 0; f < d->n_frames; ++f)
    for (int64_t j = 0; j < n_traj; ++j) {
      if (views[(size_t)(f * n_traj + j)] < 2) continue;
      if (last[(size_t)j] >= 0 && d->xyz_gap > 0) {
        const int64_t gap = f - last[(size_t)j] - 1;
        count[(size_t)j] += gap < (int64_t)d->xyz_gap ? gap : (int64_t)d->xyz_gap;
      }
      ++count[(size_t)j];
      last[(size_t)j] = f;
    }
  for (int64_t j = 0; j < n_traj; ++j)
    if (count[(size_t)j] > 3 * (int64_t)d->filter_order && count[(size_t)j] <= traj_pad(d->filter_order)) { *n_found = count[(size_t)j]; return j; }
  return -1;
}

// 0, or the negative code the call returns with `msg` set (-1 CBA_ERR_INVALID, -4 CBA_ERR_UNSUPPORTED).  memory: bytes the buffers
// may take, <= 0: not checked.
inline int traj_validate(const cba_traj_desc* d, double memory, std::string& msg) {
  const std::string what = "cba_reconstruct_trajectories: ";
  if (!d) { msg = what + "null argument"; return -1; }
  if (d->n_cams < 0 || d->n_frames < 0 || d->n_traj < 0 || d->n_rows < 0) { msg = what + "negative size"; return -1; }
  if (d->filter_b) {
    if (d->filter_order < 1 || d->filter_order > CBA_TRAJ_MAX_ORDER) {
      msg = what + "filter order " + std::to_string(d->filter_order) + " outside 1.." + std::to_string(CBA_TRAJ_MAX_ORDER);
      return -4;
    }
    if (!d->filter_a || !d->filter_zi) { msg = what + "null argument"; return -1; }
    if (d->filter_a[0] != 1.0) { msg = what + "filter_a[0] must be 1"; return -1; }
  }
  if (d->n_rows == 0) return 0;
  if (d->n_cams == 0 || d->n_frames == 0 || d->n_traj == 0) { msg = what + "rows without a grid"; return -1; }
  if (!d->row_cam || !d->row_slot || !d->row_xy || !d->row_time || !d->cam_posed || !d->cam_model || !d->cam_intr || !d->cam_P) {
    msg = what + "null argument";
    return -1;
  }
  if ((double)d->n_frames * (double)d->n_traj * (double)d->n_cams >= 9.0e15) { msg = what + "grid too large to index"; return -4; }
  for (int32_t c = 0; c < d->n_cams; ++c)
    if (d->cam_posed[c] && d->cam_model[c] != 0 && d->cam_model[c] != 1) {
      msg = what + "camera " + std::to_string(c) + ": unknown model " + std::to_string(d->cam_model[c]);
      return -1;
    }
  const int64_t n_traj = d->n_traj, n_slots = d->n_frames * n_traj;
  const auto where = [&](int64_t i) { return what + "row " + std::to_string(i) + ": "; };
  for (int64_t i = 0; i < d->n_rows; ++i) {
    const int32_t c = d->row_cam[i];
    const int64_t s = d->row_slot[i];
    if (c < 0 || c >= d->n_cams) { msg = where(i) + "camera " + std::to_string(c) + " out of range [0, " + std::to_string(d->n_cams) + ")"; return -1; }
    if (s < 0 || s >= n_slots) { msg = where(i) + "slot " + std::to_string(s) + " out of range [0, " + std::to_string(n_slots) + ")"; return -1; }
    if (!std::isfinite(d->row_xy[2 * i]) || !std::isfinite(d->row_xy[2 * i + 1])) { msg = where(i) + "pixel is not finite"; return -1; }
    if (i == 0) continue;
    const int32_t c0 = d->row_cam[i - 1];
    const int64_t s0 = d->row_slot[i - 1], j0 = s0 % n_traj, j = s % n_traj;
    if (c0 == c && s0 == s) { msg = where(i) + "duplicate of row " + std::to_string(i - 1) + " (same camera, frame and trajectory)"; return -1; }
    if (c0 > c || (c0 == c && (j0 > j || (j0 == j && s0 > s)))) { msg = where(i) + "rows are not sorted by (camera, trajectory, frame)"; return -1; }
  }
  if (memory > 0.0 && traj_device_bytes(d) > memory) {
    msg = what + "the grid of " + std::to_string(d->n_cams) + " cameras x " + std::to_string(d->n_frames) + " frames x " + std::to_string(n_traj) +
          " trajectories needs " + std::to_string((long long)traj_device_bytes(d)) + " bytes of device memory, " + std::to_string((long long)memory) +
          " are available";
    return -4;
  }
  if (d->filter_b) {
    int64_t n = 0;
    const int64_t j = traj_unfilterable(d, &n);
    if (j >= 0) {
      msg = what + "trajectory " + std::to_string(j) + " has " + std::to_string(n) + " samples: the order-" + std::to_string(d->filter_order) +
            " filter needs more than " + std::to_string(traj_pad(d->filter_order)) + " (or at most " + std::to_string(3 * d->filter_order) +
            ", which are left unfiltered)";
      return -1;
    }
  }
  return 0;
}

}  // namespace cba
