/* caliscope/time_offsets.h — C ABI of the per-camera time offsets of a recording in libcaliscope_ba.so
 * (caliscope_amd/csrc/time_offset_lib.hip, caliscope_amd/csrc/time_offset_math.h).
 *
 * Every stage after calibration takes the rows of one sync_index as exposed at one instant.  Unsynchronised cameras keep two timing
 * errors after the grouping: a constant latency of each camera, which the timestamps do not show, and the spread of the timestamps
 * inside a group, which they show and which nothing used.  cba_estimate_time_offsets estimates the first, accounts for both, and
 * returns the trajectories at the nominal frame times together with, for every input row, the pixel its camera would have seen at
 * the nominal time.  The grid is that of cba_reconstruct_trajectories (caliscope_trajectory.h: cba_traj_desc, slot s = f n_traj + j).
 * There is no CPU fallback.  The symbol is bound by caliscope_amd/time_offsets.py.
 *
 * Model.
 *     tau_f    the nominal time of frame f: the fixed-order mean of the row times of the frame (k_traj_frame_time).
 *     lag      row (c, f, j) was exposed at row_time + delta_c: its lag against the slot is s = row_time - tau_f + delta_c.
 *     motion   near tau_f the landmark moves at constant velocity, X_j(tau_f + s) = X_fj + V_fj s.
 *     V_fj     the central difference of the previous round's positions at the nearest slot with a point before and after frame
 *              f, both within max_neighbour_gap frames, over the difference of their tau.  A slot without both has V = 0: its rows
 *              determine its point and drop out of the offset equations by themselves.
 *     cost     F(X, delta) = 1/2 sum rho(|u - pi_c(X_fj + V_fj s)|^2) over the rows of posed cameras in slots with a point (two or
 *              more such rows).  rho is linear, or Huber: huber_px = k > 0 gives every row the weight w = min(1, k / |r|),
 *              recomputed at each evaluation (IRLS), and rho = |r|^2 inside k, 2 k |r| - k^2 outside.
 *     gauge    delta_ref = 0 for the reference camera (reference_cam, -1: the lowest posed camera with rows).
 *     limit    There is no acceleration term: the model error of a row is 1/2 a s^2 for the acceleration a of its landmark.  It is
 *              not estimated and not reported; on curved motion it biases the offsets by the part of it that correlates with V.
 *     bound    |delta_c| <= max_offset (seconds; 0: one median interval of the tau_f of the frames with rows).  An iterate that
 *              reaches it is clamped there and its camera gets the status CBA_OFFSET_AT_LIMIT.  Whole-frame misalignment is the
 *              sync mapping's job, not this call's.
 *
 * Algorithm.  Start from the plain DLT triangulation of the grid (traj_triangulate_slot; no 2-D hole filling), delta = 0.  The
 * synchronous start is the DLT points taken to the minimum of F with V = 0 and every offset fixed, by the iteration below: the DLT
 * minimises an algebraic error on undistorted points, and a V differenced from it would carry that into every later round.  A
 * round freezes V from the current positions and runs Gauss-Newton on (X, delta) jointly:
 *     per slot   H = sum w B^T B (3 x 3), g = sum w B^T r, with B = d pi_c / dX at X + V s and r = pi_c(X + V s) - u
 *     per view   a_c = B_c V (d r / d delta_c), E_c = w B_c^T a_c, d_c = w a_c^T a_c, b_c = w a_c^T r
 *     reduced    S = diag(sum d_c) - sum_slots E^T H^-1 E, rhs = sum b_c - sum E_c^T H^-1 g over the cameras.  With H = L L^T,
 *                q_c = L^-1 E_c and q_n = L^-1 g, S = D - Q^T Q and rhs = b - Q^T q_n: one Gram matrix of a (3 n_slots) x n_posed
 *                array, q_n in the column of the reference camera, whose own column nothing needs.
 *     fixed      the row and column of the reference camera and of every camera with fewer than min_rows rows in slots with
 *                V != 0 are removed; such a camera is CBA_OFFSET_UNDETERMINED, its offset is held at 0 and reported as NaN, as
 *                its sigma.  The set is decided once, with the V of the first round, and kept for the call.
 *     step       S d = -rhs by Cholesky; dX = -L^-T (q_n + sum q_c d_c) per slot.
 *     safeguard  step halving: the trial point (X, delta) + alpha (dX, d), alpha = 1, is evaluated; it is kept when
 *                F(trial) <= F + 1e-10 (1 + F), that is unless it raises F beyond what F resolves; otherwise alpha is halved and
 *                the trial repeated, at most 10 times, after which the round ends at the point it has.  A round also ends after
 *                a kept step whose predicted decrease 1/2 (q_n^T q_n + d^T S d) is at most 1e-18 px^2 per row, and after
 *                CBA_OFFSET_MAX_INNER evaluations.
 *     rounds     stop when max_c |delta_c - delta_c of the round before| < tol (seconds; 0: 1e-6 of the median interval): converged;
 *                or after max_rounds.  An offset that ends below tol in size is not told from zero by this criterion and is set to
 *                zero: the rows of cameras that are synchronous come back bit for bit.
 *     report     sigma0^2 = 2 F / (2 rows - 3 slots - free cameras) at the end, offset_sigma_c = sigma0 sqrt((S^-1)_cc) with S at
 *                the end, the RMS reprojection error per camera at the synchronous start (its points, no lags) and at the end,
 *                the rows in use per camera, the rounds taken and the converged flag.
 *     pixels     the compensated pixel of a row in use is u - (pi_c(X + V s) - pi_c(X)) at the end; a row of an unposed camera or of
 *                a slot without a point keeps its pixel and is marked unused.
 *
 * Device (time_offset_lib.hip): k_sync_velocity and k_sync_build one thread per slot, k_sync_gram the Gram matrix with
 * v_mfma_f64_16x16x4 in a 4 x 4 grid of 16 x 16 tiles, one partial per workgroup, k_sync_reduce_solve one workgroup,
 * k_sync_update one thread per slot, k_sync_rows one workgroup per camera.  No floating-point atomics and every sum in a fixed
 * order: two calls on one input return the same bytes.  Null stream, launches in issue order.  Per evaluation the host reads four
 * doubles, per round the offsets.
 *
 * Refusals, before any launch, with the offender named.  CBA_ERR_INVALID: what cba_reconstruct_trajectories refuses; a row_time that
 * is not finite; tau_f that do not increase strictly over the frames with rows; a reference camera out of range, unposed or without
 * rows; an option that is not finite, is negative, or (max_neighbour_gap, min_rows, max_rounds) is below 1; xy_gap, xyz_gap or a filter
 * in the descriptor.  CBA_ERR_UNSUPPORTED: more than CBA_OFFSET_MAX_CAMS = 64 posed cameras (the Gram accumulator is the 4 x 4 tile
 * grid, S and the inverse of its factor take 2 x 32 KiB of LDS); buffers beyond memory_limit.  n_rows == 0, or no posed camera with
 * rows, succeeds without a launch: every camera status 0, NaN offsets, no points.
 */
#ifndef CALISCOPE_TIME_OFFSETS_H
#define CALISCOPE_TIME_OFFSETS_H

#include <stdint.h>

#include "../caliscope_trajectory.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CBA_OFFSET_MAX_CAMS 64  /* posed cameras */
#define CBA_OFFSET_MAX_INNER 30 /* evaluations of a round */

/* status of a camera */
#define CBA_OFFSET_NONE 0         /* unposed, or posed without a row in use */
#define CBA_OFFSET_REFERENCE 1    /* offset 0 by the gauge, sigma 0 */
#define CBA_OFFSET_ESTIMATED 2
#define CBA_OFFSET_AT_LIMIT 3     /* estimated, and clamped at +-max_offset */
#define CBA_OFFSET_UNDETERMINED 4 /* fewer than min_rows rows in moving slots: held at 0, reported as NaN */

typedef struct {
  int32_t reference_cam;     /* index into the cameras of the descriptor; -1: the lowest posed camera with rows */
  int32_t max_neighbour_gap; /* frames, >= 1 */
  int32_t min_rows;          /* >= 1 */
  int32_t max_rounds;        /* >= 1 */
  double huber_px;           /* 0: linear loss */
  double max_offset;         /* seconds; 0: one median frame interval */
  double tol;                /* seconds; 0: 1e-6 of the median frame interval */
} cba_time_offset_options;

/* Every pointer may be NULL: that output is not returned. */
typedef struct {
  double* offsets;     /* [n_cams] seconds; NaN: status 0 or 4 */
  double* sigma;       /* [n_cams] */
  uint8_t* status;     /* [n_cams] CBA_OFFSET_* */
  double* rms_before;  /* [n_cams] px over the rows in use at the synchronous start; NaN without rows in use */
  double* rms_after;   /* [n_cams] */
  int64_t* rows;       /* [n_cams] rows in use */
  double* sigma0_px;   /* [1] NaN without redundancy */
  int32_t* rounds;     /* [1] */
  uint8_t* converged;  /* [1] */
  double* xyz;         /* [n_slots][3] at tau_f; NaN where valid == 0 */
  uint8_t* valid;      /* [n_slots] 1: a point */
  double* velocity;    /* [n_slots][3] the V of the last round; 0 where there is none */
  double* frame_time;  /* [n_frames] tau_f; NaN: no row */
  double* row_xy;      /* [n_rows][2] compensated pixels, in the order of the rows */
  uint8_t* row_used;   /* [n_rows] */
} cba_time_offset_out;

int cba_estimate_time_offsets(const cba_traj_desc* d, const cba_time_offset_options* options, int32_t device, cba_time_offset_out* out);

#ifdef __cplusplus
}
#endif

#endif /* CALISCOPE_TIME_OFFSETS_H */
