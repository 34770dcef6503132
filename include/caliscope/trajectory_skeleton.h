/* caliscope/trajectory_skeleton.h — C ABI of the skeleton adjustment of reconstructed trajectories in libcaliscope_ba.so
 * (caliscope_amd/csrc/skeleton_lib.hip, caliscope_amd/csrc/trajectory_skeleton_math.h).
 *
 * cba_reconstruct_trajectories_uncertain (trajectory_uncertainty.h) gives every sample its 3 x 3 covariance, and every stage up to
 * there treats a landmark on its own.  The landmarks of one subject sit on a skeleton whose segments do not change length: a sample
 * that is 1 mm wide across and 3 cm deep is pulled to its neighbour along exactly the weak direction once the segment between them
 * is known to a few millimetres.  k_skel_length estimates the length of every segment over the recording, k_skel_adjust adjusts the
 * points of every frame to them, weighted by their covariances.  The result is a table and a covariance that cba_smooth_trajectories
 * (trajectory_smoother.h) takes as they are.  There is no CPU fallback.  The symbols are bound by
 * caliscope_amd/trajectory_skeleton.py.
 *
 * Inputs.  xyz, meas_cov and measured of cba_smooth_desc (Z_i, R_i of slot s = f n_traj + j); n_seg segments, segment s between the
 * trajectories seg_traj[s] = (a, b); seg_length[s], NaN: estimate it; seg_sigma[s] > 0, how rigid the segment is, world units.
 *
 * Components.  The connected components of the graph of the segments over the trajectories, numbered by their smallest trajectory;
 * a trajectory in no segment belongs to none (-1).  A component of more than CBA_SKELETON_MAX_POINTS = 54 trajectories is refused
 * (its packed triangle, 3 m (3 m + 1) / 2 doubles, is factored in the LDS of one workgroup, as k_unc_component's).
 *
 * Lengths (k_skel_length, one workgroup per segment).  Over the frames where both ends are measured d_f = |Z_a - Z_b|, n of them.
 *     med    the lower median of the d_f: the element of rank floor((n - 1) / 2) in ascending order, by a radix select over the bit
 *            patterns of the (non-negative) doubles, 8 bits a pass; exact, whatever the order of the counting
 *     mad    the lower median of |d_f - med|, by the same select
 *     length given: seg_length[s] as it is.  Otherwise the inverse-variance mean sum(d_f / v_f) / sum(1 / v_f) over the frames with
 *            |d_f - med| <= trim 1.4826 mad (mad == 0: over the frames with d_f == med), v_f = u^T (R_a + R_b) u, u the unit vector
 *            of the segment in the frame (coincident ends: u = 0, v_f = tr(R_a + R_b) / 3, so that the frame keeps a finite weight).
 *            The sums run in a fixed order: lane t of 256 adds the frames t, t + 256, .. in ascending order, lane 0 then adds the
 *            256 partial sums in ascending order.
 *     frames n.  n == 0 and no given length: length, med and mad are NaN and the segment is inactive in every frame.
 *
 * Adjustment (k_skel_adjust, one workgroup per (frame, component)).  A segment is active in a frame when both ends are measured
 * there and its length L_s is finite.  The unknowns are the measured points of the component with at least one active segment, m_f
 * of them, in ascending order of their trajectories.  With e_i = X_i - Z_i,
 *     F(X) = sum_i e_i^T R_i^-1 e_i + sum_active ((|X_a - X_b| - L_s) / sigma_s)^2
 * is minimised from X = Z by Levenberg-Marquardt on the Gauss-Newton matrix
 *     N = blockdiag(R_i^-1) + sum_s sigma_s^-2 (e_a - e_b)(e_a - e_b)^T (x) u_s u_s^T,    g = grad F / 2
 * (e_a the index vector of point a; u_s the unit vector from b to a, 0 for coincident ends: the solver's subgradient).
 *     schedule   lambda = 0 at the start.  An iteration assembles N and g at X, adds lambda diag(N) to the diagonal, factors
 *                (Cholesky, pivots by cov_con_pivot_ok), solves delta = -(N + lambda D)^-1 g and evaluates F(X + delta).  The step
 *                "lowers F" when F(X + delta) <= F(X), or, for a step too short for F to tell, when -g^T delta <= rho (1 + F)
 *                and F(X + delta) <= F(X) + rho (1 + F), rho = 1e-10: with coordinates of metres, noise of a millimetre and
 *                covariances of condition 10^2 to 10^3 the digits of F end near 10^-13 of it, so close to the minimum the
 *                change a step predicts is below what F resolves and a rise of that size is rounding, not a rise.  A step that
 *                lowers F is accepted: X += delta, lambda <- lambda / 10, and 0 once below 1e-4.  Otherwise, or when a damped
 *                pivot fails, lambda <- 1e-4 from 0 and 10 lambda from anything else, and X stays.
 *     end        after an accepted undamped step (lambda = 0) with -g^T delta <= tol^2: converged, status 1; the decrement of a
 *                damped step does not bound the distance left, so such a step never ends the loop.  After max_iter
 *                factorisations: the last accepted iterate, which is the best one, status 2.
 *     covariance one undamped factorisation at the result, inverted in place (X = L^-1): the covariance of point i is
 *                [N^-1]_ii = (X^T X)_ii (cov_tri_gram).  An undamped pivot that fails cov_con_pivot_ok: status 3, and the slots of
 *                the component pass through in that frame.
 * Assembly without atomics: a thread per point sums R_i^-1 and the blocks of its incident segments in the order of a list the host
 * uploads (ascending segment index); a thread per segment owns its off-diagonal block.  Sums over points (F, g^T delta) are partial
 * per point and added by one thread in ascending order.  Every branch on a pivot or on acceptance is uniform.
 *
 * Limits.  The adjustment correlates the points of a frame; the cross-covariances are not returned.  There is no robust loss and
 * no gating on the segment rows: w_before reports a mistracked end and nothing removes it.  No joint-angle limits, nothing through
 * time: the smoother follows.  F has several minima when the noise is comparable with a segment's length; the one reached from Z is
 * returned.
 *
 * The result is the same bits from run to run: no floating-point atomics, fixed orders throughout.
 */
#ifndef CALISCOPE_TRAJECTORY_SKELETON_H
#define CALISCOPE_TRAJECTORY_SKELETON_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CBA_SKELETON_MAX_POINTS 54

typedef struct {
  int64_t n_frames;
  int64_t n_traj;            /* n_slots = n_frames n_traj, slot s = f n_traj + j */
  const double* xyz;         /* [n_slots][3]; read where measured */
  const double* meas_cov;    /* [n_slots][6] xx xy xz yy yz zz; read where measured */
  const uint8_t* measured;   /* [n_slots] 1: measured; anything else: not */
  int64_t n_seg;
  const int32_t* seg_traj;   /* [n_seg][2] */
  const double* seg_length;  /* [n_seg]; NaN: estimated */
  const double* seg_sigma;   /* [n_seg] > 0 */
  double trim;               /* > 0, in robust standard deviations (1.4826 mad) */
  int32_t max_iter;          /* >= 1 factorisations per (frame, component) */
  double tol;                /* > 0: converged when -g^T delta <= tol^2 */
  int64_t memory_limit;      /* bytes the device buffers may take; 0: the free device memory */
} cba_skeleton_desc;

/* Every pointer may be NULL.  n_comp is what cba_skeleton_components returns.
 * Slot status: 0 unmeasured (NaN); 1 adjusted; 2 measured with nothing active (the input's bytes); 3 passed through because its
 * component failed in that frame (the input's bytes).
 * Component status: 0 nothing active in the frame (chi2 0, rows 0, iterations 0); 1 converged; 2 max_iter reached; 3 failed. */
typedef struct {
  double* pos;          /* [n_slots][3] */
  double* pos_cov;      /* [n_slots][6] */
  uint8_t* status;      /* [n_slots] */
  double* length;       /* [n_seg] the length in use */
  double* med;          /* [n_seg] */
  double* mad;          /* [n_seg] */
  int64_t* frames;      /* [n_seg] co-measured frames */
  double* len_before;   /* [n_frames][n_seg] |Z_a - Z_b|; NaN where the segment is inactive, as the next two */
  double* w_before;     /* [n_frames][n_seg] (d - L) / sqrt(sigma_s^2 + u^T (R_a + R_b) u) */
  double* len_after;    /* [n_frames][n_seg] (status 3: len_before) */
  double* chi2;         /* [n_frames][n_comp] F at the result (status 3: F at Z) */
  int32_t* rows;        /* [n_frames][n_comp] active segments: the expectation of chi2 */
  int32_t* iterations;  /* [n_frames][n_comp] factorisations, the undamped last one not counted */
  uint8_t* comp_status; /* [n_frames][n_comp] */
} cba_skeleton_out;

/* Host code only, no device: the component of every trajectory (traj_comp[n_traj], -1: in no segment).  Returns n_comp >= 0, or
 * CBA_ERR_INVALID (a null argument, a negative size, a segment index out of range, a self segment, a repeated pair) or
 * CBA_ERR_UNSUPPORTED (a component of more than 54 trajectories, its first trajectory named).  Reads n_traj, n_seg and seg_traj. */
int64_t cba_skeleton_components(const cba_skeleton_desc* desc, int32_t* traj_comp);

/* Host checks before any launch, the offender named.  CBA_ERR_INVALID: a null desc or out, a negative size, a null input with
 * something to read; those of cba_skeleton_components; seg_sigma, trim or tol not finite and positive; max_iter < 1; a given length
 * not finite and positive; a measured slot whose point or covariance is not finite, or whose covariance fails chol3.
 * CBA_ERR_UNSUPPORTED: a component too large; the device buffers exceed memory_limit: 154 bytes per slot (xyz 24, meas_cov 48,
 * measured 1; pos 24, pos_cov 48, status 1; the trajectory's component 4 and place 4 per trajectory are not counted), 32 per
 * (frame, segment) (len_before, w_before, len_after; the distances of the select), 17 per (frame, component) (chi2 8, rows 4,
 * iterations 4, status 1).  n_slots == 0, n_seg == 0 or no measured slot succeeds without a launch: the slots pass through
 * (status 2 where measured), the rest is NaN / 0 and a given length is reported as given. */
int cba_adjust_skeleton(const cba_skeleton_desc* desc, int32_t device, cba_skeleton_out* out);

#ifdef __cplusplus
}
#endif

#endif /* CALISCOPE_TRAJECTORY_SKELETON_H */
