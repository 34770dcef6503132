/* caliscope/trajectory_refine.h — C ABI of the trajectory reconstruction with robust reprojection refinement in libcaliscope_ba.so
 * (caliscope_amd/csrc/trajectory_lib.hip, caliscope_amd/csrc/trajectory_refine_math.h).
 *
 * cba_reconstruct_trajectories (../caliscope_trajectory.h) leaves in every slot the DLT point: the null vector of a 4 x 4 matrix of
 * undistorted image points, all views weighted alike.  That point minimises an algebraic error; one mistracked landmark in one
 * camera drags it by centimetres, and nothing is said about its quality.  This call puts one kernel, k_traj_refine, between the
 * triangulation and the 3-D fill: it minimises the pixel reprojection error of every slot under a robust loss, drops the views that
 * still contradict the point, and reports the views and the reprojection error per slot.  The 3-D fill and the filter run on the
 * refined points.  Conventions, data model, checks and the other launches are those of caliscope_trajectory.h; there is no CPU
 * fallback.  The symbol is bound by caliscope_amd/trajectory_refinement.py.
 *
 * Mathematics.  A slot is refined when valid == 1 after k_traj_triangulate.  Its active views are the posed cameras with a cell
 * there (cells of the 2-D fill count, as they do for the DLT); the start X0 is the DLT point.  The residual of view c, in pixels,
 * goes through the forward model (no undistortion):
 *     e_c(X) = (cx + fx xd - u,  cy + fy yd - v),   (xd, yd) = lens((R X + t)_xy / (R X + t)_z),
 * [R | t] of cam_P, fx fy cx cy and the distortion of cam_intr, lens = lens_pinhole / lens_fisheye of ba_math.h, (u, v) the FP64 cell
 * of the grid (float32_io acts through the start point only).  The objective is scipy's,
 *     F(X) = 1/2 sum_c sum_{k=0,1} s^2 rho(e_ck^2 / s^2),   s = f_scale in pixels,
 * every scalar residual with a rho of its own (robust_one of ba_math.h: linear, huber, soft_l1, cauchy, arctan).  It is minimised by
 * Levenberg-Marquardt on the three coordinates.  scipy's treatment of a scalar residual (row scale sqrt(rho' + 2 rho'' e^2) floored
 * at 2^-52, residual e rho' / that root) gives F and the gradient g = sum J_k^T rho' e_k as scipy has them, so the minimiser is
 * scipy's; the rows of H = sum rho' J_k^T J_k are weighted by rho' alone (iteratively reweighted least squares).  scipy's
 * second-order term takes all of rho' away where the loss is linear in |e| — at a DLT point that an outlier has dragged off that is
 * every row, H = 2^-52 J^T J, and eighteen steps are refused before lambda has caught up; with rho' the full step of a linear model never
 * increases F for a loss that is concave in e^2.  H (6 numbers), g (3), F and the per-view distances are added up in ONE pass over the cameras,
 * ascending; then (H + lambda diag H) delta = -g by chol3, and the pass again at X + delta.
 *
 *     lambda            1e-3 at the start of every round; x 0.1 after an accepted step (not below 1e-15), x 10 after a refused one
 *     accepted          F(X + delta) < F(X), every active view in front of its camera ((R X + t)_z > 0), F finite.  A trial that
 *                       fails one of these is refused like any other failed step; so is a lambda at which chol3 finds no
 *                       positive pivot (no evaluation is spent on it)
 *     stops, status 1   ||g||_inf <= 1e-4 px^2 / m after an accepted step (a position error of about 1e-10 m at H ~ 1e6 px^2 / m^2), or
 *                       a proposed step with ||delta||_2 <= 1e-9 (1e-9 + ||X||_2), which is not evaluated
 *     stops, status 2   max_iter evaluations in the round (the one at the round's start point included)
 *
 * Not refined: a slot whose start point has (R X0 + t)_z <= 0 in an active view, or a cost that is not finite, keeps the DLT bits
 * (status 3; views = the active views, rms_px and max_px NaN); a slot with valid == 0 is untouched (status 0, views 0, NaN,
 * every view_state 0).
 *
 * View rejection, reject_px > 0.  After a round, with d_c = ||e_c||_2 over the views in use: the view with the largest d_c (lowest
 * camera rank on a tie) is dropped when d_c > reject_px and at least min_views remain without it; then the minimiser runs again from
 * the current point with lambda = 1e-3 and max_iter evaluations.  At most max_reject rounds drop a view.  Which views are in use is
 * kept in view_state, read and written by the kernel: there is no limit on the number of cameras.
 *
 * Limits of the method.  With 3 views and one outlier, or 5 views and two, the view with the largest residual at the robust
 * minimum is the wrong one in a few percent of slots: the bad views must be a clear minority (one of four, two of six).
 *
 * The result is the same bits from run to run: no atomics, the cameras in ascending order.
 */
#ifndef CALISCOPE_TRAJECTORY_REFINE_H
#define CALISCOPE_TRAJECTORY_REFINE_H

#include <stdint.h>

#include "../caliscope_trajectory.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int32_t loss;       /* 0 linear, 1 huber, 2 soft_l1, 3 cauchy, 4 arctan, as cba_problem_desc */
  int32_t max_iter;   /* >= 1: evaluations of a round */
  double f_scale;     /* pixels; finite, and > 0 unless the loss is linear */
  double reject_px;   /* >= 0, finite; 0: no view is dropped */
  int32_t max_reject; /* >= 0: views dropped per slot at most */
  int32_t min_views;  /* >= 2: views a slot keeps */
} cba_traj_refine;

/* Every pointer may be NULL: that output is not returned.  Cells that xyz_gap fills afterwards keep views 0 and NaN. */
typedef struct {
  int32_t* views;      /* [n_slots] views in use at the end */
  double* rms_px;      /* [n_slots] sqrt(mean d_c^2) over them */
  double* max_px;      /* [n_slots] max d_c over them */
  int32_t* iterations; /* [n_slots] evaluations, all rounds together */
  uint8_t* status;     /* [n_slots] 0 no point, 1 converged, 2 iteration cap, 3 kept the DLT point */
  uint8_t* view_state; /* [n_cams][n_slots] 0 no cell / camera unposed / slot without a point, 1 used, 2 rejected */
} cba_traj_quality;

/* cba_reconstruct_trajectories with k_traj_refine (one thread per slot) between k_traj_triangulate and k_traj_fill3d.
 * Further checks on the host before anything is launched, CBA_ERR_INVALID with the field named: a null `refine`, an unknown loss,
 * f_scale not finite or (loss != linear) not positive, max_iter < 1, reject_px negative or not finite, min_views < 2,
 * max_reject < 0.  The memory check counts n_cams * n_slots + 25 * n_slots bytes more.  n_rows == 0 succeeds without a launch. */
int cba_reconstruct_trajectories_refined(const cba_traj_desc* d, const cba_traj_refine* refine, int32_t device, cba_traj_out* out,
                                         cba_traj_quality* quality);

#ifdef __cplusplus
}
#endif

#endif /* CALISCOPE_TRAJECTORY_REFINE_H */
