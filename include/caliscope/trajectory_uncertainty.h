/* caliscope/trajectory_uncertainty.h — C ABI of the trajectory reconstruction with a 3-D covariance per sample in libcaliscope_ba.so
 * (caliscope_amd/csrc/trajectory_lib.hip, caliscope_amd/csrc/trajectory_cov_math.h).
 *
 * cba_reconstruct_trajectories (../caliscope_trajectory.h) and cba_reconstruct_trajectories_refined (trajectory_refine.h) return
 * points; the refined call adds how well each point fits its views.  Neither says how well the views determine the point: a
 * two-view sample with a 5 degree baseline reprojects to a fraction of a pixel and is uncertain by centimetres in depth, and the
 * uncertainty of the calibration itself (cba_parameter_covariance, uncertainty.h) reaches no trajectory.  This call puts one kernel,
 * k_traj_cov, after k_traj_refine (after k_traj_triangulate in the plain call) and before k_traj_fill3d: per slot, the covariance of
 * the reconstructed point from the pixel noise of the recording and from the covariance of the camera parameters.  Everything else
 * is the call it extends, launch for launch: xyz, valid, the times, the grids and the quality are the bytes that call returns.
 * There is no CPU fallback.  The symbol is bound by caliscope_amd/trajectory_uncertainty.py.
 *
 * Mathematics.  A slot has the point X and the views c in use: in the refined call the cameras with view_state == 1 at the end, in
 * the plain call the posed cameras with a cell in the filled 2-D grid.  With pi_c(X, theta_c) the pixel projection and theta_c the
 * camera's bundle-adjustment parameters (rvec, tvec and, for a 9-wide camera, s, k1, k2, as cam_prepare of ba_math.h reads them),
 *     B_c = d pi_c / d X        (2 x 3, pixels per world unit)
 *     A_c = d pi_c / d theta_c  (2 x n_c, pixels; the intrinsic columns of a 6-wide camera are zero)
 *     V   = sum_c B_c^T B_c
 *     M_c = V^-1 B_c^T A_c      (3 x n_c)
 *     cov_noise = sigma_px^2 V^-1
 *     cov_calib = sum_{c, c'} M_c cam_cov[c, c'] M_c'^T
 *     cov       = cov_noise + cov_calib
 * the first-order (Gauss-Newton) propagation of the reprojection-error minimiser, dX = V^-1 sum_c B_c^T (du_c - A_c dtheta_c), the
 * pixel noise of the recording and the error of the calibration independent.  cam_cov is cam_cov_full of cba_parameter_covariance
 * (already scaled by sigma0^2; parameter units do not depend on the residual units); sigma_px is the standard deviation of a
 * tracked 2-D landmark, the caller's to give: a tracker's noise is not the board corners'.  B_c and A_c are project_full's of
 * ba_math.h times fx0; V^-1 through chol3; the cameras ascending, the pairs (c, c') with c' <= c and the transpose added for c' < c.
 *
 * Limits.  The covariance is exact for a point refined under the linear loss; first-order for a DLT point (the plain call: the DLT
 * minimises an algebraic error, not this one); approximate under a robust loss, where the views in use are weighted alike (as w is
 * in reliability.h).  It is relative to the free-network datum of the calibration: no overall similarity (position, orientation,
 * scale of the whole rig) is included.  It is the covariance of the sample before the 3-D fill and the Butterworth filter: a cell
 * the fill adds has none, and the smoothing, which correlates neighbouring samples, is not propagated.  The camera tables must be
 * those the covariance was computed at.
 *
 * The result is the same bits from run to run: no atomics, the cameras in ascending order.
 */
#ifndef CALISCOPE_TRAJECTORY_UNCERTAINTY_H
#define CALISCOPE_TRAJECTORY_UNCERTAINTY_H

#include <stdint.h>

#include "trajectory_refine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per camera of the grid (rank c of cba_traj_desc; the rows of cameras with cam_posed == 0 are not read). */
typedef struct {
  const int32_t* cam_nparams; /* [n_cams] 6 (rvec, tvec) or 9 (+ s, k1, k2; pinhole only), as cba_cov_desc */
  const double* cam_const;    /* [n_cams][12] fx0 fy0 cx cy d0..d4 0 0 0, as cba_cov_desc */
  const double* cam_x;        /* [n_cams][9] rvec, tvec, s, k1, k2 (the last three are read for a 9-parameter camera only) */
  const int64_t* cam_offset;  /* [n_cams] first row of the camera in cam_cov; -1: no covariance, the camera is taken as exact */
  int64_t ncp;                /* rows of cam_cov */
  const double* cam_cov;      /* [ncp][ncp] covariance of the camera parameters; NULL: the noise term only (no pair pass runs,
                                 cam_offset and ncp are not read) */
  double sigma_px;            /* standard deviation of a 2-D landmark in pixels; finite, > 0 */
} cba_traj_uncertainty;

/* cov and cov_status may be NULL like every output of the call.  Rows are xx xy xz yy yz zz, in world units squared. */
typedef struct {
  double* cov;         /* [n_slots][6] cov_noise + cov_calib */
  double* cov_calib;   /* [n_slots][6] cov_calib alone; may be NULL; NaN when cam_cov is NULL */
  uint8_t* cov_status; /* [n_slots] 0 no point, 1 ok, 2 not computable: a view in use with (R X + t)_z <= 0, chol3(V) without a
                          positive pivot, or a cell that xyz_gap filled.  Rows of status 0 or 2 are NaN, rows of status 1 never */
} cba_traj_cov_out;

/* cba_reconstruct_trajectories (refine == NULL, and then quality must be NULL) or cba_reconstruct_trajectories_refined with
 * k_traj_cov (one thread per slot) in front of k_traj_fill3d.  Further checks on the host before anything is launched,
 * CBA_ERR_INVALID with the offender named: sigma_px not finite or not positive; for a posed camera cam_nparams other than 6 or 9
 * (a fisheye camera with 9: CBA_ERR_UNSUPPORTED, as cba_cov_desc); with cam_cov given, a cam_offset below -1, a block
 * [cam_offset, cam_offset + cam_nparams) that leaves [0, ncp) or meets the block of another posed camera, an entry of cam_cov that is
 * not finite, and |cam_cov[i][j] - cam_cov[j][i]| > 1e-12 max|diag|.  The memory check counts the buffers of this call as well:
 * 49 n_slots bytes (48 more with cov_calib), 396 n_cams and 8 ncp^2.  n_rows == 0 succeeds without a launch. */
int cba_reconstruct_trajectories_uncertain(const cba_traj_desc* d, const cba_traj_refine* refine, const cba_traj_uncertainty* uncertainty,
                                           int32_t device, cba_traj_out* out, cba_traj_quality* quality, cba_traj_cov_out* cov_out);

#ifdef __cplusplus
}
#endif

#endif /* CALISCOPE_TRAJECTORY_UNCERTAINTY_H */
