/* caliscope_pose.h — C ABI of the pose-bootstrap kernels in libcaliscope_ba.so (caliscope_amd/csrc/pose_lib.hip).
 *
 * The initial pose network of an unposed board session (caliscope_amd/pose_network.py): a PnP solve per board view and
 * the stereo reprojection RMSE of every aggregated camera pair; for sessions without object geometry
 * (caliscope_amd/epipolar_pose.py) essential-matrix RANSAC per camera pair and RANSAC resection against a point cloud.  Conventions are those of caliscope_ba.h: every entry
 * point returns 0 or a negative CBA_ERR_*, cba_last_error() describes a failure, and there is no CPU fallback (without a
 * HIP device: CBA_ERR_NO_DEVICE).  These symbols are bound by caliscope_amd/pose_network.py and caliscope_amd/epipolar_pose.py, not by
 * caliscope_amd/_lib.py.
 */
#ifndef CALISCOPE_POSE_H
#define CALISCOPE_POSE_H

#include <stdint.h>

#include "caliscope_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

enum cba_pnp_status { CBA_PNP_OK = 0, CBA_PNP_TOO_FEW = 1, CBA_PNP_FAILED = 2 };

/* Board views in CSR form.  View v holds observations view_start[v] .. view_start[v+1] - 1 of camera view_cam[v]. */
typedef struct {
  int32_t n_cams;
  const int32_t* cam_model;  /* [n_cams] 0 pinhole (k1 k2 p1 p2 k3), 1 fisheye (k1..k4) */
  const double* cam_intr;    /* [n_cams][9] fx fy cx cy d0..d4 */
  int64_t n_views;
  const int64_t* view_start; /* [n_views + 1], non-decreasing, view_start[0] = 0 */
  const int32_t* view_cam;   /* [n_views] */
  const double* obs_xy;      /* [n_obs][2] pixel coordinates */
  const double* obs_obj;     /* [n_obs][3] object points (obj_loc); a NaN z is read as 0 */
  int32_t min_points;        /* planar views need min_points, non-planar views max(min_points, 6) */
  int32_t float32_io;        /* round pixels, undistorted points and object points to float32 (as cba_triangulate) */
} cba_pose_pnp_desc;

/* Undistortion + PnP of every view, one thread per view (views ordered by point count inside).  pose_out[n_views][12]:
 * R row-major then t (X_cam = R X_obj + t); rmse_out[n_views]: sqrt(mean |uv - proj|^2) in normalised coordinates;
 * status_out[n_views]: cba_pnp_status (a view that is not CBA_PNP_OK gets R = I, t = 0, rmse = 0).  undistorted_out
 * (optional, [n_obs][2]): the normalised image points the solve used. */
int cba_pose_pnp_batch(const cba_pose_pnp_desc* d, int32_t device, double* pose_out, double* rmse_out, int32_t* status_out,
                       double* undistorted_out);

/* Common observations of camera pairs in CSR form, already undistorted and normalised. */
typedef struct {
  int64_t n_pairs;
  const double* pair_pose;   /* [n_pairs][12]: R row-major then t of camera B relative to camera A */
  const int64_t* pair_start; /* [n_pairs + 1] */
  const double* obs_a;       /* [n_obs][2] */
  const double* obs_b;       /* [n_obs][2] */
} cba_pose_pair_desc;

/* Stereo RMSE of every pair, one workgroup per pair: two-view DLT (A at [I | 0], B at [R | t]), reprojection into both,
 * rmse_out[p] = sqrt(sum of squared errors / (2 m)) over its m observations (0 when m = 0), count_out[p] = m.  The sum runs
 * in a fixed order: the result does not change from run to run. */
int cba_pose_pair_rmse(const cba_pose_pair_desc* d, int32_t device, double* rmse_out, int64_t* count_out);

/* 2-D-only sessions (caliscope_amd/epipolar_pose.py).  Statuses: 0 OK, 1 too few correspondences / points, 2 failed (no
 * hypothesis with a minimal set of inliers, degenerate essential matrix, non-finite refinement). */
enum cba_epi_status { CBA_EPI_OK = 0, CBA_EPI_TOO_FEW = 1, CBA_EPI_FAILED = 2 };

/* Camera pairs and their correspondences in CSR form.  Correspondence i of pair p (pair_start[p] <= i < pair_start[p+1])
 * joins observation rows corr_a[i] (camera A) and corr_b[i] (camera B). */
typedef struct {
  int32_t n_cams;
  const int32_t* cam_model;  /* as cba_pose_pnp_desc */
  const double* cam_intr;
  int64_t n_obs;
  const double* obs_xy;      /* [n_obs][2] pixels */
  const int32_t* obs_cam;    /* [n_obs] camera index */
  int64_t n_pairs;
  const int64_t* pair_start; /* [n_pairs + 1], non-decreasing, pair_start[0] = 0 */
  const int64_t* corr_a;     /* [n_corr] rows of obs_* */
  const int64_t* corr_b;
  const double* threshold;   /* [n_pairs] Sampson gate in normalised units (inlier: squared distance <= threshold^2) */
  int32_t n_hyp;             /* RANSAC hypotheses per pair, 1 .. 65536 */
  uint64_t seed;
  int32_t float32_io;        /* round pixels and undistorted points to float32 */
} cba_pose_essential_desc;

/* Essential-matrix RANSAC of every pair: undistortion of every row once, n_hyp 8-point hypotheses per pair, Sampson
 * scoring, the winner (most inliers, lowest index on ties) decomposed by cheirality and refined by Levenberg-Marquardt on
 * its inliers' Sampson residuals.  pose_out[n_pairs][12]: R row-major then unit t of camera B in camera A's frame (I, 0 when
 * the status is not CBA_EPI_OK); n_inliers_out / n_cheiral_out: inliers and inliers in front of both cameras at the final
 * pose; conditioning_out: sigma_2 / sigma_1 of the linear fit on the final inliers; winner_out (optional): the winning
 * hypothesis (-1: none); corr_flag_out[n_corr]: 0 outlier, 1 inlier, 2 inlier in front of both; xyz_out (optional,
 * [n_corr][3]): the two-view point (A at [I | 0]), NaN unless flag 2 and |w| > 1e-12; undistorted_out (optional, [n_obs][2]).
 * Deterministic for a given seed. */
int cba_pose_essential_batch(const cba_pose_essential_desc* d, int32_t device, double* pose_out, int32_t* status_out, int64_t* n_inliers_out,
                             int64_t* n_cheiral_out, double* conditioning_out, int32_t* winner_out, uint8_t* corr_flag_out, double* xyz_out,
                             double* undistorted_out);

/* Resection jobs in CSR form: job j holds points job_start[j] .. job_start[j+1] - 1 (object point, normalised image point). */
typedef struct {
  int64_t n_jobs;
  const int64_t* job_start;  /* [n_jobs + 1] */
  const double* obj;         /* [n][3] */
  const double* uv;          /* [n][2] */
  const double* threshold;   /* [n_jobs] reprojection gate, normalised units */
  int32_t n_hyp;             /* 1 .. 65536 */
  int32_t min_points;        /* jobs with fewer points (or fewer than 6) are CBA_EPI_TOO_FEW */
  uint64_t seed;
} cba_pose_resect_desc;

/* RANSAC resection of every job: n_hyp 6-point DLT hypotheses, reprojection scoring, the winner refined by
 * Levenberg-Marquardt on its inliers.  pose_out[n_jobs][12]: R, t with X_cam = R X + t; n_inliers_out at the final pose;
 * winner_out (optional); err_out[n]: |uv - proj| at the final pose (NaN for a job that is not CBA_EPI_OK). */
int cba_pose_resect_batch(const cba_pose_resect_desc* d, int32_t device, double* pose_out, int32_t* status_out, int64_t* n_inliers_out,
                          int32_t* winner_out, double* err_out);

/* Intrinsic calibration of every camera of a rig from its board views (caliscope_amd/calibrate_intrinsics.py).  Statuses per
 * camera: 0 OK, 1 too few (fewer than 3 usable views, or fewer residuals than unknowns), 2 failed (no solvable system at the
 * start, non-finite result).  View statuses are cba_pnp_status. */
enum cba_intr_status { CBA_INTR_OK = 0, CBA_INTR_TOO_FEW = 1, CBA_INTR_FAILED = 2 };

typedef struct {
  int32_t n_cams;
  const int32_t* cam_model;  /* [n_cams] 0 pinhole (fx fy cx cy k1 k2 p1 p2 k3), 1 fisheye (fx fy cx cy k1..k4) */
  const double* cam_size;    /* [n_cams][2] image width, height in pixels */
  const double* cam_start;   /* optional [n_cams][9] start intrinsics fx fy cx cy d0..d4; a row whose fx is not > 0 (and a null
                                pointer) takes the default: pinhole f = max(w, h), c = ((w-1)/2, (h-1)/2); fisheye f = max(w, h) / pi,
                                c = (w/2 - 0.5, h/2 - 0.5); zero coefficients */
  int64_t n_views;
  const int64_t* view_start; /* [n_views + 1], non-decreasing, view_start[0] = 0: views in CSR form as cba_pose_pnp_desc */
  const int32_t* view_cam;   /* [n_views] */
  const double* obs_xy;      /* [n_obs][2] pixels */
  const double* obs_obj;     /* [n_obs][3] object points; a NaN z is read as 0 */
  int32_t float32_io;        /* round pixels and object points to float32 (the reference's astype(np.float32)) */
  int32_t max_iter;          /* linearisations per camera; 0: the default (100) */
} cba_intrinsics_desc;

/* One workgroup per camera: start poses by PnP on the pixels undistorted with the start intrinsics (views with fewer than 4
 * corners, a failed PnP, a fisheye corner beyond 1.5 rad or a corner behind the camera at the start are left out), then
 * Levenberg-Marquardt over the intrinsics and one pose per view on the pixel reprojection error, skew fixed at 0.
 * intr_out[n_cams][9]: fx fy cx cy d0..d4 (the start values when the status is not OK); rmse_out[n_cams]: sqrt(sum |e|^2 /
 * n_corners) in pixels over the views used (0 when not OK); iters_out (optional): linearisations; pose_out[n_views][12]: R
 * row-major then t of every view (I, 0 for a view left out; for a camera that is not OK the pose at which its solve stopped, the
 * PnP start pose when it never stepped); view_rmse_out[n_views]: the same RMSE per view (0 for a view left
 * out); view_status_out[n_views].  Sums run in a fixed order: the result does not change from run to run. */
int cba_pose_intrinsics_batch(const cba_intrinsics_desc* d, int32_t device, double* intr_out, double* rmse_out, int32_t* status_out,
                              int32_t* iters_out, double* pose_out, double* view_rmse_out, int32_t* view_status_out);

/* Frame selection and coverage report for the intrinsic calibration of every camera of a rig (caliscope_amd/frame_selector.py; the
 * reference's core/frame_selector.py).  Frames in CSR form over the rows, cameras in CSR form over the frames: the frames of a
 * camera are contiguous and ascending in sync_index, and a frame number in the outputs counts from the camera's first frame.
 * Statuses of a frame's homography: */
enum cba_frame_homog_status { CBA_FSEL_OK = 0, CBA_FSEL_TOO_FEW = 1, CBA_FSEL_FAILED = 2 };

typedef struct {
  int32_t n_cams;
  const int64_t* cam_frame_start; /* [n_cams + 1], non-decreasing, [0] = 0, [n_cams] = n_frames */
  const double* cam_size;         /* [n_cams][2] image width, height in pixels */
  int64_t n_frames;
  const int64_t* frame_start;     /* [n_frames + 1], non-decreasing, [0] = 0 */
  const int64_t* homog_start;     /* optional [n_frames]: first row of the rows the frame's homography is fitted to, */
  const int32_t* homog_count;     /* [n_frames] and their number, inside the frame; both null: the whole frame */
  const double* obs_xy;           /* [n_obs][2] pixels */
  const double* obs_obj;          /* [n_obs][2] board x, y */
  int32_t grid_size;              /* coverage grid, 1..8 (the cell mask has 64 bits: bit row * grid_size + col); beyond: CBA_ERR_UNSUPPORTED */
  int32_t min_corners;            /* rows a frame needs to be eligible */
  int32_t target_count;           /* frames to select per camera, >= 1 */
  int32_t float32_io;             /* homography inputs rounded to float32, board coordinates normalised in float (the reference) */
} cba_frame_select_desc;

/* Two launches.  Per frame: cell_mask_out[n_frames]; pose_feat_out[n_frames][5] centroid x y, spread x y (each / image size),
 * aspect; orient_out[n_frames][3] tilt direction [0, 2 pi), tilt magnitude, in-plane rotation [0, 2 pi) from the least-squares
 * homography of the pixel transfer error (three zeros unless the status is OK); homog_status_out; homog_rmse_out: transfer RMSE in
 * pixels.  Per camera: selected_out[n_cams][target_count] frame numbers in selection order (anchors of the occupied tilt bins
 * first, then the greedy coverage phase), -1 beyond n_selected_out; n_anchors_out: occupied bins; bin_mask_out: their bits;
 * eligible_out: frames with at least min_corners rows.  Ties go to the lowest frame; every reduction runs in a fixed order: the
 * result does not change from run to run.  A decreasing CSR array or a subrange outside its frame is CBA_ERR_INVALID, the message
 * names the position.  n_frames == 0 or n_cams == 0 succeeds without a launch. */
int cba_pose_select_frames(const cba_frame_select_desc* d, int32_t device, uint64_t* cell_mask_out, double* pose_feat_out, double* orient_out,
                           int32_t* homog_status_out, double* homog_rmse_out, int32_t* selected_out, int32_t* n_selected_out,
                           int32_t* n_anchors_out, int32_t* bin_mask_out, int32_t* eligible_out);

#ifdef __cplusplus
}
#endif

#endif /* CALISCOPE_POSE_H */
