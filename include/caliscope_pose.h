/* caliscope_pose.h — C ABI of the pose-bootstrap kernels in libcaliscope_ba.so (caliscope_amd/csrc/pose_lib.hip).
 *
 * The initial pose network of an unposed board session (caliscope_amd/pose_network.py): a PnP solve per board view and
 * the stereo reprojection RMSE of every aggregated camera pair.  Conventions are those of caliscope_ba.h: every entry
 * point returns 0 or a negative CBA_ERR_*, cba_last_error() describes a failure, and there is no CPU fallback (without a
 * HIP device: CBA_ERR_NO_DEVICE).  These symbols are bound by caliscope_amd/pose_network.py, not by caliscope_amd/_lib.py.
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

#ifdef __cplusplus
}
#endif

#endif /* CALISCOPE_POSE_H */
