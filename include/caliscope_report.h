/* caliscope_report.h — C ABI of the reprojection statistics and the outlier filter in libcaliscope_ba.so
 * (caliscope_amd/csrc/report_lib.hip).
 *
 * The step between the solver passes of calibrate_extrinsics (caliscope_amd/reprojection_stats.py; the reference's
 * core/capture_volume.py:150-235 and :607-753): pixel errors of every observation, their sums per camera and per (object, keypoint)
 * group, and the keep mask of the percentile or the absolute filter with its safety floor, in one call.  Conventions are those of
 * caliscope_ba.h: the entry point returns 0 or a negative CBA_ERR_*, cba_last_error() describes a failure, and there is no CPU
 * fallback (without a HIP device: CBA_ERR_NO_DEVICE).  The symbol is bound by caliscope_amd/reprojection_stats.py, not by
 * caliscope_amd/_lib.py.
 */
#ifndef CALISCOPE_REPORT_H
#define CALISCOPE_REPORT_H

#include <stdint.h>

#include "caliscope_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CBA_REPORT_STATS 0      /* errors and sums only */
#define CBA_REPORT_PERCENTILE 1 /* value: the percentage of observations to remove, in (0, 100] */
#define CBA_REPORT_ABSOLUTE 2   /* value: the largest pixel error that is kept, > 0 */

#define CBA_REPORT_PER_CAMERA 0 /* one percentile threshold per camera */
#define CBA_REPORT_OVERALL 1    /* one threshold over all observations */

typedef struct {
  int32_t n_cams;
  int64_t n_points;
  int64_t n_obs;
  int32_t n_groups;
  /* cameras with locked intrinsics and points; not read (may be NULL) when err_in is given */
  const int32_t* cam_model; /* [n_cams] 0 pinhole (k1 k2 p1 p2 k3), 1 fisheye (k1..k4) */
  const double* cam_const;  /* [n_cams][12] fx fy cx cy d0..d4 0 0 0, as cba_problem_desc */
  const double* cam_pose;   /* [n_cams][6] rvec, tvec */
  const double* points;     /* [n_points][3] */
  const int32_t* obs_cam;   /* [n_obs] in [0, n_cams) */
  const int32_t* obs_pt;    /* [n_obs] in [0, n_points); not read when err_in is given */
  const double* obs_uv;     /* [n_obs][2] pixels; not read when err_in is given */
  const int32_t* obs_group; /* [n_obs] in [0, n_groups), or NULL: no per-group sums */
  const double* err_in;     /* [n_obs] Euclidean pixel errors, finite and >= 0, or NULL: the errors are computed by projection */
  int32_t mode;             /* CBA_REPORT_STATS / _PERCENTILE / _ABSOLUTE */
  int32_t scope;            /* CBA_REPORT_PER_CAMERA / _OVERALL (percentile only) */
  double value;
  int64_t min_per_camera;   /* safety floor of the two filters, >= 1 */
} cba_report_desc;

/* Every pointer may be NULL: that output is not returned. */
typedef struct {
  double* err_xy;         /* [n_obs][2] projected - observed, pixels (residual times fx); not written when err_in is given */
  double* err;            /* [n_obs] sqrt(ex^2 + ey^2), or err_in */
  double* cam_sumsq;      /* [n_cams] sum of err^2 */
  int64_t* cam_count;     /* [n_cams] */
  double* group_sumsq;    /* [n_groups] */
  int64_t* group_count;   /* [n_groups] */
  double* overall_sumsq;  /* [1] */
  int64_t* n_nonfinite;   /* [1] observations whose error is NaN or infinite */
  double* cam_threshold;  /* [n_cams] filters: the threshold in force per camera after the floor (+inf: a camera without rows) */
  uint8_t* keep;          /* [n_obs] filters: 1 kept, 0 removed */
  int64_t* cam_kept;      /* [n_cams] filters */
  int64_t* n_floor_cams;  /* [1] filters: cameras topped up by the safety floor */
} cba_report_out;

/* One call: an error kernel (projection with ba_math.h, sums in LDS partials per workgroup), and for the filters a radix select
 * over the bit patterns of the errors (eight passes of a histogram kernel and a refinement kernel per round: non-negative doubles
 * order like their bits read as unsigned integers, so every order statistic is found with integer atomics and without a sort), the
 * percentile interpolation of numpy's default method on the host, a mask kernel, and a second select round with one query per
 * camera below the floor.
 *
 * Keep rule: err <= threshold of the camera.  Floor: a camera with n rows that keeps fewer than r = min(min_per_camera, n) keeps
 * err <= (its r-th smallest error) instead; ties at that value are all kept; every camera below the floor is topped up.
 *
 * Reproducibility: counts, order statistics, thresholds, keep, cam_kept and n_floor_cams are exact and identical from run to run.
 * The floating sums (cam_sumsq, group_sumsq, overall_sumsq) are added with atomics in the order of arrival: they vary in the last
 * bits between runs (relative error at most n 2^-53 for a sum of n terms).
 *
 * Checks on the host before anything is launched (CBA_ERR_INVALID, the message names the observation): every camera, point and
 * group index in range, err_in finite and not negative.  n_obs == 0 or n_cams == 0 succeeds without a launch (zero sums, +inf
 * thresholds).  When an error is not finite (n_nonfinite != 0) a filter call returns the errors and sums and leaves the filter
 * outputs untouched: the caller decides. */
int cba_reprojection_filter(const cba_report_desc* d, int32_t device, cba_report_out* out);

#ifdef __cplusplus
}
#endif

#endif /* CALISCOPE_REPORT_H */
