/* caliscope/uncertainty.h — C ABI of the free-network parameter covariance in libcaliscope_ba.so
 * (caliscope_amd/csrc/covariance_lib.hip, caliscope_amd/csrc/covariance_math.h).
 *
 * How well the observations determine every camera and every point of a calibration: the covariance of the bundle-adjustment
 * parameters in the inner-constraint (minimum-trace, free-network) gauge, Sigma = sigma0^2 pinv(J^T J), without ever forming
 * J^T J or a pseudo-inverse (caliscope_amd/uncertainty.py; the reference computes no covariance).  Conventions are those of
 * caliscope_ba.h: the entry point returns 0 or a negative CBA_ERR_*, cba_last_error() describes a failure, and there is no CPU
 * fallback (without a HIP device: CBA_ERR_NO_DEVICE).  The symbol is bound by caliscope_amd/uncertainty.py, not by
 * caliscope_amd/_lib.py.
 */
#ifndef CALISCOPE_UNCERTAINTY_H
#define CALISCOPE_UNCERTAINTY_H

#include <stdint.h>

#include "../caliscope_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int32_t n_cams;
  int64_t n_points;
  int64_t n_obs;
  const int32_t* cam_model;   /* [n_cams] 0 pinhole (k1 k2 p1 p2 k3), 1 fisheye (k1..k4) */
  const int32_t* cam_nparams; /* [n_cams] 6 (rvec, tvec) or 9 (+ s, k1, k2; pinhole only) */
  const double* cam_const;    /* [n_cams][12] fx0 fy0 cx cy d0..d4 0 0 0, as cba_problem_desc */
  const double* cam_x;        /* [n_cams][9] rvec, tvec, s, k1, k2 (the last three are read for a 9-parameter camera only) */
  const double* points;       /* [n_points][3] */
  const int32_t* obs_cam;     /* [n_obs] in [0, n_cams) */
  const int32_t* obs_pt;      /* [n_obs] in [0, n_points) */
  const double* obs_uv;       /* [n_obs][2] pixels */
  int32_t loss;               /* 0 linear, 1 huber, 2 soft_l1, 3 cauchy, 4 arctan, as cba_problem_desc */
  double f_scale;             /* > 0, in residual units (pixels / fx0); not read for the linear loss */
} cba_cov_desc;

/* Every pointer may be NULL: that output is not returned.  ncp = sum of cam_nparams; a camera's parameters start at the sum of
 * the widths of the cameras before it. */
typedef struct {
  double* cam_cov;      /* [n_cams][9][9] the camera's own block, upper-left nparams x nparams used, the rest 0 */
  double* cam_cov_full; /* [ncp][ncp] all camera parameters, cross-covariances included */
  double* point_cov;    /* [n_points][6] xx xy xz yy yz zz */
  double* sigma0_sq;    /* [1] 2 cost / dof */
  int64_t* dof;         /* [1] 2 n_obs - (ncp + 3 n_points) + 7 */
  double* cost;         /* [1] 0.5 sum rho(residual^2), the solver's cost at this point */
} cba_cov_out;

/* J is the Jacobian the solver uses (residuals in pixels / fx0, rows scaled for the robust loss as scipy scales them), H = J^T J =
 * [[U, W], [W^T, V]] with U block-diagonal per camera and V per point.  The seven columns of N (translation, rotation, scale of
 * the world) span the null space of J at any parameter vector; with Np, Nc its point and camera rows,
 *     D = Np^T V^-1 Np,  B = Nc - W V^-1 Np,  St = (U - W V^-1 W^T) + B D^-1 B^T  (symmetric positive definite),
 *     pinv(H)_cc = St^-1,
 *     pinv(H)_pp,i = V_i^-1 - Z_i D^-1 Z_i^T + T_i St^-1 T_i^T,   Z_i = V_i^-1 Np,i,   T_i = (W_i V_i^-1)^T + Z_i D^-1 B^T.
 * One call: a kernel per camera (tables, gauge rows), one per observation (Jacobian blocks, U, cost), one workgroup per point
 * (V^-1, Z, the point's terms of B and of the dense Schur complement), a reduction for D, the assembly of St with a symmetric
 * Jacobi scaling, the solver's blocked FP64-MFMA Cholesky that builds T = L^-T beside the factor, an MFMA product T T^T, and a
 * workgroup per point for the 3 x 3 formula.  D (7 x 7) is inverted on the host between two launches.
 *
 * Scope: reprojection rows only.  A volume with distance constraints couples points and fixes the scale: not handled by this entry
 * point but by the one of uncertainty_constrained.h, which leaves everything here as it is.
 *
 * Reproducibility: U, the cost, B, D and the Schur complement are added with floating-point atomics in the order of arrival, so
 * every output varies in its last bits from run to run (relative to the norm of its block: a few ulp times the condition of St).
 *
 * Checks on the host before anything is launched (CBA_ERR_INVALID, the message names the offender): n_obs > 0, every camera and
 * point index in range, cam_nparams 6 or 9, a fisheye camera with 9 parameters (CBA_ERR_UNSUPPORTED), every point with at least
 * two observations, every camera with at least one, dof > 0, f_scale > 0 for a robust loss.  A pivot that is not safely positive
 * (a point whose rays are parallel, all points on one line, a planar scene in front of fronto-parallel cameras with free focal
 * lengths) returns CBA_ERR_NUMERIC and writes nothing; no output is ever NaN without an error code. */
int cba_parameter_covariance(const cba_cov_desc* d, int32_t device, cba_cov_out* out);

#ifdef __cplusplus
}
#endif

#endif /* CALISCOPE_UNCERTAINTY_H */
