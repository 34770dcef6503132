/* caliscope/reliability.h — C ABI of the per-observation reliability report in libcaliscope_ba.so
 * (caliscope_amd/csrc/reliability_lib.hip, caliscope_amd/csrc/reliability_math.h).
 *
 * How strongly the other observations control each observation of a calibration, and which observations are statistically
 * incompatible with the adjustment: per residual row j the redundancy number r_j, the diagonal of R = I - J pinv(J^T J) J^T, and the
 * standardised residual w_j = f~_j / (sigma0 sqrt(r_j)) of Baarda's / Pope's data snooping (caliscope_amd/reliability.py; the
 * reference has a percentile / absolute cut on the raw reprojection error only).  The dense 2 n_obs x 2 n_obs projector is never
 * formed.  The input structure, the host checks, the error codes and the numeric refusals are those of cba_parameter_covariance
 * (uncertainty.h), whose launches up to C = St^-1 this call shares; conventions are those of caliscope_ba.h, and there is no CPU
 * fallback.  The symbol is bound by caliscope_amd/reliability.py.
 */
#ifndef CALISCOPE_RELIABILITY_H
#define CALISCOPE_RELIABILITY_H

#include <stdint.h>

#include "uncertainty.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every pointer may be NULL: that output is not returned.  Rows are in the CALLER's observation order. */
typedef struct {
  double* redundancy;      /* [n_obs][3] R_oo = I - P_oo of the observation's two rows: uu, uv, vv; r_u = uu, r_v = vv (not clamped) */
  double* w;               /* [n_obs][2] standardised residuals; NaN where r_j <= 1e-10 (REL_R_TINY of reliability_math.h) */
  double* residual;        /* [n_obs][2] f~: the residual (pixels / fx0) scaled for the robust loss as scipy scales it */
  double* sigma0_sq;       /* [1] 2 cost / dof, as cba_cov_out */
  int64_t* dof;            /* [1] 2 n_obs - (ncp + 3 n_points) + 7 */
  double* cost;            /* [1] 0.5 sum rho(residual^2) */
  int64_t* n_uncontrolled; /* [1] residual rows with r_j <= 1e-10: a blunder there cannot be seen at all */
} cba_rel_out;

/* With the notation of uncertainty.h, for observation o of camera a and point i with scaled Jacobian blocks A_o (2 x np_a), B_o (2 x 3):
 *     P_oo = B_o (V_i^-1 + Q_i) B_o^T + A_o C_aa A_o^T - A_o G_o B_o^T - (A_o G_o B_o^T)^T,
 *     G_o  = sum_b' C_{a,cam(b')} Y_b'  (np_a x 3),   Q_i = sum_b Y_b^T G_b  (3 x 3),   b, b' over the observations of point i,
 *     R_oo = I - P_oo,   r = diag(R_oo),   w_j = f~_j / (sigma0 sqrt(min(max(r_j, 0), 1))).
 * J (J^T J)^- J^T is the same for every generalised inverse, so the gauge terms of the point covariance do not appear.  sum_j r_j
 * = dof.  One more kernel behind the launches of cba_parameter_covariance: one wave per point, sixteen lanes per observation (a lane
 * per row of G_o); A_o and B_o are recomputed, nothing is added across points, so this pass uses no floating-point atomics and
 * repeats its bits whenever C does; with CBA_DETERMINISTIC=1 a permutation of the rows of the call permutes the outputs bit for bit (the
 * observations of a point are put in an order of their own before anything is added).
 *
 * Scope: reprojection rows only, as uncertainty.h.  For a robust loss J and f~ are scipy's scaled ones and w is an approximation
 * (the scaled problem is treated as a linear-loss problem with unit weights).  With cost == 0 (sigma0 == 0) w is not finite.
 * A call that fails a check (CBA_ERR_INVALID, CBA_ERR_UNSUPPORTED, CBA_ERR_NUMERIC, CBA_ERR_NO_DEVICE) writes nothing: the arrays are
 * copied from the device straight into the caller's memory after the last check. */
int cba_observation_reliability(const cba_cov_desc* d, int32_t device, cba_rel_out* out);

#ifdef __cplusplus
}
#endif

#endif /* CALISCOPE_RELIABILITY_H */
