/* caliscope/uncertainty_constrained.h — C ABI of the free-network parameter covariance of a problem WITH rigid-distance constraint rows
 * in libcaliscope_ba.so (caliscope_amd/csrc/covariance_lib.hip, covariance_constraint_plan.h, covariance_constraint_math.h).
 *
 * caliscope/uncertainty.h stays as it is (cba_cov_desc, cba_cov_out and cba_parameter_covariance are used by existing harnesses and
 * bindings); this header adds one structure and one entry point on top of it.  The symbol is bound by caliscope_amd/uncertainty.py
 * (CONSTRAINED_UNCERTAINTY_SIGNATURES).
 */
#ifndef CALISCOPE_UNCERTAINTY_CONSTRAINED_H
#define CALISCOPE_UNCERTAINTY_CONSTRAINED_H

#include <stdint.h>

#include "uncertainty.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The rows of cba_set_constraints (caliscope_ba.h): r = weight (|| mean points[groups_a] - mean points[groups_b] || - distance).  A corner
 * endpoint names one point four times, a centroid endpoint four points. */
typedef struct {
  int32_t n_con;
  const int32_t* groups_a;  /* [n_con][4] rows of desc->points */
  const int32_t* groups_b;  /* [n_con][4] rows of desc->points */
  const double* distances;  /* [n_con] >= 0, finite */
  const double* weights;    /* [n_con] >= 0, finite; a row of weight 0 is dropped */
} cba_cov_constraints;

/* Sigma = sigma0^2 pinv(J^T J) with J the solver's Jacobian INCLUDING the constraint rows, every row (constraint rows too) scaled for
 * the robust loss as scipy scales it.  H = [[U, W], [W^T, V~]] with V~ = V + C^T C, C the scaled constraint rows: V~ is block-diagonal
 * per connected component of the constraint graph (the eight point indices of a row are connected; a point in no row is a component of
 * its own).  Distances are invariant under rigid motions and not under scale: the gauge has the first SIX columns of N (translation,
 * rotation), dof = 2 n_obs + n_con - n_params + 6 (n_con: the rows of positive weight) and sigma0^2 = 2 cost / dof with the constraint
 * rows in the cost.  The bordered elimination of uncertainty.h carries over with V~ for V and six columns for seven:
 *     Z = V~^-1 Np,  D = Np^T Z (6 x 6),  B = Nc - W Z,  St = U - W V~^-1 W^T + B D^-1 B^T,  pinv(H)_cc = St^-1,
 *     pinv(H)_pp,i = [V~_k^-1]_ii + Z_i F Z_i^T + sum_cc' Y_c[:, i]^T C_cc' Y_c'[:, i] + sum_c sym(Y_c[:, i]^T E_c Z_i^T),
 * Y_c = W_c,k V~_k^-1 the block row of camera c against the whole component k of point i.
 *
 * One workgroup per component with at least one row assembles V~_k in LDS (packed lower triangle), factors and inverts it there and
 * leaves Z_k, Y_c, the component's terms of B and of the Schur complement; points in no row go through the kernels of the
 * unconstrained call with six gauge columns.  A component holds at most COV_COMPONENT_CAP = 54 points (covariance_math.h: the packed
 * triangle of 162 x 162 doubles is 105.6 KB of the 160 KiB of LDS); the number of rows is not limited.
 *
 * With constraints == NULL, n_con == 0 or every weight 0 the call IS cba_parameter_covariance: seven columns, the same launches.
 *
 * A point needs two observations or a row of positive weight.  Refused on the host before anything is launched, the message naming the
 * offender: a group index outside [0, n_points) (CBA_ERR_INVALID), a weight or distance that is not finite or negative
 * (CBA_ERR_INVALID), a component of more than COV_COMPONENT_CAP points (CBA_ERR_UNSUPPORTED: its first point and its size), device
 * buffers beyond the free device memory (CBA_ERR_UNSUPPORTED), and CBA_DETERMINISTIC=1 together with constraint rows
 * (CBA_ERR_UNSUPPORTED: the fixed-order sums of the unconstrained call are not built for the component kernel).  A component whose
 * V~_k has no positive pivot, or a pivot of St at or below COV_PIVOT_TINY, is CBA_ERR_NUMERIC and writes nothing. */
int cba_parameter_covariance_constrained(const cba_cov_desc* d, const cba_cov_constraints* constraints, int32_t device, cba_cov_out* out);

#ifdef __cplusplus
}
#endif

#endif /* CALISCOPE_UNCERTAINTY_CONSTRAINED_H */
