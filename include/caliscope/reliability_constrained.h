/* caliscope/reliability_constrained.h — C ABI of the reliability report of a problem WITH rigid-distance constraint rows in
 * libcaliscope_ba.so (caliscope_amd/csrc/reliability_lib.hip, reliability_constraint_math.h).
 *
 * caliscope/reliability.h and caliscope/uncertainty_constrained.h stay as they are; this header adds one structure and one entry point on
 * top of them.  The symbol is bound by caliscope_amd/reliability.py (RELIABILITY_CONSTRAINED_SIGNATURES).
 */
#ifndef CALISCOPE_RELIABILITY_CONSTRAINED_H
#define CALISCOPE_RELIABILITY_CONSTRAINED_H

#include <stdint.h>

#include "reliability.h"
#include "uncertainty_constrained.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every pointer may be NULL: that output is not returned.  Rows are in the CALLER's constraint order; a row of weight 0 is no row of
 * the adjustment and is NaN in all three arrays. */
typedef struct {
  double* redundancy;      /* [n_con] r_j = 1 - P_jj (not clamped) */
  double* w;               /* [n_con] f~_j / (sigma0 sqrt(clamp(r_j, 0, 1))); NaN where r_j <= 1e-10 (REL_R_TINY) */
  double* residual;        /* [n_con] f~_j: weight (|| mean a - mean b || - distance), scaled for the robust loss as scipy scales it */
  int64_t* n_uncontrolled; /* [1] constraint rows of positive weight with r_j <= 1e-10 */
} cba_rel_con_out;

/* Notation of uncertainty_constrained.h: J holds the reprojection rows and the constraint rows of positive weight, all scaled for the
 * loss; V~ = V + C^T C is block-diagonal per component, Y_c = W_c,k V~_k^-1, C = St^-1 with six gauge columns.
 *     G^- = [[ C, -C Y ], [ -Y^T C, V~^-1 + Y^T C Y ]]
 * is a generalised inverse of J^T J, so P = J G^- J^T is the projector and the gauge terms E, F, Z do not appear (the argument of
 * reliability.h).  R = I - P, sum_j r_j = dof = 2 n_obs + n_con - n_params + 6 over ALL rows, sigma0^2 = 2 cost / dof with the
 * constraint rows in the cost.
 *   Observation o (camera a) of a point i in no row: the formula of reliability.h with six gauge columns behind C.
 *   Observation o (camera a) of a point i of component k; e, e' over the (component camera, Yc block) entries of point i:
 *       G_e  = sum_e' C_{cam(e),cam(e')} Yc[e']   (np x 3),      Q_i = sum_e Yc[e]^T G_e,
 *       P_oo = B_o ([V~_k^-1]_ii + Q_i) B_o^T + A_o C_aa A_o^T - A_o G_e(a) B_o^T - (A_o G_e(a) B_o^T)^T,
 *     e(a) the entry of the observation's own camera.  A repeated (camera, point) pair shares one entry and has two output rows.
 *   Constraint row j of component k, c_j = sum_s coef[s] (e_loc[s] (x) u) its scaled Jacobian row, X = L^-1 of V~_k = L L^T:
 *       P_jj = |X c_j^T|^2 + sum_cc' v_c^T C_cc' v_c',   v_c = Y_c c_j^T   (c, c' over the cameras that see the component),
 *       w_j  = f~_j / (sigma0 sqrt(clamp(r_j, 0, 1))).
 *     A row with coincident endpoints has a zero Jacobian row: r_j = 1 exactly.
 * Behind the launches of cba_parameter_covariance_constrained (k_unc_component also leaves |X c_j^T|^2 per row): the point kernel of
 * cba_observation_reliability on the points in no row, a sibling on the points of the components (one wave per point, sixteen lanes per
 * entry, G_e kept in a device store), and one wave per constraint row.  Nothing is added across points or rows in this pass.
 *
 * out->dof / sigma0_sq / cost are those of the constrained adjustment; out->n_uncontrolled counts observation rows, con_out->n_uncontrolled
 * constraint rows.  `out` and `con_out` may each be NULL.  With constraints == NULL, n_con == 0 or every weight 0 the call IS
 * cba_observation_reliability (seven gauge columns, the same launches) and the constraint arrays are all NaN.
 *
 * Refusals are those of cba_parameter_covariance_constrained, under this call's name: indices, weights and distances (CBA_ERR_INVALID),
 * a component of more than COV_COMPONENT_CAP = 54 points, device buffers (this call's stores included) beyond the free device memory,
 * CBA_DETERMINISTIC=1 together with constraint rows (CBA_ERR_UNSUPPORTED), and the numeric ones (CBA_ERR_NUMERIC).  A call that fails
 * a check writes nothing: the arrays are written after the last check. */
int cba_observation_reliability_constrained(const cba_cov_desc* d, const cba_cov_constraints* constraints, int32_t device, cba_rel_out* out,
                                            cba_rel_con_out* con_out);

#ifdef __cplusplus
}
#endif

#endif /* CALISCOPE_RELIABILITY_CONSTRAINED_H */
