/* caliscope_vertical.h — C ABI of the batched gravity fit in libcaliscope_ba.so (caliscope_amd/csrc/vertical_lib.hip).
 *
 * Per-camera vertical estimation (caliscope_amd/vertical.py; the reference's estimators/vertical_solver.py): for every frame the
 * four dense perspective fields of the field network (up direction, its confidence, latitude, its confidence) are fitted by a
 * 2-DOF Levenberg-Marquardt on the unit sphere with the focal lengths fixed.  Conventions are those of caliscope_ba.h: the entry
 * point returns 0 or a negative CBA_ERR_*, cba_last_error() describes a failure, and there is no CPU fallback (without a HIP
 * device: CBA_ERR_NO_DEVICE).  The symbol is bound by caliscope_amd/vertical.py, not by caliscope_amd/_lib.py.
 */
#ifndef CALISCOPE_VERTICAL_H
#define CALISCOPE_VERTICAL_H

#include <stdint.h>

#include "caliscope_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-fit status (status_out). */
enum {
  CBA_VERTICAL_OK = 0,
  CBA_VERTICAL_NONFINITE = 1, /* the cost of the first pass is not finite (NaN or infinity in a field or a confidence) */
  CBA_VERTICAL_SINGULAR = 2   /* the Hessian at the final vector is exactly singular or not finite: no uncertainty exists */
};

/* Fits of different shapes may share a call.  Fit f reads pixels [offset[f], offset[f] + height[f] * width[f]) of every plane,
 * row-major; ranges of different fits may overlap (the planes are only read). */
typedef struct {
  int32_t n_fits;
  int32_t num_steps;      /* LM step budget, 0 allowed (the result is then the start vector's) */
  int64_t n_pixels;       /* length of each of the five planes */
  const int32_t* height;  /* [n_fits] >= 2 */
  const int32_t* width;   /* [n_fits] >= 2 */
  const double* focal_x;  /* [n_fits] > 0, in pixels of the field */
  const double* focal_y;  /* [n_fits] > 0 */
  const int64_t* offset;  /* [n_fits] first pixel of the fit in the planes */
  const void* up_x;       /* [n_pixels] float or double, see is_f32 */
  const void* up_y;
  const void* up_conf;
  const void* lat;        /* latitude in radians */
  const void* lat_conf;
  int32_t is_f32;         /* 1: the planes are float32 (the network's type; widened exactly in the kernels), 0: float64 */
} cba_vertical_desc;

/* fit_out[n_fits][8]: roll, pitch, roll / pitch / gravity uncertainty (radians), initial cost, final cost, stop_step;
 * stop_step_out[n_fits]; status_out[n_fits].  A fit whose status is not CBA_VERTICAL_OK has no valid angles or uncertainties.
 * num_steps + 1 pairs of a partial-sum kernel (one workgroup per fit and chunk of pixels) and an update kernel (one wave per fit)
 * on one stream, no host synchronisation in between; sums in a fixed order and no atomics, so a fit does not depend on the rest of
 * the batch and two runs agree bit for bit.  All shapes, focals and offsets are checked on the host before anything is launched
 * (CBA_ERR_INVALID, the message names the fit).  n_fits == 0 succeeds without a launch. */
int cba_vertical_fit(const cba_vertical_desc* d, int32_t device, double* fit_out, int32_t* stop_step_out, int32_t* status_out);

#ifdef __cplusplus
}
#endif

#endif /* CALISCOPE_VERTICAL_H */
