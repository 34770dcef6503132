/* caliscope/trajectory_smoother.h — C ABI of the covariance-weighted fixed-interval smoother of reconstructed trajectories in
 * libcaliscope_ba.so (caliscope_amd/csrc/trajectory_lib.hip, caliscope_amd/csrc/trajectory_smooth_math.h).
 *
 * cba_reconstruct_trajectories_uncertain (trajectory_uncertainty.h) gives every sample its 3 x 3 covariance.  The Butterworth filter
 * of the call (k_traj_filtfilt) does not use it: it weights every sample alike, coordinate by coordinate, fills no hole, returns no
 * velocity and leaves the covariance behind.  k_traj_smooth is the smoother that uses it: per trajectory the exact posterior mean
 * and covariance of position and velocity at every frame under the model below, holes included.  There is no CPU fallback.  The
 * symbols are bound by caliscope_amd/trajectory_smoother.py.
 *
 * Model.  Per trajectory j over the frames f of the grid (consecutive sync_index), dt = 1 / fps, slot s = f n_traj + j:
 *     state        x = (p, v) in R^6
 *     transition   x_{f+1} = F x_f + w,  F = [[I, dt I], [0, I]]
 *     process      w ~ N(0, Q),  Q = q^2 [[dt^3/3 I, dt^2/2 I], [dt^2/2 I, dt I]]: white-noise acceleration of density q = accel_density
 *                  in world units / s^1.5
 *     measurement  a measured frame has z = xyz[s] = H x + e, H = [I 0], e ~ N(0, R), R = meas_cov[s] (in the reconstruction:
 *                  cov_noise[s] = sigma_px^2 V^-1 of trajectory_uncertainty.h, the sample before any fill or filter)
 *     span         from the first measured frame f0 of the trajectory to the last, f1
 *     start        at f0: x = (z, 0), P = diag(R, sv0^2 I), sv0 = velocity_prior_std: a proper prior on the initial velocity, none on
 *                  the position
 * A frame inside the span without a measurement is a prediction-only step; the recursion runs through holes of any length.  A
 * trajectory without a measured frame produces nothing.
 *
 * Recursion.  Forward the Kalman filter: x^- = F x, P^- = F P F^T + Q; at a measured frame y = z - p^-, S = P^-_pp + R, S^-1 through
 * chol3 of ba_math.h, u = S^-1 y, nis = y^T u, and with P^- = [[A, B], [B^T, C]]
 *     x = x^- + [A; B^T] u,   P = [[R S^-1 A, R S^-1 B], [., C - B^T S^-1 B]]
 * (I - K H = [[R S^-1, 0], [-B^T S^-1, I]]: products, where I - A S^-1 would be the difference of two nearly equal matrices when the
 * prediction is much less certain than the sample).  Backward the modified Bryson-Frazier form on the filtered pairs, which needs
 * S^-1 alone and no 6 x 6 solve: with the adjoint pair lambda (6), Lambda (6 x 6 symmetric), zero behind f1,
 *     smoothed x = x - P lambda,   smoothed P = P - P Lambda P
 *     at a measured frame other than f0, G = (I - K H)^T = [[S^-1 R, -S^-1 B], [0, I]]:
 *         lambda <- G lambda - H^T u,   Lambda <- G Lambda G^T + H^T S^-1 H
 *     lambda <- F^T lambda,   Lambda <- F^T Lambda F
 * One thread per trajectory runs both passes: a serial recurrence like k_traj_filtfilt, bound by latency, not by throughput.
 * Symmetric matrices are held as their upper triangles (P as the blocks A (6), B (9), C (6)), every index a constant after
 * unrolling.  The forward pass parks, per slot of the span, the filtered x (6) and P (21) and, at a measured frame, u (3), S^-1 (6)
 * and N = -S^-1 B (9): 45 doubles, 360 bytes, component-major ([45][n_slots]) so that the accesses of a wave, whose lanes are
 * neighbouring trajectories of one frame, are consecutive.  R is read again in the backward pass.  The loads of the next frame
 * (z, R and the flag forward; the parked rows backward) are issued before the arithmetic of the current one.
 *
 * Limits.  meas_cov is the noise term alone.  The calibration error (cov_calib of trajectory_uncertainty.h) is common to all frames,
 * does not average out over time, and is not carried through the recursion: the smoothed covariance is the noise part, and the
 * sample's cov_calib stands beside it unchanged (caliscope_amd.trajectory_smoother.smoothed_frame: as it is for status 1, NaN for
 * status 2).  There is no innovation gating (the refinement rejects views before the smoother sees a sample), the frame times are
 * 1 / fps apart, and nothing is parallel in time or spread over devices.  With velocity_prior_std far above the velocities in the
 * data the velocity covariance of the first frames loses digits to cancellation (4e-6 relative at 100, world units of metres);
 * the default of the Python layer is 10.
 *
 * The result is the same bits from run to run: no atomics, one thread per trajectory, a fixed order.
 */
#ifndef CALISCOPE_TRAJECTORY_SMOOTHER_H
#define CALISCOPE_TRAJECTORY_SMOOTHER_H

#include <stdint.h>

#include "trajectory_uncertainty.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The model.  All three reals finite and positive, max_gap >= 0. */
typedef struct {
  double fps;                /* frames per second: dt = 1 / fps */
  double accel_density;      /* q, world units / s^1.5 */
  double velocity_prior_std; /* sv0, world units / s */
  int32_t max_gap;           /* an unmeasured frame gets a row (status 2) when its hole is at most this many frames long */
} cba_traj_smoother;

/* The smoother alone, on the caller's points. */
typedef struct {
  int64_t n_frames;
  int64_t n_traj;          /* n_slots = n_frames n_traj, slot s = f n_traj + j */
  const double* xyz;       /* [n_slots][3]; read where measured */
  const double* meas_cov;  /* [n_slots][6] xx xy xz yy yz zz; read where measured */
  const uint8_t* measured; /* [n_slots] 1: measured; anything else: not */
  double fps;              /* the model, as cba_traj_smoother */
  double accel_density;
  double velocity_prior_std;
  int32_t max_gap;
  int64_t memory_limit;    /* bytes the device buffers may take; 0: the free device memory */
} cba_smooth_desc;

/* Every pointer may be NULL.  status: 0 nothing (outside the span, or inside a hole longer than max_gap), 1 measured and smoothed,
 * 2 interpolated (an unmeasured frame inside a hole of at most max_gap frames between two measured ones).  Rows of status 0 are
 * NaN, rows of status 1 and 2 never. */
typedef struct {
  double* pos;      /* [n_slots][3] */
  double* vel;      /* [n_slots][3] */
  double* pos_cov;  /* [n_slots][6] */
  double* vel_cov;  /* [n_slots][6] */
  double* nis;      /* [n_slots] y^T S^-1 y of the forward pass at a measured frame; NaN at f0 and at an unmeasured frame */
  uint8_t* status;  /* [n_slots] */
  double* meas_cov; /* [n_slots][6] cba_reconstruct_trajectories_smoothed only: the R it used, cov_noise where cov_status == 1, NaN
                       elsewhere; cba_smooth_trajectories does not write it */
} cba_traj_smooth_out;

/* Host checks before any launch, the offender named.  CBA_ERR_INVALID: a null desc or out, a negative size, n_slots > 0 with a null
 * input; fps, accel_density or velocity_prior_std not finite or not positive; max_gap < 0; a measured slot whose point is not
 * finite, or whose meas_cov is not finite or has no positive chol3 pivots.  CBA_ERR_UNSUPPORTED: the device buffers, 586 n_slots
 * bytes (xyz 24, meas_cov 48, measured 1; the outputs 153; the parked rows 360), exceed memory_limit.  n_slots == 0, or no measured
 * slot, succeeds without a launch (NaN, status 0). */
int cba_smooth_trajectories(const cba_smooth_desc* desc, int32_t device, cba_traj_smooth_out* out);

/* cba_reconstruct_trajectories_uncertain with k_traj_smooth behind k_traj_cov: measured iff cov_status == 1 (a slot of status 2 is
 * unmeasured), z the point of the call, R the noise term, which k_traj_cov stores in a buffer of its own before it adds the
 * calibration term (it is never formed as cov - cov_calib).  out, quality and cov_out are the bytes of the uncertain call.  Further
 * checks, CBA_ERR_INVALID with the offender named: smoother or smooth_out null; the reals and max_gap as above; xyz_gap > 0 or a
 * filter in the same call (the smoother does both jobs).  uncertainty is required as in the uncertain call.  The memory check counts
 * 561 n_slots bytes more than the uncertain call (meas_cov 48, the outputs 153, the parked rows 360).  n_rows == 0 succeeds
 * without a launch. */
int cba_reconstruct_trajectories_smoothed(const cba_traj_desc* d, const cba_traj_refine* refine, const cba_traj_uncertainty* uncertainty,
                                          const cba_traj_smoother* smoother, int32_t device, cba_traj_out* out, cba_traj_quality* quality,
                                          cba_traj_cov_out* cov_out, cba_traj_smooth_out* smooth_out);

#ifdef __cplusplus
}
#endif

#endif /* CALISCOPE_TRAJECTORY_SMOOTHER_H */
