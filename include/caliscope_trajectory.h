/* caliscope_trajectory.h — C ABI of the reconstruction of a recording's 3-D trajectories in libcaliscope_ba.so
 * (caliscope_amd/csrc/trajectory_lib.hip).
 *
 * The per-use stage after calibration (caliscope_amd/reconstruction.py; the reference's reconstruction/reconstruct_xyz.py and the
 * post-processing of core/point_data.py): gap filling of the 2-D tracks, undistortion + DLT triangulation of every (frame,
 * trajectory) slot, gap filling of the 3-D trajectories and the zero-phase Butterworth low-pass, in one call on one dense grid.
 * Conventions are those of caliscope_ba.h: the entry point returns 0 or a negative CBA_ERR_*, cba_last_error() describes a failure,
 * and there is no CPU fallback (without a HIP device: CBA_ERR_NO_DEVICE).  The symbol is bound by caliscope_amd/reconstruction.py,
 * not by caliscope_amd/_lib.py.
 *
 * Data model.  Frame f = sync_index - (smallest sync_index), trajectory j = rank of (object_id, keypoint_id), camera c = rank of
 * cam_id among the cameras of the table; slot s = f * n_traj + j.  The caller passes only the observation rows (camera, slot,
 * pixel, frame time), sorted by (camera, trajectory, frame) and without duplicates; the device scatters them into grids
 * xy[c][s][2] and ft[c][s] that hold NaN where there is no row.
 */
#ifndef CALISCOPE_TRAJECTORY_H
#define CALISCOPE_TRAJECTORY_H

#include <stdint.h>

#include "caliscope_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CBA_TRAJ_MAX_ORDER 8 /* largest filter order */

typedef struct {
  int32_t n_cams;
  int64_t n_frames;
  int64_t n_traj;
  int64_t n_rows;
  const int32_t* cam_model;  /* [n_cams] 0 pinhole (k1 k2 p1 p2 k3), 1 fisheye (k1..k4); read for posed cameras */
  const double* cam_intr;    /* [n_cams][9] fx fy cx cy d0..d4, as cba_triangulate_desc */
  const double* cam_P;       /* [n_cams][12] normalised [R | t], row-major */
  const uint8_t* cam_posed;  /* [n_cams] 1: the camera takes part in the triangulation; 0: its tracks are filled and its frame
                                times count, nothing else */
  const int32_t* row_cam;    /* [n_rows] in [0, n_cams) */
  const int64_t* row_slot;   /* [n_rows] in [0, n_frames * n_traj); (row_cam, slot % n_traj, slot / n_traj) strictly ascending */
  const double* row_xy;      /* [n_rows][2] pixels, finite */
  const double* row_time;    /* [n_rows] frame_time; NaN: the row has none */
  int32_t xy_gap;            /* holes of the 2-D tracks: the first min(hole, xy_gap) frames are filled; <= 0: none */
  int32_t xyz_gap;           /* the same for the 3-D trajectories */
  int32_t float32_io;        /* round pixels and undistorted points to float32 (as cba_triangulate) */
  int32_t filter_order;      /* 1..CBA_TRAJ_MAX_ORDER when filter_b is given */
  const double* filter_b;    /* [filter_order + 1] numerator, or NULL: no smoothing */
  const double* filter_a;    /* [filter_order + 1] denominator, a[0] == 1 */
  const double* filter_zi;   /* [filter_order] steady state of a unit step (scipy.signal.lfilter_zi) */
  int64_t memory_limit;      /* bytes the device buffers of the call may take; 0: what hipMemGetInfo reports as free */
} cba_traj_desc;

/* Every pointer may be NULL: that output is not returned. */
typedef struct {
  double* xyz;         /* [n_slots][3]; NaN where valid == 0 */
  uint8_t* valid;      /* [n_slots] 0: no point; 1: triangulated from two or more posed views; 2: filled by xyz_gap */
  double* slot_time;   /* [n_slots] frame_time of the output row: the frame's mean, interpolated in cells that xyz_gap filled */
  double* frame_time;  /* [n_frames] mean of the frame times of all cells of the frame, real and filled; NaN: none */
  double* xy_filled;   /* [n_cams][n_slots][2] the observation grid after the 2-D fill */
  double* ft_filled;   /* [n_cams][n_slots] the time grid after the 2-D fill */
} cba_traj_out;

/* One call, every launch on one stream:
 *   k_traj_fill2d       one thread per row: its cell, and the first min(hole, xy_gap) cells of the hole behind it, on the straight
 *                       line v_left + (v_right - v_left) * (i / (k + 1.0)) towards the next row of the track (pixels and time).  A
 *                       hole longer than xy_gap still aims at the far neighbour over k + 1 steps, as the reference does.
 *   k_traj_frame_time   one thread per frame: the mean over the non-NaN times of the frame, cameras then trajectories ascending.
 *   k_traj_triangulate  one thread per slot: undistort_one and the DLT of cba_triangulate over the posed cameras, ascending.
 *   k_traj_fill3d       one thread per slot: a triangulated cell followed by a hole fills it as above (xyz and time).
 *   k_traj_filtfilt     one thread per (trajectory, coordinate): scipy.signal.filtfilt with its defaults over the trajectory's
 *                       cells in frame order, holes skipped.  A trajectory of n <= 3 * order cells is left as it is.
 *
 * The result is the same bits from run to run: no atomics, every sum in a fixed order.
 *
 * Checks on the host before anything is launched.  CBA_ERR_INVALID, the message names the row: camera or slot out of range, a
 * pixel that is not finite, rows out of order, two rows of one (camera, frame, trajectory); and the message names the trajectory
 * for a trajectory that would reach the filter with 3 * order < n <= 3 * (order + 1) cells (scipy raises there).
 * CBA_ERR_UNSUPPORTED: a filter order outside 1..CBA_TRAJ_MAX_ORDER, and buffers larger than memory_limit (the message gives both
 * sizes).  n_rows == 0 succeeds without a launch (nothing valid, NaN times). */
int cba_reconstruct_trajectories(const cba_traj_desc* d, int32_t device, cba_traj_out* out);

#ifdef __cplusplus
}
#endif

#endif /* CALISCOPE_TRAJECTORY_H */
