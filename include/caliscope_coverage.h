/* caliscope_coverage.h — C ABI of the camera-pair coverage count in libcaliscope_ba.so (caliscope_amd/csrc/coverage_lib.hip).
 *
 * The pre-flight check of a calibration session (caliscope_amd/coverage_analysis.py; the reference's core/coverage_analysis.py):
 * how many observation keys (sync_index, object_id, keypoint_id) every pair of cameras shares.  Conventions are those of
 * caliscope_ba.h: the entry point returns 0 or a negative CBA_ERR_*, cba_last_error() describes a failure, and there is no CPU
 * fallback (without a HIP device: CBA_ERR_NO_DEVICE).  The symbol is bound by caliscope_amd/coverage_analysis.py, not by
 * caliscope_amd/_lib.py.
 */
#ifndef CALISCOPE_COVERAGE_H
#define CALISCOPE_COVERAGE_H

#include <stdint.h>

#include "caliscope_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Observations in any order; a key is the caller's dense or compressed index of (sync_index, object_id, keypoint_id). */
typedef struct {
  int32_t n_cams;
  int64_t n_keys;
  int64_t n_obs;
  const int64_t* obs_key; /* [n_obs] in [0, n_keys) */
  const int32_t* obs_cam; /* [n_obs] camera index in [0, n_cams), or -1: a camera outside the caller's map, skipped */
  int64_t slab_words;     /* 64-bit words of the key range handled per pass and camera; 0: the library's default (a bit table of
                             256 MiB per pass).  Any value gives the same counts: tests force several passes on small inputs with it. */
} cba_coverage_desc;

/* counts_out[n_cams][n_cams], symmetric: [i][j] = number of keys seen by both camera i and camera j, [i][i] = number of distinct
 * keys of camera i (repeated rows count once).  Two kernels per pass over the key range, no sort: every observation sets its bit
 * in a table of one bit row per camera, then popcount(row_i & row_j) is summed per camera pair; integer sums, so the result does
 * not change from run to run.  Every key and camera index is checked on the host before anything is launched: one outside its
 * range is CBA_ERR_INVALID and the message names the observation; more than 32 768 cameras is CBA_ERR_UNSUPPORTED.  n_cams == 0
 * or n_obs == 0 succeeds (zero matrix) without a launch. */
int cba_coverage_counts(const cba_coverage_desc* d, int32_t device, int64_t* counts_out);

#ifdef __cplusplus
}
#endif

#endif /* CALISCOPE_COVERAGE_H */
