// CPU harness around caliscope_amd/csrc/frame_select_math.h — TEST INFRASTRUCTURE (built by g++ in tests/frame_select_native.py).
// It runs the frame selection with the arithmetic k_frame_features and k_frame_select of pose_lib.hip inline, frame after frame
// and camera after camera (max and min are exact, so a sequential argmax equals the workgroup's), so that the non-GPU suite can
// check it against the reference's fixtures and drive caliscope_amd/frame_selector.py through its `_solver` hook.  It is not a CPU
// fallback: nothing in caliscope_amd/ loads it.
#include <cstdint>
#include <vector>

#include "frame_select_math.h"

using namespace cba;

namespace {

// the ops of fsel_select over the frames of one camera (all arrays start at the camera's first frame)
struct FrameSelHost {
  int nf; const int64_t* fstart; int min_corners;
  const uint64_t* mask; const double* feat; const double* orient;
  uint64_t edge, corner;
  double* dist; int32_t* sel;
  bool eligible(int f) const { return fstart[f + 1] - fstart[f] >= (int64_t)min_corners; }
  uint64_t mask_of(int f) const { return mask[f]; }
  void take(int k, int f) { sel[k] = f; }
  int best_in_bin(int b) {
    double bv = 0.0;
    int bf = -1;
    for (int f = 0; f < nf; ++f)
      if (eligible(f) && fsel_bin(orient + 3 * f) == b && fsel_better(orient[3 * f + 1], f, bv, bf)) { bv = orient[3 * f + 1]; bf = f; }
    return bf;
  }
  void start(const int* anchors, int na) {
    for (int f = 0; f < nf; ++f) dist[f] = fsel_start_dist(feat, f, eligible(f), anchors, na);
  }
  int best_score(int last, uint64_t covered, bool have, double* score) {
    double bv = 0.0;
    int bf = -1;
    for (int f = 0; f < nf; ++f) {
      double s;
      if (fsel_round_item(feat, f, last, mask[f], covered, edge, corner, have, dist + f, &s) && fsel_better(s, f, bv, bf)) { bv = s; bf = f; }
    }
    *score = bv;
    return bf;
  }
};

}  // namespace

extern "C" {

// the homography of one frame: H[9] (h33 = 1), orientation o[3], transfer RMSE; returns the status
int fh_homography(const double* obj, const double* xy, int n, int f32, double* H, double* o, double* rmse) {
  const int st = fsel_homography(obj, xy, n, f32, H, rmse);
  o[0] = o[1] = o[2] = 0.0;
  if (st == FSEL_OK) fsel_orientation_of(H, o);
  return st;
}

// what cba_pose_select_frames computes (homog_start / homog_count: both null for the whole frame); the caller has checked the arguments
void fh_select_frames(int32_t n_cams, const int64_t* cam_frame_start, const double* cam_size, int64_t n_frames, const int64_t* frame_start,
                      const int64_t* homog_start, const int32_t* homog_count, const double* obs_xy, const double* obs_obj, int grid,
                      int min_corners, int target, int f32, uint64_t* mask_out, double* feat_out, double* orient_out, int32_t* status_out,
                      double* rmse_out, int32_t* selected_out, int32_t* n_selected_out, int32_t* n_anchors_out, int32_t* bin_mask_out,
                      int32_t* eligible_out) {
  std::vector<double> dist((size_t)n_frames, 0.0);
  for (int32_t c = 0; c < n_cams; ++c) {
    const int64_t f0 = cam_frame_start[c], f1 = cam_frame_start[c + 1];
    const double w = cam_size[2 * c], h = cam_size[2 * c + 1];
    for (int64_t f = f0; f < f1; ++f) {
      const int64_t a = frame_start[f];
      const int n = (int)(frame_start[f + 1] - a);
      mask_out[f] = fsel_coverage(obs_xy + 2 * a, n, w, h, grid);
      fsel_pose_features(obs_xy + 2 * a, n, w, h, feat_out + 5 * f);
      const int64_t ha = homog_start ? homog_start[f] : a;
      const int hn = homog_start ? homog_count[f] : n;
      status_out[f] = fsel_orientation(obs_obj + 2 * ha, obs_xy + 2 * ha, hn, f32, orient_out + 3 * f, rmse_out + f);
    }
    for (int k = 0; k < target; ++k) selected_out[(int64_t)c * target + k] = -1;
    FrameSelHost ops{(int)(f1 - f0), frame_start + f0, min_corners, mask_out + f0, feat_out + 5 * f0, orient_out + 3 * f0, fsel_edge_mask(grid),
                     fsel_corner_mask(grid), dist.data() + f0, selected_out + (int64_t)c * target};
    int n_el = 0;
    for (int f = 0; f < ops.nf; ++f) n_el += ops.eligible(f) ? 1 : 0;
    int na, bins;
    n_selected_out[c] = fsel_select(ops, target, &na, &bins);
    n_anchors_out[c] = na;
    bin_mask_out[c] = bins;
    eligible_out[c] = n_el;
  }
}

}
