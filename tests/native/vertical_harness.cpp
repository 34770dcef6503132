// CPU harness around caliscope_amd/csrc/vertical_math.h — TEST INFRASTRUCTURE (built by g++ in tests/vertical_native.py).
// It evaluates cba_vertical_fit with the checks, the per-pixel terms, the serial update and the summation order of vertical_lib.hip:
// per pass every (fit, chunk) "workgroup" runs its 256 threads one after the other, folds each wave with the kernel's offsets, adds
// the waves and then the chunks in index order.  The non-GPU suite checks it against the reference's recorded answers and drives
// caliscope_amd.vertical through its `_solver` hook with it.  It is not a CPU fallback: nothing in caliscope_amd/ loads it.
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "vertical_math.h"

using namespace cba;

namespace {
std::string g_error;

template <typename T>
void partial(int32_t h, int32_t w, double fx, double fy, int64_t base, int64_t c0, int64_t c1, const T* up_x, const T* up_y, const T* up_conf,
             const double* sin_lat, const T* lat_conf, const double* vec, double* out) {
  std::vector<double> acc((size_t)VERT_BLOCK * VERT_NSUM, 0.0);
  for (int t = 0; t < VERT_BLOCK; ++t)
    for (int64_t p = c0 + t; p < c1; p += VERT_BLOCK) {
      const int64_t g = base + p;
      vert_pixel(h, w, fx, fy, p, (double)up_x[g], (double)up_y[g], (double)up_conf[g], sin_lat[g], (double)lat_conf[g], vec, &acc[(size_t)t * VERT_NSUM]);
    }
  for (int k = 0; k < VERT_NSUM; ++k) {
    double v = 0.0;
    for (int wv = 0; wv < VERT_BLOCK / VERT_WAVE; ++wv) {
      double lane[VERT_WAVE];
      for (int l = 0; l < VERT_WAVE; ++l) lane[l] = acc[(size_t)(wv * VERT_WAVE + l) * VERT_NSUM + k];
      const double s = vert_fold_wave_serial(lane);
      v = wv == 0 ? s : v + s;
    }
    out[k] = v;
  }
}

template <typename T>
void fit_all(int32_t n_fits, int32_t num_steps, int64_t n_pixels, const int32_t* height, const int32_t* width, const double* focal_x, const double* focal_y,
             const int64_t* offset, const void* const* planes, std::vector<VertState>& state) {
  const T* up_x = (const T*)planes[0];
  const T* up_y = (const T*)planes[1];
  const T* up_conf = (const T*)planes[2];
  const T* lat = (const T*)planes[3];
  const T* lat_conf = (const T*)planes[4];
  std::vector<double> sin_lat((size_t)n_pixels);
  for (int64_t p = 0; p < n_pixels; ++p) sin_lat[p] = std::sin((double)lat[p]);  // k_vert_sinlat
  for (int32_t pass = 0; pass <= num_steps; ++pass)
    for (int32_t f = 0; f < n_fits; ++f) {
      if (state[f].done) continue;
      const int64_t n = (int64_t)height[f] * width[f];
      double s[VERT_NSUM], part[VERT_NSUM];
      for (int64_t c = 0; c < vert_n_chunks(n); ++c) {  // k_vert_partial, then the chunk sum of k_vert_update
        const int64_t c0 = c * VERT_CHUNK_PIXELS, c1 = c0 + VERT_CHUNK_PIXELS < n ? c0 + VERT_CHUNK_PIXELS : n;
        partial<T>(height[f], width[f], focal_x[f], focal_y[f], offset[f], c0, c1, up_x, up_y, up_conf, sin_lat.data(), lat_conf, state[f].vec, part);
        for (int k = 0; k < VERT_NSUM; ++k) s[k] = c == 0 ? part[k] : s[k] + part[k];
      }
      vert_update(state[f], s, n, pass, num_steps);
    }
}
}  // namespace

extern "C" {

const char* vh_last_error() { return g_error.c_str(); }

// VERT_CHUNK_PIXELS, VERT_BLOCK, VERT_WAVE, VERT_NSUM, VERT_MAX_SIDE, VERT_MAX_STEPS
void vh_constants(int32_t* out) {
  out[0] = VERT_CHUNK_PIXELS; out[1] = VERT_BLOCK; out[2] = VERT_WAVE; out[3] = VERT_NSUM; out[4] = VERT_MAX_SIDE; out[5] = VERT_MAX_STEPS;
}

int64_t vh_n_chunks(int64_t n_pixels) { return vert_n_chunks(n_pixels); }

void vh_gravity_vec(double roll, double pitch, double* vec) { vert_gravity_vec(roll, pitch, vec); }
void vh_roll_pitch(const double* vec, double* out) { vert_roll_pitch(vec, out[0], out[1]); }

// cba_vertical_fit on the host: 0 or -1 (invalid) with vh_last_error() set
int vh_vertical_fit(int32_t n_fits, int32_t num_steps, int64_t n_pixels, const int32_t* height, const int32_t* width, const double* focal_x,
                    const double* focal_y, const int64_t* offset, const void* up_x, const void* up_y, const void* up_conf, const void* lat,
                    const void* lat_conf, int32_t is_f32, double* fit_out, int32_t* stop_step_out, int32_t* status_out) {
  const void* planes[5] = {up_x, up_y, up_conf, lat, lat_conf};
  const int rc = vert_validate(n_fits, num_steps, n_pixels, height, width, focal_x, focal_y, offset, planes, is_f32, g_error);
  if (rc) return rc;
  if (n_fits == 0) return 0;
  std::vector<VertState> state((size_t)n_fits);
  for (int32_t f = 0; f < n_fits; ++f) vert_state_init(state[f], num_steps);
  if (is_f32) fit_all<float>(n_fits, num_steps, n_pixels, height, width, focal_x, focal_y, offset, planes, state);
  else fit_all<double>(n_fits, num_steps, n_pixels, height, width, focal_x, focal_y, offset, planes, state);
  for (int32_t f = 0; f < n_fits; ++f) {
    for (int k = 0; k < 8; ++k) fit_out[(size_t)f * 8 + k] = state[f].out[k];
    stop_step_out[f] = state[f].stop_step;
    status_out[f] = state[f].status;
  }
  return 0;
}

}
