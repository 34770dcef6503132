// cba_vertical_fit of libcaliscope_ba.so (C ABI: include/caliscope_vertical.h): a batch of 2-DOF gravity fits to perspective fields.
// The per-pixel terms, the serial update, the chunk plan and the host-side checks are vertical_math.h (shared with
// tests/native/vertical_harness.cpp); this file holds the three kernels and the entry point.
//
//   k_vert_sinlat   one thread per pixel of the latitude plane, once per call: sin(latitude) into a float64 plane, so that the
//                   num_steps + 1 passes do not repeat it.
//   k_vert_partial  one 256-thread workgroup per (fit, chunk of VERT_CHUNK_PIXELS pixels).  A thread strides its chunk with the 11
//                   sums in registers (FP64; float32 planes are widened exactly on load), a wave folds them with shuffles in a
//                   fixed order, lane 0 of each wave puts them in LDS, and threads 0 .. 10 add the four waves in order and store
//                   the chunk's partials.  No atomics.  Workgroups of a finished fit return at once.
//   k_vert_update   one wave per fit: lanes 0 .. 10 add the fit's chunk partials in index order, lane 0 runs vert_update (stop test,
//                   damping, the 2 x 2 solve, the step on the sphere, or the final covariance) and writes the fit's state.
//
// One upload per input array; the prologue and num_steps + 1 partial / update pairs on the null stream without a host
// synchronisation; one copy-back of the states.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/caliscope_vertical.h"
#include "device_call.h"
#include "vertical_math.h"

using namespace cba;

namespace {

template <typename T>
__global__ void __launch_bounds__(VERT_BLOCK)
k_vert_sinlat(int64_t n_pixels, const T* __restrict__ lat, double* __restrict__ sin_lat) {
  const int64_t p = (int64_t)blockIdx.x * VERT_BLOCK + threadIdx.x;
  if (p < n_pixels) sin_lat[p] = sin((double)lat[p]);
}

template <typename T>
__global__ void __launch_bounds__(VERT_BLOCK)
k_vert_partial(const int32_t* __restrict__ chunk_fit, const int64_t* __restrict__ first_chunk, const int32_t* __restrict__ height,
               const int32_t* __restrict__ width, const double* __restrict__ focal_x, const double* __restrict__ focal_y,
               const int64_t* __restrict__ offset, const T* __restrict__ up_x, const T* __restrict__ up_y, const T* __restrict__ up_conf,
               const double* __restrict__ sin_lat, const T* __restrict__ lat_conf, const VertState* __restrict__ state, double* __restrict__ partials) {
  __shared__ double s_wave[VERT_BLOCK / VERT_WAVE][VERT_NSUM];
  const int32_t fit = chunk_fit[blockIdx.x];
  if (state[fit].done) return;  // uniform over the workgroup
  const int32_t h = height[fit], w = width[fit];
  const double fx = focal_x[fit], fy = focal_y[fit];
  const int64_t base = offset[fit], n = (int64_t)h * w;
  const int64_t c0 = ((int64_t)blockIdx.x - first_chunk[fit]) * VERT_CHUNK_PIXELS;
  const int64_t c1 = c0 + VERT_CHUNK_PIXELS < n ? c0 + VERT_CHUNK_PIXELS : n;
  const double vec[3] = {state[fit].vec[0], state[fit].vec[1], state[fit].vec[2]};
  double acc[VERT_NSUM];
#pragma unroll
  for (int k = 0; k < VERT_NSUM; ++k) acc[k] = 0.0;
  const int t = threadIdx.x;
  for (int64_t p = c0 + t; p < c1; p += VERT_BLOCK) {
    const int64_t g = base + p;  // < n_pixels: checked on the host
    vert_pixel(h, w, fx, fy, p, (double)up_x[g], (double)up_y[g], (double)up_conf[g], sin_lat[g], (double)lat_conf[g], vec, acc);
  }
#pragma unroll
  for (int k = 0; k < VERT_NSUM; ++k) {
    double v = acc[k];
#pragma unroll
    for (int off = VERT_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, VERT_WAVE);
    acc[k] = v;
  }
  if ((t & (VERT_WAVE - 1)) == 0) {
#pragma unroll
    for (int k = 0; k < VERT_NSUM; ++k) s_wave[t / VERT_WAVE][k] = acc[k];
  }
  __syncthreads();
  if (t < VERT_NSUM) {
    double v = s_wave[0][t];
    for (int wv = 1; wv < VERT_BLOCK / VERT_WAVE; ++wv) v += s_wave[wv][t];
    partials[(int64_t)blockIdx.x * VERT_NSUM + t] = v;
  }
}

__global__ void __launch_bounds__(VERT_WAVE)
k_vert_update(const int64_t* __restrict__ first_chunk, const int32_t* __restrict__ height, const int32_t* __restrict__ width,
              const double* __restrict__ partials, VertState* __restrict__ state, int32_t pass, int32_t num_steps) {
  __shared__ double s[VERT_NSUM];
  const int32_t fit = blockIdx.x;
  if (state[fit].done) return;
  const int64_t n = (int64_t)height[fit] * width[fit];
  const int64_t k0 = first_chunk[fit], k1 = k0 + vert_n_chunks(n);
  const int t = threadIdx.x;
  if (t < VERT_NSUM) {
    double v = partials[k0 * VERT_NSUM + t];
    for (int64_t k = k0 + 1; k < k1; ++k) v += partials[k * VERT_NSUM + t];
    s[t] = v;
  }
  __syncthreads();
  if (t == 0) {
    VertState st = state[fit];
    vert_update(st, s, n, pass, num_steps);
    state[fit] = st;
  }
}

// The planes (float32 or float64: T), the work buffers and the passes of one call; the states come back in `state`.
template <typename T>
void run(Buffers& buf, const cba_vertical_desc* d, const void* const* planes, int64_t total_chunks, const int32_t* dcfit, const int64_t* dfirst,
         const int32_t* dh, const int32_t* dw, const double* dfx, const double* dfy, const int64_t* doff, std::vector<VertState>& state) {
  const T* plane[5];
  for (int k = 0; k < 5; ++k) plane[k] = buf.in((const T*)planes[k], d->n_pixels);
  const T *up_x = plane[0], *up_y = plane[1], *up_conf = plane[2], *lat = plane[3], *lat_conf = plane[4];
  double* dsin = buf.make<double>(d->n_pixels);
  double* dpart = buf.make<double>(total_chunks, VERT_NSUM);
  VertState* dstate = buf.in(state.data(), d->n_fits);
  if (buf.status()) return;
  hipLaunchKernelGGL(k_vert_sinlat<T>, dim3((unsigned)((d->n_pixels + VERT_BLOCK - 1) / VERT_BLOCK)), dim3(VERT_BLOCK), 0, 0, d->n_pixels, lat, dsin);
  hipError_t e = hipGetLastError();
  for (int32_t pass = 0; pass <= d->num_steps && e == hipSuccess; ++pass) {
    hipLaunchKernelGGL(k_vert_partial<T>, dim3((unsigned)total_chunks), dim3(VERT_BLOCK), 0, 0, dcfit, dfirst, dh, dw, dfx, dfy, doff, up_x, up_y, up_conf,
                       dsin, lat_conf, dstate, dpart);
    hipLaunchKernelGGL(k_vert_update, dim3((unsigned)d->n_fits), dim3(VERT_WAVE), 0, 0, dfirst, dh, dw, dpart, dstate, pass, d->num_steps);
    e = hipGetLastError();
  }
  buf.check(e);
  buf.out(state.data(), dstate, d->n_fits);
}

}  // namespace

extern "C" int cba_vertical_fit(const cba_vertical_desc* d, int32_t device, double* fit_out, int32_t* stop_step_out, int32_t* status_out) {
  const char* what = "cba_vertical_fit";
  if (!d) return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  // every index the kernels use, checked on the host before anything reaches the device
  const void* planes[5] = {d->up_x, d->up_y, d->up_conf, d->lat, d->lat_conf};
  std::string msg;
  int rc = vert_validate(d->n_fits, d->num_steps, d->n_pixels, d->height, d->width, d->focal_x, d->focal_y, d->offset, planes, d->is_f32, msg);
  if (rc) return err(rc, msg);
  const int32_t n_fits = d->n_fits;
  if (n_fits == 0) return CBA_OK;
  if (!fit_out || !stop_step_out || !status_out) return err(CBA_ERR_INVALID, std::string(what) + ": null argument");
  // the plan: chunks of every fit, one after the other
  std::vector<int64_t> first((size_t)n_fits);
  std::vector<int32_t> cfit;
  int64_t total = 0;
  for (int32_t f = 0; f < n_fits; ++f) {
    first[f] = total;
    total += vert_n_chunks((int64_t)d->height[f] * d->width[f]);
    if (total > 0x7fffffff) return err(CBA_ERR_UNSUPPORTED, std::string(what) + ": more than 2^31 - 1 pixel chunks in one call");
  }
  cfit.resize((size_t)total);
  for (int32_t f = 0; f < n_fits; ++f) {
    const int64_t end = f + 1 < n_fits ? first[f + 1] : total;
    for (int64_t k = first[f]; k < end; ++k) cfit[k] = f;
  }
  std::vector<VertState> state((size_t)n_fits);
  for (int32_t f = 0; f < n_fits; ++f) vert_state_init(state[f], d->num_steps);

  rc = select_device(device, what);
  if (rc) return rc;
  Buffers buf;
  const int32_t* dcfit = buf.in(cfit.data(), total);
  const int64_t* dfirst = buf.in(first.data(), n_fits);
  const int32_t* dh = buf.in(d->height, n_fits);
  const int32_t* dw = buf.in(d->width, n_fits);
  const double* dfx = buf.in(d->focal_x, n_fits);
  const double* dfy = buf.in(d->focal_y, n_fits);
  const int64_t* doff = buf.in(d->offset, n_fits);
  if (d->is_f32) run<float>(buf, d, planes, total, dcfit, dfirst, dh, dw, dfx, dfy, doff, state);
  else run<double>(buf, d, planes, total, dcfit, dfirst, dh, dw, dfx, dfy, doff, state);
  if (buf.status()) return buf.result(what);
  for (int32_t f = 0; f < n_fits; ++f) {
    for (int k = 0; k < 8; ++k) fit_out[(size_t)f * 8 + k] = state[f].out[k];
    stop_step_out[f] = state[f].stop_step;
    status_out[f] = state[f].status;
  }
  return CBA_OK;
}
