// Frame selection for the intrinsic calibration (reference core/frame_selector.py): the arithmetic of
// caliscope_amd/frame_selector.py, host + device inline functions.  hipcc compiles it into k_frame_features and k_frame_select of
// pose_lib.hip; g++ compiles it into tests/native/frame_select_harness.cpp.
//
// Per frame (one thread per frame on the device), all from the frame's n rows of pixels xy[n][2] and board points obj[n][2]:
//   coverage     fsel_coverage: bit row * g + col of every cell of the g x g grid (g <= FSEL_MAX_GRID) a corner falls in,
//                cell = clamp((int)(x / (width / g)), 0, g - 1) on the float64 pixels (corners outside the image: border cells).
//   pose         fsel_pose_features: centroid / size, sample standard deviation (ddof = 1) / size (0 for a single corner),
//                aspect = spread_x / spread_y (1 when spread_y <= 1e-6); float64 pixels, summed in row order.
//   orientation  fsel_orientation over the frame's homography subrange: board x, y normalised to [0, 1] over the subrange's own
//                min / max (a range below 1e-6 is 1), with f32 both inputs rounded to float32 and min, range, subtraction and
//                division done in float, as the reference's float32 arrays; then the homography of the pixel transfer error
//                sum |proj(H (X, Y, 1)) - u|^2 in double: DLT on centred, scaled points (homog_dlt_add of pnp_math.h, h33 = 1 in
//                those coordinates), Levenberg-Marquardt on the 8 free entries in the same coordinates (an isotropic scale of
//                the pixels does not move the minimum) until an accepted step is below FSEL_STEP_TOL relative, the damping
//                exceeds 1e16 or FSEL_LM_MAX_ITER iterations, then at most FSEL_POLISH_ITER undamped steps while each is less
//                than half the one before (as pnp_refine).  H is scaled so that h33 = 1; tilt_direction = atan2(h32, h31) in
//                [0, 2 pi), tilt_magnitude = sqrt(h31^2 + h32^2), in_plane_rotation = the angle of the orthogonal polar factor
//                of A = H[:2, :2] in closed form: atan2(a21 - a12, a11 + a22) for det A >= 0; a reflection for det A < 0, of
//                which the reference reads atan2(R[1, 0], R[0, 0]) = atan2(a21 + a12, a11 - a22).  Also the transfer RMSE in
//                pixels, sqrt(sum / n).  FSEL_TOO_FEW (fewer than 4 corners) and FSEL_FAILED (no spread of the points, singular
//                normal equations, non-finite result, h33 = 0) give three zeros and rmse 0: no NaN leaves this file.
//
// Per camera (one workgroup per camera on the device): fsel_select is a template over an OPS object that owns the camera's frames
// (the pattern of intr_calibrate); every thread of a workgroup calls it with the same arguments and gets the same answers.
//   best_in_bin(b)                    the eligible frame of tilt bin b with the largest tilt magnitude, lowest frame on ties; -1
//   start(anchors, na)                running distance of every frame: fsel_start_dist
//   best_score(last, covered, have, &score)   folds frame `last` (-1: none) into the running distances, scores every
//                                     remaining frame (fsel_round_item) and returns the best, lowest frame on ties; -1: none left
//   mask_of(f), take(k, f)            a frame's cell mask; selection slot k = frame f
// Frames of a camera are numbered from 0 in ascending sync_index, so "lowest frame" is the reference's "lowest sync_index".
// The running distance of a frame is +inf while nothing is selected, its distance in the 5 pose features to the nearest selected
// frame afterwards (min is exact: equal to recomputing it over all selected frames), and FSEL_TAKEN (-1) once it is selected or
// when it is not eligible.
#pragma once
#include "pnp_math.h"

// no contraction, as pnp_math.h: the device then rounds as the g++ build does
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace cba {

constexpr int FSEL_OK = 0;
constexpr int FSEL_TOO_FEW = 1;
constexpr int FSEL_FAILED = 2;
constexpr int FSEL_MAX_GRID = 8;
constexpr int FSEL_BINS = 8;                 // 45 degree sectors of the tilt direction
constexpr int FSEL_MIN_HOMOG_POINTS = 4;
constexpr double FSEL_MIN_TILT = 0.1;        // below it a board is frontal: no bin
constexpr double FSEL_MIN_SCORE = 0.01;      // the greedy phase stops below it
constexpr double FSEL_EDGE_WEIGHT = 0.2, FSEL_CORNER_WEIGHT = 0.3, FSEL_DIVERSITY_WEIGHT = 0.3;
constexpr double FSEL_TAKEN = -1.0;
constexpr int FSEL_LM_MAX_ITER = 60;
constexpr int FSEL_POLISH_ITER = 6;
constexpr double FSEL_STEP_TOL = 1e-12;
constexpr double FSEL_TWO_PI = 6.283185307179586;  // 2 * M_PI, the reference's 2 * np.pi

CBA_HD int fsel_cell(double x, double cell, int g) {
  const double q = x / cell;
  if (!(q > 0.0)) return 0;
  return q >= (double)(g - 1) ? g - 1 : (int)q;
}

CBA_HD uint64_t fsel_coverage(const double* xy, int n, double width, double height, int g) {
  const double cw = width / (double)g, ch = height / (double)g;
  uint64_t mask = 0;
  for (int i = 0; i < n; ++i) mask |= (uint64_t)1 << (fsel_cell(xy[2 * i + 1], ch, g) * g + fsel_cell(xy[2 * i], cw, g));
  return mask;
}

// cells of the border rows and columns / the four corner cells of the g x g grid
CBA_HD uint64_t fsel_edge_mask(int g) {
  uint64_t m = 0;
  for (int r = 0; r < g; ++r)
    for (int c = 0; c < g; ++c)
      if (r == 0 || r == g - 1 || c == 0 || c == g - 1) m |= (uint64_t)1 << (r * g + c);
  return m;
}

CBA_HD uint64_t fsel_corner_mask(int g) {
  return ((uint64_t)1 << 0) | ((uint64_t)1 << (g - 1)) | ((uint64_t)1 << ((g - 1) * g)) | ((uint64_t)1 << ((g - 1) * g + g - 1));
}

CBA_HD void fsel_pose_features(const double* xy, int n, double width, double height, double* f) {
  double sx = 0.0, sy = 0.0;
  for (int i = 0; i < n; ++i) { sx += xy[2 * i]; sy += xy[2 * i + 1]; }
  const double mx = n > 0 ? sx / (double)n : 0.0, my = n > 0 ? sy / (double)n : 0.0;
  double spx = 0.0, spy = 0.0;
  if (n > 1) {
    double vx = 0.0, vy = 0.0;
    for (int i = 0; i < n; ++i) {
      const double dx = xy[2 * i] - mx, dy = xy[2 * i + 1] - my;
      vx += dx * dx;
      vy += dy * dy;
    }
    spx = sqrt(vx / (double)(n - 1)) / width;
    spy = sqrt(vy / (double)(n - 1)) / height;
  }
  f[0] = mx / width;
  f[1] = my / height;
  f[2] = spx;
  f[3] = spy;
  f[4] = spy > 1e-6 ? spx / spy : 1.0;
}

// Normalisation of the board coordinates of one homography subrange: lo[2] and range[2] (double copies of the float values when f32).
CBA_HD void fsel_board_range(const double* obj, int n, int f32, double* lo, double* range) {
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (f32) {
      float a = (float)obj[k], b = a;
      for (int i = 1; i < n; ++i) {
        const float v = (float)obj[2 * i + k];
        a = v < a ? v : a;
        b = v > b ? v : b;
      }
      float r = b - a;
      if (r < 1e-6f) r = 1.0f;
      lo[k] = (double)a;
      range[k] = (double)r;
    } else {
      double a = obj[k], b = a;
      for (int i = 1; i < n; ++i) {
        const double v = obj[2 * i + k];
        a = v < a ? v : a;
        b = v > b ? v : b;
      }
      double r = b - a;
      if (r < 1e-6) r = 1.0;
      lo[k] = a;
      range[k] = r;
    }
  }
}

// Corner i as the fit sees it: normalised board point X[2] and pixel u[2].
CBA_HD void fsel_load(const double* obj, const double* xy, int i, int f32, const double* lo, const double* range, double* X, double* u) {
  if (f32) {
    X[0] = (double)(((float)obj[2 * i] - (float)lo[0]) / (float)range[0]);
    X[1] = (double)(((float)obj[2 * i + 1] - (float)lo[1]) / (float)range[1]);
    u[0] = (double)(float)xy[2 * i];
    u[1] = (double)(float)xy[2 * i + 1];
  } else {
    X[0] = (obj[2 * i] - lo[0]) / range[0];
    X[1] = (obj[2 * i + 1] - lo[1]) / range[1];
    u[0] = xy[2 * i];
    u[1] = xy[2 * i + 1];
  }
}

// Where the fit runs: board points (X - oc) / so, pixels (u - ic) / si.
struct FselFrame {
  const double* obj; const double* xy; int n; int f32;
  double lo[2], range[2], oc[2], ic[2], io, ii;
};

CBA_HD void fsel_scaled(const FselFrame& fr, int i, double* x, double* y, double* uu, double* vv) {
  double X[2], u[2];
  fsel_load(fr.obj, fr.xy, i, fr.f32, fr.lo, fr.range, X, u);
  *x = (X[0] - fr.oc[0]) * fr.io;
  *y = (X[1] - fr.oc[1]) * fr.io;
  *uu = (u[0] - fr.ic[0]) * fr.ii;
  *vv = (u[1] - fr.ic[1]) * fr.ii;
}

// Transfer cost of h (h33 = 1) in the scaled coordinates; with want_normal also J^T J (packed 8 x 8) and -J^T r.
template <bool want_normal>
CBA_HD double fsel_homog_cost(const FselFrame& fr, const double* h, double* JtJ, double* g) {
  if (want_normal) {
#pragma unroll
    for (int k = 0; k < 36; ++k) JtJ[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) g[k] = 0.0;
  }
  double cost = 0.0;
  for (int i = 0; i < fr.n; ++i) {
    double x, y, uu, vv;
    fsel_scaled(fr, i, &x, &y, &uu, &vv);
    const double iw = 1.0 / (h[6] * x + h[7] * y + 1.0);
    const double pu = (h[0] * x + h[1] * y + h[2]) * iw, pv = (h[3] * x + h[4] * y + h[5]) * iw;
    const double ru = pu - uu, rv = pv - vv;
    cost += ru * ru + rv * rv;
    if (want_normal) {
      const double xw = x * iw, yw = y * iw;
      const double ju[8] = {xw, yw, iw, 0.0, 0.0, 0.0, -pu * xw, -pu * yw};
      const double jv[8] = {0.0, 0.0, 0.0, xw, yw, iw, -pv * xw, -pv * yw};
      normal_add<8>(JtJ, g, ju, -ru);
      normal_add<8>(JtJ, g, jv, -rv);
    }
  }
  return cost;
}

// Least-squares homography of one frame's subrange: H[9] row-major with h33 = 1 (board coordinates normalised to [0, 1]), rmse in pixels.
CBA_HD int fsel_homography(const double* obj, const double* xy, int n, int f32, double* H, double* rmse) {
  *rmse = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) H[k] = 0.0;
  if (n < FSEL_MIN_HOMOG_POINTS) return FSEL_TOO_FEW;
  FselFrame fr;
  fr.obj = obj; fr.xy = xy; fr.n = n; fr.f32 = f32;
  fsel_board_range(obj, n, f32, fr.lo, fr.range);
  double oc[2] = {0.0, 0.0}, ic[2] = {0.0, 0.0};
  for (int i = 0; i < n; ++i) {
    double X[2], u[2];
    fsel_load(obj, xy, i, f32, fr.lo, fr.range, X, u);
    oc[0] += X[0]; oc[1] += X[1];
    ic[0] += u[0]; ic[1] += u[1];
  }
  const double inv_n = 1.0 / (double)n;
  fr.oc[0] = oc[0] * inv_n; fr.oc[1] = oc[1] * inv_n;
  fr.ic[0] = ic[0] * inv_n; fr.ic[1] = ic[1] * inv_n;
  double so = 0.0, si = 0.0;  // mean distances from the centroids
  for (int i = 0; i < n; ++i) {
    double X[2], u[2];
    fsel_load(obj, xy, i, f32, fr.lo, fr.range, X, u);
    so += sqrt((X[0] - fr.oc[0]) * (X[0] - fr.oc[0]) + (X[1] - fr.oc[1]) * (X[1] - fr.oc[1]));
    si += sqrt((u[0] - fr.ic[0]) * (u[0] - fr.ic[0]) + (u[1] - fr.ic[1]) * (u[1] - fr.ic[1]));
  }
  so *= inv_n;
  si *= inv_n;
  if (!(so > 0.0) || !(si > 0.0) || !pnp_finite(so) || !pnp_finite(si)) return FSEL_FAILED;
  fr.io = 1.0 / so;
  fr.ii = 1.0 / si;
  double JtJ[36], g[8], h[8];
#pragma unroll
  for (int k = 0; k < 36; ++k) JtJ[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k) h[k] = 0.0;
  for (int i = 0; i < n; ++i) {
    double x, y, uu, vv;
    fsel_scaled(fr, i, &x, &y, &uu, &vv);
    homog_dlt_add(JtJ, h, x, y, uu, vv);
  }
  if (!chol_solve<8>(JtJ, h)) return FSEL_FAILED;
  // Levenberg-Marquardt from the DLT start; a rejected step keeps the linearisation, an accepted one renews it
  double cost = fsel_homog_cost<true>(fr, h, JtJ, g);
  if (!pnp_finite(cost)) return FSEL_FAILED;
  double mu = 1e-3;
  for (int it = 0; it < FSEL_LM_MAX_ITER; ++it) {
    double A[36], d[8];
    double dmax = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) dmax = fmax(dmax, JtJ[k * (k + 1) / 2 + k]);
#pragma unroll
    for (int k = 0; k < 36; ++k) A[k] = JtJ[k];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      A[k * (k + 1) / 2 + k] += mu * fmax(JtJ[k * (k + 1) / 2 + k], 1e-12 * dmax);
      d[k] = g[k];
    }
    if (chol_solve<8>(A, d)) {
      double hn[8], step = 0.0, size = 1.0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        hn[k] = h[k] + d[k];
        step = fmax(step, fabs(d[k]));
        size = fmax(size, fabs(h[k]));
      }
      const double cn = fsel_homog_cost<false>(fr, hn, A, d);
      if (pnp_finite(cn) && cn < cost) {
#pragma unroll
        for (int k = 0; k < 8; ++k) h[k] = hn[k];
        cost = fsel_homog_cost<true>(fr, h, JtJ, g);
        mu = fmax(mu * 0.1, 1e-15);
        if (step <= FSEL_STEP_TOL * size) break;
        continue;
      }
    }
    mu *= 10.0;
    if (mu > 1e16) break;
  }
  double prev = 1e300;
  for (int it = 0; it < FSEL_POLISH_ITER; ++it) {
    double A[36], d[8], hn[8];
#pragma unroll
    for (int k = 0; k < 36; ++k) A[k] = JtJ[k];
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = g[k];
    if (!chol_solve<8>(A, d)) break;
    double dn = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      dn = fmax(dn, fabs(d[k]));
      hn[k] = h[k] + d[k];
    }
    if (!(dn < 0.5 * prev) || dn == 0.0) break;
    const double cn = fsel_homog_cost<false>(fr, hn, A, d);
    if (!pnp_finite(cn) || cn > cost * (1.0 + 1e-10)) break;
#pragma unroll
    for (int k = 0; k < 8; ++k) h[k] = hn[k];
    const double cl = fsel_homog_cost<true>(fr, h, JtJ, g);
    cost = cl < cost ? cl : cost;
    prev = dn;
  }
  // back to normalised board coordinates and pixels: H = Ti^-1 Hn To, To = [io 0 -oc_x io; 0 io -oc_y io; 0 0 1], Ti^-1 = [si 0 ic_x; 0 si ic_y; 0 0 1]
  double M[9];
  M[0] = si * h[0] + fr.ic[0] * h[6]; M[1] = si * h[1] + fr.ic[0] * h[7]; M[2] = si * h[2] + fr.ic[0];
  M[3] = si * h[3] + fr.ic[1] * h[6]; M[4] = si * h[4] + fr.ic[1] * h[7]; M[5] = si * h[5] + fr.ic[1];
  M[6] = h[6];                        M[7] = h[7];                        M[8] = 1.0;
  double G[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    G[3 * r] = M[3 * r] * fr.io;
    G[3 * r + 1] = M[3 * r + 1] * fr.io;
    G[3 * r + 2] = M[3 * r + 2] - (M[3 * r] * fr.oc[0] + M[3 * r + 1] * fr.oc[1]) * fr.io;
  }
  const double h33 = G[8];
  bool fin = pnp_finite(h33) && h33 != 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    G[k] = G[k] / h33;
    fin = fin && pnp_finite(G[k]);
  }
  if (!fin) return FSEL_FAILED;
  double sum = 0.0;
  for (int i = 0; i < n; ++i) {
    double X[2], u[2];
    fsel_load(obj, xy, i, f32, fr.lo, fr.range, X, u);
    const double w = G[6] * X[0] + G[7] * X[1] + G[8];
    const double ru = (G[0] * X[0] + G[1] * X[1] + G[2]) / w - u[0], rv = (G[3] * X[0] + G[4] * X[1] + G[5]) / w - u[1];
    sum += ru * ru + rv * rv;
  }
  const double r = sqrt(sum * inv_n);
  if (!pnp_finite(r)) return FSEL_FAILED;
#pragma unroll
  for (int k = 0; k < 9; ++k) H[k] = G[k];
  *rmse = r;
  return FSEL_OK;
}

CBA_HD double fsel_wrap(double a) { return a < 0.0 ? a + FSEL_TWO_PI : a; }

// tilt_direction, tilt_magnitude, in_plane_rotation of a homography with h33 = 1
CBA_HD void fsel_orientation_of(const double* H, double* o) {
  o[0] = fsel_wrap(atan2(H[7], H[6]));
  o[1] = sqrt(H[6] * H[6] + H[7] * H[7]);
  const double det = H[0] * H[4] - H[1] * H[3];
  o[2] = det < 0.0 ? fsel_wrap(atan2(H[3] + H[1], H[0] - H[4])) : fsel_wrap(atan2(H[3] - H[1], H[0] + H[4]));
}

// Orientation features o[3] and transfer RMSE of one frame's homography subrange; returns the status.
CBA_HD int fsel_orientation(const double* obj, const double* xy, int n, int f32, double* o, double* rmse) {
  double H[9];
  const int st = fsel_homography(obj, xy, n, f32, H, rmse);
  o[0] = o[1] = o[2] = 0.0;
  if (st != FSEL_OK) return st;
  fsel_orientation_of(H, o);
  if (!pnp_finite(o[0]) || !pnp_finite(o[1]) || !pnp_finite(o[2])) {
    o[0] = o[1] = o[2] = 0.0;
    *rmse = 0.0;
    return FSEL_FAILED;
  }
  return FSEL_OK;
}

// ---- per camera ----------------------------------------------------------------------------------------------------------------

// the tilt bin of a frame, -1 for a frontal board
CBA_HD int fsel_bin(const double* o) {
  if (o[1] < FSEL_MIN_TILT) return -1;
  const int b = (int)(o[0] / FSEL_TWO_PI * (double)FSEL_BINS);
  return b < FSEL_BINS - 1 ? b : FSEL_BINS - 1;
}

CBA_HD double fsel_dist(const double* a, const double* b) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 5; ++k) s += (a[k] - b[k]) * (a[k] - b[k]);
  return sqrt(s);
}

// (value, frame) beats (best value, best frame): larger value, lower frame on ties; a frame < 0 is no candidate
CBA_HD bool fsel_better(double v, int f, double bv, int bf) { return f >= 0 && (bf < 0 || v > bv || (v == bv && f < bf)); }

// running distance of frame f of a camera (feat: the camera's [nf][5]) at the start of the greedy phase
CBA_HD double fsel_start_dist(const double* feat, int f, bool eligible, const int* anchors, int na) {
  if (!eligible) return FSEL_TAKEN;
  double m = HUGE_VAL;
#pragma unroll
  for (int k = 0; k < FSEL_BINS; ++k)
    if (k < na) {
      if (anchors[k] == f) return FSEL_TAKEN;
      m = fmin(m, fsel_dist(feat + 5 * f, feat + 5 * anchors[k]));
    }
  return m;
}

// One frame in one greedy round: folds `last` (the frame selected in the round before, -1: none) into its running distance
// *dist, and returns true with its score when the frame is still a candidate.
CBA_HD bool fsel_round_item(const double* feat, int f, int last, uint64_t mask, uint64_t covered, uint64_t edge, uint64_t corner,
                            bool have, double* dist, double* score) {
  double m = *dist;
  if (m < 0.0) return false;
  if (last >= 0) {
    if (f == last) {
      *dist = FSEL_TAKEN;
      return false;
    }
    m = fmin(m, fsel_dist(feat + 5 * f, feat + 5 * last));
    *dist = m;
  }
  const uint64_t fresh = mask & ~covered;
  double s = (double)__builtin_popcountll(fresh);
  s += (double)__builtin_popcountll(fresh & edge) * FSEL_EDGE_WEIGHT;
  s += (double)__builtin_popcountll(fresh & corner) * FSEL_CORNER_WEIGHT;
  if (have) s += m * FSEL_DIVERSITY_WEIGHT;
  *score = s;
  return true;
}

// The two phases for one camera; target >= 1.  Returns the number selected.
template <class Ops>
CBA_HD int fsel_select(Ops& ops, int target, int* n_anchors, int* bin_mask) {
  int anchors[FSEL_BINS];
  int na = 0, bins = 0;
#pragma unroll
  for (int b = 0; b < FSEL_BINS; ++b) {
    anchors[b] = -1;
    const int f = ops.best_in_bin(b);
    if (f >= 0) {
      bins |= 1 << b;
#pragma unroll
      for (int k = 0; k < FSEL_BINS; ++k)
        if (k == na) anchors[k] = f;  // (no runtime index: the list stays in registers)
      ++na;
    }
  }
  *n_anchors = na;
  *bin_mask = bins;
  int n_sel = 0;
  uint64_t covered = 0;
#pragma unroll
  for (int k = 0; k < FSEL_BINS; ++k)
    if (k < na && n_sel < target) {
      ops.take(n_sel++, anchors[k]);
      covered |= ops.mask_of(anchors[k]);
    }
  if (na >= target) return n_sel;
  ops.start(anchors, na);
  int last = -1;
  while (n_sel < target) {
    double score;
    const int f = ops.best_score(last, covered, n_sel > 0, &score);
    if (f < 0 || score < FSEL_MIN_SCORE) break;
    ops.take(n_sel++, f);
    covered |= ops.mask_of(f);
    last = f;
  }
  return n_sel;
}

}  // namespace cba
