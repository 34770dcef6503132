// The compact Schur record of six-parameter cameras (caliscope_amd/csrc/ba_math.h: rec6_pack, rec6_xy, rec6_expand) against the twelve values of the
// full record (Y = R X, Q = G^T Z) evaluated in long double — TEST INFRASTRUCTURE, built by g++ as a stand-alone program in
// tests/test_compact_records.py.  For every case it prints the error of the full double path ("old": the twelve values kept) and of the compact
// path ("new": ten values kept — Y, 1/Zc and two rows of Q; the normalised point rebuilt from the camera's translation and Q's third row from it,
// with the arithmetic of pair6, k_tprep and k_backsub_rec) against the same long double values:
//     case <name> rec <old> <new> blk <old> <new> rot <old> <new> rhs <old> <new> step <old> <new>
// Errors are entrywise, relative to the largest long double entry of the same group (Y, Q; the four 3 x 3 quarters of a block — "rot" is the
// rotation-rotation quarter alone, relative to its own size; the two halves of a right-hand side; a back-substitution term).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ba_math.h"

typedef long double LD;

// project_factors' G and the normalised point in long double, from the doubles of the camera row
static void factors_ld(const cba::CamTab& c, const double* X, LD* Y, LD G[2][3]) {
  for (int r = 0; r < 3; ++r) Y[r] = (LD)c.R[3 * r] * X[0] + (LD)c.R[3 * r + 1] * X[1] + (LD)c.R[3 * r + 2] * X[2];
  const LD Zc = Y[2] + c.t[2], iz = 1.0L / Zc, x = (Y[0] + c.t[0]) * iz, y = (Y[1] + c.t[1]) * iz;
  LD dxx, dxy, dyy;
  const double* d = c.d;
  if (c.model != 0.0) {
    const LD r2 = x * x + y * y, r = sqrtl(r2);
    if (r > 1e-8L) {
      const LD th = atanl(r), t2 = th * th;
      const LD poly = 1.0L + t2 * (d[0] + t2 * (d[1] + t2 * (d[2] + t2 * d[3])));
      const LD dpoly = 1.0L + t2 * (3.0L * d[0] + t2 * (5.0L * d[1] + t2 * (7.0L * d[2] + t2 * 9.0L * d[3])));
      const LD thd = th * poly, cd = thd / r, g = (dpoly / (1.0L + r2) * r - thd) / (r * r * r);
      dxx = cd + x * x * g; dxy = x * y * g; dyy = cd + y * y * g;
    } else {
      dxx = 1.0L; dxy = 0.0L; dyy = 1.0L;
    }
  } else {
    const LD k1 = d[0], k2 = d[1], p1 = d[2], p2 = d[3], k3 = d[4];
    const LD r2 = x * x + y * y;
    const LD cd = 1.0L + r2 * (k1 + r2 * (k2 + r2 * k3)), dcd2 = 2.0L * (k1 + r2 * (2.0L * k2 + r2 * (3.0L * k3)));
    dxx = cd + x * x * dcd2 + p1 * 2.0L * y + 3.0L * p2 * 2.0L * x;
    dxy = x * y * dcd2 + p1 * 2.0L * x + p2 * 2.0L * y;
    dyy = cd + y * y * dcd2 + 3.0L * p1 * 2.0L * y + p2 * 2.0L * x;
  }
  const LD fxs = (LD)c.fx * c.inv_fx0, fys = (LD)c.fy * c.inv_fx0;
  G[0][0] = fxs * dxx * iz; G[0][1] = fxs * dxy * iz; G[0][2] = -(G[0][0] * x + G[0][1] * y);
  G[1][0] = fys * dxy * iz; G[1][1] = fys * dyy * iz; G[1][2] = -(G[1][0] * x + G[1][1] * y);
}

template <typename T> struct Obs { T Y[3], Q[9]; };  // the full record

template <typename T> static void cross(const T* a, const T* b, T* o) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
// T' = [[Y]x Q ; Q] (6 x 3)
template <typename T> static void primed(const T* Y, const T* Q, T* Tp) {
  for (int m = 0; m < 3; ++m) {
    const T col[3] = {Q[m], Q[3 + m], Q[6 + m]};
    T c[3];
    cross(Y, col, c);
    for (int r = 0; r < 3; ++r) { Tp[3 * r + m] = c[r]; Tp[3 * (3 + r) + m] = col[r]; }
  }
}
template <typename T> static void add_block(const T* Ti, const T* Tj, T* blk) {
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) blk[6 * r + c] += Ti[3 * r] * Tj[3 * c] + Ti[3 * r + 1] * Tj[3 * c + 1] + Ti[3 * r + 2] * Tj[3 * c + 2];
}
// [Y x (Q y) ; Q y] added to b
template <typename T> static void add_rhs(const T* Y, const T* Q, const T* y, T* b) {
  T qy[3], c[3];
  for (int r = 0; r < 3; ++r) qy[r] = Q[3 * r] * y[0] + Q[3 * r + 1] * y[1] + Q[3 * r + 2] * y[2];
  cross(Y, qy, c);
  for (int r = 0; r < 3; ++r) { b[r] += c[r]; b[3 + r] += qy[r]; }
}
// Q^T (w x Y + dt)
template <typename T> static void step_term(const T* Y, const T* Q, const T* w, const T* dt, T* o) {
  T m[3];
  cross(w, Y, m);
  for (int r = 0; r < 3; ++r) m[r] += dt[r];
  for (int k = 0; k < 3; ++k) o[k] = Q[k] * m[0] + Q[3 + k] * m[1] + Q[6 + k] * m[2];
}

// max |a - ref| over a group of n entries, relative to the group's largest reference entry
static double group_err(const double* a, const LD* ref, int n, int stride_a = 1, int stride_r = 1) {
  LD scale = 0.0L, err = 0.0L;
  for (int k = 0; k < n; ++k) scale = std::max(scale, fabsl(ref[k * stride_r]));
  for (int k = 0; k < n; ++k) err = std::max(err, fabsl((LD)a[k * stride_a] - ref[k * stride_r]));
  return scale > 0.0L ? (double)(err / scale) : (double)err;
}
static double block_err(const double* blk, const LD* ref, bool rot_only = false) {
  double e = 0.0;
  for (int qr = 0; qr < (rot_only ? 1 : 2); ++qr)
    for (int qc = 0; qc < (rot_only ? 1 : 2); ++qc) {
      double a[9]; LD r[9];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { a[3 * i + j] = blk[6 * (3 * qr + i) + 3 * qc + j]; r[3 * i + j] = ref[6 * (3 * qr + i) + 3 * qc + j]; }
      e = std::max(e, group_err(a, r, 9));
    }
  return e;
}

struct Lcg {  // fixed pseudo-random numbers in (-1, 1)
  unsigned long long s;
  double next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)((s >> 11) & ((1ULL << 53) - 1)) / (double)(1ULL << 52) - 1.0; }
};

static int failures = 0;

// two cameras (camera 0 and 1 of `tabs`), N points given in the frame of camera 0's optical axis: Xc0[p] is the point in camera 0's frame
static void run_case(const char* name, const cba::CamTab* tabs, const std::vector<double>& Xw, Lcg& rng) {
  const int N = (int)Xw.size() / 3;
  std::vector<Obs<LD>> ref(2 * N);
  std::vector<Obs<double>> old(2 * N);
  std::vector<double> rec(2 * N * 10);
  double e_rec_old = 0.0, e_rec_new = 0.0;
  for (int cam = 0; cam < 2; ++cam)
    for (int p = 0; p < N; ++p) {
      const cba::CamTab& c = tabs[cam];
      const double* X = &Xw[3 * p];
      double Z[2][3];
      for (int r = 0; r < 2; ++r)
        for (int k = 0; k < 3; ++k) Z[r][k] = 0.4 * rng.next();
      const int o = cam * N + p;
      LD Gl[2][3];
      factors_ld(c, X, ref[o].Y, Gl);
      for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) ref[o].Q[3 * r + k] = Gl[0][r] * Z[0][k] + Gl[1][r] * Z[1][k];
      double G[2][3], Yr[3], Aint[2][3], B[2][3], nrm[3];
      cba::project_factors(c, X[0], X[1], X[2], G, Yr, Aint, B, nrm);
      for (int r = 0; r < 3; ++r) {
        old[o].Y[r] = Yr[r];
        for (int k = 0; k < 3; ++k) old[o].Q[3 * r + k] = G[0][r] * Z[0][k] + G[1][r] * Z[1][k];
      }
      double* rc = &rec[10 * o];
      cba::rec6_pack(G, Yr, c.t, Z, rc);
      double xr, yr;
      cba::rec6_xy(rc, c.t, &xr, &yr);
      if (xr != nrm[0] || yr != nrm[1] || rc[3] != nrm[2] || std::memcmp(rc, Yr, 3 * sizeof(double)) != 0) {
        std::printf("%s: the record's normalised point differs from project_factors' own\n", name); ++failures;
      }
      double full[12];
      cba::rec6_expand(rc, c.t, full);
      e_rec_old = std::max(e_rec_old, std::max(group_err(old[o].Y, ref[o].Y, 3), group_err(old[o].Q, ref[o].Q, 9)));
      e_rec_new = std::max(e_rec_new, std::max(group_err(full, ref[o].Y, 3), group_err(full + 3, ref[o].Q, 9)));
    }
  // block of the camera pair (0, 1) and the diagonal block of camera 0; right-hand side of camera 1; step terms of both
  double e_blk_old = 0.0, e_blk_new = 0.0, e_rot_old = 0.0, e_rot_new = 0.0;
  for (int diag = 0; diag < 2; ++diag) {
    const int ci = 0, cj = diag ? 0 : 1;
    LD bl[36] = {0}; double bo[36] = {0}, bn[36] = {0};
    for (int p = 0; p < N; ++p) {
      const int oi = ci * N + p, oj = cj * N + p;
      LD Ti[18], Tj[18]; primed(ref[oi].Y, ref[oi].Q, Ti); primed(ref[oj].Y, ref[oj].Q, Tj); add_block(Ti, Tj, bl);
      double Ui[18], Uj[18]; primed(old[oi].Y, old[oi].Q, Ui); primed(old[oj].Y, old[oj].Q, Uj); add_block(Ui, Uj, bo);
      // compact: Y and the three rows of Q from the ten values and the camera's translation, as the pair kernel rebuilds them
      double Vi[18], Vj[18];
      for (int s = 0; s < 2; ++s) {
        const double* rc = &rec[10 * (s ? oj : oi)];
        double x, y, Q[9];
        cba::rec6_xy(rc, tabs[s ? cj : ci].t, &x, &y);
        for (int k = 0; k < 3; ++k) { Q[k] = rc[4 + k]; Q[3 + k] = rc[7 + k]; Q[6 + k] = -(x * rc[4 + k] + y * rc[7 + k]); }
        primed(rc, Q, s ? Vj : Vi);
      }
      add_block(Vi, Vj, bn);
    }
    e_blk_old = std::max(e_blk_old, block_err(bo, bl));
    e_blk_new = std::max(e_blk_new, block_err(bn, bl));
    e_rot_old = std::max(e_rot_old, block_err(bo, bl, true));
    e_rot_new = std::max(e_rot_new, block_err(bn, bl, true));
  }
  double e_rhs_old = 0.0, e_rhs_new = 0.0, e_step_old = 0.0, e_step_new = 0.0;
  for (int cam = 0; cam < 2; ++cam) {
    LD rl[6] = {0}; double ro[6] = {0}, rn[6] = {0};
    double w[3], dt[3];
    for (int k = 0; k < 3; ++k) { w[k] = 0.01 * rng.next(); dt[k] = 0.02 * rng.next(); }
    const LD wl[3] = {w[0], w[1], w[2]}, dl[3] = {dt[0], dt[1], dt[2]};
    for (int p = 0; p < N; ++p) {
      const int o = cam * N + p;
      double y[3]; LD yl[3];
      for (int k = 0; k < 3; ++k) { y[k] = rng.next(); yl[k] = y[k]; }
      add_rhs(ref[o].Y, ref[o].Q, yl, rl);
      add_rhs(old[o].Y, old[o].Q, y, ro);
      const double* rc = &rec[10 * o];
      double x, yy, Q[9];
      cba::rec6_xy(rc, tabs[cam].t, &x, &yy);
      for (int k = 0; k < 3; ++k) { Q[k] = rc[4 + k]; Q[3 + k] = rc[7 + k]; Q[6 + k] = -(x * rc[4 + k] + yy * rc[7 + k]); }
      add_rhs(rc, Q, y, rn);
      LD sl[3]; double so[3], sn[3];
      step_term(ref[o].Y, ref[o].Q, wl, dl, sl);
      step_term(old[o].Y, old[o].Q, w, dt, so);
      {  // k_backsub_rec's form: m = w x Y + dt, Q^T m = Q_row0^T (m0 - x m2) + Q_row1^T (m1 - y m2)
        double m[3];
        cross(w, rc, m);
        for (int r = 0; r < 3; ++r) m[r] += dt[r];
        const double v0 = m[0] - x * m[2], v1 = m[1] - yy * m[2];
        for (int k = 0; k < 3; ++k) sn[k] = rc[4 + k] * v0 + rc[7 + k] * v1;
      }
      e_step_old = std::max(e_step_old, group_err(so, sl, 3));
      e_step_new = std::max(e_step_new, group_err(sn, sl, 3));
    }
    e_rhs_old = std::max(e_rhs_old, std::max(group_err(ro, rl, 3), group_err(ro + 3, rl + 3, 3)));
    e_rhs_new = std::max(e_rhs_new, std::max(group_err(rn, rl, 3), group_err(rn + 3, rl + 3, 3)));
  }
  std::printf("case %s rec %.3e %.3e blk %.3e %.3e rot %.3e %.3e rhs %.3e %.3e step %.3e %.3e\n", name, e_rec_old, e_rec_new, e_blk_old, e_blk_new, e_rot_old,
              e_rot_new, e_rhs_old, e_rhs_new, e_step_old, e_step_new);
}

// camera with rotation vector r looking at points `depth` in front of it: the world points are X = R^T (Xc - t)
static std::vector<double> points_in_front(const cba::CamTab& c, double depth, int n, Lcg& rng) {
  std::vector<double> X(3 * n);
  for (int p = 0; p < n; ++p) {
    const double xc[3] = {0.35 * depth * rng.next(), 0.3 * depth * rng.next(), depth * (1.0 + 0.1 * rng.next())};
    const double v[3] = {xc[0] - c.t[0], xc[1] - c.t[1], xc[2] - c.t[2]};
    for (int k = 0; k < 3; ++k) X[3 * p + k] = c.R[k] * v[0] + c.R[3 + k] * v[1] + c.R[6 + k] * v[2];
  }
  return X;
}

int main() {
  const double cc_pin[9] = {905.3, 911.7, 640.2, 355.9, -0.23, 0.09, 0.0011, -0.0007, -0.013};
  const double cc_fish[9] = {512.4, 509.8, 318.1, 242.6, 0.031, -0.012, 0.0042, -0.0009, 0.0};
  const double rv[2][3] = {{0.31, -0.42, 0.17}, {0.28, -0.47, 0.21}};  // two nearby views: both see the points in front of the first
  struct Case { const char* name; double tlen; double depth; };
  // t = 0; |t| = 100 with the points one unit in front (Yc = Y + t cancels two digits); the smallest depth of the synthetic scenes (a 3 m ring
  // around points within 0.6 m of the axis: depths from 2.3) and a tenth of it
  const Case cases[] = {{"t0", 0.0, 3.0}, {"t100_depth1", 100.0, 1.0}, {"ring_depth2", 3.0, 2.0}, {"ring_depth0.2", 3.0, 0.2}};
  const double tdir[3] = {0.48, -0.6, 0.64};
  Lcg rng{12345};
  for (int model = 0; model < 2; ++model)
    for (const Case& cs : cases) {
      cba::CamTab tabs[2];
      for (int cam = 0; cam < 2; ++cam) {
        double xc[cba::MAX_NC] = {rv[cam][0], rv[cam][1], rv[cam][2], cs.tlen * tdir[0], cs.tlen * tdir[1], cs.tlen * tdir[2], 1.0, 0.0, 0.0};
        if (cam == 1) { xc[3] += 0.05 * cs.depth; xc[4] -= 0.03 * cs.depth; }
        cba::cam_prepare(xc, model ? cc_fish : cc_pin, model, 6, &tabs[cam], 6 * cam);
      }
      const std::vector<double> X = points_in_front(tabs[0], cs.depth, 12, rng);
      char name[64];
      std::snprintf(name, sizeof name, "%s_%s", model ? "fisheye" : "pinhole", cs.name);
      run_case(name, tabs, X, rng);
    }
  if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
  std::printf("all cases ran\n");
  return 0;
}
