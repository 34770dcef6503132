// CPU harness around caliscope_amd/csrc/epipolar_math.h — TEST INFRASTRUCTURE (built by g++ in tests/epipolar_native.py).
// It does what cba_pose_essential_batch and cba_pose_resect_batch do, job after job, with the arithmetic the kernels of
// pose_lib.hip inline and their workgroup sums replayed in the same fixed tree, so that the non-GPU suite can check the maths
// and drive caliscope_amd/epipolar_pose.py through its `_epi` hook.  It is not a CPU fallback: nothing in caliscope_amd/ loads it.
#include <cmath>
#include <cstdint>
#include <vector>

#include "epipolar_math.h"

using namespace cba;

namespace {

constexpr int NT = EPI_REDUCE_NT;

// the workgroup reduction of pose_lib.hip wg_sum: "thread" tid sums items tid, tid + NT, ... of [s, e); then the tree
template <int K, class Item>
void tree_sum(int64_t s, int64_t e, Item item, double* out) {
  std::vector<double> part((size_t)NT * K, 0.0);
  for (int tid = 0; tid < NT; ++tid)
    for (int64_t i = s + tid; i < e; i += NT) item(i, &part[(size_t)tid * K]);
  for (int st = NT / 2; st > 0; st >>= 1)
    for (int tid = 0; tid < st; ++tid)
      for (int k = 0; k < K; ++k) part[(size_t)tid * K + k] += part[(size_t)(tid + st) * K + k];
  for (int k = 0; k < K; ++k) out[k] = part[k];
}

struct EpiSumHost {
  const double* und; const int64_t* ca; const int64_t* cb; const uint8_t* flag; int64_t s, e;
  void operator()(const double* R, const double* t, double* out) {
    double E[9], dE[5][9];
    essential_from_pose(R, t, E);
    essential_jacobian(R, t, dE);
    tree_sum<EPI_NSUM>(s, e, [&](int64_t i, double* acc) {
      if (flag[i]) epi_sampson_normal(E, dE, und[2 * ca[i]], und[2 * ca[i] + 1], und[2 * cb[i]], und[2 * cb[i] + 1], acc);
    }, out);
  }
};

struct ResSumHost {
  const double* obj; const double* uv; const double* Rh; const double* th; double thr2; int64_t s, e;
  void operator()(const double* R, const double* t, double* out) {
    tree_sum<RES_NSUM>(s, e, [&](int64_t i, double* acc) {
      if (res_err2(Rh, th, obj + 3 * i, uv[2 * i], uv[2 * i + 1]) <= thr2) res_point_normal(R, t, obj + 3 * i, uv[2 * i], uv[2 * i + 1], acc);
    }, out);
  }
};

// the winner: maximum count, lowest index on ties
int select_winner(const std::vector<int64_t>& count, unsigned* best) {
  int w = -1;
  int64_t c = -1;
  for (size_t h = 0; h < count.size(); ++h)
    if (count[h] > c) { c = count[h]; w = (int)h; }
  *best = (unsigned)(c < 0 ? 0 : c);
  return w;
}

}  // namespace

extern "C" {

// draws of the sampler (tests)
void eh_sample(uint64_t seed, int64_t job, int64_t h, int64_t n, int k, int64_t* idx) {
  if (k == EPI_SAMPLE) sample_distinct<EPI_SAMPLE>(seed, job, h, n, idx);
  else sample_distinct<RES_SAMPLE>(seed, job, h, n, idx);
}

double eh_sampson(const double* E, double xa, double ya, double xb, double yb) { return epi_sampson(E, xa, ya, xb, yb); }

// the four (R, t) of E and the index recoverPose's rule picks for n correspondences (c: [n][4] xa ya xb yb); -1: rank < 2
int eh_decompose(const double* E, int64_t n, const double* c, double* rt_out /*[4][12]*/, int64_t* count_out /*[4]*/) {
  double rt[4][12];
  if (!essential_candidates(E, rt)) return -1;
  int best = 0;
  for (int k = 0; k < 4; ++k) {
    count_out[k] = 0;
    for (int64_t i = 0; i < n; ++i) {
      double w[4];
      count_out[k] += epi_in_front(rt[k], c[4 * i], c[4 * i + 1], c[4 * i + 2], c[4 * i + 3], w) ? 1 : 0;
    }
    for (int j = 0; j < 12; ++j) rt_out[12 * k + j] = rt[k][j];
    if (count_out[k] > count_out[best]) best = k;
  }
  return best;
}

// The inlier count of every hypothesis of one job over a chosen list of its items (tests: what k_score has to add up over
// all tiles, and what it would add up over some of them).  The job holds correspondences / points s .. s + n - 1; its
// hypotheses are drawn as the batch calls draw them for job index `job`; items[] are offsets into the job.
void eh_essential_counts(const double* und, const int64_t* ca, const int64_t* cb, int64_t s, int64_t n, double thr, int32_t n_hyp, uint64_t seed,
                         int64_t job, int64_t n_items, const int64_t* items, int64_t* count_out) {
  auto corr = [&](int64_t i, double* c) { c[0] = und[2 * ca[i]]; c[1] = und[2 * ca[i] + 1]; c[2] = und[2 * cb[i]]; c[3] = und[2 * cb[i] + 1]; };
  for (int h = 0; h < n_hyp; ++h) {
    count_out[h] = 0;
    if (n < EPI_SAMPLE) continue;
    int64_t idx[EPI_SAMPLE];
    sample_distinct<EPI_SAMPLE>(seed, job, h, n, idx);
    double c[EPI_SAMPLE][4], E[9];
    for (int k = 0; k < EPI_SAMPLE; ++k) corr(s + idx[k], c[k]);
    essential_hypothesis(c, E);
    for (int64_t q = 0; q < n_items; ++q) {
      double cc[4];
      corr(s + items[q], cc);
      count_out[h] += epi_sampson(E, cc[0], cc[1], cc[2], cc[3]) <= thr * thr ? 1 : 0;
    }
  }
}

void eh_resect_counts(const double* obj, const double* uv, int64_t s, int64_t n, double thr, int32_t n_hyp, uint64_t seed, int64_t job,
                      int64_t n_items, const int64_t* items, int64_t* count_out) {
  for (int h = 0; h < n_hyp; ++h) {
    count_out[h] = 0;
    if (n < RES_SAMPLE) continue;
    int64_t idx[RES_SAMPLE];
    sample_distinct<RES_SAMPLE>(seed, job, h, n, idx);
    double P[RES_SAMPLE][5], Rh[9], th[3];
    for (int k = 0; k < RES_SAMPLE; ++k) {
      const int64_t i = s + idx[k];
      P[k][0] = obj[3 * i]; P[k][1] = obj[3 * i + 1]; P[k][2] = obj[3 * i + 2]; P[k][3] = uv[2 * i]; P[k][4] = uv[2 * i + 1];
    }
    if (!res_hypothesis(P, Rh, th)) continue;
    for (int64_t q = 0; q < n_items; ++q) {
      const int64_t i = s + items[q];
      count_out[h] += res_err2(Rh, th, obj + 3 * i, uv[2 * i], uv[2 * i + 1]) <= thr * thr ? 1 : 0;
    }
  }
}

// what cba_pose_essential_batch computes (und: [n_obs][2] out)
void eh_essential_batch(int32_t n_cams, const int32_t* cam_model, const double* cam_intr, int64_t n_obs, const double* obs_xy, const int32_t* obs_cam,
                        int64_t n_pairs, const int64_t* pair_start, const int64_t* ca, const int64_t* cb, const double* thr, int32_t n_hyp, uint64_t seed,
                        int32_t f32, double* pose_out, int32_t* status_out, int64_t* n_inl, int64_t* n_chr, double* cond_out, int32_t* winner_out,
                        uint8_t* flag, double* xyz, double* und) {
  (void)n_cams;
  for (int64_t i = 0; i < n_obs; ++i) {
    const int c = obs_cam[i];
    undistort_one(cam_model[c], cam_intr + 9 * c, obs_xy[2 * i], obs_xy[2 * i + 1], f32, &und[2 * i], &und[2 * i + 1]);
  }
  const double nan = std::nan("");
  for (int64_t p = 0; p < n_pairs; ++p) {
    const int64_t s = pair_start[p], e = pair_start[p + 1], n = e - s;
    const double thr2 = thr[p] * thr[p];
    auto corr = [&](int64_t i, double* c) { c[0] = und[2 * ca[i]]; c[1] = und[2 * ca[i] + 1]; c[2] = und[2 * cb[i]]; c[3] = und[2 * cb[i] + 1]; };
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
    int st = EPI_OK, w = -1;
    if (n < EPI_SAMPLE) st = EPI_TOO_FEW;
    std::vector<double> hyp;
    unsigned best = 0;
    if (st == EPI_OK) {
      hyp.assign((size_t)n_hyp * 9, 0.0);
      std::vector<int64_t> count(n_hyp, 0);
      for (int h = 0; h < n_hyp; ++h) {
        int64_t idx[EPI_SAMPLE];
        sample_distinct<EPI_SAMPLE>(seed, p, h, n, idx);
        double c[EPI_SAMPLE][4];
        for (int k = 0; k < EPI_SAMPLE; ++k) corr(s + idx[k], c[k]);
        essential_hypothesis(c, &hyp[(size_t)h * 9]);
        for (int64_t i = s; i < e; ++i) {
          double cc[4];
          corr(i, cc);
          count[h] += epi_sampson(&hyp[(size_t)h * 9], cc[0], cc[1], cc[2], cc[3]) <= thr2 ? 1 : 0;
        }
      }
      w = select_winner(count, &best);
      if (w < 0 || best < (unsigned)EPI_SAMPLE) st = EPI_FAILED;
    }
    double rt[4][12];
    if (st == EPI_OK) {
      const double* E = &hyp[(size_t)w * 9];
      for (int64_t i = s; i < e; ++i) {
        double c[4];
        corr(i, c);
        flag[i] = epi_sampson(E, c[0], c[1], c[2], c[3]) <= thr2 ? 1 : 0;
      }
      if (!essential_candidates(E, rt)) st = EPI_FAILED;
    }
    if (st == EPI_OK) {
      unsigned cnt[4] = {0, 0, 0, 0};
      for (int64_t i = s; i < e; ++i)
        if (flag[i]) {
          double c[4], wv[4];
          corr(i, c);
          for (int k = 0; k < 4; ++k) cnt[k] += epi_in_front(rt[k], c[0], c[1], c[2], c[3], wv) ? 1u : 0u;
        }
      int kb = 0;
      for (int k = 1; k < 4; ++k) if (cnt[k] > cnt[kb]) kb = k;
      for (int k = 0; k < 9; ++k) R[k] = rt[kb][k];
      for (int k = 0; k < 3; ++k) t[k] = rt[kb][9 + k];
      EpiSumHost sum{und, ca, cb, flag, s, e};
      if (!pnp_finite(epi_refine(sum, R, t))) st = EPI_FAILED;
      unsigned prev = best;
      for (int lo = 0; lo < EPI_LO_ROUNDS && st == EPI_OK; ++lo) {
        double Ec[9];
        essential_from_pose(R, t, Ec);
        unsigned cnt = 0;
        for (int64_t i = s; i < e; ++i) {
          double c[4];
          corr(i, c);
          flag[i] = epi_sampson(Ec, c[0], c[1], c[2], c[3]) <= thr2 ? 1 : 0;
          cnt += flag[i];
        }
        if (cnt <= prev) break;
        prev = cnt;
        if (!pnp_finite(epi_refine(sum, R, t))) st = EPI_FAILED;
      }
    }
    if (st != EPI_OK) {
      for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
      t[0] = t[1] = t[2] = 0.0;
    }
    double Ef[9], rtf[12];
    essential_from_pose(R, t, Ef);
    for (int k = 0; k < 9; ++k) rtf[k] = R[k];
    for (int k = 0; k < 3; ++k) rtf[9 + k] = t[k];
    int64_t m1 = 0, m2 = 0;
    for (int64_t i = s; i < e; ++i) {
      double c[4], wv[4];
      corr(i, c);
      uint8_t f = 0;
      double X = nan, Y = nan, Z = nan;
      if (st == EPI_OK && epi_sampson(Ef, c[0], c[1], c[2], c[3]) <= thr2) {
        f = 1;
        if (epi_in_front(rtf, c[0], c[1], c[2], c[3], wv)) {
          f = 2;
          if (std::fabs(wv[3]) > 1e-12) { X = wv[0] / wv[3]; Y = wv[1] / wv[3]; Z = wv[2] / wv[3]; }
        }
      }
      flag[i] = f;
      m1 += f >= 1;
      m2 += f == 2;
      if (xyz) { xyz[3 * i] = X; xyz[3 * i + 1] = Y; xyz[3 * i + 2] = Z; }
    }
    double N[EPI_LIN_NSUM];
    tree_sum<EPI_LIN_NSUM>(s, e, [&](int64_t i, double* acc) {
      if (flag[i]) { double c[4]; corr(i, c); epi_linear_normal(c[0], c[1], c[2], c[3], acc); }
    }, N);
    cond_out[p] = st == EPI_OK ? epi_conditioning(N, Ef) : 0.0;
    for (int k = 0; k < 12; ++k) pose_out[12 * p + k] = rtf[k];
    status_out[p] = st;
    n_inl[p] = m1;
    n_chr[p] = m2;
    winner_out[p] = w;
  }
}

// what cba_pose_resect_batch computes
void eh_resect_batch(int64_t n_jobs, const int64_t* job_start, const double* obj, const double* uv, const double* thr, int32_t n_hyp, int32_t min_points,
                     uint64_t seed, double* pose_out, int32_t* status_out, int64_t* n_inl, int32_t* winner_out, double* err_out) {
  for (int64_t j = 0; j < n_jobs; ++j) {
    const int64_t s = job_start[j], e = job_start[j + 1], n = e - s;
    const double thr2 = thr[j] * thr[j];
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
    int st = EPI_OK, w = -1;
    if (n < RES_SAMPLE || n < min_points) st = EPI_TOO_FEW;
    std::vector<double> hyp;
    if (st == EPI_OK) {
      hyp.assign((size_t)n_hyp * 12, std::nan(""));
      std::vector<int64_t> count(n_hyp, 0);
      for (int h = 0; h < n_hyp; ++h) {
        int64_t idx[RES_SAMPLE];
        sample_distinct<RES_SAMPLE>(seed, j, h, n, idx);
        double P[RES_SAMPLE][5];
        for (int k = 0; k < RES_SAMPLE; ++k) {
          const int64_t i = s + idx[k];
          P[k][0] = obj[3 * i]; P[k][1] = obj[3 * i + 1]; P[k][2] = obj[3 * i + 2]; P[k][3] = uv[2 * i]; P[k][4] = uv[2 * i + 1];
        }
        double Rh[9], th[3];
        if (!res_hypothesis(P, Rh, th)) continue;
        for (int k = 0; k < 9; ++k) hyp[(size_t)h * 12 + k] = Rh[k];
        for (int k = 0; k < 3; ++k) hyp[(size_t)h * 12 + 9 + k] = th[k];
        for (int64_t i = s; i < e; ++i) count[h] += res_err2(Rh, th, obj + 3 * i, uv[2 * i], uv[2 * i + 1]) <= thr2 ? 1 : 0;
      }
      unsigned best;
      w = select_winner(count, &best);
      if (w < 0 || best < (unsigned)RES_SAMPLE) st = EPI_FAILED;
    }
    if (st == EPI_OK) {
      const double* H = &hyp[(size_t)w * 12];
      for (int k = 0; k < 9; ++k) R[k] = H[k];
      for (int k = 0; k < 3; ++k) t[k] = H[9 + k];
      ResSumHost sum{obj, uv, H, H + 9, thr2, s, e};
      if (!pnp_finite(res_refine(sum, R, t))) st = EPI_FAILED;
    }
    if (st != EPI_OK) {
      for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
      t[0] = t[1] = t[2] = 0.0;
    }
    int64_t m = 0;
    for (int64_t i = s; i < e; ++i) {
      m += (st == EPI_OK && res_err2(R, t, obj + 3 * i, uv[2 * i], uv[2 * i + 1]) <= thr2) ? 1 : 0;
      err_out[i] = st == EPI_OK ? res_err(R, t, obj + 3 * i, uv[2 * i], uv[2 * i + 1]) : std::nan("");
    }
    for (int k = 0; k < 9; ++k) pose_out[12 * j + k] = R[k];
    for (int k = 0; k < 3; ++k) pose_out[12 * j + 9 + k] = t[k];
    status_out[j] = st;
    n_inl[j] = m;
    winner_out[j] = w;
  }
}

}
