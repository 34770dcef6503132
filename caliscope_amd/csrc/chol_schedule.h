// Launch geometry of the blocked Cholesky of the dense camera-system solve (k_chol_step of cba_kernels.h, enqueue_chol_factor of cba_lib.hip):
// which workgroup of launch k plays which role on which block, how many there are of each, and which blocks each reads and writes.  Plain
// C++, __host__ __device__ under hipcc: the kernel decodes blockIdx.x with chol_decode, the host sizes the grid with chol_counts, and the CPU
// suite replays chol_for_each_access / chol_for_each_action for every launch (tests/native/chol_schedule_check.cpp).
//
// nbk = ceil(n / NB) column blocks; row block nbk is the rhs row.  P_m(i, j) = L_im L_jm^T is the rank-NB update of panel m.
// Launch -1 is one workgroup that factors D_0.  Launch k >= 0, L_kk and X_k = L_kk^-1 ready:
//
//   EARLY (the default schedule)
//     panel workgroup b = k + 1 .. nbk     W_bk arrives complete.  L_bk = W_bk X_k^T in place; D_b -= P_k(b, b); b == k + 1 factors D_b.
//                                          b >= k + 2, column block k + 1 existing, then completes (b, k + 1) for the next launch:
//                                            W_b,k+1 <- (W_b,k+1 - P_k-1(b, k + 1) [k >= 1]) - P_k(b, k + 1),
//                                          P_k from its own L_bk and a private L_k+1,k = U_k+1,k X_k^T.  U_k+1,k is read from SIDE SLOT k, not
//                                          from W: the critical workgroup b = k + 1 overwrites W_k+1,k with L_k+1,k in this very launch.
//                                          b == k + 2 stores what it completed to side slot k + 1 as well (launch -1 copies W_10 to slot 0).
//     trailing workgroup (i, j)            k + 2 <= j < i <= nbk (k >= 1):  W_ij -= P_k-1(i, j).  Column k + 1 belongs to the panel workgroups.
//   PARENT (CBA_CHOL_EARLY=0, the A/B reference)
//     panel workgroup b                    first W_bk -= P_k-1(b, k) (k >= 1), then as above without the early update and the side slots.
//     trailing workgroup (i, j)            k + 1 <= j < i <= nbk.
//   inverse workgroup (i >= k, j < k)      both schedules, k >= 1, where T = L^-T is wanted: block (j, i) of T takes the term of panel k - 1.
//
// Either way every block (i, j) receives P_0, P_1, .., P_j-1 once each in ascending order, so the factor is the same to the bit.
//
// PAIRED FIRST LAUNCH (CBA_CHOL_PAIR, the default; the solver's call on the early schedule with the folded end, nbk >= 2): launches -1 and 0 are ONE
// launch of nbk panel workgroups.  Every one factors D_0 PRIVATELY (the same pivot code on the same bits) and takes X_0 from its own LDS, then runs
// launch 0's body as above; b == 1 alone stores L_00, X_0 and T_00.  D_0 and U_10 are read from side slots (chol_side_d0 and slot 0) that the
// producers of the work matrix fill, since b == 1 overwrites both blocks in place while the others still read them.  chol_pair_* below.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CHOL_HD __host__ __device__
#else
#define CHOL_HD
#endif

namespace cba {

// Block width of the factorisation: the one definition.  k_chol_step and its neighbours (cba_kernels.h), the solver's work matrix (cba_lib.hip)
// and the covariance's own buffers and k_unc_ttt grid (covariance_lib.hip) all size themselves with it.
constexpr int NB = 32;

enum CholRole : int { CHOL_FACTOR0 = 0, CHOL_PANEL = 1, CHOL_TRAILING = 2, CHOL_INVERSE = 3 };

// side slots live behind the nbk + 1 inverses of the diagonal blocks, in the same buffer: [2 (nbk + 1) + 1][NB][NB]; the last one is D_0's
CHOL_HD inline int chol_xinv_blocks(int nbk) { return 2 * (nbk + 1) + 1; }
CHOL_HD inline int chol_side_slot(int nbk, int s) { return nbk + 1 + s; }  // index of side slot s in units of NB x NB blocks
CHOL_HD inline int chol_side_d0(int nbk) { return nbk + 1; }               // the side slot that holds D_0 for the paired first launch

struct CholCounts {
  int panel, trailing, inverse;
  CHOL_HD int total() const { return panel + trailing + inverse; }
};

template <bool EARLY>
CHOL_HD inline int chol_first_trailing_column(int k) { return k + (EARLY ? 2 : 1); }

template <bool EARLY>
CHOL_HD inline CholCounts chol_counts(int nbk, int k, bool with_inverse) {
  CholCounts c;
  c.panel = (k < 0) ? 1 : nbk - k;
  const int x = nbk - chol_first_trailing_column<EARLY>(k);  // columns j0 .. nbk - 1, column j with nbk - j blocks below it
  c.trailing = (k < 1 || x < 1) ? 0 : x * (x + 1) / 2;
  c.inverse = (with_inverse && k >= 1) ? (nbk - k) * k : 0;
  return c;
}

// What workgroup `wg` of launch k does.
//   (bi, bj)     the block of its role: panel (b, k); trailing (i, j); inverse: block (bj, bi) of T; launch -1: (0, 0)
//   critical     the panel workgroup b == k + 1 (and launch -1): it factors the next diagonal block
//   upd_col      >= 0: the workgroup subtracts P_m(bi, upd_col) for m = upd_first .. upd_first + upd_terms - 1 from block (bi, upd_col)
//   early        a panel workgroup with the early update (upd_col == k + 1): reads side slot k
//   side_write   >= 0: the side slot that receives a copy of the block it completed (launch -1: of W_10)
//   factor_first the paired first launch: the workgroup factors D_0 privately in front of launch 0's body; store_first: and stores L_00, X_0, T_00
struct CholWork {
  int role, bi, bj;
  bool critical, early;
  int upd_col, upd_first, upd_terms, side_write;
  bool factor_first, store_first;
};

template <bool EARLY>
CHOL_HD inline CholWork chol_decode(int nbk, int k, int wg, bool with_inverse) {
  const CholCounts cnt = chol_counts<EARLY>(nbk, k, with_inverse);
  CholWork w;
  w.critical = false; w.early = false;
  w.upd_col = -1; w.upd_first = 0; w.upd_terms = 0; w.side_write = -1;
  w.factor_first = false; w.store_first = false;
  if (k < 0) {
    w.role = CHOL_FACTOR0; w.bi = 0; w.bj = 0; w.critical = true;
    if (EARLY && nbk >= 2) w.side_write = 0;
    return w;
  }
  if (wg < cnt.panel) {
    w.role = CHOL_PANEL; w.bi = k + 1 + wg; w.bj = k;
    w.critical = wg == 0;
    if (EARLY) {
      if (w.bi >= k + 2 && k + 1 < nbk) {
        w.early = true;
        w.upd_col = k + 1; w.upd_first = (k >= 1) ? k - 1 : k; w.upd_terms = (k >= 1) ? 2 : 1;
        if (w.bi == k + 2 && k + 2 < nbk) w.side_write = k + 1;
      }
    } else if (k >= 1) {
      w.upd_col = k; w.upd_first = k - 1; w.upd_terms = 1;
    }
    return w;
  }
  if (wg < cnt.panel + cnt.trailing) {
    int t = wg - cnt.panel, bj = chol_first_trailing_column<EARLY>(k);
    while (t >= nbk - bj) { t -= nbk - bj; ++bj; }
    w.role = CHOL_TRAILING; w.bi = bj + 1 + t; w.bj = bj;
    w.upd_col = bj; w.upd_first = k - 1; w.upd_terms = 1;
    return w;
  }
  const int t2 = wg - cnt.panel - cnt.trailing;
  w.role = CHOL_INVERSE; w.bi = k + t2 / k; w.bj = t2 % k;
  return w;
}

// ---- the blocks a workgroup touches, for the replay of the CPU suite ------------------------------------------------------------------------
enum CholBuf : int { CHOL_W = 0, CHOL_XINV = 1, CHOL_SIDE = 2, CHOL_T = 3 };
struct CholRef {
  int buf, i, j;  // CHOL_W / CHOL_T: block (i, j); CHOL_XINV / CHOL_SIDE: slot i, j = 0
};

// f(CholRef, bool write) for every block workgroup `wg` of launch k reads or writes (a block read and written is reported twice)
template <bool EARLY, class F>
inline void chol_for_each_access(int nbk, int k, int wg, bool with_inverse, F&& f) {
  const CholWork w = chol_decode<EARLY>(nbk, k, wg, with_inverse);
  const auto rd = [&](int buf, int i, int j) { f(CholRef{buf, i, j}, false); };
  const auto wr = [&](int buf, int i, int j) { f(CholRef{buf, i, j}, true); };
  if (w.role == CHOL_FACTOR0) {
    rd(CHOL_W, 0, 0); wr(CHOL_W, 0, 0); wr(CHOL_XINV, 0, 0);
    if (with_inverse) wr(CHOL_T, 0, 0);
    if (w.side_write >= 0) { rd(CHOL_W, 1, 0); wr(CHOL_SIDE, w.side_write, 0); }
    return;
  }
  if (w.role == CHOL_PANEL) {
    const int b = w.bi;
    const bool has_diag = b < nbk;
    rd(CHOL_W, b, k); rd(CHOL_XINV, k, 0); wr(CHOL_W, b, k);
    if (has_diag) { rd(CHOL_W, b, b); wr(CHOL_W, b, b); }
    if (w.critical && has_diag) { wr(CHOL_XINV, k + 1, 0); if (with_inverse) wr(CHOL_T, b, b); }
    if (w.upd_col >= 0) {
      for (int m = w.upd_first; m < k; ++m) { rd(CHOL_W, b, m); rd(CHOL_W, w.upd_col, m); }  // P_k-1 from global operands; P_k is the workgroup's own
      if (w.early) { rd(CHOL_SIDE, k, 0); rd(CHOL_W, b, w.upd_col); wr(CHOL_W, b, w.upd_col); }
      if (w.side_write >= 0) wr(CHOL_SIDE, w.side_write, 0);
    }
    return;
  }
  if (w.role == CHOL_TRAILING) {
    rd(CHOL_W, w.bi, w.bj); rd(CHOL_W, w.bi, k - 1); rd(CHOL_W, w.bj, k - 1); wr(CHOL_W, w.bi, w.bj);
    return;
  }
  const int m = k - 1;  // inverse role: block (bj, bi) of T
  if (m != w.bj) rd(CHOL_T, w.bj, w.bi);
  rd(CHOL_T, w.bj, m); rd(CHOL_W, w.bi, m);
  if (w.bi == k) rd(CHOL_XINV, k, 0);
  wr(CHOL_T, w.bj, w.bi);
}

// What a workgroup does to the factorisation, in its own program order:
//   CHOL_ACT_APPLY   block (i, j) -= P_m(i, j)
//   CHOL_ACT_SOLVE   block (i, j), i > j, becomes L_ij = W_ij X_j^T       (m = j)
//   CHOL_ACT_FACTOR  diagonal block (i, i) is factored                     (m = i)
//   CHOL_ACT_PRIVATE_FACTOR  the paired first launch: a private copy of D_0 is factored, nothing of it is stored   (i = j = m = 0)
enum CholAct : int { CHOL_ACT_APPLY = 0, CHOL_ACT_SOLVE = 1, CHOL_ACT_FACTOR = 2, CHOL_ACT_PRIVATE_FACTOR = 3 };

// f(CholAct, i, j, m) for every action of workgroup `wg` of launch k (the inverse role has none: it does not touch the factor)
template <bool EARLY, class F>
inline void chol_for_each_action(int nbk, int k, int wg, bool with_inverse, F&& f) {
  const CholWork w = chol_decode<EARLY>(nbk, k, wg, with_inverse);
  if (w.role == CHOL_FACTOR0) { f(CHOL_ACT_FACTOR, 0, 0, 0); return; }
  if (w.role == CHOL_INVERSE) return;
  if (w.role == CHOL_TRAILING) { f(CHOL_ACT_APPLY, w.bi, w.bj, w.upd_first); return; }
  const int b = w.bi;
  if (!w.early && w.upd_col >= 0) f(CHOL_ACT_APPLY, b, k, w.upd_first);  // the parent's pending update, in front of the solve
  f(CHOL_ACT_SOLVE, b, k, k);
  if (w.early)
    for (int t = 0; t < w.upd_terms; ++t) f(CHOL_ACT_APPLY, b, w.upd_col, w.upd_first + t);
  if (b < nbk) {
    f(CHOL_ACT_APPLY, b, b, k);
    if (w.critical) f(CHOL_ACT_FACTOR, b, b, b);
  }
}

// ---- the paired first launch: launches -1 and 0 as one (see the head of the file) -------------------------------------------------------------------
CHOL_HD inline bool chol_pair_applies(int nbk, bool early, bool folded_end) { return early && folded_end && nbk >= 2; }
CHOL_HD inline int chol_first_launch(bool pair) { return pair ? 0 : -1; }  // the k of the first launch of the sequence; pair: it is the paired one

CHOL_HD inline CholCounts chol_pair_counts(int nbk) {
  CholCounts c;
  c.panel = nbk; c.trailing = 0; c.inverse = 0;
  return c;
}

CHOL_HD inline CholWork chol_pair_decode(int nbk, int wg, bool with_inverse) {
  CholWork w = chol_decode<true>(nbk, 0, wg, with_inverse);  // launch 0 has panel workgroups only
  w.factor_first = true;
  w.store_first = w.critical;
  return w;
}

template <class F>
inline void chol_pair_for_each_access(int nbk, int wg, bool with_inverse, F&& f) {
  const CholWork w = chol_pair_decode(nbk, wg, with_inverse);
  f(CholRef{CHOL_SIDE, chol_side_d0(nbk), 0}, false);
  if (w.store_first) {
    f(CholRef{CHOL_W, 0, 0}, true); f(CholRef{CHOL_XINV, 0, 0}, true);
    if (with_inverse) f(CholRef{CHOL_T, 0, 0}, true);
  }
  chol_for_each_access<true>(nbk, 0, wg, with_inverse, [&](CholRef r, bool write) {
    if (!write && r.buf == CHOL_XINV && r.i == 0) return;  // X_0 comes from the workgroup's own LDS
    f(r, write);
  });
}

template <class F>
inline void chol_pair_for_each_action(int nbk, int wg, bool with_inverse, F&& f) {
  const CholWork w = chol_pair_decode(nbk, wg, with_inverse);
  f(w.store_first ? CHOL_ACT_FACTOR : CHOL_ACT_PRIVATE_FACTOR, 0, 0, 0);
  chol_for_each_action<true>(nbk, 0, wg, with_inverse, f);
}

// ---- the end of the solver's launch sequence (k_chol_last_apply of cba_kernels.h, enqueue_cholesky of cba_lib.hip; CBA_CHOL_ENDS=0: off) --------------
// nbk >= 2: launches -1 .. nbk - 2 as above, then ONE launch of nbk workgroups in the place of launch nbk - 1 and the backward substitution
// (k_chol_apply).  Launch nbk - 1 is the rhs row's panel workgroup, y_last = W_nbk,last X_last^T, and the inverse workgroups (last, j < last) that
// finish the last block column of T; here workgroup j, block row j of T, forms y_last and T(j, last) PRIVATELY (the same instructions: the parent
// schedule's pending update P_last-1 of the rhs block included) and goes on to the row sums x_j = sum_{c >= j} T(j, c) y_c.  It writes x only:
// nothing reads T, y or L after the solve, so the launch has no shared block to race on.
CHOL_HD inline int chol_last_apply_workgroups(int nbk) { return nbk; }

// f(CholRef) for every block workgroup j of the last launch reads
template <bool EARLY, class F>
inline void chol_last_apply_for_each_read(int nbk, int j, F&& f) {
  const int last = nbk - 1;
  const auto rd = [&](int buf, int bi, int bj) { f(CholRef{buf, bi, bj}); };
  rd(CHOL_W, nbk, last); rd(CHOL_XINV, last, 0);                              // y_last
  if (!EARLY) { rd(CHOL_W, nbk, last - 1); rd(CHOL_W, last, last - 1); }      // ... behind the pending update of the parent schedule
  if (j < last) {                                                             // T(j, last): the term of panel last - 1, then X_last
    if (last - 1 != j) rd(CHOL_T, j, last);
    rd(CHOL_T, j, last - 1); rd(CHOL_W, last, last - 1);
  } else {
    rd(CHOL_T, last, last);
  }
  for (int c = j; c < last; ++c) { rd(CHOL_T, j, c); rd(CHOL_W, nbk, c); }    // the row sums over the finished columns
}

// f(CholAct, i, j, m) for what workgroup j does to ITS OWN copy of the rhs block (nbk, last), in program order (every workgroup the same)
template <bool EARLY, class F>
inline void chol_last_apply_for_each_action(int nbk, int j, F&& f) {
  (void)j;
  const int last = nbk - 1;
  if (!EARLY) f(CHOL_ACT_APPLY, nbk, last, last - 1);
  f(CHOL_ACT_SOLVE, nbk, last, last);
}

}  // namespace cba
