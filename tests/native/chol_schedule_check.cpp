// Replay of the launch geometry of the blocked Cholesky (csrc/chol_schedule.h) on the host, for nbk = 1 .. 40 column blocks (nbk = 1: the rhs
// row is the only panel block of the only launch; with and without the inverse role), both schedules.  Per launch:
//   * the workgroup counts of chol_counts are what chol_decode hands out roles for, every role block is inside the matrix;
//   * every block (work matrix, inverse slot, side slot, T) is written by at most one workgroup;
//   * no workgroup reads a block another workgroup of the same launch writes;
//   * an update P_m(i, j) reads L_im and L_jm solved by an earlier launch, or the workgroup's own L_im of this launch, or — L_jm only — a private
//     copy from side slot m and X_m; the side slot was written by an earlier launch with the complete block (m + 1, m);
//   * a panel solve finds its block complete and the diagonal block factored by an earlier launch.
// Over the factorisation every block (i, j) receives P_0 .. P_j-1 once each, ascending, then is solved (factored) once.  The early schedule
// also has column block k + 1 complete at the end of launch k — the parent's schedule passes everything but that.
// Exit status 0 and "all checks passed", or the first violation.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <tuple>
#include <vector>

#include "chol_schedule.h"

using namespace cba;

namespace {

[[noreturn]] void die(const char* what, bool early, int nbk, int k, int wg, int i, int j, int m) {
  std::printf("FAILED (%s schedule, nbk %d, launch %d, workgroup %d): %s [block (%d, %d), term %d]\n", early ? "early" : "parent", nbk, k, wg, what, i, j, m);
  std::exit(1);
}

struct Block {
  int applied = 0;          // P_0 .. P_applied-1 are in
  int last_apply = -2;      // launch of the last update
  int solved = -2;          // launch that solved (factored) it, -2: not yet
  int solved_wg = -1;
};

template <bool EARLY>
void replay(int nbk, bool with_inverse) {
  // blocks (i, j), j <= i <= nbk, j < nbk
  std::vector<std::vector<Block>> blk(nbk + 1, std::vector<Block>(nbk));
  std::vector<int> side_written(nbk + 1, -2);  // launch that wrote side slot s
  for (int k = -1; k < nbk; ++k) {
    const CholCounts cnt = chol_counts<EARLY>(nbk, k, with_inverse);
    if (cnt.panel < 1 || cnt.trailing < 0 || cnt.inverse < 0) die("workgroup counts", EARLY, nbk, k, -1, 0, 0, 0);
    // ---- who writes what
    std::map<std::tuple<int, int, int>, int> writer;
    for (int wg = 0; wg < cnt.total(); ++wg) {
      const CholWork w = chol_decode<EARLY>(nbk, k, wg, with_inverse);
      const int want = (k < 0) ? CHOL_FACTOR0 : wg < cnt.panel ? CHOL_PANEL : wg < cnt.panel + cnt.trailing ? CHOL_TRAILING : CHOL_INVERSE;
      if (w.role != want) die("role of a workgroup", EARLY, nbk, k, wg, w.bi, w.bj, 0);
      if (w.role == CHOL_PANEL && !(w.bi > k && w.bi <= nbk && w.bj == k)) die("panel block outside the matrix", EARLY, nbk, k, wg, w.bi, w.bj, 0);
      if (w.role == CHOL_TRAILING && !(w.bj > k && w.bj < w.bi && w.bi <= nbk && w.bj < nbk)) die("trailing block outside the matrix", EARLY, nbk, k, wg, w.bi, w.bj, 0);
      if (w.role == CHOL_INVERSE && !(w.bi >= k && w.bi < nbk && w.bj >= 0 && w.bj < k)) die("block of T outside the matrix", EARLY, nbk, k, wg, w.bi, w.bj, 0);
      chol_for_each_access<EARLY>(nbk, k, wg, with_inverse, [&](CholRef r, bool write) {
        if (r.buf == CHOL_SIDE && !(EARLY && r.i >= 0 && chol_side_slot(nbk, r.i) < chol_xinv_blocks(nbk))) die("side slot outside the buffer", EARLY, nbk, k, wg, r.i, r.j, 0);
        if (r.buf == CHOL_XINV && !(r.i >= 0 && r.i <= nbk)) die("inverse slot outside the buffer", EARLY, nbk, k, wg, r.i, r.j, 0);
        if (!write) return;
        const auto key = std::make_tuple(r.buf, r.i, r.j);
        const auto it = writer.find(key);
        if (it != writer.end() && it->second != wg) die("a block is written by two workgroups", EARLY, nbk, k, wg, r.i, r.j, r.buf);
        writer[key] = wg;
      });
    }
    // ---- nobody reads what another workgroup writes
    for (int wg = 0; wg < cnt.total(); ++wg)
      chol_for_each_access<EARLY>(nbk, k, wg, with_inverse, [&](CholRef r, bool write) {
        if (write) return;
        const auto it = writer.find(std::make_tuple(r.buf, r.i, r.j));
        if (it != writer.end() && it->second != wg) die("a workgroup reads a block another workgroup of the launch writes", EARLY, nbk, k, wg, r.i, r.j, r.buf);
        if (r.buf == CHOL_SIDE && !(side_written[r.i] >= -1 && side_written[r.i] < k)) die("side slot read before an earlier launch wrote it", EARLY, nbk, k, wg, r.i, 0, 0);
      });
    // ---- the arithmetic, in each workgroup's program order
    for (int wg = 0; wg < cnt.total(); ++wg) {
      bool reads_side[2] = {false, false};  // side slot k and X_k: the private copy of L_k+1,k
      chol_for_each_access<EARLY>(nbk, k, wg, with_inverse, [&](CholRef r, bool write) {
        if (!write && r.buf == CHOL_SIDE && r.i == k) reads_side[0] = true;
        if (!write && r.buf == CHOL_XINV && r.i == k) reads_side[1] = true;
      });
      const auto reads = [&](int buf, int i, int j) {
        bool found = false;
        chol_for_each_access<EARLY>(nbk, k, wg, with_inverse, [&](CholRef r, bool write) { found = found || (!write && r.buf == buf && r.i == i && r.j == j); });
        return found;
      };
      chol_for_each_action<EARLY>(nbk, k, wg, with_inverse, [&](int act, int i, int j, int m) {
        if (!(j >= 0 && j < nbk && i >= j && i <= nbk)) die("action outside the matrix", EARLY, nbk, k, wg, i, j, m);
        Block& b = blk[i][j];
        const auto w_it = writer.find(std::make_tuple((int)CHOL_W, i, j));
        if (w_it == writer.end() || w_it->second != wg) die("an action on a block the workgroup does not write", EARLY, nbk, k, wg, i, j, m);
        if (b.solved != -2) die("an action on a finished block", EARLY, nbk, k, wg, i, j, m);
        if (act == CHOL_ACT_APPLY) {
          if (m != b.applied || m >= j) die("updates out of order, repeated or too many", EARLY, nbk, k, wg, i, j, m);
          // operands L_im and L_jm
          const Block& li = blk[i][m];
          const bool own_li = li.solved == k && li.solved_wg == wg;
          if (!(own_li || (li.solved >= -1 && li.solved < k && reads(CHOL_W, i, m)))) die("update reads an L_im that is not there", EARLY, nbk, k, wg, i, j, m);
          if (i != j) {
            const Block& lj = blk[j][m];
            const bool from_w = lj.solved >= -1 && lj.solved < k && reads(CHOL_W, j, m);
            const bool private_copy = m == k && j == k + 1 && reads_side[0] && reads_side[1];
            if (!(from_w || private_copy)) die("update reads an L_jm that is not there", EARLY, nbk, k, wg, i, j, m);
          }
          ++b.applied;
          b.last_apply = k;
        } else if (act == CHOL_ACT_SOLVE) {
          if (!(i > j && j == k && m == j)) die("panel solve of a block outside panel k", EARLY, nbk, k, wg, i, j, m);
          if (b.applied != j) die("panel solve of an incomplete block", EARLY, nbk, k, wg, i, j, m);
          if (EARLY && b.last_apply >= k) die("the block was completed in the launch that solves it", EARLY, nbk, k, wg, i, j, m);
          if (!(blk[j][j].solved >= -1 && blk[j][j].solved < k)) die("panel solve before an earlier launch factored the diagonal block", EARLY, nbk, k, wg, i, j, m);
          b.solved = k; b.solved_wg = wg;
        } else {
          if (!(i == j && m == i && i == k + 1)) die("factorisation of another block than D_k+1", EARLY, nbk, k, wg, i, j, m);
          if (b.applied != i) die("factorisation of an incomplete diagonal block", EARLY, nbk, k, wg, i, j, m);
          b.solved = k; b.solved_wg = wg;
        }
      });
    }
    // ---- side slots written in this launch hold a complete block
    for (const auto& kv : writer)
      if (std::get<0>(kv.first) == CHOL_SIDE) {
        const int s = std::get<1>(kv.first);
        if (s != k + 1 || s + 1 > nbk || blk[s + 1][s].applied != s || blk[s + 1][s].solved != -2) die("side slot written with an incomplete block", EARLY, nbk, k, kv.second, s + 1, s, 0);
        if (s >= 1) {  // the writer is the workgroup that completed the block in this launch
          const auto w_it = writer.find(std::make_tuple((int)CHOL_W, s + 1, s));
          if (w_it == writer.end() || w_it->second != kv.second) die("side slot written by another workgroup than the one completing the block", EARLY, nbk, k, kv.second, s + 1, s, 0);
        }
        side_written[s] = k;
      }
    // ---- the early schedule: column block k + 1 is complete when launch k ends
    if (EARLY && k + 1 < nbk)
      for (int i = k + 2; i <= nbk; ++i)
        if (blk[i][k + 1].applied != k + 1) die("column block k + 1 is not complete at the end of launch k", EARLY, nbk, k, -1, i, k + 1, blk[i][k + 1].applied);
  }
  for (int j = 0; j < nbk; ++j)
    for (int i = j; i <= nbk; ++i)
      if (blk[i][j].applied != j || blk[i][j].solved == -2) die("a block is not finished at the end", EARLY, nbk, nbk, -1, i, j, blk[i][j].applied);
}

}  // namespace

int main() {
  for (int nbk = 1; nbk <= 40; ++nbk)
    for (int with_inverse = 0; with_inverse < 2; ++with_inverse) {
      replay<true>(nbk, with_inverse != 0);
      replay<false>(nbk, with_inverse != 0);
    }
  // the grid of the early schedule against the parent's: column k + 1 moved from the trailing to the panel workgroups
  for (int nbk = 1; nbk <= 40; ++nbk)
    for (int k = 1; k < nbk; ++k) {
      const CholCounts e = chol_counts<true>(nbk, k, true), p = chol_counts<false>(nbk, k, true);
      if (e.panel != p.panel || e.inverse != p.inverse || e.trailing != p.trailing - (nbk - k - 1)) die("workgroup counts against the parent's", true, nbk, k, -1, 0, 0, 0);
    }
  std::printf("all checks passed\n");
  return 0;
}
