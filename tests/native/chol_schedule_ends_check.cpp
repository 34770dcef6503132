// Replay of the solver's launch sequence of the dense solve with its last launch folded into the backward substitution (csrc/chol_schedule.h:
// launches -1 .. nbk - 2 of k_chol_step, then k_chol_last_apply), for nbk = 1 .. 40 column blocks and both schedules.  With T and nbk >= 2 that is
// the new sequence; nbk = 1 and the factorisation without T (what cba_parameter_covariance enqueues, and CBA_CHOL_ENDS=0) keep every launch of the
// old one and are replayed as such.  Per size:
//   * every block of the work matrix, inverse slot, side slot and block of T is written by at most one workgroup of a launch;
//   * no workgroup reads a block another workgroup of the same launch writes (the last launch writes x only: chol_last_apply_for_each_read is all
//     it touches of the shared buffers);
//   * every block receives P_0 .. P_j-1 once each, ascending, before it is solved or factored — the rhs block (nbk, last) in every workgroup's
//     private copy of the last launch, whose operands were solved by earlier launches;
//   * block (j, i) of T receives the terms of the panels j .. i - 1 once each, ascending, from operands that are final, and is finished with X_i
//     — the last block column in the private copy of workgroup j of the last launch;
//   * the row sums of workgroup j find T(j, j .. last - 1) and the rhs blocks 0 .. last - 1 final, written by earlier launches, and named among its reads.
// Exit status 0 and "all checks passed", or the first violation.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
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
  int applied = 0;   // P_0 .. P_applied-1 are in
  int solved = -2;   // launch that solved (factored) it, -2: not yet
};
struct TBlock {
  int terms = 0;     // block (j, i) of T: the terms of panels j .. j + terms - 1 are in
  int final_at = -2; // launch that finished it
};

template <bool EARLY>
void replay(int nbk, bool with_T) {
  const bool fold = with_T && nbk >= 2;
  const int last = nbk - 1, n_step_launches = fold ? nbk - 1 : nbk;  // launches -1 .. n_step_launches - 1 of k_chol_step
  std::vector<std::vector<Block>> blk(nbk + 1, std::vector<Block>(nbk));
  std::vector<std::vector<TBlock>> T(nbk, std::vector<TBlock>(nbk));
  const auto before = [](int launch, int k) { return launch >= -1 && launch < k; };
  for (int k = -1; k < n_step_launches; ++k) {
    const CholCounts cnt = chol_counts<EARLY>(nbk, k, with_T);
    std::map<std::tuple<int, int, int>, int> writer;
    for (int wg = 0; wg < cnt.total(); ++wg)
      chol_for_each_access<EARLY>(nbk, k, wg, with_T, [&](CholRef r, bool write) {
        if (!write) return;
        const auto key = std::make_tuple(r.buf, r.i, r.j);
        const auto it = writer.find(key);
        if (it != writer.end() && it->second != wg) die("a block is written by two workgroups", EARLY, nbk, k, wg, r.i, r.j, r.buf);
        writer[key] = wg;
      });
    for (int wg = 0; wg < cnt.total(); ++wg)
      chol_for_each_access<EARLY>(nbk, k, wg, with_T, [&](CholRef r, bool write) {
        if (write) return;
        const auto it = writer.find(std::make_tuple(r.buf, r.i, r.j));
        if (it != writer.end() && it->second != wg) die("a workgroup reads a block another workgroup of the launch writes", EARLY, nbk, k, wg, r.i, r.j, r.buf);
      });
    // the factor, in each workgroup's program order (operands and side slots: tests/native/chol_schedule_check.cpp replays those)
    for (int wg = 0; wg < cnt.total(); ++wg)
      chol_for_each_action<EARLY>(nbk, k, wg, with_T, [&](int act, int i, int j, int m) {
        Block& b = blk[i][j];
        if (b.solved != -2) die("an action on a finished block", EARLY, nbk, k, wg, i, j, m);
        if (act == CHOL_ACT_APPLY) {
          if (m != b.applied || m >= j) die("updates out of order, repeated or too many", EARLY, nbk, k, wg, i, j, m);
          ++b.applied;
        } else {
          if (b.applied != j) die("an incomplete block is solved or factored", EARLY, nbk, k, wg, i, j, m);
          if (act == CHOL_ACT_SOLVE && !before(blk[j][j].solved, k)) die("panel solve before an earlier launch factored the diagonal block", EARLY, nbk, k, wg, i, j, m);
          b.solved = k;
        }
      });
    // T: the diagonal block of a factored D_i is X_i^T; the inverse workgroups (bi >= k, bj < k) add the term of panel k - 1
    if (!with_T) continue;
    for (int i = 0; i < nbk; ++i)
      if (blk[i][i].solved == k) T[i][i].final_at = k;
    for (int wg = cnt.panel + cnt.trailing; wg < cnt.total(); ++wg) {
      const CholWork w = chol_decode<EARLY>(nbk, k, wg, with_T);
      const int bi = w.bi, bj = w.bj, m = k - 1;
      TBlock& t = T[bj][bi];
      if (w.role != CHOL_INVERSE || t.final_at != -2) die("inverse role on a finished block of T", EARLY, nbk, k, wg, bj, bi, m);
      if (bj + t.terms != m) die("terms of T out of order, repeated or missing", EARLY, nbk, k, wg, bj, bi, m);
      if (!before(T[bj][m].final_at, k)) die("a term of T reads a T_jm that is not final", EARLY, nbk, k, wg, bj, m, m);
      if (!before(blk[bi][m].solved, k)) die("a term of T reads an L_im that is not solved", EARLY, nbk, k, wg, bi, m, m);
      ++t.terms;
      if (bi == k) {
        if (!before(blk[k][k].solved, k)) die("T is finished with an X_k that is not there", EARLY, nbk, k, wg, bj, bi, m);
        t.final_at = k;
      }
    }
  }
  if (fold) {
    if (chol_last_apply_workgroups(nbk) != nbk) die("workgroups of the last launch", EARLY, nbk, last, -1, 0, 0, 0);
    for (int j = 0; j < nbk; ++j) {
      std::set<std::tuple<int, int, int>> reads;
      chol_last_apply_for_each_read<EARLY>(nbk, j, [&](CholRef r) {
        if (r.buf == CHOL_SIDE || (r.buf == CHOL_XINV && r.i != last)) die("the last launch reads a slot it has no use for", EARLY, nbk, last, j, r.i, r.j, r.buf);
        if ((r.buf == CHOL_W && !(r.j >= 0 && r.j < nbk && r.i >= r.j && r.i <= nbk)) || (r.buf == CHOL_T && !(r.i >= 0 && r.i <= r.j && r.j < nbk)))
          die("the last launch reads outside the matrix", EARLY, nbk, last, j, r.i, r.j, r.buf);
        reads.insert(std::make_tuple(r.buf, r.i, r.j));
      });
      const auto has = [&](int buf, int bi, int bj) { return reads.count(std::make_tuple(buf, bi, bj)) != 0; };
      // the private rhs block
      Block y = blk[nbk][last];
      if (y.solved != -2) die("the rhs block of the last panel was solved by an earlier launch", EARLY, nbk, last, j, nbk, last, 0);
      if (!has(CHOL_W, nbk, last)) die("the rhs block is not among the reads", EARLY, nbk, last, j, nbk, last, 0);
      chol_last_apply_for_each_action<EARLY>(nbk, j, [&](int act, int bi, int bj, int m) {
        if (bi != nbk || bj != last) die("the last launch acts on another block than the rhs block", EARLY, nbk, last, j, bi, bj, m);
        if (act == CHOL_ACT_APPLY) {
          if (m != y.applied || m >= last) die("updates of the private rhs block out of order", EARLY, nbk, last, j, bi, bj, m);
          if (!(before(blk[nbk][m].solved, last) && has(CHOL_W, nbk, m) && before(blk[last][m].solved, last) && has(CHOL_W, last, m)))
            die("update of the private rhs block reads an operand that is not there", EARLY, nbk, last, j, bi, bj, m);
          ++y.applied;
        } else if (act == CHOL_ACT_SOLVE) {
          if (y.applied != last) die("the private rhs block is solved incomplete", EARLY, nbk, last, j, bi, bj, m);
          if (!(before(blk[last][last].solved, last) && has(CHOL_XINV, last, 0))) die("the private rhs block is solved without X_last", EARLY, nbk, last, j, bi, bj, m);
          y.solved = last;
        } else {
          die("the last launch factors", EARLY, nbk, last, j, bi, bj, m);
        }
      });
      if (y.solved != last) die("the last launch does not solve the rhs block", EARLY, nbk, last, j, nbk, last, 0);
      // the private block T(j, last)
      if (j < last) {
        const TBlock& t = T[j][last];
        if (t.final_at != -2 || j + t.terms != last - 1) die("T(j, last) does not miss exactly the last term", EARLY, nbk, last, j, j, last, t.terms);
        if (t.terms > 0 && !has(CHOL_T, j, last)) die("the terms T(j, last) has are not among the reads", EARLY, nbk, last, j, j, last, 0);
        if (!(before(T[j][last - 1].final_at, last) && has(CHOL_T, j, last - 1))) die("the last term of T(j, last) reads a T that is not final", EARLY, nbk, last, j, j, last - 1, 0);
        if (!(before(blk[last][last - 1].solved, last) && has(CHOL_W, last, last - 1))) die("the last term of T(j, last) reads an L that is not solved", EARLY, nbk, last, j, last, last - 1, 0);
        if (!(before(blk[last][last].solved, last) && has(CHOL_XINV, last, 0))) die("T(j, last) is finished without X_last", EARLY, nbk, last, j, j, last, 0);
      } else if (!(before(T[last][last].final_at, last) && has(CHOL_T, last, last))) {
        die("T(last, last) is not there", EARLY, nbk, last, j, last, last, 0);
      }
      // the row sums over the finished columns
      for (int c = j; c < last; ++c) {
        if (!(before(T[j][c].final_at, last) && has(CHOL_T, j, c))) die("a row sum reads a block of T that is not final", EARLY, nbk, last, j, j, c, 0);
        if (!(before(blk[nbk][c].solved, last) && has(CHOL_W, nbk, c))) die("a row sum reads a rhs block that is not solved", EARLY, nbk, last, j, nbk, c, 0);
      }
    }
  }
  // everything the sequence leaves in the shared buffers is finished, but for what the last launch keeps private
  for (int j = 0; j < nbk; ++j)
    for (int i = j; i <= nbk; ++i) {
      const bool priv = fold && i == nbk && j == last;
      if (priv ? blk[i][j].solved != -2 : (blk[i][j].applied != j || blk[i][j].solved == -2)) die("a block is not finished at the end", EARLY, nbk, nbk, -1, i, j, blk[i][j].applied);
    }
  if (with_T)
    for (int j = 0; j < nbk; ++j)
      for (int i = j; i < nbk; ++i) {
        const bool priv = fold && i == last && j < last;
        if (priv ? T[j][i].final_at != -2 : T[j][i].final_at == -2) die("a block of T is not finished at the end", EARLY, nbk, nbk, -1, j, i, T[j][i].terms);
      }
}

}  // namespace

int main() {
  for (int nbk = 1; nbk <= 40; ++nbk)
    for (int with_T = 0; with_T < 2; ++with_T) {
      replay<true>(nbk, with_T != 0);
      replay<false>(nbk, with_T != 0);
    }
  std::printf("all checks passed\n");
  return 0;
}
