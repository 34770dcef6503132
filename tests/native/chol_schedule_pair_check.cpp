// Replay of the solver's launch sequence of the blocked Cholesky with the paired first launch (csrc/chol_schedule.h: launches -1 and 0 as ONE launch,
// every workgroup factoring D_0 privately) on the host, for nbk = 1 .. 40 column blocks with and without T, early schedule, folded end (the regular
// launches end at nbk - 2; nbk = 1 is not paired and keeps its two launches).  Per launch:
//   * every block (work matrix, inverse slot, side slot, T) is written by at most one workgroup;
//   * no workgroup reads a block another workgroup of the same launch writes — D_0 and U_10 come from side slots the producers of the work matrix
//     filled, because workgroup b == 1 overwrites both blocks of the work matrix in place;
//   * every block (i, j) receives P_0 .. P_j-1 once each, ascending, before its solve, every diagonal block before its factorisation; a panel solve
//     of column 0 in the paired launch follows the workgroup's OWN factorisation of D_0 (stored or private), an update with a private L_10 too.
// At the end the history of every block of W, Xinv and T — which terms it took in which order, solved, factored, written — is compared with the
// unpaired sequence's: k_chol_last_apply finds what it finds today.
// Exit status 0 and "all checks passed", or the first violation.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <tuple>
#include <vector>

#include "chol_schedule.h"

using namespace cba;

namespace {

[[noreturn]] void die(const char* what, bool pair, int nbk, int k, int wg, int i, int j, int m) {
  std::printf("FAILED (%s sequence, nbk %d, launch %d, workgroup %d): %s [block (%d, %d), term %d]\n", pair ? "paired" : "unpaired", nbk, k, wg, what, i, j, m);
  std::exit(1);
}

struct Block {
  int applied = 0;      // P_0 .. P_applied-1 are in
  int last_apply = -2;  // launch of the last update
  int solved = -2;      // launch that solved (factored) it, -2: not yet
  int solved_wg = -1;
};

using Key = std::tuple<int, int, int>;            // buffer, i, j
using History = std::map<Key, std::vector<int>>;  // what happened to a block of W, Xinv or T, in order

constexpr int PRODUCER = -1;  // "launch" of the kernels that write the work matrix (and, for the paired sequence, the side slots of D_0 and U_10)

// the sequence's launches through one interface: launch k of the paired sequence is the paired one where k == 0
struct Seq {
  int nbk;
  bool with_inverse, pair;
  bool paired(int k) const { return pair && k == 0; }
  CholCounts counts(int k) const { return paired(k) ? chol_pair_counts(nbk) : chol_counts<true>(nbk, k, with_inverse); }
  CholWork decode(int k, int wg) const { return paired(k) ? chol_pair_decode(nbk, wg, with_inverse) : chol_decode<true>(nbk, k, wg, with_inverse); }
  template <class F>
  void access(int k, int wg, F&& f) const {
    if (paired(k)) chol_pair_for_each_access(nbk, wg, with_inverse, f); else chol_for_each_access<true>(nbk, k, wg, with_inverse, f);
  }
  template <class F>
  void action(int k, int wg, F&& f) const {
    if (paired(k)) chol_pair_for_each_action(nbk, wg, with_inverse, f); else chol_for_each_action<true>(nbk, k, wg, with_inverse, f);
  }
};

History replay(int nbk, bool with_inverse, bool want_pair) {
  const bool pair = want_pair && chol_pair_applies(nbk, true, true);
  const Seq seq{nbk, with_inverse, pair};
  const int d0 = chol_side_d0(nbk);
  if (chol_side_slot(nbk, d0) >= chol_xinv_blocks(nbk)) die("the side slot of D_0 is outside the buffer", pair, nbk, -1, -1, 0, 0, 0);
  std::vector<std::vector<Block>> blk(nbk + 1, std::vector<Block>(nbk));
  std::vector<int> side_written(nbk + 2, -2);  // launch that wrote side slot s (slot nbk + 1: D_0)
  if (pair) side_written[0] = side_written[d0] = PRODUCER;
  History hist;
  const int k_end = (nbk >= 2) ? nbk - 1 : nbk;  // the folded end: launch nbk - 1 belongs to k_chol_last_apply
  if (chol_first_launch(pair) != (pair ? 0 : -1)) die("first launch of the sequence", pair, nbk, -1, -1, 0, 0, 0);
  for (int k = chol_first_launch(pair); k < k_end; ++k) {
    const CholCounts cnt = seq.counts(k);
    if (cnt.panel < 1 || cnt.trailing < 0 || cnt.inverse < 0) die("workgroup counts", pair, nbk, k, -1, 0, 0, 0);
    if (seq.paired(k) && !(cnt.panel == nbk && cnt.trailing == 0 && cnt.inverse == 0)) die("the paired launch has nbk panel workgroups and no other role", pair, nbk, k, -1, 0, 0, 0);
    // ---- who writes what
    std::map<Key, int> writer;
    for (int wg = 0; wg < cnt.total(); ++wg) {
      const CholWork w = seq.decode(k, wg);
      if (seq.paired(k) && !(w.role == CHOL_PANEL && w.factor_first && w.store_first == (w.bi == 1) && w.critical == (w.bi == 1))) die("role in the paired launch", pair, nbk, k, wg, w.bi, w.bj, 0);
      if (!seq.paired(k) && (w.factor_first || w.store_first)) die("a private factorisation outside the paired launch", pair, nbk, k, wg, w.bi, w.bj, 0);
      seq.access(k, wg, [&](CholRef r, bool write) {
        if (r.buf == CHOL_SIDE && !(r.i >= 0 && chol_side_slot(nbk, r.i) < chol_xinv_blocks(nbk))) die("side slot outside the buffer", pair, nbk, k, wg, r.i, r.j, 0);
        if (r.buf == CHOL_XINV && !(r.i >= 0 && r.i <= nbk)) die("inverse slot outside the buffer", pair, nbk, k, wg, r.i, r.j, 0);
        if ((r.buf == CHOL_W || r.buf == CHOL_T) && !(r.i >= 0 && r.i <= nbk && r.j >= 0 && r.j <= nbk)) die("block outside the matrix", pair, nbk, k, wg, r.i, r.j, 0);
        if (!write) return;
        const Key key{r.buf, r.i, r.j};
        const auto it = writer.find(key);
        if (it != writer.end() && it->second != wg) die("a block is written by two workgroups", pair, nbk, k, wg, r.i, r.j, r.buf);
        writer[key] = wg;
      });
    }
    // ---- nobody reads what another workgroup writes; side slots were filled earlier
    for (int wg = 0; wg < cnt.total(); ++wg)
      seq.access(k, wg, [&](CholRef r, bool write) {
        if (write) return;
        const auto it = writer.find(Key{r.buf, r.i, r.j});
        if (it != writer.end() && it->second != wg) die("a workgroup reads a block another workgroup of the launch writes", pair, nbk, k, wg, r.i, r.j, r.buf);
        if (r.buf == CHOL_SIDE && !(side_written[r.i] >= PRODUCER && side_written[r.i] < k)) die("side slot read before an earlier launch wrote it", pair, nbk, k, wg, r.i, 0, 0);
      });
    // ---- the arithmetic, in each workgroup's program order
    for (int wg = 0; wg < cnt.total(); ++wg) {
      const CholWork w = seq.decode(k, wg);
      const auto reads = [&](int buf, int i, int j) {
        bool found = false;
        seq.access(k, wg, [&](CholRef r, bool write) { found = found || (!write && r.buf == buf && r.i == i && r.j == j); });
        return found;
      };
      bool own_x = false;  // the workgroup has factored D_k itself in this launch (the paired launch: X_0 in its own LDS)
      seq.action(k, wg, [&](int act, int i, int j, int m) {
        if (!(j >= 0 && j < nbk && i >= j && i <= nbk)) die("action outside the matrix", pair, nbk, k, wg, i, j, m);
        Block& b = blk[i][j];
        if (act == CHOL_ACT_PRIVATE_FACTOR) {
          if (!(seq.paired(k) && i == 0 && j == 0 && !w.store_first && !own_x)) die("private factorisation of another block than D_0, or twice", pair, nbk, k, wg, i, j, m);
          if (!reads(CHOL_SIDE, d0, 0)) die("private factorisation without the side copy of D_0", pair, nbk, k, wg, i, j, m);
          own_x = true;
          return;
        }
        const auto w_it = writer.find(Key{CHOL_W, i, j});
        if (w_it == writer.end() || w_it->second != wg) die("an action on a block the workgroup does not write", pair, nbk, k, wg, i, j, m);
        if (b.solved != -2) die("an action on a finished block", pair, nbk, k, wg, i, j, m);
        if (act == CHOL_ACT_APPLY) {
          if (m != b.applied || m >= j) die("updates out of order, repeated or too many", pair, nbk, k, wg, i, j, m);
          const Block& li = blk[i][m];
          const bool own_li = li.solved == k && li.solved_wg == wg;
          if (!(own_li || (li.solved >= -1 && li.solved < k && reads(CHOL_W, i, m)))) die("update reads an L_im that is not there", pair, nbk, k, wg, i, j, m);
          if (i != j) {
            const Block& lj = blk[j][m];
            const bool from_w = lj.solved >= -1 && lj.solved < k && reads(CHOL_W, j, m);
            const bool private_copy = m == k && j == k + 1 && reads(CHOL_SIDE, k, 0) && (seq.paired(k) ? own_x : reads(CHOL_XINV, k, 0));
            if (!(from_w || private_copy)) die("update reads an L_jm that is not there", pair, nbk, k, wg, i, j, m);
          }
          ++b.applied;
          b.last_apply = k;
          hist[Key{CHOL_W, i, j}].push_back(m);
        } else if (act == CHOL_ACT_SOLVE) {
          if (!(i > j && j == k && m == j)) die("panel solve of a block outside panel k", pair, nbk, k, wg, i, j, m);
          if (b.applied != j) die("panel solve of an incomplete block", pair, nbk, k, wg, i, j, m);
          if (b.last_apply >= k) die("the block was completed in the launch that solves it", pair, nbk, k, wg, i, j, m);
          const bool earlier = blk[j][j].solved >= -1 && blk[j][j].solved < k && reads(CHOL_XINV, j, 0);
          if (!(seq.paired(k) ? own_x : earlier)) die("panel solve without the inverse of the diagonal block", pair, nbk, k, wg, i, j, m);
          b.solved = k; b.solved_wg = wg;
          hist[Key{CHOL_W, i, j}].push_back(1000 + j);
        } else if (act == CHOL_ACT_FACTOR) {
          const bool first = seq.paired(k) && i == 0 && w.store_first && !own_x;  // D_0 in the paired launch, by the workgroup that stores it
          if (!(i == j && m == i && (i == k + 1 || first))) die("factorisation of another block than D_k+1", pair, nbk, k, wg, i, j, m);
          if (b.applied != i) die("factorisation of an incomplete diagonal block", pair, nbk, k, wg, i, j, m);
          if (first) {
            if (!reads(CHOL_SIDE, d0, 0)) die("D_0 is not read from its side slot", pair, nbk, k, wg, i, j, m);
            own_x = true;
          }
          if (writer.find(Key{CHOL_XINV, i, 0}) == writer.end() || writer[Key{CHOL_XINV, i, 0}] != wg) die("a factorisation that does not store the inverse", pair, nbk, k, wg, i, j, m);
          b.solved = k; b.solved_wg = wg;
          hist[Key{CHOL_W, i, j}].push_back(2000);
        } else {
          die("unknown action", pair, nbk, k, wg, i, j, m);
        }
      });
      if (seq.paired(k) && !own_x) die("a workgroup of the paired launch without its own X_0", pair, nbk, k, wg, w.bi, w.bj, 0);
      // what the launch leaves in Xinv and T: the inverse role adds the term of panel k - 1 and finalises row k; the others store a diagonal block
      seq.access(k, wg, [&](CholRef r, bool write) {
        if (!write) return;
        if (r.buf == CHOL_XINV) hist[Key{CHOL_XINV, r.i, 0}].push_back(1);
        if (r.buf == CHOL_T) hist[Key{CHOL_T, r.i, r.j}].push_back(w.role == CHOL_INVERSE ? 2 * (k - 1) + (w.bi == k ? 1 : 0) : -1);
      });
    }
    // ---- side slots written in this launch hold a complete block, written by the workgroup that completed it
    for (const auto& kv : writer)
      if (std::get<0>(kv.first) == CHOL_SIDE) {
        const int s = std::get<1>(kv.first);
        if (pair && (s == 0 || s == d0)) die("a launch writes a side slot of the producers", pair, nbk, k, kv.second, s, 0, 0);
        if (s != k + 1 || s + 1 > nbk || blk[s + 1][s].applied != s || blk[s + 1][s].solved != -2) die("side slot written with an incomplete block", pair, nbk, k, kv.second, s + 1, s, 0);
        if (s >= 1) {
          const auto w_it = writer.find(Key{CHOL_W, s + 1, s});
          if (w_it == writer.end() || w_it->second != kv.second) die("side slot written by another workgroup than the one completing the block", pair, nbk, k, kv.second, s + 1, s, 0);
        }
        side_written[s] = k;
      }
    // ---- column block k + 1 is complete when launch k ends
    if (k + 1 < nbk)
      for (int i = k + 2; i <= nbk; ++i)
        if (blk[i][k + 1].applied != k + 1) die("column block k + 1 is not complete at the end of launch k", pair, nbk, k, -1, i, k + 1, blk[i][k + 1].applied);
  }
  return hist;
}

}  // namespace

int main() {
  int paired = 0;
  for (int nbk = 1; nbk <= 40; ++nbk)
    for (int with_inverse = 0; with_inverse < 2; ++with_inverse) {
      const History p = replay(nbk, with_inverse != 0, true), u = replay(nbk, with_inverse != 0, false);
      paired += chol_pair_applies(nbk, true, true) ? 1 : 0;
      // block for block: the same terms in the same order, the same solves, factorisations and stores
      for (const auto& kv : u) {
        const auto it = p.find(kv.first);
        if (it == p.end() || it->second != kv.second)
          die("a block's history differs from the unpaired sequence's", true, nbk, nbk, std::get<0>(kv.first), std::get<1>(kv.first), std::get<2>(kv.first), 0);
      }
      if (p.size() != u.size()) die("the paired sequence touches a block the unpaired one does not", true, nbk, nbk, -1, 0, 0, 0);
    }
  if (paired != 2 * 39) die("the pairing applies from two blocks on", true, 0, 0, -1, 0, 0, paired);
  if (chol_pair_applies(5, false, true) || chol_pair_applies(5, true, false) || chol_pair_applies(1, true, true)) die("the pairing applies where it must not", true, 0, 0, -1, 0, 0, 0);
  std::printf("all checks passed\n");
  return 0;
}
