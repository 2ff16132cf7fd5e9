// Stand-alone check of csrc/commit_next.h: the finalize block (a whole DevCtrl) and the other workgroups of the append
// launch (a CommitRegs filled from the same block) must compute the same next round - for committed rounds, faulted rounds,
// rounds that run into the iteration cap, the misses threshold, the node / border capacity and the border table's size.
// Prints "ok <cases>" or the first difference.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <random>
#include "commit_next.h"

using namespace sffk;

// (the workgroups' registers: commit_regs_load is the list of fields hand_request loads - a field commit_next_round starts
// to read without it being on that list stays zero here as it would there, and the comparison below fails.  The border
// count before the round reaches them beside the block, KH_NB0)
static CommitRegs regs_of(const DevCtrl& c) { return commit_regs_load(&c, c.n_borders); }

#define SAME(field) do { if ((long long)k.field != (long long)c.field) { \
  printf("case %d: %s differs: regs %lld block %lld\n", t, #field, (long long)k.field, (long long)c.field); return 1; } } while (0)

int main() {
  std::mt19937_64 rng(12345);
  auto pick = [&](long long lo, long long hi) { return (long long)(lo + (long long)(rng() % (unsigned long long)(hi - lo + 1))); };
  int cases = 0, faults = 0, capped = 0, over = 0;
  for (int t = 0; t < 200000; ++t) {
    DevForestView f;
    memset(&f, 0, sizeof f);
    f.threshold_misses = (int)pick(1, 8);
    f.max_iterations = (int)pick(1, 100000);
    f.node_cap = (int)pick(64, 40000);
    f.border_cap = (int)pick(8, 4000);
    f.bt_mask = (1ULL << pick(4, 14)) - 1ULL;
    f.words_per = t & 1 ? 6 : 3;
    f.prio.n_heaps = (t % 5 == 0) ? 4 : 0;
    DevCtrl c;
    memset(&c, 0, sizeof c);
    // a block as round_begin_next leaves it for a round of n samples
    const int n = (int)pick(1, 3000);
    c.act_cnt = n + (int)pick(0, 40) * (int)pick(0, 1);
    c.n_act = n;
    c.round = (int)pick(1, f.threshold_misses);
    c.iter0 = (int)pick(0, f.max_iterations);
    c.iter = c.iter0 + n;
    c.N0 = c.n_nodes = (int)pick(1, 30000);
    c.n_borders = (int)pick(0, 3000);
    c.frontier_n = (int)pick(0, 30000);
    c.act_sel = (int)pick(0, 1);
    c.solved = pick(0, 50) == 0;
    c.words_base = (unsigned long long)pick(0, 1LL << 40);
    c.cursor = c.words_base + (unsigned long long)f.words_per * (unsigned long long)n;
    c.rounds = (unsigned long long)pick(1, 5000);
    c.round_nodes = (unsigned long long)pick(1LL << 20, 1LL << 40);
    c.round_queries = (unsigned long long)pick(1LL << 20, 1LL << 40);
    c.epoch = (unsigned long long)pick(0, 1LL << 33);
    c.in_wave = 1;
    const int n_acc = (int)pick(0, n), n_ev = (int)pick(0, n - n_acc);
    const bool faulted = pick(0, 9) == 0;
    CommitRegs k = regs_of(c), ka = regs_of(c);
    commit_next_round(f, &c, n_acc, n_ev, faulted);
    commit_next_round(f, &k, n_acc, n_ev, faulted);
    commit_applied(&ka, faulted);
    // what the other workgroups read off their registers
    SAME(app_n); SAME(n_act); SAME(halt);
    if (ka.app_n != c.app_n) { printf("case %d: commit_applied app_n %d block %d\n", t, ka.app_n, c.app_n); return 1; }
    if (!faulted) {
      SAME(app_N0); SAME(app_fn0); SAME(app_act_sel); SAME(app_act_cnt); SAME(iter0_app); SAME(app_nb0); SAME(epoch);
      SAME(act_sel); SAME(act_cnt); SAME(round); SAME(n_nodes); SAME(n_borders); SAME(frontier_n); SAME(fault);
      if (c.n_act > 0) { SAME(words_base); SAME(N0); SAME(iter0); SAME(iter); }
      if (ka.app_N0 != c.app_N0 || ka.app_fn0 != c.app_fn0 || ka.app_act_sel != c.app_act_sel || ka.app_act_cnt != c.app_act_cnt ||
          ka.iter0_app != c.iter0_app || ka.app_nb0 != c.app_nb0 || ka.epoch != c.epoch) { printf("case %d: commit_applied differs\n", t); return 1; }
      if (c.n_act > 0 && c.n_act < c.act_cnt) ++capped;
      if (c.fault) ++over;
    } else {
      ++faults;
      if (c.halt != 1 || c.app_n != 0 || c.n_act != 0 || c.iter != c.iter0) { printf("case %d: roll-back\n", t); return 1; }
    }
    ++cases;
  }
  if (!faults || !capped || !over) { printf("cases missing: faults %d capped %d capacity %d\n", faults, capped, over); return 1; }
  printf("ok %d\n", cases);
  return 0;
}
