// commit_next.h — what a committed round does to the control block, written once.
//
// Plain SFF: k_commit ends at its walks and leaves the control block as it found it.  The append launch behind it has one
// extra workgroup (the finalize block, commit_finalize in devforest.hip) that writes the block, and every OTHER workgroup of
// that launch needs the very values the finalize block is about to write (the committed round's size and bases, the next
// round's size, word base, list) - before they are written.  Both sides call commit_next_round: the finalize block on
// the DevCtrl it copied to LDS, the others on a CommitRegs filled from the old block.  What the readers assume and what
// gets written can then not differ.  SFF* keeps the tail inside k_commit (the star stage between the two launches reads
// the block) and calls the same functions there.
//
// The functions are templates over "something with DevCtrl's field names"; they read the forest's limits from the view.
#pragma once
#include <stdint.h>
#include "kernels.h"
#include "sff_pmath.h"

namespace sffk {

// The fields of DevCtrl the three functions below touch, for a workgroup that only derives them (registers).
struct CommitRegs {
  int32_t n_act, halt, n_nodes, iter, round, solved, fault, N0, iter0, n_borders, frontier_n, act_sel, act_cnt;
  int32_t app_n, app_N0, app_fn0, app_act_sel, iter0_app, app_act_cnt, app_nb0;
  unsigned long long cursor, words_base, rounds, round_nodes, round_queries, epoch;
};

// The fields commit_next_round READS, from a control block as the commit found it (everything else starts at zero): the one
// list of them - the append launch's workgroups fill their registers through it, and so does the host check
// (tests/commit_next_harness.cpp).  nb0 = the border count before the round, from where k_commit left it: the block's own
// n_borders word is rewritten with the exact count by a workgroup of the append launch itself (border_finalize).
SFF_HD CommitRegs commit_regs_load(const DevCtrl* c, int32_t nb0) {
  CommitRegs k{};
  k.n_act = c->n_act; k.halt = c->halt; k.iter = c->iter; k.round = c->round; k.solved = c->solved;
  k.N0 = c->N0; k.iter0 = c->iter0; k.n_borders = nb0; k.frontier_n = c->frontier_n;
  k.act_sel = c->act_sel; k.act_cnt = c->act_cnt; k.cursor = c->cursor; k.epoch = c->epoch;
  return k;
}

// Sizes the next round from the active list (already in place, act_cnt entries): src/forest.h:155 - i <
// ThresholdMisses && expandResult && iter < maxIterations.
template <class C> SFF_HD void round_begin_next(const DevForestView& f, C* c) {
  const int cnt = c->act_cnt;
  int n = 0;
  if (c->round < f.threshold_misses && cnt > 0 && c->iter < f.max_iterations && !c->solved) {
    const int left = f.max_iterations - c->iter;
    n = cnt < left ? cnt : left;
  }
  c->n_act = n;
  if (n > 0) {
    // the arrays a round can grow: one node / frontier entry / border per sample at most
    if (c->n_nodes + n > f.node_cap - 8 || c->n_borders + n > f.border_cap) {
      c->fault = SFFK_FAULT_CAPACITY;
      c->halt = 1;
      c->n_act = 0;
    } else if ((unsigned long long)(c->n_borders + n) * 2ULL > f.bt_mask + 1ULL) {
      c->fault = SFFK_FAULT_BORDER_TABLE;
      c->halt = 1;
      c->n_act = 0;
    } else {
      c->round += 1;
      c->iter0 = c->iter;
      c->iter += n;
      c->N0 = c->n_nodes;
      c->words_base = c->cursor;
      c->cursor += (unsigned long long)f.words_per * (unsigned long long)n;
      c->rounds += 1;
      c->round_nodes += (unsigned long long)(c->n_nodes + n);
      c->round_queries += (unsigned long long)n;
    }
  }
}

// A bounded device list overflowed somewhere in the round (or the goal was reached in it): nothing is committed, the
// bookkeeping of the round's begin is rolled back and the host redoes the round on its unbounded path.
template <class C> SFF_HD void commit_roll_back(C* k) {
  const int n = k->n_act;
  k->fault = SFFK_FAULT_LISTS;
  k->halt = 1;
  k->round -= 1;
  k->iter = k->iter0;
  k->cursor = k->words_base;
  k->rounds -= 1;
  k->round_nodes -= (unsigned long long)(k->N0 + n);
  k->round_queries -= (unsigned long long)n;
  k->n_act = 0;
  k->app_n = 0;
}

// The part of the commit that needs no totals: what the append has to apply (the committed round's size and the bases its
// nodes, frontier entries, borders and iteration stamps count from, which list it was), and the commit's epoch.  A faulted
// round is rolled back instead: app_n = 0.  The workgroups of the append launch that create nodes or enter border events
// need nothing else.
template <class C> SFF_HD void commit_applied(C* k, bool faulted) {
  if (faulted) { commit_roll_back(k); return; }
  k->app_n = k->n_act;           // the append applies this commit
  k->app_N0 = k->N0;
  k->app_fn0 = k->frontier_n;
  k->app_act_sel = k->act_sel;
  k->app_act_cnt = k->act_cnt;
  k->iter0_app = k->iter0;
  k->app_nb0 = k->n_borders;
  k->epoch += 1ULL;
}

// The control block behind the commit of a round of k->n_act samples, from the block as the round found it: n_acc
// samples became nodes, n_ev border events were counted (plain SFF: every event - an upper bound until the append launch
// has entered the ones that own their key).  The next round's active list = the slots of this round that were not
// accepted, then the slots the iteration cap kept out of it.
template <class C> SFF_HD void commit_next_round(const DevForestView& f, C* k, int n_acc, int n_ev, bool faulted) {
  commit_applied(k, faulted);
  if (faulted) return;
  const int n = k->app_n, fn0 = k->app_fn0, act_cnt = k->app_act_cnt;
  k->n_nodes = k->app_N0 + n_acc;
  k->frontier_n = f.prio.n_heaps ? fn0 : fn0 + n_acc;
  k->n_borders = k->app_nb0 + n_ev;
  k->act_sel = k->app_act_sel ^ 1;
  k->act_cnt = (n - n_acc) + (act_cnt - n);
  round_begin_next(f, k);
}

// ---- node ids, plain SFF: the accepted samples before each 64-sample group, from the workgroup lines k_commit leaves.
// A line's KC_ACC word is (launch number << 32 | accepted samples of the workgroup); it counts when it carries the
// commit's launch number `seq`.  The lines above the round's size are thereby out: their workgroups leave before they
// publish, the words still carry an earlier launch's number.
SFF_HD unsigned commit_line_count(unsigned long long word, unsigned seq) {
  return (unsigned)(word >> 32) == seq ? (unsigned)word : 0u;
}
// The prefix has two levels, the ones a workgroup of the append launch computes it in (hand_lines, devforest.hip): the
// lines in chunks of 64 - one wavefront's lines, scanned across its lanes there - and the chunks' totals, part[k] (low half:
// accepted samples of chunk k; the device keeps the chunk's border events in the high half).  SFFK_DEV_MAX_GROUPS lines
// at most, so 16 chunks.
#define SFFK_LINE_CHUNKS (SFFK_DEV_MAX_GROUPS / 64)
// accepted samples of every chunk below group g's.  part[0..3] are always there (chunks without lines hold 0): a wave of
// up to 16 384 slots reads them in one go and selects, only larger waves walk on (a loop of dependent LDS reads on the
// device).
SFF_HD int commit_prefix_base(const unsigned long long* part, int g) {
  const int c = g >> 6;
  const int p0 = (int)(unsigned)part[0], p1 = (int)(unsigned)part[1], p2 = (int)(unsigned)part[2], p3 = (int)(unsigned)part[3];
  int base = (c > 0 ? p0 : 0) + (c > 1 ? p1 : 0) + (c > 2 ? p2 : 0) + (c > 3 ? p3 : 0);
  for (int k = 4; k < c; ++k) base += (int)(unsigned)part[k];
  return base;
}
// pref[g] = accepted samples of the groups below g (a sample's node id = N0 + pref[i >> 6] + its rank in its word);
// returns the round's accepted samples, -1 for more lines than a wave can have.  acc = the KC_ACC word of line 0,
// `stride` words from one line to the next.  tests/commit_prefix_harness.cpp holds it against a plain running sum.
SFF_HD int commit_line_prefix(const unsigned long long* acc, int stride, int n_lines, unsigned seq, int32_t* pref) {
  if (n_lines < 0 || n_lines > SFFK_DEV_MAX_GROUPS) return -1;
  unsigned long long part[SFFK_LINE_CHUNKS] = {};
  const int chunks = (n_lines + 63) >> 6;
  for (int k = 0; k < chunks; ++k) {
    unsigned run = 0;                                   // (the wavefront's scan: exclusive within the chunk)
    for (int g = k * 64; g < n_lines && g < k * 64 + 64; ++g) {
      pref[g] = (int32_t)run;
      run += commit_line_count(acc[(size_t)g * (size_t)stride], seq);
    }
    part[k] = run;
  }
  for (int g = 0; g < n_lines; ++g) pref[g] += commit_prefix_base(part, g);
  return commit_prefix_base(part, chunks * 64);
}

}  // namespace sffk
