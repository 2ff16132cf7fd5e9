// forest_batch.cpp — forest batches: many independent forests of waves of ONE slot advanced in lock step.
//
// Waves of one slot are the reference's own loop order (src/forest.h:122-202), and one forest of them keeps one wavefront
// busy (k_seq_waves_batch) - or, speculated, a couple of hundred workgroups for a factor of four (k_spec_waves).  Independent
// forests need neither speculation nor co-residency: k_seq_waves_batch gives every member a wavefront of its own, and the
// host does for every member what run_device_seq does for one.  The lock step itself is run_lockstep (batch_lockstep.h);
// here is what is a forest's own in it:
//   - a member is live until it has terminated or run its max_waves; one a host-engine wave was left unfinished in (in_wave)
//     is advanced on its own through run_device(1) first, as run_device_seq does, and joins the same step;
//   - eight kinds (SFF / SFF*; plain, priority frontier, single goal, or priority + goal: the template instances of the
//     kernel), at most 4 096 waves a launch;
//   - a member is taken in exactly like a single forest: dev_finish_wave (growth, re-celling) and, after a list fault,
//     that one wave on the host-replay engine (seq_lists_fault).
#include "batch_lockstep.h"

namespace sff {

namespace {
struct ForestFamily {
  using Args = sffk::SeqArgs;
  static constexpr int n_kinds = 8;   // the template instance that runs a member: Forest::seq_kind
  Forest* const* m;
  int n, max_waves;
  std::vector<uint64_t> w0, w_launch;
  std::vector<double> alone_ms;   // time the member's own run_device(1) calls have already booked

  int device() { return m[0]->ctx->device; }
  void begin(int i) {
    Forest& f = *m[i];
    if (!f.dev.active) f.dev_upload_state();
    f.ctx->sync();
    w0[i] = f.dev.last.waves;
  }
  int plan(int i) {
    Forest& f = *m[i];
    const sffk::DevCtrl& k = f.dev.last;
    while (k.in_wave) {   // (a wave the host-replay engine left unfinished: through the round engine, alone)
      const double before = f.st.total_ms;
      f.seq_suspended = true;
      f.run_device(1);
      f.seq_suspended = false;
      alone_ms[i] += f.st.total_ms - before;
      f.ctx->sync();
    }
    if (k.terminated) return 0;
    if (max_waves > 0 && (int)(k.waves - w0[i]) >= max_waves) return 0;
    return f.seq_launch_waves(max_waves > 0 ? max_waves - (int)(k.waves - w0[i]) : 0);
  }
  uint64_t words_needed(int i, int waves) {
    const uint64_t end = m[i]->seq_words_end(waves);
    return end > m[i]->dev.wr.produced ? end - m[i]->dev.wr.produced : 0;
  }
  Mt64& gen(int i) { return m[i]->rng; }
  void ring_append(int i, const uint64_t* w, size_t nw) { m[i]->dev_ring_append(w, nw); }
  WordRing& ring(int i) { return m[i]->dev.wr; }
  Args prepare(int i, int waves) {
    w_launch[i] = m[i]->dev.last.waves;
    return m[i]->seq_prepare(waves);
  }
  int kind(int i) { return m[i]->seq_kind(); }
  hipStream_t stream(int i) { return m[i]->ctx->stream; }
  StatusBlock status(int i) { return {m[i]->dev.h_ctrl.p, m[i]->dev.ctrl.p, sizeof(sffk::DevCtrl)}; }
  hipError_t launch(hipStream_t s, const Args* a, int count, int kind, size_t lds) {
    return sffk::launch_seq_waves_batch(s, a, count, (kind & 1) != 0, (kind & 2) != 0, (kind & 4) != 0, lds);
  }
  void take_in(int i, double* wait_ms) {
    Forest& f = *m[i];
    f.dev.status_copied[0] = true;
    f.dev.host_stale = true;
    ++f.st.batch_launches;
    const int fault = f.dev_finish_wave(wait_ms, 0, true);
    f.seq_note_launch(w_launch[i]);
    if (fault == SFFK_FAULT_LISTS) f.seq_lists_fault();
    f.ctx->sync();   // (growth, re-celling and the upload run on the member's own stream: done before the next launch)
  }
  void finish(double wall, double wait_ms) {
    for (int i = 0; i < n; ++i) {
      m[i]->seq_suspended = false;
      m[i]->st.total_ms += std::max(0.0, wall - alone_ms[i]);
      m[i]->st.host_ms += std::max(0.0, wall - alone_ms[i] - wait_ms);
    }
  }
};
}  // namespace

void run_forest_batch(Forest* const* members, int n, int max_waves, int* failed) {
  ForestFamily fam{members, n, max_waves, std::vector<uint64_t>((size_t)n), std::vector<uint64_t>((size_t)n, 0), std::vector<double>((size_t)n, 0.0)};
  run_lockstep(fam, n, failed);
}

}  // namespace sff
