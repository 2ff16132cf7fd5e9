// forest_batch.cpp — forest batches: many independent forests of waves of ONE slot advanced in lock step.
//
// Waves of one slot are the reference's own loop order (src/forest.h:122-202), and one forest of them keeps one wavefront
// busy (k_seq_waves) - or, speculated, a couple of hundred workgroups for a factor of four (k_spec_waves).  Independent
// forests need neither speculation nor co-residency: k_seq_waves_batch gives every member a wavefront of its own, and the
// host does for every member what run_device_seq does for one.  A step of the lock step:
//   1. every member that has neither terminated nor run its max_waves is prepared: its engine words are generated (on up
//      to 16 threads - at 256 members this is the host's largest share), its ring is topped up on its own copy stream, its
//      SeqArgs are built;
//   2. per kind (SFF / SFF*, plain / priority frontier: four template instances, so up to four launches) the members'
//      SeqArgs go up as one array, the kind's stream waits for the members' ring copies, ONE launch runs all of them, their
//      status blocks are copied back on that same stream (the first member's of the kind: a step costs one submission per
//      kind, not one per member);
//   3. one wait per kind;
//   4. every member is taken in exactly like a single forest: dev_finish_wave (growth, re-celling) and, after a list
//      fault, that one wave on the host-replay engine (seq_lists_fault).
// A member a host-engine wave was left unfinished in (in_wave) is advanced on its own through run_device(1) first, as
// run_device_seq does, and joins the same step.  Members drop out as they terminate; the call ends when none is left.
// A launch lasts as long as its slowest member (at most 4 096 waves each): members that end early idle until the step ends.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <exception>
#include <thread>
#include <vector>

#include "engine.h"

namespace sff {

#define HIPCHK(x) hip_check((x), #x)
using Clock = std::chrono::steady_clock;
static double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

namespace {
struct ArgBufs {   // the members' SeqArgs: pinned staging + device array, kind by kind
  PinBuf h;
  DevBuf d;
  ~ArgBufs() { h.release(); d.release(); }
};
}  // namespace

void run_forest_batch(Forest* const* members, int n, int max_waves, int* failed) {
  *failed = -1;
  HIPCHK(hipSetDevice(members[0]->ctx->device));
  const auto t0 = Clock::now();
  double wait_ms = 0;
  std::vector<uint64_t> w0((size_t)n), w_launch((size_t)n, 0);
  // kind of a member = the template instance that runs it: bit 0 SFF*, bit 1 priority frontier
  auto kind_of = [&](int i) { return (members[i]->cfg.optimize ? 1 : 0) | (members[i]->use_priority() ? 2 : 0); };
  std::vector<double> alone_ms((size_t)n, 0.0);   // time the member's own run_device(1) calls have already booked
  std::vector<int> waves_now((size_t)n, 0);
  std::vector<std::vector<uint64_t>> words((size_t)n);
  std::vector<int> live, order;
  ArgBufs args;
  args.h.ensure((size_t)n * sizeof(sffk::SeqArgs));
  args.d.ensure((size_t)n * sizeof(sffk::SeqArgs));
  std::exception_ptr err;
  auto fail = [&](int i) { if (!err) { err = std::current_exception(); *failed = i; } };
  auto book = [&]() {
    const double wall = ms_since(t0);
    for (int i = 0; i < n; ++i) {
      members[i]->seq_suspended = false;
      members[i]->st.total_ms += std::max(0.0, wall - alone_ms[i]);
      members[i]->st.host_ms += std::max(0.0, wall - alone_ms[i] - wait_ms);
    }
  };
  int cur = 0;
  try {
    for (cur = 0; cur < n; ++cur) {
      Forest& f = *members[cur];
      if (!f.dev.active) f.dev_upload_state();
      f.ctx->sync();
      w0[cur] = f.dev.last.waves;
    }
    while (true) {
      // ---- 1. who takes part, and for how many waves
      live.clear();
      for (cur = 0; cur < n; ++cur) {
        Forest& f = *members[cur];
        const sffk::DevCtrl& k = f.dev.last;
        while (k.in_wave) {   // (a wave the host-replay engine left unfinished: through the round engine, alone)
          const double before = f.st.total_ms;
          f.seq_suspended = true;
          f.run_device(1);
          f.seq_suspended = false;
          alone_ms[cur] += f.st.total_ms - before;
          f.ctx->sync();
        }
        if (k.terminated) continue;
        if (max_waves > 0 && (int)(k.waves - w0[cur]) >= max_waves) continue;
        waves_now[cur] = f.seq_launch_waves(max_waves > 0 ? max_waves - (int)(k.waves - w0[cur]) : 0);
        live.push_back(cur);
      }
      if (live.empty()) break;
      // ---- the engine words the launch may need, from every member's own generator: pure host work, on up to 16 threads
      uint64_t short_total = 0;
      for (int i : live) {
        Forest& f = *members[i];
        const uint64_t end = f.seq_words_end(waves_now[i]);
        words[i].resize(end > f.dev.produced ? (size_t)(end - f.dev.produced) : 0);
        short_total += words[i].size();
      }
      {
        std::atomic<size_t> next{0};
        auto work = [&]() {
          for (size_t j = next++; j < live.size(); j = next++) {
            Forest& f = *members[live[j]];
            if (!words[live[j]].empty()) f.rng.fill(words[live[j]].data(), words[live[j]].size());
          }
        };
        const unsigned nt = short_total < (1u << 16) ? 1u
                            : std::max(1u, std::min({16u, std::thread::hardware_concurrency(), (unsigned)live.size()}));
        std::vector<std::thread> th;
        for (unsigned t = 1; t < nt; ++t) th.emplace_back(work);
        work();
        for (auto& x : th) x.join();
      }
      // ---- rings and arguments; the members kind by kind
      order.clear();
      int n_kind[4] = {0, 0, 0, 0};
      size_t first_of[4] = {0, 0, 0, 0};
      for (int kind = 0; kind < 4; ++kind) {
        first_of[kind] = order.size();
        for (int i : live) if (kind_of(i) == kind) { order.push_back(i); ++n_kind[kind]; }
      }
      sffk::SeqArgs* ha = args.h.as<sffk::SeqArgs>();
      size_t lds[4] = {0, 0, 0, 0};
      for (size_t s = 0; s < order.size(); ++s) {   // (every member's drawn words reach its ring, whatever happens to another one:
        cur = order[s];                             // a generator ahead of its ring would be an inconsistent forest)
        try {
          if (!words[cur].empty()) members[cur]->dev_ring_append(words[cur].data(), words[cur].size());
        } catch (...) { fail(cur); }
      }
      if (err) break;
      for (size_t s = 0; s < order.size(); ++s) {
        cur = order[s];
        Forest& f = *members[cur];
        w_launch[cur] = f.dev.last.waves;
        ha[s] = f.seq_prepare(waves_now[cur]);
        const int kind = kind_of(cur);
        lds[kind] = std::max(lds[kind], sffk::collide_lds_bytes(ha[s].rob.n_tri, 1));
      }
      // ---- 2. + 3. per kind: arguments up, one launch, the status blocks back - on the stream of the kind's first member
      bool launched[4] = {false, false, false, false};
      try {
        for (int kind = 0; kind < 4; ++kind) {
          if (!n_kind[kind]) continue;
          const size_t first = first_of[kind];
          cur = order[first];
          hipStream_t s = members[cur]->ctx->stream;
          for (size_t j = first; j < first + (size_t)n_kind[kind]; ++j) {
            DevEngine& d = members[order[j]]->dev;
            if (d.ring_pending) {
              HIPCHK(hipStreamWaitEvent(s, d.ev_ring, 0));
              d.ring_pending = false;
            }
          }
          HIPCHK(hipMemcpyAsync(args.d.as<sffk::SeqArgs>() + first, ha + first, (size_t)n_kind[kind] * sizeof(sffk::SeqArgs),
                                hipMemcpyHostToDevice, s));
          HIPCHK(sffk::launch_seq_waves_batch(s, args.d.as<sffk::SeqArgs>() + first, n_kind[kind], (kind & 1) != 0, (kind & 2) != 0, lds[kind]));
          launched[kind] = true;
          for (size_t j = first; j < first + (size_t)n_kind[kind]; ++j) {
            DevEngine& d = members[order[j]]->dev;
            HIPCHK(hipMemcpyAsync(d.h_ctrl.as<sffk::DevCtrl>(), d.ctrl.p, sizeof(sffk::DevCtrl), hipMemcpyDeviceToHost, s));
          }
        }
      } catch (...) { fail(cur); }
      const auto tw = Clock::now();
      for (int kind = 0; kind < 4; ++kind) {
        if (!launched[kind]) continue;
        cur = order[first_of[kind]];
        try { HIPCHK(hipStreamSynchronize(members[cur]->ctx->stream)); } catch (...) { fail(cur); launched[kind] = false; }
      }
      wait_ms += ms_since(tw);
      // ---- 4. every member that ran is taken in, whatever happens to another one
      for (size_t s = 0; s < order.size(); ++s) {
        cur = order[s];
        Forest& f = *members[cur];
        if (!launched[kind_of(cur)]) continue;
        try {
          f.dev.status_copied[0] = true;
          f.dev.host_stale = true;
          ++f.st.batch_launches;
          const int fault = f.dev_finish_wave(&wait_ms, 0, true);
          f.seq_note_launch(w_launch[cur]);
          if (fault == SFFK_FAULT_LISTS) f.seq_lists_fault();
          f.ctx->sync();   // (growth, re-celling and the upload run on the member's own stream: done before the next launch)
        } catch (...) { fail(cur); }
      }
      if (err) break;
    }
  } catch (...) { fail(cur); }
  book();
  if (err) std::rethrow_exception(err);
}

}  // namespace sff
