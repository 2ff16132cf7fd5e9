// batch_lockstep.h — the lock step of forest batches (forest_batch.cpp) and session batches (rrt_batch.cpp), once.
//
// n independent members, each on a context of its own, every one a wavefront of its own in ONE launch per kind (a kind = a
// template instance of the batch kernel).  A step:
//   1. who takes part, and for how much: Family::plan (whatever a member has to do alone first happens in there);
//   2. the engine words the launch may need are generated from every member's own generator (pure host work, on up to 16
//      threads - at 256 members the host's largest share), every ring is topped up on its member's copy stream, every
//      member's argument struct is built;
//   3. per kind, on the stream of the kind's first member: the arguments go up as one array, the stream waits for the
//      members' ring copies, one launch runs all of them, their status blocks are copied back on that same stream (a step
//      costs one submission per kind, not one per member); then one wait per kind;
//   4. every member of a launched kind is taken in, whatever happens to another one.
// Members drop out as plan() returns 0; the call ends when none is left.  A launch lasts as long as its slowest member.
// The first exception wins: *failed names its member, the step is finished for the others as far as the order above allows,
// Family::finish books the call and the exception goes on to the caller.
//
// Family (a plain struct, see the two adapters):
//   using Args; static constexpr int n_kinds;
//   int device();  void begin(int i);  int plan(int i);                    // plan: the member's amount for this step, 0 = not live
//   uint64_t words_needed(int i, int amount);  Mt64& gen(int i);           // words to draw beyond the ring's `produced`
//   void ring_append(int i, const uint64_t* w, size_t n);  WordRing& ring(int i);
//   Args prepare(int i, int amount);  int kind(int i);  hipStream_t stream(int i);
//   StatusBlock status(int i);
//   hipError_t launch(hipStream_t s, const Args* dev_args, int n, int kind, size_t lds_bytes);
//   void take_in(int i, double* wait_ms);  void finish(double wall_ms, double wait_ms);
#pragma once
#include <atomic>
#include <chrono>
#include <exception>
#include <thread>
#include <vector>

#include "engine.h"

namespace sff {

struct StatusBlock {   // a member's status block: where the kernel leaves it, where the host reads it
  void* host;
  const void* dev;
  size_t bytes;
};

template <class Family>
void run_lockstep(Family& fam, int n, int* failed) {
  using Args = typename Family::Args;
  using Clock = std::chrono::steady_clock;
  constexpr int K = Family::n_kinds;
  auto ms_since = [](Clock::time_point t) { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); };
  struct ArgBufs {   // the members' arguments: pinned staging + device array, kind by kind
    PinBuf h;
    DevBuf d;
    ~ArgBufs() { h.release(); d.release(); }
  } args;
  const auto t0 = Clock::now();
  double wait_ms = 0;
  std::vector<int> amount((size_t)n, 0), live, order;
  std::vector<std::vector<uint64_t>> words((size_t)n);
  std::exception_ptr err;
  int cur = 0;   // the member being worked for - only ever a member's index, so whatever is thrown has a member to name
  auto fail = [&]() { if (!err) { err = std::current_exception(); *failed = cur; } };
  *failed = -1;
  try {
    hip_check(hipSetDevice(fam.device()), "hipSetDevice");
    args.h.ensure((size_t)n * sizeof(Args));
    args.d.ensure((size_t)n * sizeof(Args));
    for (int i = 0; i < n; ++i) { cur = i; fam.begin(i); }
    while (true) {
      // ---- 1. who takes part, and for how much
      live.clear();
      for (int i = 0; i < n; ++i) {
        cur = i;
        if ((amount[i] = fam.plan(i)) > 0) live.push_back(i);
      }
      if (live.empty()) break;
      // ---- the engine words the launch may need, from every member's own generator
      uint64_t short_total = 0;
      for (int i : live) {
        cur = i;
        words[i].resize((size_t)fam.words_needed(i, amount[i]));
        short_total += words[i].size();
      }
      {
        std::atomic<size_t> next{0};
        auto work = [&]() {
          for (size_t j = next++; j < live.size(); j = next++) {
            std::vector<uint64_t>& w = words[live[j]];
            if (!w.empty()) fam.gen(live[j]).fill(w.data(), w.size());
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
      int n_kind[K] = {};
      size_t first_of[K] = {}, lds[K] = {};
      for (int kind = 0; kind < K; ++kind) {
        first_of[kind] = order.size();
        for (int i : live) if (fam.kind(i) == kind) { order.push_back(i); ++n_kind[kind]; }
      }
      for (int i : order) {   // (every member's drawn words reach its ring, whatever happens to another one: a generator
        cur = i;              // ahead of its ring would be an inconsistent member)
        try {
          if (!words[i].empty()) fam.ring_append(i, words[i].data(), words[i].size());
        } catch (...) { fail(); }
      }
      if (err) break;
      Args* ha = args.h.template as<Args>();
      Args* da = args.d.template as<Args>();
      for (size_t s = 0; s < order.size(); ++s) {
        cur = order[s];
        ha[s] = fam.prepare(cur, amount[cur]);
        const int kind = fam.kind(cur);
        lds[kind] = std::max(lds[kind], sffk::collide_lds_bytes(ha[s].rob.n_tri, 1));
      }
      // ---- 2. + 3. per kind: arguments up, one launch, the status blocks back - on the stream of the kind's first member
      bool launched[K] = {};
      try {
        for (int kind = 0; kind < K; ++kind) {
          if (!n_kind[kind]) continue;
          const size_t first = first_of[kind], end = first + (size_t)n_kind[kind];
          cur = order[first];
          hipStream_t s = fam.stream(cur);
          for (size_t j = first; j < end; ++j) fam.ring(order[j]).wait_on(s);
          hip_check(hipMemcpyAsync(da + first, ha + first, (size_t)n_kind[kind] * sizeof(Args), hipMemcpyHostToDevice, s), "batch arguments");
          hip_check(fam.launch(s, da + first, n_kind[kind], kind, lds[kind]), "batch launch");
          launched[kind] = true;
          for (size_t j = first; j < end; ++j) {
            const StatusBlock b = fam.status(order[j]);
            hip_check(hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, s), "batch status block");
          }
        }
      } catch (...) { fail(); }
      const auto tw = Clock::now();
      for (int kind = 0; kind < K; ++kind) {
        if (!launched[kind]) continue;
        cur = order[first_of[kind]];
        try { hip_check(hipStreamSynchronize(fam.stream(cur)), "batch wait"); } catch (...) { fail(); launched[kind] = false; }
      }
      wait_ms += ms_since(tw);
      // ---- 4. every member that ran is taken in, whatever happens to another one
      for (int i : order) {
        if (!launched[fam.kind(i)]) continue;
        cur = i;
        try { fam.take_in(i, &wait_ms); } catch (...) { fail(); }
      }
      if (err) break;
    }
  } catch (...) { fail(); }
  fam.finish(ms_since(t0), wait_ms);
  if (err) std::rethrow_exception(err);
}

}  // namespace sff
