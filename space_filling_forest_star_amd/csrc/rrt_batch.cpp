// rrt_batch.cpp — session batches: many independent RRT / RRT* / Multi-T-RRT sessions advanced in lock step.
//
// One session one iteration at a time (src/rrt.h:93-99) keeps one wavefront busy and nothing else; independent sessions
// need neither speculation nor co-residency: k_rrt_seq_batch gives every member a wavefront of its own that runs the
// reference's loop - nearest node, steer, pose and parent edge, the other live trees, RRT* choose-parent / rewire, append -
// with every edge checked only when the loop reaches it.  A step of the lock step:
//   1. every member that still has iterations to run is prepared: an iteration the kernel handed over (link + merge, an
//      exact tie in a merged tree's list, a capacity) runs alone through Rrt::expand and the device block is uploaded again;
//      its engine words are generated from the block's own copy of the generator (on up to 16 threads), its ring is topped
//      up on its own copy stream, its RrtSeqArgs are built;
//   2. per kind (RRT, RRT*: two template instances, so two launches) the members' arguments go up as one array, the kind's
//      stream waits for the members' ring copies, ONE launch runs all of them, their status blocks are copied back on that
//      same stream;
//   3. one wait per kind;
//   4. every member is taken in: node count of the store, the grid re-celled when its overflow list asks for it.
// The host mirror (nodes, tree lists, counters, the Mt64) is refreshed lazily (batch_sync_host): by the getters, by
// sffgpu_rrt_run and by the host iteration.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <exception>
#include <thread>
#include <vector>

#include "engine.h"

namespace sff {

#define HIPCHK(x) hip_check((x), #x)
using Clock = std::chrono::steady_clock;
static double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

Rrt::~Rrt() {
  BatchDev& d = bd;
  DevBuf* bufs[] = {&d.ctrl, &d.parent, &d.root_tree, &d.d_root, &d.d_closest, &d.iter, &d.live, &d.tree_cnt, &d.ring, &d.ktab};
  for (DevBuf* b : bufs) b->release();
  d.h_ctrl.release();
  d.h_ring.release();
  if (d.ev_ring) (void)hipEventDestroy(d.ev_ring);
}

bool Rrt::batch_done(int iter0, int max_iters) const {
  const int it = batch_iter();
  if (solved || it >= cfg.max_iterations) return true;                           // :93
  return max_iters > 0 && it - iter0 >= max_iters;
}

void Rrt::batch_upload() {
  Ctx& c = *ctx;
  BatchDev& d = bd;
  HIPCHK(hipSetDevice(c.device));
  if (!c.grid_on) throw HipError{"rrt batch: the session has no grid over its store (SFFGPU_RRT_NO_GRID)"};
  c.sync();
  if (c.store_n != (int)nodes.size()) throw HipError{"rrt batch: the context's node store is not this session's (another session was created on the context)"};
  c.grid_insert_new();
  c.grid_check();
  if (!d.inited) {
    HIPCHK(hipEventCreateWithFlags(&d.ev_ring, hipEventDisableTiming));
    d.ring_words = 1u << 17;   // (>= batch_launch_iters x 9 words + slack)
    d.ring.ensure((size_t)d.ring_words * 8);
    d.h_ring.ensure((size_t)d.ring_words * 8);
    d.ctrl.ensure(sizeof(sffk::RrtCtrl));
    d.h_ctrl.ensure(sizeof(sffk::RrtCtrl));
    // k = (size_t)(2e log10(#nodes)) (src/rrt.h:160): the node counts at which it steps, found with the C library's log10 in
    // the reference's own expression (the kernel only compares integers)
    std::vector<int32_t> ktab(64, 0x7fffffff);
    auto k_of = [](long long nn) { return (long long)(size_t)(2 * M_E * std::log10((double)nn)); };
    ktab[0] = 0;
    for (int m = 1; m < 64; ++m) {
      long long lo = 1, hi = 0x7fffffffLL;
      if (k_of(hi) < m) continue;
      while (lo < hi) {
        const long long mid = (lo + hi) / 2;
        if (k_of(mid) >= m) hi = mid; else lo = mid + 1;
      }
      ktab[m] = (int32_t)lo;
    }
    d.ktab.ensure(64 * 4);
    HIPCHK(hipMemcpy(d.ktab.p, ktab.data(), 64 * 4, hipMemcpyHostToDevice));
    d.live.ensure(trees.size() * 4);
    d.tree_cnt.ensure(trees.size() * 4);
    d.inited = true;
  }
  d.node_cap = c.store_cap;
  const size_t cap = (size_t)d.node_cap, n = nodes.size();
  d.parent.ensure(cap * 4);
  d.root_tree.ensure(cap * 4);
  d.iter.ensure(cap * 4);
  d.d_root.ensure(cap * 8);
  d.d_closest.ensure(cap * 8);
  std::vector<int32_t> par(n), root(n), tcnt(trees.size()), live(tree_frontier.begin(), tree_frontier.end());
  std::vector<uint32_t> its(n);
  std::vector<double> dr(n), dc(n);
  for (size_t i = 0; i < n; ++i) {
    par[i] = nodes[i].parent; root[i] = nodes[i].root_tree; its[i] = nodes[i].iter;
    dr[i] = nodes[i].d_root; dc[i] = nodes[i].d_closest;
  }
  for (size_t t = 0; t < trees.size(); ++t) tcnt[t] = (int32_t)trees[t].size();
  HIPCHK(hipMemcpy(d.parent.p, par.data(), n * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d.root_tree.p, root.data(), n * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d.iter.p, its.data(), n * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d.d_root.p, dr.data(), n * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d.d_closest.p, dc.data(), n * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d.tree_cnt.p, tcnt.data(), tcnt.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d.live.p, live.data(), live.size() * 4, hipMemcpyHostToDevice));
  sffk::RrtCtrl k{};
  k.n_nodes = (int32_t)n;
  k.iter = iter;
  k.cursor = rng.draws;
  k.collide_calls = st.collide_calls;
  k.path_free_calls = st.path_free_calls;
  k.nn_queries = st.nn_queries;
  HIPCHK(hipMemcpy(d.ctrl.p, &k, sizeof k, hipMemcpyHostToDevice));
  d.last = k;
  // the ring starts over at the generator's position: a copy of it runs ahead, the session's own moves when the mirror does
  d.gen = rng;
  d.produced = rng.draws;
  d.ring_pending = false;
  d.host_nodes = (int)n;
  d.valid = true;
  d.host_stale = false;
}

void Rrt::batch_sync_host() {
  BatchDev& d = bd;
  if (!d.valid || !d.host_stale) return;
  Ctx& c = *ctx;
  HIPCHK(hipSetDevice(c.device));
  const int n = d.last.n_nodes, n0 = d.host_nodes;
  // RRT*: a rewire changes parent, Root and the two distances of an older node (src/rrt.h:193-198) - all rows come back
  const int first = cfg.optimize ? 0 : n0;
  const size_t m = (size_t)(n - first), fresh = (size_t)(n - n0);
  std::vector<int32_t> par(m), root(m), tr(fresh);
  std::vector<uint32_t> its(fresh);
  std::vector<double> dr(m), dc(m), pos(fresh * 6);
  if (m) {
    HIPCHK(hipMemcpy(par.data(), d.parent.as<int32_t>() + first, m * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(root.data(), d.root_tree.as<int32_t>() + first, m * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(dr.data(), d.d_root.as<double>() + first, m * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(dc.data(), d.d_closest.as<double>() + first, m * 8, hipMemcpyDeviceToHost));
  }
  if (fresh) {
    HIPCHK(hipMemcpy(its.data(), d.iter.as<uint32_t>() + n0, fresh * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(tr.data(), c.stree.as<int32_t>() + n0, fresh * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(pos.data(), c.spos.as<double>() + 6 * (size_t)n0, fresh * 48, hipMemcpyDeviceToHost));
  }
  for (int i = first; i < n0; ++i) {
    RNode& nd = nodes[i];
    nd.parent = par[i - first]; nd.root_tree = root[i - first]; nd.d_root = dr[i - first]; nd.d_closest = dc[i - first];
  }
  nodes.reserve((size_t)n);
  for (int i = n0; i < n; ++i) {   // (the kernel merges nothing: a new node joins the list of the tree it was grown from, in id order)
    RNode nd;
    memcpy(nd.pos, &pos[6 * (size_t)(i - n0)], sizeof nd.pos);
    nd.tree = tr[i - n0];
    nd.parent = par[i - first]; nd.root_tree = root[i - first]; nd.d_root = dr[i - first]; nd.d_closest = dc[i - first];
    nd.iter = its[i - n0];
    nd.idx_in_tree = (int)trees[nd.tree].size();
    trees[nd.tree].push_back(i);
    nodes.push_back(nd);
    for (int a = 0; a < 3; ++a) c.store_maxabs = std::max(c.store_maxabs, std::fabs(nd.pos[a]));   // (as Ctx::store_append keeps it)
  }
  iter = d.last.iter;
  st.collide_calls = d.last.collide_calls;
  st.path_free_calls = d.last.path_free_calls;
  st.nn_queries = d.last.nn_queries;
  if (rng.draws > d.last.cursor) throw HipError{"rrt batch: the generator is past the kernel's cursor (internal error)"};
  while (rng.draws < d.last.cursor) (void)rng.next();
  d.host_nodes = n;
  d.host_stale = false;
}

void Rrt::batch_ring_append(const uint64_t* words, size_t n) {   // words for absolute positions [produced, produced + n)
  BatchDev& d = bd;
  Ctx& c = *ctx;
  uint64_t* hr = d.h_ring.as<uint64_t>();
  size_t done = 0;
  while (done < n) {
    const uint64_t at = (d.produced + done) & (d.ring_words - 1);
    const size_t run = std::min<size_t>(n - done, (size_t)(d.ring_words - at));
    memcpy(hr + at, words + done, run * 8);
    HIPCHK(hipMemcpyAsync(d.ring.as<uint64_t>() + at, hr + at, run * 8, hipMemcpyHostToDevice, c.copy_stream));
    done += run;
  }
  d.produced += n;
  HIPCHK(hipEventRecord(d.ev_ring, c.copy_stream));
  d.ring_pending = true;
}

sffk::RrtSeqArgs Rrt::batch_prepare(int iters) {
  Ctx& c = *ctx;
  BatchDev& d = bd;
  sffk::RrtSeqArgs a{};
  a.ctrl = d.ctrl.as<sffk::RrtCtrl>();
  a.st = sffk::NodeStoreMut{c.sx.as<float>(), c.sy.as<float>(), c.sz.as<float>(), c.syaw.as<float>(),
                            c.spitch.as<float>(), c.sroll.as<float>(), c.stree.as<int32_t>(), c.spos.as<double>()};
  a.g = c.gridv;
  a.env = c.envv;
  a.rob = c.robv;
  a.parent = d.parent.as<int32_t>();
  a.root_tree = d.root_tree.as<int32_t>();
  a.d_root = d.d_root.as<double>();
  a.d_closest = d.d_closest.as<double>();
  a.iter = d.iter.as<uint32_t>();
  a.live = d.live.as<int32_t>();
  a.tree_cnt = d.tree_cnt.as<int32_t>();
  a.ring = d.ring.as<uint64_t>();
  a.ring_mask = d.ring_words - 1;
  a.words_end = d.produced;
  a.ktab = d.ktab.as<int32_t>();
  memcpy(a.limits, cfg.limits, sizeof a.limits);
  memcpy(a.goal, cfg.goal, sizeof a.goal);
  a.priority_bias = cfg.priority_bias;
  a.dist_tree = cfg.dist_tree;
  a.sampling_dist = cfg.sampling_dist;
  // (the store's largest coordinate is only known up to the host mirror: the nodes the kernel adds lie within one step of the limits)
  double reach = std::max(c.store_maxabs, c.env_maxabs);
  for (int k = 0; k < 6; ++k) reach = std::max(reach, std::fabs(cfg.limits[k]) + cfg.sampling_dist);
  a.sweep_abs_eps = reach * std::ldexp(1.0, -20);
  a.cell_edge = c.grid_cell;
  a.knn_slack = 8 * a.sweep_abs_eps;
  a.dim = cfg.dim;
  a.max_iters = iters;
  a.iter_limit = cfg.max_iterations;
  a.node_cap = std::min(d.node_cap, c.store_cap);
  a.pick_range = num_trees + 1;
  a.n_live = (int)tree_frontier.size();
  a.merged = st.merges > 0 ? 1 : 0;
  a.grid_ovf_limit = c.grid_rebuild_at();
  return a;
}

void Rrt::batch_take_in() {
  Ctx& c = *ctx;
  BatchDev& d = bd;
  const sffk::RrtCtrl before = d.last;
  d.last = *d.h_ctrl.as<sffk::RrtCtrl>();
  d.host_stale = true;
  ++st.batch_launches;
  c.store_n = d.last.n_nodes;        // (the kernel wrote store and grid itself)
  c.grid_inserted = d.last.n_nodes;
  if (d.last.status == SFFK_RRT_GRID || d.last.grid_ovf > c.grid_rebuild_at()) {
    if (d.last.grid_ovf > c.gridv.ovf_cap) throw HipError{"rrt batch: neighbour grid overflow list exhausted during a launch (nodes were dropped)"};
    HIPCHK(hipSetDevice(c.device));
    c.grid_check(/*bulk=*/true);
    if (d.last.status == SFFK_RRT_GRID && d.last.iter == before.iter && d.last.grid_ovf <= before.grid_ovf && before.status == SFFK_RRT_GRID)
      throw HipError{"rrt batch: the neighbour grid cannot take the session's nodes (internal error)"};
  }
}

void Rrt::batch_host_iteration() {
  batch_sync_host();
  bd.valid = false;
  ++iter;
  const int tree = tree_frontier[rng.uniform_int(0, num_trees)];                 // :95
  expand(tree, (unsigned)iter);
  ++st.batch_host_iterations;
}

namespace {
struct RrtArgBufs {   // the members' RrtSeqArgs: pinned staging + device array, RRT members first
  PinBuf h;
  DevBuf d;
  ~RrtArgBufs() { h.release(); d.release(); }
};
}  // namespace

void run_rrt_batch(Rrt* const* members, int n, int max_iterations, int* failed) {
  *failed = -1;
  HIPCHK(hipSetDevice(members[0]->ctx->device));
  const auto t0 = Clock::now();
  std::vector<int> iter0((size_t)n), iters_now((size_t)n, 0);
  std::vector<std::vector<uint64_t>> words((size_t)n);
  std::vector<int> live, order;
  RrtArgBufs args;
  args.h.ensure((size_t)n * sizeof(sffk::RrtSeqArgs));
  args.d.ensure((size_t)n * sizeof(sffk::RrtSeqArgs));
  std::exception_ptr err;
  auto fail = [&](int i) { if (!err) { err = std::current_exception(); *failed = i; } };
  int cur = 0;
  try {
    for (cur = 0; cur < n; ++cur) iter0[cur] = members[cur]->batch_iter();
    while (true) {
      // ---- 1. who takes part, and for how many iterations
      live.clear();
      for (cur = 0; cur < n; ++cur) {
        Rrt& r = *members[cur];
        // (an iteration the kernel handed over: alone, through the host path - then the block goes up again)
        while (!r.batch_done(iter0[cur], max_iterations) && r.bd.valid && r.bd.last.status == SFFK_RRT_HOST_ITER) r.batch_host_iteration();
        if (r.batch_done(iter0[cur], max_iterations)) continue;
        if (!r.bd.valid) r.batch_upload();
        int left = r.cfg.max_iterations - r.bd.last.iter;
        if (max_iterations > 0) left = std::min(left, max_iterations - (r.bd.last.iter - iter0[cur]));
        iters_now[cur] = std::min(left, Rrt::batch_launch_iters);
        live.push_back(cur);
      }
      if (live.empty()) break;
      // ---- the engine words the launch may need, from every member's own generator: pure host work, on up to 16 threads
      uint64_t short_total = 0;
      for (int i : live) {
        Rrt& r = *members[i];
        const uint64_t end = r.bd.last.cursor + (uint64_t)iters_now[i] * 9 + 16;
        if (end - r.bd.last.cursor > r.bd.ring_words) throw HipError{"rrt batch: engine-word ring too small (internal error)"};
        words[i].resize(end > r.bd.produced ? (size_t)(end - r.bd.produced) : 0);
        short_total += words[i].size();
      }
      {
        std::atomic<size_t> next{0};
        auto work = [&]() {
          for (size_t j = next++; j < live.size(); j = next++) {
            Rrt& r = *members[live[j]];
            if (!words[live[j]].empty()) r.bd.gen.fill(words[live[j]].data(), words[live[j]].size());
          }
        };
        const unsigned nt = short_total < (1u << 16) ? 1u
                            : std::max(1u, std::min({16u, std::thread::hardware_concurrency(), (unsigned)live.size()}));
        std::vector<std::thread> th;
        for (unsigned t = 1; t < nt; ++t) th.emplace_back(work);
        work();
        for (auto& x : th) x.join();
      }
      // ---- rings and arguments; RRT members in front of RRT* members
      order.clear();
      for (int kind = 0; kind < 2; ++kind)
        for (int i : live) if ((members[i]->cfg.optimize ? 1 : 0) == kind) order.push_back(i);
      const int n_kind[2] = {(int)std::count_if(order.begin(), order.end(), [&](int i) { return !members[i]->cfg.optimize; }),
                             (int)std::count_if(order.begin(), order.end(), [&](int i) { return members[i]->cfg.optimize != 0; })};
      sffk::RrtSeqArgs* ha = args.h.as<sffk::RrtSeqArgs>();
      size_t lds[2] = {0, 0};
      for (size_t s = 0; s < order.size(); ++s) {   // (every member's drawn words reach its ring, whatever happens to another one:
        cur = order[s];                             // a generator ahead of its ring would be an inconsistent session)
        try {
          if (!words[cur].empty()) members[cur]->batch_ring_append(words[cur].data(), words[cur].size());
        } catch (...) { fail(cur); }
      }
      if (err) break;
      for (size_t s = 0; s < order.size(); ++s) {
        cur = order[s];
        Rrt& r = *members[cur];
        ha[s] = r.batch_prepare(iters_now[cur]);
        const int kind = r.cfg.optimize ? 1 : 0;
        lds[kind] = std::max(lds[kind], sffk::collide_lds_bytes(ha[s].rob.n_tri, 1));
      }
      // ---- 2. + 3. per kind: arguments up, one launch, the status blocks back - on the stream of the kind's first member
      bool launched[2] = {false, false};
      try {
        for (int kind = 0; kind < 2; ++kind) {
          if (!n_kind[kind]) continue;
          const size_t first = kind ? (size_t)n_kind[0] : 0;
          cur = order[first];
          hipStream_t s = members[cur]->ctx->stream;
          for (size_t j = first; j < first + (size_t)n_kind[kind]; ++j) {
            Rrt::BatchDev& d = members[order[j]]->bd;
            if (d.ring_pending) {
              HIPCHK(hipStreamWaitEvent(s, d.ev_ring, 0));
              d.ring_pending = false;
            }
          }
          HIPCHK(hipMemcpyAsync(args.d.as<sffk::RrtSeqArgs>() + first, ha + first, (size_t)n_kind[kind] * sizeof(sffk::RrtSeqArgs),
                                hipMemcpyHostToDevice, s));
          HIPCHK(sffk::launch_rrt_seq_batch(s, args.d.as<sffk::RrtSeqArgs>() + first, n_kind[kind], kind != 0, lds[kind]));
          launched[kind] = true;
          for (size_t j = first; j < first + (size_t)n_kind[kind]; ++j) {
            Rrt::BatchDev& d = members[order[j]]->bd;
            HIPCHK(hipMemcpyAsync(d.h_ctrl.as<sffk::RrtCtrl>(), d.ctrl.p, sizeof(sffk::RrtCtrl), hipMemcpyDeviceToHost, s));
          }
        }
      } catch (...) { fail(cur); }
      for (int kind = 0; kind < 2; ++kind) {
        if (!launched[kind]) continue;
        cur = order[kind ? (size_t)n_kind[0] : 0];
        try { HIPCHK(hipStreamSynchronize(members[cur]->ctx->stream)); } catch (...) { fail(cur); launched[kind] = false; }
      }
      // ---- 4. every member that ran is taken in, whatever happens to another one
      for (size_t s = 0; s < order.size(); ++s) {
        cur = order[s];
        Rrt& r = *members[cur];
        if (!launched[r.cfg.optimize ? 1 : 0]) continue;
        try { r.batch_take_in(); } catch (...) { fail(cur); }
      }
      if (err) break;
    }
  } catch (...) { fail(cur); }
  const double wall = ms_since(t0);
  for (int i = 0; i < n; ++i) members[i]->st.total_ms += wall;
  if (err) std::rethrow_exception(err);
}

}  // namespace sff
