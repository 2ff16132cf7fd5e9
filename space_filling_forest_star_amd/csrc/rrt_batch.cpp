// rrt_batch.cpp — session batches: many independent RRT / RRT* / Multi-T-RRT sessions advanced in lock step.
//
// One session one iteration at a time (src/rrt.h:93-99) keeps one wavefront busy and nothing else; independent sessions
// need neither speculation nor co-residency: k_rrt_seq_batch gives every member a wavefront of its own that runs the
// reference's loop - nearest node, steer, pose and parent edge, the other live trees, RRT* choose-parent / rewire, append -
// with every edge checked only when the loop reaches it.  The lock step itself is run_lockstep (batch_lockstep.h); here is
// what is a session's own in it:
//   - a member is live while it has iterations to run; an iteration the kernel handed over (link + merge, an exact tie in a
//     merged tree's list, a capacity) runs alone through Rrt::expand first and the device block is uploaded again;
//   - its engine words come from the block's own copy of the generator;
//   - four kinds (RRT, RRT*, lazy RRT, lazy RRT*: the template instances of the kernel), at most batch_launch_iters iterations
//     a launch; a lazy edge (created under SFFGPU_LAZY_BATCH=1) that reaches its goal comes back solved and takes no further part;
//   - a member is taken in: node count of the store, the grid re-celled when its overflow list asks for it.
// The host mirror (nodes, tree lists, counters, the Mt64) is refreshed lazily (batch_sync_host): by the getters, by
// sffgpu_rrt_run and by the host iteration.
#include <cmath>
#include <cstring>

#include "batch_lockstep.h"

namespace sff {

#define HIPCHK(x) hip_check((x), #x)

Rrt::~Rrt() {
  BatchDev& d = bd;
  DevBuf* bufs[] = {&d.ctrl, &d.parent, &d.root_tree, &d.d_root, &d.d_closest, &d.iter, &d.live, &d.tree_cnt, &d.ktab};
  for (DevBuf* b : bufs) b->release();
  d.h_ctrl.release();
  d.wr.release();
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
    d.wr.init(1u << 17);   // (>= batch_launch_iters x 9 words + slack)
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
  d.wr.produced = rng.draws;
  d.wr.ring_pending = false;
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
  a.ring = d.wr.ring.as<uint64_t>();
  a.ring_mask = d.wr.ring_words - 1;
  a.words_end = d.wr.produced;
  a.ktab = d.ktab.as<int32_t>();
  memcpy(a.limits, cfg.limits, sizeof a.limits);
  memcpy(a.goal, cfg.goal, sizeof a.goal);
  a.priority_bias = cfg.priority_bias;
  a.dist_tree = cfg.dist_tree;
  a.sampling_dist = cfg.sampling_dist;
  // (the store's largest coordinate is only known up to the host mirror: the nodes the kernel adds lie within one step of the limits)
  double reach = std::max(c.store_maxabs, c.env_maxabs());
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
  if (d.last.status == SFFK_RRT_SOLVED) {   // a lazy edge reached its goal (Rrt::lazy_goal_check, on the device): the member is done
    solved = true;
    lazy_last = d.last.lazy_last;
    lazy_distance = d.last.lazy_distance;
  }
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
  expand(pick_tree(), (unsigned)iter);   // (a lazy edge: no word for the tree, and expand ends with lazy_goal_check)
  ++st.batch_host_iterations;
}

namespace {
struct RrtFamily {
  using Args = sffk::RrtSeqArgs;
  static constexpr int n_kinds = 4;   // RRT, RRT*, lazy RRT, lazy RRT*
  Rrt* const* m;
  int n, max_iterations;
  std::vector<int> iter0;

  int device() { return m[0]->ctx->device; }
  void begin(int i) { iter0[i] = m[i]->batch_iter(); }
  int plan(int i) {
    Rrt& r = *m[i];
    // (an iteration the kernel handed over: alone, through the host path - then the block goes up again)
    while (!r.batch_done(iter0[i], max_iterations) && r.bd.valid && r.bd.last.status == SFFK_RRT_HOST_ITER) r.batch_host_iteration();
    if (r.batch_done(iter0[i], max_iterations)) return 0;
    if (!r.bd.valid) r.batch_upload();
    int left = r.cfg.max_iterations - r.bd.last.iter;
    if (max_iterations > 0) left = std::min(left, max_iterations - (r.bd.last.iter - iter0[i]));
    return std::min(left, Rrt::batch_launch_iters);
  }
  uint64_t words_needed(int i, int iters) {
    const Rrt::BatchDev& d = m[i]->bd;
    const uint64_t ahead = (uint64_t)iters * 9 + 16, end = d.last.cursor + ahead;
    if (ahead > d.wr.ring_words) throw HipError{"rrt batch: engine-word ring too small (internal error)"};
    return end > d.wr.produced ? end - d.wr.produced : 0;
  }
  Mt64& gen(int i) { return m[i]->bd.gen; }
  void ring_append(int i, const uint64_t* w, size_t nw) { m[i]->bd.wr.append(m[i]->ctx->copy_stream, w, nullptr, nw); }
  WordRing& ring(int i) { return m[i]->bd.wr; }
  Args prepare(int i, int iters) { return m[i]->batch_prepare(iters); }
  int kind(int i) { return (m[i]->cfg.lazy_edge ? 2 : 0) + (m[i]->cfg.optimize ? 1 : 0); }
  hipStream_t stream(int i) { return m[i]->ctx->stream; }
  StatusBlock status(int i) { return {m[i]->bd.h_ctrl.p, m[i]->bd.ctrl.p, sizeof(sffk::RrtCtrl)}; }
  hipError_t launch(hipStream_t s, const Args* a, int count, int kind, size_t lds) { return sffk::launch_rrt_seq_batch(s, a, count, (kind & 1) != 0, (kind & 2) != 0, lds); }
  void take_in(int i, double*) { m[i]->batch_take_in(); }
  void finish(double wall, double) { for (int i = 0; i < n; ++i) m[i]->st.total_ms += wall; }
};
}  // namespace

void run_rrt_batch(Rrt* const* members, int n, int max_iterations, int* failed) {
  RrtFamily fam{members, n, max_iterations, std::vector<int>((size_t)n)};
  run_lockstep(fam, n, failed);
}

}  // namespace sff
