// paths_batch.cpp — path extraction of n forests together (engine.h: run_paths_batch; the kernel: devpaths.hip / devpaths.h).
//
// A call: every member's stream is drained.  The members whose state lives on the device (device-resident, ahead of the
// host mirror, between two waves, at most 64 trees) go to k_paths_batch - their arguments up as ONE copy, one launch on the
// first such member's stream, the headers back as ONE copy, one wait; the headers say how much of every member's packed
// answer is used, k_paths_gather puts those parts side by side and they come down as ONE copy: the surviving plans and the
// fp64 positions of their entries, nothing that grows with the forests or with a capacity.  Every other member, and a
// member whose plan pool ran out, takes the host route: sync_host, then max_connected + get_paths + get_all_paths on the
// mirror.  Only when every answer is on the host (and every host-route mirror is current) are the forests touched - pure
// host work, member by member.
#include <chrono>
#include <cstring>
#include <exception>

#include "devpaths.h"
#include "engine.h"

namespace sff {

namespace {

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
constexpr int kDefaultPathsCap = 8192;   // plan entries of a forest's pool (56 bytes each + the rows)

struct Answer {
  bool device = false, fallback = false, synced = false;
  std::vector<Forest::Holder> nm;
  std::vector<int> connected;
  std::unordered_map<int, std::array<double, 6>> pos;
  uint64_t entries = 0;
  std::vector<int32_t> b_ta, b_tb;   // the mirror's share of the device's border columns (host_borders > 0)
  std::vector<double> b_dist;
};

bool device_route(const Forest& f) {
  return f.dev.active && f.dev.host_stale && !f.dev.last.in_wave && f.num_roots <= SFFK_PATHS_MAX_TREES;
}

void paths_buffers(Forest& f) {
  const int T = f.num_roots;
  f.pd.cap = f.kn.test_paths_cap > 0 ? f.kn.test_paths_cap : kDefaultPathsCap;
  f.pd.rows.ensure((size_t)T * T * sizeof(sffk::PathRow));
  f.pd.pool.ensure(std::max<size_t>(8, (size_t)f.pd.cap * 4));
  f.pd.packed.ensure(std::max<size_t>(8, sffk::paths_packed_bytes(T * (T - 1) / 2, f.pd.cap)));
}

sffk::PathsArgs paths_args(Forest& f, sffk::PathsHead* head_dev) {
  const Ctx& c = *f.ctx;
  const DevEngine& d = f.dev;
  sffk::PathsArgs a{};
  a.ctrl = d.ctrl.as<sffk::DevCtrl>();
  a.spos = c.spos.as<double>();
  a.stree = c.stree.as<int32_t>();
  a.parent = d.parent.as<int32_t>();
  a.d_root = d.d_root.as<double>();
  a.b_n1 = d.b_n1.as<int32_t>(); a.b_n2 = d.b_n2.as<int32_t>(); a.b_ta = d.b_ta.as<int32_t>(); a.b_tb = d.b_tb.as<int32_t>();
  a.b_dist = d.b_dist.as<double>();
  a.pair = d.pair.as<uint8_t>();
  a.rows = f.pd.rows.as<sffk::PathRow>();
  a.pool = f.pd.pool.as<int32_t>();
  a.packed = f.pd.packed.as<char>();
  a.head = head_dev;
  a.n_trees = f.num_roots;
  a.pool_cap = f.pd.cap;
  // what the kernel may index: the smallest extent of the arrays it reads per node / per border
  a.node_cap = (int)std::min<size_t>({(size_t)d.node_cap, (size_t)c.store_cap, d.parent.cap / 4, d.d_root.cap / 8, c.spos.cap / 48, c.stree.cap / 4});
  a.border_cap = (int)std::min<size_t>({(size_t)d.border_cap, d.b_n1.cap / 4, d.b_n2.cap / 4, d.b_ta.cap / 4, d.b_tb.cap / 4, d.b_dist.cap / 8});
  return a;
}

// a member's packed answer -> the forest's rows, checked against what the forest can hold
void take_answer(const Forest& f, const sffk::PathsHead& h, const char* packed, Answer& out) {
  const int T = f.num_roots;
  if (h.n_connected < 0 || h.n_connected > T) throw HipError{"paths: the connected set came back out of range"};
  out.connected.assign(h.connected, h.connected + h.n_connected);
  for (int t : out.connected)
    if (t < 0 || t >= T) throw HipError{"paths: a connected tree came back out of range"};
  out.nm.assign((size_t)T * T, Forest::Holder());
  const sffk::PathRowOut* rows = reinterpret_cast<const sffk::PathRowOut*>(packed);
  const int32_t* ids = reinterpret_cast<const int32_t*>(packed + (size_t)h.n_rows * sizeof(sffk::PathRowOut));
  const double* pos = reinterpret_cast<const double*>(packed + (size_t)h.n_rows * sizeof(sffk::PathRowOut) + (((size_t)h.n_entries * 4 + 7) & ~(size_t)7));
  size_t at = 0;
  for (int r = 0; r < h.n_rows; ++r) {
    const sffk::PathRowOut& o = rows[r];
    if (o.i < 0 || o.i >= o.j || o.j >= T || o.len < 2 || at + (size_t)o.len > (size_t)h.n_entries || o.n1 < 0 || o.n2 < 0 || o.n1 >= h.n_nodes || o.n2 >= h.n_nodes)
      throw HipError{"paths: a row came back out of range"};
    Forest::Holder& H = out.nm[(size_t)o.i * T + o.j];
    H.n1 = o.n1;
    H.n2 = o.n2;
    H.dist = o.dist;
    H.plan.assign(ids + at, ids + at + o.len);
    for (int q = 0; q < o.len; ++q) {
      const int id = ids[at + (size_t)q];
      if (id < 0 || id >= h.n_nodes) throw HipError{"paths: a plan entry came back out of range"};
      std::array<double, 6> p;
      memcpy(p.data(), pos + 6 * (at + (size_t)q), 48);
      out.pos[id] = p;
    }
    at += (size_t)o.len;
  }
  if (at != (size_t)h.n_entries) throw HipError{"paths: the plans came back with an impossible length"};
  out.entries = at;
}

}  // namespace

const double* Forest::node_pos(int id) const {
  if (id >= 0 && (size_t)id < nodes.size()) return nodes[(size_t)id].pos;
  const auto it = pos_cache.find(id);
  return it == pos_cache.end() ? nullptr : it->second.data();
}

void run_paths_batch(Forest* const* members, int n, int* failed) {
  using Clock = std::chrono::steady_clock;
  const auto t0 = Clock::now();
  *failed = -1;
  int cur = 0;   // the member being worked for: whatever is thrown has a member to name
  std::vector<Answer> ans((size_t)n);
  std::vector<int> devm;   // the device-route members
  uint64_t launches = 0;
  try {
    hip_check(hipSetDevice(members[0]->ctx->device), "hipSetDevice");
    for (int i = 0; i < n; ++i) {
      cur = i;
      members[i]->ctx->sync();
      if (device_route(*members[i])) {
        ans[(size_t)i].device = true;
        devm.push_back(i);
        paths_buffers(*members[i]);
      }
    }
    if (!devm.empty()) {
      cur = devm[0];
      Ctx& c0 = *members[cur]->ctx;
      hipStream_t s = c0.stream;
      const size_t nD = devm.size();
      // ---- the launch: member arguments | answer headers
      const size_t o_head = up256(nD * sizeof(sffk::PathsArgs)), bytes1 = o_head + nD * sizeof(sffk::PathsHead);
      c0.pp_pin.ensure(bytes1);
      c0.pp_dev.ensure(bytes1);
      char* hb = c0.pp_pin.as<char>();
      char* db = c0.pp_dev.as<char>();
      memset(hb, 0, bytes1);
      sffk::PathsArgs* ha = reinterpret_cast<sffk::PathsArgs*>(hb);
      for (size_t k = 0; k < nD; ++k) {
        cur = devm[k];
        ha[k] = paths_args(*members[cur], reinterpret_cast<sffk::PathsHead*>(db + o_head) + k);
      }
      cur = devm[0];
      hip_check(hipMemcpyAsync(db, hb, o_head, hipMemcpyHostToDevice, s), "paths: member arguments");
      hip_check(sffk::launch_paths_batch(s, reinterpret_cast<const sffk::PathsArgs*>(db), (int)nD), "paths: launch");
      ++launches;
      hip_check(hipMemcpyAsync(hb + o_head, db + o_head, nD * sizeof(sffk::PathsHead), hipMemcpyDeviceToHost, s), "paths: headers");
      hip_check(hipStreamSynchronize(s), "paths: wait");
      std::vector<sffk::PathsHead> heads(nD);
      memcpy(heads.data(), hb + o_head, nD * sizeof(sffk::PathsHead));
      // ---- the used parts of the answers, side by side
      std::vector<size_t> part_off(nD, 0), part_bytes(nD, 0);
      size_t total = 0;
      for (size_t k = 0; k < nD; ++k) {
        cur = devm[k];
        const sffk::PathsHead& h = heads[k];
        Forest& f = *members[cur];
        if (h.status == SFFK_PATHS_POOL_FULL) { ans[(size_t)cur].fallback = true; continue; }
        if (h.status != SFFK_PATHS_OK) throw HipError{"paths: the forest's device state is inconsistent (a count or an id outside its arrays)"};
        const int T = f.num_roots;
        if (h.n_rows < 0 || h.n_rows > T * (T - 1) / 2 || h.n_entries < 0 || h.n_entries > f.pd.cap)
          throw HipError{"paths: an answer header came back out of range"};
        part_off[k] = total;
        part_bytes[k] = sffk::paths_packed_bytes(h.n_rows, h.n_entries);
        total += part_bytes[k];
      }
      cur = devm[0];
      if (total > 0) {
        const size_t o_data = up256(nD * sizeof(sffk::PathsGather)), bytes2 = o_data + total;
        c0.pp_pin.ensure(bytes2);
        c0.pp_dev.ensure(bytes2);
        hb = c0.pp_pin.as<char>();
        db = c0.pp_dev.as<char>();
        sffk::PathsGather* hg = reinterpret_cast<sffk::PathsGather*>(hb);
        memset(hb, 0, o_data);
        for (size_t k = 0; k < nD; ++k) {
          hg[k].src = members[devm[k]]->pd.packed.as<char>();
          hg[k].dst = db + o_data + part_off[k];
          hg[k].bytes = part_bytes[k];
        }
        hip_check(hipMemcpyAsync(db, hb, o_data, hipMemcpyHostToDevice, s), "paths: gather table");
        hip_check(sffk::launch_paths_gather(s, reinterpret_cast<const sffk::PathsGather*>(db), (int)nD), "paths: gather");
        hip_check(hipMemcpyAsync(hb + o_data, db + o_data, total, hipMemcpyDeviceToHost, s), "paths: plans");
        hip_check(hipStreamSynchronize(s), "paths: wait");
        hb += o_data;
      }
      for (size_t k = 0; k < nD; ++k) {
        cur = devm[k];
        Answer& a = ans[(size_t)cur];
        if (a.fallback) continue;
        Forest& f = *members[cur];
        take_answer(f, heads[k], hb + part_off[k], a);
        // get_paths rewrites every border's dist: the borders the mirror already holds take theirs from the device column
        const int hbn = std::min(f.dev.host_borders, heads[k].n_borders);
        if (hbn > 0) {
          a.b_ta.resize((size_t)hbn); a.b_tb.resize((size_t)hbn); a.b_dist.resize((size_t)hbn);
          hip_check(hipMemcpy(a.b_ta.data(), f.dev.b_ta.p, (size_t)hbn * 4, hipMemcpyDeviceToHost), "paths: border columns");
          hip_check(hipMemcpy(a.b_tb.data(), f.dev.b_tb.p, (size_t)hbn * 4, hipMemcpyDeviceToHost), "paths: border columns");
          hip_check(hipMemcpy(a.b_dist.data(), f.dev.b_dist.p, (size_t)hbn * 8, hipMemcpyDeviceToHost), "paths: border columns");
        }
      }
    }
    // ---- the host route's download (the only part of it that can fail)
    for (int i = 0; i < n; ++i) {
      Answer& a = ans[(size_t)i];
      if (a.device && !a.fallback) continue;
      cur = i;
      Forest& f = *members[i];
      a.synced = f.dev.active && f.dev.host_stale;
      f.sync_host();
    }
  } catch (...) {
    *failed = cur;
    throw;
  }
  // ---- every answer is here: the forests take theirs
  const double ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
  for (int i = 0; i < n; ++i) {
    Forest& f = *members[i];
    Answer& a = ans[(size_t)i];
    if (a.device && !a.fallback) {
      f.nm.swap(a.nm);
      f.connected.swap(a.connected);
      f.pos_cache.swap(a.pos);
      // the flat list keeps every pair's list order (forest_dev.cpp, dev_upload_state): entry by entry, pair by pair
      std::map<std::pair<int, int>, size_t> next;
      for (size_t e = 0; e < a.b_dist.size(); ++e) {
        const std::pair<int, int> key{std::min(a.b_ta[e], a.b_tb[e]), std::max(a.b_ta[e], a.b_tb[e])};
        const auto it = f.borders.find(key);
        size_t& q = next[key];
        if (it != f.borders.end() && q < it->second.size()) it->second[q].dist = a.b_dist[e];
        ++q;
      }
      f.ps.device_calls += 1;
      f.ps.launches += launches;
      f.ps.entries += a.entries;
    } else {
      f.max_connected();                 // Solver::connectedTrees as Solve() leaves it (src/forest.h:196-206)
      f.get_paths();
      f.get_all_paths();
      f.pos_cache.clear();
      if (a.device) { f.ps.fallbacks += 1; f.ps.launches += launches; }
      else f.ps.host_calls += 1;
    }
    if (a.synced) f.ps.host_syncs += 1;
    f.ps.calls += 1;
    uint64_t pairs = 0;
    for (const Forest::Holder& h : f.nm) pairs += h.exists() ? 1 : 0;
    f.ps.pairs = pairs;
    f.ps.ms += ms;
  }
}

}  // namespace sff
