// smooth_batch.cpp — path smoothing on the device: the paths of n planners through k_smooth_paths (kernels.h: SmoothPathArgs,
// smooth_paths.inc), one wavefront per path, and what each planner makes of the answer.  engine.h says what a member is.
//
// A call: every member's stream is drained; the fp64 positions of every plan entry are gathered from the members' host
// mirrors (sffgpu_forest_paths / sffgpu_rrt_paths have synced them) or, behind sffgpu_forest_paths_batch's device route,
// from the positions that came down with the plans, and go up with the path table and the control blocks as
// ONE copy; one launch on the first member's stream, the control blocks and output rows back as ONE copy, one wait; again
// while a path is unfinished (a launch tests at most Knobs::smooth_edges edges of a path).  A step the kernel hands over
// (SFFK_SMOOTH_HOST) is finished here through the member's Ctx::collide_segments.  Only when every path of every member is
// decided are the planners touched, member by member - pure host work that cannot fail half way.
#include <chrono>
#include <cstring>
#include <exception>

#include "engine.h"
#include "sff_geom.h"

namespace sff {

namespace {

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

struct PathRef { int member, path, len; size_t pos_off; };   // pos_off: first entry of the path in the positions / output arrays

}  // namespace

void run_smooth_batch(SmoothMember* members, int n, int* failed) {
  using Clock = std::chrono::steady_clock;
  const auto t0 = Clock::now();
  *failed = -1;
  int cur = 0;   // the member being worked for: whatever is thrown has a member to name
  std::vector<PathRef> tab;                       // the paths with an edge to test (three entries or more)
  std::vector<std::vector<std::vector<int32_t>>> steps((size_t)n);   // per member, per path: the chosen t of every step
  std::vector<uint64_t> pf_add((size_t)n, 0), cc_add((size_t)n, 0), host_edges((size_t)n, 0);
  uint64_t launches = 0;
  try {
    hip_check(hipSetDevice(members[0].ctx->device), "hipSetDevice");
    size_t total = 0, lds = 0;
    for (int i = 0; i < n; ++i) {
      cur = i;
      SmoothMember& m = members[i];
      m.ctx->sync();
      steps[(size_t)i].resize(m.plans.size());
      for (size_t p = 0; p < m.plans.size(); ++p) {
        const int len = (int)m.plans[p]->size();
        if (len == 2) steps[(size_t)i][p].push_back(0);   // (g = 1: no candidate, t = g - 1)
        if (len < 3) continue;
        if (!m.ctx->have_env() || !m.ctx->have_robot()) throw HipError{"smooth_paths: upload ENV and ROBOT meshes first"};
        tab.push_back(PathRef{i, (int)p, len, total});
        total += (size_t)len;
        lds = std::max(lds, sffk::collide_lds_bytes(m.ctx->robv.n_tri, 1));
      }
    }
    if (!tab.empty()) {
      cur = tab[0].member;
      Ctx& c0 = *members[cur].ctx;
      hipStream_t s = c0.stream;
      const size_t nP = tab.size();
      // one image, host and device: path table | control blocks | output rows | positions
      const size_t o_ctrl = up256(nP * sizeof(sffk::SmoothPathArgs)), o_out = o_ctrl + up256(nP * sizeof(sffk::SmoothCtrl)),
                   o_pos = o_out + up256(total * sizeof(int32_t)), bytes = o_pos + total * 6 * sizeof(double);
      c0.sm_pin.ensure(bytes);
      c0.sm_dev.ensure(bytes);
      char* hb = c0.sm_pin.as<char>();
      char* db = c0.sm_dev.as<char>();
      sffk::SmoothPathArgs* ha = reinterpret_cast<sffk::SmoothPathArgs*>(hb);
      sffk::SmoothCtrl* hc = reinterpret_cast<sffk::SmoothCtrl*>(hb + o_ctrl);
      int32_t* hout = reinterpret_cast<int32_t*>(hb + o_out);
      double* hpos = reinterpret_cast<double*>(hb + o_pos);
      memset(hb, 0, o_pos);
      for (size_t k = 0; k < nP; ++k) {
        const PathRef& r = tab[k];
        cur = r.member;
        SmoothMember& m = members[r.member];
        const std::vector<int>& plan = *m.plans[(size_t)r.path];
        for (int e = 0; e < r.len; ++e) memcpy(hpos + 6 * (r.pos_off + (size_t)e), m.pos(plan[(size_t)e]), 48);
        sffk::SmoothPathArgs& a = ha[k];
        a.ctrl = reinterpret_cast<sffk::SmoothCtrl*>(db + o_ctrl) + k;
        a.pos = reinterpret_cast<const double*>(db + o_pos) + 6 * r.pos_off;
        a.out = reinterpret_cast<int32_t*>(db + o_out) + r.pos_off;
        a.env = m.ctx->envv;
        a.rob = m.ctx->robv;
        a.len = r.len;
        a.max_edges = std::max(1, m.max_edges);
        hc[k].g = r.len - 1;
      }
      cur = tab[0].member;
      hip_check(hipMemcpyAsync(db, hb, bytes, hipMemcpyHostToDevice, s), "smooth_paths: path table");
      std::vector<sffk::SmoothCtrl> before(nP);
      while (true) {
        bool live = false;
        for (size_t k = 0; k < nP; ++k) live = live || hc[k].g > 0;
        if (!live) break;
        memcpy(before.data(), hc, nP * sizeof(sffk::SmoothCtrl));
        cur = tab[0].member;
        hip_check(sffk::launch_smooth_paths(s, reinterpret_cast<const sffk::SmoothPathArgs*>(db), (int)nP, lds), "smooth_paths: launch");
        ++launches;
        hip_check(hipMemcpyAsync(hb + o_ctrl, db + o_ctrl, o_pos - o_ctrl, hipMemcpyDeviceToHost, s), "smooth_paths: control blocks");
        hip_check(hipStreamSynchronize(s), "smooth_paths: wait");
        // ---- a step the kernel could not decide: its remaining candidates in one batch on the member's own context, the
        // first free one taken, counted like the early stop (the host walk of paths.cpp from t_next on)
        bool handed = false, moved = false;
        for (size_t k = 0; k < nP; ++k) {
          sffk::SmoothCtrl& c = hc[k];
          moved = moved || c.g != before[k].g || c.t_next != before[k].t_next || c.n_out != before[k].n_out;
          if (c.status != SFFK_SMOOTH_HOST) continue;
          const PathRef& r = tab[k];
          cur = r.member;
          const int g = c.g, m = g - 1 - c.t_next;
          if (g <= 0 || g >= r.len || m <= 0 || c.n_out < 0 || c.n_out >= r.len) throw HipError{"smooth_paths: a control block came back out of range"};
          const double* P = hpos + 6 * r.pos_off;
          std::vector<double> a((size_t)m * 6), b((size_t)m * 6);
          for (int q = 0; q < m; ++q) {
            memcpy(&a[6 * (size_t)q], P + 6 * (size_t)(c.t_next + q), 48);
            memcpy(&b[6 * (size_t)q], P + 6 * (size_t)g, 48);
          }
          std::vector<uint8_t> fr((size_t)m);
          std::vector<int32_t> fh((size_t)m), nsv((size_t)m);
          members[cur].ctx->collide_segments(a.data(), b.data(), m, fr.data(), fh.data(), nsv.data());
          int q = 0;
          for (; q < m; ++q) {
            c.path_free_calls += 1;
            c.collide_calls += fh[(size_t)q] > 0 ? (uint64_t)fh[(size_t)q] : (uint64_t)nsv[(size_t)q];
            host_edges[(size_t)cur] += 1;
            if (fr[(size_t)q]) break;
          }
          const int t = c.t_next + q;   // (q == m: none was free, t = g - 1)
          hout[r.pos_off + (size_t)c.n_out] = t;
          c.n_out += 1;
          c.g = t;
          c.t_next = 0;
          c.status = SFFK_SMOOTH_RAN;
          handed = moved = true;
        }
        cur = tab[0].member;
        if (!moved) throw HipError{"smooth_paths: a launch made no progress"};
        if (handed) hip_check(hipMemcpyAsync(db + o_ctrl, hb + o_ctrl, o_pos - o_ctrl, hipMemcpyHostToDevice, s), "smooth_paths: control blocks up");
      }
      for (size_t k = 0; k < nP; ++k) {
        const PathRef& r = tab[k];
        cur = r.member;
        const sffk::SmoothCtrl& c = hc[k];
        if (c.n_out < 1 || c.n_out >= r.len) throw HipError{"smooth_paths: a path came back with an impossible step count"};
        const int32_t* o = hout + r.pos_off;
        for (int q = 0, g = r.len - 1; q < c.n_out; g = o[q], ++q)   // every t is a candidate of its step, or g - 1
          if (o[q] < 0 || o[q] >= g) throw HipError{"smooth_paths: a path came back with an impossible step"};
        steps[(size_t)r.member][(size_t)r.path].assign(o, o + c.n_out);
        pf_add[(size_t)r.member] += c.path_free_calls;
        cc_add[(size_t)r.member] += c.collide_calls;
      }
    }
  } catch (...) {
    *failed = cur;
    throw;
  }
  // ---- every path is decided: the planners take their answers
  const double ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
  std::vector<uint8_t> launched((size_t)n, 0);
  for (const PathRef& r : tab) launched[(size_t)r.member] = 1;
  for (int i = 0; i < n; ++i) {
    SmoothMember& m = members[i];
    uint64_t n_steps = 0;
    for (size_t p = 0; p < m.plans.size(); ++p) {
      const std::vector<int32_t>& ts = steps[(size_t)i][p];
      n_steps += ts.size();
      m.apply((int)p, ts.data(), (int)ts.size());
    }
    *m.path_free_calls += pf_add[(size_t)i];
    *m.collide_calls += cc_add[(size_t)i];
    m.stats->launches += launched[(size_t)i] ? launches : 0;
    m.stats->paths += m.plans.size();
    m.stats->steps += n_steps;
    m.stats->edges += pf_add[(size_t)i];
    m.stats->host_edges += host_edges[(size_t)i];
    m.stats->ms += ms;
  }
}

// Forest: the walk of Forest::smooth_paths (paths.cpp) with the answer of every step known - the same fp64 expressions in the
// same order, so the costs come out bit for bit (cum, prev_dist, h.dist -= dif)
SmoothMember smooth_member(Forest& f) {
  SmoothMember m;
  m.ctx = f.ctx;
  m.max_edges = f.kn.smooth_edges;
  m.stats = &f.sm;
  // (while the device holds the forest's counters - paths extracted there, nothing downloaded - st is not what the getters read)
  const bool behind = f.dev.active && f.dev.host_stale;
  m.path_free_calls = behind ? &f.post_path_free : &f.st.path_free_calls;
  m.collide_calls = behind ? &f.post_collide : &f.st.collide_calls;
  std::vector<Forest::Holder*> holders;
  for (int i = 0; i < f.num_roots; ++i)
    for (int j = i + 1; j < f.num_roots; ++j) {
      Forest::Holder& h = f.NM(i, j);
      if (!h.exists()) continue;
      holders.push_back(&h);
      m.plans.push_back(&h.plan);
    }
  Forest* F = &f;
  // (positions through the forest's accessor: the mirror's, or - after sffgpu_forest_paths_batch took the device route and
  // nothing has been downloaded since - the ones that came down with the plans)
  m.pos = [F](int node) {
    const double* p = F->node_pos(node);
    if (!p) throw HipError{"smooth_paths: the position of a plan entry is not on the host"};
    return p;
  };
  m.apply = [F, holders](int path, const int32_t* ts, int n_ts) {
    Forest::Holder& h = *holders[(size_t)path];
    std::vector<int>& plan = h.plan;
    int g = (int)plan.size() - 1, k = 0;
    double prev_dist = h.dist;
    while (g > 0 && k < n_ts) {
      const int chosen = ts[k++];
      int p = 0, t = 0;
      double cum = 0;
      bool changed = false;
      while (t < g - 1) {
        if (p != t) cum += sffg::dist6(F->node_pos(plan[t]), F->node_pos(plan[p]));
        if (t == chosen) { changed = true; break; }
        p = t;
        ++t;
      }
      if (t == g - 1) cum += sffg::dist6(F->node_pos(plan[t]), F->node_pos(plan[p]));
      if (changed) {
        double dif = prev_dist - cum - sffg::dist6(F->node_pos(plan[t]), F->node_pos(plan[g]));
        h.dist -= dif;
        plan.erase(plan.begin() + t + 1, plan.begin() + g);
      }
      prev_dist = cum;
      g = t;
    }
  };
  return m;
}

// Rrt: the link plans shrink; neighboringMatrix keeps the copies made earlier (rrt.cpp, Rrt::smooth_paths)
SmoothMember smooth_member(Rrt& r) {
  SmoothMember m;
  m.ctx = r.ctx;
  m.max_edges = r.kn.smooth_edges;
  m.stats = &r.sm;
  m.path_free_calls = &r.st.path_free_calls;
  m.collide_calls = &r.st.collide_calls;
  for (std::vector<int>& plan : r.link_plans) m.plans.push_back(&plan);
  Rrt* R = &r;
  m.pos = [R](int node) { return R->nodes[(size_t)node].pos; };
  m.apply = [R](int path, const int32_t* ts, int n_ts) {
    std::vector<int>& plan = R->link_plans[(size_t)path];
    int g = (int)plan.size() - 1;
    for (int k = 0; k < n_ts && g > 0; ++k) {
      const int t = ts[k];
      if (t < g - 1) plan.erase(plan.begin() + t + 1, plan.begin() + g);
      g = t;
    }
  };
  return m;
}

}  // namespace sff
