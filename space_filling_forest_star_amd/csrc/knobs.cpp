// knobs.cpp — the one place of libsffgpu that reads the environment (knobs.h: when, and what each knob means).
#include "knobs.h"

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>

namespace sff {
namespace {

bool is_set(const char* name) { return getenv(name) != nullptr; }
// NAME=0 / NAME=1; unset = dflt
bool flag(const char* name, bool dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) != 0 : dflt;
}
// set: the value, clamped to [lo, hi]; unset = dflt (which may lie outside: "unset" stays distinguishable)
int int_in(const char* name, int dflt, int lo = INT_MIN, int hi = INT_MAX) {
  const char* e = getenv(name);
  return e ? std::min(hi, std::max(lo, atoi(e))) : dflt;
}
double double_min(const char* name, double dflt, double lo) {
  const char* e = getenv(name);
  return e ? std::max(lo, atof(e)) : dflt;
}
bool is(const char* name, const char* word) {
  const char* e = getenv(name);
  return e && !strcmp(e, word);
}

}  // namespace

Knobs Knobs::from_env() {
  Knobs k;
  k.timer_stride = int_in("SFFGPU_TIMER_STRIDE", k.timer_stride, 1);
  k.profile = is_set("SFFGPU_PROFILE");
  k.no_cand = flag("SFFGPU_NO_CAND", k.no_cand);
  k.no_clearance = flag("SFFGPU_NO_CLEARANCE", k.no_clearance);
  k.clear_cells = double_min("SFFGPU_CLEAR_CELLS", k.clear_cells, 512.0);
  k.clear_hdiv = double_min("SFFGPU_CLEAR_HDIV", k.clear_hdiv, 0.5);
  k.no_trigrid = flag("SFFGPU_NO_TRIGRID", k.no_trigrid);
  k.tg_div = double_min("SFFGPU_TG_DIV", k.tg_div, 1.0);
  k.test_grid_bk = int_in("SFFGPU_TEST_GRID_BK", k.test_grid_bk, 1, 8);
  k.test_grid_bkmax = int_in("SFFGPU_TEST_GRID_BKMAX", k.test_grid_bkmax, 1, 64);
  k.test_grid_ovf = int_in("SFFGPU_TEST_GRID_OVF", k.test_grid_ovf);
  k.compact_grid = flag("SFFGPU_COMPACT_GRID", k.compact_grid);
  k.test_grid_pool = int_in("SFFGPU_TEST_GRID_POOL", k.test_grid_pool, 1, 1 << 26);

  k.query = is("SFFGPU_QUERY", "wide") ? QUERY_WIDE : is("SFFGPU_QUERY", "block") ? QUERY_BLOCK : QUERY_AUTO;
  k.share = is_set("SFFGPU_SHARE") ? (flag("SFFGPU_SHARE", false) ? 1 : 0) : -1;
  k.seg_blocks = int_in("SFFGPU_SEG_BLOCKS", k.seg_blocks, 1, 4096);
  k.cull_blocks = int_in("SFFGPU_CULL_BLOCKS", k.cull_blocks);
  k.seg_listcap = int_in("SFFGPU_SEG_LISTCAP", k.seg_listcap);
  k.star_knn = is("SFFGPU_STAR_KNN", "lone") ? STAR_KNN_LONE : STAR_KNN_WG;

  k.engine = is("SFFGPU_ENGINE", "host") ? ENGINE_HOST : is("SFFGPU_ENGINE", "device") ? ENGINE_DEVICE : ENGINE_AUTO;
  k.prio_device = flag("SFFGPU_PRIO_DEVICE", k.prio_device);
  k.prio_seq = flag("SFFGPU_PRIO_SEQ", k.prio_seq);
  k.prio_loop = flag("SFFGPU_PRIO_LOOP", k.prio_loop);
  k.goal_loop = flag("SFFGPU_GOAL_LOOP", k.goal_loop);
  k.prio_goal_loop = flag("SFFGPU_PRIO_GOAL_LOOP", k.prio_goal_loop);
  k.no_order = flag("SFFGPU_NO_ORDER", k.no_order);
  k.order_min_wave = int_in("SFFGPU_ORDER_MIN_WAVE", k.order_min_wave, 2);
  k.test_hitcap = int_in("SFFGPU_TEST_HITCAP", k.test_hitcap, 1, 64);
  k.test_nbcap = int_in("SFFGPU_TEST_NBCAP", k.test_nbcap, 1);
  k.test_star_passes = int_in("SFFGPU_TEST_STAR_PASSES", k.test_star_passes, 1);
  k.test_exchange_self = is_set("SFFGPU_TEST_EXCHANGE_SELF");
  k.star_tail = flag("SFFGPU_STAR_TAIL", k.star_tail);
  k.star_tail_wgs = int_in("SFFGPU_STAR_TAIL_WGS", k.star_tail_wgs, 1);
  k.test_star_stall = int_in("SFFGPU_TEST_STAR_STALL", k.test_star_stall, 0);
  k.test_star_items = int_in("SFFGPU_TEST_STAR_ITEMS", k.test_star_items);
  k.test_border_cap = int_in("SFFGPU_TEST_BORDER_CAP", k.test_border_cap);
  k.no_graph = is_set("SFFGPU_NO_GRAPH") ? (flag("SFFGPU_NO_GRAPH", false) ? 1 : 0) : -1;
  {
    const char* pre = getenv("LD_PRELOAD");
    k.profiler_preloaded = pre && strstr(pre, "rocprofiler");
  }
  k.no_wave_ahead = is_set("SFFGPU_NO_WAVE_AHEAD");
  k.no_fused_sample = flag("SFFGPU_NO_FUSED_SAMPLE", k.no_fused_sample);
  k.no_zc_status = flag("SFFGPU_NO_ZC_STATUS", k.no_zc_status);
  k.fallback_whole_wave = is_set("SFFGPU_FALLBACK_WHOLE_WAVE");
  k.kc_trace = int_in("SFFGPU_KC_TRACE", k.kc_trace);
  k.digest = is_set("SFFGPU_DIGEST");
  k.no_seq = flag("SFFGPU_NO_SEQ", k.no_seq);
  k.spec = flag("SFFGPU_SPEC", k.spec);
  k.spec_depth = int_in("SFFGPU_SPEC_DEPTH", k.spec_depth);
  k.spec_sets = int_in("SFFGPU_SPEC_SETS", k.spec_sets);
  k.spec_pipe = flag("SFFGPU_SPEC_PIPE", k.spec_pipe);
  k.test_spec_stall = int_in("SFFGPU_TEST_SPEC_STALL", k.test_spec_stall);
  k.no_dev_trig = flag("SFFGPU_NO_DEV_TRIG", k.no_dev_trig);
  if (const char* e = getenv("SFFGPU_SEQ_TRACE")) k.seq_trace = e;

  k.rrt_chain = flag("SFFGPU_RRT_CHAIN", k.rrt_chain);
  k.rrt_fork = flag("SFFGPU_RRT_FORK", k.rrt_fork);
  k.rrt_repair = flag("SFFGPU_RRT_REPAIR", k.rrt_repair);
  k.rrt_dry = flag("SFFGPU_RRT_DRY", k.rrt_dry);
  k.rrt_one_chain = flag("SFFGPU_RRT_ONE_CHAIN", k.rrt_one_chain);
  k.rrt_split = int_in("SFFGPU_RRT_SPLIT", k.rrt_split, 1);
  k.rrt_small = int_in("SFFGPU_RRT_SMALL", k.rrt_small, 1);
  k.rrt_grow = int_in("SFFGPU_RRT_GROW", k.rrt_grow, 100);
  k.rrt_no_grid = is_set("SFFGPU_RRT_NO_GRID");
  k.rrt_no_chain_conn = is_set("SFFGPU_RRT_NO_CHAIN_CONN");
  k.lazy_batch = flag("SFFGPU_LAZY_BATCH", k.lazy_batch);

  k.smooth_loop = flag("SFFGPU_SMOOTH_LOOP", k.smooth_loop);
  k.smooth_edges = int_in("SFFGPU_SMOOTH_EDGES", k.smooth_edges, 1);

  k.paths_dev = flag("SFFGPU_PATHS_DEV", k.paths_dev);
  k.test_paths_cap = int_in("SFFGPU_TEST_PATHS_CAP", k.test_paths_cap, 1, 1 << 24);
  return k;
}

}  // namespace sff
