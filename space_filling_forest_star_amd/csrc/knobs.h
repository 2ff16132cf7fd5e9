// knobs.h — every SFFGPU_* environment knob of libsffgpu, as one plain struct.
//
// The environment is read in ONE place, Knobs::from_env() (knobs.cpp), and at these moments only: when a context is
// created, a mesh is uploaded, a stand-alone node store / index is set up (sffgpu_nodes_reset / sffgpu_nodes_index) and
// when a forest or an RRT session is created.  Ctx::kn holds the snapshot of the last of them; a Forest / Rrt keeps a copy
// of its own and behaves for its whole life as the environment said when it was created, graph captures included.
// No HIP in here: the host compiler builds knobs.cpp alone (tests/knobs_harness.cpp).
#pragma once
#include <string>

namespace sff {

struct Knobs {
  enum Engine { ENGINE_AUTO, ENGINE_HOST, ENGINE_DEVICE };
  enum Query { QUERY_AUTO, QUERY_WIDE, QUERY_BLOCK };
  enum StarKnn { STAR_KNN_WG, STAR_KNN_LONE };

  // ---- context, meshes, node grid
  int timer_stride = 32;            // SFFGPU_TIMER_STRIDE (>= 1): every n-th wave / round is launched eagerly with HIP events around the timed
                                    // kernels (an event-bracketed wave costs ~0.25 ms more than its graph replay: 8 -> 32 is + 2-3 % on the headline job)
  bool profile = false;             // SFFGPU_PROFILE (set at all): phase clocks and host events on stderr
  bool no_cand = false;             // SFFGPU_NO_CAND=1: candidate triangles gathered from the four arrays (A/B) instead of the packed records
  bool no_clearance = false;        // SFFGPU_NO_CLEARANCE=1: no clearance bits
  double clear_cells = 134217728.0; // SFFGPU_CLEAR_CELLS (>= 512): cell budget of the clearance grid
  double clear_hdiv = 2.0;          // SFFGPU_CLEAR_HDIV (>= 0.5): clearance cell = robot radius / x
  bool no_trigrid = false;          // SFFGPU_NO_TRIGRID=1: box hierarchy instead of the triangle grid
  double tg_div = 3.0;              // SFFGPU_TG_DIV (>= 1): the triangle grid's cell size divisor
  int test_grid_bk = 8;             // SFFGPU_TEST_GRID_BK (1..8), tests: tiny buckets to start with
  int test_grid_bkmax = 64;         // SFFGPU_TEST_GRID_BKMAX (1..64), tests: shallow buckets
  int test_grid_ovf = -1;           // SFFGPU_TEST_GRID_OVF, tests: tiny overflow list (raw value, < 0 = unset; Ctx::grid_setup scales it)
  bool compact_grid = false;        // SFFGPU_COMPACT_GRID=1: a member context (sffgpu_create_member) created under it starts with the compact node grid
                                    // (sffk::GridView::bucket: buckets from a pool sized by the node store); sffgpu_create contexts never do
  int test_grid_pool = 0;           // SFFGPU_TEST_GRID_POOL=n (>= 1), tests: first pool capacity of a compact grid (0 = unset: the store's capacity)

  // ---- launch shapes (kernels.hip / devstar.hip)
  Query query = QUERY_AUTO;         // SFFGPU_QUERY=wide / block: force k_query_classify / k_query_block
  int share = -1;                   // SFFGPU_SHARE=0 / 1: many-candidate items shared by the workgroup's wavefronts never / always (-1 = unset: by triangle count)
  int seg_blocks = 0;               // SFFGPU_SEG_BLOCKS (1..4096): grid of the exact kernels (0 = unset: each launcher's own width)
  int cull_blocks = 2048;           // SFFGPU_CULL_BLOCKS: grid of the cull kernel's edge part
  int seg_listcap = -1;             // SFFGPU_SEG_LISTCAP, tests: shrink the survivor / work-item list so that the table-scan path runs (< 0 = unset)
  StarKnn star_knn = STAR_KNN_WG;   // SFFGPU_STAR_KNN=lone: the one-wavefront k-nearest kernel instead of k_star_knn_wg

  // ---- forest
  Engine engine = ENGINE_AUTO;      // SFFGPU_ENGINE=host / device: the host-replay engine / insist on the device-resident one
  bool prio_device = true;          // SFFGPU_PRIO_DEVICE=0: priority-frontier mode stays on the host-replay engine
  bool prio_seq = false;            // SFFGPU_PRIO_SEQ=1 (tests): picks by the sequential k_prio_begin instead of k_prio_plan
  bool prio_loop = false;           // SFFGPU_PRIO_LOOP=1: a priority-frontier forest without a goal of waves of ONE slot runs on the device, in the
                                    // single-wavefront loop (k_seq_waves_batch<., true>), and may be a member of a forest batch; 0 = the host-replay engine
  bool goal_loop = false;           // SFFGPU_GOAL_LOOP=1: a single-goal forest (has_goal, no priority frontier) of waves of ONE slot runs in the
                                    // single-wavefront loop (k_seq_waves_batch<., false, true>) and may be a member of a forest batch; 0 = the round engine,
                                    // the solving wave replayed on the host
  bool prio_goal_loop = false;      // SFFGPU_PRIO_GOAL_LOOP=1: a forest with BOTH a goal and a priority bias (one heap per start tree, keyed by the distance
                                    // to the goal) of waves of ONE slot runs in the single-wavefront loop (k_seq_waves_batch<., true, true>) and may be a member
                                    // of a forest batch; 0 = the host-replay engine.  Neither prio_loop nor goal_loop covers the combination
  bool no_order = false;            // SFFGPU_NO_ORDER=1: a round's samples by index instead of in the wave's spatial order (sffk::OrderView)
  int order_min_wave = 4096;        // SFFGPU_ORDER_MIN_WAVE (>= 2): smallest wave that uses the order
  int test_hitcap = 64;             // SFFGPU_TEST_HITCAP (1..64: one lane per hit), tests: device hit list
  int test_nbcap = 15;              // SFFGPU_TEST_NBCAP (>= 1), tests: device neighbour list
  int test_star_passes = 0;         // SFFGPU_TEST_STAR_PASSES (>= 1): most passes of an SFF* round's fixed point (0 = the kernels' own limit)
  bool test_exchange_self = false;  // SFFGPU_TEST_EXCHANGE_SELF (set at all): a one-rank forest packs / unpacks its records too
  bool star_tail = true;            // SFFGPU_STAR_TAIL=0: one launch per SFF* pass instead of k_star_tail
  int star_tail_wgs = 0;            // SFFGPU_STAR_TAIL_WGS (>= 1): upper bound of k_star_tail's grid (0 = one workgroup per CU)
  int test_star_stall = 0;          // SFFGPU_TEST_STAR_STALL=n (>= 0), tests: in every n-th round one workgroup never arrives at the first barrier
  int test_star_items = -1;         // SFFGPU_TEST_STAR_ITEMS, tests: survivor items of one SFF* pass (raw value, < 0 = unset)
  int test_border_cap = -1;         // SFFGPU_TEST_BORDER_CAP, tests: first border capacity, small table: force growth (raw value, < 0 = unset)
  int no_graph = -1;                // SFFGPU_NO_GRAPH=1 / 0: waves launched kernel by kernel / as a graph whatever is preloaded (-1 = unset: SFF* waves
                                    // go kernel by kernel under a profiler, see profiler_preloaded)
  bool profiler_preloaded = false;  // LD_PRELOAD names a rocprofiler library
  bool no_wave_ahead = false;       // SFFGPU_NO_WAVE_AHEAD (set at all): no wave kept enqueued ahead
  bool no_fused_sample = false;     // SFFGPU_NO_FUSED_SAMPLE=1: k_append + k_sample_steer as two launches
  bool no_zc_status = false;        // SFFGPU_NO_ZC_STATUS=1: the wave's status block comes by a copy launch instead of the pinned ring
  bool fallback_whole_wave = false; // SFFGPU_FALLBACK_WHOLE_WAVE (set at all): a list fault hands the rest of the wave (not one round) to the host
  int kc_trace = -1;                // SFFGPU_KC_TRACE=<round>: that round's k_commit timeline with SFFGPU_PROFILE (-1 = off)
  bool digest = false;              // SFFGPU_DIGEST (set at all): the host-replay engine prints every round's answers
  // waves of one slot
  bool no_seq = false;              // SFFGPU_NO_SEQ=1: through the round engine instead of k_seq_waves_batch / k_spec_waves
  bool spec = true;                 // SFFGPU_SPEC=0: the single wavefront (k_seq_waves_batch) instead of the speculative kernel
  int spec_depth = 0;               // SFFGPU_SPEC_DEPTH: waves per step (0 = 3, the tree; SFF*: 4, the chain)
  int spec_sets = 1;                // SFFGPU_SPEC_SETS: sets of workers that take the steps in turn
  bool spec_pipe = true;            // SFFGPU_SPEC_PIPE=0: write a step's nodes before the next one is published
  int test_spec_stall = 0;          // SFFGPU_TEST_SPEC_STALL=8 x step + slot, tests: that worker never answers
  bool no_dev_trig = false;         // SFFGPU_NO_DEV_TRIG=1: no cos / sin / acos table
  std::string seq_trace;            // SFFGPU_SEQ_TRACE=<file>: per wave node, pick, iteration, cursor, outcome (empty = off)

  // ---- RRT session
  bool rrt_chain = true;            // SFFGPU_RRT_CHAIN=0: separate batch calls instead of nearest -> steer -> pose -> parent edge -> k nearest as one chain
  bool rrt_fork = true;             // SFFGPU_RRT_FORK=0: the chain's queries on the one stream
  bool rrt_repair = true;           // SFFGPU_RRT_REPAIR=0: slots whose nearest node would be an earlier new point of the wave are not evaluated from it
  bool rrt_dry = true;              // SFFGPU_RRT_DRY=0: edges for every surviving row instead of the rows the replay's walk, done once ahead, takes
  bool rrt_one_chain = true;        // SFFGPU_RRT_ONE_CHAIN=0: the repaired rows as a second chain instead of inside the wave's one chain
  int rrt_split = 2;                // SFFGPU_RRT_SPLIT (>= 1, at most 4 used): an RRT* wave's member edges in that many batches
  int rrt_small = 48;               // SFFGPU_RRT_SMALL (>= 1): a cut wave is followed by 4 x what survived, up to this many slots
  int rrt_grow = 150;               // SFFGPU_RRT_GROW (>= 100): ... or by this percentage of what survived (+ 1)
  bool rrt_no_grid = false;         // SFFGPU_RRT_NO_GRID (set at all): k-nearest by linear sweep
  bool rrt_no_chain_conn = false;   // SFFGPU_RRT_NO_CHAIN_CONN (set at all): Multi-T-RRT, the other trees' query as a call of its own
  bool lazy_batch = false;          // SFFGPU_LAZY_BATCH=1: a lazy_edge session (LazyTSP::runRRT, src/lazy.h:160-284) may be a member of a session batch
                                    // (k_rrt_seq_batch<., true>); 0 = a batch refuses it

  // ---- path smoothing (forests and RRT sessions)
  bool smooth_loop = false;         // SFFGPU_SMOOTH_LOOP=1: sffgpu_forest_smooth_paths / sffgpu_rrt_smooth_paths of a planner created under it walk the
                                    // paths on the device (k_smooth_paths, the batch runner with one member); 0 = the host walk, one edge batch per step
  int smooth_edges = 64;            // SFFGPU_SMOOTH_EDGES (>= 1): most edges one launch of k_smooth_paths tests per path before the host launches again

  // ---- path extraction (forests)
  bool paths_dev = false;           // SFFGPU_PATHS_DEV=1: sffgpu_forest_paths of a forest created under it is sffgpu_forest_paths_batch with one member
                                    // (k_paths_batch where the forest's state is on the device); 0 = sync_host + the host's getPaths / getAllPaths
  int test_paths_cap = 0;           // SFFGPU_TEST_PATHS_CAP=n (>= 1), tests: plan entries of the forest's pool on the device (0 = unset: 8192)

  static Knobs from_env();
};

}  // namespace sff
