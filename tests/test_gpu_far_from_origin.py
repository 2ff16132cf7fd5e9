"""Far from the origin: every engine against the CPU oracle in worlds moved to |coordinate| ~ 2^20 .. 2^22.

Every fp32 fast path of the library (the superset filters of the query kernels, the cube gathers of the SFF* k-nearest
kernels, sq_knn and the ball queries of the one-slot loops and of k_rrt_seq_batch, k_rrt_mates' x filter, k_knn_grid_wg
inside Ctx::rrt_chain, the fp32 cell placement of grid_put / grid_coord) is exact only because of slacks that scale with the
largest coordinate in play: Ctx::sweep_eps() = max(store_maxabs, env_maxabs) * 2^-20, the session batches' reach * 2^-20
(Rrt::batch_prepare) and lin_slack (Ctx::build_clearance).  On the shipped maps (|coordinate| < 2 100: an fp32 ulp is 1e-4,
the slack 0.002) nothing could tell a right slack from a wrong or a forgotten one.  Here the whole world - environment mesh,
limits, start points - is moved by SHIFT_A or SHIFT_B (common.scenario(name, shift)); the oracle is fp64 throughout and runs
the moved problem as it is.  Each case builds the oracle object and the library's object from the same moved arrays, runs
both and compares them with the assertions of the unshifted tests: bit-equal fp64 positions, costs and distances, equal
parents, trees, iterations, borders or links, every counter, paths and plans where trees merge.  No tolerances.

Every case also asserts that it is not vacuous: the shift bites (far_and_not_trivial) and the oracle's tree has at least
about half the nodes its run has on the CPU today.

What the file can and cannot catch was measured once with a library whose two magnitude slacks were zero:
test_dense2d_forty_trees_that_meet[B] and the Multi-T-RRT session at wave 1 (both shifts) fail on it; the other cases pass,
because their kernels use the slack to choose cells and re-test the cells' items in fp64 - they guard the placement (node
and query in the same cells at these magnitudes), not the last ulps of the slack."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import common
import test_gpu_forest_batch as FB
import test_gpu_goal_loop as GL
import test_gpu_lazy_batch as LB
import test_gpu_prio_goal_loop as PGL
import test_gpu_prio_loop as PL
import test_gpu_rrt_batch as RB
from test_gpu_device_engine import engine, make
from test_gpu_parity import assert_same_forest

pytestmark = pytest.mark.gpu

# mixed signs and three different exponents
SHIFT_A = (2.0 ** 20, -2.0 ** 21, 2.0 ** 19)
# an fp32 out there is a multiple of 0.5: an eighth of triang's step
SHIFT_B = (2.0 ** 22, 2.0 ** 22, -2.0 ** 22)
SHIFTS = {"A": SHIFT_A, "B": SHIFT_B}
BOTH = pytest.mark.parametrize("at", ["A", "B"])
N_CTX = 8


def shift_of(name, at):
    s = SHIFTS[at]
    return (s[0], s[1], 0.0) if common.SCENARIOS[name][6] == 2 else s      # (a 2-D world stays in z = 0)


@pytest.fixture(scope="module")
def S():
    import space_filling_forest_star_amd as S
    return S


@pytest.fixture(scope="module")
def ctx(S):
    c = S.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool(S):
    cs = [S.Context(0) for _ in range(N_CTX)]
    yield cs
    for c in cs:
        c.close()


_oracle = {}   # (job, shift) -> the oracle forest after its run: computed once, shared by the cases of the job, never advanced again


def oracle_once(key, fo):
    if key not in _oracle:
        fo.run()
        _oracle[key] = fo
    return _oracle[key]


def far_and_not_trivial(so, pos, min_nodes):
    """the oracle grew a tree and asked for neighbours; the library's fp64 node positions are not fp32 numbers - and what an
    fp32 copy of them loses is what it loses at |coordinate| >= 2^19 (ulp 2^-4 and more), not next to the origin (2^-13)"""
    assert so["n_nodes"] > min_nodes and so["nn_queries"] > 0, so
    p = pos[:, :3]
    back = p.astype(np.float32).astype(np.float64)
    assert np.any(back != p)
    assert np.abs(p).max() >= 2.0 ** 19 and np.abs(back - p).max() > 2.0 ** -8


def forest_pair(S, ctx, job, at, name, wave, iters, seed=3, **kw):
    fo, fg = make(S, ctx, name, wave, iters, seed=seed, shift=shift_of(name, at), **kw)
    return oracle_once((job, at), fo), fg


def check_forest(fo, fg, min_nodes):
    assert_same_forest(fo, fg)
    far_and_not_trivial(fo.stats(), fg.nodes()["pos"], min_nodes)


# ---- forests on the round engines -----------------------------------------------------------------------------------------

@BOTH
@pytest.mark.parametrize("env", [dict(), dict(SFFGPU_QUERY="block")], ids=["classify", "query_block"])
def test_triang_forest(S, ctx, at, env):
    """wave 64 on triang: k_query_classify by default, k_query_block under SFFGPU_QUERY=block"""
    fo, fg = forest_pair(S, ctx, "triang64", at, "triang", 64, 4000, **env)
    assert fg.device_engine()
    fg.run()
    check_forest(fo, fg, 400)
    fg.close()


@BOTH
@pytest.mark.parametrize("env", [dict(), dict(SFFGPU_ORDER_MIN_WAVE=64), dict(SFFGPU_QUERY="wide")],
                         ids=["query_block", "spatial_order", "classify"])
def test_dense3d_forest(S, ctx, at, env):
    """wave 256 on dense3d: k_query_block by default, once more with the spatial order of the slots at this small wave, and
    k_query_classify under SFFGPU_QUERY=wide"""
    fo, fg = forest_pair(S, ctx, "dense3d256", at, "dense3d", 256, 8000, **env)
    assert fg.device_engine()
    fg.run()
    check_forest(fo, fg, 700)
    fg.close()


@BOTH
def test_building_forest(S, ctx, at):
    """above 4 096 triangles: the shared exact kernel"""
    fo, fg = forest_pair(S, ctx, "building64", at, "building", 64, 3000)
    fg.run()
    check_forest(fo, fg, 400)
    fg.close()


@BOTH
def test_dense2d_forest_paths_and_smoothing(S, ctx, at):
    """the flat grid; its trees meet, so the root-to-root cost matrix, the plans and smoothPaths' shortcuts - the edge batches
    of paths.cpp - are compared the way test_path_costs_and_plans_match compares them"""
    fo, fg = make(S, ctx, "dense2d", 16, 3000, seed=3, shift=shift_of("dense2d", at))
    fo.run()
    fg.run()
    check_forest(fo, fg, 150)
    assert fo.stats()["n_borders"] > 0
    do = fo.paths()
    dg, conn = fg.paths()
    assert len(conn) >= 3
    finite = do < 1e300
    assert finite.sum() > len(do)
    assert np.array_equal(finite, dg < 1e300)
    assert np.array_equal(do[finite], dg[finite])
    pairs = [(i, j) for i in range(len(do)) for j in range(i + 1, len(do))]
    for i, j in pairs:
        assert np.array_equal(fo.plan(i, j), fg.plan(i, j))
    so, sg = fo.smooth(), fg.smooth()
    assert np.array_equal(so[finite], sg[finite])
    assert np.all(so[finite] <= do[finite] + 1e-9) and np.any(so[finite] < do[finite] - 1e-6)     # (the oracle's own figures)
    for i, j in pairs:
        assert np.array_equal(fo.plan(i, j), fg.plan(i, j))
    assert fo.stats()["collide_calls"] == fg.stats()["collide_calls"]
    fg.close()


@BOTH
def test_dense2d_forty_trees_that_meet(S, ctx, at):
    """The jobs above reach the fp32 filters but leave them little to decide: a same-tree neighbour acts only below the
    parent distance, a whole step-to-tree-distance margin inside the query radius, and in 6-D a neighbour within the radius
    differs in its angles too, so its position is well inside.  What sits AT the radius is a node of another tree in a flat
    world: forty seeded start points on dense2d (the builders above take the map's own four) meet about 600 times in
    6 000 iterations (234 borders), and at SHIFT_B one of those neighbours is less than an fp32 rounding (0.5) inside the
    radius of 100 (counted on the CPU, with the filter's own expression and a slack of zero, beside the oracle's exact
    test).  A library built with Ctx::sweep_eps() = 0 drops it and fails this case at SHIFT_B."""
    from test_gpu_parity import load_world
    import oracle_lib as O
    sc, w = load_world(ctx, "dense2d", shift_of("dense2d", at))
    roots = common.free_roots(w.collide, sc["limits"], 40, seed=3, dim=2)
    kw = dict(dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"], dim=2, max_iterations=6000, wave=16, seed=3)
    fo = O.Forest(w, roots, sc["limits"], **kw)
    with engine(SFFGPU_ENGINE="device"):
        fg = S.Forest(ctx, roots, sc["limits"], **kw)
    fo.run()
    fg.run()
    check_forest(fo, fg, 340)      # (692 nodes on the CPU today)
    assert fo.stats()["n_borders"] > 100
    fg.close()


def test_dense3d_coarse_forest(S, ctx):
    """the 2-D file's distances on the 3-D map (a 100-unit neighbour radius: many neighbours per sample), at SHIFT_B"""
    fo, fg = forest_pair(S, ctx, "coarse64", "B", "dense3d_coarse", 64, 2000)
    fg.run()
    check_forest(fo, fg, 190)      # (396 nodes on the CPU today)
    fg.close()


@BOTH
def test_host_replay_engine(S, ctx, at):
    """SFFGPU_ENGINE=host: the host-replay engine's own query and k-nearest calls"""
    fo, fg = forest_pair(S, ctx, "triang64", at, "triang", 64, 4000, which="host")
    assert not fg.device_engine()
    fg.run()
    check_forest(fo, fg, 400)
    fg.close()


@BOTH
@pytest.mark.parametrize("env", [dict(), dict(SFFGPU_STAR_KNN="lone"), dict(SFFGPU_STAR_TAIL=0)], ids=["default", "knn_lone", "chain"])
def test_triang_sff_star(S, ctx, at, env):
    """SFF* on the device engine: k_star_knn_wg and the passes as one launch by default, k_star_knn under SFFGPU_STAR_KNN=lone,
    one launch per pass under SFFGPU_STAR_TAIL=0"""
    fo, fg = forest_pair(S, ctx, "triang64star", at, "triang", 64, 3000, optimize=True, **env)
    assert fg.device_engine()
    fg.run()
    check_forest(fo, fg, 350)
    sg = fg.stats()
    assert sg["star_rounds"] > 0 and sg["star_members"] > 0 and sg["host_fallback_waves"] == 0, sg
    par = fo.nodes()["parent"]
    assert np.any(par > np.arange(len(par)))      # rewiring really happened
    fg.close()


@BOTH
def test_building_sff_star(S, ctx, at):
    fo, fg = forest_pair(S, ctx, "building64star", at, "building", 64, 3000, optimize=True)
    assert fg.device_engine()
    fg.run()
    check_forest(fo, fg, 400)
    assert fg.stats()["star_rounds"] > 0
    fg.close()


@BOTH
def test_priority_frontier_on_the_device_engine(S, ctx, at):
    fo, fg = FB.member(S, ctx, "triang", 3, 3000, wave=64, n_roots=3, priority_bias=0.95, shift=shift_of("triang", at))
    assert fg.device_engine()
    fo.run()
    fg.run()
    check_forest(fo, fg, 340)      # (693 .. 748 nodes on the CPU today)
    fg.close()


@BOTH
def test_single_goal_on_the_device_engine(S, ctx, at):
    """the first job of test_single_goal_mode_on_the_device_engine, moved"""
    fo, fg = make(S, ctx, "triang", 64, 60000, seed=8, n_roots=2, goal_offset=[12, 8, 5], shift=shift_of("triang", at))
    fo.run()
    fg.run()
    check_forest(fo, fg, 470)      # (953 nodes on the CPU today)
    st = fg.stats()
    assert fg.device_engine() and st["solved"] == 1 and st["n_borders"] >= 1
    assert st["waves"] > st["host_fallback_waves"] >= 1
    fg.close()


# ---- forests of waves of one slot -----------------------------------------------------------------------------------------

@BOTH
@pytest.mark.parametrize("spec", [True, False], ids=["k_spec_waves", "k_seq_waves"])
@pytest.mark.parametrize("name,iters,optimize,min_nodes", [("triang", 800, False, 140), ("triang", 800, True, 140),
                                                           ("dense3d", 600, False, 90), ("dense3d", 600, True, 90)])
def test_waves_of_one_slot(S, ctx, at, spec, name, iters, optimize, min_nodes):
    """plain SFF and SFF* in the default loop (k_spec_waves) and under SFFGPU_SPEC=0 (k_seq_waves)"""
    env = dict() if spec else dict(SFFGPU_SPEC=0)
    fo, fg = forest_pair(S, ctx, ("one_slot", name, optimize), at, name, 1, iters, optimize=optimize, **env)
    fg.run()
    check_forest(fo, fg, min_nodes)      # (280 and 188 nodes on the CPU today)
    sg = fg.stats()
    assert sg["host_fallback_waves"] == 0
    if spec:
        assert sg["spec_committed"] == fo.stats()["iterations"] and sg["spec_steps"] > 0
    else:
        assert sg["spec_steps"] == 0 and sg["sweeps"] == fo.stats()["iterations"]
    fg.close()


@BOTH
def test_priority_loop(S, pool, at):
    """SFFGPU_PRIO_LOOP=1: the smallest triang job of test_gpu_prio_loop.py"""
    job = PL.SINGLE["triang_star"]
    fo, fg = PL.pair(S, pool[0], shift=shift_of("triang", at), **job)
    fg.run()
    PL.ran_in_the_loop(fg, job["iters"])
    check_forest(fo, fg, 420)      # (852 .. 962 nodes on the CPU today)
    fg.close()


@BOTH
def test_goal_loop(S, pool, at):
    """SFFGPU_GOAL_LOOP=1: the smallest triang job of test_gpu_goal_loop.py"""
    job = dict(GL.LONE["triang_2roots"][0], seed=8, iters=60000, offset=GL.GOAL_OFF["triang"])
    fo, fg = GL.pair(S, pool[0], shift=shift_of("triang", at), **job)
    fg.run()
    so = fo.stats()
    assert so["solved"] == 1 and so["n_borders"] == 1
    GL.ran_in_the_loop(fg, so["iterations"])
    check_forest(fo, fg, 200)      # (414 nodes on the CPU today)
    fg.close()


@BOTH
@pytest.mark.parametrize("case,min_nodes", [("triang_2roots", 80), ("dense2d_2roots", 50)])
def test_priority_goal_loop(S, pool, at, case, min_nodes):
    """SFFGPU_PRIO_GOAL_LOOP=1: the smallest triang job of test_gpu_prio_goal_loop.py and its first dense2d job"""
    job = dict(dict(seed=8, iters=60000), **PGL.LONE[case][0])
    fo, fg = PGL.pair(S, pool[0], shift=shift_of(job["name"], at), **job)
    fg.run()
    so = fo.stats()
    assert so["solved"] == 1 and so["n_borders"] == 1
    PGL.ran_in_the_loop(fg, so["iterations"])
    check_forest(fo, fg, min_nodes)      # (167 and 103 nodes on the CPU today)
    fg.close()


def test_forest_batch_of_every_kind_at_both_shifts(S, pool):
    """eight members of 6 000 iterations in one call: plain SFF, SFF* and the three knobs, at both shifts inside the batch"""
    def m(i, name, at, seed, **kw):
        return FB.member(S, pool[i], name, seed, 6000, shift=shift_of(name, at), **kw)

    pairs = [m(0, "dense3d", "A", 100),
             m(1, "triang", "B", 300),
             m(2, "triang", "A", 301, optimize=True),
             m(3, "building", "B", 600, optimize=True),
             m(4, "triang", "A", 32, n_roots=4, optimize=True, priority_bias=0.95, SFFGPU_PRIO_LOOP=1),
             m(5, "triang", "B", 8, n_roots=2, goal_offset=[12, 8, 5], SFFGPU_GOAL_LOOP=1),
             m(6, "triang", "A", 8, n_roots=2, goal_offset=[57, -5, -20], priority_bias=0.95, SFFGPU_PRIO_GOAL_LOOP=1),
             m(7, "dense2d", "B", 8, n_roots=2, goal_offset=[-60, -1270, 0], priority_bias=0.95, SFFGPU_PRIO_GOAL_LOOP=1)]
    fos, fgs = [p[0] for p in pairs], [p[1] for p in pairs]
    todo = [fo for fo in fos if fo.stats()["iterations"] == 0]      # (member() has run - and keeps - the plain ones)
    with ThreadPoolExecutor(len(todo)) as ex:
        list(ex.map(lambda fo: fo.run(), todo))
    S.run_batch(fgs)
    # (on the CPU today: 1 312, 1 360, 1 355, 1 540 and 1 572 nodes for the members that run 6 000 iterations; 414, 167 and
    # 103 for the goal members, which end when they are solved)
    for i, (fo, fg, min_nodes) in enumerate(zip(fos, fgs, (650, 650, 650, 650, 650, 200, 80, 50))):
        st = fg.stats()
        assert st["batch_launches"] >= 1 and st["spec_steps"] == 0 and st["host_fallback_waves"] == 0, (i, st)
        try:
            check_forest(fo, fg, min_nodes)
        except AssertionError as e:
            raise AssertionError("member %d: %s" % (i, e))
    assert all(fo.stats()["solved"] == 1 for fo in fos[5:])
    fps = [fg.fingerprint() for fg in fgs]
    assert len(set(fps)) == len(fps)
    FB.close_all(fgs)


# ---- RRT sessions ---------------------------------------------------------------------------------------------------------

RRT_JOBS = {
    # job -> (arguments of test_gpu_rrt_batch.member, the oracle's n_nodes lower bound, does the oracle merge trees)
    "multi_t_triang": (dict(name="triang", seed=3, iters=1500, n_roots=4), 250, True),
    "rrt_star_goal_triang": (dict(name="triang", seed=3, iters=600, optimize=True, goal=True, bias=0.1), 100, True),
    "rrt_star_dense3d": (dict(name="dense3d", seed=3, iters=1500, optimize=True), 30, False),
    "rrt_dense2d": (dict(name="dense2d", seed=3, iters=800, n_roots=3), 80, True),
}


def session_pair(S, ctx, job, at, **how):
    spec, min_nodes, merges = RRT_JOBS[job]
    ro, rg = RB.member(S, ctx, shift=shift_of(spec["name"], at), **dict(spec, **how))
    return oracle_once(("rrt", job, at), ro), rg, min_nodes, merges


def check_session(ro, rg, min_nodes, merges=False):
    RB.assert_same_session(ro, rg, min_nodes)
    far_and_not_trivial(ro.stats(), rg.nodes()["pos"], min_nodes)
    if merges:
        assert ro.stats()["merges"] > 0 and rg.stats()["merges"] > 0


@BOTH
@pytest.mark.parametrize("job", sorted(RRT_JOBS))
def test_rrt_session_at_the_default_wave(S, ctx, at, job):
    """adaptive speculative waves: Ctx::rrt_chain with k_rrt_mates, k_rrt_steer and k_knn_grid_wg"""
    ro, rg, min_nodes, merges = session_pair(S, ctx, job, at)
    rg.run()
    assert rg.stats()["waves"] < ro.stats()["iterations"]
    check_session(ro, rg, min_nodes, merges)
    rg.close()


@BOTH
@pytest.mark.parametrize("how", ["wave_1", "no_grid"])
def test_multi_t_rrt_one_by_one_and_without_the_grid(S, ctx, at, how):
    """wave = 1 (one iteration per round trip; wave = 0 is the default, above) and SFFGPU_RRT_NO_GRID=1 (k-nearest by sweep)"""
    with engine(**(dict(SFFGPU_RRT_NO_GRID=1) if how == "no_grid" else dict())):
        ro, rg, min_nodes, merges = session_pair(S, ctx, "multi_t_triang", at, wave=(1 if how == "wave_1" else 0))
    rg.run()
    check_session(ro, rg, min_nodes, merges)
    rg.close()


def grid_walk(name, at, n_tree):
    """the cells a nearest-node query of rrt_seq_body would walk for a tree of n_tree nodes (rrt_seq_batch.inc: the cube of
    cells up to the tree's typical node spacing; the query sweeps the store instead while this is not below the node count),
    from the session's grid: cells of 1.01 * max(step, tree distance) over the limits (Rrt::Rrt, Ctx::grid_setup)"""
    sc = common.scenario(name, shift_of(name, at))
    cell = 1.01 * max(sc["sampling_dist"], sc["dist_tree"])
    lim = sc["limits"]
    n = [int(np.floor((lim[2 * a + 1] - lim[2 * a]) / cell)) + 1 for a in range(3)]
    per = np.float32(n[0]) * np.float32(n[1]) * np.float32(n[2]) / np.float32(max(n_tree, 1))
    w = np.float32(2.0) * (np.cbrt(per) if n[2] > 1 else np.sqrt(per)) + np.float32(3.0)
    return float(w * w * w if n[2] > 1 else w * w)


def test_session_batch_of_every_kind_at_both_shifts(S, pool):
    """eight members in one call, both template instances of k_rrt_seq_batch (RRT / RRT*), both shifts.

    rrt_seq_body answers a nearest-node query from the grid (sq_knn) or by a sweep of the store (rrt_knn_sweep), whichever
    looks cheaper for the tree's size against the grid's cells; both ran here, which grid_walk() shows on the oracle's
    figures: member 1 (dense3d, 300 iterations, a few dozen nodes) stays below the walk's cost to its end, so every query
    of it sweeps - as do those of member 0, dense3d at 3 000 iterations, whose 2 415 nodes stay below the ~3 500 at which
    that map's 786 000 cells would pay - while member 2 (one tree on triang's 32 000 cells, 1 278 nodes) crosses over at
    about 850 nodes and the trees of member 6 (dense2d, 462 cells) within their first few dozen."""
    specs = [dict(name="dense3d", seed=100, iters=3000), dict(name="dense3d", seed=7, iters=300),
             dict(name="triang", seed=5, iters=1500),
             dict(name="dense3d", seed=201, iters=1500, optimize=True),
             dict(name="triang", seed=3, iters=1500, n_roots=4), dict(name="triang", seed=4, iters=1500, n_roots=4),
             dict(name="dense2d", seed=3, iters=800, n_roots=3),
             dict(name="triang", seed=3, iters=600, optimize=True, goal=True, bias=0.1)]
    ats = ["A", "B", "B", "B", "A", "B", "B", "A"]
    pairs = [RB.member(S, pool[i], shift=shift_of(sp["name"], at), **sp) for i, (sp, at) in enumerate(zip(specs, ats))]
    ros, rgs = [p[0] for p in pairs], [p[1] for p in pairs]
    RB.run_oracles(ros)
    n = [ro.stats()["n_nodes"] for ro in ros]
    # (a walk for a tree of t nodes is compared with the n nodes of the store; one tree: t = n, and the walk falls as t grows)
    assert grid_walk("dense3d", "B", 1) >= 1 and grid_walk("dense3d", "B", n[1]) >= n[1]          # sweeps from start to end
    assert grid_walk("dense3d", "A", n[0]) >= n[0]
    assert grid_walk("triang", "B", 1) >= 1 and grid_walk("triang", "B", n[2]) < n[2]            # sweeps first, the grid later
    # (three trees: the largest holds a third of the store at least)
    assert grid_walk("dense2d", "B", 1) >= 3 and grid_walk("dense2d", "B", n[6] // 3) < n[6]
    S.run_rrt_batch(rgs)
    for sp, ro, rg in zip(specs, ros, rgs):
        so, st = ro.stats(), rg.stats()
        assert st["iterations"] == so["iterations"] and st["batch_launches"] >= 1 and st["waves"] == 0 and st["speculated"] == 0, (sp, st)
        assert st["batch_host_iterations"] <= st["merges"] + st["iterations"] // 100, (sp, st)
    # (on the CPU today: 2 415, 24, 1 278, 1 114, 538, 500, 163 and 210 nodes)
    for i, (ro, rg, min_nodes) in enumerate(zip(ros, rgs, (1200, 10, 600, 500, 250, 250, 80, 100))):
        try:
            check_session(ro, rg, min_nodes, merges=i in (4, 5, 6, 7))
        except AssertionError as e:
            raise AssertionError("member %d: %s" % (i, e))
    RB.close_all(rgs)


@BOTH
def test_lazy_edges_in_a_session_batch(S, pool, at):
    """SFFGPU_LAZY_BATCH=1: the tour of test_gpu_lazy_batch.py - its smallest edge set, RRT and RRT* -, moved"""
    sh = shift_of("dense2d", at)
    pairs = [LB.lazy_member(S, pool[i], jb, shift=sh) for i, jb in enumerate(LB.TOUR)]
    ros, rgs = [p[0] for p in pairs], [p[1] for p in pairs]
    with ThreadPoolExecutor(len(ros)) as ex:
        list(ex.map(lambda ro: ro.run(), ros))
    # the oracle's figures do not move with the world (what moves is only where roundings fall, and none of them flips here)
    LB.assert_tour_oracles(ros)
    S.run_rrt_batch(rgs)
    LB.in_one_launch(rgs)
    LB.check_all(ros, rgs)
    for ro, rg in zip(ros, rgs):
        far_and_not_trivial(ro.stats(), rg.nodes()["pos"], 70)      # (143 .. 582 nodes)
    LB.close_all(rgs)
