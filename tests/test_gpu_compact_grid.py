"""The compact node grid (SFFGPU_COMPACT_GRID=1 at sffgpu_create_member; DESIGN.md section 3, "Compact node grid"): only the
cells that hold a node have a bucket, the buckets come from a pool as large as the node store.  The one-wavefront loops -
forest batches, session batches - work on it; everything else makes the grid dense first.  One world (dense3d) is uploaded
once; compact members, dense members (created without the knob) and the CPU oracle run the same jobs, and every comparison
is bit-equal fp64 (assert_same_forest / assert_same_session), as in test_gpu_ctx_member.py."""
import numpy as np
import pytest

import common
import oracle_lib as O
from test_gpu_device_engine import engine
from test_gpu_parity import assert_same_forest, load_world
from test_gpu_rrt_batch import assert_same_session, run_oracles

pytestmark = pytest.mark.gpu

N_EACH = 6
KNOB = dict(SFFGPU_COMPACT_GRID=1)


@pytest.fixture(scope="module")
def S():
    import space_filling_forest_star_amd as S
    return S


def compact_member(owner):
    with engine(**KNOB):     # (read by sffgpu_create_member, and never after)
        return owner.member()


@pytest.fixture(scope="module")
def world(S):
    """dense3d uploaded ONCE: the owner, six members created under the knob and six created without it"""
    owner = S.Context(0)
    load_world(owner, "dense3d")
    compact = [compact_member(owner) for _ in range(N_EACH)]
    dense = [owner.member() for _ in range(N_EACH)]
    yield dict(owner=owner, compact=compact, dense=dense)
    for c in compact + dense + [owner]:
        c.close()


_oracle = {}   # job -> the oracle forest after its run: computed once, shared, never advanced again


def forest(S, ctx, name="dense3d", seed=100, iters=600, optimize=False, wave=1, n_roots=5, goal_offset=None, priority_bias=0.0,
           oracle=True, **env):
    """(the oracle after its run - or None -, the library's forest before its first wave) on a context that already holds
    the scenario's meshes (its own, or its owner's): test_gpu_forest_batch.member without the upload"""
    sc = common.scenario(name)
    w = O.World(sc["env"], sc["robot"], O.TRIG_PORTABLE)
    roots = common.free_roots(w.collide, sc["limits"], n_roots, seed=seed, dim=sc["dim"])
    kw = dict(dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"], dim=sc["dim"], max_iterations=iters,
              wave=wave, seed=seed, optimize=optimize, priority_bias=priority_bias)
    if goal_offset is not None:
        g = roots[0].copy()
        g[:3] += np.array(goal_offset, dtype=np.float64)
        kw["goal"] = g
    key = (name, seed, iters, optimize, wave, n_roots, None if goal_offset is None else tuple(goal_offset), priority_bias)
    fo = None
    if oracle:
        if key not in _oracle:
            _oracle[key] = O.Forest(w, roots, sc["limits"], **kw)
            _oracle[key].run()
        fo = _oracle[key]
    with engine(SFFGPU_ENGINE="device", **env):
        fg = S.Forest(ctx, roots, sc["limits"], **kw)
    return fo, fg


def session(S, ctx, seed, iters, optimize=False, n_roots=1, lazy=False, name="dense3d"):
    """test_gpu_ctx_member.session (dense3d_coarse: the same two meshes, longer steps), and a lazy edge (root = point 0,
    goal = point 4) created under SFFGPU_LAZY_BATCH=1"""
    sc = common.scenario(name)
    w = O.World(sc["env"], sc["robot"], O.TRIG_PORTABLE)
    pts = common.free_roots(w.collide, sc["limits"], max(6, n_roots), seed=seed, dim=sc["dim"])
    kw = dict(dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"], dim=sc["dim"], optimize=optimize,
              goal=pts[4] if lazy else None, priority_bias=0.0, max_iterations=iters, seed=seed, lazy_edge=lazy)
    ro = O.Rrt(w, pts[:n_roots], sc["limits"], **kw)
    with engine(SFFGPU_LAZY_BATCH=1 if lazy else 0):
        rg = S.Rrt(ctx, pts[:n_roots], sc["limits"], wave=0, **kw)
    rg.n_trees = n_roots
    return ro, rg


def same_results(fa, fb):
    """two forests of the library: what assert_same_forest compares between a forest and its oracle"""
    assert fa.fingerprint() == fb.fingerprint()
    na, nb = fa.nodes(), fb.nodes()
    for k in ("parent", "tree", "iter", "pos", "cost", "dpar"):
        assert np.array_equal(na[k], nb[k]), k
    ba, bb = fa.borders(), fb.borders()
    for k in ba:
        assert np.array_equal(ba[k], bb[k]), k
    sa, sb = fa.stats(), fb.stats()
    for k in ("iterations", "solved", "n_nodes", "n_trees", "frontier_size", "closed_size", "n_connected", "n_borders",
              "collide_calls", "path_free_calls", "nn_queries", "waves"):
        assert sa[k] == sb[k], (k, sa[k], sb[k])


def close_all(xs):
    for x in xs:
        x.close()


BATCH_JOBS = [dict(seed=s, iters=600) for s in range(100, 104)] + [dict(seed=s, iters=600, optimize=True) for s in (200, 201)]


# ------------------------------------------------------------------------------------------------ 1. memory
def test_memory_of_a_compact_member(S):
    """The bound is worked out from the job, not taken from the grid code: cells from the limits and the cell edge
    (1.01 x the larger of the two planner distances; the library adds a few fp32 ulps, which can only make cells fewer),
    8 items per bucket, the overflow list's 65 536 entries, the store's capacity from store_bytes (76 B per node: six fp32
    columns, the tree id, the fp64 position).  Pool buckets are not visible from outside: the bound takes the most the
    pool may have, the store's capacity + 12.5 %."""
    sc = common.scenario("dense3d")
    owner = S.Context(0)
    load_world(owner, "dense3d")
    a, b = compact_member(owner), compact_member(owner)
    plain = owner.member()
    assert owner.grid_compact() == 0 and plain.grid_compact() == 0
    assert a.grid_compact() == 1 and b.grid_compact() == 1
    fo, fg = forest(S, a, **BATCH_JOBS[0])
    _, ft = forest(S, plain, **BATCH_JOBS[0])
    m, mp = a.memory(), plain.memory()
    print("compact member with a forest:", m)
    print("dense member with the same forest:", mp)
    lim = sc["limits"]
    cell = 1.01 * max(sc["sampling_dist"], sc["dist_tree"])
    cells = 1
    for ax in range(3):
        cells *= int(np.floor((lim[2 * ax + 1] - lim[2 * ax]) / cell)) + 1
    bk, ovf_cap = 8, 65536
    assert m["store_bytes"] % 76 == 0
    store_cap = m["store_bytes"] // 76
    assert store_cap >= 4096
    pool = store_cap + store_cap // 8
    bound = 8 * cells + 64 * bk * pool + 64 * ovf_cap + 64
    print("cells %d, store capacity %d, bound %d, grid_bytes %d (dense %d)" % (cells, store_cap, bound, m["grid_bytes"], mp["grid_bytes"]))
    assert a.grid_compact() == 1 and m["round_grid_bytes"] == 0
    assert 0 < m["grid_bytes"] <= bound
    assert m["store_bytes"] == mp["store_bytes"]
    assert 10 * m["grid_bytes"] < mp["grid_bytes"]
    assert b.memory()["grid_bytes"] == 0 and b.grid_compact() == 1        # (a grid comes with the first forest)
    S.run_batch([fg, ft])
    assert_same_forest(fo, fg)
    assert_same_forest(fo, ft)
    after = a.memory()
    assert after["grid_bytes"] == m["grid_bytes"] and after["round_grid_bytes"] == 0 and a.grid_compact() == 1
    close_all([fg, ft, a, b, plain, owner])


# ------------------------------------------------------------------------------------------------ 2. forest batch
def test_forest_batch_on_compact_members(S, world):
    pairs = [forest(S, c, **job) for c, job in zip(world["compact"], BATCH_JOBS)]
    twins = [forest(S, c, **job)[1] for c, job in zip(world["dense"], BATCH_JOBS)]
    fgs = [p[1] for p in pairs]
    S.run_batch(fgs + twins)
    for (fo, fg), tw in zip(pairs, twins):
        st = fg.stats()
        assert st["batch_launches"] >= 1 and st["spec_steps"] == 0 and st["host_fallback_waves"] == 0 and st["grid_rebuilds"] == 0, st
        assert fo.stats()["n_nodes"] > 40
        assert_same_forest(fo, fg)
        same_results(fg, tw)
    assert len({fg.fingerprint() for fg in fgs}) == len(fgs)
    assert [c.grid_compact() for c in world["compact"]] == [1] * N_EACH
    assert [c.grid_compact() for c in world["dense"]] == [0] * N_EACH
    for c in world["compact"]:
        assert c.memory()["round_grid_bytes"] == 0
    close_all(fgs + twins)


# ------------------------------------------------------------------------------------------------ 3. the other kinds
def test_priority_goal_and_priority_goal_members(S, world):
    jobs = [dict(seed=31, iters=600, priority_bias=0.5, SFFGPU_PRIO_LOOP=1),
            dict(seed=32, iters=600, n_roots=4, goal_offset=[30, 25, 8], SFFGPU_GOAL_LOOP=1),
            dict(seed=33, iters=600, n_roots=2, goal_offset=[150, 125, 40], priority_bias=0.95, SFFGPU_PRIO_GOAL_LOOP=1)]
    pairs = [forest(S, c, **job) for c, job in zip(world["compact"], jobs)]
    twins = [forest(S, c, oracle=False, **job)[1] for c, job in zip(world["dense"], jobs)]
    fgs = [p[1] for p in pairs]
    S.run_batch(fgs + twins)
    for (fo, fg), tw in zip(pairs, twins):
        st = fg.stats()
        assert st["batch_launches"] >= 1 and st["spec_steps"] == 0 and st["host_fallback_waves"] == 0, st
        assert st["n_nodes"] > 40
        same_results(fg, tw)
        assert_same_forest(fo, fg)
    assert [c.grid_compact() for c in world["compact"][:3]] == [1, 1, 1]
    close_all(fgs + twins)


# ------------------------------------------------------------------------------------------------ 4. session batch
def test_session_batch_on_compact_members(S, world):
    """RRT, RRT*, a Multi-T-RRT whose trees merge (the merge re-labels nodes: the grid is rebuilt, compact, through the
    multi-threaded insert kernel) and a lazy edge"""
    specs = [dict(seed=7, iters=300), dict(seed=200, iters=600, optimize=True), dict(name="dense3d_coarse", seed=3, iters=700, n_roots=5), dict(seed=5, iters=600, lazy=True)]
    pairs = [session(S, c, **sp) for c, sp in zip(world["compact"], specs)]
    twins = [session(S, c, **sp)[1] for c, sp in zip(world["dense"], specs)]
    run_oracles([p[0] for p in pairs])
    rgs = [p[1] for p in pairs]
    S.run_rrt_batch(rgs + twins)
    for sp, (ro, rg), tw in zip(specs, pairs, twins):
        st, tt = rg.stats(), tw.stats()
        assert st["batch_launches"] >= 1 and st["waves"] == 0, (sp, st)
        for k in ro.stats():
            assert st[k] == tt[k], (sp, k, st[k], tt[k])
        ng, nt = rg.nodes(), tw.nodes()
        for k in ng:
            assert np.array_equal(ng[k], nt[k]), (sp, k)
        if sp.get("lazy"):
            so = ro.stats()
            for k in so:
                assert so[k] == st[k], (k, so[k], st[k])
            assert np.array_equal(ro.lazy_plan(), rg.lazy_plan()) and np.array_equal(tw.lazy_plan(), rg.lazy_plan())
        else:
            assert_same_session(ro, rg, min_nodes=5 if sp["iters"] == 300 else 30)
    assert rgs[2].stats()["merges"] >= 1 and pairs[2][0].stats()["merges"] >= 1
    assert [c.grid_compact() for c in world["compact"][:4]] == [1, 1, 1, 1]
    close_all(rgs + twins)


# ------------------------------------------------------------------------------------------------ 5. edge paths while compact
@pytest.mark.parametrize("env", [dict(SFFGPU_TEST_GRID_POOL=4), dict(SFFGPU_TEST_GRID_BK=1, SFFGPU_TEST_GRID_OVF=16)],
                         ids=["pool_of_four", "one_item_buckets"])
def test_pool_exhaustion_and_recelling_while_compact(S, world, env):
    """a pool of four buckets runs out with the first nodes (the items go to the overflow list, the pool doubles until it
    holds); buckets of one item and a list of sixteen entries re-cell the grid.  SFF and SFF*"""
    pairs = [forest(S, c, **dict(job, **env)) for c, job in zip(world["compact"], (BATCH_JOBS[0], BATCH_JOBS[4]))]
    fgs = [p[1] for p in pairs]
    S.run_batch(fgs)
    for fo, fg in pairs:
        st = fg.stats()
        print(env, "grid_rebuilds", st["grid_rebuilds"], "launches", st["batch_launches"])
        assert st["grid_rebuilds"] > 0 and st["host_fallback_waves"] == 0, st
        assert_same_forest(fo, fg)
    assert [c.grid_compact() for c in world["compact"][:2]] == [1, 1]
    close_all(fgs)


# ------------------------------------------------------------------------------------------------ 6. several roots in one cell
def test_dense2d_forty_trees_on_a_compact_member(S):
    """test_gpu_far_from_origin's forty seeded start points on dense2d, in waves of one slot: roots share cells, so the
    fused insert of the roots' append has several threads opening the same cell's bucket at once"""
    owner = S.Context(0)
    load_world(owner, "dense2d")
    ctx = compact_member(owner)
    fo, fg = forest(S, ctx, name="dense2d", seed=3, iters=600, n_roots=40)
    assert ctx.grid_compact() == 1
    S.run_batch([fg])
    assert fo.stats()["n_borders"] > 0 and fo.stats()["n_nodes"] > 100
    assert_same_forest(fo, fg)
    assert ctx.grid_compact() == 1 and ctx.memory()["round_grid_bytes"] == 0
    close_all([fg, ctx, owner])


# ------------------------------------------------------------------------------------------------ 7. materialisation
def test_a_wave_of_many_slots_makes_the_grid_dense(S, world):
    ctx, plain = world["compact"][4], world["dense"][4]
    job = dict(seed=110, iters=1500, wave=256)
    fo, fg = forest(S, ctx, **job)
    _, tw = forest(S, plain, oracle=False, **job)
    before = ctx.memory()["grid_bytes"]
    assert ctx.grid_compact() == 1               # (not with the forest: with its first wave)
    fg.run()
    tw.run()
    assert_same_forest(fo, fg)
    same_results(fg, tw)
    m = ctx.memory()
    assert ctx.grid_compact() == 0 and m["grid_bytes"] > before and m["round_grid_bytes"] > 0
    assert m["grid_bytes"] >= plain.memory()["grid_bytes"]
    close_all([fg, tw])


def test_the_speculative_kernel_makes_the_grid_dense(S, world):
    """sffgpu_forest_run of a plain wave-1 forest takes k_spec_waves; then a staged run - a batch first, a single run to the
    end - against the run in one piece"""
    owner = world["owner"]
    ctx, ctx2, plain = compact_member(owner), compact_member(owner), world["dense"][5]
    job = BATCH_JOBS[1]
    fo, fg = forest(S, ctx, **job)
    _, tw = forest(S, plain, **job)
    before = ctx.memory()["grid_bytes"]
    fg.run()
    tw.run()
    assert fg.stats()["spec_steps"] > 0
    assert_same_forest(fo, fg)
    same_results(fg, tw)
    assert ctx.grid_compact() == 0 and ctx.memory()["grid_bytes"] > before
    _, staged = forest(S, ctx2, **job)
    S.run_batch([staged], max_waves=150)
    assert staged.stats()["waves"] == 150 and ctx2.grid_compact() == 1
    staged.run()
    assert ctx2.grid_compact() == 0
    assert_same_forest(fo, staged)
    same_results(staged, fg)
    close_all([fg, tw, staged, ctx, ctx2])


def test_nodes_index_and_knn_make_the_grid_dense(S, world):
    owner = world["owner"]
    ctx, plain = compact_member(owner), world["dense"][5]
    sc = common.scenario("dense3d")
    pts = common.random_poses(sc["limits"], 3000, 11)
    tree = (np.arange(len(pts)) % 3).astype(np.int32)
    q = common.random_poses(sc["limits"], 64, 12)
    got = []
    assert ctx.grid_compact() == 1
    before = ctx.memory()["grid_bytes"]
    for c in (ctx, plain):
        c.nodes_reset(len(pts))
        c.nodes_append(pts, tree)
        c.nodes_index(sc["limits"], 1.01 * sc["sampling_dist"])
        got.append(c.knn(q, 8))
    for x, y in zip(got[0], got[1]):
        assert np.array_equal(x, y)
    assert ctx.grid_compact() == 0 and ctx.memory()["grid_bytes"] > before
    ctx.close()


# ------------------------------------------------------------------------------------------------ 8. knob unset
def test_without_the_knob_nothing_changes(S, world):
    owner = world["owner"]
    with engine(SFFGPU_COMPACT_GRID=0):
        off = owner.member()
    a, b = world["dense"][0], off
    assert a.grid_compact() == 0 and b.grid_compact() == 0 and owner.grid_compact() == 0
    fo, fa = forest(S, a, **BATCH_JOBS[0])
    _, fb = forest(S, b, **BATCH_JOBS[0])
    plain = S.Context(0)
    load_world(plain, "dense3d")
    _, fp = forest(S, plain, **BATCH_JOBS[0])
    ma, mb, full = a.memory(), b.memory(), plain.memory()
    # (what test_gpu_ctx_member expects of a member: no round grid, the node grid and store of a plain context)
    assert mb["round_grid_bytes"] == 0 and full["round_grid_bytes"] > 0
    assert mb["grid_bytes"] == full["grid_bytes"] and mb["store_bytes"] == full["store_bytes"]
    assert ma["grid_bytes"] >= mb["grid_bytes"]      # (a has held other forests: capacities never shrink)
    S.run_batch([fa, fb, fp])
    for f in (fa, fb, fp):
        assert_same_forest(fo, f)
    assert a.grid_compact() == 0 and b.grid_compact() == 0
    close_all([fa, fb, fp, off, plain])
