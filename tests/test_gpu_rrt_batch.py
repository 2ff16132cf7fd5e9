"""Session batches (sffgpu_rrt_run_batch / S.run_rrt_batch): N independent RRT / RRT* / Multi-T-RRT sessions, each on a
context of its own, advanced together - one wavefront per session, one launch of k_rrt_seq_batch per kind for all of them.
Every member is compared with the CPU oracle's run of the same seed the way test_gpu_parity.test_rrt_identical compares
(every key of the oracle's statistics, every array of its nodes and links, paths and plans where trees can merge); the last
test compares the batch with the library's own single-session paths."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import common
import oracle_lib as O
from test_gpu_parity import load_world

pytestmark = pytest.mark.gpu

N_CTX = 32


@pytest.fixture(scope="module")
def S():
    import space_filling_forest_star_amd as S
    return S


@pytest.fixture(scope="module")
def pool(S):
    cs = [S.Context(0) for _ in range(N_CTX)]
    yield cs
    for c in cs:
        c.close()


def member(S, ctx, name, seed, iters, optimize=False, n_roots=1, goal=False, bias=0.0, wave=0, lazy_edge=False, run_oracle=True,
           shift=None):
    """one member on ITS context, built the way test_rrt_identical builds a session: the map's own points where it has
    some, free roots of the member's seed otherwise; the oracle of the same job is created, not yet run (run_oracles)"""
    sc, w = load_world(ctx, name, shift)
    pts = sc["xml_points"] if sc["xml_points"] is not None else common.free_roots(w.collide, sc["limits"], max(6, n_roots), seed=seed,
                                                                                 dim=sc["dim"])
    roots = pts[:n_roots]
    kw = dict(dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"], dim=sc["dim"], optimize=optimize,
              goal=pts[4] if (goal or lazy_edge) else None, priority_bias=bias, max_iterations=iters, seed=seed, lazy_edge=lazy_edge)
    ro = O.Rrt(w, roots, sc["limits"], **kw) if run_oracle else None
    rg = S.Rrt(ctx, roots, sc["limits"], wave=wave, **kw)
    rg.n_trees = n_roots + (1 if goal else 0)
    return ro, rg


def run_oracles(ros):
    """the oracles of a batch, each with a world of its own, on up to 16 threads (the calls release the interpreter lock)"""
    todo = [ro for ro in ros if ro is not None]
    if todo:
        with ThreadPoolExecutor(min(16, len(todo))) as ex:
            list(ex.map(lambda ro: ro.run(), todo))


def build(S, pool, specs):
    assert len(specs) <= len(pool)
    pairs = [member(S, pool[i], **sp) for i, sp in enumerate(specs)]
    run_oracles([p[0] for p in pairs])
    return [p[0] for p in pairs], [p[1] for p in pairs]


def assert_same_session(ro, rg, min_nodes=30):
    so, sg = ro.stats(), rg.stats()
    assert so["n_nodes"] > min_nodes
    for k in so:
        assert so[k] == sg[k], (k, so[k], sg[k])
    no, ng = ro.nodes(), rg.nodes()
    for k in no:
        assert np.array_equal(no[k], ng[k]), k            # (bit-exact fp64 positions, costs, parent distances)
    lo, lg = ro.links(), rg.links()
    for k in lo:
        assert np.array_equal(lo[k], lg[k]), k
    nt = rg.n_trees
    if nt > 1:
        do, co = ro.paths(nt)
        dg, cg = rg.paths(nt)
        assert co == len(cg) and np.array_equal(do, dg)
        for a in range(nt):
            for b in range(a + 1, nt):
                assert np.array_equal(ro.plan(a, b), rg.plan(a, b))


def check_all(ros, rgs, min_nodes=30):
    for i, (ro, rg) in enumerate(zip(ros, rgs)):
        try:
            assert_same_session(ro, rg, min_nodes)
        except AssertionError as e:
            raise AssertionError("member %d: %s" % (i, e))


def close_all(rgs):
    for rg in rgs:
        rg.close()


def test_batch_rrt(S, pool):
    ros, rgs = build(S, pool, [dict(name="dense3d", seed=s, iters=3000) for s in range(100, 132)])
    S.run_rrt_batch(rgs)
    for rg in rgs:
        st = rg.stats()
        assert st["iterations"] == 3000
        assert st["batch_launches"] >= 1 and st["waves"] == 0 and st["speculated"] == 0 and st["batch_host_iterations"] == 0, st
    check_all(ros, rgs)
    assert len({rg.stats()["collide_calls"] for rg in rgs}) > 16, "the members of the batch are the same session"
    close_all(rgs)


def test_batch_rrt_star(S, pool):
    specs = [dict(name="dense3d", seed=s, iters=1500, optimize=True) for s in range(200, 216)]
    specs += [dict(name="building", seed=s, iters=500, optimize=True) for s in range(3, 7)]
    ros, rgs = build(S, pool, specs)
    S.run_rrt_batch(rgs)
    rewired = 0
    for sp, rg in zip(specs, rgs):
        st = rg.stats()
        assert st["iterations"] == sp["iters"]
        assert st["batch_launches"] >= 1 and st["waves"] == 0 and st["speculated"] == 0, st
        par = rg.nodes()["parent"]
        rewired += int(np.any(par > np.arange(len(par))))       # a node whose parent is younger than itself was rewired
    assert rewired >= 1
    check_all(ros, rgs)
    close_all(rgs)


def test_batch_mixed_environments_kinds_and_lengths(S, pool):
    """different maps and robots (LDS sizes), both template instances, trees that merge, a goal with bias, a member that ends early"""
    specs = [dict(name="triang", seed=3, iters=1500, n_roots=4),           # Multi-T-RRT: trees merge until one is left
             dict(name="dense3d", seed=3, iters=6000, n_roots=10),
             dict(name="dense2d", seed=3, iters=800, n_roots=3),
             dict(name="dense3d_coarse", seed=3, iters=700, n_roots=5),
             dict(name="triang", seed=3, iters=600, optimize=True, goal=True, bias=0.1),
             dict(name="dense3d", seed=7, iters=300)]
    ros, rgs = build(S, pool, specs)
    S.run_rrt_batch(rgs)
    for sp, ro, rg in zip(specs, ros, rgs):
        so, st = ro.stats(), rg.stats()
        print(sp, "merges", st["merges"], "host iterations", st["batch_host_iterations"], "launches", st["batch_launches"])
        assert st["iterations"] == so["iterations"] and st["batch_launches"] >= 1 and st["waves"] == 0 and st["speculated"] == 0, (sp, st)
        if so["merges"] > 0:
            assert st["merges"] > 0
        # the hand-over may not carry the run: link + merge iterations (merges <= trees - 1) and the odd tie or capacity
        assert st["batch_host_iterations"] <= st["merges"] + st["iterations"] // 100, (sp, st)
    assert ros[0].stats()["merges"] > 0 and ros[0].stats()["n_live_trees"] == 1
    # (min_nodes guards against a job that grows nothing; it is a statement about the ORACLE's tree.  The member that ends
    # early runs 300 iterations in a cluttered map, a tenth of test_batch_rrt's budget: a tenth of its bound of 30, rounded up
    # to "more than a handful", is what can be asked of it)
    check_all(ros, rgs, min_nodes=5)
    close_all(rgs)


def test_batch_staged_with_getters_and_a_member_advanced_alone(S, pool):
    specs = [dict(name="dense3d", seed=s, iters=1500, optimize=(s % 2 == 1)) for s in range(100, 106)]
    specs += [dict(name="triang", seed=3, iters=1500, n_roots=4), dict(name="dense3d", seed=3, iters=1500, n_roots=5)]
    ros, rgs = build(S, pool, specs)
    calls = 0
    while True:
        before = [rg.stats()["iterations"] for rg in rgs] if calls == 0 else after
        S.run_rrt_batch(rgs, max_iterations=97)
        calls += 1
        for rg in (rgs[1], rgs[6]):
            assert len(rg.nodes()["parent"]) == rg.stats()["n_nodes"]
            rg.links()
        after = [rg.stats()["iterations"] for rg in rgs]
        assert all(0 <= a - b <= 97 for a, b in zip(after, before))
        if after == before:
            break
        if calls == 2:
            i0 = rgs[3].stats()["iterations"]
            rgs[3].run(50)                       # one member alone, on the single-session path, in between
            assert rgs[3].stats()["iterations"] == i0 + 50
            after[3] = i0 + 50
    assert calls > 3
    check_all(ros, rgs)
    snap = [(rg.stats()["rng_draws"], rg.stats()["n_nodes"], rg.stats()["collide_calls"], rg.stats()["batch_launches"]) for rg in rgs]
    S.run_rrt_batch(rgs)                         # nothing left to do
    assert [(rg.stats()["rng_draws"], rg.stats()["n_nodes"], rg.stats()["collide_calls"], rg.stats()["batch_launches"]) for rg in rgs] == snap
    check_all(ros, rgs)
    close_all(rgs)


def test_batch_refusals_leave_a_bystander_alone(S, pool):
    ro, by = member(S, pool[0], name="dense3d", seed=100, iters=1500)
    ro.run()
    by.run(60)
    keys = ("iterations", "n_nodes", "collide_calls", "path_free_calls", "nn_queries", "rng_draws", "batch_launches", "waves")

    def state():
        n = by.nodes()
        return tuple(by.stats()[k] for k in keys), n["pos"].tobytes(), n["parent"].tobytes(), n["cost"].tobytes()

    st0 = state()

    def refused(others):
        with pytest.raises(S.SffGpuError):
            S.run_rrt_batch([by] + others)
        assert state() == st0
        with pytest.raises(S.SffGpuError):
            S.run_rrt_batch(others + [by])
        assert state() == st0

    _, lazy = member(S, pool[1], name="dense3d", seed=101, iters=1500, lazy_edge=True, run_oracle=False)
    refused([lazy])
    lazy.close()
    _, a = member(S, pool[2], name="dense3d", seed=101, iters=1500, run_oracle=False)
    _, b = member(S, pool[2], name="dense3d", seed=102, iters=1500, run_oracle=False)      # (the same context: it took a's store)
    refused([a, b])
    a.close()
    refused([b, b])                                                        # the same session twice
    refused([by])
    refused([None])                                                        # NULL
    L = S.lib()
    assert L.sffgpu_rrt_run_batch(None, 0, 0, None) == -1
    # ... and the bystander is still a member like any other
    S.run_rrt_batch([by, b])
    assert by.stats()["batch_launches"] >= 1
    assert_same_session(ro, by)
    close_all([by, b])


def test_batch_error_names_the_member_it_came_from(S, pool):
    """a host-side refusal inside the lock step (Rrt::batch_upload: the context's store is another session's) carries the
    index of the member it came from, wherever that member stands, and leaves the other member as it was"""
    ro, by = member(S, pool[0], name="dense3d", seed=100, iters=1500)
    ro.run()
    by.run(60)
    keys = ("iterations", "n_nodes", "collide_calls", "path_free_calls", "nn_queries", "rng_draws", "batch_launches", "waves")

    def state():
        n = by.nodes()
        return tuple(by.stats()[k] for k in keys), n["pos"].tobytes(), n["parent"].tobytes(), n["cost"].tobytes()

    st0 = state()
    _, a = member(S, pool[1], name="dense3d", seed=101, iters=1500, run_oracle=False)
    a.run(60)
    assert a.stats()["n_nodes"] > 1                                        # (more nodes than its roots)
    _, b = member(S, pool[1], name="dense3d", seed=102, iters=1500, run_oracle=False)      # (the same context: it took a's store)
    for members, idx in (([by, a], 1), ([a, by], 0)):
        with pytest.raises(S.SffGpuError) as e:
            S.run_rrt_batch(members)
        print(e.value)
        assert "member %d" % idx in str(e.value) and "node store is not this session's" in str(e.value), str(e.value)
    assert state() == st0
    a.close()
    S.run_rrt_batch([by, b])
    assert by.stats()["batch_launches"] >= 1
    assert_same_session(ro, by)
    close_all([by, b])


def test_batch_equals_the_sessions_run_alone(S, pool):
    """the three paths of this library on the same eight jobs: k_rrt_seq_batch, the one-by-one host loop, speculative waves"""
    keys = ("iterations", "solved", "n_nodes", "n_live_trees", "merges", "n_links", "collide_calls", "path_free_calls",
            "nn_queries", "rng_draws", "lazy_distance")
    specs = [dict(name="dense3d", seed=s, iters=1200, optimize=(s % 2 == 0), n_roots=(3 if s >= 306 else 1)) for s in range(300, 308)]
    res = []
    for how in ("batch", 1, 0):
        _, rgs = build(S, pool, [dict(sp, wave=(0 if how == "batch" else how), run_oracle=False) for sp in specs])
        if how == "batch":
            S.run_rrt_batch(rgs)
            assert all(rg.stats()["batch_launches"] >= 1 and rg.stats()["waves"] == 0 for rg in rgs)
        else:
            for rg in rgs:
                rg.run()
            assert all(rg.stats()["batch_launches"] == 0 for rg in rgs)
        out = []
        for rg in rgs:
            n, l, st = rg.nodes(), rg.links(), rg.stats()
            out.append((tuple(st[k] for k in keys), tuple(n[k].tobytes() for k in sorted(n)), tuple(l[k].tobytes() for k in sorted(l))))
        res.append(out)
        close_all(rgs)
    assert res[0] == res[1], "batch against wave = 1"
    assert res[0] == res[2], "batch against wave = 0"
    assert len({r[0] for r in res[0]}) == 8 and all(r[0][2] > 40 for r in res[0])
