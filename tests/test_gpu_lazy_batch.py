"""Lazy edges (LazyTSP::runRRT, src/lazy.h:160-284: one tree from one root, no tree pick in the engine stream,
k = 2e log10(size + 1), solved when a new node comes within treeDistance of the goal) as members of a session batch
(sffgpu_rrt_run_batch / S.run_rrt_batch, k_rrt_seq_batch<., true>), for sessions created under SFFGPU_LAZY_BATCH=1.
Every case first asserts the CPU oracle's own figures of the job, so that it cannot pass on a job that does nothing, and then
compares every member with the oracle's run of the same job: every key of the oracle's statistics (lazy_distance and the
stream position among them), every node array bit for bit, and the edge's plan."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import common
import oracle_lib as O
from test_gpu_parity import load_world
from test_gpu_rrt_batch import assert_same_session, member as other_member

pytestmark = pytest.mark.gpu

N_CTX = 16
KNOB = "SFFGPU_LAZY_BATCH"
UNSOLVED = 1e300


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


class knob:
    """SFFGPU_LAZY_BATCH for the time a session is created (value None: unset) - it is read then, and never after"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.pop(KNOB, None)
        if self.value is not None:
            os.environ[KNOB] = str(self.value)

    def __exit__(self, *a):
        os.environ.pop(KNOB, None)
        if self.old is not None:
            os.environ[KNOB] = self.old


_oracle = {}   # job -> the oracle session after its run: computed once, shared by the tests that use the job, never advanced again


def job(name, a, b, seed, iters, optimize, skip=0):
    return (name, a, b, seed, iters, bool(optimize), skip)


def lazy_member(S, ctx, jb, on=1, wave=0, shift=None):
    """(the job's oracle - run or not yet, run_oracles -, the library's session before its first iteration) of one lazy edge
    on ITS context: root = point a, goal = point b of the map's own points, else of the free roots test_lazy_edge_rrt_identical uses"""
    name, a, b, seed, iters, optimize, skip = jb
    sc, w = load_world(ctx, name, shift)
    pts = sc["xml_points"] if sc["xml_points"] is not None else common.free_roots(w.collide, sc["limits"], 6, seed=3, dim=sc["dim"])
    kw = dict(goal=pts[b], dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"], dim=sc["dim"], optimize=optimize,
              max_iterations=iters, seed=seed, lazy_edge=True, rng_skip=skip)
    ro = (_oracle.get(jb) if shift is None else None) or O.Rrt(w, pts[a:a + 1], sc["limits"], **kw)
    with knob(on):
        rg = S.Rrt(ctx, pts[a:a + 1], sc["limits"], wave=wave, **kw)
    rg.n_trees = 1
    return ro, rg


def run_oracles(jobs, ros):
    """the oracles that have not run yet, each with a world of its own, on up to 16 threads (the calls release the interpreter lock)"""
    todo = {jb: ro for jb, ro in zip(jobs, ros) if jb not in _oracle}
    if todo:
        with ThreadPoolExecutor(min(16, len(todo))) as ex:
            list(ex.map(lambda ro: ro.run(), todo.values()))
        _oracle.update(todo)
    return [_oracle[jb] for jb in jobs]


def build(S, pool, jobs, **how):
    assert len(jobs) <= len(pool)
    pairs = [lazy_member(S, pool[i], jb, **how) for i, jb in enumerate(jobs)]
    return run_oracles(jobs, [p[0] for p in pairs]), [p[1] for p in pairs]


def assert_same_edge(ro, rg):
    so, sg = ro.stats(), rg.stats()
    for k in so:
        assert so[k] == sg[k], (k, so[k], sg[k])
    no, ng = ro.nodes(), rg.nodes()
    for k in no:
        assert np.array_equal(no[k], ng[k]), k            # (bit-exact fp64 positions, costs, parent distances)
    assert np.array_equal(ro.lazy_plan(), rg.lazy_plan())


def check_all(ros, rgs):
    for i, (ro, rg) in enumerate(zip(ros, rgs)):
        try:
            assert_same_edge(ro, rg)
        except AssertionError as e:
            raise AssertionError("member %d: %s" % (i, e))


def in_one_launch(rgs):
    for rg in rgs:
        st = rg.stats()
        assert st["batch_launches"] == 1 and st["waves"] == 0 and st["speculated"] == 0 and st["batch_host_iterations"] == 0, st


def close_all(rgs):
    for rg in rgs:
        rg.close()


def figures(ro):
    s = ro.stats()
    return s["solved"], s["iterations"], s["n_nodes"], s["rng_draws"]


def rewired(nodes):
    par = nodes["parent"]
    return bool(np.any(par > np.arange(len(par))))       # a node whose parent is younger than itself


# ---- the unplanned edges of one tour, dim 2: edge j in the window j x 2 x maxIterations of the solver's stream
TOUR_EDGES = ((0, 1), (1, 2), (2, 3), (3, 0))
TOUR = [job("dense2d", a, b, 5, 3000, opt, skip=j * 2 * 3000) for opt in (False, True) for j, (a, b) in enumerate(TOUR_EDGES)]
TOUR_FIGURES = [(1, 1571, 582, 3142), (1, 1060, 343, 8120), (1, 572, 250, 13144), (1, 333, 143, 18666)]
TOUR_PLANS = [44, 33, 32, 33, 16, 11, 13, 10]


def assert_tour_oracles(ros):
    assert [figures(ro) for ro in ros] == TOUR_FIGURES * 2
    assert [len(ro.lazy_plan()) for ro in ros] == TOUR_PLANS
    assert all(rewired(ro.nodes()) for ro in ros[4:]) and not any(rewired(ro.nodes()) for ro in ros[:4])
    assert all(ro.stats()["lazy_distance"] < UNSOLVED for ro in ros)


def test_a_tour_pass_whose_members_finish_at_different_times(S, pool):
    """eight members, two kinds, one call: every edge is solved in the one launch of its kind, at its own iteration"""
    ros, rgs = build(S, pool, TOUR)
    assert_tour_oracles(ros)
    S.run_rrt_batch(rgs)
    in_one_launch(rgs)
    check_all(ros, rgs)
    close_all(rgs)


def test_dim_6_solved_and_unsolved_in_one_batch(S, pool):
    edges = (((3, 0), 12), ((2, 1), 12), ((2, 1), 11), ((0, 1), 12))      # the last start is walled in
    jobs = [job("dense3d_coarse", a, b, seed, 1200, opt) for opt in (False, True) for (a, b), seed in edges]
    ros, rgs = build(S, pool, jobs)
    assert [figures(ro) for ro in ros] == [(1, 60, 50, 420), (1, 935, 682, 6545), (0, 1200, 907, 8400), (0, 1200, 10, 8400)] * 2
    S.run_rrt_batch(rgs)
    check_all(ros, rgs)
    for ro, rg in zip(ros, rgs):
        st = rg.stats()
        assert st["batch_launches"] >= 1 and st["waves"] == 0 and st["speculated"] == 0 and st["batch_host_iterations"] == 0, st
        if ro.stats()["solved"]:
            assert st["lazy_distance"] < UNSOLVED and len(rg.lazy_plan()) > 2
        else:                                                              # DBL_MAX edge, no plan (src/lazy.h:280)
            assert st["solved"] == 0 and st["lazy_distance"] > UNSOLVED and len(rg.lazy_plan()) == 0
    close_all(rgs)


def test_solved_by_the_first_node(S, pool):
    """goal = the root itself: the first k (log10(2): 1 with only the root in the tree), the goal test on the first append, a
    launch that ends after one iteration"""
    jobs = [job(name, 0, 0, seed, 200, opt) for name in ("dense2d", "triang") for opt in (False, True) for seed in (1, 2, 3)]
    ros, rgs = build(S, pool, jobs)
    for jb, ro in zip(jobs, ros):
        step = common.scenario(jb[0])["sampling_dist"]
        assert figures(ro) == (1, 1, 2, 2 if jb[0] == "dense2d" else 7), jb
        assert list(ro.lazy_plan()) == [0, 1]
        assert abs(ro.stats()["lazy_distance"] - 2 * step) < 1e-9 * step, jb
    S.run_rrt_batch(rgs)
    in_one_launch(rgs)
    check_all(ros, rgs)                                                    # (lazy_distance: the oracle's bits)
    close_all(rgs)


def test_staged_with_getters_and_a_member_advanced_alone(S, pool):
    ros, rgs = build(S, pool, TOUR)
    assert_tour_oracles(ros)
    want = [ro.stats()["iterations"] for ro in ros]
    calls = 0
    after = [rg.stats()["iterations"] for rg in rgs]
    while True:
        before = after
        S.run_rrt_batch(rgs, max_iterations=97)
        calls += 1
        st = rgs[5].stats()
        assert len(rgs[5].nodes()["parent"]) == st["n_nodes"]
        assert (len(rgs[5].lazy_plan()) > 0) == bool(st["solved"])
        after = [rg.stats()["iterations"] for rg in rgs]
        assert all(0 <= a - b <= 97 for a, b in zip(after, before))
        assert all(a <= w for a, w in zip(after, want))
        assert all(bool(rg.stats()["solved"]) == (a == w) for rg, a, w in zip(rgs, after, want))
        if after == before:
            break
        if calls == 2:
            i0 = rgs[4].stats()["iterations"]
            rgs[4].run(50)                       # one member alone, on the single-session path, in between: it rejoins
            assert rgs[4].stats()["iterations"] == i0 + 50 < want[4]
            after[4] = i0 + 50
    assert calls > 3
    check_all(ros, rgs)
    assert rgs[4].stats()["batch_launches"] >= 3

    def snap():
        return [tuple(rg.stats()[k] for k in ("iterations", "rng_draws", "n_nodes", "collide_calls", "batch_launches", "lazy_distance")) for rg in rgs]

    s0 = snap()
    S.run_rrt_batch(rgs)                         # nothing left to do
    assert snap() == s0
    for rg in rgs:
        rg.run()                                 # ... on the single-session path neither
    assert snap() == s0
    check_all(ros, rgs)
    close_all(rgs)


def test_mixed_with_the_other_kinds(S, pool):
    """a lazy RRT, a lazy RRT*, an RRT, an RRT* and a Multi-T-RRT member in one call: four kinds, the last member of the RRT's"""
    jobs = [TOUR[1], TOUR[5]]
    ros, rgs = build(S, pool, jobs)
    others = [other_member(S, pool[2], name="dense3d", seed=100, iters=1500),
              other_member(S, pool[3], name="dense3d", seed=201, iters=1500, optimize=True),
              other_member(S, pool[4], name="triang", seed=3, iters=1500, n_roots=4)]
    with ThreadPoolExecutor(3) as ex:
        list(ex.map(lambda p: p[0].run(), others))
    assert [figures(ro) for ro in ros] == [TOUR_FIGURES[1]] * 2
    assert others[2][0].stats()["merges"] > 0
    S.run_rrt_batch(rgs + [p[1] for p in others])
    # (four kinds, so four launches per step at most - which the statistics cannot show: batch_launches counts the launches
    # ONE member took part in, one per step it was live in, and a later step exists for whoever handed an iteration over or
    # had its grid re-celled.  What they do show: each lazy member was done in the first step's launch of its own kind.)
    in_one_launch(rgs)
    check_all(ros, rgs)
    for ro, rg in others:
        assert rg.stats()["batch_launches"] >= 1 and rg.stats()["waves"] == 0
        assert_same_session(ro, rg)
    close_all(rgs + [p[1] for p in others])


def test_the_knob_is_the_sessions_not_the_calls(S, pool):
    ro, by = other_member(S, pool[0], name="dense3d", seed=100, iters=1500)
    ro.run()
    by.run(60)
    keys = ("iterations", "n_nodes", "collide_calls", "path_free_calls", "nn_queries", "rng_draws", "batch_launches", "waves")

    def state():
        n = by.nodes()
        return tuple(by.stats()[k] for k in keys), n["pos"].tobytes(), n["parent"].tobytes(), n["cost"].tobytes()

    st0 = state()

    def refused(members):
        for ms in (members, members[::-1]):
            with pytest.raises(S.SffGpuError) as e:
                S.run_rrt_batch(ms)
            assert "sffgpu error -1" in str(e.value), str(e.value)
            assert state() == st0

    # created with the knob unset (and with it set to 0): refused, also while the variable is set around the call
    for value in (None, 0):
        _, off = lazy_member(S, pool[1], TOUR[3], on=value)
        refused([by, off])
        with knob(1):
            refused([by, off])
        assert off.stats()["iterations"] == 0 and off.stats()["batch_launches"] == 0
        off.close()
    # created under the knob: accepted with the variable unset at the call
    (ro_on,), (on,) = build(S, pool[1:2], [TOUR[3]])
    assert figures(ro_on) == TOUR_FIGURES[3]
    refused([by, on, on])                                                  # the same session twice
    with knob(None):
        S.run_rrt_batch([on, by])
    in_one_launch([on])
    assert_same_edge(ro_on, on)
    assert by.stats()["batch_launches"] >= 1
    assert_same_session(ro, by)
    # two lazy sessions on one context (the second took the first one's store)
    _, a = lazy_member(S, pool[2], TOUR[2])
    _, b = lazy_member(S, pool[2], TOUR[3])
    with pytest.raises(S.SffGpuError) as e:
        S.run_rrt_batch([a, b])
    assert "sffgpu error -1" in str(e.value), str(e.value)
    close_all([by, on, a, b])


def test_batch_equals_the_sessions_run_alone(S, pool):
    """the three paths of this library on the tour's eight edges: k_rrt_seq_batch, the one-by-one host loop, speculative waves"""
    keys = ("iterations", "solved", "n_nodes", "n_live_trees", "merges", "n_links", "collide_calls", "path_free_calls",
            "nn_queries", "rng_draws", "lazy_distance")
    res = []
    for how in ("batch", 1, 0):
        ros, rgs = build(S, pool, TOUR, wave=(0 if how == "batch" else how))
        if how == "batch":
            assert_tour_oracles(ros)
            S.run_rrt_batch(rgs)
            in_one_launch(rgs)
        else:
            for rg in rgs:
                rg.run()
            assert all(rg.stats()["batch_launches"] == 0 for rg in rgs)
        out = []
        for rg in rgs:
            n, st = rg.nodes(), rg.stats()
            out.append((tuple(st[k] for k in keys), tuple(n[k].tobytes() for k in sorted(n)), rg.lazy_plan().tobytes()))
        res.append(out)
        close_all(rgs)
    assert res[0] == res[1], "batch against wave = 1"
    assert res[0] == res[2], "batch against wave = 0"
    assert [r[0][0] for r in res[0]] == [f[1] for f in TOUR_FIGURES] * 2 and all(r[0][1] == 1 for r in res[0])
