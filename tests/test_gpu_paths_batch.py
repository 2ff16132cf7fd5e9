"""Path extraction for forests together (S.paths_batch -> sffgpu_forest_paths_batch -> k_paths_batch) against the CPU oracle's
paths() / plan() and against a twin forest that called its own paths(), bit for bit: the cost matrix where finite, every
plan, connectedTrees and its order, the borders' rewritten distances.  The jobs and their references: smooth_shapes.py.  The
only tolerance anywhere is equality; every member and every pair is compared."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import smooth_shapes as H
from test_gpu_device_engine import engine

pytestmark = pytest.mark.gpu

DBL_MAX = 1.7976931348623157e308
TOL = 1e-9


@pytest.fixture(scope="module")
def S():
    import space_filling_forest_star_amd as S
    return S


@pytest.fixture(scope="module")
def contexts(S):
    """(scenario, k) -> a context with that world uploaded; made on first use, closed with the module"""
    made = {}

    def get(sc_name, sc, k=0):
        if (sc_name, k) not in made:
            c = S.Context(0)
            c.upload_env(sc["env"])
            c.upload_robot(sc["robot"])
            made[(sc_name, k)] = c
        return made[(sc_name, k)]
    yield get
    for c in made.values():
        c.close()


SLOT = {"T": 0, "E": 1, "TS": 2, "D2": 0, "D3": 0}     # (three shapes live on triang: three contexts of it)


def fresh(S, contexts, name, k=None, **env):
    ref = H.forest_ref(name)
    ctx = contexts(ref["scenario"], ref["sc"], SLOT[name] if k is None else k)
    with engine(**env):
        return S.Forest(ctx, ref["roots"], ref["sc"]["limits"], **ref["kw"])


def grown(S, contexts, name, k=None, **env):
    fg = fresh(S, contexts, name, k, **env)
    fg.run()
    assert fg.stats()["n_nodes"] == H.forest_ref(name)["n_nodes"]
    return fg


_twin = {}


def twin(S, contexts, name):
    """what a forest of the same job that called its own paths() reports: computed once per shape"""
    if name not in _twin:
        t = grown(S, contexts, name, 7)
        d, conn = t.paths()
        assert t.paths_stats()["calls"] == 0          # (the default: today's route, none of the new code)
        n = len(d)
        _twin[name] = dict(dist=d, connected=conn, plans={(i, j): t.plan(i, j) for i in range(n) for j in range(i + 1, n)},
                           borders=t.borders(), fingerprint=t.fingerprint())
        t.close()
    return _twin[name]


def pick_of(borders, i, j):
    """getPaths' pick among the borders of a pair, in list order (None: the pair has no border)"""
    best = None
    for ta, tb, d in zip(borders["ta"], borders["tb"], borders["dist"]):
        if (min(ta, tb), max(ta, tb)) == (i, j) and (best is None or d < best - TOL):
            best = d
    return best


def shape_facts(name):
    """from the oracle alone: pairs with a path but no border, pairs whose border's pick the closure replaced, most borders
    of a pair, trees without any path"""
    ref = H.forest_ref(name)
    fo = ref["keep"][0]
    b, raw, n = fo.borders(), ref["raw"], ref["n"]
    closure_only, replaced, per_pair = set(), set(), {}
    for ta, tb in zip(b["ta"], b["tb"]):
        key = (min(ta, tb), max(ta, tb))
        per_pair[key] = per_pair.get(key, 0) + 1
    for i in range(n):
        for j in range(i + 1, n):
            pick = pick_of(b, i, j)
            if raw[i, j] < 1e300 and pick is None:
                closure_only.add((i, j))
            if pick is not None:
                assert raw[i, j] <= pick
                if raw[i, j] < pick - TOL:
                    replaced.add((i, j))
    lonely = [t for t in range(n) if all(raw[t, u] > 1e300 for u in range(n) if u != t)]
    return dict(closure_only=closure_only, replaced=replaced, most=max(per_pair.values()) if per_pair else 0, lonely=lonely,
                borders=len(b["ta"]))


def test_the_shapes_hold_what_the_kernel_must_decide():
    """the properties each shape is here for, from the oracle alone: a changed fixture cannot empty the suite"""
    t = shape_facts("T")
    assert t["closure_only"] == {(0, 5), (1, 3), (1, 4), (1, 5), (2, 3), (2, 4), (2, 5)}
    assert t["replaced"] == {(0, 3)} and t["most"] == 96 and t["borders"] == 329
    d3 = shape_facts("D3")
    assert d3["closure_only"] == {(1, 2), (1, 4)} and d3["replaced"] == {(3, 4)}
    assert len(d3["lonely"]) == 1 and H.forest_ref("D3")["n"] == 5
    ts = shape_facts("TS")
    assert ts["closure_only"] == {(1, 3), (2, 3)} and ts["replaced"] == set() and H.forest_ref("TS")["kw"]["optimize"]
    assert shape_facts("E")["borders"] == 0 and not np.any(H.forest_ref("E")["raw"][~np.eye(5, dtype=bool)] < 1e300)
    assert H.forest_ref("D2")["kw"]["wave"] == 16
    n_paths = {n: sum(1 for p in H.forest_ref(n)["raw_plans"].values() if len(p)) for n in H.FORESTS}
    assert n_paths == dict(T=15, D2=6, D3=6, E=0, TS=6)


def assert_paths_equal(S, contexts, name, fg, d, conn, ref=None, against_twin=True):
    ref = ref or H.forest_ref(name)
    finite = ref["raw"] < 1e300
    assert np.array_equal(finite, d < 1e300), name
    assert np.array_equal(ref["raw"][finite], d[finite]), name
    assert np.all(d[~finite] == DBL_MAX) and np.all(np.diag(d) == 0), name
    for ij, p in ref["raw_plans"].items():
        assert np.array_equal(p, fg.plan(*ij)), (name, ij)
    if against_twin:
        tw = twin(S, contexts, name)
        assert np.array_equal(tw["dist"], d), name
        assert np.array_equal(tw["connected"], conn), (name, tw["connected"], conn)
        for ij, p in tw["plans"].items():
            assert np.array_equal(p, fg.plan(*ij)), (name, ij)


def entries_of(name):
    return sum(len(p) for p in H.forest_ref(name)["raw_plans"].values())


@pytest.mark.parametrize("name", ["T", "D3", "TS", "E", "D2"])
def test_one_member(S, contexts, name):
    """each shape alone; D2 here as the device engine's rounds of 16 slots leave it (in the call of five it is a host-route member)"""
    fg = grown(S, contexts, name)
    assert fg.device_engine() and fg.paths_stats()["calls"] == 0
    ((d, conn),) = S.paths_batch([fg])
    assert_paths_equal(S, contexts, name, fg, d, conn)
    ps = fg.paths_stats()
    want = dict(calls=1, launches=1, device_calls=1, host_calls=0, fallbacks=0, host_syncs=0,
                pairs=dict(T=15, D3=6, TS=6, E=0, D2=6)[name], entries=entries_of(name))
    assert {k: ps[k] for k in want} == want, ps
    fg.close()


def test_all_five_in_one_call(S, contexts):
    """four device-route members and D2 - wave 16, grown by the host-replay engine: a host-route member - in one call"""
    names = ["T", "D2", "D3", "E", "TS"]
    members = [grown(S, contexts, n, **(dict(SFFGPU_ENGINE="host") if n == "D2" else {})) for n in names]
    assert len({id(f.ctx) for f in members}) == 5
    assert not members[1].device_engine()
    out = S.paths_batch(members)
    assert len(out) == 5
    for n, fg, (d, conn) in zip(names, members, out):
        assert_paths_equal(S, contexts, n, fg, d, conn)
        ps = fg.paths_stats()
        if n == "D2":
            assert (ps["device_calls"], ps["host_calls"], ps["host_syncs"], ps["launches"]) == (0, 1, 0, 0), ps
        else:
            assert (ps["device_calls"], ps["host_calls"], ps["host_syncs"], ps["launches"]) == (1, 0, 0, 1), ps
    for n, fg in zip(names, members):           # (the getters download the forest now: as the twin's)
        tw = twin(S, contexts, n)
        b = fg.borders()
        for k in ("ta", "tb", "n1", "n2", "dist"):
            assert np.array_equal(tw["borders"][k], b[k]), (n, k)
        assert fg.fingerprint() == tw["fingerprint"], n
        for ij, p in tw["plans"].items():
            assert np.array_equal(p, fg.plan(*ij)), (n, ij)
        fg.close()


def test_a_partly_grown_forest_and_on(S, contexts):
    """T after 1500 waves of a forest batch against the oracle's run(1500); its borders read (the mirror now holds them);
    grown to the end and extracted again - the device route once more, the mirror's borders patched from the device's"""
    ref = H.forest_ref("T")
    w = O.World(ref["sc"]["env"], ref["sc"]["robot"], O.TRIG_PORTABLE)
    fo = O.Forest(w, ref["roots"], ref["sc"]["limits"], **ref["kw"])
    fo.run(1500)
    assert 0 < fo.stats()["n_nodes"] < ref["n_nodes"]
    n = ref["n"]
    part = dict(raw=fo.paths(), raw_plans={(i, j): fo.plan(i, j) for i in range(n) for j in range(i + 1, n)})
    assert np.any(part["raw"][~np.eye(n, dtype=bool)] < 1e300)
    fg = fresh(S, contexts, "T")
    S.run_batch([fg], 1500)
    assert fg.stats()["n_nodes"] == fo.stats()["n_nodes"]
    ((d, conn),) = S.paths_batch([fg])
    assert_paths_equal(S, contexts, "T", fg, d, conn, ref=part, against_twin=False)
    bo, bg = fo.borders(), fg.borders()
    for k in ("ta", "tb", "n1", "n2", "dist"):
        assert np.array_equal(bo[k], bg[k]), k
    S.run_batch([fg])
    assert fg.stats()["n_nodes"] == ref["n_nodes"]
    fo = ref["keep"][0]                          # (the oracle's whole run, its paths extracted)
    ((d, conn),) = S.paths_batch([fg])
    assert_paths_equal(S, contexts, "T", fg, d, conn)
    ps = fg.paths_stats()
    assert (ps["calls"], ps["device_calls"], ps["host_syncs"], ps["fallbacks"]) == (2, 2, 0, 0), ps
    bo, bg = fo.borders(), fg.borders()
    assert len(bo["dist"]) == 329
    for k in ("ta", "tb", "n1", "n2", "dist"):
        assert np.array_equal(bo[k], bg[k]), k
    assert fg.fingerprint() == twin(S, contexts, "T")["fingerprint"]
    fg.close()


def test_paths_then_smoothing_without_a_download(S, contexts):
    names = ["T", "D3", "TS"]
    members = [grown(S, contexts, n) for n in names]
    S.paths_batch(members)
    mats = S.smooth_batch(members)
    for n, fg, d in zip(names, members, mats):
        ref = H.forest_ref(n)
        want = ref["stages"][0]
        finite = ref["raw"] < 1e300
        assert np.array_equal(finite, d < 1e300) and np.array_equal(want["dist"][finite], d[finite]), n
        for ij, p in want["plans"].items():
            assert np.array_equal(p, fg.plan(*ij)), (n, ij)
        st = fg.stats()
        assert st["path_free_calls"] == want["path_free_calls"] and st["collide_calls"] == want["collide_calls"], n
        assert fg.smooth_stats()["edges"] == want["edges"], n
        assert fg.paths_stats()["host_syncs"] == 0
    # nothing has been downloaded: a second extraction still finds the state on the device ...
    probe = members[0]
    S.paths_batch([probe])
    ps = probe.paths_stats()
    assert (ps["device_calls"], ps["host_calls"], ps["host_syncs"]) == (2, 0, 0), ps
    # ... and the first getter that needs the forest brings the oracle's down, with the counters smoothing left
    for n, fg in zip(names, members):
        ref = H.forest_ref(n)
        no, ng = ref["keep"][0].nodes(), fg.nodes()
        for k in no:
            assert np.array_equal(no[k], ng[k]), (n, k)
        st = fg.stats()
        want = ref["stages"][0]
        assert st["path_free_calls"] == want["path_free_calls"] and st["collide_calls"] == want["collide_calls"], n
        fg.close()


def test_a_full_plan_pool_falls_back_to_the_host_route(S, contexts):
    fg = grown(S, contexts, "T", SFFGPU_TEST_PATHS_CAP=8)
    ((d, conn),) = S.paths_batch([fg])
    assert_paths_equal(S, contexts, "T", fg, d, conn)
    ps = fg.paths_stats()
    want = dict(calls=1, launches=1, device_calls=0, host_calls=0, fallbacks=1, host_syncs=1, pairs=15)
    assert {k: ps[k] for k in want} == want, ps
    tw = twin(S, contexts, "T")
    assert np.array_equal(tw["borders"]["dist"], fg.borders()["dist"]) and fg.fingerprint() == tw["fingerprint"]
    fg.close()


def test_a_solved_goal_forest(S):
    """two start trees and a goal tree, solved in the loop of waves of one slot (a job of test_gpu_goal_loop.py)"""
    from test_gpu_forest_batch import member
    job = dict(name="triang", seed=8, iters=60000, n_roots=2, goal_offset=[12, 8, 5])
    c1, c2 = S.Context(0), S.Context(0)
    fo, fg = member(S, c1, SFFGPU_GOAL_LOOP=1, **job)
    _, tw = member(S, c2, SFFGPU_GOAL_LOOP=1, **job)
    fo.run()
    so = fo.stats()
    assert (so["solved"], so["iterations"], so["n_nodes"], so["n_borders"], so["n_trees"]) == (1, 1643, 414, 1, 3), so
    fg.run()
    tw.run()
    ((d, conn),) = S.paths_batch([fg])
    dt, ct = tw.paths()
    raw = fo.paths()
    assert np.sum(raw[np.triu_indices(3, 1)] < 1e300) == 1
    assert np.array_equal(raw, d) and np.array_equal(dt, d) and np.array_equal(ct, conn)
    for i in range(3):
        for j in range(i + 1, 3):
            assert np.array_equal(fo.plan(i, j), fg.plan(i, j)) and np.array_equal(tw.plan(i, j), fg.plan(i, j)), (i, j)
    ps = fg.paths_stats()
    assert (ps["device_calls"], ps["host_syncs"], ps["pairs"]) == (1, 0, 1), ps
    assert fg.fingerprint() == tw.fingerprint() == fo.fingerprint()
    for f in (fg, tw):
        f.close()
    c1.close()
    c2.close()


def test_the_knob(S, contexts):
    fg = grown(S, contexts, "T", SFFGPU_PATHS_DEV=1)
    d, conn = fg.paths()
    assert_paths_equal(S, contexts, "T", fg, d, conn)
    ps = fg.paths_stats()
    assert (ps["calls"], ps["device_calls"], ps["host_syncs"]) == (1, 1, 0), ps
    fg.close()
    off = grown(S, contexts, "T")
    d0, conn0 = off.paths()
    assert np.array_equal(d0, d) and np.array_equal(conn0, conn)
    assert off.paths_stats()["calls"] == 0
    off.close()


def test_refusals(S, contexts):
    t = grown(S, contexts, "T")
    S.paths_batch([t])
    before = {ij: t.plan(*ij) for ij in H.forest_ref("T")["raw_plans"]}
    L = S.lib()
    n = H.forest_ref("T")["n"]
    mat = np.full((n, n), -1.0)
    dist = (C.POINTER(C.c_double) * 2)(mat.ctypes.data_as(C.POINTER(C.c_double)), None)

    def call(handles, count):
        failed = C.c_int32(-7)
        rc = L.sffgpu_forest_paths_batch(handles, count, dist, None, None, C.byref(failed))
        return rc, failed.value

    assert call((C.c_void_p * 2)(t.h, t.h), 2) == (-1, -1)          # the same forest twice
    assert call((C.c_void_p * 2)(t.h, None), 2) == (-1, -1)         # a NULL member
    assert call((C.c_void_p * 2)(t.h, None), 0) == (-1, -1)
    assert call(None, 1) == (-1, -1)
    with pytest.raises(S.SffGpuError):
        S.paths_batch([t, t])
    with pytest.raises(S.SffGpuError):
        S.paths_batch([])
    assert np.all(mat == -1.0)
    assert t.paths_stats()["calls"] == 1
    for ij, p in before.items():
        assert np.array_equal(p, t.plan(*ij))
    t.close()
