"""Path smoothing on the device (k_smooth_paths through S.smooth_batch / S.smooth_rrt_batch, and through the single calls
under SFFGPU_SMOOTH_LOOP=1) against the CPU oracle's smooth(), bit for bit: cost matrices where finite, every plan, the two
reference-equivalent counters, and the number of edges the walk tested = the oracle's growth of path_free_calls - the walk
stops at the first free candidate of a step, as the reference does.  The jobs and their references: smooth_shapes.py.
The only tolerance anywhere is equality; every member and every path is compared."""
import ctypes as C

import numpy as np
import pytest

import smooth_shapes as H
from test_gpu_device_engine import engine

pytestmark = pytest.mark.gpu

DBL_MAX = 1.7976931348623157e308


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


def grown_forest(S, contexts, name, k=0, **env):
    """the library's forest of a shape, run, its raw paths extracted and checked against the oracle's"""
    ref = H.forest_ref(name)
    ctx = contexts(ref["scenario"], ref["sc"], k)
    with engine(**env):
        fg = S.Forest(ctx, ref["roots"], ref["sc"]["limits"], **ref["kw"])
    fg.run()
    assert fg.stats()["n_nodes"] == ref["n_nodes"]
    dg, _ = fg.paths()
    finite = ref["raw"] < 1e300
    assert np.array_equal(finite, dg < 1e300) and np.array_equal(ref["raw"][finite], dg[finite])
    for ij, p in ref["raw_plans"].items():
        assert np.array_equal(p, fg.plan(*ij)), (name, ij)
    return fg, dg


def assert_forest_equal(name, fg, d, stage=0, edges_before=0):
    """equal to the oracle after its (stage + 1)-th smooth()"""
    ref = H.forest_ref(name)
    want = ref["stages"][stage]
    finite = ref["raw"] < 1e300
    assert np.array_equal(finite, d < 1e300), name
    assert np.array_equal(want["dist"][finite], d[finite]), name
    assert set(want["plans"]) == {(i, j) for i in range(ref["n"]) for j in range(i + 1, ref["n"])}
    for ij, p in want["plans"].items():
        assert np.array_equal(p, fg.plan(*ij)), (name, ij)
    st, sm = fg.stats(), fg.smooth_stats()
    assert st["path_free_calls"] == want["path_free_calls"], name
    assert st["collide_calls"] == want["collide_calls"], name
    assert sm["edges"] - edges_before == want["edges"], (name, sm, want["edges"])
    assert sm["host_edges"] == 0, name


def test_the_shapes_have_what_the_kernel_must_decide():
    """the properties each shape was chosen for, from the oracle alone"""
    n_paths = {n: sum(1 for p in H.forest_ref(n)["raw_plans"].values() if len(p)) for n in H.FORESTS}
    assert n_paths == dict(T=15, D2=6, D3=6, E=0, TS=6)
    edges = {n: H.forest_ref(n)["stages"][0]["edges"] for n in H.FORESTS}
    assert edges == dict(T=20, D2=496, D3=30, E=0, TS=8)
    assert max(len(p) for p in H.forest_ref("D2")["raw_plans"].values()) == 56
    assert max(len(p) for p in H.forest_ref("T")["raw_plans"].values()) == 23
    assert H.session_ref("R1")["edges"] == 232 and sorted(len(p) for p in H.session_ref("R1")["plans"]) == [3, 6, 7]
    assert H.session_ref("R2")["edges"] == 245 and len(H.session_ref("R2")["plans"]) == 2


def test_the_walks_have_what_the_kernel_must_decide():
    """the walk replayed edge by edge on the oracle (T and D2; D3's edges of up to 6 846 samples cost the CPU seconds - its
    30 edges and 9 steps are asserted where it runs)"""
    # T: short edges only - the inline clearance path (edges of at most 512 samples) can decide every free one
    t = H.walk_figures("T")
    assert (t["steps"], len(t["edges"])) == (17, 20)
    assert sum(1 for fr, _, _ in t["edges"] if fr) == 16 and max(ns for _, _, ns in t["edges"]) <= 491
    # D2: long edges, first hits far along them, and two steps without a free candidate
    d2 = H.walk_figures("D2")
    assert (d2["steps"], d2["none_free"], len(d2["edges"])) == (33, 2, 496)
    assert max(ns for _, _, ns in d2["edges"]) == 22364 and max(fh for fr, fh, _ in d2["edges"] if not fr) == 12267
    assert sum(1 for fr, fh, _ in d2["edges"] if not fr and fh > 256) == 431


@pytest.mark.parametrize("name", ["T", "D2", "D3"])
def test_one_member(S, contexts, name):
    fg, raw = grown_forest(S, contexts, name)
    assert fg.smooth_stats()["launches"] == 0
    (d,) = S.smooth_batch([fg])
    assert_forest_equal(name, fg, d)
    sm = fg.smooth_stats()
    assert sm["launches"] >= 1
    assert (sm["paths"], sm["steps"]) == dict(T=(15, 17), D2=(6, 33), D3=(6, 9))[name]
    finite = raw < 1e300
    assert np.any(d[finite] < raw[finite] - 1e-6)
    fg.close()


def test_mixed_batch(S, contexts):
    """five forests of four kinds of world in one call, each on a context of its own; every member equals its oracle and a
    twin (same seed, another context) smoothed by the host walk of smooth()"""
    names = ["T", "D2", "D3", "E", "TS"]
    slot = {"T": 0, "E": 1, "TS": 2, "D2": 0, "D3": 0}          # (three of them live on triang: three contexts of it)
    members = [grown_forest(S, contexts, n, slot[n])[0] for n in names]
    assert len({id(f.ctx) for f in members}) == 5
    mats = S.smooth_batch(members)
    assert len(mats) == 5
    for n, fg, d in zip(names, members, mats):
        assert_forest_equal(n, fg, d)
        twin, _ = grown_forest(S, contexts, n, 7)
        assert twin.ctx is not fg.ctx
        dt = twin.smooth()
        assert twin.smooth_stats()["launches"] == 0
        assert np.array_equal(dt, d), n
        for i in range(len(d)):
            for j in range(i + 1, len(d)):
                assert np.array_equal(twin.plan(i, j), fg.plan(i, j)), (n, i, j)
        for k in ("path_free_calls", "collide_calls"):
            assert twin.stats()[k] == fg.stats()[k], (n, k)
        twin.close()
    e = mats[names.index("E")]
    assert np.all(e[~np.eye(len(e), dtype=bool)] == DBL_MAX) and np.all(np.diag(e) == 0)
    sm = members[names.index("E")].smooth_stats()
    assert sm["edges"] == 0 and sm["paths"] == 0
    for f in members:
        f.close()


def test_resumption(S, contexts):
    """one edge per launch and path: the walk stops and continues inside its steps, and counts nothing twice"""
    fg, _ = grown_forest(S, contexts, "D2", SFFGPU_SMOOTH_EDGES=1)
    (d,) = S.smooth_batch([fg])
    assert_forest_equal("D2", fg, d)
    sm = fg.smooth_stats()
    assert sm["launches"] > 1 and sm["edges"] == H.forest_ref("D2")["stages"][0]["edges"]
    fg.close()


@pytest.mark.parametrize("name", ["T", "D2"])
def test_twice(S, contexts, name):
    fg, _ = grown_forest(S, contexts, name)
    (d1,) = S.smooth_batch([fg])
    assert_forest_equal(name, fg, d1)
    first = fg.smooth_stats()["edges"]
    (d2,) = S.smooth_batch([fg])
    assert_forest_equal(name, fg, d2, stage=1, edges_before=first)
    fg.close()


def test_knob(S, contexts):
    fg, _ = grown_forest(S, contexts, "D2", SFFGPU_SMOOTH_LOOP=1)
    d = fg.smooth()
    assert_forest_equal("D2", fg, d)
    assert fg.smooth_stats()["launches"] > 0
    fg.close()
    fg, _ = grown_forest(S, contexts, "D2")
    d0 = fg.smooth()
    assert fg.smooth_stats()["launches"] == 0 and np.array_equal(d0, d)
    fg.close()


def grown_session(S, contexts, name, k=0, **env):
    ref = H.session_ref(name)
    ctx = contexts(ref["scenario"], ref["sc"], k)
    with engine(**env):
        rg = S.Rrt(ctx, ref["roots"], ref["sc"]["limits"], wave=0, **ref["kw"])
    rg.run()
    d, _ = rg.paths(ref["nt"])
    assert np.array_equal(d, ref["dist"])
    return rg, d


def assert_session_equal(name, rg, plans):
    ref = H.session_ref(name)
    assert len(plans) == len(ref["plans"]) > 0
    for x, y in zip(ref["plans"], plans):
        assert np.array_equal(x, y), name
    st, sm = rg.stats(), rg.smooth_stats()
    assert st["path_free_calls"] == ref["path_free_calls"] and st["collide_calls"] == ref["collide_calls"], name
    assert sm["edges"] == ref["edges"] and sm["host_edges"] == 0 and sm["launches"] >= 1, (name, sm)


def test_rrt(S, contexts):
    r1, m1 = grown_session(S, contexts, "R1", 5)
    r2, m2 = grown_session(S, contexts, "R2", 5)
    p1, p2 = S.smooth_rrt_batch([r1, r2])
    assert_session_equal("R1", r1, p1)
    assert_session_equal("R2", r2, p2)
    for rg, m, name in ((r1, m1, "R1"), (r2, m2, "R2")):
        again, _ = rg.paths(H.session_ref(name)["nt"])
        assert np.array_equal(again, m)
        rg.close()
    rg, _ = grown_session(S, contexts, "R1", 5, SFFGPU_SMOOTH_LOOP=1)
    assert_session_equal("R1", rg, rg.smooth())
    rg.close()
    rg, _ = grown_session(S, contexts, "R1", 5)
    plans = rg.smooth()
    assert rg.smooth_stats()["launches"] == 0
    for x, y in zip(p1, plans):
        assert np.array_equal(x, y)
    rg.close()


def test_refusals(S, contexts):
    t, _ = grown_forest(S, contexts, "T")
    ref3 = H.forest_ref("D3")
    with engine():
        d3 = S.Forest(contexts(ref3["scenario"], ref3["sc"]), ref3["roots"], ref3["sc"]["limits"], **ref3["kw"])
    d3.run()                                                     # (no paths())
    L = S.lib()
    before = {ij: t.plan(*ij) for ij in H.forest_ref("T")["raw_plans"]}
    arr = (C.c_void_p * 2)(t.h, d3.h)
    failed = C.c_int32(-7)
    assert L.sffgpu_forest_smooth_paths_batch(arr, 2, None, C.byref(failed)) == -3      # SFFGPU_ERR_STATE
    assert failed.value == 1
    with pytest.raises(S.SffGpuError, match="member 1"):
        S.smooth_batch([t, d3])
    for ij, p in before.items():
        assert np.array_equal(p, t.plan(*ij))
    assert t.smooth_stats()["launches"] == 0 and t.smooth_stats()["edges"] == 0
    twice = (C.c_void_p * 2)(t.h, t.h)
    failed = C.c_int32(-7)
    assert L.sffgpu_forest_smooth_paths_batch(twice, 2, None, C.byref(failed)) == -1    # SFFGPU_ERR_ARG
    assert failed.value == -1
    with pytest.raises(S.SffGpuError):
        S.smooth_batch([t, t])
    (d,) = S.smooth_batch([t])
    assert_forest_equal("T", t, d)
    t.close()
    d3.close()
