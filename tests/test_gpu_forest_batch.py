"""Forest batches (sffgpu_forest_run_batch / S.run_batch): N independent forests of waves of ONE slot, each on a context of
its own, advanced together - one wavefront per forest, one launch of k_seq_waves_batch for all of them.  Every member is
compared with the CPU oracle's sequential run of the same seed (bit-equal fp64 positions, costs, parents, borders,
counters, fingerprint); the last test compares the batch with the library's own single-forest path."""
import numpy as np
import pytest

import common
import oracle_lib as O
from test_gpu_device_engine import engine
from test_gpu_parity import assert_same_forest, load_world

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


_oracle_runs = {}   # (scenario, seed, iterations, optimize, shift) -> the oracle forest after its run (cases share members)


def member(S, ctx, name, seed, iters, optimize=False, wave=1, n_roots=5, goal_offset=None, priority_bias=0.0, shift=None, **env):
    """one member on ITS context, the way test_gpu_device_engine.make builds a forest: roots of its own seed"""
    sc, w = load_world(ctx, name, shift)
    roots = sc["xml_points"][:n_roots] if sc["xml_points"] is not None else \
        common.free_roots(w.collide, sc["limits"], n_roots, seed=seed, dim=sc["dim"])
    kw = dict(dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"], dim=sc["dim"], max_iterations=iters,
              wave=wave, seed=seed, optimize=optimize, priority_bias=priority_bias)
    if goal_offset is not None:
        g = roots[0].copy()
        g[:3] += np.array(goal_offset, dtype=np.float64)
        kw["goal"] = g
    key = (name, seed, iters, optimize, None if shift is None else tuple(shift))
    plain = wave == 1 and goal_offset is None and priority_bias == 0.0 and n_roots == 5
    if plain and key in _oracle_runs:
        fo = _oracle_runs[key]
    else:
        fo = O.Forest(w, roots, sc["limits"], **kw)
        if plain:
            fo.run()
            _oracle_runs[key] = fo
    with engine(SFFGPU_ENGINE="device", **env):
        fg = S.Forest(ctx, roots, sc["limits"], **kw)
    return fo, fg


def build(S, pool, specs):
    assert len(specs) <= len(pool)
    pairs = [member(S, pool[i], **sp) for i, sp in enumerate(specs)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def check_all(fos, fgs, min_nodes=40):
    for fo, fg in zip(fos, fgs):
        assert fo.stats()["n_nodes"] > min_nodes
        assert_same_forest(fo, fg)
    fps = [fg.fingerprint() for fg in fgs]
    assert len(set(fps)) == len(fps), "two members of the batch are the same forest"


def close_all(fgs):
    for fg in fgs:
        fg.close()


def test_batch_sff(S, pool):
    fos, fgs = build(S, pool, [dict(name="dense3d", seed=s, iters=1500) for s in range(100, 132)])
    S.run_batch(fgs)
    for fo, fg in zip(fos, fgs):
        st = fg.stats()
        assert st["iterations"] == 1500 == fo.stats()["iterations"]
        assert st["batch_launches"] >= 1 and st["spec_steps"] == 0 and st["host_fallback_waves"] == 0, st
        assert 379 <= st["n_nodes"] <= 463
    check_all(fos, fgs)
    close_all(fgs)


def test_batch_sff_star(S, pool):
    fos, fgs = build(S, pool, [dict(name="dense3d", seed=s, iters=1200, optimize=True) for s in range(200, 216)])
    S.run_batch(fgs)
    for fo, fg in zip(fos, fgs):
        st = fg.stats()
        assert st["iterations"] == 1200
        assert st["batch_launches"] >= 1 and st["spec_steps"] == 0 and st["host_fallback_waves"] == 0 and st["star_rounds"] > 0, st
        assert 314 <= st["n_nodes"] <= 375
    check_all(fos, fgs)
    close_all(fgs)


def test_batch_mixed_environments_kinds_and_lengths(S, pool):
    """different maps and robots (LDS sizes), both template instances, members that finish long before others"""
    specs = [dict(name="triang", seed=300 + i, iters=it) for i, it in enumerate((2000, 1500, 1000, 500))]
    specs += [dict(name="dense2d", seed=s, iters=1500) for s in range(400, 404)]
    specs += [dict(name="building", seed=s, iters=1500, optimize=True) for s in range(600, 604)]
    specs += [dict(name="dense3d", seed=7, iters=300)]
    fos, fgs = build(S, pool, specs)
    S.run_batch(fgs)
    for sp, fg in zip(specs, fgs):
        st = fg.stats()
        assert st["iterations"] == sp["iters"] and st["batch_launches"] >= 1 and st["spec_steps"] == 0, (sp, st)
    assert fgs[-1].stats()["n_nodes"] == 117
    check_all(fos, fgs)
    close_all(fgs)


def test_batch_staged_with_getters_and_a_member_advanced_alone(S, pool):
    fos, fgs = build(S, pool, [dict(name="dense3d", seed=s, iters=1500) for s in range(100, 108)])
    calls = 0
    while True:
        before = [fg.stats()["waves"] for fg in fgs]
        S.run_batch(fgs, max_waves=97)
        calls += 1
        after = [fg.stats()["waves"] for fg in fgs]
        assert all(0 <= a - b <= 97 for a, b in zip(after, before))
        for fg in (fgs[1], fgs[6]):
            assert len(fg.nodes()["parent"]) == fg.stats()["n_nodes"]
        if after == before:
            break
        if calls == 2:
            w0 = fgs[3].stats()["waves"]
            fgs[3].run(50)                       # one member alone, on the single-forest path, in between
            assert fgs[3].stats()["waves"] == w0 + 50
    assert calls > 3
    check_all(fos, fgs)
    fps = [fg.fingerprint() for fg in fgs]
    S.run_batch(fgs)                             # nothing left to do
    assert [fg.fingerprint() for fg in fgs] == fps
    close_all(fgs)


def test_batch_member_that_faults_to_the_host_path(S, pool):
    """a hit list of three entries: member A's overflows hand single waves to the host-replay engine, the others never notice"""
    fos, fgs = [], []
    for i, sp in enumerate([dict(name="dense3d_coarse", seed=4, iters=6000, SFFGPU_TEST_HITCAP=3),
                            dict(name="dense3d_coarse", seed=2, iters=6000),
                            dict(name="dense3d", seed=100, iters=1500), dict(name="dense3d", seed=101, iters=1500)]):
        fo, fg = member(S, pool[i], **sp)
        fos.append(fo)
        fgs.append(fg)
    S.run_batch(fgs)
    assert fgs[0].stats()["host_fallback_waves"] > 0
    for fg in fgs[1:]:
        assert fg.stats()["host_fallback_waves"] == 0
    check_all(fos, fgs)
    close_all(fgs)


def test_batch_refusals_leave_a_bystander_alone(S, pool):
    _, by = member(S, pool[0], name="dense3d", seed=100, iters=1500)
    by.run(60)
    fp, waves = by.fingerprint(), by.stats()["waves"]

    def refused(others):
        with pytest.raises(S.SffGpuError):
            S.run_batch([by] + others)
        assert by.fingerprint() == fp and by.stats()["waves"] == waves
        with pytest.raises(S.SffGpuError):
            S.run_batch(others + [by])
        assert by.fingerprint() == fp and by.stats()["waves"] == waves

    _, a = member(S, pool[1], name="dense3d", seed=101, iters=1500)
    _, b = member(S, pool[1], name="dense3d", seed=102, iters=1500)      # (the same context: it took a's store)
    refused([a, b])
    a.close()
    refused([b, b])                                                        # the same forest twice
    refused([by])
    b.close()
    _, wide = member(S, pool[2], name="dense3d", seed=103, iters=1500, wave=64)
    refused([wide])
    _, goal = member(S, pool[3], name="triang", seed=104, iters=1500, n_roots=2, goal_offset=[12, 8, 5])
    refused([goal])
    _, prio = member(S, pool[4], name="dense3d", seed=105, iters=1500, priority_bias=0.5)
    refused([prio])
    L = S.lib()
    assert L.sffgpu_forest_run_batch(None, 0, 0, None) == -1
    # ... and the bystander is still a member like any other
    _, ok = member(S, pool[5], name="dense3d", seed=101, iters=1500)
    S.run_batch([by, ok])
    fo, _unused = member(S, pool[6], name="dense3d", seed=100, iters=1500)
    assert_same_forest(fo, by)
    close_all([by, wide, goal, prio, ok, _unused])


def test_batch_equals_the_forests_run_alone(S, pool):
    """the two paths of this library (k_seq_waves_batch here, k_spec_waves by default there) on the same eight jobs"""
    keys = ("iterations", "solved", "n_nodes", "n_trees", "frontier_size", "closed_size", "n_connected", "n_borders",
            "collide_calls", "path_free_calls", "nn_queries", "waves")
    sc = common.scenario("dense3d")
    res = []
    for batch in (True, False):
        fgs = []
        for i, seed in enumerate(range(100, 108)):
            _, w = load_world(pool[i], "dense3d")
            roots = common.free_roots(w.collide, sc["limits"], 5, seed=seed, dim=sc["dim"])
            fgs.append(S.Forest(pool[i], roots, sc["limits"], dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"],
                                dim=sc["dim"], max_iterations=6000, wave=1, seed=seed))
        if batch:
            S.run_batch(fgs)
        else:
            for fg in fgs:
                fg.run()
        res.append([(fg.fingerprint(), tuple(fg.stats()[k] for k in keys)) for fg in fgs])
        if batch:
            assert all(fg.stats()["batch_launches"] >= 1 and fg.stats()["spec_steps"] == 0 for fg in fgs)
        else:
            assert all(fg.stats()["batch_launches"] == 0 for fg in fgs)
        close_all(fgs)
    assert res[0] == res[1]
    assert len({r[0] for r in res[0]}) == 8 and all(r[1][2] > 40 for r in res[0])
