"""The priority-frontier mode (Problem::priorityBias, src/forest.h:126-147,160-181,360-363) in the loop of waves of ONE slot
(k_seq_waves<., true>) and in forest batches (k_seq_waves_batch<., true>), for forests created under SFFGPU_PRIO_LOOP=1.
Every case compares with the CPU oracle's sequential run of the same seed through assert_same_forest: bit-equal fp64
positions and costs, equal parents, borders, reference-equivalent counters and fingerprint.  The heap ARRAY order is part of
the result (random entries are popped by index), so a push, a removal or a put-back in the wrong place shows."""
import pytest

from test_gpu_forest_batch import member
from test_gpu_parity import assert_same_forest

pytestmark = pytest.mark.gpu

N_CTX = 12
KNOB = dict(SFFGPU_PRIO_LOOP=1)


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


_oracle = {}   # job -> the oracle forest after its run: computed once, shared by the tests that use the job, never advanced again


def pair(S, ctx, name, seed, iters, bias, n_roots=5, optimize=False, knob=True, shift=None, **env):
    """(oracle after its whole run, the library's forest before its first wave) of one job"""
    if knob:
        env = dict(env, **KNOB)
    fo, fg = member(S, ctx, name, seed, iters, optimize=optimize, n_roots=n_roots, priority_bias=bias, shift=shift, **env)
    key = (name, seed, iters, bias, n_roots, optimize) + (() if shift is None else (tuple(shift),))
    if key not in _oracle:
        if bias != 0.0:   # (member() has run - and keeps - the plain ones)
            fo.run()
        _oracle[key] = fo
    return _oracle[key], fg


def ran_in_the_loop(fg, iters):
    st = fg.stats()
    assert fg.device_engine()
    # the persistent wavefront: one "sweep" per iteration, no step of the speculative kernel, no wave graph of the round engine
    assert st["sweeps"] == st["iterations"] == iters and st["spec_steps"] == 0 and st["graph_launches"] == 0, st
    assert st["host_fallback_waves"] == 0, st


SINGLE = {
    # half the pops are random entries, across 90 heaps
    "dense3d": dict(name="dense3d", n_roots=10, seed=31, iters=3000, bias=0.5),
    "triang_star": dict(name="triang", n_roots=4, seed=32, iters=3000, bias=0.95, optimize=True),
    "dense3d_coarse": dict(name="dense3d_coarse", n_roots=5, seed=4, iters=2500, bias=0.95),
}
SINGLE_NODES = {"dense3d": 1108, "triang_star": 865, "dense3d_coarse": 621}


@pytest.mark.parametrize("case", sorted(SINGLE))
def test_single_forest_equals_the_oracle(S, pool, case):
    job = SINGLE[case]
    fo, fg = pair(S, pool[0], **job)
    assert fo.stats()["n_nodes"] == SINGLE_NODES[case] and fo.stats()["iterations"] == job["iters"]
    fg.run()
    ran_in_the_loop(fg, job["iters"])
    assert_same_forest(fo, fg)
    # without the knob the same job is the host-replay engine's, as before - and the same forest
    _, off = pair(S, pool[1], knob=False, **job)
    assert not off.device_engine()
    off.run()
    assert off.fingerprint() == fg.fingerprint()
    fg.close()
    off.close()


def test_heaps_run_empty_and_fill_again_from_the_closed_list(S, pool):
    """dense2d, six trees: on the way to the end every heap runs empty while the forest is not yet connected - the waves
    then expand nodes of the closed list (one engine word, no tree / heap / coin word), whose children fill the heaps again."""
    job = dict(name="dense2d", n_roots=6, seed=5, iters=6000, bias=0.95)
    fo, fg = pair(S, pool[0], **job)
    so = fo.stats()
    assert so["solved"] and so["iterations"] == 3745 and so["n_nodes"] == 536, so
    # the precondition, on the oracle: stages of 50 waves that end with every node closed (all heaps empty), not solved
    stepped, _unused = member(S, pool[1], job["name"], job["seed"], job["iters"], n_roots=job["n_roots"], priority_bias=job["bias"])
    _unused.close()
    drained, last_drained_nodes = 0, 0
    while True:
        w0 = stepped.stats()["waves"]
        stepped.run(50)
        st = stepped.stats()
        if st["waves"] == w0:
            break
        if st["closed_size"] == st["n_nodes"] and not st["solved"]:
            drained += 1
            last_drained_nodes = st["n_nodes"]
    assert drained == 6 and so["n_nodes"] > last_drained_nodes
    assert stepped.fingerprint() == fo.fingerprint()
    fg.run()
    ran_in_the_loop(fg, so["iterations"])
    assert_same_forest(fo, fg)
    _, off = pair(S, pool[1], knob=False, **job)
    assert not off.device_engine()
    off.run()
    assert off.fingerprint() == fg.fingerprint()
    fg.close()
    off.close()


def test_staged_runs_show_the_heap_order_at_every_stage(S, pool):
    job = dict(name="dense3d", n_roots=10, seed=31, iters=1500, bias=0.5)
    fo, fg = pair(S, pool[0], **job)
    _, twin = pair(S, pool[1], knob=False, **job)       # the host-replay engine, advanced by the same calls
    assert fg.device_engine() and not twin.device_engine()
    stages = 0
    while True:
        w0 = fg.stats()["waves"]
        fg.run(97)
        twin.run(97)
        st = fg.stats()
        assert 0 <= st["waves"] - w0 <= 97 and st["waves"] == twin.stats()["waves"]
        assert len(fg.nodes()["parent"]) == st["n_nodes"] == twin.stats()["n_nodes"]
        front = fg.frontier()       # the first heap of every tree, in heap ARRAY order
        assert len(front) > 0 and front.tolist() == twin.frontier().tolist(), stages
        if st["waves"] == w0:
            break
        stages += 1
    assert stages > 3
    ran_in_the_loop(fg, job["iters"])
    assert_same_forest(fo, fg)
    fg.close()
    twin.close()


def test_a_wave_handed_to_the_host_in_the_middle(S, pool):
    """a hit list of three entries: attempts whose neighbour query overflows it are rolled back and their wave - its node
    popped from its heap, its slot's tree and heap in the control block - is finished by the host-replay engine"""
    job = SINGLE["dense3d_coarse"]
    fo, fg = pair(S, pool[0], SFFGPU_TEST_HITCAP=3, **job)
    fg.run()
    st = fg.stats()
    assert fg.device_engine() and st["host_fallback_waves"] > 0 and st["spec_steps"] == 0, st
    assert_same_forest(fo, fg)
    fg.close()


def test_node_arrays_and_heaps_grow_mid_run(S, pool):
    """no node budget: the store starts at 4 096 nodes, so node arrays and heaps (entries, keys, position maps) are re-grown"""
    job = dict(name="dense3d", n_roots=10, seed=41, iters=12000, bias=0.95)
    fo, fg = pair(S, pool[0], **job)
    assert fo.stats()["n_nodes"] == 4801
    fg.run()
    ran_in_the_loop(fg, job["iters"])
    assert_same_forest(fo, fg)
    fg.close()


BATCH = ([dict(name="dense3d", seed=s, iters=1200, bias=0.95) for s in range(100, 104)] +
         [dict(name="dense3d", seed=s, iters=1200, bias=0.95, optimize=True) for s in (200, 201)] +
         [dict(name="building", seed=s, iters=1200, bias=0.95, optimize=True) for s in (600, 601)] +
         [dict(name="dense2d", seed=s, iters=1200, bias=0.7) for s in (400, 401)] +
         [dict(name="dense3d", seed=s, iters=1200, bias=0.0) for s in (104, 105)])      # plain members ride along


def test_batch_of_priority_and_plain_members(S, pool):
    pairs = [pair(S, pool[i], **job) for i, job in enumerate(BATCH)]
    fos, fgs = [p[0] for p in pairs], [p[1] for p in pairs]
    S.run_batch(fgs)
    for job, fo, fg in zip(BATCH, fos, fgs):
        st = fg.stats()
        assert st["batch_launches"] >= 1 and st["spec_steps"] == 0 and st["host_fallback_waves"] == 0, (job, st)
        assert fo.stats()["n_nodes"] > 40
        assert_same_forest(fo, fg)
    fps = [fg.fingerprint() for fg in fgs]
    assert len(set(fps)) == len(fps)
    for fg in fgs:
        fg.close()
    # staged, and one priority member advanced alone between two calls
    again = [BATCH[0], BATCH[4], BATCH[8], BATCH[10]]
    pairs = [pair(S, pool[i], **job) for i, job in enumerate(again)]
    fos, fgs = [p[0] for p in pairs], [p[1] for p in pairs]
    calls = 0
    while True:
        before = [fg.stats()["waves"] for fg in fgs]
        S.run_batch(fgs, max_waves=97)
        calls += 1
        after = [fg.stats()["waves"] for fg in fgs]
        assert all(0 <= a - b <= 97 for a, b in zip(after, before))
        if after == before:
            break
        if calls == 2:
            w0 = fgs[1].stats()["waves"]
            fgs[1].run(50)
            assert fgs[1].stats()["waves"] == w0 + 50 and fgs[1].stats()["spec_steps"] == 0
    assert calls > 3
    for fo, fg in zip(fos, fgs):
        assert_same_forest(fo, fg)
        fg.close()


def test_refusals_unchanged(S, pool):
    _, by = member(S, pool[0], name="dense3d", seed=100, iters=1500)
    by.run(60)
    fp, waves = by.fingerprint(), by.stats()["waves"]
    _, no_knob = member(S, pool[1], name="dense3d", seed=105, iters=1500, priority_bias=0.5)
    _, goal = member(S, pool[2], name="triang", seed=104, iters=1500, n_roots=2, goal_offset=[12, 8, 5], priority_bias=0.95, **KNOB)
    for other in (no_knob, goal):
        for batch in ([by, other], [other, by]):
            with pytest.raises(S.SffGpuError):
                S.run_batch(batch)
            assert by.fingerprint() == fp and by.stats()["waves"] == waves
    # ... while the same job created under the knob is a member like any other
    fo, ok = pair(S, pool[3], name="dense3d", seed=105, iters=1500, bias=0.5)
    S.run_batch([by, ok])
    assert_same_forest(fo, ok)
    for fg in (by, no_knob, goal, ok):
        fg.close()
