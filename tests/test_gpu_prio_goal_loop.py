"""A forest with BOTH a goal and a priority bias (src/forest.h:104-108: one heap per start tree, keyed by the distance to the
goal; bias 0.95 = greedy best-first search towards it) in the loop of waves of ONE slot (k_seq_waves<., true, true>) and in
forest batches (k_seq_waves_batch<., true, true>), for forests created under SFFGPU_PRIO_GOAL_LOOP=1.  Every case first
asserts, on the CPU oracle, the exact figures of the job (so it cannot pass on a job that never meets the goal) and then
compares with the oracle's sequential run of the same seed through assert_same_forest: bit-equal fp64 positions and costs,
equal parents, the one border, reference-equivalent counters and fingerprint."""
import pytest

from test_gpu_forest_batch import member
from test_gpu_parity import assert_same_forest

pytestmark = pytest.mark.gpu

N_CTX = 20
KNOB = dict(SFFGPU_PRIO_GOAL_LOOP=1)


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


def pair(S, ctx, name, seed, iters, n_roots, offset, bias=0.95, optimize=False, knob=True, shift=None, **env):
    """(oracle after its whole run, the library's forest before its first wave) of one priority + goal job"""
    if knob:
        env = dict(env, **KNOB)
    fo, fg = member(S, ctx, name, seed, iters, optimize=optimize, n_roots=n_roots, goal_offset=offset, priority_bias=bias, shift=shift, **env)
    key = (name, seed, iters, n_roots, tuple(offset), bias, optimize) + (() if shift is None else (tuple(shift),))
    if key not in _oracle:
        fo.run()
        _oracle[key] = fo
    return _oracle[key], fg


def ran_in_the_loop(fg, iters):
    st = fg.stats()
    assert fg.device_engine()
    # the persistent wavefront: one "sweep" per iteration, no step of the speculative kernel, no wave graph of the round engine
    assert st["sweeps"] == st["iterations"] == iters and st["spec_steps"] == 0 and st["graph_launches"] == 0, st
    assert st["host_fallback_waves"] == 0, st


# job -> (arguments, the oracle's iterations, nodes, waves, closed)
LONE = {
    "triang_2roots": (dict(name="triang", n_roots=2, offset=[57, -5, -20]), 400, 167, 182, 18),
    "triang_2roots_star": (dict(name="triang", n_roots=2, offset=[57, -5, -20], optimize=True), 400, 167, 182, 18),
    "triang_3roots_star": (dict(name="triang", n_roots=3, offset=[-25, -64, -20], optimize=True), 1816, 432, 608, 180),
    # bias 0.5: half of the pops take an entry at a drawn index instead of the top
    "triang_2roots_bias_half": (dict(name="triang", n_roots=2, offset=[57, -5, -20], bias=0.5), 1031, 300, 379, 82),
    "building": (dict(name="building", n_roots=1, offset=[57, 54, 62]), 514, 174, 205, 33),
    "building_star": (dict(name="building", n_roots=1, offset=[57, 54, 62], optimize=True), 514, 174, 205, 33),
    "building_far": (dict(name="building", n_roots=1, offset=[88, 57, 92]), 4675, 865, 1378, 515),
    "dense2d_2roots": (dict(name="dense2d", n_roots=2, offset=[-60, -1270, 0]), 565, 103, 168, 68),      # dim 2
    "dense2d_3roots_bias_half": (dict(name="dense2d", n_roots=3, offset=[-60, -1270, 0], bias=0.5), 2578, 361, 710, 353),
    "dense3d_4roots": (dict(name="dense3d", n_roots=4, seed=10, offset=[-1575, 15, -584]), 3464, 1556, 1707, 156),
}


@pytest.mark.parametrize("case", sorted(LONE))
def test_lone_forest_is_solved_in_the_loop(S, pool, case):
    job, iters, nodes, waves, closed = LONE[case]
    job = dict(dict(seed=8, iters=60000), **job)
    fo, fg = pair(S, pool[0], **job)
    so = fo.stats()
    got = (so["solved"], so["iterations"], so["n_nodes"], so["waves"], so["closed_size"], so["n_borders"], so["n_connected"])
    assert got == (1, iters, nodes, waves, closed, 1, 2), so
    fg.run()
    ran_in_the_loop(fg, iters)
    st = fg.stats()
    assert st["solved"] == 1 and st["n_borders"] == 1, st
    assert_same_forest(fo, fg)
    # without the knob the same job is today's path - the host-replay engine - and the same forest, heap order included
    _, off = pair(S, pool[1], knob=False, **job)
    assert not off.device_engine()
    off.run()
    assert off.fingerprint() == fg.fingerprint()
    assert off.frontier().tolist() == fg.frontier().tolist()
    fg.close()
    off.close()


def test_a_goal_that_cannot_be_reached(S, pool):
    """dense2d, the scenario's four start points, a goal pose that collides: its edge check is never free, so the forest is
    never solved.  Every node of the start trees ends on the closed list: whenever every heap has run empty the waves expand
    nodes of the closed list (no heap is popped, nothing is pushed back), whose children fill the heaps again."""
    import common
    import oracle_lib as O
    from test_gpu_device_engine import engine
    from test_gpu_parity import load_world
    goal = [867.2352075241184, 1352.519189507453, 0, 0, 0, 0]

    def make(ctx, **env):
        sc, w = load_world(ctx, "dense2d")
        roots = common.scenario("dense2d")["xml_points"][:4]
        kw = dict(dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"], dim=2, max_iterations=6000, wave=1, seed=5, goal=goal,
                  priority_bias=0.95)
        with engine(SFFGPU_ENGINE="device", **env):
            fg = S.Forest(ctx, roots, sc["limits"], **kw)
        return O.Forest(w, roots, sc["limits"], **kw), fg

    fo, fg = make(pool[0], **KNOB)
    _, twin = make(pool[1])
    assert fg.device_engine() and not twin.device_engine()
    fo.run()
    so = fo.stats()
    want = dict(solved=0, iterations=6000, n_nodes=884, waves=1777, closed_size=883, n_borders=0, n_connected=1)
    assert {k: so[k] for k in want} == want, so
    # stages of 50 waves in the loop, against a twin without the knob advanced by the same calls
    stages = 0
    while True:
        w0 = fg.stats()["waves"]
        fg.run(50)
        twin.run(50)
        st = fg.stats()
        assert 0 <= st["waves"] - w0 <= 50 and st["waves"] == twin.stats()["waves"], stages
        assert fg.frontier().tolist() == twin.frontier().tolist(), stages
        if st["waves"] == w0:
            break
        stages += 1
        assert not st["solved"]
    assert stages == 36                          # 1 777 waves
    assert_same_forest(fo, fg)
    ran_in_the_loop(fg, 6000)
    assert twin.fingerprint() == fg.fingerprint()
    fg.close()
    twin.close()


def test_a_wave_handed_to_the_host_in_the_middle(S, pool):
    """a hit list of three entries: attempts whose neighbour query overflows it are rolled back - the wave's node stays popped
    from its heap - and their wave is finished by the host-replay engine, which knows both modes; the forest goes back to
    the loop and is solved there or on the host, wherever the solving wave happens to run."""
    job = dict(name="dense3d_coarse", seed=2, iters=60000, n_roots=2, offset=[1000, 1900, 250])
    fo, fg = pair(S, pool[0], SFFGPU_TEST_HITCAP=3, **job)
    so = fo.stats()
    assert (so["solved"], so["iterations"], so["n_nodes"], so["waves"]) == (1, 448, 173, 197), so
    fg.run()
    st = fg.stats()
    assert fg.device_engine() and st["host_fallback_waves"] > 0 and st["spec_steps"] == 0, st
    assert_same_forest(fo, fg)
    fg.close()


BATCH = ([dict(name="triang", seed=s, n_roots=2, offset=[57, -5, -20], optimize=bool(s & 1)) for s in range(100, 108)] +
         [dict(name="dense2d", seed=s, n_roots=2, offset=[-60, -1270, 0]) for s in range(400, 404)] +
         [dict(name="building", seed=s, n_roots=1, offset=[57, 54, 62], optimize=True) for s in (600, 601)])
BATCH_ITERS = [291, 189, 264, 323, 336, 346, 459, 400, 1623, 237, 2424, 3601, 6000, 6000]
BATCH_UNSOLVED_NODES = {600: 1030, 601: 1093}
PLAIN = [dict(name="dense3d", seed=s, iters=1200) for s in (104, 105)]      # members of the other kinds ride along
GOAL_ONLY = dict(name="triang", seed=104, iters=6000, n_roots=2, goal_offset=[12, 8, 5], SFFGPU_GOAL_LOOP=1)
PRIO_ONLY = dict(name="dense3d", seed=105, iters=1500, priority_bias=0.5, SFFGPU_PRIO_LOOP=1)


def other_kind(S, ctx, job):
    fo, fg = member(S, ctx, **job)
    if fo.stats()["iterations"] == 0:            # (member() shares the oracles of plain jobs, already run)
        fo.run()
    return fo, fg


def batch_members(S, pool, jobs, others):
    fos, fgs = [], []
    for i, job in enumerate(jobs):
        fo, fg = pair(S, pool[i], iters=6000, **job)
        fos.append(fo)
        fgs.append(fg)
    for j, job in enumerate(others):
        fo, fg = other_kind(S, pool[len(jobs) + j], job)
        fos.append(fo)
        fgs.append(fg)
    return fos, fgs


def test_batch_of_mixed_kinds(S, pool):
    others = PLAIN + [GOAL_ONLY, PRIO_ONLY]
    other_iters = [1200, 1200, 2385, 1500]
    fos, fgs = batch_members(S, pool, BATCH, others)
    for job, iters, fo in zip(BATCH, BATCH_ITERS, fos):
        so = fo.stats()
        if job["seed"] in BATCH_UNSOLVED_NODES:
            assert (so["solved"], so["iterations"], so["n_nodes"]) == (0, 6000, BATCH_UNSOLVED_NODES[job["seed"]]), (job, so)
        else:
            assert so["solved"] == 1 and so["iterations"] == iters and so["n_borders"] == 1, (job, so)
    for iters, fo in zip(other_iters, fos[len(BATCH):]):
        assert fo.stats()["iterations"] == iters, fo.stats()
    assert fos[-2].stats()["solved"] == 1 and fos[-1].stats()["n_nodes"] > 40
    S.run_batch(fgs)
    for job, iters, fo, fg in zip(BATCH + others, BATCH_ITERS + other_iters, fos, fgs):
        st = fg.stats()
        assert st["iterations"] == iters and st["solved"] == fo.stats()["solved"], (job, st)
        assert st["batch_launches"] >= 1 and st["spec_steps"] == 0 and st["host_fallback_waves"] == 0, (job, st)
        assert_same_forest(fo, fg)
    fps = [fg.fingerprint() for fg in fgs]
    assert len(set(fps)) == len(fps)
    for fg in fgs:
        fg.close()
    # staged, one priority + goal member advanced alone between two calls, and one call more after every member has ended
    again = [BATCH[0], BATCH[3], BATCH[8], BATCH[9]]
    fos, fgs = batch_members(S, pool, again, PLAIN[:1])
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
            # (1 623 iterations are 325 waves at least: 2 x 97 + 50 waves do not end this member)
            w0 = fgs[2].stats()["waves"]
            fgs[2].run(50)
            assert fgs[2].stats()["waves"] == w0 + 50 and fgs[2].stats()["spec_steps"] == 0
    assert calls > 3
    for fo, fg in zip(fos, fgs):
        assert fg.stats()["host_fallback_waves"] == 0
        assert_same_forest(fo, fg)
    fps = [fg.fingerprint() for fg in fgs]
    stats = [fg.stats() for fg in fgs]
    S.run_batch(fgs)                             # nothing left to do
    assert [fg.fingerprint() for fg in fgs] == fps
    for st, fg in zip(stats, fgs):
        now = fg.stats()
        assert all(now[k] == st[k] for k in ("iterations", "waves", "n_nodes", "n_borders", "solved", "batch_launches")), (st, now)
        fg.close()


def test_refusals_and_opt_in(S, pool):
    _, by = member(S, pool[0], name="dense3d", seed=100, iters=1500)
    by.run(60)
    fp, waves = by.fingerprint(), by.stats()["waves"]
    job = dict(name="triang", seed=104, iters=6000, n_roots=2, offset=[57, -5, -20], optimize=False)
    # the knobs of the two single modes together do not cover the combination
    _, single_knobs = pair(S, pool[1], knob=False, SFFGPU_PRIO_LOOP=1, SFFGPU_GOAL_LOOP=1, **job)
    # the loop switched off: the new knob alone does not put the forest on the device engine
    _, no_seq = pair(S, pool[2], SFFGPU_NO_SEQ=1, **job)
    assert not single_knobs.device_engine() and not no_seq.device_engine()
    for other in (single_knobs, no_seq):
        for batch in ([by, other], [other, by]):
            with pytest.raises(S.SffGpuError):
                S.run_batch(batch)
            assert by.fingerprint() == fp and by.stats()["waves"] == waves
            assert other.stats()["waves"] == 0
    # ... while the same job created under the new knob alone is a member like any other
    fo, ok = pair(S, pool[3], **job)
    assert fo.stats()["solved"] == 1 and fo.stats()["iterations"] == 336
    assert ok.device_engine()
    S.run_batch([by, ok])
    assert ok.stats()["batch_launches"] >= 1 and ok.stats()["host_fallback_waves"] == 0
    assert_same_forest(fo, ok)
    for fg in (by, single_knobs, no_seq, ok):
        fg.close()


def test_a_wave_the_caller_left_half_done(S, pool):
    """a caller that drives rounds itself (round_begin / round_commit: the host-replay engine) may leave a wave half done, its
    node popped from its heap; run() and run_batch() finish that wave on the host-replay engine - the round engine has no
    priority + goal - and go on in the loop"""
    job = dict(name="triang", seed=8, iters=60000, n_roots=2, offset=[57, -5, -20])
    _, by = member(S, pool[2], name="dense3d", seed=100, iters=1500)
    for ctx, finish in ((pool[0], lambda fg: fg.run()), (pool[1], lambda fg: S.run_batch([by, fg]))):
        fo, fg = pair(S, ctx, **job)
        assert fo.stats()["iterations"] == 400
        fg.run(20)
        for _ in range(100):                     # (a wave is half done when its first attempt was not accepted)
            rec, done = fg.round_begin()
            assert not done
            fg.round_commit(rec, [len(rec)])
            if fg.in_wave():
                break
        assert fg.in_wave()
        finish(fg)
        st = fg.stats()
        assert fg.device_engine() and st["graph_launches"] == 0 and st["spec_steps"] == 0 and not fg.in_wave(), st
        assert_same_forest(fo, fg)
        fg.close()
    by.close()
