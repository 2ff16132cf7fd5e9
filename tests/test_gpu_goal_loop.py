"""The single-goal mode (Problem::hasGoal, src/forest.h:91-109,196-201,283-299,369-372) in the loop of waves of ONE slot
(k_seq_waves<., false, true>) and in forest batches (k_seq_waves_batch<., false, true>), for forests created under
SFFGPU_GOAL_LOOP=1.  Every case first asserts, on the CPU oracle, the exact figures of the job (so it cannot pass on a job
that never meets the goal) and then compares with the oracle's sequential run of the same seed through assert_same_forest:
bit-equal fp64 positions and costs, equal parents, the one border, reference-equivalent counters and fingerprint."""
import pytest

from test_gpu_forest_batch import member
from test_gpu_parity import assert_same_forest

pytestmark = pytest.mark.gpu

N_CTX = 16
KNOB = dict(SFFGPU_GOAL_LOOP=1)
GOAL_OFF = {"triang": [12, 8, 5], "building": [12, 8, 5], "dense3d": [30, 25, 8], "dense2d": [300, 200, 0]}


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


def pair(S, ctx, name, seed, iters, n_roots, offset=None, optimize=False, knob=True, shift=None, **env):
    """(oracle after its whole run, the library's forest before its first wave) of one goal job"""
    if knob:
        env = dict(env, **KNOB)
    fo, fg = member(S, ctx, name, seed, iters, optimize=optimize, n_roots=n_roots, goal_offset=offset, shift=shift, **env)
    key = (name, seed, iters, n_roots, tuple(offset), optimize) + (() if shift is None else (tuple(shift),))
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


# job -> (arguments, the oracle's iterations, nodes, waves)
LONE = {
    "triang_1root": (dict(name="triang", n_roots=1), 2381, 546, 785),
    "triang_1root_star": (dict(name="triang", n_roots=1, optimize=True), 2381, 546, 785),
    # two start trees: the other tree's nodes are qualifying neighbours that reject attempts without an edge check
    "triang_2roots": (dict(name="triang", n_roots=2), 1643, 414, 557),
    "triang_2roots_star": (dict(name="triang", n_roots=2, optimize=True), 1643, 414, 557),
    "building": (dict(name="building", n_roots=1), 635, 186, 235),
    "building_star": (dict(name="building", n_roots=1, optimize=True), 635, 186, 235),
    "dense3d_4roots": (dict(name="dense3d", n_roots=4), 2228, 589, 793),
    "dense2d": (dict(name="dense2d", n_roots=2), 453, 72, 126),      # dim 2
}


@pytest.mark.parametrize("case", sorted(LONE))
def test_lone_forest_is_solved_in_the_loop(S, pool, case):
    job, iters, nodes, waves = LONE[case]
    job = dict(job, seed=8, iters=60000, offset=GOAL_OFF[job["name"]])
    fo, fg = pair(S, pool[0], **job)
    so = fo.stats()
    assert (so["solved"], so["iterations"], so["n_nodes"], so["waves"], so["n_borders"]) == (1, iters, nodes, waves, 1), so
    fg.run()
    ran_in_the_loop(fg, iters)
    st = fg.stats()
    assert st["solved"] == 1 and st["n_borders"] == 1, st
    assert_same_forest(fo, fg)
    # without the knob the same job is today's path - the round engine, its solving wave replayed on the host - and the same forest
    _, off = pair(S, pool[1], knob=False, **job)
    off.run()
    assert off.stats()["host_fallback_waves"] >= 1
    assert off.fingerprint() == fg.fingerprint()
    fg.close()
    off.close()


def test_a_goal_that_cannot_be_reached(S, pool):
    """dense2d, the scenario's four start points, a goal pose that collides: its edge check is never free, so the forest is
    never solved - an empty frontier does not solve a goal forest - and once every node is closed the waves expand nodes of
    the closed list, whose children fill the frontier again, until max_iterations."""
    import common
    import oracle_lib as O
    from test_gpu_device_engine import engine
    from test_gpu_parity import load_world
    goal = [867.2352075241184, 1352.519189507453, 0, 0, 0, 0]

    def make(ctx, **env):
        sc, w = load_world(ctx, "dense2d")
        roots = common.scenario("dense2d")["xml_points"][:4]
        kw = dict(dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"], dim=2, max_iterations=6000, wave=1, seed=5, goal=goal)
        with engine(SFFGPU_ENGINE="device", **env):
            fg = S.Forest(ctx, roots, sc["limits"], **kw)
        return O.Forest(w, roots, sc["limits"], **kw), fg

    fo, fg = make(pool[0], **KNOB)
    stepped, twin = make(pool[1])
    fo.run()
    so = fo.stats()
    want = dict(solved=0, iterations=6000, n_nodes=879, waves=1763, frontier_size=0, closed_size=878, n_borders=0, n_connected=1)
    assert {k: so[k] for k in want} == want, so
    # the precondition, on a second oracle forest: stages of 50 waves that end with an empty frontier
    empty, first = 0, None
    while True:
        w0 = stepped.stats()["waves"]
        stepped.run(50)
        st = stepped.stats()
        if st["waves"] == w0:
            break
        if st["frontier_size"] == 0:
            empty += 1
            first = st["waves"] if first is None else first
    assert (empty, first) == (17, 500) and stepped.fingerprint() == fo.fingerprint()
    # the same stages in the loop, against a twin without the knob advanced by the same calls
    empty, first, stages = 0, None, 0
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
        if st["frontier_size"] == 0:
            empty += 1
            first = st["waves"] if first is None else first
    assert (empty, first) == (17, 500)
    ran_in_the_loop(fg, 6000)
    assert_same_forest(fo, fg)
    assert twin.fingerprint() == fg.fingerprint()
    fg.close()
    twin.close()


def test_a_wave_handed_to_the_host_in_the_middle(S, pool):
    """a hit list of three entries: attempts whose neighbour query overflows it are rolled back and their wave is finished by
    the host-replay engine, which knows the goal mode; the forest goes back to the loop and is solved there or on the host,
    wherever the solving wave happens to run.  This 2-root job overflows a hit list of three, so the 3-root variant is not used."""
    job = dict(name="dense3d_coarse", seed=2, iters=60000, n_roots=2, offset=[250, 150, 60])
    fo, fg = pair(S, pool[0], SFFGPU_TEST_HITCAP=3, **job)
    so = fo.stats()
    assert (so["solved"], so["iterations"], so["n_nodes"], so["waves"]) == (1, 1248, 258, 392), so
    fg.run()
    st = fg.stats()
    assert fg.device_engine() and st["host_fallback_waves"] > 0 and st["spec_steps"] == 0, st
    assert_same_forest(fo, fg)
    fg.close()


BATCH = ([dict(name="triang", seed=s, n_roots=2, optimize=bool(s & 1)) for s in range(100, 108)] +
         [dict(name="dense2d", seed=s, n_roots=2) for s in range(400, 404)] +
         [dict(name="building", seed=s, n_roots=1, optimize=True) for s in (600, 601)])
BATCH_ITERS = [5204, 809, 1093, 3205, 2385, 697, 2854, 158, 194, 148, 196, 37, 1571, 1457]
PLAIN = [dict(name="dense3d", seed=s, iters=1200) for s in (104, 105)]      # members without a goal ride along


def batch_members(S, pool, jobs_iters, plain):
    fos, fgs = [], []
    for i, (job, _it) in enumerate(jobs_iters):
        fo, fg = pair(S, pool[i], iters=6000, offset=GOAL_OFF[job["name"]], **job)
        fos.append(fo)
        fgs.append(fg)
    for j, job in enumerate(plain):
        fo, fg = member(S, pool[len(jobs_iters) + j], **job)
        fos.append(fo)
        fgs.append(fg)
    return fos, fgs


def test_batch_of_goal_and_plain_members(S, pool):
    jobs = list(zip(BATCH, BATCH_ITERS))
    fos, fgs = batch_members(S, pool, jobs, PLAIN)
    for (job, iters), fo in zip(jobs, fos):
        so = fo.stats()
        assert so["solved"] == 1 and so["iterations"] == iters and so["n_borders"] == 1, (job, so)
    S.run_batch(fgs)
    for (job, iters), fo, fg in zip(jobs + [(p, p["iters"]) for p in PLAIN], fos, fgs):
        st = fg.stats()
        assert st["iterations"] == iters and st["solved"] == (1 if "n_roots" in job else 0), (job, st)
        assert st["batch_launches"] >= 1 and st["spec_steps"] == 0 and st["host_fallback_waves"] == 0, (job, st)
        assert_same_forest(fo, fg)
    fps = [fg.fingerprint() for fg in fgs]
    assert len(set(fps)) == len(fps)
    for fg in fgs:
        fg.close()
    # staged, one goal member advanced alone between two calls, and one call more after every member has ended
    again = [jobs[0], jobs[3], jobs[7], jobs[8], jobs[12]]
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
            w0 = fgs[1].stats()["waves"]
            fgs[1].run(50)
            assert fgs[1].stats()["waves"] == w0 + 50 and fgs[1].stats()["spec_steps"] == 0
    assert calls > 3
    for fo, fg in zip(fos, fgs):
        assert_same_forest(fo, fg)
    fps = [fg.fingerprint() for fg in fgs]
    stats = [fg.stats() for fg in fgs]
    # a member that has solved its query idles while the others go on: 78 waves are one launch of 97, 1 665 are eighteen
    assert stats[2]["batch_launches"] == 1 and stats[0]["batch_launches"] == 18 == calls - 1, [st["batch_launches"] for st in stats]
    S.run_batch(fgs)                             # nothing left to do
    assert [fg.fingerprint() for fg in fgs] == fps
    for st, fg in zip(stats, fgs):
        now = fg.stats()
        assert all(now[k] == st[k] for k in ("iterations", "waves", "n_nodes", "n_borders", "solved", "batch_launches")), (st, now)
        fg.close()


def test_refusals(S, pool):
    _, by = member(S, pool[0], name="dense3d", seed=100, iters=1500)
    by.run(60)
    fp, waves = by.fingerprint(), by.stats()["waves"]
    job = dict(name="triang", seed=104, iters=6000, n_roots=2, offset=GOAL_OFF["triang"])
    _, no_knob = pair(S, pool[1], knob=False, **job)
    _, prio_goal = member(S, pool[2], name="triang", seed=104, iters=6000, n_roots=2, goal_offset=GOAL_OFF["triang"],
                          priority_bias=0.95, SFFGPU_PRIO_LOOP=1, **KNOB)
    for other in (no_knob, prio_goal):
        for batch in ([by, other], [other, by]):
            with pytest.raises(S.SffGpuError):
                S.run_batch(batch)
            assert by.fingerprint() == fp and by.stats()["waves"] == waves
            assert other.stats()["waves"] == 0
    # ... while the same goal job created under the knob is a member like any other
    fo, ok = pair(S, pool[3], **job)
    assert fo.stats()["solved"] == 1 and fo.stats()["iterations"] == 2385
    S.run_batch([by, ok])
    assert ok.stats()["batch_launches"] >= 1
    assert_same_forest(fo, ok)
    for fg in (by, no_knob, prio_goal, ok):
        fg.close()
