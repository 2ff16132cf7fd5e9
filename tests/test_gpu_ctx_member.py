"""Member contexts (sffgpu_create_member / Context.member()): contexts that share ONE uploaded environment - nothing is
uploaded or built for them - and carry no round grid until a round engine needs one.  The world is loaded once on an owner;
every planner on a member is compared with the CPU oracle the way the batch tests compare (bit-equal fp64), and the memory
figures are the exact ones of Context.memory()."""
import numpy as np
import pytest

import common
import oracle_lib as O
from test_gpu_boundaries import edges_ref, tangent_ref
from test_gpu_device_engine import engine
from test_gpu_forest_batch import _oracle_runs
from test_gpu_parity import assert_same_forest, load_world
from test_gpu_rrt_batch import assert_same_session, run_oracles

pytestmark = pytest.mark.gpu

ERR_STATE = r"sffgpu error -3"      # SFFGPU_ERR_STATE, as Context._chk words it


@pytest.fixture(scope="module")
def S():
    import space_filling_forest_star_amd as S
    return S


@pytest.fixture(scope="module")
def shared(S):
    """dense3d (dense3d_coarse is the same two meshes with longer steps), uploaded ONCE: the owner and six members.
    The forest batch below has seven jobs and a context owns one node store, hence six."""
    owner = S.Context(0)
    load_world(owner, "dense3d")
    members = [owner.member() for _ in range(6)]
    yield dict(owner=owner, members=members, all=[owner] + members)
    for c in members + [owner]:
        c.close()


def forest(S, ctx, name, seed, iters, optimize=False, wave=1, oracle=True, **env):
    """test_gpu_forest_batch.member without its upload: the scenario's meshes are already on ctx (its own, or its owner's).
    The oracle gets a world of its own, as there: a World counts the calls of everything that runs on it"""
    sc = common.scenario(name)
    w = O.World(sc["env"], sc["robot"], O.TRIG_PORTABLE)
    roots = common.free_roots(w.collide, sc["limits"], 5, seed=seed, dim=sc["dim"])
    kw = dict(dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"], dim=sc["dim"], max_iterations=iters,
              wave=wave, seed=seed, optimize=optimize)
    key = (name, seed, iters, optimize, None)
    fo = None
    if oracle and wave == 1 and key in _oracle_runs:
        fo = _oracle_runs[key]
    elif oracle:
        fo = O.Forest(w, roots, sc["limits"], **kw)
        fo.run()
        if wave == 1:
            _oracle_runs[key] = fo
    with engine(SFFGPU_ENGINE="device", **env):
        fg = S.Forest(ctx, roots, sc["limits"], **kw)
    return fo, fg


BATCH_JOBS = [dict(name="dense3d", seed=s, iters=600) for s in range(100, 104)] + \
             [dict(name="dense3d", seed=s, iters=600, optimize=True) for s in (200, 201)]
TINY_JOB = dict(name="dense3d", seed=7, iters=300)


# ------------------------------------------------------------------------------------------------ 1. same answers
def random_queries(name):
    sc = common.scenario(name)
    poses = np.vstack([common.random_poses(sc["limits"], 200, 5), common.poses_near_surface(sc["env"], 300, 6, 0.4 * sc["scale"])])
    a = common.poses_near_surface(sc["env"], 300, 8, 3.0 * sc["scale"])
    rs = np.random.RandomState(9)
    d = rs.normal(0, 1, (len(a), 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    b = a.copy()
    b[:, :3] += d * sc["sampling_dist"] * rs.uniform(0.01, 1.5, (len(a), 1))
    b[:, 3:] = a[:, 3:] + rs.uniform(-0.5, 0.5, (len(a), 3))
    b[0] = a[0]                                  # degenerate edges: zero length, shorter than one step
    b[1, :3] = a[1, :3] + 1e-3
    return sc, poses, a, b


def same_bytes(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("name", ["dense3d", "building"])
def test_member_answers_equal_the_owners(S, name):
    sc, poses, a, b = random_queries(name)
    owner = S.Context(0)
    owner.upload_env(sc["env"])
    owner.upload_robot(sc["robot"])
    assert owner.memory()["env_holders"] == 1
    member = owner.member()
    mo, mm = owner.memory(), member.memory()
    assert mo["env_bytes"] > 0 and mm["env_bytes"] == 0
    assert mo["env_holders"] == 2 and mm["env_holders"] == 2
    assert mm["total_bytes"] == mm["store_bytes"] + mm["grid_bytes"] + mm["round_grid_bytes"] + mm["other_bytes"]
    assert mo["total_bytes"] == mo["env_bytes"] + mo["store_bytes"] + mo["grid_bytes"] + mo["round_grid_bytes"] + mo["other_bytes"]
    ho, hm = owner.collide_poses(poses), member.collide_poses(poses)
    assert same_bytes(ho, hm) and 0.05 < ho.mean() < 0.95
    w = O.World(sc["env"], sc["robot"], O.TRIG_PORTABLE)
    assert np.array_equal(hm, w.collide_many(poses))
    so, sm = owner.collide_segments(a, b), member.collide_segments(a, b)
    for x, y in zip(so, sm):
        assert same_bytes(x, y)
    assert 0.02 < so[0].mean() < 0.98
    grand = member.member()                      # a member of a member holds the same models
    assert grand.memory()["env_holders"] == 3 and grand.memory()["env_bytes"] == 0
    assert same_bytes(grand.collide_poses(poses), ho)
    for c in (owner, grand, member):
        c.close()


def test_member_answers_on_the_boundary_cases(S):
    """tests/boundary_cases.py: robots that touch a triangle with one vertex / stand 1e-6 off it, at the origin and at 2^20,
    and edges whose first contact is sample 1, 8, 9, 10 or 20 - owner, member and the definition's answers"""
    robot = common.scenario("dense3d")["robot"]
    for offset in (0.0, 2.0 ** 20):
        for shape in ("tip", "flat"):
            for gap in (0.0, 2.0 ** -44, 1e-6):
                poses, env, brute = tangent_ref("dense3d", 256, gap, offset, shape)
                owner = S.Context(0)
                owner.upload_env(env)
                owner.upload_robot(robot)
                member = owner.member()
                ho, hm = owner.collide_poses(poses), member.collide_poses(poses)
                assert same_bytes(ho, hm) and np.array_equal(hm, brute), (offset, shape, gap)
                member.close()
                owner.close()
        for gap in (0.0, 1e-6):
            a, b, env, ks, want = edges_ref("dense3d", gap, offset, "tip")
            owner = S.Context(0)
            owner.upload_env(env)
            owner.upload_robot(robot)
            member = owner.member()
            so, sm = owner.collide_segments(a, b), member.collide_segments(a, b)
            for x, y in zip(so, sm):
                assert same_bytes(x, y)
            assert np.array_equal(np.stack(sm, axis=1).astype(np.int64), want), (offset, gap)
            owner.close()                        # (the owner first)
            member.close()


# ------------------------------------------------------------------------------------------------ 2. forest batch
def test_a_refused_create_leaves_no_hip_error_behind(S, shared):
    """sffgpu_create of a device that does not exist must not touch HIP with that index: an error it left on the thread
    would surface in the next call that asks for the last error - a batch launch"""
    import ctypes as C
    h = C.c_void_p()
    assert S.lib().sffgpu_create(99, C.byref(h)) < 0 and not h.value
    fo, fg = forest(S, shared["owner"], **TINY_JOB)
    S.run_batch([fg])
    assert_same_forest(fo, fg)
    fg.close()


def test_forest_batch_on_shared_contexts(S, shared):
    pairs = [forest(S, shared["owner"], **TINY_JOB)]
    pairs += [forest(S, c, **job) for c, job in zip(shared["members"], BATCH_JOBS)]
    fos, fgs = [p[0] for p in pairs], [p[1] for p in pairs]
    lean = shared["members"][0].memory()         # (a fresh context with its first forest: compared with a plain one below)
    S.run_batch(fgs)
    assert fgs[0].stats()["n_nodes"] == 117
    for fo, fg in zip(fos, fgs):
        st = fg.stats()
        assert st["batch_launches"] >= 1 and st["spec_steps"] == 0 and st["host_fallback_waves"] == 0, st
        assert fo.stats()["n_nodes"] > 40
        assert_same_forest(fo, fg)
    fps = [fg.fingerprint() for fg in fgs]
    assert len(set(fps)) == len(fps), "two members of the batch are the same forest"
    for c in shared["members"]:
        m = c.memory()
        print("member context after a wave-1 batch:", m)
        assert m["round_grid_bytes"] == 0 and m["env_bytes"] == 0 and m["env_holders"] == 7
        assert m["grid_bytes"] > 0 and m["store_bytes"] > 0
    # a context of sffgpu_create with a forest of the same batch has both grids, as it always had
    mo = shared["owner"].memory()
    print("owner context after the same batch:", mo)
    assert mo["round_grid_bytes"] > 0 and mo["env_bytes"] > 0
    for fg in fgs:
        fg.close()
    plain = S.Context(0)
    load_world(plain, "dense3d")
    fo, fg = forest(S, plain, **BATCH_JOBS[0])
    full = plain.memory()
    assert full["round_grid_bytes"] > 0 and full["grid_bytes"] == lean["grid_bytes"] and full["store_bytes"] == lean["store_bytes"]
    S.run_batch([fg])
    assert_same_forest(fo, fg)
    fg.close()
    plain.close()


# ------------------------------------------------------------------------------------------------ 3. the owner goes first
def test_members_outlive_their_owner(S):
    owner = S.Context(0)
    load_world(owner, "dense3d")
    members = [owner.member(), owner.member()]
    assert members[0].memory()["env_holders"] == 3
    owner.close()
    assert [m.memory()["env_holders"] for m in members] == [2, 2]
    pairs = [forest(S, c, **job) for c, job in zip(members, BATCH_JOBS[:2])]
    S.run_batch([p[1] for p in pairs])
    for fo, fg in pairs:
        assert fg.stats()["batch_launches"] >= 1
        assert_same_forest(fo, fg)
        fg.close()
    assert members[0].memory()["env_holders"] == 2
    late = members[1].member()                   # ... and a member can still be an owner
    assert late.memory()["env_holders"] == 3
    members[1].close()
    members[0].close()
    fo, fg = forest(S, late, **BATCH_JOBS[1])
    fg.run()
    assert_same_forest(fo, fg)
    fg.close()
    assert late.memory()["env_holders"] == 1
    late.close()


# ------------------------------------------------------------------------------------------------ 4. the round grid arrives when needed
def test_round_grid_arrives_with_a_faulted_wave(S, shared):
    """the faulting member of test_gpu_forest_batch.test_batch_member_that_faults_to_the_host_path (a hit list of three
    entries hands single waves to the host-replay engine, which works through the round grid) beside a plain member"""
    a_ctx, b_ctx = shared["members"][0], shared["members"][1]
    fo_a, fa = forest(S, a_ctx, name="dense3d_coarse", seed=4, iters=6000, SFFGPU_TEST_HITCAP=3)
    fo_b, fb = forest(S, b_ctx, **BATCH_JOBS[0])
    assert a_ctx.memory()["round_grid_bytes"] == 0 and b_ctx.memory()["round_grid_bytes"] == 0
    S.run_batch([fa, fb])
    assert fa.stats()["host_fallback_waves"] > 0 and fb.stats()["host_fallback_waves"] == 0
    assert a_ctx.memory()["round_grid_bytes"] > 0
    assert b_ctx.memory()["round_grid_bytes"] == 0
    assert_same_forest(fo_a, fa)
    assert_same_forest(fo_b, fb)
    fa.close()
    fb.close()


@pytest.mark.parametrize("optimize", [False, True])
def test_round_grid_arrives_with_a_wave_of_many_slots(S, shared, optimize):
    ctx = shared["members"][2 + int(optimize)]
    assert ctx.memory()["round_grid_bytes"] == 0
    fo, fg = forest(S, ctx, name="dense3d", seed=110, iters=1500, wave=64, optimize=optimize)
    assert ctx.memory()["round_grid_bytes"] == 0     # (not with the forest: with its first wave)
    fg.run()
    assert fg.device_engine() and fg.stats()["host_fallback_waves"] == 0
    assert_same_forest(fo, fg)
    m = ctx.memory()
    assert m["round_grid_bytes"] > 0 and m["env_bytes"] == 0
    fg.close()


def test_round_grid_arrives_on_a_context_that_was_lean(S, shared):
    ctx = shared["members"][4]
    fo, fg = forest(S, ctx, **BATCH_JOBS[1])
    fg.run(40)
    assert fg.stats()["waves"] == 40
    assert ctx.memory()["round_grid_bytes"] == 0
    fg.run()                                     # (to the end on the one-wavefront loop: still lean)
    assert_same_forest(fo, fg)
    assert ctx.memory()["round_grid_bytes"] == 0
    fg.close()
    fo, fg = forest(S, ctx, name="dense3d", seed=110, iters=1500, wave=64)
    fg.run(3)
    grown = ctx.memory()["round_grid_bytes"]
    assert grown > 0
    fg.run()
    assert_same_forest(fo, fg)
    fg.close()
    # a forest that follows on the same context finds the grid it has (a re-celling keeps the state)
    fo, fg = forest(S, ctx, **BATCH_JOBS[1])
    assert ctx.memory()["round_grid_bytes"] >= grown
    fg.run()
    assert_same_forest(fo, fg)
    fg.close()


def test_round_grid_arrives_with_the_host_round_protocol(S, shared):
    """sffgpu_forest_round_begin / _commit (the multi-GPU protocol with one rank) on a member context"""
    ctx = shared["members"][5]
    assert ctx.memory()["round_grid_bytes"] == 0
    sc = common.scenario("dense3d")
    w = O.World(sc["env"], sc["robot"], O.TRIG_PORTABLE)
    roots = common.free_roots(w.collide, sc["limits"], 5, seed=110, dim=6)
    kw = dict(dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"], dim=6, max_iterations=1500, wave=64, seed=110)
    fo = O.Forest(w, roots, sc["limits"], **kw)
    fo.run()
    with engine(SFFGPU_ENGINE="host"):
        fg = S.Forest(ctx, roots, sc["limits"], **kw)
    fg.run()
    assert not fg.device_engine()
    assert_same_forest(fo, fg)
    assert ctx.memory()["round_grid_bytes"] > 0
    fg.close()


# ------------------------------------------------------------------------------------------------ 5. sessions and smoothing
def session(S, ctx, seed, iters, optimize=False, n_roots=1):
    """test_gpu_rrt_batch.member without its upload (dense3d); the oracle gets a world of its own (run_oracles runs them
    on threads)"""
    sc = common.scenario("dense3d")
    w = O.World(sc["env"], sc["robot"], O.TRIG_PORTABLE)
    pts = common.free_roots(w.collide, sc["limits"], max(6, n_roots), seed=seed, dim=sc["dim"])
    kw = dict(dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"], dim=sc["dim"], optimize=optimize, goal=None,
              priority_bias=0.0, max_iterations=iters, seed=seed, lazy_edge=False)
    ro = O.Rrt(w, pts[:n_roots], sc["limits"], **kw)
    rg = S.Rrt(ctx, pts[:n_roots], sc["limits"], wave=0, **kw)
    rg.n_trees = n_roots
    return ro, rg


def test_session_batch_and_smoothing_on_shared_contexts(S, shared):
    """RRT, RRT* and two Multi-T-RRT: the smallest dense3d jobs of tests/test_gpu_rrt_batch.py"""
    specs = [dict(seed=7, iters=300), dict(seed=200, iters=1500, optimize=True),
             dict(seed=3, iters=1500, n_roots=5), dict(seed=306, iters=1200, optimize=True, n_roots=3)]
    pairs = [session(S, c, **sp) for c, sp in zip(shared["all"], specs)]
    run_oracles([p[0] for p in pairs])
    rgs = [p[1] for p in pairs]
    S.run_rrt_batch(rgs)
    for sp, (ro, rg) in zip(specs, pairs):
        st = rg.stats()
        assert st["iterations"] == sp["iters"] and st["batch_launches"] >= 1 and st["waves"] == 0, (sp, st)
        # (min_nodes: test_gpu_rrt_batch's bound for the 300-iteration job, and its usual one)
        assert_same_session(ro, rg, min_nodes=5 if sp["iters"] == 300 else 30)
        if rg.n_trees == 1:                      # (assert_same_session has extracted the paths of the others, on both sides)
            rg.paths(1)
            ro.paths(1)
    plans = S.smooth_rrt_batch(rgs)
    assert len(plans) == len(rgs)
    for (ro, rg), got in zip(pairs, plans):
        want = ro.smooth()
        assert len(want) == len(got)
        for x, y in zip(want, got):
            assert np.array_equal(x, y)
        for k in ("path_free_calls", "collide_calls"):
            assert ro.stats()[k] == rg.stats()[k], k
    for c in shared["members"][:3]:
        assert c.memory()["env_bytes"] == 0
    for rg in rgs:
        rg.close()


def smoothed(fg):
    n = fg.stats()["n_trees"]
    return dict(plans={(i, j): fg.plan(i, j).tobytes() for i in range(n) for j in range(i + 1, n)},
                counters=tuple(fg.stats()[k] for k in ("path_free_calls", "collide_calls")))


def test_smooth_batch_on_shared_contexts(S, shared):
    """the forests of the batch test's shape (at 600 iterations their trees have not met: members without a path) and one of
    dense3d_coarse whose five trees are all connected, through S.smooth_batch; each equals a twin - same job, run alone -
    smoothed by its own single call, as test_gpu_smooth_batch.test_mixed_batch compares"""
    jobs = BATCH_JOBS + [dict(name="dense3d_coarse", seed=2, iters=3000)]
    ctxs = shared["members"] + [shared["owner"]]
    fgs = [forest(S, c, oracle=False, **job)[1] for c, job in zip(ctxs, jobs)]
    S.run_batch(fgs)
    raw = [fg.paths()[0] for fg in fgs]
    mats = S.smooth_batch(fgs)
    got = [smoothed(fg) for fg in fgs]
    off = ~np.eye(5, dtype=bool)
    assert int((raw[-1][off] < 1e300).sum()) == 12, "the coarse forest has paths to smooth"
    assert np.any(mats[-1][off] < raw[-1][off] - 1e-6)
    assert fgs[-1].smooth_stats()["launches"] >= 1 and fgs[-1].smooth_stats()["edges"] > 0
    for fg in fgs:
        fg.close()
    for c, job, d, g in zip(ctxs, jobs, mats, got):
        twin = forest(S, c, oracle=False, **job)[1]
        twin.run()
        twin.paths()
        dt = twin.smooth()
        assert twin.smooth_stats()["launches"] == 0
        assert np.array_equal(dt, d), job
        assert smoothed(twin) == g, job
        twin.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals(S):
    sc = common.scenario("dense3d")
    owner = S.Context(0)
    owner.upload_env(sc["env"])
    with pytest.raises(S.SffGpuError, match=ERR_STATE):
        owner.member()                           # one mesh only: a member of half a world has no use
    only_robot = S.Context(0)
    only_robot.upload_robot(sc["robot"])
    with pytest.raises(S.SffGpuError, match=ERR_STATE):
        only_robot.member()
    only_robot.close()
    owner.upload_robot(sc["robot"])
    member = owner.member()
    poses = common.poses_near_surface(sc["env"], 300, 6, 0.4)
    before = owner.collide_poses(poses)
    for c in (owner, member):
        with pytest.raises(S.SffGpuError, match=ERR_STATE):
            c.upload_env(sc["env"][:100])
        with pytest.raises(S.SffGpuError, match=ERR_STATE):
            c.upload_robot(sc["robot"])
    assert owner.memory()["env_holders"] == 2
    assert np.array_equal(owner.collide_poses(poses), before) and np.array_equal(member.collide_poses(poses), before)
    fo, fg = forest(S, member, **BATCH_JOBS[0])
    fg.run()
    assert_same_forest(fo, fg)
    fg.close()
    assert S.lib().sffgpu_ctx_get_memory(member.h, None) == -1     # SFFGPU_ERR_ARG
    member.close()
    assert owner.memory()["env_holders"] == 1
    owner.upload_env(sc["env"][:100])            # alone again: the upload works
    owner.upload_robot(sc["robot"])
    after = owner.collide_poses(poses)
    w100 = O.World(sc["env"][:100], sc["robot"], O.TRIG_PORTABLE)
    assert np.array_equal(after, w100.collide_many(poses))
    owner.close()
