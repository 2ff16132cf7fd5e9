"""The sampling kernels' short chain (csrc/kernels_dev.h sample_fetch / sample_finish, csrc/devforest.hip
append_list_one): k_append_sample takes the next sample's node from the committed round's parent list instead of
looking its slot up, k_sample_steer asks for slot_node[thread] at once when the wave's active list is still the
identity (DevCtrl::act_identity).  Every case builds the forest three times - CPU oracle, the fused chain, and
SFFGPU_NO_FUSED_SAMPLE=1 (one k_sample_steer per round through the slot look-up: the old chain) - and asks for the
same forest node for node.  The shapes are the smallest at which the new paths can go wrong: waves that are no multiple
of 64 / 256 (threads behind the round), the iteration cap inside a round (slots kept out of the committed round), waves
resumed mid-way after a fault (no identity), SFF*, the priority frontier, closed-list picks, libm parity (dv.trig)."""
import pytest

import common
import oracle_lib as O
from test_gpu_device_engine import make, engine
from test_gpu_parity import assert_same_forest, load_world

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import space_filling_forest_star_amd as S
    return S


@pytest.fixture(scope="module")
def ctx(S):
    c = S.Context(0)
    yield c
    c.close()


# One k_sample_steer per round.  Not the old chain to the letter: the first round of a fresh wave takes the identity
# shortcut under the knob too; from the second round on (and in a resumed wave) the slot is looked up in the active list.
OLD_CHAIN = dict(SFFGPU_NO_FUSED_SAMPLE=1)


def both_chains(S, ctx, build, **env):
    """build(**env) -> (oracle forest, GPU forest), not run yet.  Runs the oracle once, the GPU forest on the fused
    chain and on the old one; returns the oracle and the two GPU runs' stats."""
    fo, fg = build(**env)
    fo.run()
    fg.run()
    assert fg.device_engine()
    assert_same_forest(fo, fg)
    fp, new = fg.fingerprint(), fg.stats()
    fg.close()
    _, fk = build(**dict(env, **OLD_CHAIN))
    fk.run()
    assert fk.device_engine()
    assert_same_forest(fo, fk)
    assert fk.fingerprint() == fp == fo.fingerprint()
    old = fk.stats()
    fk.close()
    for k in ("collide_calls", "path_free_calls", "nn_queries", "waves", "slow_path_samples"):
        assert new[k] == old[k], (k, new[k], old[k])
    return fo, new, old


@pytest.mark.parametrize("name,wave,iters", [("dense3d", 192, 6000), ("triang", 300, 5000)])
def test_waves_that_are_no_multiple_of_the_workgroup(S, ctx, name, wave, iters):
    """the last workgroup of both kernels has threads behind the round (i >= n): clamped loads, no sample"""
    fo, _, _ = both_chains(S, ctx, lambda **e: make(S, ctx, name, wave, iters, seed=3, **e))
    assert fo.stats()["n_nodes"] > 40


def test_iteration_cap_inside_a_round(S, ctx):
    """1 003 iterations at waves of 70 slots: the cap keeps slots out of a round while the sampler runs - they stay on
    the list behind the still-failing ones and have no entry in the committed round's parent list"""
    fo, _, _ = both_chains(S, ctx, lambda **e: make(S, ctx, "dense3d", 70, 1003, seed=8, **e))
    assert fo.stats()["iterations"] == 1003


@pytest.mark.parametrize("env", [dict(SFFGPU_TEST_HITCAP=3), dict(SFFGPU_TEST_HITCAP=3, SFFGPU_NO_ORDER=1)])
def test_waves_resumed_after_a_fault(S, ctx, env):
    """a bounded list overflows, the host finishes the round and the device engine resumes the wave mid-way: the active
    list is no identity then, k_sample_steer has to look the slots up"""
    _, new, old = both_chains(S, ctx, lambda **e: make(S, ctx, "dense3d_coarse", 256, 12000, seed=4, **e), **env)
    assert new["slow_path_samples"] > 0 and old["slow_path_samples"] > 0      # the fault path ran


def test_sff_star(S, ctx):
    """SFF*: the accepted samples are appended by the star stage, the sampler runs behind it"""
    fo, _, _ = both_chains(S, ctx, lambda **e: make(S, ctx, "dense3d", 256, 8000, seed=5, optimize=True, **e))
    assert fo.stats()["n_nodes"] > 300


def prio_pair(S, ctx, **env):
    sc, w = load_world(ctx, "dense3d")
    roots = common.free_roots(w.collide, sc["limits"], 6, seed=22, dim=6)
    kw = dict(dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"], dim=6, max_iterations=2 ** 31 - 1,
              node_budget=20000, wave=256, seed=22, priority_bias=0.95)
    fo = O.Forest(w, roots, sc["limits"], **kw)
    with engine(SFFGPU_PRIO_DEVICE=1, **env):
        fg = S.Forest(ctx, roots, sc["limits"], **kw)
    return fo, fg


@pytest.mark.parametrize("env", [dict(SFFGPU_PRIO_SEQ=1), dict()])
def test_priority_frontier(S, ctx, env):
    """priority mode, waves of 256 slots to a 20 000-node budget: the slots (and the identity list) are written by
    k_prio_begin (SFFGPU_PRIO_SEQ=1: the picks one after the other) or by k_prio_plan, their nodes by k_prio_pops"""
    fo, new, _ = both_chains(S, ctx, lambda **e: prio_pair(S, ctx, **e), **env)
    assert fo.stats()["n_nodes"] > 10000
    if env:
        assert new["prio_seq_waves"] == new["waves"] > 0      # (k_prio_begin's sequential picks ran, in every wave)


def test_saturating_forest_with_closed_list_picks(S, ctx):
    """coarse steps at waves of 200 slots: the frontier runs empty and the waves pick from the closed list (no claims at
    the wave's end, the same node in many slots) until every tree is connected"""
    fo, _, _ = both_chains(S, ctx, lambda **e: make(S, ctx, "dense3d_coarse", 200, 10 ** 7, seed=2, **e))
    so = fo.stats()
    assert so["solved"] == 1 and so["frontier_size"] == 0 and so["closed_size"] > 100


def libm_pair(S, ctx, **env):
    sc, _ = load_world(ctx, "dense3d")
    wl = O.World(sc["env"], sc["robot"], O.TRIG_LIBM)
    roots = common.free_roots(wl.collide, sc["limits"], 5, seed=9, dim=6)
    kw = dict(dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"], dim=6, max_iterations=4000, wave=64, seed=9)
    fo = O.Forest(wl, roots, sc["limits"], **kw)
    with engine(SFFGPU_ENGINE="device", **env):
        fg = S.Forest(ctx, roots, sc["limits"], libm_sampling=True, **kw)
    return fo, fg


def test_libm_parity_mode(S, ctx):
    """libm_sampling at waves of 64 slots on the device engine: the host's cos / sin / acos values of the engine words
    (DevRound::trig) are fetched with the words"""
    fo, _, _ = both_chains(S, ctx, lambda **e: libm_pair(S, ctx, **e))
    assert fo.stats()["n_nodes"] > 100
