"""The commit's hand-off (plain SFF on the device engine): k_commit ends at its walks, the append launch's finalize
block writes the control block, and every other workgroup of that launch derives the committed round's and the next
round's scalars from the block as the commit found it plus the round's totals (csrc/commit_next.h).

Every case builds the forest on the CPU oracle and on the device engine and asks for the same forest node for node
(nodes, borders, fingerprint: assert_same_forest) and for the oracle's counters - they come out of the finalize block.
The shapes are the smallest at which the hand-off can go wrong: one / two commit workgroups, one / two append blocks,
the iteration cap and the node budget inside a round, rolled-back rounds, capacity faults and resumed waves, the
wave's end from the frontier and from the closed list."""
import re

import pytest

from test_gpu_device_engine import engine, make
from test_gpu_parity import assert_same_forest, load_world  # noqa: F401  (load_world: what make() builds its worlds with)

pytestmark = pytest.mark.gpu

COUNTERS = ("collide_calls", "path_free_calls", "nn_queries", "waves", "iterations")


@pytest.fixture(scope="module")
def S():
    import space_filling_forest_star_amd as S
    return S


@pytest.fixture(scope="module")
def ctx(S):
    c = S.Context(0)
    yield c
    c.close()


def same(fo, fg):
    assert_same_forest(fo, fg)
    so, sg = fo.stats(), fg.stats()
    for k in COUNTERS:
        assert so[k] == sg[k], (k, so[k], sg[k])


def both(S, ctx, *a, **kw):
    fo, fg = make(S, ctx, *a, **kw)
    fo.run()
    fg.run()
    assert fg.device_engine()
    same(fo, fg)
    return fo, fg


@pytest.mark.parametrize("name", ["dense3d", "triang"])
@pytest.mark.parametrize("wave", [40, 65, 192, 257, 300])
def test_workgroup_boundaries(S, ctx, name, wave):
    """40 slots: one commit workgroup, one append block; 65: two commit workgroups (two lines to add up); 192: three;
    257 and 300: two append blocks of each kind, five workgroup lines.  In every one of these runs the last round of a
    wave is applied by k_append (no next round to draw): it posts the exhausted slots' claims and sets claims_done
    beside the finalize block's write-back - the wave's end skips its own claim pass, and the forest is the oracle's."""
    fo, _ = both(S, ctx, name, wave, 5000, seed=3)
    assert fo.stats()["n_nodes"] > 40 and fo.stats()["waves"] > 3


def test_iteration_cap_inside_a_round(S, ctx):
    """1003 iterations at waves of 70 slots: the derived size of the next round is cut by max_iterations - iter, and the
    slots the cap kept out stay on the list behind the failing ones"""
    fo, fg = both(S, ctx, "dense3d", 70, 1003, seed=8)
    assert fo.stats()["iterations"] == fg.stats()["iterations"] == 1003


def test_node_budget_reached_inside_a_wave(S, ctx):
    """a budget 300 nodes above the 5 roots at waves of 256: the wave's end reads the node count from the written block"""
    fo, fg = both(S, ctx, "dense3d", 256, 10 ** 7, seed=5, budget=305)
    assert fg.stats()["n_nodes"] >= 305 and fg.stats()["waves"] >= 2


@pytest.mark.parametrize("env", [dict(), dict(SFFGPU_NO_ORDER=1)])
def test_faulted_round_is_rolled_back_by_the_finalize_block(S, ctx, env):
    """hit lists of 3 entries overflow: the round's fault flag is up when k_commit ends, the finalize block rolls the round
    back and clears the flag, the append side applies nothing, the host redoes the round"""
    fo, fg = both(S, ctx, "dense3d_coarse", 256, 12000, seed=4, SFFGPU_TEST_HITCAP=3, **env)
    assert fg.stats()["slow_path_samples"] > 0


@pytest.mark.parametrize("wave,iters,seed,nodes,borders", [(256, 26000, 6, 3000, 300), (192, 10000, 9, 1400, 64)])
def test_growth_faults_from_the_derived_scalars(S, ctx, wave, iters, seed, nodes, borders):
    """no node budget (the store starts at 4096 nodes) and a border list of 64 entries: capacity and border-table faults
    are raised by the finalize block's sizing of the next round, the host grows the arrays, k_wave_begin resumes the wave
    from the written block.  The sizing uses the border count before the round + every event of the round: a workgroup
    that took the count from the block's n_borders word - which the launch's own border_finalize rewrites - would size
    the round before a capacity fault differently from the finalize block.  The second job (three commit workgroups,
    another seed) ends with more borders than the list first held (the oracle's figures: 1478 nodes, 95 borders)."""
    fo, _ = both(S, ctx, "dense3d_coarse", wave, iters, seed=seed, SFFGPU_TEST_BORDER_CAP=64)
    assert fo.stats()["n_nodes"] > nodes and fo.stats()["n_borders"] > borders


MATE_CASE = ("dense3d_coarse", 256, 12000, 4, 5)      # world, wave, iterations, seed, roots
MATE_EVENTS = re.compile(r"border events with a neighbour accepted in the same round (\d+)")


def test_border_event_whose_neighbour_was_accepted_in_the_same_round(S, ctx, capfd):
    """The one consumer of the id prefix left inside k_commit: the event's stamp needs the new node's id.  That the run
    reaches the path is read off the device: under SFFGPU_PROFILE k_commit counts these events (DevCtrl::prof[4], the
    last figure of the profile line a run prints).  A scan over dense3d, triang and dense3d_coarse at waves of 64 to
    4096 slots found none in the first two worlds and 4 such events in this job (6 at waves of 1024): the test reads
    the figure again and asserts it."""
    name, wave, iters, seed, n_roots = MATE_CASE
    fo, fg = make(S, ctx, name, wave, iters, seed=seed, n_roots=n_roots, SFFGPU_PROFILE=1)
    fo.run()
    capfd.readouterr()
    fg.run()
    err = capfd.readouterr().err
    found = MATE_EVENTS.findall(err)
    assert found and int(found[-1]) > 0, err[-2000:]
    same(fo, fg)


def test_wave_ends_with_closed_list_picks(S, ctx):
    """a saturating forest at waves of 200 slots: the frontier runs empty, the waves pick from the closed list
    (use_closed: a wave that is over posts no claims) until every tree is connected"""
    fo, fg = both(S, ctx, "dense3d_coarse", 200, 10 ** 7, seed=2)
    assert fg.stats()["solved"] == 1 and fo.stats()["closed_size"] > 100


def test_priority_frontier(S, ctx):
    from test_gpu_sampling_chain import prio_pair
    fo, fg = prio_pair(S, ctx)
    fo.run()
    fg.run()
    assert fg.device_engine() and fo.stats()["n_nodes"] > 10000
    same(fo, fg)


def test_single_goal_job(S, ctx):
    """the goal is reached in a walk of k_commit: the fault flag, the finalize block's roll-back, the host's replay"""
    fo, fg = make(S, ctx, "triang", 64, 60000, seed=8, n_roots=2, goal_offset=[12, 8, 5])
    fo.run()
    fg.run()
    same(fo, fg)
    st = fg.stats()
    assert fg.device_engine() and st["solved"] == 1 and st["waves"] > st["host_fallback_waves"] >= 1


def test_sff_star_keeps_the_tail_in_k_commit(S, ctx):
    fo, fg = make(S, ctx, "dense3d", 65, 4000, seed=3, optimize=True)
    fo.run()
    fg.run()
    assert fg.device_engine() and fg.stats()["star_rounds"] > 0
    same(fo, fg)


def test_staged_runs_read_the_block_between_waves(S, ctx):
    fo, fg = both(S, ctx, "dense3d", 257, 9000, seed=5)
    _, fs = make(S, ctx, "dense3d", 257, 9000, seed=5)
    calls = 0
    while True:
        w0 = fs.stats()["waves"]
        fs.run(3)
        if fs.stats()["waves"] == w0:
            break
        calls += 1
    assert calls > 3
    assert fs.fingerprint() == fg.fingerprint()
    for k in COUNTERS + ("n_nodes", "n_borders"):
        assert fs.stats()[k] == fg.stats()[k], k
    same(fo, fs)


def test_query_clock_counts_every_round(S, ctx):
    """the query kernel's clock bracket reaches the finalize block through k_commit's workgroup 0 (the sampling
    workgroups reset the shards in the finalize block's own launch): one bracket per round"""
    _, fg = both(S, ctx, "dense3d", 192, 5000, seed=3)
    st = fg.stats()
    assert st["sweeps"] >= 20 and st["query_clock_launches"] == st["sweeps"], (st["sweeps"], st["query_clock_launches"])
