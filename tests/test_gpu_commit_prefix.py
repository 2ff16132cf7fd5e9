"""The commit's node-id prefix (plain SFF on the device engine): k_commit no longer adds up the accepted samples of the
lower workgroups - the append launch derives the prefix per 64-sample group from the workgroups' lines (hand_lines in
csrc/devforest.hip, commit_line_prefix in csrc/commit_next.h), and only a commit workgroup that holds a border event
whose neighbour was accepted in the same round still waits for the lower workgroups' counts.

Every case builds the forest on the CPU oracle and on the device engine and asks for the same forest node for node
(assert_same_forest) and for the oracle's counters.  A wrong prefix gives a node another id: parents, frontier, borders
and the next round's list all move.  The shapes are the smallest at which the prefix can go wrong: one full line, a
second line of one sample, two append blocks (a prefix read across a block edge), 17 lines (the scan crosses a
wavefront edge); the rare branch of k_commit is entered (counted on the device) with the neighbour in the event's own
and in a lower workgroup, with the fused and the separate sampling launch; one job rolls rounds back."""
import re

import pytest

from test_gpu_commit_handoff import both, same
from test_gpu_device_engine import make

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


@pytest.mark.parametrize("name", ["dense3d", "triang"])
@pytest.mark.parametrize("wave", [64, 65, 128, 129, 257, 1025])
def test_line_and_block_edges(S, ctx, name, wave):
    """64 slots: exactly one full line; 65: a second line holding one sample; 128 / 129: two full lines / a third of one
    sample; 257: two append blocks of each kind - the second block's first group takes its prefix from the first
    block's four lines; 1025: 17 lines in five blocks of each kind, the fifth with one sample."""
    fo, _ = both(S, ctx, name, wave, 5000, seed=3)
    assert fo.stats()["n_nodes"] > 40 and fo.stats()["waves"] > 2


def test_scan_across_a_wavefront_edge(S, ctx):
    """4161 slots: 66 lines, one per thread - lines 64 and 65 are scanned by the second wavefront, their prefix is the
    first wavefront's total (through LDS) plus the scan within the second (17 lines, the case above, stay inside one)."""
    fo, _ = both(S, ctx, "dense3d", 4161, 20000, seed=3)
    assert fo.stats()["n_nodes"] > 1000 and fo.stats()["waves"] > 2


# The rare branch: a border event whose neighbour was accepted in the same round (k_commit, step 4).  The profile line
# carries how often it ran and how often the neighbour sat in a LOWER commit workgroup (DevCtrl::prof[4], both halves).
MATE_WORLD, MATE_ITERS, MATE_ROOTS = "dense3d_coarse", 12000, 5
MATE_SEED = {256: 4, 1024: 4}
MATE_COUNTS = re.compile(r"border events with a neighbour accepted in the same round (\d+), in a lower workgroup (\d+)")
_oracle = {}


def mate_case(S, ctx, capfd, wave, **env):
    """the device forest of the job and its two counts; the oracle's forest is built once per wave and only read"""
    fo, fg = make(S, ctx, MATE_WORLD, wave, MATE_ITERS, seed=MATE_SEED[wave], n_roots=MATE_ROOTS, SFFGPU_PROFILE=1, **env)
    if wave not in _oracle:
        fo.run()
        _oracle[wave] = fo
    capfd.readouterr()
    fg.run()
    err = capfd.readouterr().err
    found = MATE_COUNTS.findall(err)
    assert found, err[-2000:]
    assert fg.device_engine()
    same(_oracle[wave], fg)
    return tuple(int(v) for v in found[-1])


@pytest.mark.parametrize("env", [dict(), dict(SFFGPU_NO_FUSED_SAMPLE=1)], ids=["fused", "two_launches"])
@pytest.mark.parametrize("wave", [256, 1024])
def test_event_whose_neighbour_was_accepted_in_the_same_round(S, ctx, capfd, wave, env):
    """k_commit computes the neighbour's new id itself: the accepted samples of the workgroups below the neighbour's,
    from their KC_ACC words.  The job must enter the branch (a condition of the test, not a measurement), and at
    waves of 1024 slots with the neighbour in a lower workgroup - there the sum stops below the event's own
    workgroup.  With SFFGPU_NO_FUSED_SAMPLE=1 every round is applied by k_append."""
    mates, lower = mate_case(S, ctx, capfd, wave, **env)
    print("wave %d: %d events with a neighbour of the same round, %d of them in a lower workgroup" % (wave, mates, lower))
    assert mates > 0 and lower <= mates
    if wave == 1024:
        assert lower > 0


def test_rolled_back_rounds_apply_nothing(S, ctx):
    """hit lists of 3 entries overflow: the finalize block rolls the round back, the node-creating and the list
    workgroups - which have scanned the lines of a round that does not count - apply nothing, the host redoes it"""
    _, fg = both(S, ctx, "dense3d_coarse", 256, 12000, seed=4, SFFGPU_TEST_HITCAP=3)
    assert fg.stats()["slow_path_samples"] > 0
