"""SFF* k-nearest kernels in rounds that accept more than 16 x 64 samples.

The stage "samples accepted earlier in this round" (csrc/knn_dev.h: star_earlier_samples, shared by k_star_knn_wg and
k_star_knn) has three branches: the list of the accepted samples scanned from registers (up to 16 x 64 of them), the scan
of the whole list for a tree wanted whole, and the cube over the round's own grid.  The other SFF* tests reach only the
first.  The two cases here are built so that a later sample of a round cannot get its set without the second or the third:
the preconditions are asserted on the CPU oracle alone, the forest must equal the oracle's bit for bit under the default
kernel and under SFFGPU_STAR_KNN=lone."""
import math

import numpy as np
import pytest

import common
import oracle_lib as O
from test_gpu_device_engine import engine
from test_gpu_parity import assert_same_forest, load_world

pytestmark = pytest.mark.gpu

LIST_MAX = 16 * 64      # accepted samples of a round the list branch takes


@pytest.fixture(scope="module")
def S():
    import space_filling_forest_star_amd as S
    return S


@pytest.fixture(scope="module")
def ctx(S):
    c = S.Context(0)
    yield c
    c.close()


def k_of(n_nodes):
    return int(2.0 * math.e * math.log10(n_nodes))      # src/forest.h:309


CASES = {
    # some round of the last wave accepts more than 1024 samples of trees that hold k nodes and more: the round-grid cube
    "cube": dict(n_roots=64, wave=16384, waves=14, threshold_misses=5),
    # round 1 accepts more than 1024 samples while every tree is smaller than k: the scan of the whole list
    "whole": dict(n_roots=3000, wave=4096, waves=1, threshold_misses=2),
}
_worlds = {}


def world_of(ctx, case):
    """scenario, world, roots, arguments and the oracle's finished forest of a case: computed once, never changed"""
    if case not in _worlds:
        c = CASES[case]
        sc, w = load_world(ctx, "triang")
        roots = common.free_roots(w.collide, sc["limits"], c["n_roots"], seed=3)
        kw = dict(dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"], dim=sc["dim"], max_iterations=10 ** 7,
                  wave=c["wave"], seed=3, optimize=True, threshold_misses=c["threshold_misses"])
        fo = O.Forest(w, roots, sc["limits"], **kw)
        n_after = [fo.stats()["n_nodes"]]
        for _ in range(c["waves"]):
            fo.run(1)
            n_after.append(fo.stats()["n_nodes"])
        so, trees = fo.stats(), fo.nodes()["tree"]
        if case == "cube":
            added = np.diff(n_after)
            big = int(np.argmax(added))
            # at most threshold_misses rounds per wave: some round of that wave accepted more than LIST_MAX samples
            assert added[big] > c["threshold_misses"] * LIST_MAX, added
            # every tree held k nodes before that wave began: no sample of it wants its tree whole
            per_tree = np.bincount(trees[:n_after[big]], minlength=c["n_roots"])
            assert per_tree.min() >= k_of(so["n_nodes"]), (per_tree.min(), k_of(so["n_nodes"]))
        else:
            # the samples round 1 accepts: every start tree draws one, the rejected ones once more in round 2
            assert 2 * c["n_roots"] - so["iterations"] > LIST_MAX, so["iterations"]
            # every tree stays smaller than the smallest k of the wave: all of them are wanted whole
            per_tree = np.bincount(trees, minlength=c["n_roots"])
            assert per_tree.max() < k_of(c["n_roots"]), (per_tree.max(), k_of(c["n_roots"]))
        _worlds[case] = (sc, roots, kw, fo)
    return _worlds[case]


@pytest.mark.parametrize("env", [dict(), dict(SFFGPU_STAR_KNN="lone")], ids=["default", "knn_lone"])
@pytest.mark.parametrize("case", ["cube", "whole"])
def test_rounds_beyond_the_list_branch_equal_the_oracle(S, ctx, case, env):
    sc, roots, kw, fo = world_of(ctx, case)
    with engine(**env):
        fg = S.Forest(ctx, roots, sc["limits"], **kw)
    assert fg.device_engine()
    fg.run(CASES[case]["waves"])
    assert_same_forest(fo, fg)
    sg = fg.stats()
    assert sg["host_fallback_waves"] == 0 and sg["star_rounds"] > 0
    fg.close()
