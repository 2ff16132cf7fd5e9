"""The CPU side of test_gpu_far_from_origin.py, which takes the oracle's runs of moved worlds as given: the helper that moves a
world (common.scenario(name, shift)) and the oracle's own behaviour under the move.  No GPU."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import common
import oracle_lib as O

SHIFT_A = (2.0 ** 20, -2.0 ** 21, 2.0 ** 19)
SHIFT_B = (2.0 ** 22, 2.0 ** 22, -2.0 ** 22)
SHIFTS = {"A": SHIFT_A, "B": SHIFT_B}


def shift_of(name, at):
    s = SHIFTS[at]
    return (s[0], s[1], 0.0) if common.SCENARIOS[name][6] == 2 else s


@pytest.mark.parametrize("at", sorted(SHIFTS))
@pytest.mark.parametrize("name", sorted(common.SCENARIOS))
def test_moved_scenario_minus_the_shift_is_the_scenario(name, at):
    """one fp64 rounding at the moved magnitude per coordinate, no more: |(v + s) - s - v| <= ulp(v + s); limits and start
    points likewise; the robot, the distances and the dimension untouched"""
    s = np.array(shift_of(name, at))
    base, far = common.scenario(name), common.scenario(name, tuple(s))
    assert far["env"].shape == base["env"].shape and far["env"].dtype == np.float64 and far["env"].flags["C_CONTIGUOUS"]
    s9 = np.tile(s, 3)
    assert np.all(np.abs((far["env"] - s9) - base["env"]) <= np.spacing(np.abs(far["env"])))
    moved = np.abs(far["env"] - base["env"]).reshape(-1, 3).min(axis=0)
    assert np.all(moved >= np.abs(s) - np.spacing(np.abs(s)))                      # every vertex went along
    assert np.array_equal(far["robot"], base["robot"])
    for k in ("dist_tree", "sampling_dist", "dim", "scale"):
        assert far[k] == base[k]
    assert len(far["limits"]) == 6 and all(isinstance(v, float) for v in far["limits"])
    for a in range(3):
        for e in range(2):
            assert far["limits"][2 * a + e] == base["limits"][2 * a + e] + s[a]     # (integers plus powers of two: exact)
    if base["xml_points"] is None:
        assert far["xml_points"] is None
    else:
        d = (far["xml_points"][:, :3] - s) - base["xml_points"][:, :3]
        assert np.all(np.abs(d) <= np.spacing(np.abs(far["xml_points"][:, :3])))
        assert np.array_equal(far["xml_points"][:, 3:], base["xml_points"][:, 3:])


def test_no_shift_is_the_scenario_bit_for_bit_and_a_flat_world_stays_flat():
    for name in common.SCENARIOS:
        a, b = common.scenario(name), common.scenario(name, None)
        assert a["env"].tobytes() == b["env"].tobytes() and a["robot"].tobytes() == b["robot"].tobytes()
        assert a["limits"] == b["limits"] == common.SCENARIOS[name][3] and "shift" not in a
        assert (a["xml_points"] is None) == (b["xml_points"] is None)
        if a["xml_points"] is not None:
            assert a["xml_points"].tobytes() == b["xml_points"].tobytes()
    with pytest.raises(AssertionError):
        common.scenario("dense2d", SHIFT_A)
    common.scenario("dense2d", (SHIFT_A[0], SHIFT_A[1], 0.0))


def oracle_run(name, wave, iters, shift):
    sc = common.scenario(name, shift)
    w = O.World(sc["env"], sc["robot"], O.TRIG_PORTABLE)
    roots = sc["xml_points"][:5] if sc["xml_points"] is not None else common.free_roots(w.collide, sc["limits"], 5, seed=3, dim=sc["dim"])
    fo = O.Forest(w, roots, sc["limits"], dist_tree=sc["dist_tree"], sampling_dist=sc["sampling_dist"], dim=sc["dim"],
                  max_iterations=iters, wave=wave, seed=3)
    fo.run()
    return fo, roots


@pytest.mark.parametrize("name,wave,iters,min_nodes", [("dense3d", 256, 8000, 700), ("dense2d", 16, 3000, 150)])
def test_the_oracle_grows_the_same_forest_in_the_moved_world(name, wave, iters, min_nodes):
    """On these two maps no tolerance comparison of the oracle sits close enough to its threshold for the move's roundings
    to flip it: the moved runs have the unshifted run's node count, parents, tree ids, iterations and borders, and every
    node lies where the unshifted node lies, moved - to within the roundings of a few steps at the moved magnitude.
    (On triang they do flip - 917 / 925 / 895 nodes at wave 64 - which is why the GPU is only ever compared with the
    oracle's run of the SAME moved problem.)"""
    shifts = [None, shift_of(name, "A"), shift_of(name, "B")]
    with ThreadPoolExecutor(3) as ex:      # (the calls release the interpreter lock)
        runs = list(ex.map(lambda s: oracle_run(name, wave, iters, s), shifts))
    (f0, r0), n0, s0 = runs[0], runs[0][0].nodes(), runs[0][0].stats()
    assert s0["n_nodes"] > min_nodes and s0["nn_queries"] > 0
    for (fo, roots), s in zip(runs[1:], shifts[1:]):
        s = np.array(s)
        assert np.all(np.abs((roots[:, :3] - s) - r0[:, :3]) <= np.spacing(np.abs(roots[:, :3])))     # the same start points
        st, nd = fo.stats(), fo.nodes()
        for k in ("iterations", "solved", "n_nodes", "n_trees", "n_borders", "frontier_size", "closed_size", "n_connected", "waves"):
            assert st[k] == s0[k], (k, st[k], s0[k])
        for k in ("parent", "tree", "iter"):
            assert np.array_equal(nd[k], n0[k]), k
        b0, b1 = f0.borders(), fo.borders()
        for k in ("ta", "tb", "n1", "n2"):
            assert np.array_equal(b0[k], b1[k]), k
        # a node is its parent plus a step: each generation adds an fp64 rounding at the moved magnitude (2^-30 at 2^22) to
        # what the root carried; 1e-4 is four orders above a deep tree's sum of them and four below a step
        assert np.abs((nd["pos"][:, :3] - s) - n0["pos"][:, :3]).max() < 1e-4
        # (the angles of a 6-D step are scaled by step / distance, a distance that carries the positions' roundings: the same bound)
        assert np.abs(nd["pos"][:, 3:] - n0["pos"][:, 3:]).max() < 1e-4
