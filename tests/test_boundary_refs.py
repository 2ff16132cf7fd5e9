"""CPU checks of tests/boundary_cases.py: the exact integer / rational references agree with the oracle's fp64 expressions
on the lattice inputs, and the boundary generators produce what they promise (on the oracle) - which is what keeps the
GPU tests of tests/test_gpu_boundaries.py from passing emptily."""
import numpy as np
import pytest

import boundary_cases as B
import common
import oracle_lib as O

GAPS = [0.0, 2.0 ** -50, 2.0 ** -44, 1e-12, 1e-9, 1e-6]
OFFSETS = [0.0, 2.0 ** 20]


def rotation(p):
    R = np.zeros(9)
    O.lib().sffo_rotation(O.dp(O.f64(p)), O.TRIG_PORTABLE, O.dp(R))
    return R


def robots():
    return {"dense3d": common.scenario("dense3d")["robot"], "building": common.scenario("building")["robot"],
            "one_triangle": B.ONE_TRIANGLE_ROBOT}


def oracle_contact(P, Q):
    return bool(O.lib().sffo_tri_contact(O.dp(O.f64(P)), O.dp(O.f64(Q))))


def oracle_radius(pts, q, r, cap=4096):
    idx, dist = np.zeros(cap, np.int32), np.zeros(cap)
    n = O.lib().sffo_radius(O.dp(O.f64(pts)), len(pts), O.dp(O.f64(q)), r, O.ip(idx), O.dp(dist), cap)
    assert n <= cap
    return idx[:n].tolist(), dist[:n].tolist()


def oracle_knn(pts, q, k):
    idx, dist = np.zeros(k, np.int32), np.zeros(k)
    m = O.lib().sffo_knn(O.dp(O.f64(pts)), len(pts), O.dp(O.f64(q)), k, O.ip(idx), O.dp(dist))
    return idx[:m].tolist(), dist[:m].tolist()


def test_pair_table_covers_what_it_names():
    T = B.lattice_triangle_pairs()
    assert len(T) >= 40 and len({n for n, _, _, _ in T}) == len(T)
    assert sum(t is True for _, _, _, t in T) >= 20 and sum(t is False for _, _, _, t in T) >= 10
    assert sum(t is None for _, _, _, t in T) >= 8


def test_exact_contact_equals_the_oracle_and_the_geometry():
    for name, P, Q, truth in B.lattice_triangle_pairs():
        e = B.exact_tri_contact(P, Q)
        assert e == B.exact_tri_contact(Q, P), name
        assert oracle_contact(P, Q) == e and oracle_contact(Q, P) == e, name
        if truth is not None:
            assert e == truth, name


def test_exact_contact_one_unit_shifts():
    """the table's pairs moved by one unit along every axis: touching becomes separated or penetrating; still exact"""
    n_flip = 0
    for name, P, Q, _ in B.lattice_triangle_pairs():
        base = B.exact_tri_contact(P, Q)
        for a in range(3):
            for s in (-1, 1):
                Qs = np.array(Q, dtype=np.float64).reshape(3, 3)
                Qs[:, a] += s
                e = B.exact_tri_contact(P, Qs.reshape(9))
                assert oracle_contact(P, Qs.reshape(9)) == e, (name, a, s)
                n_flip += e != base
    assert n_flip > 50


STORES = [("all", None), ("families", None), ("clump", None), ("block", None)] + [("all", n) for n in B.STORE_SIZES]


@pytest.mark.parametrize("pitch,shift", [(1.0, 0.0), (0.25, 2.0 ** 22)])
def test_exact_neighbours_equal_the_oracle(pitch, shift):
    n_tied = 0
    for kind, n in STORES:
        st = B.lattice_store(kind, n, pitch=pitch, shift=shift)
        for q in st["queries"][:6] if n is None else st["queries"][:2]:
            for r0 in st["radii"][:4] if n is None else st["radii"][:1]:
                for r in B.nudged(r0):
                    ei, ed = B.exact_radius(st["pts"], q, r)
                    oi, od = oracle_radius(st["pts"], q, r)
                    assert ei == oi and ed == od, (kind, n, q, r)       # float ==: bit-equal (no NaN, no -0)
                at = [d for d in B.exact_radius(st["pts"], q, float(np.nextafter(r0, np.inf)))[1] if d == r0]
                n_tied += len(at)
            for k in (1, 2, 33, 64):
                ei, ed = B.exact_knn(st["pts"], q, k)
                oi, od = oracle_knn(st["pts"], q, k)
                assert ei == oi and ed == od, (kind, n, q, k)
    assert n_tied > 100, "the radii must sit exactly on populated distances"


def test_exact_domain_guard():
    """sqrt(2) is no lattice distance: fl(sqrt 2)^2 > 2, so the integer test and the fp64 test differ there, and exact_radius
    refuses instead of answering"""
    pts = np.array([[1, 1, 0, 0, 0, 0]], dtype=np.float64)
    with pytest.raises(AssertionError):
        B.exact_radius(pts, np.zeros(6), float(np.sqrt(2.0)))


def test_twin_store_is_a_trap():
    st = B.twin_store()
    assert len(st["pts"]) > 64
    assert B.exact_knn(st["pts"], st["queries"][0], 2) == ([2, 0], [0.0, 5.0])
    cell = np.floor(st["pts"][:2, :3] - st["limits"][0::2]) - np.floor(st["queries"][0, :3] - st["limits"][0::2])
    assert np.abs(cell[0]).max() == 5 and np.abs(cell[1]).max() == 4     # the lower id lies one shell farther out
    assert oracle_knn(st["pts"], st["queries"][0], 2) == ([2, 0], [0.0, 5.0])


def test_wrap_seam_pairs_sit_on_the_seam():
    st = B.wrap_seam_store()
    diffs = set()
    for q in st["queries"]:
        for p in st["pts"]:
            diffs |= {float(p[3 + a] - q[3 + a]) for a in range(3)}
    for b in (B.PI, -B.PI, 3 * B.PI, -3 * B.PI):
        for v in (b, float(np.nextafter(b, 0.0)), float(np.nextafter(b, 2 * b))):
            assert v in diffs, v
    # the definition wraps once: 3 pi stays at pi, and pi itself is excluded by r = pi but not its lower neighbour
    q = st["queries"][0]
    ids, d = oracle_radius(st["pts"], q, B.PI)
    assert 0 < len(ids) < len(oracle_radius(st["pts"], q, float(np.nextafter(B.PI, 4.0)))[0])


@pytest.mark.parametrize("shape", ["tip", "flat"])
@pytest.mark.parametrize("name", ["dense3d", "building", "one_triangle"])
def test_tangent_world_conditions(name, shape):
    """gap 0: every pose hits; the largest gap: every pose is free; in between the oracle decides, hierarchy == brute force.
    The shares of hits on the ladder are printed (pytest -s): the 2^-50 rung is mixed."""
    robot = robots()[name]
    n = 256
    for offset in OFFSETS:
        shares = []
        for gap in GAPS:
            poses, env = B.tangent_world(robot, n, 7, gap, offset, rotation, shape)
            w = O.World(env, robot, O.TRIG_PORTABLE)
            brute = np.array([w.collide_brute(p) for p in poses], np.uint8)
            assert np.array_equal(w.collide_many(poses), brute), (name, offset, gap)
            shares.append(int(brute.sum()))
            if gap == 0.0:
                assert brute.all(), (name, offset, np.flatnonzero(brute == 0)[:8])
            if gap == GAPS[-1]:
                assert not brute.any(), (name, offset, np.flatnonzero(brute)[:8])
        print("tangent ladder %s %s offset %g: hits of %d at gaps %s = %s" % (name, shape, offset, n, GAPS, shares))


@pytest.mark.parametrize("shape", ["tip", "flat"])
def test_tangent_world_three_levels(shape):
    robot = robots()["one_triangle"]
    for offset in OFFSETS:
        for gap in (0.0, GAPS[-1]):
            poses, env = B.tangent_world(robot, 4160, 8, gap, offset, rotation, shape)
            w = O.World(env, robot, O.TRIG_PORTABLE)
            fast = w.collide_many(poses)
            assert fast.all() if gap == 0.0 else not fast.any()
            some = np.arange(0, 4160, 13)
            assert np.array_equal(fast[some], np.array([w.collide_brute(p) for p in poses[some]], np.uint8))


@pytest.mark.parametrize("shape", ["tip", "flat"])
@pytest.mark.parametrize("name", ["dense3d", "building", "one_triangle"])
def test_tangent_edge_conditions(name, shape):
    robot = robots()[name]
    for offset in OFFSETS:
        a, b, env, ks = B.tangent_edges(robot, 40, 9, 0.0, offset, shape)
        assert sorted(set(ks.tolist())) == sorted(B.edge_targets())
        w = O.World(env, robot, O.TRIG_PORTABLE)
        for i in range(len(a)):
            assert w.path_free(a[i], b[i]) == (0, int(ks[i]), 20), (name, offset, i)
            for k in range(1, 21):                 # hierarchy == brute force on every sample of the edge
                p = np.concatenate([B.edge_sample(a[i], b[i], k), np.zeros(3)])
                assert w.collide(p) == w.collide_brute(p)
        a, b, env, ks = B.tangent_edges(robot, 40, 9, GAPS[-1], offset, shape)
        w = O.World(env, robot, O.TRIG_PORTABLE)
        for i in range(len(a)):
            assert w.path_free(a[i], b[i]) == (1, -1, 20), (name, offset, i)
        a, b, env = B.short_edges(robot, offset)
        w = O.World(env, robot, O.TRIG_PORTABLE)
        for i in range(2):
            assert w.collide_brute(b[i]) == 1, "the end pose is tangent"
            assert w.path_free(a[i], b[i]) == (1, -1, 0)
