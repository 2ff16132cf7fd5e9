"""The GPU entry points on inputs that sit ON the boundaries their conservative shortcuts decide (tests/boundary_cases.py).

Collision: robots that touch a triangle in exactly one shared vertex, the same contact opened by gaps from 2^-50 to 1e-6
of the coordinates' magnitude, integer triangle pairs in every touching configuration.  The bounding-sphere filters
(tri_far, dist2_far, plane_clear), the clearance bits and the closed boxes may only ever skip work: the answer is the
definition's (brute force over the 17-axis test), and on integers plain exact arithmetic.
Neighbour queries: exact distance ties on a lattice - the strict `d < r`, the (distance, id) order, the shell search of the
grid index, the fp32 superset filter at coordinates fp32 cannot hold - against integer arithmetic; the angle wrap seam
against the oracle."""
import numpy as np
import pytest

import boundary_cases as B
import common
import oracle_lib as O

pytestmark = pytest.mark.gpu

GAPS = [0.0, 2.0 ** -50, 2.0 ** -44, 1e-12, 1e-9, 1e-6]
OFFSETS = [0.0, 2.0 ** 20]
CLEARANCE = {"default": {}, "off": {"SFFGPU_NO_CLEARANCE": "1"}, "coarse": {"SFFGPU_CLEAR_CELLS": "4096"}}
KS = [1, 2, 31, 32, 33, 63, 64]


@pytest.fixture(scope="module")
def S():
    import space_filling_forest_star_amd as S
    return S


def rotation(p):
    R = np.zeros(9)
    O.lib().sffo_rotation(O.dp(O.f64(p)), O.TRIG_PORTABLE, O.dp(R))
    return R


def robot_mesh(name):
    return B.ONE_TRIANGLE_ROBOT if name == "one_triangle" else common.scenario(name)["robot"]


def context(S, monkeypatch, clearance):
    """the knobs are read when the context is created"""
    for k, v in CLEARANCE[clearance].items():
        monkeypatch.setenv(k, v)
    return S.Context(0)


def upload(ctx, env, robot, order):
    if order == "env_first":
        ctx.upload_env(env)
        ctx.upload_robot(robot)
    else:
        ctx.upload_robot(robot)     # the clearance grid is built when the second mesh arrives
        ctx.upload_env(env)


_TANGENT = {}


def tangent_ref(name, n, gap, offset, shape):
    """(poses, env, brute-force answers of the definition), computed once per world"""
    key = (name, n, gap, offset, shape)
    if key not in _TANGENT:
        robot = robot_mesh(name)
        poses, env = B.tangent_world(robot, n, 7, gap, offset, rotation, shape)
        w = O.World(env, robot, O.TRIG_PORTABLE)
        _TANGENT[key] = (poses, env, np.array([w.collide_brute(p) for p in poses], np.uint8))
    return _TANGENT[key]


def check_tangent(name, n, shape, run, offsets=OFFSETS):
    """run(poses, env) -> hits, for every rung of the ladder"""
    for offset in offsets:
        for gap in GAPS:
            poses, env, brute = tangent_ref(name, n, gap, offset, shape)
            got = run(poses, env)
            print("tangent %s %s n=%d offset=%g gap=%g: oracle hits %d, gpu hits %d, differ %d"
                  % (name, shape, n, offset, gap, brute.sum(), got.sum(), (got != brute).sum()))
            assert np.array_equal(got, brute), (name, n, offset, gap, np.flatnonzero(got != brute)[:8])
            if gap == 0.0:
                assert got.all(), "a shared vertex is a contact"
            if gap == GAPS[-1]:
                assert not got.any(), "a gap of 1e-6 of the magnitude is free"


# 256 triangles: two levels of the box hierarchy, 4160: three
TANGENT_CASES = [("dense3d", 256), ("one_triangle", 256), ("one_triangle", 4160)]
# "tip": the triangle stands on the bounding sphere's tangent plane with one vertex (the sphere-against-triangle distance
# is exactly the radius); "flat": it lies in that plane (the sphere-against-plane distance is exactly the radius)
SHAPES = ["tip", "flat"]


@pytest.mark.parametrize("order", ["env_first", "robot_first"])
@pytest.mark.parametrize("clearance", list(CLEARANCE))
@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name,n", TANGENT_CASES)
def test_tangent_poses(S, monkeypatch, name, n, shape, offset, clearance, order):
    ctx = context(S, monkeypatch, clearance)
    robot = robot_mesh(name)

    def run(poses, env):
        upload(ctx, env, robot, order)
        return ctx.collide_poses(poses)

    check_tangent(name, n, shape, run, [offset])
    ctx.close()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name,n", [("dense3d", 256), ("one_triangle", 4160)])
def test_tangent_transforms(S, monkeypatch, name, n, shape):
    """the same worlds with the robot placed by explicit transforms (R of the definition's rotation, T = xyz)"""
    ctx = context(S, monkeypatch, "default")
    robot = robot_mesh(name)

    def run(poses, env):
        upload(ctx, env, robot, "env_first")
        return ctx.collide_transforms(B.transforms_of(poses, rotation))

    check_tangent(name, n, shape, run)
    ctx.close()


_EDGES = {}


def edges_ref(name, gap, offset, shape):
    key = (name, gap, offset, shape)
    if key not in _EDGES:
        robot = robot_mesh(name)
        a, b, env, ks = B.tangent_edges(robot, 40, 9, gap, offset, shape)
        sa, sb, senv = B.short_edges(robot, offset, shift=4000.0)      # far from the long ones: one world
        a, b, env = np.vstack([a, sa]), np.vstack([b, sb]), np.vstack([env, senv])
        w = O.World(env, robot, O.TRIG_PORTABLE)
        want = np.array([w.path_free(a[i], b[i]) for i in range(len(a))], np.int64)
        _EDGES[key] = (a, b, env, ks, want)
    return _EDGES[key]


@pytest.mark.parametrize("clearance", list(CLEARANCE))
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", ["dense3d", "building", "one_triangle"])
def test_tangent_edges(S, monkeypatch, name, shape, clearance):
    """(free, first_hit, n_samples) of edges whose robot touches a triangle at sample 1, 8, 9, 10 or 20 - the clearance
    bits' edge plane reasons in groups of eight samples - and of edges too short to have a sample"""
    ctx = context(S, monkeypatch, clearance)
    robot = robot_mesh(name)
    for offset in OFFSETS:
        for gap in (0.0, GAPS[-1]):
            a, b, env, ks, want = edges_ref(name, gap, offset, shape)
            upload(ctx, env, robot, "env_first")
            free, fh, ns = ctx.collide_segments(a, b)
            got = np.stack([free, fh, ns], axis=1).astype(np.int64)
            print("edges %s %s offset=%g gap=%g: rows that differ %d" % (name, shape, offset, gap, (got != want).any(axis=1).sum()))
            assert np.array_equal(got, want), (name, offset, gap, np.flatnonzero((got != want).any(axis=1))[:8])
            if gap == 0.0:
                assert np.array_equal(fh[:len(ks)], ks) and not free[:len(ks)].any()
            else:
                assert free.all() and (fh == -1).all()
            assert np.array_equal(ns[len(ks):], [0, 0]) and free[len(ks):].all()
    ctx.close()


# ------------------------------------------------------------------------------------------------ lattice pairs
def _boxes(tris):
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3, 3)
    return t.min(axis=1), t.max(axis=1)


_LATTICE = {}


def lattice_world(rotate):
    if rotate not in _LATTICE:
        _LATTICE[rotate] = _lattice_world(rotate)
    return _LATTICE[rotate]


def _lattice_world(rotate):
    """env triangle j = (M_j Q_j) + S_j, robot placements (shape, M_j, S_j + shift): the table's pair j, moved to its own
    place on a super-lattice of pitch 4096 and (rotate) turned by one of the 24 axis rotations.  Expected by exact
    arithmetic over ALL env triangles."""
    T = B.lattice_triangle_pairs()
    rots = B.rotations24()
    ident = np.eye(3, dtype=np.int64)
    Ms = [rots[j % 24] if rotate else ident for j in range(len(T))]
    env = np.array([(np.array(Q, dtype=np.int64).reshape(3, 3) @ Ms[j].T + B.super_lattice(j)).reshape(9)
                    for j, (_, _, Q, _) in enumerate(T)])
    elo, ehi = _boxes(env)
    shifts = [np.zeros(3, dtype=np.int64)] + [s * np.eye(3, dtype=np.int64)[a] for a in range(3) for s in (-1, 1)]
    shapes = {}
    for j, (name, P, _, truth) in enumerate(T):
        for sh in shifts:
            t = B.super_lattice(j) + sh
            W = (np.array(P, dtype=np.int64).reshape(3, 3) @ Ms[j].T + t).reshape(9)
            lo, hi = _boxes(W)
            near = np.flatnonzero(((elo <= hi) & (lo <= ehi)).all(axis=1))     # closed boxes: the exact test's own precondition
            want = any(B.exact_tri_contact(env[k], W) for k in near)
            if truth is not None and not sh.any():
                assert want == truth, name
            shapes.setdefault(tuple(P), []).append((Ms[j], t, want, name))
    return env.astype(np.float64), shapes


@pytest.mark.parametrize("clearance", list(CLEARANCE))
def test_lattice_pairs_through_poses(S, monkeypatch, clearance):
    """integer translations, zero angles: the rotation is the exact identity, every product of the path is exact, and the
    expected answer is exact Python arithmetic.  Each pose also moved by one unit along each axis."""
    ctx = context(S, monkeypatch, clearance)
    env, shapes = lattice_world(rotate=False)
    ctx.upload_env(env)
    assert len(shapes) >= 6
    n_hit = n_all = 0
    for P, rows in shapes.items():
        ctx.upload_robot(np.array([P], dtype=np.float64))
        poses = np.zeros((len(rows), 6))
        poses[:, :3] = [t for _, t, _, _ in rows]
        want = np.array([w for _, _, w, _ in rows], np.uint8)
        got = ctx.collide_poses(poses)
        bad = np.flatnonzero(got != want)
        print("lattice pairs, robot %s: %d poses, %d hits, %d differ" % (P, len(rows), want.sum(), len(bad)))
        assert len(bad) == 0, [(rows[i][3], rows[i][1].tolist(), int(want[i])) for i in bad[:8]]
        n_hit, n_all = n_hit + int(want.sum()), n_all + len(rows)
    assert n_all >= 7 * 80 and n_hit >= 100 and n_all - n_hit >= 100
    ctx.close()


def test_lattice_pairs_through_transforms(S, monkeypatch):
    """the same pairs turned by the 24 rotations that permute the axes (entries 0 / +-1, exact) with integer translations"""
    ctx = context(S, monkeypatch, "default")
    env, shapes = lattice_world(rotate=True)
    ctx.upload_env(env)
    for P, rows in shapes.items():
        ctx.upload_robot(np.array([P], dtype=np.float64))
        rt = np.array([np.concatenate([M.reshape(9), t]) for M, t, _, _ in rows], dtype=np.float64)
        want = np.array([w for _, _, w, _ in rows], np.uint8)
        got = ctx.collide_transforms(rt)
        bad = np.flatnonzero(got != want)
        print("lattice pairs (rotated), robot %s: %d placements, %d hits, %d differ" % (P, len(rows), want.sum(), len(bad)))
        assert len(bad) == 0, [(rows[i][3], rows[i][1].tolist(), int(want[i])) for i in bad[:8]]
    ctx.close()


# ------------------------------------------------------------------------------------------------ neighbour queries
def fill(ctx, st, index=False):
    ctx.nodes_reset(0)
    ctx.nodes_append(st["pts"], st["tree"])
    if index:
        ctx.nodes_index(st["limits"], st["cell"])


def check_radius(ctx, st, ref, radii, cap=2048):
    """every query x every radius in one call; no filter, a per-tree filter, a max_id filter; then a cap that overflows.
    ref(pts, q, r, tree, want_tree, max_id) -> (ids, distances)"""
    Q = np.repeat(st["queries"], len(radii), axis=0)
    R = np.tile(np.asarray(radii, dtype=np.float64), len(st["queries"]))
    n = len(st["pts"])
    trees = (np.arange(len(Q)) % 3).astype(np.int32)
    maxid = np.array([[1, 40, 131, 700, n][i % 5] for i in range(len(Q))], np.int32)
    n_tied = 0
    for label, kw in (("plain", {}), ("tree", {"tree": trees}), ("max_id", {"max_id": maxid})):
        idx, dist, cnt = ctx.radius(Q, R, cap=cap, **kw)
        small = ctx.radius(Q, R, cap=8, **kw)
        for i in range(len(Q)):
            ei, ed = ref(st["pts"], Q[i], R[i], st["tree"], int(trees[i]) if label == "tree" else -1,
                         int(maxid[i]) if label == "max_id" else None)
            assert len(ei) <= cap
            m = int(cnt[i])
            assert m == len(ei), (label, Q[i], R[i], m, len(ei))
            assert idx[i, :m].tolist() == ei, (label, Q[i], R[i])
            assert dist[i, :m].tolist() == ed, (label, Q[i], R[i])          # bit-equal
            n_tied += sum(d == R[i] for d in ref(st["pts"], Q[i], float(np.nextafter(R[i], np.inf)), st["tree"], -1, None)[1])
            # cap < cnt: the count is still the total, the entries kept are some of the hits, in (distance, id) order
            si, sd, sc = small[0][i], small[1][i], int(small[2][i])
            assert sc == len(ei)
            keep = min(sc, 8)
            pairs = list(zip(sd[:keep].tolist(), si[:keep].tolist()))
            assert pairs == sorted(pairs) and len(set(pairs)) == keep and set(pairs) <= set(zip(ed, ei)), (label, Q[i], R[i])
    return n_tied


def nudged_all(radii):
    return [r for r0 in radii for r in B.nudged(r0)]


@pytest.mark.parametrize("kind", ["all", "families", "clump", "block", "twin"])
def test_radius_is_strict_and_ordered_on_the_lattice(S, kind):
    """r exactly at a populated distance excludes the nodes AT that distance, its upper neighbour includes them, ties come
    out by id: against integer arithmetic"""
    ctx = S.Context(0)
    st = B.twin_store() if kind == "twin" else B.lattice_store(kind)
    fill(ctx, st)
    n_tied = check_radius(ctx, st, B.exact_radius, nudged_all(st["radii"]))
    print("radius %s: %d nodes, %d (query, r) pairs with nodes at exactly d == r" % (kind, len(st["pts"]), n_tied))
    assert n_tied >= 2
    ctx.close()


def check_knn(ctx, st, ref, ks, n_big=2056):
    """the three routes give the reference's lists: no index (k_knn_grid_wg's sweep below 2048 queries, k_knn_linear above),
    the grid index below 2048 queries (k_knn_grid_wg) and above (k_knn_grid)"""
    Q = st["queries"]
    big = np.tile(Q, (n_big // len(Q) + 1, 1))[:n_big]
    assert len(Q) <= 2048 < len(big)
    want = {k: [ref(st["pts"], q, k) for q in Q] for k in ks}
    for index in (False, True):
        fill(ctx, st, index)
        for k in ks:
            for label, qq in (("few", Q), ("many", big)):
                idx, dist, cnt = ctx.knn(qq, k)
                for i in range(len(qq)):
                    ei, ed = want[k][i % len(Q)]
                    m = int(cnt[i])
                    where = (len(st["pts"]), "index" if index else "no index", label, k, qq[i].tolist())
                    assert m == len(ei) == min(k, len(st["pts"])), where
                    assert idx[i, :m].tolist() == ei, where + (idx[i, :m].tolist(), ei)
                    assert dist[i, :m].tolist() == ed, where


@pytest.mark.parametrize("n", B.STORE_SIZES)
def test_knn_ties_at_every_store_size(S, n):
    ctx = S.Context(0)
    check_knn(ctx, B.lattice_store("all", n), B.exact_knn, KS)
    ctx.close()


@pytest.mark.parametrize("kind", ["all", "families", "clump", "block", "twin"])
def test_knn_ties_on_the_lattice(S, kind):
    """queries on a node (d = 0 ties inside the 100-fold clump), on cell faces, edges and corners, outside the limits; the
    twin store keeps its lower-id twin one shell farther out than the higher-id one"""
    ctx = S.Context(0)
    st = B.twin_store() if kind == "twin" else B.lattice_store(kind)
    check_knn(ctx, st, B.exact_knn, KS)
    ctx.close()


def test_magnitude_quarter_lattice_at_2_pow_22(S):
    """the same lattice at x y z = 2^22 + quarter-integers: fp32 holds these to 0.5, fp64 exactly.  The fp32 filters have to
    carry that rounding in their slack (sweep_eps, the shell slack); the answers are the exact ones."""
    ctx = S.Context(0)
    st = B.lattice_store("all", pitch=0.25, shift=2.0 ** 22)
    assert not np.array_equal(st["pts"].astype(np.float32).astype(np.float64), st["pts"])
    fill(ctx, st)
    n_tied = check_radius(ctx, st, B.exact_radius, nudged_all([5.0, 0.75]))
    assert n_tied >= 2
    check_knn(ctx, st, B.exact_knn, [1, 2, 33, 64])
    ctx.close()


def oracle_radius(pts, q, r, tree, want_tree, max_id, cap=4096):
    keep = np.array([(max_id is None or i < max_id) and (want_tree < 0 or tree[i] == want_tree) for i in range(len(pts))])
    ids = np.flatnonzero(keep)
    sub = O.f64(pts[ids])
    idx, dist = np.zeros(cap, np.int32), np.zeros(cap)
    m = O.lib().sffo_radius(O.dp(sub), len(sub), O.dp(O.f64(q)), r, O.ip(idx), O.dp(dist), cap) if len(sub) else 0
    return ids[idx[:m]].tolist(), dist[:m].tolist()


def oracle_knn(pts, q, k):
    idx, dist = np.zeros(k, np.int32), np.zeros(k)
    m = O.lib().sffo_knn(O.dp(O.f64(pts)), len(pts), O.dp(O.f64(q)), k, O.ip(idx), O.dp(dist))
    return idx[:m].tolist(), dist[:m].tolist()


def test_wrap_seam(S):
    """angle differences on, next to and beyond +-pi and +-3 pi: the definition wraps once (3 pi stays at pi), `>= pi`
    wraps and `< -pi` wraps.  The reference is the oracle's fp64 expressions."""
    ctx = S.Context(0)
    st = B.wrap_seam_store()
    fill(ctx, st)
    check_radius(ctx, st, oracle_radius, st["radii"])
    check_knn(ctx, st, oracle_knn, [1, 2, 31, 64])
    ctx.close()
