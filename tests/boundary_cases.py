"""Inputs that sit ON the boundaries the kernels decide, and exact references for them.

Nothing here needs a GPU or imports the product.  Two kinds of content:

* exact references in plain Python integers / fractions.Fraction (exact_tri_contact, exact_radius, exact_knn), valid
  on inputs where the fp64 expressions of the definition (oracle/sff_oracle.cpp) round nowhere;
* generators of worlds whose answer hangs on a conservative filter's last bit: robots that touch a triangle in exactly
  one shared vertex (tangent_world, tangent_edges), integer triangle pairs in every touching configuration
  (lattice_triangle_pairs), node sets with exact distance ties (lattice_store).

The generators that need the pose -> rotation matrix map take it as an argument (`rotation(pose6) -> 9 floats`), so
that the caller decides whose trigonometry is used.
"""
import functools
import itertools
import math
from fractions import Fraction

import numpy as np

# ---------------------------------------------------------------------------------------------- exact triangle contact
# Convention (the definition's, oracle/sff_oracle.cpp: tri_contact = aabb_overlap_tri && sat17):
#   * the boxes are CLOSED: boxes that share a face, an edge or a corner pass the precondition;
#   * an axis separates only with a STRICT gap (min of one > max of the other): touching is contact;
#   * a zero axis (parallel edges, a degenerate triangle's normal) projects everything to 0 and never separates.
#     >>> exact_tri_contact([0,0,0, 4,0,0, 0,4,0], [4,0,0, 8,0,0, 4,4,4])      # one shared vertex
#     True
#     >>> exact_tri_contact([0,0,0, 4,0,0, 0,4,0], [0,0,1, 4,0,1, 0,4,1])      # parallel, one unit apart
#     False


def _frac3(t):
    t = [Fraction(x) for x in np.asarray(t, dtype=np.float64).reshape(9).tolist()]
    return [t[0:3], t[3:6], t[6:9]]


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def exact_tri_contact(P, Q):
    """closed-box precondition + the 17-axis separating-axis test in exact rational arithmetic; P, Q = 9 numbers each"""
    p, q = _frac3(P), _frac3(Q)
    for a in range(3):
        pa, qa = [v[a] for v in p], [v[a] for v in q]
        if min(pa) > max(qa) or min(qa) > max(pa):
            return False
    e = [_sub(p[1], p[0]), _sub(p[2], p[1]), _sub(p[0], p[2])]
    f = [_sub(q[1], q[0]), _sub(q[2], q[1]), _sub(q[0], q[2])]
    n, m = _cross(e[0], e[1]), _cross(f[0], f[1])
    axes = [n, m] + [_cross(ei, fj) for ei in e for fj in f] + [_cross(ei, n) for ei in e] + [_cross(fi, m) for fi in f]
    assert len(axes) == 17
    for ax in axes:
        pp, qq = [_dot(ax, v) for v in p], [_dot(ax, v) for v in q]
        if min(pp) > max(qq) or min(qq) > max(pp):
            return False
    return True


# ---------------------------------------------------------------------------------------------- exact neighbours
# Input domain on which these equal the fp64 definition (distance6 / Hit ordering of oracle/sff_oracle.cpp) bit for bit:
#   * x y z are integers or quarter-integers (the stores; queries on the middle of a cell face may sit on sixteenths) with
#     |x| <= 2^22 + 2^10: differences and their squares are exact doubles, the six-term sum stays far below 2^53 units;
#   * all angles are multiples of 0.25 (sixteenths for the queries) and every |b - a| < 3 < pi, so wrap_angle never fires
#     and the angle term is the plain difference (its sign does not matter: it is squared);
#   * for exact_radius, r is a populated distance r0 whose square lies on the same grid (5, 3, 7, 2, 0.75 ...) or one of
#     its two nextafter neighbours.  Every other node then differs from r0^2 by >= 1/256 in d^2, worlds away from the
#     rounding of sqrt, and `sqrt(d2) < r` in doubles equals `d2 < r^2` in integers.  exact_radius asserts this.
# The distance returned is math.sqrt of the exact sum: sqrt is correctly rounded in IEEE arithmetic, here and on the device.


def _scaled_ints(rows):
    """rows of dyadic floats -> (rows of Python ints, S) with value = int / S, S a power of two"""
    S = 1
    for row in rows:
        for x in row:
            S = max(S, float(x).as_integer_ratio()[1])
    return [[int(Fraction(float(x)) * S) for x in row] for row in rows], S


def _d2_ints(pts, q):
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 6)
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(6)
    return _d2_ints_cached(pts.tobytes(), q.tobytes())


@functools.lru_cache(maxsize=64)
def _d2_ints_cached(pts_bytes, q_bytes):
    pts = np.frombuffer(pts_bytes, dtype=np.float64).reshape(-1, 6)
    q = np.frombuffer(q_bytes, dtype=np.float64)
    assert len(pts) == 0 or np.abs(pts[:, 3:] - q[3:]).max() < 3.0, "outside the exact domain: an angle difference that could wrap"
    rows, S = _scaled_ints(pts.tolist() + [q.tolist()])
    qi = rows[-1]
    return [sum((x - y) ** 2 for x, y in zip(row, qi)) for row in rows[:-1]], S


def _dist(d2, S):
    d = math.sqrt(d2 / (S * S))          # int / int is correctly rounded; exact here (d2 < 2^53, S a power of two)
    assert Fraction(d2, S * S) == Fraction(d2 / (S * S)), "outside the exact domain: the squared distance is no double"
    return d


def exact_radius(pts, q, r, tree=None, want_tree=-1, max_id=None):
    """ids and distances of the nodes with d < r (STRICT), ordered by (d^2, id); d^2 < r^2 decided in integers.
    tree / want_tree / max_id: the filters of sffgpu_radius (node's tree == want_tree unless < 0, id < max_id)"""
    d2, S = _d2_ints(pts, q)
    rn, rd = float(r).as_integer_ratio()
    out = []
    for i, v in enumerate(d2):
        inside = v * rd * rd < rn * rn * S * S
        assert inside == (_dist(v, S) < r), "outside the exact domain: r is not at (or next to) a lattice distance"
        if not inside or (max_id is not None and i >= max_id) or (want_tree >= 0 and tree[i] != want_tree):
            continue
        out.append((v, i))
    out.sort()
    return [i for _, i in out], [_dist(v, S) for v, _ in out]


def exact_knn(pts, q, k, tree=None, want_tree=-1, max_id=None):
    """the k nearest by (d^2, id) - an exact tie is broken by the node id"""
    d2, S = _d2_ints(pts, q)
    out = sorted((v, i) for i, v in enumerate(d2)
                 if (max_id is None or i < max_id) and (want_tree < 0 or tree[i] == want_tree))[:k]
    return [i for _, i in out], [_dist(v, S) for v, _ in out]


# ---------------------------------------------------------------------------------------------- tangent worlds
def robot_sphere(robot_tri9):
    """centre of the robot's bounding box, its farthest vertex (first of equals) and the radius, as the definition and the
    library compute them"""
    v = np.asarray(robot_tri9, dtype=np.float64).reshape(-1, 3)
    rc = 0.5 * (v.min(axis=0) + v.max(axis=0))
    d2 = np.zeros(len(v))
    for i in range(3):
        d2 += (v[:, i] - rc[i]) * (v[:, i] - rc[i])
    far = int(np.argmax(d2))
    return rc, v[far].copy(), float(np.sqrt(d2[far]))


def xform(R, T, v):
    """world = R v + T in the definition's evaluation order, ((R0*v0 + R1*v1) + R2*v2) + T"""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    return np.array([((R[i, 0] * v[0] + R[i, 1] * v[1]) + R[i, 2] * v[2]) + T[i] for i in range(3)])


def _perp_frame(u):
    e = np.zeros(3)
    e[int(np.argmin(np.abs(u)))] = 1.0
    a = np.cross(u, e)
    a /= np.linalg.norm(a)
    b = np.cross(u, a)
    return a, b / np.linalg.norm(b)


def _tip_triangle(w, u, gap, size, slot, flat=None):
    """a triangle with one vertex at w + gap * u (in vertex slot `slot`) that opens away from w along u: it lies in the
    half-space (x - w) . u >= gap and meets its boundary plane in that one vertex.  flat = (e1, e2), two directions
    perpendicular to u: the triangle (tip, tip + size e1, tip + size e2) lies IN that boundary plane instead - its own
    plane is then tangent to the robot's bounding sphere, which is what a sphere-against-plane filter decides on"""
    a, b = _perp_frame(u)
    tip = w + gap * u
    t = [tip, tip + size * (u + 0.5 * a), tip + size * (u + 0.5 * b)]
    if flat is not None:
        t = [tip, tip + size * flat[0], tip + size * flat[1]]
    t = t[-slot:] + t[:-slot] if slot else t
    return np.concatenate(t)


def coarse_lattice(n, pitch, offset):
    side = int(math.ceil(n ** (1.0 / 3.0) - 1e-9))
    i = np.arange(n)
    g = np.stack([i % side, (i // side) % side, i // (side * side)], axis=1).astype(np.float64)
    return g * pitch + offset


def tangent_world(robot, n, seed, gap, offset, rotation, shape="tip", angles=None):
    """n poses and n environment triangles: pose i's robot touches triangle i in exactly one point when gap == 0.

    The point is the world position of the robot's farthest vertex (from the centre of its bounding sphere, so the whole
    robot lies on one side of the sphere's tangent plane there), evaluated with `rotation` and the definition's xform
    order - bit for bit what the definition transforms.  Triangle i has that point as vertex i % 3 and opens outward.
    gap > 0 moves the triangle outward by gap * max(radius, |offset|): a strict gap, of the order of `gap` relative to
    the coordinates in play.  Poses sit on a lattice of pitch 40 radii (a pose can only touch its own triangle), angles
    are uniform in [-pi, pi).  shape "tip": the triangle stands on the sphere's tangent plane with one vertex (its own
    plane cuts the sphere); "flat": it lies in the tangent plane.  angles: an n x 3 array (yaw pitch roll) used instead
    of the uniform draw.  Returns (poses n x 6, env n x 9)."""
    rc, vfar, radius = robot_sphere(robot)
    rs = np.random.RandomState(seed)
    poses = np.zeros((n, 6))
    poses[:, :3] = coarse_lattice(n, 40.0 * radius, float(offset))
    poses[:, 3:] = rs.uniform(-np.pi, np.pi, (n, 3))
    if angles is not None:
        poses[:, 3:] = np.asarray(angles, dtype=np.float64).reshape(n, 3)
    scale = max(radius, abs(float(offset)))
    env = np.zeros((n, 9))
    for i in range(n):
        R = rotation(poses[i])
        w, c = xform(R, poses[i, :3], vfar), xform(R, poses[i, :3], rc)
        u = (w - c) / np.linalg.norm(w - c)
        env[i] = _tip_triangle(w, u, gap * scale, radius, i % 3, _perp_frame(u) if shape == "flat" else None)
    return poses, env


def transforms_of(poses, rotation):
    """the rt12 rows (rotation row-major, then translation) that place the robot like `poses` do"""
    return np.array([np.concatenate([np.asarray(rotation(p), dtype=np.float64).reshape(9), p[:3]]) for p in poses])


EDGE_LEN = 2.05          # 20.5 parts of 0.1: samples 1 .. 20


def edge_targets():
    """sample indices a tangent edge is aimed at: the first, both sides of the first group-of-eight seam, the middle, the last"""
    return [1, 8, 9, 10, 20]


def tangent_edges(robot, n, seed, gap, offset, shape="tip"):
    """n edges (a, b) and n triangles: the robot of edge i, un-rotated like every edge sample, touches triangle i in one
    point at sample k_i (and nowhere before), k_i cycling through edge_targets().  The edge runs perpendicular to the
    direction of the robot's farthest vertex, so all its samples touch one plane and the triangle stands on that plane at
    sample k_i.  The sample positions are the definition's: parts = distance / 0.1, pos = a + k * dir / parts.
    shape "flat": the triangle lies in that plane and opens along the edge's direction, away from the earlier samples.
    Returns (a n x 6, b n x 6, env n x 9, k n)."""
    rc, vfar, radius = robot_sphere(robot)
    u = (vfar - rc) / np.linalg.norm(vfar - rc)
    rs = np.random.RandomState(seed)
    scale = max(radius, abs(float(offset)))
    a6, b6 = np.zeros((n, 6)), np.zeros((n, 6))
    a6[:, :3] = coarse_lattice(n, 40.0 * max(radius, EDGE_LEN), float(offset))
    env, ks = np.zeros((n, 9)), np.zeros(n, np.int32)
    targets = edge_targets()
    for i in range(n):
        p, q = _perp_frame(u)
        phi = rs.uniform(0, 2 * np.pi)
        d = math.cos(phi) * p + math.sin(phi) * q
        b6[i, :3] = a6[i, :3] + EDGE_LEN * d
        k = targets[i % len(targets)]
        pos = edge_sample(a6[i], b6[i], k)
        w = xform(np.eye(3), pos, vfar)
        e = np.cross(u, d)
        env[i] = _tip_triangle(w, u, gap * scale, radius, i % 3, (d + 0.5 * e, d - 0.5 * e) if shape == "flat" else None)
        ks[i] = k
    return a6, b6, env, ks


def edge_parts(a, b):
    """distance6(a, b) / 0.1 for poses whose angles are equal (the xyz part only)"""
    s = 0.0
    for i in range(3):
        d = a[i] - b[i]
        s += d * d
    return math.sqrt(s) / 0.1


def edge_sample(a, b, k):
    parts = edge_parts(a, b)
    return np.array([a[i] + float(k) * (b[i] - a[i]) / parts for i in range(3)])


def short_edges(robot, offset, shift=0.0):
    """two edges without samples whose END pose is tangent to a triangle: a zero-length edge and one of 0.05 (half a
    step), `shift` away from where tangent_edges puts its edges.  End points are never sampled, so both are free with
    zero samples.  Returns (a 2 x 6, b 2 x 6, env 2 x 9)."""
    rc, vfar, radius = robot_sphere(robot)
    u = (vfar - rc) / np.linalg.norm(vfar - rc)
    p, _ = _perp_frame(u)
    a6, b6 = np.zeros((2, 6)), np.zeros((2, 6))
    a6[:, :3] = coarse_lattice(2, 40.0 * max(radius, EDGE_LEN), float(offset)) + shift
    b6[0] = a6[0]
    b6[1, :3] = a6[1, :3] + 0.05 * p
    env = np.array([_tip_triangle(xform(np.eye(3), b6[i, :3], vfar), u, 0.0, radius, i) for i in range(2)])
    return a6, b6, env


ONE_TRIANGLE_ROBOT = np.array([[0.25, -0.125, 0.0, -0.125, 0.25, 0.0625, 0.0, 0.0, 0.375]])

# ---------------------------------------------------------------------------------------------- lattice triangle pairs
_P = [0, 0, 0, 4, 0, 0, 0, 4, 0]           # the z = 0 right triangle
_P3 = [0, 0, 0, 4, 0, 0, 0, 4, 4]          # box [0,4]^3, plane y = z
_PT = [0, 0, 0, 4, 0, 4, 0, 4, 0]          # plane x = z

# (name, P, Q, truth): truth is the geometric fact where the construction makes it certain, None for degenerate
# triangles (there only the exact 17-axis answer is defined)
_BASE_PAIRS = [
    ("pierce_face", _P, [1, 1, -2, 1, 1, 2, 3, 3, 2], True),
    ("pierce_two_edges", _P, [1, 1, -1, 2, 1, 1, 1, 2, 1], True),
    ("vertex_vertex_coplanar_side", _P, [4, 0, 0, 8, 0, 0, 4, 4, 4], True),
    ("vertex_vertex_above", _P, [0, 0, 0, -1, -1, 3, -2, 1, 3], True),
    ("vertex_edge_coplanar", _P, [2, 0, 0, 1, -3, 0, 3, -3, 0], True),
    ("vertex_edge_upright", _P, [2, 0, 0, 2, -1, 3, 2, 1, 3], True),
    ("vertex_on_hypotenuse", _P, [2, 2, 0, 3, 3, 2, 4, 4, 0], True),
    ("vertex_face", _P, [1, 1, 0, 1, 1, 3, 2, 1, 3], True),
    ("face_vertex", [1, 1, 0, 1, 1, 3, 2, 1, 3], _P, True),
    ("edge_edge_cross_point", _P, [2, -2, -2, 2, 2, 2, 2, -2, 2], True),
    ("edge_edge_collinear_coplanar", _P, [1, 0, 0, 3, 0, 0, 2, -3, 0], True),
    ("edge_edge_collinear_upright", _P, [1, 0, 0, 3, 0, 0, 2, 0, -3], True),
    ("edge_edge_collinear_partial", _P, [2, 0, 0, 6, 0, 0, 4, 0, 3], True),
    ("edge_edge_collinear_one_point", _P, [4, 0, 0, 8, 0, 0, 6, 0, 3], True),
    ("coplanar_apart_boxes_apart", _P, [5, 0, 0, 9, 0, 0, 5, 4, 0], False),
    ("coplanar_apart_boxes_overlap", _P, [4, 1, 0, 1, 4, 0, 4, 4, 0], False),
    ("coplanar_apart_below", _P, [0, -1, 0, 4, -1, 0, 2, -5, 0], False),
    ("coplanar_share_vertex", _P, [4, 0, 0, 8, 0, 0, 4, 4, 0], True),
    ("coplanar_share_edge", _P, [0, 0, 0, 4, 0, 0, 0, -4, 0], True),
    ("coplanar_share_hypotenuse", _P, [4, 0, 0, 0, 4, 0, 4, 4, 0], True),
    ("coplanar_contained", _P, [1, 1, 0, 2, 1, 0, 1, 2, 0], True),
    ("coplanar_containing", _P, [-4, -4, 0, 12, -4, 0, -4, 12, 0], True),
    ("coplanar_identical", _P, list(_P), True),
    ("coplanar_overlap", _P, [1, 1, 0, 5, 1, 0, 1, 5, 0], True),
    ("parallel_one_apart_boxes_apart", _P, [0, 0, 1, 4, 0, 1, 0, 4, 1], False),
    ("parallel_one_apart_boxes_overlap", _PT, [1, 0, 0, 5, 0, 4, 1, 4, 0], False),
    ("parallel_one_apart_shifted", _PT, [-1, 0, 0, 3, 0, 4, -1, 4, 0], False),
    ("boxes_touch_face", _P3, [4, 3, 1, 6, 3, 1, 4, 4, 3], False),
    ("boxes_touch_edge", _P3, [4, 4, 1, 6, 5, 1, 5, 6, 3], False),
    ("boxes_touch_corner", _P3, [4, 4, 4, 6, 5, 5, 5, 6, 6], False),
    ("boxes_overlap_tri_under", _P3, [2, 3, 1, 3, 3, 1, 2, 4, 1], False),
    ("collinear_in_face", _P, [1, 1, 0, 2, 2, 0, 3, 3, 0], None),
    ("collinear_through_face", _P, [1, 1, -1, 1, 1, 0, 1, 1, 1], None),
    ("collinear_near_boxes_overlap", _P, [3, 3, -1, 4, 4, 1, 5, 5, 3], None),
    ("collinear_near_above", _P, [1, 1, 1, 2, 2, 1, 3, 3, 1], None),
    ("two_equal_touching", _P, [1, 1, 0, 1, 1, 0, 1, 1, 3], None),
    ("two_equal_near", _P, [3, 3, -1, 3, 3, -1, 3, 3, 1], None),
    ("point_in_face", _P, [1, 1, 0, 1, 1, 0, 1, 1, 0], None),
    ("point_on_vertex", _P, [4, 0, 0, 4, 0, 0, 4, 0, 0], None),
    ("point_near_in_plane", _P, [3, 3, 0, 3, 3, 0, 3, 3, 0], None),
    ("point_near_above", _P3, [1, 2, 3, 1, 2, 3, 1, 2, 3], None),
]


def _map_tri(t, M, s, T):
    v = np.asarray(t, dtype=np.int64).reshape(3, 3)
    return ((v @ np.asarray(M, dtype=np.int64).T) * s + np.asarray(T, dtype=np.int64)).reshape(9).tolist()


def lattice_triangle_pairs():
    """[(name, P, Q, truth)] with integer coordinates, |x| <= 512: every product of the 17-axis test is exact in fp64.
    The hand-built pairs, and each of them again rotated by 90 degrees about two axes, scaled by 32 and moved far from the
    origin - the same geometric fact in other coordinates (other axes carry the decision, other magnitudes)."""
    out = [(n, list(p), list(q), t) for n, p, q, t in _BASE_PAIRS]
    M = [[0, 0, 1], [1, 0, 0], [0, -1, 0]]
    for n, p, q, t in _BASE_PAIRS:
        out.append((n + "/moved", _map_tri(p, M, 32, [37, -120, 101]), _map_tri(q, M, 32, [37, -120, 101]), t))
    for _, p, q, _ in out:
        assert max(abs(x) for x in p + q) <= 512
    return out


def rotations24():
    """the 24 proper rotations that permute the axes (entries 0 / +-1): exact in any arithmetic"""
    out = []
    for perm in itertools.permutations(range(3)):
        for sg in itertools.product((1, -1), repeat=3):
            M = np.zeros((3, 3), dtype=np.int64)
            for i in range(3):
                M[i, perm[i]] = sg[i]
            if round(np.linalg.det(M)) == 1:
                out.append(M)
    assert len(out) == 24
    return out


def super_lattice(j, pitch=4096):
    return np.array([j % 4, (j // 4) % 4, j // 16], dtype=np.int64) * pitch


# ---------------------------------------------------------------------------------------------- lattice node stores
STORE_SIZES = [1, 63, 64, 65, 255, 256, 257, 1021, 1022, 1023]
CENTRE = (4, 4, 4)           # the families' centre = the main query, a corner of the cell grid
CLUMP_AT = (6, 4, 4)         # 100 bit-identical nodes, also on a cell corner


def _signed_perms(v):
    out = set()
    for p in itertools.permutations(v):
        for sg in itertools.product((1, -1), repeat=len(v)):
            out.add(tuple(a * b for a, b in zip(p, sg)))
    return sorted(out)


def _family(axis_len, legs):
    """offsets at distance axis_len: the six axis points FIRST (lower ids, and in a shell of the cell grid farther out than
    the mixed ones: |offset|_inf is larger), then the signed permutations of `legs`"""
    return [o + (0, 0, 0) for o in _signed_perms((axis_len, 0, 0))] + [o + (0, 0, 0) for o in _signed_perms(legs)]


def _units():
    """the whole node set in lattice units (integers), ordered so that every prefix in STORE_SIZES is interesting"""
    c = np.array(CENTRE + (0, 0, 0))
    rows = [tuple(c)]                                                         # n = 1: one node, at the query
    rows += [tuple(c + np.array(o)) for o in _family(5, (3, 4, 0))]            # 30 at exactly 5 (ids 1..30)
    rows += [tuple(np.array(CLUMP_AT + (0, 0, 0)))] * 100                      # ids 31..130: cut at 63 / 64 / 65 inside it
    rows += [tuple(c + np.array(o)) for o in _family(3, (1, 2, 2))]            # 30 at exactly 3
    six = [o for o in _signed_perms((1, 1, 1, 1, 0, 0)) if sum(o) in (4, -4, 0) and o[0] >= 0][:56]
    rows += [tuple(c + np.array(o)) for o in _signed_perms((2, 0, 0, 0, 0, 0))]  # 12 at exactly 2, angle axes included
    rows += [tuple(c + np.array(o)) for o in six]                              # (1,1,1,1) in 6-D: exactly 2
    rows += [tuple(c + np.array(o)) for o in _family(7, (2, 3, 6))]            # 54 at exactly 7
    block = [(x, y, z, 0, 0, 0) for z in range(9) for y in range(9) for x in range(9)]   # 729: every cell corner of [0,8]^3
    rows += block
    rows += [tuple(c + np.array(o)) for o in _family(20, (12, 16, 0))]         # 30 at exactly 20 (5 at quarter pitch)
    return np.array(rows, dtype=np.int64)


def lattice_store(kind="all", n=None, pitch=1.0, shift=0.0):
    """Node sets on a lattice, as a dict: pts (n x 6), tree (n), limits / cell for sffgpu_nodes_index (the set's extent and
    the lattice pitch), queries (nq x 6), radii (populated distances whose squares are on the lattice).

    kind: "families" (3-4-5, 1-2-2, 2-3-6, 12-16-20 and the 6-D (1,1,1,1) offsets around the centre, axis points first),
    "clump" (100 bit-identical nodes - more than a top-64 list, more than a grid bucket - plus the centre and its 3-4-5
    shell), "block" (a full 9 x 9 x 9 block at the cell pitch: nodes on cell faces, edges, corners and on the outer
    faces of the index limits), "all" (everything; `n` cuts a prefix of it - STORE_SIZES).
    Coordinates = units * pitch (+ shift on x y z): pitch 1 gives integers, pitch 0.25 quarter-integers and angles that
    are multiples of 0.25."""
    U = _units()
    block0 = 1 + 30 + 100 + 30 + 12 + 56 + 54
    if kind == "families":
        U = np.vstack([U[:31], U[131:block0], U[block0 + 729:]])
    elif kind == "clump":
        U = U[:131]
    elif kind == "block":
        U = U[block0:block0 + 729]
    else:
        assert kind == "all"
    if n is not None:
        assert n <= len(U)
        U = U[:n]
    pts = U.astype(np.float64) * pitch
    pts[:, :3] += shift
    tree = (np.arange(len(U)) % 3).astype(np.int32)
    lo, hi = pts[:, :3].min(axis=0), pts[:, :3].max(axis=0)
    limits = [lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]]
    qu = np.array([
        CENTRE + (0, 0, 0),                 # on a node, the centre of every family
        CLUMP_AT + (0, 0, 0),               # on the clump: 100 nodes at d = 0
        (4.5, 4.5, 4, 0, 0, 0),             # on a cell face
        (4.5, 4, 4, 0, 0, 0),               # on a cell edge
        (0, 0, 0, 0, 0, 0),                 # a corner of the block
        (8, 8, 8, 0.25, -0.5, 0.75),         # the opposite corner, with angles
        (-30, 4, 4, 0, 0, 0),               # outside the limits, on a face's normal
        (41.25, 40, -34.75, 0, 0, 0),       # outside the limits, off a corner
    ], dtype=np.float64) * pitch
    qu[:, :3] += shift
    return dict(pts=pts, tree=tree, limits=limits, cell=float(pitch), queries=qu,
                radii=[5.0 * pitch, 3.0 * pitch, 7.0 * pitch, 2.0 * pitch, 20.0 * pitch])


def twin_store():
    """Two nodes at exactly 5 from the query (4,4,4): id 0 = (4,4,9) lies in shell 5 of a unit cell grid, id 1 = (7,8,4) in
    shell 4.  With the query's own node (id 2) the two nearest are [2, 0]: a shell search that stops as soon as it holds k
    nodes no farther than the shells it has seen keeps id 1 instead.  Padded with far nodes to more than 64."""
    rows = [(4, 4, 9, 0, 0, 0), (7, 8, 4, 0, 0, 0), (4, 4, 4, 0, 0, 0)]
    rows += [(x, y, 0, 0, 0, 0) for x in range(-8, 17, 2) for y in range(-8, 17, 2) if abs(x - 4) + abs(y - 4) > 12]
    pts = np.array(rows, dtype=np.float64)
    lo, hi = pts[:, :3].min(axis=0), pts[:, :3].max(axis=0)
    return dict(pts=pts, tree=np.zeros(len(pts), np.int32), limits=[lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]], cell=1.0,
                queries=np.array([[4, 4, 4, 0, 0, 0]], dtype=np.float64), radii=[5.0])


def nudged(r):
    """r and its two neighbours in the doubles"""
    return [float(np.nextafter(r, 0.0)), float(r), float(np.nextafter(r, np.inf))]


# ---------------------------------------------------------------------------------------------- the wrap seam
PI = 3.14159265358979323846          # SFFG_PI / M_PI as a double


def _angle_at(a, delta):
    """an angle b near a + delta with fl(b - a) == delta exactly (the sum itself rounds)"""
    b0 = a + delta
    cand = [b0]
    up = dn = b0
    for _ in range(8):
        up, dn = float(np.nextafter(up, np.inf)), float(np.nextafter(dn, -np.inf))
        cand += [up, dn]
    for b in cand:
        if b - a == delta:
            return b
    raise AssertionError("no angle realises the difference %r from %r" % (delta, a))


def wrap_seam_store():
    """node / query angle pairs whose difference b - a sits on +-pi and +-3 pi, on their neighbours towards zero and on
    their neighbours away from zero (the definition wraps ONCE: a difference of 3 pi stays at pi), |angle| < 8.
    Query j has all three angles at A_j; for each of its differences and each angle axis there is one node at the query's
    own xyz (its distance IS the wrapped angle) and one a lattice unit away.  Every query also sees every other query's
    nodes.  Reference: the oracle's fp64 expressions, not the exact integers."""
    fam = [(0.0, PI), (0.0, -PI), (-4.5, 3 * PI), (4.5, -3 * PI)]
    rows, queries = [], []
    for a, base in fam:
        if [1, 1, 0, a, a, a] not in queries:
            queries.append([1, 1, 0, a, a, a])
        for dl in (base, float(np.nextafter(base, 0.0)), float(np.nextafter(base, base * 2))):
            b = _angle_at(a, dl)
            for axis in range(3):
                for xyz in ((1, 1, 0), (1, 2, 0)):
                    r = list(xyz) + [a, a, a]
                    r[3 + axis] = b
                    rows.append(r)
    pts = np.array(rows, dtype=np.float64)
    queries = np.array(queries, dtype=np.float64)
    assert np.abs(pts[:, 3:]).max() < 8 and np.abs(queries[:, 3:]).max() < 8
    return dict(pts=pts, tree=np.zeros(len(pts), np.int32), limits=[0.0, 2.0, 0.0, 3.0, 0.0, 1.0], cell=1.0, queries=queries,
                radii=nudged(PI) + [float(np.hypot(PI, 1.0)), 4.0, 7.5])
