"""The gfx950 build of csrc/sff_pmath.h / sff_geom.h on the arguments where that code branches, through the public entry
points only.  tests/test_pmath.py shows that the HOST build is right (against exact values); here the device build has to
produce the host build's bits:

  a) sffgpu_sample_steer on crafted engine words (tests/trig_cases.py): angles on quadrant boundaries and on the pi/4
     literal of psin / pcos, the u64 -> double conversion on ties and at the r >= 1 clamp, pacos's branch points, the
     `< 0.5` flip, the closed limits, centres on the wrap seam of steer;
  b) the device's rotation matrix at edge angles, through tangent worlds whose answer hangs on its last bit;
  c) the in-lane evaluation of a sample's five transcendental values (SFFGPU_NO_DEV_TRIG=1) in every one-slot kernel.

The tests without the gpu mark check, on the CPU, that every crafted group reaches the branch it names: a list that misses
its branch fails where no GPU is needed."""
import functools
import math

import numpy as np
import pytest

import boundary_cases as B
import common
import oracle_lib as O
import trig_cases as T

gpu = pytest.mark.gpu

LIM = [-60.0, 2060.0, -60.0, 2110.0, 0.0, 1000.0]
DIST = 14.0


@pytest.fixture(scope="module")
def S():
    import space_filling_forest_star_amd as S
    return S


# ------------------------------------------------------------------------------------------------ a) the crafted rows
def _slot_lists(dim):
    """{group name: (word slot, words)}"""
    cw = T.conversion_words()
    conv = cw["ties"] + cw["near"] + cw["mid"] + cw["small"]
    top = T.top_words()
    top_few = top[:4] + top[-3:] + top[512:516]
    g = {}
    for t, ws in T.angle_words().items():
        g["phi %+.17g" % t] = (0, ws)
    g["phi conversion"] = (0, conv)
    g["phi top"] = (0, top)
    if dim == 6:
        for t, ws in T.angle_words().items():
            g["theta %+.17g" % t] = (1, ws)
        g["theta conversion"] = (1, conv + top_few)
        g["yaw conversion"] = (2, conv + top_few)
        g["pitch"] = (3, T.pitch_words())
        g["pitch conversion"] = (3, conv + top_few)
        g["flip"] = (4, T.flip_words())
        g["roll conversion"] = (5, conv + top_few)
    return g


def _find_centre(c, sign, lim, inside):
    """a centre coordinate near c with c + sign * DIST exactly on lim (inside) or one step of the doubles beyond it"""
    c = float(c)
    assert c + sign * DIST == lim
    if inside:
        return c
    for _ in range(8):
        c = float(np.nextafter(c, sign * np.inf))
        if (c + sign * DIST - lim) * sign > 0:
            return c
    raise AssertionError("no centre puts the sample beyond %r" % lim)


def _limit_rows():
    """dim 2, phi on an axis: cos / sin are exactly +-1, out = c +- DIST an exact sum.  (word, centre, axis, expected flag)"""
    rows = []
    for word, axis, sign, lim in ((1 << 63, 0, 1.0, LIM[1]), (0, 0, -1.0, LIM[0]), (3 << 62, 1, 1.0, LIM[3]), (1 << 62, 1, -1.0, LIM[2])):
        for inside in (True, False):
            c = [500.0, 500.0, 0.0, 0.0, 0.0, 0.0]
            c[axis] = _find_centre(lim - sign * DIST, sign, lim, inside)
            rows.append((word, c, axis, sign, lim, inside))
    return rows


@functools.lru_cache(maxsize=None)
def crafted(dim):
    """words (n x 6, uint64), centres (n x 6), groups {name: row indices}, extra: the seam / limit rows' intentions"""
    groups, words, cen = {}, [], []
    lists = _slot_lists(dim)
    n_edge = sum(len(ws) for _, ws in lists.values())
    n_seam = 40 if dim == 6 else 0
    n = n_edge + 4 * n_seam * len(T.seam_deltas()) * 2      # (a seam row may need a few candidates: T.from_angle)
    rs = np.random.RandomState(17 + dim)
    rnd = rs.randint(0, 2 ** 63, size=(n, 6), dtype=np.uint64) * np.uint64(2) + rs.randint(0, 2, (n, 6)).astype(np.uint64)
    base = common.random_poses(LIM, n, 4, dim)
    base[:, 3:] *= 2.2
    i = 0
    for name, (slot, ws) in lists.items():
        for w in ws:
            row = [int(v) for v in rnd[i]]
            row[slot] = int(w)
            words.append(row)
            cen.append(base[i].tolist())
            groups.setdefault(name, []).append(len(words) - 1)
            i += 1
    seam = []
    for _ in range(n_seam):
        for pslot, wslot in ((3, 2), (5, 5)):
            for delta, wraps in T.seam_deltas():
                a = None
                while a is None:
                    row = [int(v) for v in rnd[i]]
                    c = base[i].tolist()
                    a = T.from_angle(T.sample_angle(row[wslot]), delta)
                    i += 1
                c[pslot] = a
                groups.setdefault("seam", []).append(len(words))
                seam.append((len(words), pslot, wslot, delta, wraps))
                words.append(row)
                cen.append(c)
    limit = []
    if dim == 2:
        for word, c, axis, sign, lim, inside in _limit_rows():
            words.append([word, 0, 0, 0, 0, 0])
            cen.append(c)
            groups.setdefault("limits", []).append(len(words) - 1)
            limit.append((len(words) - 1, axis, sign, lim, inside))
    return np.array(words, dtype=np.uint64), np.array(cen, dtype=np.float64), groups, dict(seam=seam, limit=limit)


@functools.lru_cache(maxsize=None)
def oracle_samples(dim):
    words, cen, _, _ = crafted(dim)
    L = O.lib()
    out, ok = np.zeros((len(words), 6)), np.zeros(len(words), np.uint8)
    limv = O.f64(LIM)
    for i in range(len(words)):
        ok[i] = L.sffo_sample_from_words(words[i].ctypes.data_as(O.c_u64p), O.dp(cen[i]), DIST, dim, O.dp(limv),
                                         O.TRIG_PORTABLE, O.dp(out[i]))
    return out, ok


def _trig(name, x):
    return getattr(O.lib(), "sffo_" + name)(float(x), O.TRIG_PORTABLE)


def model_sample(w, c, dim):
    """sample_point of csrc/sff_geom.h restated on the word model of tests/trig_cases.py (the oracle's trig and steer)"""
    w = [int(v) for v in w]
    phi = T.sample_angle(w[0])
    if dim == 2:
        return [c[0] + _trig("cos", phi) * DIST, c[1] + _trig("sin", phi) * DIST, 0.0, 0.0, 0.0, 0.0]
    theta = T.sample_angle(w[1])
    temp = np.zeros(6)
    temp[0] = c[0] + _trig("cos", theta) * _trig("sin", phi) * DIST
    temp[1] = c[1] + _trig("sin", theta) * _trig("sin", phi) * DIST
    temp[2] = c[2] + _trig("cos", phi) * DIST
    temp[3] = T.sample_angle(w[2])
    pitch = _trig("acos", T.sample_acos_arg(w[3])) + T.PI_2
    if T.flips(w[4]):
        pitch = pitch + T.PI if pitch < 0 else pitch - T.PI
    temp[4] = pitch
    temp[5] = T.sample_angle(w[5])
    out = np.zeros(6)
    O.lib().sffo_steer(O.dp(O.f64(c)), O.dp(temp), DIST, O.dp(out))
    return out.tolist()


@pytest.mark.parametrize("dim", [6, 2])
def test_the_word_model_is_the_oracles_arithmetic(dim):
    """every crafted row: the oracle's sample equals the model's bit for bit - so the angle, the arccosine argument and
    the flip the model reports for a word are the ones the oracle (and the kernels' shared header) computes"""
    words, cen, groups, _ = crafted(dim)
    out, _ = oracle_samples(dim)
    assert 1000 <= len(words) <= 6000
    for i in range(len(words)):
        assert model_sample(words[i], cen[i], dim) == out[i].tolist(), (i, words[i])


def test_the_angle_words_reach_their_branches():
    """per target k pi/4: the seven words' angles are consecutive values around the target, lie on both sides of it, and
    (odd k) fall into two different quadrants of rem_pio2 or (k = +-1) on both sides of the |x| <= pi/4 literal"""
    aw = T.angle_words()
    assert len(aw) == 9 + 4           # (the literal IS the double nearest pi/4: its own entry coincides with k = +-1)
    for t, ws in aw.items():
        ang = [T.sample_angle(w) for w in ws]
        assert ang == sorted(ang) and max(abs(a - t) for a in ang) < 8 * 2.0 ** -51, (t, ang)
        k = round(t / (T.PI / 4))
        if abs(k) == 4:                                  # the ends of the range: word 0 gives -pi, no word reaches +pi
            assert (ang[0] == -T.PI and ws[0] == 0) if k < 0 else (ang[-1] < T.PI and ws[-1] == T.TOP)
            continue
        assert ang[0] < t < ang[-1] or t in ang, (t, ang)
        if k == 0:
            assert 0.0 in ang and ws[ang.index(0.0)] == 1 << 63 and min(ang) < 0 < max(ang)
        if abs(k) == 1:
            ax = [abs(a) for a in ang]
            assert min(ax) <= T.BRANCH < max(ax), (t, ang)               # both sides of the literal
        if abs(k) == 3:
            assert len({T.quadrant(a) for a in ang}) == 2, (t, ang)       # both sides of a quadrant boundary
        if abs(k) == 2:
            assert len({T.quadrant(a) for a in ang}) == 1 and T.PI_2 in [abs(a) for a in ang]


def test_the_conversion_words_round_as_intended():
    cw = T.conversion_words()
    two53 = 2.0 ** 53
    n_even = n_odd = 0
    for w in cw["ties"]:
        m = w >> 11
        assert w & 0x7FF == 0x400 and w >= 1 << 63
        want = m if m % 2 == 0 else m + 1                  # a tie goes to the even neighbour
        assert T.canonical(w) == min(want / two53, 1 - 2.0 ** -53), w
        n_even, n_odd = n_even + (m % 2 == 0), n_odd + (m % 2 == 1)
    assert n_even >= 3 and n_odd >= 3
    for w in cw["near"]:
        m = w >> 11
        assert T.canonical(w) == min((m if w & 0x7FF == 0x3FF else m + 1) / two53, 1 - 2.0 ** -53), w
    assert [float(w) - 2.0 ** 55 for w in cw["mid"]] == [0.0, 16.0, 0.0, 8.0]
    assert [T.canonical(w) for w in cw["small"]] == [0.0, 2.0 ** -64, 2047 * 2.0 ** -64]
    top = T.top_words()
    assert [float(w) == 2.0 ** 64 for w in top] == [False, False] + [True] * 1024       # the r >= 1 clamp from 2^64 - 2^10 on
    assert all(T.canonical(w) == 1 - 2.0 ** -53 for w in top)


def test_the_pitch_and_flip_words_reach_their_branches():
    arg = {w: T.sample_acos_arg(w) for w in T.pitch_words()}
    assert arg[1 << 62] == 0.5 and arg[3 << 62] == -0.5 and arg[1 << 63] == 0.0 and arg[0] == 1.0
    assert arg[T.STEP] == 1 - 2.0 ** -52 and arg[(1 << 64) - T.STEP] == -(1 - 2.0 ** -52) == arg[T.TOP]
    # one step below / above +-0.5: pacos's `ax < 0.5` branch and its square-root branches, both signs
    assert abs(arg[(1 << 62) + T.STEP]) < 0.5 < abs(arg[(1 << 62) - T.STEP])
    assert abs(arg[(3 << 62) - T.STEP]) < 0.5 < abs(arg[(3 << 62) + T.STEP]) and arg[(3 << 62) + T.STEP] < 0
    # next to 0: |x| = 2^-52, far above the 2^-57 threshold - only 0 itself takes that branch
    assert abs(arg[(1 << 63) + T.STEP]) == 2.0 ** -52 and arg[(1 << 63) - T.STEP] == 2.0 ** -52
    fw = T.flip_words()
    assert [T.canonical(w) for w in fw] == [0.5 - 2.0 ** -54, 0.5, 0.5, 0.5, 0.5 + 2.0 ** -53]
    assert [T.flips(w) for w in fw] == [True, False, False, False, False]


def test_the_seam_and_limit_rows_are_what_they_claim():
    words, cen, groups, extra = crafted(6)
    wrapped = 0
    for i, pslot, wslot, delta, wraps in extra["seam"]:
        d = T.sample_angle(int(words[i][wslot])) - cen[i][pslot]
        assert d == delta and (d >= T.PI or d < -T.PI) == wraps, (i, d, delta)
        wrapped += wraps
    assert wrapped == len(extra["seam"]) // 2 > 0
    words, cen, groups, extra = crafted(2)
    out, ok = oracle_samples(2)
    assert len(extra["limit"]) == 8
    for i, axis, sign, lim, inside in extra["limit"]:
        phi = T.sample_angle(int(words[i][0]))
        cs = (_trig("cos", phi), _trig("sin", phi))
        assert cs[axis] == sign and abs(cs[1 - axis]) < 2.0 ** -52, (phi, cs)         # exactly +-1 on the axis in question
        assert out[i][axis] == cen[i][axis] + sign * DIST                              # an exact sum: no rounding to hide behind
        assert (out[i][axis] == lim) == inside and ((out[i][axis] - lim) * sign > 0) == (not inside), (i, out[i][axis], lim)
        assert LIM[2 - 2 * axis] < out[i][1 - axis] < LIM[3 - 2 * axis]                # the other axis is well inside
        assert ok[i] == inside, (i, ok[i], inside)                                     # the closed limits, as the oracle has them


@gpu
@pytest.mark.parametrize("dim", [6, 2])
def test_sample_steer_on_crafted_words_bit_exact(S, dim):
    """one launch per dim; positions and the in_limits flag equal the oracle's bit for bit, reported per group"""
    words, cen, groups, _ = crafted(dim)
    want, want_ok = oracle_samples(dim)
    ctx = S.Context(0)
    out, ok = ctx.sample_steer(words, cen, DIST, dim, LIM)
    ctx.close()
    bad = (out.view(np.uint64) != want.view(np.uint64)).any(axis=1) | (ok != want_ok)
    for name, idx in groups.items():
        nb = int(bad[idx].sum())
        if nb or name in ("seam", "limits", "flip", "pitch", "phi top"):
            print("sample_steer dim %d, %-28s %4d rows, %d differ" % (dim, name, len(idx), nb))
    first = np.flatnonzero(bad)[:4]
    assert not bad.any(), [(int(i), [g for g, idx in groups.items() if i in idx], words[i].tolist(), out[i].tolist(), want[i].tolist())
                           for i in first]
    assert 0 < want_ok.sum() < len(want_ok) or dim == 6


# ------------------------------------------------------------------------------------------------ b) rotation matrices
N_TANGENT = 256
TANGENT_GAPS = [0.0, 2.0 ** -50, 1e-6]


def test_the_edge_angle_triples_reach_their_branches():
    tri, groups = T.edge_angle_triples(N_TANGENT)
    assert tri.shape == (N_TANGENT, 3) and np.abs(tri).max() < T.DOMAIN
    edge = T.edge_angles()
    assert len(edge) == 17 * 3
    for k in range(-8, 9):
        lo, mid, hi = sorted(T.neighbours(k * T.PI / 4, 1))
        assert lo < mid < hi
        if k % 2:                   # odd: a quadrant boundary of the reduction (or, k = +-1, the pi/4 literal) lies at or next to it
            assert abs(k) == 1 and min(abs(lo), abs(hi)) <= T.BRANCH <= max(abs(lo), abs(hi)) or \
                len({T.quadrant(a) for a in T.neighbours(k * T.PI / 4, 3)}) == 2, k
    for slot in range(3):           # every edge angle occurs in yaw, pitch and roll
        assert set(edge) <= set(tri[groups["edge"] + groups["edge_all"], slot].tolist())
        assert {0.0, 5e-324, 2.0 ** -27} <= set(tri[groups["tiny"], slot].tolist())
        assert any(math.copysign(1.0, v) < 0 and v == 0 for v in tri[groups["tiny"], slot])
    assert tri[groups["zero"][0]].tolist() == [0.0, 0.0, 0.0]
    assert np.abs(tri[groups["far"]]).max() > 5e4 and 2 * T.PI < np.abs(tri[groups["drift"]]).max() < 2.2 * T.PI


_WORLDS = {}


def edge_world(name, gap, shape):
    """(poses, env, the definition's brute-force answers) of the tangent world at the edge angles, computed once"""
    from test_gpu_boundaries import robot_mesh, rotation
    key = (name, gap, shape)
    if key not in _WORLDS:
        robot = robot_mesh(name)
        tri, _ = T.edge_angle_triples(N_TANGENT)
        poses, env = B.tangent_world(robot, N_TANGENT, 7, gap, 0.0, rotation, shape, angles=tri)
        w = O.World(env, robot, O.TRIG_PORTABLE)
        _WORLDS[key] = (poses, env, np.array([w.collide_brute(p) for p in poses], np.uint8))
    return _WORLDS[key]


def test_tangent_world_keeps_its_default_angles():
    """the generator with angles=None is what it was; with angles it differs in the angles only"""
    from test_gpu_boundaries import rotation
    p0, e0 = B.tangent_world(B.ONE_TRIANGLE_ROBOT, 12, 7, 0.0, 0.0, rotation)
    assert np.array_equal(p0[:, 3:], np.random.RandomState(7).uniform(-np.pi, np.pi, (12, 3)))
    tri, _ = T.edge_angle_triples(N_TANGENT)
    p1, e1 = B.tangent_world(B.ONE_TRIANGLE_ROBOT, 12, 7, 0.0, 0.0, rotation, angles=tri[:12])
    assert np.array_equal(p1[:, :3], p0[:, :3]) and np.array_equal(p1[:, 3:], tri[:12]) and not np.array_equal(e0, e1)


@gpu
@pytest.mark.parametrize("clearance", ["default", "off"])
@pytest.mark.parametrize("shape", ["tip", "flat"])
@pytest.mark.parametrize("name", ["one_triangle", "dense3d"])
def test_tangent_poses_at_edge_angles(S, monkeypatch, name, shape, clearance):
    """a robot that shares exactly one vertex with a triangle, posed at angles on the trig's branches: the answer hangs on
    the last bit of the device's rotation matrix.  gap 0: every pose hits; 1e-6: none; 2^-50: the definition's answer.
    Through the pose entry point (device trig) and through explicit transforms (the oracle's matrix)."""
    from test_gpu_boundaries import context, robot_mesh, rotation, upload
    ctx = context(S, monkeypatch, clearance)
    robot = robot_mesh(name)
    for gap in TANGENT_GAPS:
        poses, env, brute = edge_world(name, gap, shape)
        upload(ctx, env, robot, "env_first")
        for label, got in (("poses", ctx.collide_poses(poses)), ("transforms", ctx.collide_transforms(B.transforms_of(poses, rotation)))):
            print("edge angles %s %s %s gap=%g: oracle hits %d, gpu hits %d, differ %d"
                  % (name, shape, label, gap, brute.sum(), got.sum(), (got != brute).sum()))
            assert np.array_equal(got, brute), (label, gap, np.flatnonzero(got != brute)[:8], poses[np.flatnonzero(got != brute)[:4], 3:])
            if gap == 0.0:
                assert got.all(), "a shared vertex is a contact"
            if gap == TANGENT_GAPS[-1]:
                assert not got.any(), "a gap of 1e-6 of the magnitude is free"
    ctx.close()


# ------------------------------------------------------------------------------------------------ c) the in-lane trig path
IN_LANE = [
    ("k_seq_waves", "dense3d_coarse", 6000, 2, False, dict(SFFGPU_SPEC=0)),
    ("k_spec_waves", "dense3d", 3000, 7, False, dict()),
    ("one word per sample", "dense2d", 3000, 4, False, dict()),
    ("SFF*", "dense3d", 3000, 7, True, dict()),
]


@gpu
@pytest.mark.parametrize("label,name,iters,seed,optimize,env", IN_LANE, ids=[c[0].replace(" ", "_") for c in IN_LANE])
def test_in_lane_trig_builds_the_same_forest(S, label, name, iters, seed, optimize, env):
    """SFFGPU_NO_DEV_TRIG=1 at creation: no cos / sin / acos table, the one-slot kernels evaluate a sample's five values in two
    lanes.  The forest equals the oracle's and the same job's with the table."""
    from test_gpu_device_engine import make
    from test_gpu_parity import assert_same_forest
    ctx = S.Context(0)
    fo, fg = make(S, ctx, name, 1, iters, seed=seed, optimize=optimize, SFFGPU_NO_DEV_TRIG=1, **env)
    fo.run()
    fg.run()
    assert fo.stats()["n_nodes"] > 60
    assert_same_forest(fo, fg)
    sg = fg.stats()
    assert sg["host_fallback_waves"] == 0 and (sg["spec_steps"] > 0) == ("SFFGPU_SPEC" not in env)
    fp = fg.fingerprint()
    fg.close()
    _, ft = make(S, ctx, name, 1, iters, seed=seed, optimize=optimize, **env)
    ft.run()
    assert ft.fingerprint() == fp and ft.stats()["host_fallback_waves"] == 0
    ft.close()
    ctx.close()


@gpu
def test_in_lane_trig_in_a_forest_batch(S):
    from test_gpu_forest_batch import check_all, close_all, member
    ctxs = [S.Context(0) for _ in range(4)]
    specs = [dict(name="dense3d", seed=100, iters=1500), dict(name="dense3d", seed=101, iters=1500, optimize=True),
             dict(name="dense2d", seed=400, iters=1500), dict(name="triang", seed=300, iters=1000)]
    fps = []
    for knob in (dict(SFFGPU_NO_DEV_TRIG=1), dict()):
        pairs = [member(S, c, **sp, **knob) for c, sp in zip(ctxs, specs)]
        fos, fgs = [p[0] for p in pairs], [p[1] for p in pairs]
        for fo in fos:
            if fo.stats()["iterations"] == 0:
                fo.run()
        S.run_batch(fgs)
        for fg in fgs:
            st = fg.stats()
            assert st["batch_launches"] >= 1 and st["spec_steps"] == 0 and st["host_fallback_waves"] == 0, st
        check_all(fos, fgs)
        fps.append([fg.fingerprint() for fg in fgs])
        close_all(fgs)
    assert fps[0] == fps[1]
    for c in ctxs:
        c.close()
