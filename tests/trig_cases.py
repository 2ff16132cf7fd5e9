"""Arguments that sit ON the branches of the portable trig (csrc/sff_pmath.h) and of the sampling code around it
(csrc/sff_geom.h: canonical, uniform_real, sample_point_with, steer), and the engine words that produce them.

Nothing here needs a GPU or imports the product.  word -> double follows libstdc++'s generate_canonical on one 64-bit
word: double(w) / 2^64 (round to nearest even: what Python's float(int) does), clamped below 1; an angle is
canonical * (pi - -pi) + -pi, an arccosine argument 1 - 2 * (canonical * (1 - 0) + 0).  tests/test_gpu_trig_edges.py
checks this model against the oracle's own arithmetic before anything relies on it.
"""
import math
from fractions import Fraction

import numpy as np

PI = 3.14159265358979323846            # SFFG_PI / M_PI as a double
PI_2 = 1.57079632679489661923
BRANCH = 0.78539816339744827900        # the literal of psin / pcos: |x| <= BRANCH takes the kernel without reduction
INVPIO2 = 6.36619772367581382433e-01
DOMAIN = 1048576.0 * PI_2              # SFFP_TRIG_DOMAIN: 2^20 * pi/2
STEP = 1 << 11                         # one step of the 53-bit canonical value, for words >= 2^63
TOP = (1 << 64) - 1


def canonical(w):
    r = float(int(w)) / 18446744073709551616.0
    return 0.99999999999999988898 if r >= 1.0 else r


def sample_angle(w):
    return canonical(w) * (PI - -PI) + -PI


def sample_acos_arg(w):
    return 1 - 2 * (canonical(w) * (1.0 - 0.0) + 0.0)


def flips(w):
    """the pitch flip of sample_point_with: uniform_real(w[4], 0, 1) < 0.5"""
    return canonical(w) * (1.0 - 0.0) + 0.0 < 0.5


def quadrant(x):
    """rem_pio2's k (round-half-even of x * 2/pi, as the header's rint_even gives it)"""
    big = 6755399441055744.0
    return int((x * INVPIO2 + big) - big)


def neighbours(x, n):
    """x and its n neighbours in the doubles on either side"""
    out = [float(x)]
    up = dn = float(x)
    for _ in range(n):
        up, dn = float(np.nextafter(up, np.inf)), float(np.nextafter(dn, -np.inf))
        out += [up, dn]
    return out


def clip_word(w):
    return min(max(int(w), 0), TOP)


def word_nearest_angle(t):
    """the multiple of 2^11 whose sample_angle is nearest to t (the lowest such word)"""
    c = (Fraction(t) + Fraction(PI)) / (2 * Fraction(PI))
    w0 = clip_word(int(c * (1 << 53)) * STEP)
    cand = sorted({clip_word(w0 + j * STEP) for j in range(-8, 9)})
    return min(cand, key=lambda w: (abs(Fraction(sample_angle(w)) - Fraction(t)), w))


def steps_around(w, n=3):
    return sorted({clip_word(w + j * STEP) for j in range(-n, n + 1)})


# ---------------------------------------------------------------------------------------------- the crafted words
def angle_words():
    """{target angle: words}: for k pi/4, k = -4 .. 4, the word nearest to it and that word +- 1, 2, 3 steps of 2^11;
    the same for +-BRANCH and its two neighbours (one step of the words is several ulps there: these join k = +-1)"""
    out = {}
    for k in range(-4, 5):
        out[k * PI / 4] = steps_around(word_nearest_angle(k * PI / 4))
    for s in (1.0, -1.0):
        for t in neighbours(BRANCH, 1):
            out[s * t] = steps_around(word_nearest_angle(s * t))
    return out


def conversion_words():
    """u64 -> double, for which the device has no instruction: exact ties with the kept bit even and odd, one below and one
    above a tie, the words that round up to 2^64 (the r >= 1 clamp), the smallest words"""
    rs = np.random.RandomState(41)
    ms = [1 << 52, (1 << 52) + 1, (1 << 53) - 2, (1 << 53) - 1] + [(1 << 52) + int(v) for v in rs.randint(0, 1 << 52, 8, dtype=np.int64)]
    assert any(m % 2 == 0 for m in ms[4:]) and any(m % 2 == 1 for m in ms[4:])
    ties = [STEP * m + 0x400 for m in ms]
    near = [STEP * m + d for m in ms for d in (0x3FF, 0x401)]
    # below 2^53 every word is a double; above, the kept bit moves with the magnitude: at 2^55 a double is a multiple of 8
    mid = [(1 << 55) + 4, (1 << 55) + 12, (1 << 55) + 3, (1 << 55) + 5]
    small = [0, 1, STEP - 1]
    return dict(ties=ties, near=near, mid=mid, small=small)


def top_words():
    """2^64 - 2^10 - 2 .. 2^64 - 1: from 2^64 - 2^10 on (a tie, the kept bit odd) they round up to 2^64"""
    return list(range((1 << 64) - (1 << 10) - 2, 1 << 64))


def pitch_words():
    """w[3]: sample_acos_arg = +-0.5 (pacos's 0.5 branch), 0 (its 2^-57 branch), each +- one and two steps; 1 (word 0),
    1 - 2^-52 (2^11), -(1 - 2^-52) (2^64 - 2^11 and, through the clamp, 2^64 - 1)"""
    out = []
    for w in (1 << 62, 3 << 62, 1 << 63):
        out += steps_around(w, 2)
    return out + [0, STEP, (1 << 64) - STEP, TOP]


def flip_words():
    """w[4] around `< 0.5`: 0.5 - 2^-54 (flips), a tie that rounds to 0.5 (does not), 2^63 - 1 (rounds to 0.5), 0.5, 0.5 + 2^-53"""
    return [(1 << 63) - (1 << 10), (1 << 63) - (1 << 9), (1 << 63) - 1, 1 << 63, (1 << 63) + STEP]


def all_angle_words():
    """every word that sits in an angle slot of a crafted row (one list for test_pmath and the GPU test)"""
    cw = conversion_words()
    ws = [w for v in angle_words().values() for w in v] + cw["ties"] + cw["near"] + cw["mid"] + cw["small"] + top_words()
    return sorted(set(ws))


def from_angle(to, delta):
    """an angle a near to - delta with fl(to - a) == delta exactly: what wrap_angle(to - from) in steer then decides on.
    None where no double does (a is coarser than delta when |a| >= 4: only every other difference exists)"""
    for a in neighbours(to - delta, 16):
        if to - a == delta:
            return a
    return None


def seam_deltas():
    """(delta, wraps): `>= pi` wraps, `< -pi` wraps; pi's lower neighbour and -pi itself do not"""
    return [(PI, True), (float(np.nextafter(PI, 0.0)), False), (float(np.nextafter(PI, np.inf)), True),
            (-PI, False), (float(np.nextafter(-PI, 0.0)), False), (float(np.nextafter(-PI, -np.inf)), True)]


# ---------------------------------------------------------------------------------------------- the crafted angles
def edge_angles():
    """rotation-matrix angles on the branches of psin / pcos: k pi/4 for k = -8 .. 8 and each +- 1 ulp"""
    return [a for k in range(-8, 9) for a in neighbours(k * PI / 4, 1)]


def tiny_angles():
    return [0.0, -0.0, 5e-324, 2.0 ** -27]


def edge_angle_triples(n, seed=5):
    """n x 3: each edge / tiny angle in yaw, pitch and roll independently (the other two uniform in +-pi), all three at once
    on a boundary, the all-zero triple, a few triples in +-1e5, the rest uniform in +-2.2 pi.
    Returns (triples, groups): groups maps a name to the row indices it owns."""
    rs = np.random.RandomState(seed)
    rows, groups = [], {}

    def add(name, r):
        groups.setdefault(name, []).append(len(rows))
        rows.append(r)

    for name, vals in (("edge", edge_angles()), ("tiny", tiny_angles())):
        for a in vals:
            for slot in range(3):
                r = rs.uniform(-PI, PI, 3).tolist()
                r[slot] = a
                add(name, r)
    for a in edge_angles():
        add("edge_all", [a, a, a])
    add("zero", [0.0, 0.0, 0.0])
    for _ in range(9):
        add("far", rs.uniform(-1e5, 1e5, 3).tolist())
    assert len(rows) < n, len(rows)
    while len(rows) < n:
        add("drift", rs.uniform(-2.2 * PI, 2.2 * PI, 3).tolist())
    return np.array(rows, dtype=np.float64), groups


def ulps_apart(a, b):
    """distance of two doubles in steps of the doubles (0 for +0 / -0)"""
    def key(x):
        i = np.float64(x).view(np.int64).item()
        return i if i >= 0 else -(i & 0x7FFFFFFFFFFFFFFF)
    return abs(key(a) - key(b))


def same_bits(a, b):
    return math.copysign(1.0, a) == math.copysign(1.0, b) and a == b
