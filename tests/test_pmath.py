"""The portable trig of csrc/sff_pmath.h (psin / pcos / pacos) against exact values.

Every GPU test compares the kernels with the CPU oracle, and the oracle compiles the SAME header: an error in it would
be identical on both sides.  Here the host build (through the oracle's sffo_sin / sffo_cos / sffo_acos) is compared
with mpmath at 200 bits of the same double argument, on the arguments where the code branches: quadrant boundaries,
the |x| <= pi/4 literal, pacos's 0.5 / 2^-57 / +-1 thresholds, the edge of rem_pio2's domain.

Error measure: |got - true| / 2^(floor(log2 |true|) - 52), ulps of the TRUE value; true == 0 demands got == 0.
The assertion is the header's claim: every error < 1.0.  Measured worst values are recorded in DESIGN.md section 6.
"""
import math

import numpy as np
import pytest

import oracle_lib as O
import trig_cases as T

mpmath = pytest.importorskip("mpmath")
mp = mpmath.mp
mp.prec = 200


def _fn(name):
    return getattr(O.lib(), "sffo_" + name)


def portable(name, x):
    return _fn(name)(float(x), O.TRIG_PORTABLE)


def libm(name, x):
    return _fn(name)(float(x), O.TRIG_LIBM)


def ulp_error(got, true):
    """error of `got` in ulps of the exact value `true` (an mpf)"""
    if true == 0:
        return 0.0 if got == 0.0 else math.inf
    _, e = mpmath.frexp(true)              # true = m 2^e, 0.5 <= |m| < 1: floor(log2 |true|) = e - 1
    return float(abs(mpmath.mpf(got) - true) / mpmath.ldexp(mpmath.mpf(1), int(e) - 1 - 52))


EXACT = {"sin": mpmath.sin, "cos": mpmath.cos, "acos": mpmath.acos}


def worst(name, args):
    """(worst error, its argument) of the portable function over args"""
    w, at = -1.0, None
    for x in args:
        e = ulp_error(portable(name, x), EXACT[name](mpmath.mpf(x)))
        if e > w:
            w, at = e, x
    return w, at


# ---------------------------------------------------------------------------------------------- the argument sets
def _sincos_sets():
    sets = {}
    sets["k pi/4, k = -40 .. 40, +- 3 ulps"] = [a for k in range(-40, 41) for a in T.neighbours(k * T.PI / 4, 3)]
    sets["the branch literal +- 3 ulps"] = [s * a for a in T.neighbours(T.BRANCH, 3) for s in (1.0, -1.0)]
    big = [100, 1000, 10 ** 4, 10 ** 5, 10 ** 6, 2 ** 20 - 1, 2 ** 20]
    sets["+-k pi/2 +- 2 ulps, k up to 2^20"] = [s * a for k in big for a in T.neighbours(k * T.PI / 2, 2) for s in (1.0, -1.0)]
    sets["zeros and tiny"] = [0.0, -0.0, 5e-324, 1e-300, 2.0 ** -27, 2.0 ** -26]
    sets["3000 uniform in [-pi, pi)"] = np.random.RandomState(101).uniform(-T.PI, T.PI, 3000).tolist()
    sets["2000 uniform in +-2.2 * 7"] = np.random.RandomState(102).uniform(-2.2 * 7, 2.2 * 7, 2000).tolist()
    sets["2000 uniform in +-1e6"] = np.random.RandomState(103).uniform(-1e6, 1e6, 2000).tolist()
    sets["angles of the crafted words"] = [T.sample_angle(w) for w in T.all_angle_words()]
    sets["rotation edge angles"] = T.edge_angles() + T.tiny_angles()
    return sets


def _acos_sets():
    sets = {}
    pts = [1.0, -1.0, 0.5, -0.5, 0.0, 2.0 ** -57, -2.0 ** -57, 2.0 ** -58]
    sets["branch points +- 3 ulps"] = sorted({min(1.0, max(-1.0, a)) for p in pts for a in T.neighbours(p, 3)})
    us = [0, 1, 2, 3, 2 ** 51, 2 ** 51 + 1, 3 * 2 ** 51 - 1, 3 * 2 ** 51, 2 ** 52 - 1, 2 ** 52, 2 ** 52 + 1, 2 ** 53 - 2, 2 ** 53 - 1]
    us += [int(v) for v in np.random.RandomState(104).randint(0, 2 ** 53, 4000, dtype=np.int64)]
    sets["1 - 2 u / 2^53"] = [1 - 2 * (u / 2.0 ** 53) for u in us]
    sets["arguments of the crafted pitch words"] = [T.sample_acos_arg(w) for w in T.pitch_words()]
    return sets


SINCOS = _sincos_sets()
ACOS = _acos_sets()
SINCOS_ALL = [x for v in SINCOS.values() for x in v]
ACOS_ALL = [x for v in ACOS.values() for x in v]


def test_the_sets_have_the_intended_size_and_reach_the_branches():
    assert 8000 <= len(SINCOS_ALL) <= 12000 and 4000 <= len(ACOS_ALL) <= 4200
    ax = np.abs(np.array(SINCOS_ALL))
    assert (ax <= T.BRANCH).sum() > 500 and (ax > T.BRANCH).sum() > 5000
    assert T.BRANCH in SINCOS_ALL and float(np.nextafter(T.BRANCH, 1.0)) in SINCOS_ALL
    assert {T.quadrant(x) & 3 for x in SINCOS_ALL if abs(x) > T.BRANCH} == {0, 1, 2, 3}
    assert max(abs(T.quadrant(x)) for x in SINCOS_ALL) == 2 ** 20
    a = np.abs(np.array(ACOS_ALL))
    x = np.array(ACOS_ALL)
    assert (a >= 1.0).sum() >= 2 and (a < 2.0 ** -57).sum() >= 2 and ((a < 0.5) & (a >= 2.0 ** -57)).sum() > 1000
    assert ((a >= 0.5) & (x < 0) & (a < 1)).sum() > 500 and ((a >= 0.5) & (x > 0) & (a < 1)).sum() > 500
    for p in (0.5, -0.5, float(np.nextafter(0.5, 0.0)), 2.0 ** -57, float(np.nextafter(2.0 ** -57, 0.0)), float(np.nextafter(1.0, 0.0))):
        assert p in ACOS_ALL, p


@pytest.mark.parametrize("name", ["sin", "cos"])
def test_sine_and_cosine_within_one_ulp_of_the_exact_value(name):
    w_all, at_all = -1.0, None
    for label, args in SINCOS.items():
        w, at = worst(name, args)
        print("p%s  %-36s %5d arguments, worst error %.3f ulp at %r" % (name, label, len(args), w, at))
        if w > w_all:
            w_all, at_all = w, at
    print("p%s  worst error %.3f ulp at %r (%d arguments)" % (name, w_all, at_all, len(SINCOS_ALL)))
    assert w_all < 1.0, (w_all, at_all)


def test_arccosine_within_one_ulp_of_the_exact_value():
    w_all, at_all = -1.0, None
    for label, args in ACOS.items():
        w, at = worst("acos", args)
        print("pacos %-36s %5d arguments, worst error %.3f ulp at %r" % (label, len(args), w, at))
        if w > w_all:
            w_all, at_all = w, at
    print("pacos worst error %.3f ulp at %r (%d arguments)" % (w_all, at_all, len(ACOS_ALL)))
    assert w_all < 1.0, (w_all, at_all)


def test_exact_results():
    assert T.same_bits(portable("sin", 0.0), 0.0) and T.same_bits(portable("sin", -0.0), -0.0)
    assert portable("cos", 0.0) == 1.0 and portable("cos", -0.0) == 1.0
    assert portable("sin", 5e-324) == 5e-324 and portable("sin", -5e-324) == -5e-324
    assert T.same_bits(portable("acos", 1.0), 0.0)
    assert portable("acos", -1.0) == T.PI and float(mpmath.pi) == T.PI          # the double nearest pi
    assert portable("acos", 0.0) == T.PI_2 and float(mpmath.pi / 2) == T.PI_2


@pytest.mark.parametrize("name,args", [("sin", SINCOS_ALL), ("cos", SINCOS_ALL), ("acos", ACOS_ALL)])
def test_portable_and_glibc_never_differ_by_more_than_one_ulp(name, args):
    """what README, include/sffgpu.h (libm_sampling) and the libm parity runs rely on"""
    worst_d, at, n_diff = 0, None, 0
    for x in args:
        d = T.ulps_apart(portable(name, x), libm(name, x))
        n_diff += d != 0
        if d > worst_d:
            worst_d, at = d, x
    print("p%s against glibc: differs in %d of %d arguments (%.1f %%), at most %d ulp (at %r)"
          % (name, n_diff, len(args), 100.0 * n_diff / len(args), worst_d, at))
    assert worst_d <= 1, (worst_d, at)


def test_symmetries_hold_bit_for_bit():
    for x in SINCOS_ALL:
        assert T.same_bits(portable("sin", -x), -portable("sin", x)), x
        assert T.same_bits(portable("cos", -x), portable("cos", x)), x
    ulp_pi = 2.0 ** -51
    w, at = 0.0, None
    for x in ACOS_ALL:
        e = float(abs(mpmath.mpf(portable("acos", x)) + mpmath.mpf(portable("acos", -x)) - mpmath.pi)) / ulp_pi
        if e > w:
            w, at = e, x
    print("pacos(x) + pacos(-x) - pi: at most %.3f ulp of pi (at %r)" % (w, at))
    assert w <= 2.0, (w, at)


def test_the_domain_of_the_reduction():
    """rem_pio2 is exact while k * P1 and k * P2 are exact products: P1 and P2 carry 33 significant bits, so for |k| <= 2^20,
    |x| <= SFFP_TRIG_DOMAIN = 2^20 * pi/2.  Up to there the claim holds; beyond it the error is printed only (the entry
    points refuse such angles: tests/test_gpu_edge_cases.py)."""
    for c in (1.57079632673412561417e+00, 6.07710050630396597660e-11):          # P1, P2 of rem_pio2
        m, _ = math.frexp(c)
        assert (m * 2.0 ** 33).is_integer()
    assert T.DOMAIN == 2.0 ** 20 * (math.pi / 2) and abs(T.quadrant(T.DOMAIN)) == 2 ** 20
    args = np.random.RandomState(105).uniform(-T.DOMAIN, T.DOMAIN, 2000).tolist()
    args += [s * a for a in T.neighbours(T.DOMAIN, 3) for s in (1.0, -1.0)]
    for name in ("sin", "cos"):
        w, at = worst(name, args)
        print("p%s  up to the domain bound %r: worst error %.3f ulp at %r" % (name, T.DOMAIN, w, at))
        assert w < 1.0, (name, w, at)
    for x in (1e7, 1e9, 1e12):
        print("outside the domain, x = %g: psin off by %.3g ulp, pcos by %.3g ulp"
              % (x, worst("sin", [x])[0], worst("cos", [x])[0]))


# sha256 over the result bits of psin and pcos on SINCOS_ALL and pacos on ACOS_ALL, in that order (little-endian doubles).
# The tests above hold the header to its accuracy claim; a change far below one ulp (a late digit of a coefficient, `<` against
# `<=` on a branch whose two sides are both accurate) passes them and still moves the bits every parity test and golden file
# is built on.  Not a bound: a recorded result.  Whoever changes sff_pmath.h on purpose re-records it, with the golden files.
RESULT_BITS = "9adc19e1bc75947c6f40860e2dfd560e2dff0f389bece49384bcf7b721a71a08"


def test_result_bits_are_pinned():
    import hashlib
    h = hashlib.sha256()
    for name, args in (("sin", SINCOS_ALL), ("cos", SINCOS_ALL), ("acos", ACOS_ALL)):
        h.update(np.array([portable(name, x) for x in args], dtype="<f8").tobytes())
    print("result bits: sha256 %s" % h.hexdigest())
    assert h.hexdigest() == RESULT_BITS
