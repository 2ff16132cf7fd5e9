"""The two decision rules of path extraction (csrc/paths_rules.h: getPaths' border pick, getAllPaths' join), compiled with
the host compiler alone and run on synthetic inputs.  The kernel (devpaths.hip) compiles the same header.  The expected
figures are worked out here in Python, edge by edge, in the order the reference adds them.  No GPU."""
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "space_filling_forest_star_amd", "csrc")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    out = tmp_path_factory.mktemp("paths_rules") / "paths_rules_harness"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "paths_rules_harness.cpp"), "-o", str(out)])
    text = subprocess.check_output([str(out)], text=True)
    got = {}
    for ln in text.splitlines():
        if "=" in ln.split()[0]:
            k, v = ln.split("=", 1)
            got[k] = v
        else:
            name, rest = ln.split(None, 1)
            got[name] = dict(kv.split("=", 1) for kv in rest.split() if "=" in kv)
            got[name]["none"] = rest.endswith("none")
    return got


def cost(xs):
    """the joined plan's cost over nodes on the x axis, added from left to right"""
    d = 0.0
    for a, b in zip(xs, xs[1:]):
        d += math.sqrt((a - b) * (a - b))
    return d


def test_border_pick_is_the_references_rule_not_an_argmin(lines):
    assert lines["pick2"] == "0"             # 1.0 and 1.0 - 6e-10: the first stays
    assert lines["pick3"] == "2"             # ... add 1.0 - 1.5e-9: the third wins
    assert lines["pick_first_zero"] == "0"   # a first border of cost 0 is a border (the sentinel is -1)
    assert lines["pick_exact_tol"] == "0"    # smaller by exactly the tolerance is not smaller by more
    far = 2.0 ** 53                          # d_root[n1] + d_root[n2] + dist6, in that association
    assert float(lines["border_dist"]) == (far + 1.0) + 1.0 == far != far + (1.0 + 1.0)


def test_join_strips_the_shared_tail(lines):
    assert lines["tail0"]["none"] and lines["tail0"]["shared"] == "0"
    t1 = lines["tail1"]
    assert (t1["shared"], t1["last"], t1["len"], t1["plan"]) == ("1", "9", "5", "0,1,9,6,5")
    assert float(t1["dist"]) == cost([0, 1, 9, 6, 5]) == 13.0
    t3 = lines["tail3"]
    assert (t3["shared"], t3["last"], t3["len"], t3["plan"]) == ("3", "7", "5", "0,1,7,6,5")
    assert float(t3["dist"]) == cost([0, 1, 7, 6, 5]) == 9.0
    w = lines["whole"]
    assert (w["shared"], w["last"], w["len"], w["plan"], float(w["dist"])) == ("3", "7", "3", "7,6,5", 2.0)


def test_join_reads_a_plan_in_either_direction(lines):
    for name in ("tail3_rev1", "tail3_rev2", "tail3_rev12"):
        assert {k: lines[name][k] for k in ("shared", "last", "len", "plan", "dist")} == \
               {k: lines["tail3"][k] for k in ("shared", "last", "len", "plan", "dist")}, name
    assert lines["stored_forward"] == "100"   # lower node id first; equal ids: the reversed branch, as the host's else


def test_join_is_accepted_only_if_shorter_by_more_than_the_tolerance(lines):
    assert lines["shorter_by_less"]["accept"] == "0"
    assert lines["shorter_by_more"]["accept"] == "1"
    assert lines["equal"]["accept"] == "0"
    assert lines["tail1"]["accept"] == "1"    # against a row without a path


def test_the_cost_is_added_from_left_to_right(lines):
    far = 2.0 ** 53
    first, last = (far + 1.0) + 1.0, (1.0 + 1.0) + far
    assert first == far and last == far + 2.0   # the order of the additions is part of the result
    assert lines["order_long_first"]["plan"] == "0,1,2,3" and float(lines["order_long_first"]["dist"]) == first
    assert lines["order_long_last"]["plan"] == "3,2,1,0" and float(lines["order_long_last"]["dist"]) == last
