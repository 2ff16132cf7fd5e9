"""SFFGPU_PATHS_DEV and SFFGPU_TEST_PATHS_CAP: the knob that sends sffgpu_forest_paths through the
batch entry (k_paths_batch where the forest lives on the device), off by default, and the tests' bound of a forest's plan pool
on the device.  Read by csrc/knobs.cpp like every other knob.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "space_filling_forest_star_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("paths_knobs") / "paths_knobs_harness"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "paths_knobs_harness.cpp"), os.path.join(CSRC, "knobs.cpp"), "-o", str(out)])

    def run(**env):
        return subprocess.check_output([str(out)], env=env, text=True).strip()
    return run


def test_defaults_and_their_own_variables(harness):
    off = "paths_dev=0 test_paths_cap=0"                 # (cap 0 = unset: the library's own bound)
    assert harness() == off
    assert harness(SFFGPU_PATHS_DEV="1") == "paths_dev=1 test_paths_cap=0"
    assert harness(SFFGPU_PATHS_DEV="0") == off
    assert harness(SFFGPU_TEST_PATHS_CAP="8") == "paths_dev=0 test_paths_cap=8"
    assert harness(SFFGPU_TEST_PATHS_CAP="0") == "paths_dev=0 test_paths_cap=1"       # (set: one entry at least)
    assert harness(SFFGPU_TEST_PATHS_CAP="-3") == "paths_dev=0 test_paths_cap=1"
    assert harness(SFFGPU_TEST_PATHS_CAP="1000000000") == "paths_dev=0 test_paths_cap=%d" % (1 << 24)
    assert harness(SFFGPU_PATHS_DEV="1", SFFGPU_TEST_PATHS_CAP="64") == "paths_dev=1 test_paths_cap=64"
    # no other knob switches the route on or moves the bound: not smoothing's, not the batches' own
    for other in ("SFFGPU_SMOOTH_LOOP", "SFFGPU_SMOOTH_EDGES", "SFFGPU_GOAL_LOOP", "SFFGPU_PRIO_LOOP", "SFFGPU_COMPACT_GRID",
                  "SFFGPU_TEST_GRID_POOL", "SFFGPU_TEST_BORDER_CAP"):
        assert harness(**{other: "1"}) == off, other


def test_the_knobs_are_documented():
    text = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    sec10 = text[text.index("\n## 10. "):text.index("\n## 11. ")]
    assert "SFFGPU_PATHS_DEV" in sec10 and "SFFGPU_TEST_PATHS_CAP" in sec10
