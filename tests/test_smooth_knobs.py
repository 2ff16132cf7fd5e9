"""SFFGPU_SMOOTH_LOOP and SFFGPU_SMOOTH_EDGES: the knob that sends the single smoothing calls through
the device loop (k_smooth_paths), off by default, and the cap on the edges one launch of it tests per path.  Read by
csrc/knobs.cpp like every other knob.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "space_filling_forest_star_amd", "csrc")
DEFAULT_EDGES = 64


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("smooth_knobs") / "smooth_knobs_harness"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "smooth_knobs_harness.cpp"), os.path.join(CSRC, "knobs.cpp"), "-o", str(out)])

    def run(**env):
        return subprocess.check_output([str(out)], env=env, text=True).strip()
    return run


def test_defaults_and_their_own_variables(harness):
    off = "smooth_loop=0 smooth_edges=%d" % DEFAULT_EDGES
    assert harness() == off
    assert harness(SFFGPU_SMOOTH_LOOP="1") == "smooth_loop=1 smooth_edges=%d" % DEFAULT_EDGES
    assert harness(SFFGPU_SMOOTH_LOOP="0") == off
    assert harness(SFFGPU_SMOOTH_EDGES="1") == "smooth_loop=0 smooth_edges=1"
    assert harness(SFFGPU_SMOOTH_EDGES="1000") == "smooth_loop=0 smooth_edges=1000"
    assert harness(SFFGPU_SMOOTH_EDGES="0") == "smooth_loop=0 smooth_edges=1"        # (a launch tests one edge at least)
    assert harness(SFFGPU_SMOOTH_EDGES="-5") == "smooth_loop=0 smooth_edges=1"
    assert harness(SFFGPU_SMOOTH_LOOP="1", SFFGPU_SMOOTH_EDGES="7") == "smooth_loop=1 smooth_edges=7"
    # no other knob switches the loop on or moves the cap: not the batches' own, not an RRT session's
    for other in ("SFFGPU_GOAL_LOOP", "SFFGPU_PRIO_LOOP", "SFFGPU_PRIO_GOAL_LOOP", "SFFGPU_LAZY_BATCH", "SFFGPU_RRT_CHAIN",
                  "SFFGPU_SEG_BLOCKS", "SFFGPU_RRT_SPLIT"):
        assert harness(**{other: "1"}) == off, other


def test_the_knobs_are_documented():
    text = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    sec10 = text[text.index("\n## 10. "):text.index("\n## 11. ")]
    assert "SFFGPU_SMOOTH_LOOP" in sec10 and "SFFGPU_SMOOTH_EDGES" in sec10
