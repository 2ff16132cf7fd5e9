"""SFFGPU_COMPACT_GRID and SFFGPU_TEST_GRID_POOL: the knob under which sffgpu_create_member makes a
member with the compact node grid, and the test knob that sets the first capacity of its bucket pool.  Both off by default;
read by csrc/knobs.cpp like every other knob.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "space_filling_forest_star_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("compact_grid_knob") / "compact_grid_knob_harness"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "compact_grid_knob_harness.cpp"), os.path.join(CSRC, "knobs.cpp"), "-o", str(out)])

    def run(**env):
        text = subprocess.check_output([str(out)], env=env, text=True).strip()
        return dict(word.split("=", 1) for word in text.split())
    return run


def test_compact_grid_is_off_unless_asked_for(harness):
    assert harness() == {"compact_grid": "0", "test_grid_pool": "0"}
    assert harness(SFFGPU_COMPACT_GRID="1")["compact_grid"] == "1"
    assert harness(SFFGPU_COMPACT_GRID="0")["compact_grid"] == "0"
    # no other knob switches it on: not the batches' own, not the node grid's test knobs
    for other in ("SFFGPU_GOAL_LOOP", "SFFGPU_PRIO_LOOP", "SFFGPU_PRIO_GOAL_LOOP", "SFFGPU_LAZY_BATCH", "SFFGPU_TEST_GRID_POOL",
                  "SFFGPU_TEST_GRID_BK", "SFFGPU_TEST_GRID_OVF", "SFFGPU_SMOOTH_LOOP"):
        assert harness(**{other: "1"})["compact_grid"] == "0", other


def test_pool_knob_parsing_and_clamp(harness):
    assert harness(SFFGPU_TEST_GRID_POOL="4") == {"compact_grid": "0", "test_grid_pool": "4"}
    assert harness(SFFGPU_TEST_GRID_POOL="4", SFFGPU_COMPACT_GRID="1") == {"compact_grid": "1", "test_grid_pool": "4"}
    assert harness(SFFGPU_TEST_GRID_POOL="0")["test_grid_pool"] == "1"              # set: at least one bucket
    assert harness(SFFGPU_TEST_GRID_POOL="-7")["test_grid_pool"] == "1"
    assert harness(SFFGPU_TEST_GRID_POOL="2000000000")["test_grid_pool"] == str(1 << 26)
    assert harness(SFFGPU_COMPACT_GRID="1")["test_grid_pool"] == "0"                # unset: the store's capacity


def test_both_knobs_are_documented():
    text = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    sec10 = text[text.index("\n## 10. "):text.index("\n## 11. ")]
    assert "SFFGPU_COMPACT_GRID" in sec10 and "SFFGPU_TEST_GRID_POOL" in sec10
