"""SFFGPU_LAZY_BATCH: the knob that lets a lazy_edge session (LazyTSP::runRRT) be a member of a
session batch.  Off by default; read by csrc/knobs.cpp like every other knob.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "space_filling_forest_star_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("lazy_batch_knob") / "lazy_batch_knob_harness"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "lazy_batch_knob_harness.cpp"), os.path.join(CSRC, "knobs.cpp"), "-o", str(out)])

    def run(**env):
        return subprocess.check_output([str(out)], env=env, text=True).strip()
    return run


def test_lazy_batch_is_off_unless_asked_for(harness):
    assert harness() == "lazy_batch=0"
    assert harness(SFFGPU_LAZY_BATCH="1") == "lazy_batch=1"
    assert harness(SFFGPU_LAZY_BATCH="0") == "lazy_batch=0"
    # no other knob switches it on: not the forest batches' three, not an RRT session's
    for other in ("SFFGPU_GOAL_LOOP", "SFFGPU_PRIO_LOOP", "SFFGPU_PRIO_GOAL_LOOP", "SFFGPU_RRT_CHAIN", "SFFGPU_RRT_NO_GRID"):
        assert harness(**{other: "1"}) == "lazy_batch=0", other


def test_lazy_batch_is_documented():
    text = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    sec10 = text[text.index("\n## 10. "):text.index("\n## 11. ")]
    assert "SFFGPU_LAZY_BATCH" in sec10
