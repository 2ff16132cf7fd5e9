"""SFFGPU_GOAL_LOOP: the knob that lets a single-goal forest of waves of one slot run in the
single-wavefront loop and join forest batches.  Off by default; read by csrc/knobs.cpp like every other knob.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "space_filling_forest_star_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("goal_loop_knob") / "goal_loop_knob_harness"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "goal_loop_knob_harness.cpp"), os.path.join(CSRC, "knobs.cpp"), "-o", str(out)])

    def run(**env):
        return subprocess.check_output([str(out)], env=env, text=True).strip()
    return run


def test_goal_loop_is_off_unless_asked_for(harness):
    assert harness() == "goal_loop=0"
    assert harness(SFFGPU_GOAL_LOOP="1") == "goal_loop=1"
    assert harness(SFFGPU_GOAL_LOOP="0") == "goal_loop=0"
    # the priority loop's knob does not switch it on
    assert harness(SFFGPU_PRIO_LOOP="1") == "goal_loop=0"


def test_goal_loop_is_documented():
    text = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    sec10 = text[text.index("\n## 10. "):text.index("\n## 11. ")]
    assert "SFFGPU_GOAL_LOOP" in sec10
