"""SFFGPU_PRIO_GOAL_LOOP: the knob that lets a forest with both a goal and a priority bias, run in waves
of one slot, stay in the single-wavefront loop and join forest batches.  Off by default; read by csrc/knobs.cpp like every
other knob; the knobs of the two single modes do not switch it on, and it does not switch them on.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "space_filling_forest_star_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("prio_goal_loop_knob") / "prio_goal_loop_knob_harness"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "prio_goal_loop_knob_harness.cpp"), os.path.join(CSRC, "knobs.cpp"), "-o", str(out)])

    def run(**env):
        return subprocess.check_output([str(out)], env=env, text=True).strip()
    return run


def test_prio_goal_loop_is_off_unless_asked_for(harness):
    assert harness() == "prio_goal_loop=0 prio_loop=0 goal_loop=0"
    assert harness(SFFGPU_PRIO_GOAL_LOOP="1") == "prio_goal_loop=1 prio_loop=0 goal_loop=0"
    assert harness(SFFGPU_PRIO_GOAL_LOOP="0") == "prio_goal_loop=0 prio_loop=0 goal_loop=0"


def test_the_single_modes_knobs_do_not_switch_it_on(harness):
    assert harness(SFFGPU_PRIO_LOOP="1") == "prio_goal_loop=0 prio_loop=1 goal_loop=0"
    assert harness(SFFGPU_GOAL_LOOP="1") == "prio_goal_loop=0 prio_loop=0 goal_loop=1"
    assert harness(SFFGPU_PRIO_LOOP="1", SFFGPU_GOAL_LOOP="1") == "prio_goal_loop=0 prio_loop=1 goal_loop=1"


def test_prio_goal_loop_is_documented():
    text = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    sec10 = text[text.index("\n## 10. "):text.index("\n## 11. ")]
    assert "SFFGPU_PRIO_GOAL_LOOP" in sec10
