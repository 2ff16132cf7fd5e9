"""The SFFGPU_* environment knobs: csrc/knobs.cpp is the only place of the library that reads the
environment, the document lists exactly the knobs it reads, and its defaults / clamps / three-state knobs are the ones
the inline parsers had before they moved there.  No GPU: knobs.cpp is built with the host compiler alone."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "space_filling_forest_star_amd", "csrc")
# set and read on the Python side (_lib.py, bench.py), not by the library
PYTHON_SIDE = {"SFFGPU_LIB", "SFFGPU_NATIVE_RCCL"}
# include/sff/ is the drop-in solver (header-only, compiled into the CALLER's program, where knobs.cpp does not exist):
# it keeps the variables of its own, exactly these
DROPIN_CLIENT = {
    "include/sff/lazy.h": ["SFF_SEED"],
    "include/sff/rrt.h": ["SFF_SEED"],
    "include/sff/forest.h": ["SFF_WAVE", "SFF_SEED", "SFF_LIBM"],
    "include/sff/sff_gpu.h": ["SFFGPU_DEVICE"],
}


def _sources():
    for top in (CSRC, os.path.join(ROOT, "include")):
        for d, _, files in os.walk(top):
            for f in sorted(files):
                if f.endswith((".cpp", ".h", ".hip", ".inc", ".hpp", ".H")):
                    yield os.path.join(d, f)


def test_only_knobs_cpp_reads_the_environment():
    seen = {}
    for path in _sources():
        rel = os.path.relpath(path, ROOT)
        for line in open(path, encoding="utf-8", errors="replace"):
            assert not re.search(r"static\s+const[^;]*getenv", line), (rel, line)   # no value frozen at the first call
            if "getenv" in line:
                seen.setdefault(rel, []).extend(re.findall(r'getenv\("([A-Z0-9_]+)"\)', line) or [line.strip()])
    lib = {k: v for k, v in seen.items() if not k.startswith("include/sff/")}
    assert list(lib) == ["space_filling_forest_star_amd/csrc/knobs.cpp"], lib
    assert {k: v for k, v in seen.items() if k.startswith("include/sff/")} == DROPIN_CLIENT


def _section_10():
    text = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    m = re.search(r"^## 10\. .*?(?=^## 11\. )", text, re.M | re.S)
    assert m, "DESIGN.md has no section 10"
    return m.group(0)


def _documented():
    return set(re.findall(r"SFFGPU_[A-Z0-9_]*[A-Z0-9]", _section_10()))   # (every name is spelt out in full there)


def _read_by_the_library():
    src = open(os.path.join(CSRC, "knobs.cpp"), encoding="utf-8").read()
    return set(re.findall(r'"(SFFGPU_[A-Z0-9_]+)"', src))


def test_section_10_lists_exactly_the_knobs_the_library_reads():
    code, doc = _read_by_the_library(), _documented() - PYTHON_SIDE
    assert len(code) > 50
    assert code - doc == set(), "read by knobs.cpp, missing in DESIGN.md section 10"
    assert doc - code == set(), "named in DESIGN.md section 10, not read by knobs.cpp"
    sec = _section_10()
    assert "read at every launch" not in sec and "read at the first launch" not in sec


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("knobs") / "knobs_harness"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "knobs_harness.cpp"),
                           os.path.join(CSRC, "knobs.cpp"), "-o", str(out)])

    def run(**env):
        text = subprocess.check_output([str(out)], env=env, text=True)
        return dict(line.split("=", 1) for line in text.splitlines())
    return run


# the defaults of the inline parsers these knobs had before knobs.cpp (forest.cpp, forest_dev.cpp, engine.cpp, engine.h,
# rrt.cpp, kernels.hip, devstar.hip at the commit before it), written down by hand.  Enumerations: 0 = the default choice.
DEFAULTS = {
    "timer_stride": 32, "profile": 0, "no_cand": 0, "no_clearance": 0, "clear_cells": 134217728.0, "clear_hdiv": 2.0,
    "no_trigrid": 0, "tg_div": 3.0, "test_grid_bk": 8, "test_grid_bkmax": 64, "test_grid_ovf": -1,
    "query": 0, "share": -1, "seg_blocks": 0, "cull_blocks": 2048, "seg_listcap": -1, "star_knn": 0,
    "engine": 0, "prio_device": 1, "prio_seq": 0, "no_order": 0, "order_min_wave": 4096, "test_hitcap": 64, "test_nbcap": 15,
    "test_star_passes": 0, "test_exchange_self": 0, "star_tail": 1, "star_tail_wgs": 0, "test_star_stall": 0,
    "test_star_items": -1, "test_border_cap": -1, "no_graph": -1, "profiler_preloaded": 0, "no_wave_ahead": 0,
    "no_fused_sample": 0, "no_zc_status": 0, "fallback_whole_wave": 0, "kc_trace": -1, "digest": 0, "no_seq": 0, "spec": 1,
    "spec_depth": 0, "spec_sets": 1, "spec_pipe": 1, "test_spec_stall": 0, "no_dev_trig": 0, "seq_trace": "",
    "rrt_chain": 1, "rrt_fork": 1, "rrt_repair": 1, "rrt_dry": 1, "rrt_one_chain": 1, "rrt_split": 2, "rrt_small": 48,
    "rrt_grow": 150, "rrt_no_grid": 0, "rrt_no_chain_conn": 0,
}


def test_defaults_with_an_empty_environment(harness):
    got = harness()
    assert sorted(got) == sorted(DEFAULTS)
    for name, want in DEFAULTS.items():
        have = got[name] if isinstance(want, str) else float(got[name])
        assert have == want, (name, got[name], want)


def test_clamps(harness):
    for var, value, field, want in [
            ("SFFGPU_TEST_HITCAP", "100", "test_hitcap", 64), ("SFFGPU_TEST_HITCAP", "0", "test_hitcap", 1),
            ("SFFGPU_RRT_SPLIT", "0", "rrt_split", 1), ("SFFGPU_ORDER_MIN_WAVE", "1", "order_min_wave", 2),
            ("SFFGPU_SEG_BLOCKS", "99999", "seg_blocks", 4096), ("SFFGPU_SEG_BLOCKS", "-3", "seg_blocks", 1),
            ("SFFGPU_TIMER_STRIDE", "0", "timer_stride", 1), ("SFFGPU_TEST_GRID_BK", "64", "test_grid_bk", 8),
            ("SFFGPU_TEST_GRID_BKMAX", "1000", "test_grid_bkmax", 64), ("SFFGPU_RRT_GROW", "50", "rrt_grow", 100),
            ("SFFGPU_RRT_SMALL", "0", "rrt_small", 1), ("SFFGPU_TEST_STAR_PASSES", "0", "test_star_passes", 1),
            ("SFFGPU_STAR_TAIL_WGS", "0", "star_tail_wgs", 1), ("SFFGPU_TEST_STAR_STALL", "-1", "test_star_stall", 0),
            ("SFFGPU_CLEAR_CELLS", "10", "clear_cells", 512.0), ("SFFGPU_CLEAR_HDIV", "0.1", "clear_hdiv", 0.5),
            ("SFFGPU_TG_DIV", "0.5", "tg_div", 1.0), ("SFFGPU_TEST_NBCAP", "0", "test_nbcap", 1),
            # raw values: the formula that bounds them needs run-time figures and stays at the use site
            ("SFFGPU_TEST_GRID_OVF", "7", "test_grid_ovf", 7), ("SFFGPU_TEST_STAR_ITEMS", "3", "test_star_items", 3),
            ("SFFGPU_TEST_BORDER_CAP", "5", "test_border_cap", 5), ("SFFGPU_SPEC_SETS", "9", "spec_sets", 9),
            ("SFFGPU_CULL_BLOCKS", "100000", "cull_blocks", 100000), ("SFFGPU_SEG_LISTCAP", "0", "seg_listcap", 0)]:
        assert float(harness(**{var: value})[field]) == want, (var, value)


def test_three_state_and_word_knobs(harness):
    for var, field in (("SFFGPU_SHARE", "share"), ("SFFGPU_NO_GRAPH", "no_graph")):
        assert harness()[field] == "-1"
        assert harness(**{var: "0"})[field] == "0"
        assert harness(**{var: "1"})[field] == "1"
    assert harness(SFFGPU_PRIO_SEQ="0")["prio_seq"] == "0" and harness(SFFGPU_PRIO_SEQ="1")["prio_seq"] == "1"
    assert harness(SFFGPU_NO_SEQ="0")["no_seq"] == "0" and harness(SFFGPU_NO_SEQ="1")["no_seq"] == "1"
    assert harness(SFFGPU_PRIO_DEVICE="0")["prio_device"] == "0" and harness(SFFGPU_SPEC="0")["spec"] == "0"
    # set at all, whatever the value
    assert harness(SFFGPU_PROFILE="0")["profile"] == "1" and harness(SFFGPU_NO_WAVE_AHEAD="0")["no_wave_ahead"] == "1"
    assert [harness(SFFGPU_ENGINE=w)["engine"] for w in ("host", "device", "other")] == ["1", "2", "0"]
    assert [harness(SFFGPU_QUERY=w)["query"] for w in ("wide", "block", "other")] == ["1", "2", "0"]
    assert [harness(SFFGPU_STAR_KNN=w)["star_knn"] for w in ("lone", "wg")] == ["1", "0"]
    assert harness(SFFGPU_KC_TRACE="3")["kc_trace"] == "3"
    assert harness(SFFGPU_SEQ_TRACE="/tmp/t.bin")["seq_trace"] == "/tmp/t.bin"
    assert harness(LD_PRELOAD="/x/librocprofiler-sdk-tool.so")["profiler_preloaded"] == "1"
    assert harness(LD_PRELOAD="/x/libother.so")["profiler_preloaded"] == "0"
