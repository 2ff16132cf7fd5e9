"""CPU checks of the session-batch interface (sffgpu_rrt_run_batch): declared, exported, bound, its two statistics at the
end of sffgpu_rrt_stats, and refusing an empty list before anything touches a GPU."""
import ctypes as C
import os
import re

import pytest

import space_filling_forest_star_amd as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(S.lib_path()):
        S.build_library()


def test_header_declares_and_library_exports_rrt_run_batch():
    src = open(os.path.join(ROOT, "include", "sffgpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+sffgpu_rrt_run_batch\s*\(\s*sffgpu_rrt\s*\*\s*const\s*\*\s*r\s*,\s*int\s+n\s*,\s*int\s+max_iterations\s*,"
                     r"\s*int32_t\s*\*\s*failed\s*\)\s*;", src)
    assert hasattr(S.lib(), "sffgpu_rrt_run_batch")
    assert "sffgpu_rrt_run_batch" in S.EXPORTED_SYMBOLS


def test_python_binding():
    assert callable(S.run_rrt_batch) and "run_rrt_batch" in S.__all__
    assert S.RrtStats._fields_[-2:] == [("batch_launches", C.c_uint64), ("batch_host_iterations", C.c_uint64)]
    # the header's struct has the same members in the same order: the new ones behind everything that was there before
    src = open(os.path.join(ROOT, "include", "sffgpu.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} sffgpu_rrt_stats;", src, flags=re.S).group(1), flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [k for k, _ in S.RrtStats._fields_]
    assert names[-3] == "lazy_distance"


def test_empty_batch_is_an_argument_error():
    L = S.lib()
    failed = C.c_int32(7)
    assert L.sffgpu_rrt_run_batch(None, 0, 0, None) == -1          # SFFGPU_ERR_ARG
    assert L.sffgpu_rrt_run_batch(None, 3, 0, C.byref(failed)) == -1 and failed.value == -1
    arr = (C.c_void_p * 1)(None)
    failed.value = 7
    assert L.sffgpu_rrt_run_batch(arr, 0, 0, C.byref(failed)) == -1 and failed.value == -1
    failed.value = 7
    assert L.sffgpu_rrt_run_batch(arr, -2, 0, C.byref(failed)) == -1 and failed.value == -1
    assert L.sffgpu_rrt_run_batch(arr, 1, 0, None) == -1           # a NULL member
    with pytest.raises(S.SffGpuError):
        S.run_rrt_batch([])


def test_no_getenv_outside_knobs():
    """the batch runner adds no environment knob: knobs.cpp stays the only reader (tests/test_knobs.py pins the rest)"""
    csrc = os.path.join(ROOT, "space_filling_forest_star_amd", "csrc")
    for fn in ("rrt_batch.cpp", "rrt_seq_batch.inc"):
        assert "getenv" not in open(os.path.join(csrc, fn)).read()
