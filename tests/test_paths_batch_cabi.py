"""CPU checks of the interface of path extraction for forests together (sffgpu_forest_paths_batch and its statistics
getter): declared, exported, bound, and refusing an empty list before anything touches a GPU."""
import ctypes as C
import os
import re

import pytest

import space_filling_forest_star_amd as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sffgpu_forest_paths_batch", "sffgpu_forest_get_paths_stats"]


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(S.lib_path()):
        S.build_library()


def _header():
    src = open(os.path.join(ROOT, "include", "sffgpu.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_and_library_exports_the_symbols():
    src = _header()
    ws = r"\s*"
    assert re.search(r"\bint\s+sffgpu_forest_paths_batch" + ws + r"\(" + ws + r"sffgpu_forest\s*\*\s*const\s*\*\s*f" + ws + r"," + ws
                     + r"int\s+n" + ws + r"," + ws + r"double\s*\*\s*const\s*\*\s*dist" + ws + r"," + ws
                     + r"int32_t\s*\*\s*const\s*\*\s*connected" + ws + r"," + ws + r"int32_t\s*\*\s*n_connected" + ws + r"," + ws
                     + r"int32_t\s*\*\s*failed" + ws + r"\)" + ws + ";", src)
    assert re.search(r"\bint\s+sffgpu_forest_get_paths_stats\s*\(\s*sffgpu_forest\s*\*\s*f\s*,\s*sffgpu_paths_stats\s*\*\s*out\s*\)\s*;", src)
    # the struct field for field, and the Python mirror of it
    body = re.search(r"typedef struct \{([^}]*)\} sffgpu_paths_stats;", src, flags=re.S).group(1)
    fields = [(decl.split()[0], n.strip()) for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert fields == [("uint64_t", "calls"), ("uint64_t", "launches"), ("uint64_t", "device_calls"), ("uint64_t", "host_calls"),
                      ("uint64_t", "fallbacks"), ("uint64_t", "host_syncs"), ("uint64_t", "pairs"), ("uint64_t", "entries"),
                      ("double", "ms")]
    assert S.PathsStats._fields_ == [(n, C.c_double if t == "double" else C.c_uint64) for t, n in fields]
    assert C.sizeof(S.PathsStats) == 72
    # ... and the single calls are still there
    for name in SYMBOLS + ["sffgpu_forest_paths", "sffgpu_forest_path_plan", "sffgpu_forest_smooth_paths_batch"]:
        assert hasattr(S.lib(), name), name
        assert name in S.EXPORTED_SYMBOLS, name


def test_the_other_statistics_kept_their_last_fields():
    """the new figures live in a struct of their own: nothing was added to the statistics structs there were"""
    assert S.ForestStats._fields_[-1] == ("prio_seq_waves", C.c_uint64)
    assert S.SmoothStats._fields_[-1] == ("ms", C.c_double) and len(S.SmoothStats._fields_) == 6


def test_python_binding():
    assert callable(S.paths_batch) and "paths_batch" in S.__all__
    assert "PathsStats" in S.__all__ and callable(S.Forest.paths_stats)


def test_empty_and_null_arguments_are_argument_errors():
    L = S.lib()
    arr = (C.c_void_p * 1)(None)

    def call(h, n, failed):
        return L.sffgpu_forest_paths_batch(h, n, None, None, None, failed)

    failed = C.c_int32(7)
    assert call(None, 0, None) == -1                                  # SFFGPU_ERR_ARG
    assert call(None, 3, C.byref(failed)) == -1 and failed.value == -1
    failed = C.c_int32(7)
    assert call(arr, 0, C.byref(failed)) == -1 and failed.value == -1
    assert call(arr, -2, None) == -1
    failed = C.c_int32(7)
    assert call(arr, 1, C.byref(failed)) == -1 and failed.value == -1  # a NULL member
    out = S.PathsStats()
    assert L.sffgpu_forest_get_paths_stats(None, C.byref(out)) == -1
    with pytest.raises(S.SffGpuError):
        S.paths_batch([])
