"""CPU checks of sffgpu_ctx_grid_compact: declared in the header, listed in EXPORTED_SYMBOLS, exported by the built library,
bound on the Python side, and a NULL context refused before anything touches a GPU."""
import os
import re
import subprocess

import pytest

import space_filling_forest_star_amd as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(S.lib_path()):
        S.build_library()


def test_header_declares_it():
    src = open(os.path.join(ROOT, "include", "sffgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+sffgpu_ctx_grid_compact\s*\(\s*sffgpu_ctx\s*\*\s*\w*\s*\)\s*;", code)
    # ... with the rules as its comment: the knob, and that everything outside the one-wavefront loops makes the grid dense
    comment = src[:src.index("int sffgpu_ctx_grid_compact")].rsplit("/*", 1)[1]
    assert "SFFGPU_COMPACT_GRID" in comment and "dense" in comment and "sffgpu_create" in comment


def test_library_exports_and_python_binds_it():
    assert "sffgpu_ctx_grid_compact" in S.EXPORTED_SYMBOLS
    L = S.lib()
    assert hasattr(L, "sffgpu_ctx_grid_compact")
    import ctypes as C
    assert L.sffgpu_ctx_grid_compact.argtypes == [C.c_void_p]
    assert callable(S.Context.grid_compact)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", S.lib_path()], text=True)
    assert re.search(r"\bT sffgpu_ctx_grid_compact$", syms, re.M)


def test_null_context_is_an_argument_error():
    assert S.lib().sffgpu_ctx_grid_compact(None) == -1          # SFFGPU_ERR_ARG
