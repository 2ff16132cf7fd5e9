"""CPU checks of the member-context interface (sffgpu_create_member, sffgpu_ctx_get_memory): declared, exported, bound, the
struct laid out alike in the header and in ctypes, and NULL arguments refused before anything touches a GPU."""
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


def header():
    src = open(os.path.join(ROOT, "include", "sffgpu.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_both_functions_and_the_struct():
    src = header()
    assert re.search(r"\bint\s+sffgpu_create_member\s*\(\s*sffgpu_ctx\s*\*\s*owner\s*,\s*sffgpu_ctx\s*\*\s*\*\s*out\s*\)\s*;", src)
    assert re.search(r"\bint\s+sffgpu_ctx_get_memory\s*\(\s*sffgpu_ctx\s*\*\s*\w*\s*,\s*sffgpu_ctx_memory\s*\*\s*out\s*\)\s*;", src)
    assert re.search(r"typedef struct \{[^}]*\} sffgpu_ctx_memory;", src)


def test_library_exports_and_python_binds_them():
    L = S.lib()
    for name in ("sffgpu_create_member", "sffgpu_ctx_get_memory"):
        assert hasattr(L, name), name
        assert name in S.EXPORTED_SYMBOLS
    assert L.sffgpu_create_member.argtypes == [C.c_void_p, C.POINTER(C.c_void_p)]
    assert L.sffgpu_ctx_get_memory.argtypes == [C.c_void_p, C.POINTER(S.CtxMemory)]
    assert callable(S.Context.member) and callable(S.Context.memory)
    assert "CtxMemory" in S.__all__


def test_struct_fields_agree_between_header_and_ctypes():
    body = re.search(r"typedef struct \{([^}]*)\} sffgpu_ctx_memory;", header()).group(1)
    decls = [d.strip().split(None, 1) for d in body.split(";") if d.strip()]
    assert all(t == "uint64_t" for t, _ in decls)
    names = [n.strip() for _, rest in decls for n in rest.split(",")]
    assert names == ["env_bytes", "env_holders", "store_bytes", "grid_bytes", "round_grid_bytes", "other_bytes", "total_bytes"]
    assert names == [k for k, _ in S.CtxMemory._fields_]
    assert all(t is C.c_uint64 for _, t in S.CtxMemory._fields_)
    assert C.sizeof(S.CtxMemory) == 8 * len(names)
    assert list(S.CtxMemory().as_dict()) == names


def test_null_arguments_are_argument_errors():
    L = S.lib()
    out = C.c_void_p(0x1234)
    assert L.sffgpu_create_member(None, C.byref(out)) == -1          # SFFGPU_ERR_ARG
    assert not out.value, "a refused call leaves no handle behind"
    assert L.sffgpu_create_member(None, None) == -1
    m = S.CtxMemory()
    assert L.sffgpu_ctx_get_memory(None, C.byref(m)) == -1
    assert L.sffgpu_ctx_get_memory(None, None) == -1
    # a NULL `out` is refused before the context is looked at: any non-NULL address stands in for one
    stand_in = C.create_string_buffer(64)
    assert L.sffgpu_ctx_get_memory(C.addressof(stand_in), None) == -1
    assert L.sffgpu_create_member(C.addressof(stand_in), None) == -1
