"""nbg_find_vertices / nbg_find_edges at the C boundary: the symbols are declared, exported and
bound with the header's signatures, and adding them changed no struct (ABI 7 stays)."""
import ctypes as C
import re
from pathlib import Path

import nebula_amd
from nebula_amd import _lib

HEADER = (Path(__file__).resolve().parents[1] / "include" / "nebula_amd.h").read_text()
NAMES = ("nbg_find_vertices", "nbg_find_edges")


def decl(name):
    m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", HEADER)
    assert m, f"{name} is not declared in include/nebula_amd.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbols_exported():
    L = nebula_amd.load()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert hasattr(L, name)
        assert getattr(L, name).restype is C.c_int32


def test_signatures_match_header():
    L = nebula_amd.load()
    vp, i32, sz = C.c_void_p, C.c_int32, C.c_size_t
    for name, type_arg in zip(NAMES, ("int32_t tag_id", "int32_t edge_type")):
        assert decl(name) == [
            "nbg_ctx* ctx", type_arg, "const uint8_t* where", "size_t where_len", "const uint8_t* const* yields",
            "const size_t* yield_lens", "size_t n_yields", "int32_t keep_on_device", "nbg_rows* out"]
        assert list(getattr(L, name).argtypes) == [
            vp, i32, vp, sz, C.POINTER(vp), C.POINTER(sz), sz, i32, C.POINTER(_lib.Rows)]


def test_header_documents_the_order_and_the_option():
    block = HEADER[HEADER.index("FIND props FROM tag / edge WHERE"):HEADER.index("int32_t nbg_find_vertices")]
    assert "deterministic, otherwise unspecified" in block and '"find_fast"' in block and "host_waits" in block


def test_null_context_is_refused():
    L = nebula_amd.load()
    out = _lib.Rows()
    for name in NAMES:
        assert getattr(L, name)(None, 1, None, 0, None, None, 0, 0, C.byref(out)) == -1001


def test_abi_unchanged():
    L = nebula_amd.load()
    assert L.nbg_abi_version() == 7
    assert _lib.ABI_VERSION == 7
    assert "#define NBG_ABI_VERSION 7" in HEADER
    assert L.nbg_struct_size(6) == -1


def test_operator_exported():
    assert nebula_amd.FindExecutor
    assert "FindExecutor" in nebula_amd.__all__
    assert callable(nebula_amd.GraphSpace.find_vertices) and callable(nebula_amd.GraphSpace.find_edges)
