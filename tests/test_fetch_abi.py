"""nbg_fetch_vertices / nbg_fetch_edges at the C boundary: the symbols are declared, exported and
bound with the header's signatures, and adding them changed no struct (ABI 7 stays)."""
import ctypes as C
import re
from pathlib import Path

import nebula_amd
from nebula_amd import _lib

HEADER = (Path(__file__).resolve().parents[1] / "include" / "nebula_amd.h").read_text()


def decl(name):
    m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", HEADER)
    assert m, f"{name} is not declared in include/nebula_amd.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbols_exported():
    L = nebula_amd.load()
    for name in ("nbg_fetch_vertices", "nbg_fetch_edges"):
        assert name in _lib.EXPORTS
        assert hasattr(L, name)
        assert getattr(L, name).restype is C.c_int32


def test_signatures_match_header():
    L = nebula_amd.load()
    vp, i32, sz = C.c_void_p, C.c_int32, C.c_size_t
    assert decl("nbg_fetch_vertices") == [
        "nbg_ctx* ctx", "int32_t tag_id", "const int64_t* vids", "size_t n", "int32_t keys_on_device",
        "const uint8_t* const* yields", "const size_t* yield_lens", "size_t n_yields", "int32_t distinct",
        "int32_t keep_on_device", "nbg_rows* out"]
    assert list(L.nbg_fetch_vertices.argtypes) == [
        vp, i32, vp, sz, i32, C.POINTER(vp), C.POINTER(sz), sz, i32, i32, C.POINTER(_lib.Rows)]
    assert decl("nbg_fetch_edges") == [
        "nbg_ctx* ctx", "int32_t edge_type", "const int64_t* src", "const int64_t* dst", "const int64_t* rank",
        "size_t n", "int32_t keys_on_device", "const uint8_t* const* yields", "const size_t* yield_lens",
        "size_t n_yields", "int32_t distinct", "int32_t keep_on_device", "nbg_rows* out"]
    assert list(L.nbg_fetch_edges.argtypes) == [
        vp, i32, vp, vp, vp, sz, i32, C.POINTER(vp), C.POINTER(sz), sz, i32, i32, C.POINTER(_lib.Rows)]


def test_null_context_is_refused():
    L = nebula_amd.load()
    out = _lib.Rows()
    assert L.nbg_fetch_vertices(None, 1, None, 0, 0, None, None, 0, 0, 0, C.byref(out)) == -1001
    assert L.nbg_fetch_edges(None, 1, None, None, None, 0, 0, None, None, 0, 0, 0, C.byref(out)) == -1001


def test_abi_unchanged():
    L = nebula_amd.load()
    assert L.nbg_abi_version() == 7
    assert _lib.ABI_VERSION == 7
    assert "#define NBG_ABI_VERSION 7" in HEADER
    assert L.nbg_struct_size(6) == -1


def test_operators_exported():
    assert nebula_amd.FetchVerticesExecutor and nebula_amd.FetchEdgesExecutor
    assert "FetchVerticesExecutor" in nebula_amd.__all__ and "FetchEdgesExecutor" in nebula_amd.__all__
