"""nbg_set_op at the C-ABI boundary (CPU only: the library loads without a GPU).

The call is an addition to ABI 7, as nbg_order_by was: a function and three constants, no new
caller-allocated struct and no layout change."""
import ctypes as C
import re
from pathlib import Path

from nebula_amd import SetExecutor, _lib

HEADER = (Path(__file__).resolve().parents[1] / "include" / "nebula_amd.h").read_text()


def test_header_declares_the_call_and_its_constants():
    assert re.search(r"int32_t\s+nbg_set_op\s*\(\s*nbg_ctx\s*\*\s*ctx,\s*int32_t\s+op,\s*const\s+nbg_rows\s*\*\s*left,"
                     r"\s*const\s+nbg_rows\s*\*\s*right,\s*int32_t\s+distinct,\s*int32_t\s+keep_on_device,"
                     r"\s*nbg_rows\s*\*\s*out\s*\)\s*;", HEADER)
    consts = dict(re.findall(r"#define\s+(NBG_SET_\w+)\s+(\d+)", HEADER))
    assert consts == {"NBG_SET_UNION": "1", "NBG_SET_INTERSECT": "2", "NBG_SET_MINUS": "3"}
    # the Python constants are the header's
    assert (_lib.SET_UNION, _lib.SET_INTERSECT, _lib.SET_MINUS) == (1, 2, 3)
    assert SetExecutor.OPS == {"UNION": 1, "INTERSECT": 2, "MINUS": 3}


def test_set_op_is_exported_and_bound():
    L = _lib.load()
    assert "nbg_set_op" in _lib.EXPORTS
    assert hasattr(C.CDLL(str(_lib.LIB_PATH)), "nbg_set_op")  # the built library exports it (dlsym)
    f = L.nbg_set_op
    assert f.restype is C.c_int32
    assert len(f.argtypes) == 7
    assert f.argtypes[2] == C.POINTER(_lib.Rows) and f.argtypes[3] == C.POINTER(_lib.Rows)
    assert f.argtypes[6] == C.POINTER(_lib.Rows)
    assert f.argtypes[1] is C.c_int32 and f.argtypes[4] is C.c_int32 and f.argtypes[5] is C.c_int32


def test_null_context_is_invalid_arg():
    L = _lib.load()
    a, b, out = _lib.Rows(), _lib.Rows(), _lib.Rows()
    assert L.nbg_set_op(None, _lib.SET_UNION, C.byref(a), C.byref(b), 0, 0, C.byref(out)) == -1001
    assert L.nbg_set_op(None, 0, None, None, 0, 0, None) == -1001


def test_abi_stays_at_7_without_a_new_struct():
    L = _lib.load()
    assert L.nbg_abi_version() == 7 and _lib.ABI_VERSION == 7
    assert L.nbg_struct_size(6) == -1
    assert L.nbg_struct_size(4) == C.sizeof(_lib.Rows)


def test_executor_takes_names_and_constants():
    assert SetExecutor(None, "union", distinct=True).op == _lib.SET_UNION
    assert SetExecutor(None, "Intersect").op == _lib.SET_INTERSECT
    assert SetExecutor(None, _lib.SET_MINUS).op == _lib.SET_MINUS
    try:
        SetExecutor(None, "EXCEPT")
    except ValueError:
        pass
    else:
        raise AssertionError("an unknown operator name must be refused")
