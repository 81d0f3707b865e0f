"""nbg_order_by at the C-ABI boundary, and OrderByExecutor's name resolution (CPU only: the
library loads without a GPU, and resolving `$-.name` against the YIELD aliases is pure Python).

The call is an addition to ABI 7: no struct changed and no struct index was added, which is why the
factors travel as two parallel int32 arrays."""
import ctypes as C

from nebula_amd import OrderByExecutor, _lib


def test_order_by_is_exported_and_bound():
    L = _lib.load()
    assert "nbg_order_by" in _lib.EXPORTS
    f = L.nbg_order_by
    assert f.restype is C.c_int32
    assert len(f.argtypes) == 7
    assert f.argtypes[1] == C.POINTER(_lib.Rows) and f.argtypes[6] == C.POINTER(_lib.Rows)
    assert f.argtypes[4] is C.c_size_t and f.argtypes[5] is C.c_int32


def test_null_context_is_invalid_arg():
    L = _lib.load()
    rows, out = _lib.Rows(), _lib.Rows()
    assert L.nbg_order_by(None, C.byref(rows), None, None, 0, 0, C.byref(out)) == -1001
    assert L.nbg_order_by(None, None, None, None, 0, 0, None) == -1001


def test_abi_stays_at_7_without_a_new_struct():
    L = _lib.load()
    assert L.nbg_abi_version() == 7 and _lib.ABI_VERSION == 7
    assert L.nbg_struct_size(6) == -1
    assert L.nbg_struct_size(4) == C.sizeof(_lib.Rows)
    assert _lib.GoSpec._fields_[-1][0] == "upto"


def test_executor_drops_unknown_names():
    # OrderByExecutor.cpp:91-101: a field the input schema lacks is skipped
    ex = OrderByExecutor(None, [("$-.abc", 0)], ["name", "start", "team"])
    assert ex.sort_factors == []
    ex = OrderByExecutor(None, [("$-.abc", 1), ("$-.team", 0), ("$-.nope", 0), ("$-.start", 1)],
                         ["name", "start", "team"])
    assert ex.sort_factors == [(2, 0), (1, 1)]


def test_executor_keeps_duplicates_in_order():
    ex = OrderByExecutor(None, [("$-.team", 0), ("$-.age", 1), ("$-.team", 1)], ["team", "player", "age"])
    assert ex.sort_factors == [(0, 0), (2, 1), (0, 1)]


def test_executor_maps_directions_and_bare_names():
    cols = ["team", "player", "age", "start"]
    ex = OrderByExecutor(None, [("team", "DESC"), ("$-.age", "asc"), ("start", True), ("player", False)], cols)
    assert ex.sort_factors == [(0, 1), (2, 0), (3, 1), (1, 0)]
