"""nbg_group_by at the C-ABI boundary (CPU only: the library loads without a GPU).

The call is an addition to ABI 7, as nbg_order_by and nbg_set_op were: a function and five
constants, no new caller-allocated struct and no layout change."""
import ctypes as C
import re
from pathlib import Path

import pytest

from nebula_amd import GroupByExecutor, _lib
from nebula_amd.engine import AGG_FUNCTIONS

HEADER = (Path(__file__).resolve().parents[1] / "include" / "nebula_amd.h").read_text()


def test_header_declares_the_call_and_its_constants():
    assert re.search(r"int32_t\s+nbg_group_by\s*\(\s*nbg_ctx\s*\*\s*ctx,\s*const\s+nbg_rows\s*\*\s*in,"
                     r"\s*const\s+int32_t\s*\*\s*key_cols,\s*size_t\s+n_keys,\s*const\s+int32_t\s*\*\s*agg_fns,"
                     r"\s*const\s+int32_t\s*\*\s*agg_cols,\s*size_t\s+n_aggs,\s*int32_t\s+keep_on_device,"
                     r"\s*nbg_rows\s*\*\s*out\s*\)\s*;", HEADER)
    consts = dict(re.findall(r"#define\s+(NBG_AGG_\w+)\s+(\d+)", HEADER))
    assert consts == {"NBG_AGG_SUM": "1", "NBG_AGG_COUNT": "2", "NBG_AGG_AVG": "3", "NBG_AGG_MIN": "4",
                      "NBG_AGG_MAX": "5"}
    # the Python constants are the header's
    assert (_lib.AGG_SUM, _lib.AGG_COUNT, _lib.AGG_AVG, _lib.AGG_MIN, _lib.AGG_MAX) == (1, 2, 3, 4, 5)
    assert AGG_FUNCTIONS == {"SUM": 1, "COUNT": 2, "AVG": 3, "MIN": 4, "MAX": 5}


def test_group_by_is_exported_and_bound():
    L = _lib.load()
    assert "nbg_group_by" in _lib.EXPORTS
    assert hasattr(C.CDLL(str(_lib.LIB_PATH)), "nbg_group_by")  # the built library exports it (dlsym)
    f = L.nbg_group_by
    assert f.restype is C.c_int32
    assert len(f.argtypes) == 9
    assert f.argtypes[1] == C.POINTER(_lib.Rows) and f.argtypes[8] == C.POINTER(_lib.Rows)
    assert f.argtypes[3] is C.c_size_t and f.argtypes[6] is C.c_size_t and f.argtypes[7] is C.c_int32


def test_null_context_is_invalid_arg():
    L = _lib.load()
    a, out = _lib.Rows(), _lib.Rows()
    assert L.nbg_group_by(None, C.byref(a), None, 0, None, None, 0, 0, C.byref(out)) == -1001
    assert L.nbg_group_by(None, None, None, 0, None, None, 0, 0, None) == -1001


def test_abi_stays_at_7_without_a_new_struct():
    L = _lib.load()
    assert L.nbg_abi_version() == 7 and _lib.ABI_VERSION == 7
    assert L.nbg_struct_size(6) == -1
    assert L.nbg_struct_size(4) == C.sizeof(_lib.Rows)


def test_executor_resolves_names_and_function_spellings():
    ex = GroupByExecutor(None, ["$-.team", "age"], [("count", "*"), ("Sum", "$-.age"), ("AVG", "age"),
                                                    ("min", "$-.team"), (_lib.AGG_MAX, "age"), ("COUNT", None)],
                         ["team", "age"])
    assert ex.key_cols == [0, 1]
    assert ex.aggs == [(_lib.AGG_COUNT, None), (_lib.AGG_SUM, 1), (_lib.AGG_AVG, 1), (_lib.AGG_MIN, 0),
                       (_lib.AGG_MAX, 1), (_lib.AGG_COUNT, None)]
    # a repeated key stays (it is output again), and no key at all is legal
    assert GroupByExecutor(None, ["age", "$-.age"], [], ["team", "age"]).key_cols == [1, 1]
    assert GroupByExecutor(None, [], [("COUNT", None)], ["team"]).key_cols == []


@pytest.mark.parametrize("keys, aggs", [
    (["$-.nope"], [("COUNT", None)]),   # an unknown key is not dropped the way ORDER BY drops a factor
    (["team"], [("SUM", "$-.nope")]),   # an unknown aggregate column
    (["team"], [("MEDIAN", "age")]),    # an unknown function name
    (["team"], [(6, "age")]),           # an unknown function constant
    (["team"], [("SUM", None)]),        # only COUNT goes without a column
])
def test_executor_refuses_unknown_names_and_functions(keys, aggs):
    with pytest.raises(ValueError):
        GroupByExecutor(None, keys, aggs, ["team", "age"])
