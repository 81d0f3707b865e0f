"""ABI 7: nbg_go_spec gained `upto` as its last field (GO UPTO N STEPS).  CPU only: the library
loads without a GPU, and the ctypes mirror must match the struct the library was built with."""
import ctypes as C

from nebula_amd import _lib


def test_abi_version_is_7():
    L = _lib.load()
    assert L.nbg_abi_version() == 7
    assert _lib.ABI_VERSION == 7


def test_go_spec_size_matches_library():
    L = _lib.load()
    assert L.nbg_struct_size(3) == C.sizeof(_lib.GoSpec)


def test_upto_is_last_field_and_defaults_to_zero():
    spec = _lib.GoSpec()
    assert spec.upto == 0
    name, ctype = _lib.GoSpec._fields_[-1]
    assert name == "upto" and ctype is C.c_int32
    # last in memory too: nothing but tail padding behind it
    assert _lib.GoSpec.upto.offset == max(getattr(_lib.GoSpec, n).offset for n, _ in _lib.GoSpec._fields_)
    # a positionally built spec (the pre-ABI-7 argument list) leaves it zero
    assert _lib.GoSpec(1, 3, None, 0, None, 0, None, None, 0, 1, 0).upto == 0
