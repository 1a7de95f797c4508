"""The capacity calls at the C-ABI boundary, without a GPU: nrg_stack / nrg_queue / nrg_vspace
_reserve and _capacity and nrg_set_max_capacity are exported with C linkage, answer NRG_E_INVAL for
a NULL context before they touch a device, and have their DeviceReplica wrappers."""
import ctypes as C

import pytest

SYMBOLS = ["nrg_stack_reserve", "nrg_stack_capacity", "nrg_queue_reserve", "nrg_queue_capacity",
           "nrg_vspace_reserve", "nrg_vspace_capacity", "nrg_set_max_capacity"]
WRAPPERS = ["st_reserve", "st_capacity", "qu_reserve", "qu_capacity", "vs_reserve", "vs_capacity",
            "set_max_capacity"]


@pytest.fixture(scope="module")
def lib():
    import nrgpu

    return nrgpu.load()


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_exported_and_bound(lib, name):
    from nrgpu import _lib as L

    assert hasattr(lib, name)
    assert name in L.SIGNATURES
    res, args = L.SIGNATURES[name]
    assert res is C.c_int and args[0] is C.c_void_p and len(args) == 2


@pytest.mark.parametrize("name", SYMBOLS)
def test_null_context_is_invalid(lib, name):
    from nrgpu import _lib as L

    if name.endswith("_capacity") and name != "nrg_set_max_capacity":
        n = C.c_uint64(0x5555)
        assert getattr(lib, name)(None, C.byref(n)) == L.NRG_E_INVAL
        assert n.value == 0x5555  # nothing written
    else:
        assert getattr(lib, name)(None, 100) == L.NRG_E_INVAL
        assert getattr(lib, name)(None, 0) == L.NRG_E_INVAL


def test_python_wrappers_exist():
    import nrgpu

    for w in WRAPPERS:
        assert callable(getattr(nrgpu.DeviceReplica, w)), w
