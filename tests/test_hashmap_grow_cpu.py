"""Table growth of the NrHashMap replica, the part of the C ABI that needs no GPU: the new
config field (default 0 = a fixed table), its ctypes mirror, and the argument checks of
nrg_hashmap_reserve / nrg_hashmap_capacity / nrg_open."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    import nrgpu

    return nrgpu.load()


def test_config_default_is_a_fixed_table(lib):
    from nrgpu import _lib as L

    assert ("hashmap_max_log2_slots", C.c_uint32) in L.Config._fields_
    # the field fills the padding in front of queue_capacity: no other offset and not the size moved
    assert L.Config.hashmap_max_log2_slots.offset == 76 and L.Config.queue_capacity.offset == 80
    assert C.sizeof(L.Config) == 88
    for kind in (L.NRG_DS_HASHMAP, L.NRG_DS_STACK, L.NRG_DS_SYNTHETIC, L.NRG_DS_QUEUE):
        cfg = L.Config()
        cfg.hashmap_max_log2_slots = 77
        lib.nrg_config_default(C.byref(cfg), kind)
        assert cfg.hashmap_max_log2_slots == 0
    assert L.default_config(L.NRG_DS_HASHMAP).log2_slots == 26  # the other defaults did not move


def test_null_context_is_invalid(lib):
    from nrgpu import _lib as L

    n = C.c_uint32(123)
    assert lib.nrg_hashmap_reserve(None, 1000) == L.NRG_E_INVAL
    assert lib.nrg_hashmap_capacity(None, C.byref(n)) == L.NRG_E_INVAL
    assert n.value == 123


@pytest.mark.parametrize("log2_slots,max_log2", [(10, 9), (10, 31), (4, 3)])
def test_open_rejects_a_bad_maximum(lib, log2_slots, max_log2):
    """Below log2_slots, or above what nrg_open accepts for log2_slots (30). The check comes
    before the device is looked up, so it answers NRG_E_INVAL here too; NRG_E_NODEV is tolerated
    as in test_abi.py."""
    from nrgpu import _lib as L

    cfg = L.default_config(L.NRG_DS_HASHMAP)
    cfg.log2_slots, cfg.hashmap_max_log2_slots = log2_slots, max_log2
    out = C.c_void_p()
    rc = lib.nrg_open(0, C.byref(cfg), C.byref(out))
    assert rc in (L.NRG_E_INVAL, L.NRG_E_NODEV)
    assert not out.value
