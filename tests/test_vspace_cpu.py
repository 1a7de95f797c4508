"""The replicated page table's C ABI and Python mirror, without a GPU (benches/vspace.rs:483-526
OpcodeWr::Map / MapDevice, OpcodeRd::Identify): the header declares the new symbols and
libnrgpu.so exports them, nrg_config_default gives the documented defaults through an unchanged
Config, VSpace.encode / decode round-trip, the entry points refuse a NULL context, and the
sequential model (tests/vspace_model.py) gives the answers worked out by hand below."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from vspace_model import ADDR, MB2, P, PS, RW, US, XD, VSpaceModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nrgpu.h")
VSPACE_SYMBOLS = ("nrg_vspace_round_async", "nrg_vspace_resolve", "nrg_vspace_resolve_async", "nrg_vspace_tables",
                  "nrg_vspace_dump")
KB4 = 4096


@pytest.fixture(scope="module")
def L():
    from nrgpu import _lib

    _lib.load()
    return _lib


def test_header_declares_and_library_exports_the_vspace(L):
    with open(HEADER) as f:
        h = f.read()
    assert re.search(r"#define\s+NRG_DS_VSPACE\s+5u", h)
    assert re.search(r"#define\s+NRG_VSPACE_MAP\s+0u", h) and re.search(r"#define\s+NRG_VSPACE_MAP_DEVICE\s+1u", h)
    assert re.search(r"typedef struct \{\s*uint64_t vbase;\s*uint64_t pbase;\s*uint64_t len;\s*uint32_t op;\s*"
                     r"uint32_t rights;\s*\} nrg_vspace_op;", h)
    assert re.search(r"typedef struct \{\s*uint64_t a;\s*uint64_t b;\s*\} nrg_vspace_resp;", h)
    # nrg_config is unchanged: queue_capacity is still its last field
    body = re.search(r"typedef struct \{((?:(?!typedef).)*?)\} nrg_config;", h, re.S).group(1)
    fields = re.findall(r"^\s*uint(?:32|64)_t\s+([^;]+);", body, re.M)
    assert fields[-1].strip() == "queue_capacity"
    lib = L.load()
    for name in VSPACE_SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(" % name, h, re.M), name
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
    assert (L.NRG_DS_VSPACE, L.NRG_VSPACE_MAP, L.NRG_VSPACE_MAP_DEVICE) == (5, 0, 1)


def test_config_defaults_and_layout(L):
    lib = L.load()
    assert L.Config._fields_[-1][0] == "queue_capacity"
    assert L.Config.queue_capacity.offset == 80 and C.sizeof(L.Config) == 88

    class Guarded(C.Structure):
        _fields_ = [("cfg", L.Config), ("guard", C.c_uint64 * 2)]

    g = Guarded()
    C.memset(C.byref(g), 0xA5, C.sizeof(g))
    lib.nrg_config_default(C.byref(g.cfg), L.NRG_DS_VSPACE)
    assert list(g.guard) == [0xA5A5A5A5A5A5A5A5] * 2
    cfg = g.cfg
    assert cfg.ds_kind == L.NRG_DS_VSPACE
    assert cfg.log2_slots == 18           # the pool: 2^18 tables of 4 KiB
    assert cfg.max_batch == 1 << 16
    assert cfg.pipeline == 0 and cfg.replica_id == 1
    # the earlier kinds' defaults are what they were
    old = L.default_config(L.NRG_DS_HASHMAP)
    assert (old.log2_slots, old.max_batch) == (26, 1 << 20)
    assert L.default_config(L.NRG_DS_QUEUE).max_batch == 1 << 20


def test_dtypes_and_encode_decode_round_trip():
    import nrgpu
    from nrgpu import Identify, Map, MapDevice, VSpace

    assert nrgpu.VSPACE_OP_DTYPE.itemsize == 32 and nrgpu.VSPACE_RESP_DTYPE.itemsize == 16
    assert nrgpu._lib.VSPACE_OP_DTYPE is nrgpu.VSPACE_OP_DTYPE
    assert VSpace.kind == 5 and VSpace.rec_dtype == nrgpu.VSPACE_OP_DTYPE
    ops = [Map(0x1000, 0x4000, 3, 0x20_0000), MapDevice(0x7FFF_FFFF_F000, 0x8000_0000, 0x1000),
           Map((1 << 48) - 4096, 0, 8, (1 << 48) - 4096)]
    r = VSpace.encode(ops)
    assert r.dtype == nrgpu.VSPACE_OP_DTYPE and len(r) == 3
    assert r["op"].tolist() == [0, 1, 0] and r["rights"].tolist() == [3, 0, 8]
    back = [Map(int(x["vbase"]), int(x["len"]), int(x["rights"]), int(x["pbase"])) if x["op"] == 0
            else MapDevice(int(x["vbase"]), int(x["pbase"]), int(x["len"])) for x in r]
    assert back == ops
    # the wire layout: vbase, pbase, len (u64 each), op, rights (u32 each), little-endian
    assert r[0].tobytes() == b"".join(v.to_bytes(8, "little") for v in (0x1000, 0x20_0000, 0x4000)) + \
        (0).to_bytes(4, "little") + (3).to_bytes(4, "little")
    resp = np.zeros(3, nrgpu.VSPACE_RESP_DTYPE)
    resp["a"], resp["b"] = [0x20_0000, 0, 0x5000], [0x4000, 0, 0]
    assert VSpace.decode(resp, np.array([1, 1, 0], np.uint8)) == [("ok", 0x20_0000, 0x4000), ("ok", 0, 0),
                                                                   ("err", 0x5000)]
    assert Identify(5) == Identify(5)


def test_null_context_is_an_error_not_a_crash(L):
    lib = L.load()
    n = C.c_uint64()
    buf = (C.c_uint64 * 8)()
    assert lib.nrg_vspace_tables(None, C.byref(n)) == L.NRG_E_INVAL
    assert lib.nrg_vspace_dump(None, buf, 4, C.byref(n)) == L.NRG_E_INVAL
    assert lib.nrg_vspace_resolve(None, buf, 4, buf, buf) == L.NRG_E_INVAL
    assert lib.nrg_vspace_resolve_async(None, None, 0, None, None) == L.NRG_E_INVAL
    assert lib.nrg_vspace_round_async(None, None, 0, 1, None, None) == L.NRG_E_INVAL
    # a vspace config is a known kind: without a device the open fails on the device, not the kind
    out = C.c_void_p()
    cfg = L.default_config(L.NRG_DS_VSPACE)
    assert lib.nrg_open(1 << 20, C.byref(cfg), C.byref(out)) == L.NRG_E_NODEV


# ---- the model's own known answers, worked by hand -------------------------------------------
V0 = (3 << 39) | (5 << 30) | (7 << 21)  # PML4 slot 3, PDPT slot 5, PD slot 7, 2 MiB-aligned


def test_model_four_pages_then_zero_length():
    m = VSpaceModel()
    # PML4 + PDPT + PD + PT
    assert m.dispatch_mut(V0 + 3 * KB4, 0x10_0000, 4 * KB4, 0, 3) == (1, 0x10_0000, 4 * KB4)
    assert m.tables() == 4
    va, en = m.dump()
    assert va.tolist() == [V0 + (3 + i) * KB4 for i in range(4)]
    assert en.tolist() == [(0x10_0000 + i * KB4) | P | RW | XD for i in range(4)]
    assert m.resolve(V0 + 4 * KB4 + 0x123) == (0x10_1123, 1)
    assert m.resolve(V0 + 2 * KB4) == (0, 0) and m.resolve(V0 + 7 * KB4) == (0, 0)
    assert m.resolve((0xFFFF << 48) | (V0 + 3 * KB4)) == (0x10_0000, 1)  # bits 48..63 are ignored
    # len = 0 in the next granule still creates the path down to a PT
    assert m.dispatch_mut(V0 + MB2, 0, 0, 1, 0) == (1, 0, 0)
    assert m.tables() == 5
    assert len(m.dump()[0]) == 4


def test_model_large_pages_then_small_ones():
    m = VSpaceModel()
    length = 3 * MB2 + 5 * KB4
    assert m.dispatch_mut(V0, 0x4000_0000, length, 0, 7) == (1, 0x4000_0000, length)
    assert m.tables() == 4  # PML4, PDPT, PD and the one new PT of the tail
    va, en = m.dump()
    assert va.tolist() == [V0 + i * MB2 for i in range(3)] + [V0 + 3 * MB2 + i * KB4 for i in range(5)]
    assert en[:3].tolist() == [(0x4000_0000 + i * MB2) | P | PS | RW for i in range(3)]
    assert en[3:].tolist() == [(0x4000_0000 + 3 * MB2 + i * KB4) | P | RW for i in range(5)]
    assert m.resolve(V0 + MB2 + 0x12345) == (0x4000_0000 + MB2 + 0x12345, 1)


def test_model_remap_and_run_meeting_a_pt():
    m = VSpaceModel()
    assert m.dispatch_mut(V0, 0x1000, KB4, 0, 1)[0] == 1
    assert m.dispatch_mut(V0, 0x9000, KB4, 0, 1) == (0, V0, 0)  # a remap: Err(at = vbase)
    assert m.resolve(V0) == (0x1000, 1)
    # a run of large pages from two granules below meets the PT of V0: the two large pages stay,
    # `at` is the start of the run
    start = V0 - 2 * MB2
    assert m.dispatch_mut(start, 0x8000_0000, 4 * MB2, 1, 0) == (0, start, 0)
    va, en = m.dump()
    assert va.tolist() == [start, start + MB2, V0]
    assert en[:2].tolist() == [0x8000_0000 | P | PS | RW | XD, (0x8000_0000 + MB2) | P | PS | RW | XD]
    assert m.tables() == 4
    # every right's flags (to_pt_rights): kernel rights carry US, as the reference has it
    want = {1: XD, 2: US | XD, 3: RW | XD, 4: RW | US | XD, 5: 0, 6: US, 7: RW, 8: RW | US}
    for r, fl in want.items():
        assert m.dispatch_mut(V0 + (10 + r) * KB4, r * KB4, KB4, 0, r)[0] == 1
        e = int(m.dump()[1][list(m.dump()[0]).index(V0 + (10 + r) * KB4)])
        assert e == (r * KB4) | P | fl and e & ADDR == r * KB4
