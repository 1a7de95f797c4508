"""The replicated FIFO queue's C ABI and Python mirror, without a GPU (benches/lockfree.rs:43-52
QueueWr::Push / Pop and QueueRd::Len; benches/lockfree_comparisons.rs:75-101 SegQueueWrapper):
the header declares the new symbols and libnrgpu.so exports them, nrg_config_default gives the
documented defaults through a Config whose layout matches the C struct, Queue.encode / decode
round-trip, and the entry points refuse a NULL context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nrgpu.h")
QUEUE_SYMBOLS = ("nrg_queue_init", "nrg_queue_init_range", "nrg_queue_len", "nrg_queue_dump",
                 "nrg_queue_round_async")


@pytest.fixture(scope="module")
def L():
    from nrgpu import _lib

    _lib.load()
    return _lib


def test_header_declares_and_library_exports_the_queue(L):
    with open(HEADER) as f:
        h = f.read()
    assert re.search(r"#define\s+NRG_DS_QUEUE\s+4u", h)
    assert re.search(r"#define\s+NRG_QUEUE_POP\s+0u", h) and re.search(r"#define\s+NRG_QUEUE_PUSH\s+1u", h)
    assert re.search(r"typedef struct \{\s*uint64_t val;\s*uint64_t op;\s*\} nrg_queue_op;", h)
    # the new config field is the struct's last one, so every earlier offset stays
    body = re.search(r"typedef struct \{((?:(?!typedef).)*?)\} nrg_config;", h, re.S).group(1)
    fields = re.findall(r"^\s*uint(?:32|64)_t\s+([^;]+);", body, re.M)
    assert fields[-1].strip() == "queue_capacity"
    lib = L.load()
    for name in QUEUE_SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(" % name, h, re.M), name
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
    assert (L.NRG_DS_QUEUE, L.NRG_QUEUE_POP, L.NRG_QUEUE_PUSH) == (4, 0, 1)


def test_config_defaults_and_layout(L):
    lib = L.load()
    # nrg_config: 2 u32, 5 u64, 7 u32 (padded to 8), then queue_capacity as the last u64
    assert L.Config._fields_[-1][0] == "queue_capacity"
    assert L.Config.queue_capacity.offset == 80 and C.sizeof(L.Config) == 88
    # the library writes the whole struct (memset + fields): guard words behind it stay intact and
    # the last field round-trips, so the two sides agree on the struct's size
    class Guarded(C.Structure):
        _fields_ = [("cfg", L.Config), ("guard", C.c_uint64 * 2)]

    g = Guarded()
    C.memset(C.byref(g), 0xA5, C.sizeof(g))
    lib.nrg_config_default(C.byref(g.cfg), L.NRG_DS_QUEUE)
    assert list(g.guard) == [0xA5A5A5A5A5A5A5A5] * 2
    cfg = g.cfg
    assert cfg.ds_kind == L.NRG_DS_QUEUE
    assert cfg.queue_capacity == 1 << 24       # holds the 2M-element prefill of 1M-op rounds
    assert cfg.max_batch == 1 << 20 and cfg.max_batch <= 1 << 24
    assert cfg.pipeline == 0 and cfg.replica_id == 1
    # the earlier kinds' defaults are what they were
    old = L.default_config(L.NRG_DS_STACK)
    assert (old.stack_capacity, old.max_batch, old.stack_push_resp) == (1 << 24, 1 << 20, 0)


def test_queue_encode_decode_round_trip():
    import nrgpu
    from nrgpu import Pop, Push, Queue

    assert nrgpu.QUEUE_OP_DTYPE.itemsize == 16
    assert Queue.kind == 4 and Queue.rec_dtype == nrgpu.QUEUE_OP_DTYPE
    ops = [Push(7), Pop(), Push(2**64 - 1), Push(0), Pop(), Pop()]
    r = Queue.encode(ops)
    assert r.dtype == nrgpu.QUEUE_OP_DTYPE and len(r) == 6
    assert r["op"].tolist() == [1, 0, 1, 1, 0, 0]
    assert r["val"].tolist() == [7, 0, 2**64 - 1, 0, 0, 0]
    back = [Push(int(v)) if o == 1 else Pop() for v, o in zip(r["val"], r["op"])]
    assert back == ops
    # the wire layout: val then op, little-endian u64 each
    assert r[2].tobytes() == (2**64 - 1).to_bytes(8, "little") + (1).to_bytes(8, "little")
    resp = np.array([7, 0, 2**64 - 1, 0, 5, 0], np.uint64)
    some = np.array([1, 1, 1, 1, 1, 0], np.uint8)
    assert Queue.decode(resp, some) == [7, 0, 2**64 - 1, 0, 5, None]
    assert nrgpu.Len() == nrgpu.Len()


def test_null_context_is_an_error_not_a_crash(L):
    lib = L.load()
    n = C.c_uint64()
    buf = (C.c_uint64 * 4)()
    assert lib.nrg_queue_len(None, C.byref(n)) == L.NRG_E_INVAL
    assert lib.nrg_queue_init(None, buf, 4) == L.NRG_E_INVAL
    assert lib.nrg_queue_init_range(None, 4) == L.NRG_E_INVAL
    assert lib.nrg_queue_dump(None, buf, 4, C.byref(n)) == L.NRG_E_INVAL
    assert lib.nrg_queue_round_async(None, None, 0, 1, None, None) == L.NRG_E_INVAL
    # a queue config is a known kind: without a device the open fails on the device, not the kind
    out = C.c_void_p()
    cfg = L.default_config(L.NRG_DS_QUEUE)
    rc = lib.nrg_open(1 << 20, C.byref(cfg), C.byref(out))
    assert rc == L.NRG_E_NODEV
