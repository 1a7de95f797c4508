"""nrg_open / nrg_close per data structure: the smallest configuration each kind accepts opens,
answers one 16-op round bit-exactly against the oracle, closes, and opens and closes again; every
configuration nrg_open rejects for a kind is answered with NRG_E_INVAL.

The smallest configurations: a 16-slot table, 64-op chunks, a log of the minimum size, a stack
and a queue of 64 elements, and 8 synthetic words with the default touch counts (20 / 5 cold,
2 / 1 hot: more words than hot ones). Nothing here allocates more than a few MiB.
"""
import ctypes as C
from collections import deque

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MIN_LOG_BYTES = 2 * 32 * 256 * 64  # Log::new's floor: 2 * GC_FROM_HEAD entries of 64 bytes
SMALL = dict(log_bytes=MIN_LOG_BYTES, max_batch=64)
HM_MAX_BATCH = 1 << 23  # common.hpp
N = 16


def _small(nrg, kind):
    L = nrg._lib
    return {L.NRG_DS_HASHMAP: dict(SMALL, log2_slots=4),
            L.NRG_DS_STACK: dict(SMALL, stack_capacity=64),
            L.NRG_DS_QUEUE: dict(SMALL, queue_capacity=64),
            L.NRG_DS_SYNTHETIC: dict(SMALL, synth_n=8)}[kind]


def _hashmap_round(nrg, orc, dev):
    om = orc.HashMap()
    keys = orc.gen_uniform(N, 5, 6)  # at most 6 keys in the 16 slots
    vals = orc.gen_raw(N, 6)
    recs = np.zeros(N, nrg.PUT_DTYPE)
    recs["key"], recs["val"] = keys, vals
    first = dev.log_append(recs, 1)
    prev, pf = dev.log_exec(first, first + N)
    oprev, opf = om.replay(keys, vals)
    np.testing.assert_array_equal(pf, opf)
    np.testing.assert_array_equal(prev, oprev)
    gk = np.arange(8, dtype=np.uint64)
    gv, gf = dev.hm_get(gk)
    ov, of = om.get_batch(gk)
    np.testing.assert_array_equal(gf, of)
    np.testing.assert_array_equal(gv, ov)
    assert dev.hm_digest() == om.digest()


def _stack_round(nrg, orc, dev):
    init = np.arange(3, dtype=np.uint32) + 100
    dev.st_init(init)
    os_ = orc.Stack(init)
    vals = (orc.gen_raw(N, 7) & 0xFFFFFFFF).astype(np.uint32)
    ops = np.array([0, 0, 1, 0, 0, 0, 1, 1, 1, 0, 1, 0, 1, 1, 0, 1], np.uint32)  # Pops past empty too
    recs = np.zeros(N, nrg.STACK_OP_DTYPE)
    recs["val"], recs["op"] = vals, ops
    first = dev.log_append(recs, 1)
    resp, some = dev.log_exec(first, first + N)
    oresp, osome = os_.replay(vals, ops)
    np.testing.assert_array_equal(some, osome)
    np.testing.assert_array_equal(resp, oresp)
    np.testing.assert_array_equal(dev.st_dump(), os_.dump())
    assert dev.st_peek() == os_.peek()


def _queue_round(nrg, orc, dev):
    q = deque([1000, 1001, 1002])
    dev.qu_init(np.array(q, np.uint64))
    vals = orc.gen_raw(N, 8)
    ops = np.array([0, 0, 1, 0, 0, 0, 1, 1, 1, 0, 1, 0, 1, 1, 0, 1], np.uint64)
    recs = np.zeros(N, nrg.QUEUE_OP_DTYPE)
    recs["val"], recs["op"] = vals, ops
    first = dev.log_append(recs, 1)
    resp, some = dev.log_exec(first, first + N)
    oresp, osome = np.zeros(N, np.uint64), np.zeros(N, np.uint8)
    for i, (v, o) in enumerate(zip(vals.tolist(), ops.tolist())):  # the sequential VecDeque<u64>
        if o == 1:
            q.append(v)
            oresp[i], osome[i] = v, 1
        elif q:
            oresp[i], osome[i] = q.popleft(), 1
    np.testing.assert_array_equal(some, osome)
    np.testing.assert_array_equal(resp, oresp)
    np.testing.assert_array_equal(dev.qu_dump(), np.array(q, np.uint64))
    assert dev.qu_len() == len(q)


def _synth_round(nrg, orc, dev):
    os_ = orc.Synthetic(n=8)
    raw = orc.gen_raw(4 * N, 9)
    ops = np.zeros(N, nrg.SYNTH_OP_DTYPE)
    ops["tid"], ops["r1"], ops["r2"] = raw[0::4] % 4, raw[1::4], raw[2::4]
    ops["op"] = (raw[3::4] % 4 != 0).astype(np.uint64)  # mostly ReadWrite, some WriteOnly
    first = dev.log_append(ops, 1)
    resp, some = dev.log_exec(first, first + N)
    oresp = os_.replay(np.stack([ops["tid"], ops["r1"], ops["r2"], ops["op"]], axis=1))
    np.testing.assert_array_equal(resp, oresp)
    assert np.all(some == 1)
    rd = np.zeros(N, nrg.SYNTH_RD_DTYPE)
    rd["tid"], rd["r1"], rd["r2"] = raw[0::4] % 4, raw[2::4], raw[1::4]
    np.testing.assert_array_equal(dev.sy_read(rd), os_.read(np.stack([rd["tid"], rd["r1"], rd["r2"]], axis=1)))
    np.testing.assert_array_equal(dev.sy_dump(), os_.dump())


ROUNDS = {"HASHMAP": _hashmap_round, "STACK": _stack_round, "QUEUE": _queue_round, "SYNTHETIC": _synth_round}


@pytest.mark.parametrize("name", list(ROUNDS))
def test_smallest_config_opens_answers_and_closes(nrg, orc, name):
    """Open, one round against the oracle, close; then the same again: the second context gets
    fresh buffers after the first one's were freed (each structure's own, and the shared ones)."""
    kind = getattr(nrg._lib, "NRG_DS_" + name)
    for _ in range(2):
        dev = nrg.DeviceReplica(kind, 0, **_small(nrg, kind))
        st = dev.log_state()
        assert st["size"] == MIN_LOG_BYTES // 64 and st["ds_kind"] == kind
        ROUNDS[name](nrg, orc, dev)
        dev.sync()
        assert dev._lib.nrg_close(dev._h) == nrg._lib.NRG_OK
        dev._h = None


REJECTED = [
    ("HASHMAP", dict(log2_slots=3)),
    ("HASHMAP", dict(log2_slots=31)),
    ("HASHMAP", dict(max_batch=HM_MAX_BATCH + 1)),
    ("STACK", dict(stack_capacity=0)),
    ("STACK", dict(stack_capacity=1 << 31)),
    ("STACK", dict(max_batch=(1 << 24) + 1)),
    ("QUEUE", dict(queue_capacity=0)),
    ("QUEUE", dict(queue_capacity=(1 << 32) + 1)),
    ("QUEUE", dict(max_batch=(1 << 24) + 1)),
    ("SYNTHETIC", dict(synth_n=0)),
    ("SYNTHETIC", dict(synth_hot_reads=0)),
    ("SYNTHETIC", dict(synth_n=2)),  # synth_n == synth_hot_reads
    ("SYNTHETIC", dict(synth_n=1)),  # synth_n < synth_hot_reads
    ("SYNTHETIC", dict(synth_hot_writes=0, synth_cold_writes=0)),
    ("SYNTHETIC", dict(synth_hot_writes=1, synth_cold_writes=64)),
]


@pytest.mark.parametrize("name,bad", REJECTED, ids=lambda v: v if isinstance(v, str) else
                         ",".join(f"{k}={x}" for k, x in v.items()))
def test_rejected_config_is_invalid(nrg, name, bad):
    """The smallest valid configuration with one field out of range: NRG_E_INVAL and no context;
    the unchanged configuration still opens afterwards."""
    L = nrg._lib
    kind = getattr(L, "NRG_DS_" + name)
    cfg = L.default_config(kind)
    for k, v in dict(_small(nrg, kind), **bad).items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    assert L.load().nrg_open(0, C.byref(cfg), C.byref(h)) == L.NRG_E_INVAL
    assert not h.value
    nrg.DeviceReplica(kind, 0, **_small(nrg, kind)).close()
