"""Growth on demand of the stack, the queue and the page-table pool: nrg_*_reserve / nrg_*_capacity,
automatic growth under replay (nrg_set_max_capacity) through every round path, under a combiner and
in a group, and a restore that grows first.

Expectations: the stack from the sequential Vec oracle (as test_gpu_stack.py), the queue from a
collections.deque, the page table from tests/vspace_model.py, digests from nrgpu.digest.
"""
import ctypes as C
import threading
from collections import deque

import numpy as np
import pytest

from nrgpu import digest
from vspace_model import KB4, VSpaceModel

pytestmark = pytest.mark.gpu

LOG_BYTES = 1 << 22  # 65536 log entries


def _st_ops(nrg, vals, ops):
    r = np.zeros(len(ops), nrg.STACK_OP_DTYPE)
    r["val"], r["op"] = vals, ops
    return r


def _qu_ops(nrg, vals, ops):
    r = np.zeros(len(ops), nrg.QUEUE_OP_DTYPE)
    r["val"], r["op"] = vals, ops
    return r


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


class _QueueModel:
    """Push answers Some(v); Pop the front, or None on an empty queue."""

    def __init__(self, vals=()):
        self.q = deque(int(v) for v in vals)

    def replay(self, recs):
        resp = np.zeros(len(recs), np.uint64)
        some = np.zeros(len(recs), np.uint8)
        for i, (v, o) in enumerate(zip(recs["val"].tolist(), recs["op"].tolist())):
            if o:
                self.q.append(v)
                resp[i], some[i] = v, 1
            elif self.q:
                resp[i], some[i] = self.q.popleft(), 1
        return resp, some

    def dump(self):
        return np.array(list(self.q), np.uint64)


# ---- stack ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("path", ["exec", "fused"])
def test_stack_grows_under_replay(nrg, orc, path, pipeline):
    """Capacity 64, chunks of 4096, bound 2^16: three rounds of 5000 ops at 75 % Pushes. A round is
    two chunks (4096 + 904), so the buffer grows between the chunks of one nrg_log_exec."""
    import torch

    L = nrg._lib
    n, mb, bound = 5000, 4096, 1 << 16
    dev = nrg.DeviceReplica(L.NRG_DS_STACK, 0, stack_capacity=64, max_batch=mb, pipeline=pipeline,
                            log_bytes=LOG_BYTES)
    dev.set_max_capacity(bound)
    assert dev.st_capacity() == 64
    os_ = orc.Stack(np.zeros(0, np.uint32))
    rng = np.random.default_rng(1234 + pipeline)
    for r in range(3):
        vals = rng.integers(0, 2**32 - 1, n, dtype=np.uint32)
        ops = (rng.random(n) < 0.75).astype(np.uint32)
        recs = _st_ops(nrg, vals, ops)
        if path == "exec":
            first = dev.log_append(recs, 1)
            resp, some = dev.log_exec(first, first + n)
        else:
            outs = []
            for lo in range(0, n, mb):  # a fused round takes at most max_batch ops
                k = min(mb, n - lo)
                d_ops = _cuda(recs[lo:lo + k])
                d_resp = torch.zeros(k, dtype=torch.int32, device="cuda")
                d_some = torch.zeros(k, dtype=torch.uint8, device="cuda")
                dev.st_round_device(d_ops, k, 1, d_resp, d_some)
                outs.append((d_ops, d_resp, d_some))
            dev.join()
            torch.cuda.synchronize()
            resp = np.concatenate([o[1].cpu().numpy().view(np.uint32) for o in outs])
            some = np.concatenate([o[2].cpu().numpy() for o in outs])
        oresp, osome = os_.replay(vals, ops)
        np.testing.assert_array_equal(some, osome)
        np.testing.assert_array_equal(resp, oresp)
        assert dev.st_len() == len(os_)
    dev.sync()  # no latch
    np.testing.assert_array_equal(dev.st_dump(), os_.dump())
    assert dev.digest() == tuple(digest.stack(os_.dump()))
    cap = dev.st_capacity()
    print("stack", path, pipeline, "length", len(os_), "capacity", cap)
    assert len(os_) > 4096  # (the stream really outgrew the first reallocation)
    assert len(os_) <= cap <= bound
    dev.close()


def test_stack_balanced_stream_never_reallocates(nrg, orc):
    """The host's bound on the length passes the capacity, the exact length does not: ten balanced
    rounds of 4096 ops re-read the length and leave the capacity at 8192."""
    L = nrg._lib
    dev = nrg.DeviceReplica(L.NRG_DS_STACK, 0, stack_capacity=8192, max_batch=4096, log_bytes=LOG_BYTES)
    dev.set_max_capacity(1 << 16)
    os_ = orc.Stack(np.zeros(0, np.uint32))
    ops = np.tile(np.array([1, 0], np.uint32), 2048)
    for r in range(10):
        vals = (np.arange(4096, dtype=np.uint32) + np.uint32(4096 * r)) | np.uint32(1 << 30)
        first = dev.log_append(_st_ops(nrg, vals, ops), 1)
        resp, some = dev.log_exec(first, first + 4096)
        oresp, osome = os_.replay(vals, ops)
        np.testing.assert_array_equal(some, osome)
        np.testing.assert_array_equal(resp, oresp)
    assert dev.st_len() == 0
    assert dev.st_capacity() == 8192
    dev.close()


def test_stack_latches_only_past_the_bound(nrg):
    """Capacity 64, bound 256, 1000 Pushes: grown to the bound, then the latch, reported once by the
    next nrg_sync; the length reads 256 (nrg_stack_len's clamp)."""
    L = nrg._lib
    dev = nrg.DeviceReplica(L.NRG_DS_STACK, 0, stack_capacity=64, max_batch=4096, log_bytes=LOG_BYTES)
    dev.set_max_capacity(256)
    vals = np.arange(1000, dtype=np.uint32) + np.uint32(7)
    d_ops = _cuda(_st_ops(nrg, vals, np.ones(1000, np.uint32)))
    dev.st_round_device(d_ops, 1000, 1)
    with pytest.raises(nrg.NrgError) as e:
        dev.sync()
    assert e.value.code == L.NRG_E_CAPACITY
    dev.sync()  # once
    assert dev.st_capacity() == 256
    assert dev.st_len() == 256
    np.testing.assert_array_equal(dev.st_dump(), vals[:256])
    dev.close()


@pytest.mark.parametrize("n0", [50, 70001])  # 16-B units and a tail of 2 and of 1; one and many workgroups
def test_stack_reserve(nrg, orc, n0):
    L = nrg._lib
    lib = L.load()
    dev = nrg.DeviceReplica(L.NRG_DS_STACK, 0, stack_capacity=max(64, n0), max_batch=4096, log_bytes=LOG_BYTES)
    init = np.random.default_rng(n0).integers(0, 2**32 - 1, n0, dtype=np.uint32)
    dev.st_init(init)
    os_ = orc.Stack(init)
    want = tuple(digest.stack(init))
    assert dev.digest() == want
    big = 10_000 if n0 == 50 else 200_000
    dev.st_reserve(big)
    assert dev.st_capacity() == big
    np.testing.assert_array_equal(dev.st_dump(), init)
    assert dev.st_len() == n0 and dev.digest() == want
    dev.st_reserve(10)  # never shrinks: nothing happens
    assert dev.st_capacity() == big
    np.testing.assert_array_equal(dev.st_dump(), init)
    # the room is real: Pushes past the old capacity, then Pops that reach below the copied part
    vals = np.arange(4000, dtype=np.uint32)
    ops = np.concatenate([np.ones(3000, np.uint32), np.zeros(1000, np.uint32)])
    first = dev.log_append(_st_ops(nrg, vals, ops), 1)
    resp, some = dev.log_exec(first, first + 4000)
    oresp, osome = os_.replay(vals, ops)
    np.testing.assert_array_equal(some, osome)
    np.testing.assert_array_equal(resp, oresp)
    np.testing.assert_array_equal(dev.st_dump(), os_.dump())
    # argument checks
    assert lib.nrg_stack_reserve(dev.handle, 1 << 31) == L.NRG_E_INVAL
    q = nrg.DeviceReplica(L.NRG_DS_QUEUE, 0, queue_capacity=64, max_batch=64, log_bytes=LOG_BYTES)
    n = C.c_uint64()
    assert lib.nrg_stack_reserve(q.handle, 100) == L.NRG_E_INVAL
    assert lib.nrg_stack_capacity(q.handle, C.byref(n)) == L.NRG_E_INVAL
    assert lib.nrg_queue_reserve(dev.handle, 100) == L.NRG_E_INVAL
    assert lib.nrg_vspace_reserve(dev.handle, 100) == L.NRG_E_INVAL
    q.close()
    dev.close()


def test_set_max_capacity_arguments(nrg):
    L = nrg._lib
    lib = L.load()
    st = nrg.DeviceReplica(L.NRG_DS_STACK, 0, stack_capacity=64, max_batch=64, log_bytes=LOG_BYTES)
    assert lib.nrg_set_max_capacity(st.handle, 63) == L.NRG_E_INVAL  # below the capacity
    assert lib.nrg_set_max_capacity(st.handle, 1 << 31) == L.NRG_E_INVAL  # nrg_open's bound
    assert lib.nrg_set_max_capacity(st.handle, 64) == L.NRG_OK
    assert lib.nrg_set_max_capacity(st.handle, 0) == L.NRG_OK  # off again
    st.close()
    qu = nrg.DeviceReplica(L.NRG_DS_QUEUE, 0, queue_capacity=64, max_batch=64, log_bytes=LOG_BYTES)
    assert lib.nrg_set_max_capacity(qu.handle, 63) == L.NRG_E_INVAL
    assert lib.nrg_set_max_capacity(qu.handle, (1 << 32) + 1) == L.NRG_E_INVAL
    assert lib.nrg_set_max_capacity(qu.handle, 1 << 12) == L.NRG_OK
    qu.close()
    for kind, cfg in ((L.NRG_DS_HASHMAP, dict(log2_slots=10, max_batch=64)), (L.NRG_DS_SYNTHETIC, dict(max_batch=64)),
                      (L.NRG_DS_VSPACE, dict(log2_slots=2, max_batch=64))):
        d = nrg.DeviceReplica(kind, 0, log_bytes=LOG_BYTES, **cfg)
        assert lib.nrg_set_max_capacity(d.handle, 1 << 20) == L.NRG_E_INVAL
        d.close()


# ---- queue ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("explicit", [True, False], ids=["reserve", "auto"])
def test_queue_regrows_a_wrapped_ring(nrg, explicit):
    """Capacity 64 and max_batch 64 make a ring of 128. 60 elements, then rounds of alternating
    Pop / Push until the front is past position 80: the live range wraps the ring's end. reserve:
    nrg_queue_reserve(1000) re-lays it out; then, with a bound, rounds of 64 Pushes up to 500
    elements. auto: the same Pushes without the reserve, so replay re-lays out a wrapped ring."""
    L = nrg._lib
    dev = nrg.DeviceReplica(L.NRG_DS_QUEUE, 0, queue_capacity=64, max_batch=64, log_bytes=LOG_BYTES)
    rng = np.random.default_rng(99)
    init = rng.integers(0, 2**64 - 1, 60, dtype=np.uint64)
    dev.qu_init(init)
    m = _QueueModel(init)

    def round_(recs):
        first = dev.log_append(recs, 1)
        resp, some = dev.log_exec(first, first + len(recs))
        oresp, osome = m.replay(recs)
        np.testing.assert_array_equal(some, osome)
        np.testing.assert_array_equal(resp, oresp)

    head = 0
    while head <= 80:
        round_(_qu_ops(nrg, rng.integers(0, 2**64 - 1, 64, dtype=np.uint64), np.tile(np.array([0, 1], np.uint64), 32)))
        head += 32
    assert 128 - (head % 128) < 60  # [head, head + 60) crosses the end of the ring of 128
    want = tuple(digest.queue(m.dump().tolist()))
    assert dev.digest() == want
    if explicit:
        dev.qu_reserve(1000)
        assert dev.qu_capacity() == 1000
        assert dev.qu_len() == 60
        np.testing.assert_array_equal(dev.qu_dump(), m.dump())
        assert dev.digest() == want
        dev.qu_reserve(10)
        assert dev.qu_capacity() == 1000
    dev.set_max_capacity(4096)
    while len(m.q) < 500:
        round_(_qu_ops(nrg, rng.integers(0, 2**64 - 1, 64, dtype=np.uint64), np.ones(64, np.uint64)))
    dev.sync()  # no latch
    assert dev.qu_len() == len(m.q)
    np.testing.assert_array_equal(dev.qu_dump(), m.dump())
    assert dev.digest() == tuple(digest.queue(m.dump().tolist()))
    assert len(m.q) <= dev.qu_capacity() <= 4096
    # Pops drain it in order through the new ring
    round_(_qu_ops(nrg, np.zeros(64, np.uint64), np.zeros(64, np.uint64)))
    np.testing.assert_array_equal(dev.qu_dump(), m.dump())
    dev.close()


def test_queue_chunk_larger_than_the_capacity(nrg):
    """Capacity 64, one chunk of 4096 Pushes, bound 2^14: no latch."""
    L = nrg._lib
    dev = nrg.DeviceReplica(L.NRG_DS_QUEUE, 0, queue_capacity=64, max_batch=4096, log_bytes=LOG_BYTES)
    dev.set_max_capacity(1 << 14)
    m = _QueueModel()
    recs = _qu_ops(nrg, np.arange(4096, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15), np.ones(4096, np.uint64))
    first = dev.log_append(recs, 1)
    resp, some = dev.log_exec(first, first + 4096)  # (raises on a latched NRG_E_CAPACITY)
    oresp, osome = m.replay(recs)
    np.testing.assert_array_equal(some, osome)
    np.testing.assert_array_equal(resp, oresp)
    dev.sync()
    assert dev.qu_len() == 4096
    np.testing.assert_array_equal(dev.qu_dump(), m.dump())
    assert 4096 <= dev.qu_capacity() <= 1 << 14
    dev.close()


# ---- page table ----------------------------------------------------------------------------------
def test_vspace_reserve(nrg):
    """A pool of four tables, filled exactly by a Map of four pages (PML4, PDPT, PD, PT). The digest
    before nrg_vspace_reserve(64) sized its tag buffer for four tables; the one after must use the
    new pool's. A Map in another 512 GiB region then finds room."""
    L = nrg._lib
    lib = L.load()
    dev = nrg.DeviceReplica(L.NRG_DS_VSPACE, 0, log2_slots=2, max_batch=64, log_bytes=LOG_BYTES)
    m = VSpaceModel()

    def map_(vbase, pbase, pages):
        recs = np.zeros(1, nrg.VSPACE_OP_DTYPE)
        recs[0] = (vbase, pbase, pages * KB4, L.NRG_VSPACE_MAP, 3)
        first = dev.log_append(recs, 1)
        resp, some = dev.log_exec(first, first + 1)
        a, b, osome = m.replay(recs)
        np.testing.assert_array_equal(some, osome)
        np.testing.assert_array_equal(resp["a"], a)
        np.testing.assert_array_equal(resp["b"], b)
        return int(some[0])

    assert dev.vs_capacity() == 4
    assert map_(0x200000, 0x7000_0000, 4) == 1
    assert dev.vs_tables() == 4 == m.tables()
    d0 = dev.digest()
    assert d0 == tuple(digest.vspace(*m.dump()))
    dev.vs_reserve(64)
    assert dev.vs_capacity() == 64
    assert dev.digest() == d0
    assert dev.vs_tables() == 4
    far = 5 << 39
    assert map_(far + 0x1000, 0x9000_0000, 4) == 1
    assert dev.vs_tables() == 7 == m.tables()
    va = np.array([0x200000, 0x200fff, 0x203000, 0x204000, far + 0x1000, far + 0x4abc, far, 1 << 39], np.uint64)
    pa, found = dev.vs_resolve(va)
    want = [m.resolve(int(a)) for a in va]
    np.testing.assert_array_equal(pa, np.array([w[0] for w in want], np.uint64))
    np.testing.assert_array_equal(found, np.array([w[1] for w in want], np.uint8))
    leaves = dev.vs_dump()
    mva, men = m.dump()
    np.testing.assert_array_equal(leaves["vaddr"], mva)
    np.testing.assert_array_equal(leaves["entry"], men)
    assert dev.digest() == tuple(digest.vspace(mva, men))
    dev.vs_reserve(3)
    assert dev.vs_capacity() == 64
    assert lib.nrg_vspace_reserve(dev.handle, (1 << 22) + 1) == L.NRG_E_INVAL
    assert dev.vs_capacity() == 64 and dev.vs_tables() == 7
    # nrg_open's bound stays
    with pytest.raises(nrg.NrgError) as e:
        nrg.DeviceReplica(L.NRG_DS_VSPACE, 0, log2_slots=23, max_batch=64, log_bytes=LOG_BYTES)
    assert e.value.code == L.NRG_E_INVAL
    dev.close()


# ---- restore -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stack", "queue"])
def test_restore_grows_up_to_the_bound(nrg, name):
    """An image of 1000 elements into a replica of capacity 64: with bound 4096 it grows first, with
    bound 512 it is refused with NRG_E_CAPACITY and the replica is as it was."""
    L = nrg._lib
    rng = np.random.default_rng(31)
    if name == "stack":
        kind, cfg, big = L.NRG_DS_STACK, dict(max_batch=64, log_bytes=LOG_BYTES), dict(stack_capacity=4096)
        small = dict(stack_capacity=64)
        vals, few = rng.integers(0, 2**32 - 1, 1000, dtype=np.uint32), np.arange(10, dtype=np.uint32)
        init, dump, cap = "st_init", "st_dump", "st_capacity"
    else:
        kind, cfg, big = L.NRG_DS_QUEUE, dict(max_batch=64, log_bytes=LOG_BYTES), dict(queue_capacity=4096)
        small = dict(queue_capacity=64)
        vals, few = rng.integers(0, 2**64 - 1, 1000, dtype=np.uint64), np.arange(10, dtype=np.uint64)
        init, dump, cap = "qu_init", "qu_dump", "qu_capacity"
    a = nrg.DeviceReplica(kind, 0, **cfg, **big)
    getattr(a, init)(vals)
    img = a.snapshot()
    want = a.digest()
    a.close()
    b = nrg.DeviceReplica(kind, 0, **cfg, **small)
    getattr(b, init)(few)
    b.set_max_capacity(4096)
    b.restore(img)
    assert b.digest() == want
    np.testing.assert_array_equal(getattr(b, dump)(), vals)
    assert 1000 <= getattr(b, cap)() <= 4096
    b.close()
    c = nrg.DeviceReplica(kind, 0, **cfg, **small)
    getattr(c, init)(few)
    before = c.digest()
    c.set_max_capacity(512)
    with pytest.raises(nrg.NrgError) as e:
        c.restore(img)
    assert e.value.code == L.NRG_E_CAPACITY
    assert getattr(c, cap)() == 64 and c.digest() == before
    np.testing.assert_array_equal(getattr(c, dump)(), few)
    c.close()


# ---- combiner ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stack", "queue"])
def test_growth_under_a_combiner(nrg, name):
    """Capacity 64, max_batch 128, bound 2^16: four threads each make 25 calls of 32 Pushes through
    the combiner, whose rounds grow the structure from its own thread."""
    L = nrg._lib
    T, CALLS = 4, 25
    if name == "stack":
        dev = nrg.DeviceReplica(L.NRG_DS_STACK, 0, stack_capacity=64, max_batch=128, log_bytes=LOG_BYTES)
        dtype, push = nrg.STACK_OP_DTYPE, L.NRG_STACK_PUSH
    else:
        dev = nrg.DeviceReplica(L.NRG_DS_QUEUE, 0, queue_capacity=64, max_batch=128, log_bytes=LOG_BYTES)
        dtype, push = nrg.QUEUE_OP_DTYPE, L.NRG_QUEUE_PUSH
    dev.set_max_capacity(1 << 16)
    comb = nrg.Combiner(dev, T)
    errors = []

    def client(i):
        try:
            tok = comb.register()
            for c in range(CALLS):
                recs = np.zeros(32, dtype)
                recs["op"] = push
                recs["val"] = ((i + 1) << 20) | (c << 8) | np.arange(32)
                comb.execute_mut(tok, recs)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=client, args=(i,)) for i in range(T)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    comb.close()
    assert not errors, errors[0]
    pushed = sorted(((i + 1) << 20) | (c << 8) | k for i in range(T) for c in range(CALLS) for k in range(32))
    if name == "stack":
        assert dev.st_len() == 3200
        got, cap = dev.st_dump(), dev.st_capacity()
    else:
        assert dev.qu_len() == 3200
        got, cap = dev.qu_dump(), dev.qu_capacity()
    assert sorted(int(v) for v in got) == pushed
    assert 3200 <= cap <= 1 << 16
    dev.close()


# ---- group ---------------------------------------------------------------------------------------
def test_growth_in_a_group(nrg, orc):
    """Two loopback members, stack capacity 64, the bound on each member's replica: three rounds of
    300 Pushes per member. Both replicas grow at the same record: identical digests, equal
    capacities, and the oracle's state."""
    import torch

    L = nrg._lib
    lib = L.load()
    G = 2
    cfg = L.default_config(L.NRG_DS_STACK)
    cfg.stack_capacity, cfg.max_batch, cfg.log_bytes = 64, 4096, LOG_BYTES
    L.check(lib.nrg_test_loopback_collectives(1))
    g = C.c_void_p()
    try:
        L.check(lib.nrg_group_open((C.c_int * G)(*([0] * G)), G, C.byref(cfg), C.byref(g)), "nrg_group_open")
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))
    reps = [C.c_void_p(lib.nrg_group_replica(g, i)) for i in range(G)]
    for h in reps:
        L.check(lib.nrg_set_max_capacity(h, 1 << 16), "set_max_capacity")
    os_ = orc.Stack(np.zeros(0, np.uint32))
    keep = []
    for r in range(3):
        rd = (L.Round * G)()
        for i in range(G):
            vals = (np.arange(300, dtype=np.uint32) + np.uint32(1000 * (2 * r + i))) | np.uint32(1 << 28)
            ops = np.ones(300, np.uint32)
            d_ops = _cuda(_st_ops(nrg, vals, ops))
            rd[i].recs, rd[i].n = d_ops.data_ptr(), 300
            keep.append(d_ops)
            os_.replay(vals, ops)  # (in rank order: the log is W_0 || W_1)
        torch.cuda.synchronize()
        L.check(lib.nrg_group_round_async(g, rd, None), f"round {r}")
    out = np.zeros((G, 3), np.uint64)
    same = C.c_int(-1)
    L.check(lib.nrg_group_verify(g, out.ctypes.data_as(C.c_void_p), C.byref(same)), "verify")
    assert same.value == 1
    want = tuple(digest.stack(os_.dump()))
    caps = []
    for i, h in enumerate(reps):
        assert tuple(int(x) for x in out[i]) == want, f"rank {i}"
        n = C.c_uint64()
        L.check(lib.nrg_stack_capacity(h, C.byref(n)))
        caps.append(n.value)
        got = np.zeros(1800, np.uint32)
        m = C.c_uint64()
        L.check(lib.nrg_stack_dump(h, got.ctypes.data_as(C.c_void_p), 1800, C.byref(m)), "dump")
        assert m.value == 1800
        np.testing.assert_array_equal(got, os_.dump())
    assert caps[0] == caps[1] and 1800 <= caps[0] <= 1 << 16
    assert lib.nrg_group_close(g) == L.NRG_OK
