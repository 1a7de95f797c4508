"""FIFO queue parity: the HIP replay (queue.hip) against a sequential collections.deque model.

The reference's queue is QueueWr::Push(u64) / QueueWr::Pop and QueueRd::Len
(benches/lockfree.rs:43-52) dispatched by SegQueueWrapper (benches/lockfree_comparisons.rs:75-101):
Push answers Some(v), Pop answers Some(front) or None on an empty queue, Len the length. Every
case compares each response, each `some` byte, the final contents and the length with the model,
bit for bit.
"""
import ctypes as C
import threading
from collections import Counter, deque

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 2048  # ops per workgroup of the replay kernels (queue.hip QU_TILE)
SIZES = [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, 1 << 16]


class Model:
    """The sequential queue (a VecDeque<u64>)."""

    def __init__(self, init=()):
        self.q = deque(int(v) for v in init)
        self.max_len = len(self.q)

    def replay(self, vals, ops):
        resp = np.zeros(len(ops), np.uint64)
        some = np.zeros(len(ops), np.uint8)
        q = self.q
        for i, (v, o) in enumerate(zip(vals.tolist(), ops.tolist())):
            if o == 1:
                q.append(v)
                resp[i], some[i] = v, 1
                if len(q) > self.max_len:
                    self.max_len = len(q)
            elif q:
                resp[i], some[i] = q.popleft(), 1
        return resp, some

    def dump(self):
        return np.array(list(self.q), np.uint64)


def _recs(nrg, vals, ops):
    r = np.zeros(len(ops), nrg.QUEUE_OP_DTYPE)
    r["val"], r["op"] = vals, ops
    return r


def _stream(n, seed):
    """a seeded 50/50 Push/Pop stream with distinct-looking 64-bit values"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 2**64 - 1, n, dtype=np.uint64), rng.integers(0, 2, n).astype(np.uint64)


def _open(nrg, **kw):
    kw.setdefault("max_batch", 1 << 16)
    kw.setdefault("queue_capacity", 1 << 17)
    kw.setdefault("log_bytes", 64 * (1 << 18))
    return nrg.DeviceReplica(nrg._lib.NRG_DS_QUEUE, 0, **kw)


def _check_state(dev, model):
    np.testing.assert_array_equal(dev.qu_dump(), model.dump())
    assert dev.qu_len() == len(model.q)


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _sizes_case(nrg, n, init_n, knobs=None):
    dev = _open(nrg, knobs=knobs)
    init = np.arange(init_n, dtype=np.uint64) + 1000
    dev.qu_init(init)
    model = Model(init)
    _check_state(dev, model)
    for r in range(2):  # the second round starts from the head and length the first published
        vals, ops = _stream(n, 31 * n + init_n + r)
        first = dev.log_append(_recs(nrg, vals, ops), 1)
        resp, some = dev.log_exec(first, first + n)
        oresp, osome = model.replay(vals, ops)
        np.testing.assert_array_equal(some, osome)
        np.testing.assert_array_equal(resp, oresp)
        _check_state(dev, model)
    dev.close()


@pytest.mark.parametrize("init_n", [0, 700])
@pytest.mark.parametrize("n", SIZES)
def test_queue_sizes(nrg, n, init_n):
    """One lane, one wave +-1, one tile +-1, several tiles with a ragged tail, 32 tiles."""
    _sizes_case(nrg, n, init_n)


@pytest.mark.parametrize("n", [3 * TILE + 5, 1 << 16])
def test_queue_sizes_stalled_waves(nrg, n):
    """The same with odd waves asleep wherever a workgroup reuses LDS (NRG_KNOB_STALL): a missing
    barrier gives a wrong answer."""
    _sizes_case(nrg, n, 700, knobs={"STALL": 1})


def test_queue_pops_on_empty_across_tiles(nrg):
    """10 elements, then 2 TILE + 7 Pops (failed Pops across tile boundaries), TILE Pushes and
    TILE + 3 Pops that take this chunk's own Pushes and then fail again."""
    dev = _open(nrg)
    init = np.arange(10, dtype=np.uint64) + 5
    dev.qu_init(init)
    model = Model(init)
    ops = np.concatenate([np.zeros(2 * TILE + 7), np.ones(TILE), np.zeros(TILE + 3)]).astype(np.uint64)
    vals = np.arange(len(ops), dtype=np.uint64) * 3 + (1 << 40)
    first = dev.log_append(_recs(nrg, vals, ops), 1)
    resp, some = dev.log_exec(first, first + len(ops))
    oresp, osome = model.replay(vals, ops)
    assert osome[:10].all() and not osome[10:2 * TILE + 7].any() and not osome[-3:].any()
    np.testing.assert_array_equal(some, osome)
    np.testing.assert_array_equal(resp, oresp)
    _check_state(dev, model)
    # Pops that straddle L0 in one chunk: 5 old elements, then the chunk's Pushes
    dev.qu_init(init[:5])
    model = Model(init[:5])
    ops = np.concatenate([np.ones(TILE + 9), np.zeros(TILE)]).astype(np.uint64)
    vals = np.arange(len(ops), dtype=np.uint64) + (1 << 50)
    first = dev.log_append(_recs(nrg, vals, ops), 1)
    resp, some = dev.log_exec(first, first + len(ops))
    oresp, osome = model.replay(vals, ops)
    np.testing.assert_array_equal(some, osome)
    np.testing.assert_array_equal(resp, oresp)
    _check_state(dev, model)
    dev.close()


def test_queue_chunked_exec_and_sub_window(nrg):
    """max_batch 3000: one append of 10 000 ops replays in four chunks, in order; then the same
    with responses wanted for a strict sub-range of the log indices only."""
    n = 10_000
    for window in (None, (2500, 7001)):
        dev = _open(nrg, max_batch=3000, queue_capacity=1 << 15)
        init = np.arange(100, dtype=np.uint64)
        dev.qu_init(init)
        model = Model(init)
        vals, ops = _stream(n, 5)
        first = dev.log_append(_recs(nrg, vals, ops), 1)
        lo, hi = (0, n) if window is None else window
        resp, some = dev.log_exec(first + lo, first + hi)
        oresp, osome = model.replay(vals, ops)
        assert len(resp) == hi - lo
        np.testing.assert_array_equal(some, osome[lo:hi])
        np.testing.assert_array_equal(resp, oresp[lo:hi])
        _check_state(dev, model)
        dev.close()


def test_queue_ring_wrap(nrg):
    """Capacity 1000 and max_batch 1024 give a physical ring of 2048 slots; 40 rounds of up to 500
    Pushes followed by as many Pops move the head past it many times."""
    cap = 1000
    dev = _open(nrg, max_batch=1024, queue_capacity=cap)
    init = np.arange(300, dtype=np.uint64)
    dev.qu_init(init)
    model = Model(init)
    rng = np.random.default_rng(9)
    popped = 0
    for r in range(40):
        k = int(rng.integers(300, 501))
        ops = np.concatenate([np.ones(k), np.zeros(k), np.ones(1024 - 2 * k)]).astype(np.uint64)
        ops[2 * k:] = (np.arange(1024 - 2 * k) + 1) % 2  # Push, Pop, Push, Pop, ... never above + 1
        vals = rng.integers(0, 2**64 - 1, 1024, dtype=np.uint64)
        first = dev.log_append(_recs(nrg, vals, ops), 1)
        resp, some = dev.log_exec(first, first + 1024)
        oresp, osome = model.replay(vals, ops)
        popped += int(osome[ops == 0].sum())
        np.testing.assert_array_equal(some, osome, err_msg=f"round {r}")
        np.testing.assert_array_equal(resp, oresp, err_msg=f"round {r}")
        _check_state(dev, model)
    assert model.max_len <= cap  # the rounds never overflowed: no error was latched to pass this
    assert popped > 4 * 2048     # the head passed the physical ring several times
    dev.sync()
    dev.close()


def test_queue_overflow_latches_capacity_once(nrg):
    dev = _open(nrg, max_batch=2048, queue_capacity=1000)
    n = 1500
    dev.log_append(_recs(nrg, np.arange(n, dtype=np.uint64), np.ones(n, np.uint64)), 1)
    with pytest.raises(nrg.NrgError) as e:
        dev.log_exec()
    assert e.value.code == nrg._lib.NRG_E_CAPACITY
    dev.sync()  # latched once: the error was reported and cleared
    ln = dev.qu_len()
    assert ln <= 1000
    assert len(dev.qu_dump()) == ln
    dev.close()


def test_queue_round_fused_equals_append_exec(nrg):
    """nrg_queue_round_async on one replica, append + exec on another: the same six rounds give
    the same responses and contents (and the model's); a round without response buffers leaves
    the same state."""
    import torch

    a, b = _open(nrg), _open(nrg)
    init = np.arange(500, dtype=np.uint64) * 7
    a.qu_init(init)
    b.qu_init(init)
    model = Model(init)
    for r in range(6):
        n = [5000, 1, TILE, 3 * TILE + 5, 300, 2 * TILE - 1][r]
        vals, ops = _stream(n, 400 + r)
        if r == 3:
            ops[: n // 2] = 0  # drains the queue: Pops on empty and Pops of the round's Pushes
        recs = _recs(nrg, vals, ops)
        d_ops = _cuda(recs)
        resp = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        some = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        if r == 4:
            a.qu_round_device(d_ops, n, 1, None, None)
        else:
            a.qu_round_device(d_ops, n, 1, resp, some)
        torch.cuda.synchronize()
        first = b.log_append(recs, 1)
        bresp, bsome = b.log_exec(first, first + n)
        oresp, osome = model.replay(vals, ops)
        np.testing.assert_array_equal(bsome, osome)
        np.testing.assert_array_equal(bresp, oresp)
        if r != 4:
            np.testing.assert_array_equal(some.cpu().numpy(), osome, err_msg=f"round {r}")
            np.testing.assert_array_equal(_u64(resp), oresp, err_msg=f"round {r}")
        else:
            assert (some.cpu().numpy() == 7).all()
        np.testing.assert_array_equal(a.qu_dump(), b.qu_dump())
        _check_state(a, model)
        sa, sb = a.log_state(), b.log_state()
        assert (sa["tail"], sa["ltail"]) == (sb["tail"], sb["ltail"])
    # the log copy the fused round wrote is the batch itself
    rec = np.zeros(1, nrg.QUEUE_OP_DTYPE)
    L = nrg._lib
    L.check(L.load().nrg_test_ring_read(a.handle, (a.log_state()["tail"] - 1) & (a.log_state()["size"] - 1),
                                        rec.ctypes.data))
    assert rec.tobytes() == recs[-1:].tobytes()
    a.close()
    b.close()


def test_queue_segments(nrg):
    """Three segments of unequal length and distinct origins appended in order; responses for the
    middle one only."""
    import torch

    dev = _open(nrg)
    init = np.arange(50, dtype=np.uint64)
    dev.qu_init(init)
    model = Model(init)
    lens, origins, stride = [1000, 37, 2500], [3, 1, 2], 2500
    buf = np.zeros(3 * stride, nrg.QUEUE_OP_DTYPE)
    parts = []
    for s, n in enumerate(lens):
        vals, ops = _stream(n, 70 + s)
        buf[s * stride: s * stride + n] = _recs(nrg, vals, ops)
        parts.append(model.replay(vals, ops))
    d_base = _cuda(buf)
    firsts = dev.log_append_segments(d_base, stride, lens, origins)
    assert firsts == [0, 1000, 1037]
    resp = torch.full((lens[1],), -1, dtype=torch.int64, device="cuda")
    some = torch.full((lens[1],), 7, dtype=torch.uint8, device="cuda")
    dev.log_exec_device(firsts[1], firsts[1] + lens[1], resp, some)
    dev.sync()
    np.testing.assert_array_equal(some.cpu().numpy(), parts[1][1])
    np.testing.assert_array_equal(_u64(resp), parts[1][0])
    _check_state(dev, model)
    dev.close()


def _group_sizes(G, r, full):
    """segment lengths of round r: equal, ragged with empty members, all empty, one writer, all
    but the last full"""
    kind = r % 5
    if kind == 0:
        return [full] * G
    if kind == 1:
        return [0 if i % 3 == 1 else (i * 977 + 311 + 131 * r) % full for i in range(G)]
    if kind == 2:
        return [0] * G
    if kind == 3:
        return [0] * (G - 1) + [full - 7]
    return [full] * (G - 1) + [full // 3]


@pytest.mark.parametrize("G", [2, 3])
def test_queue_group_members(nrg, G):
    """Queue group rounds over the loopback collectives: each member's responses for its own
    segment of the gathered log, and every member's final queue, equal the model's replay of
    W_0 || ... || W_{G-1}."""
    import torch

    L = nrg._lib
    lib = L.load()
    cfg = L.default_config(L.NRG_DS_QUEUE)
    cfg.max_batch, cfg.queue_capacity = 1 << 16, 1 << 17
    cfg.log_bytes = 64 * (1 << 16)
    L.check(lib.nrg_test_loopback_collectives(1))
    g = C.c_void_p()
    try:
        L.check(lib.nrg_group_open((C.c_int * G)(*([0] * G)), G, C.byref(cfg), C.byref(g)), "nrg_group_open")
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))
    ctxs = [lib.nrg_group_replica(g, i) for i in range(G)]
    init = np.arange(700, dtype=np.uint64)
    for c in ctxs:
        L.check(lib.nrg_queue_init(c, init.ctypes.data_as(C.c_void_p), len(init)))
    model = Model(init)
    outs = []
    for r in range(6):
        lens = _group_sizes(G, r, 3000)
        rd = (L.Round * G)()
        keep = []
        for i in range(G):
            n = lens[i]
            vals, ops = _stream(n, 40 * r + i)
            if n and r % 2:
                ops[: n // 2] = 0  # a Pop run deep into the earlier members' Pushes
            d_ops = _cuda(_recs(nrg, vals, ops)) if n else None
            resp = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")
            some = torch.full((max(n, 1),), 7, dtype=torch.uint8, device="cuda")
            rd[i].recs, rd[i].n = (d_ops.data_ptr() if n else 0), n
            rd[i].resp, rd[i].some = resp.data_ptr(), some.data_ptr()
            keep.append((d_ops, resp, some, n, model.replay(vals, ops)))
        torch.cuda.synchronize()
        L.check(lib.nrg_group_round_async(g, rd, None), f"queue group round {r}")
        outs.append(keep)
    L.check(lib.nrg_group_sync(g))
    for r, keep in enumerate(outs):
        for i, (_, resp, some, n, (oresp, osome)) in enumerate(keep):
            if n:
                np.testing.assert_array_equal(some[:n].cpu().numpy(), osome, err_msg=f"round {r} member {i} some")
                np.testing.assert_array_equal(_u64(resp[:n]), oresp, err_msg=f"round {r} member {i} values")
    want = model.dump()
    for i, c in enumerate(ctxs):
        n = C.c_uint64()
        L.check(lib.nrg_queue_len(c, C.byref(n)))
        assert n.value == len(want)
        out = np.zeros(max(n.value, 1), np.uint64)
        m = C.c_uint64()
        L.check(lib.nrg_queue_dump(c, out.ctypes.data_as(C.c_void_p), n.value, C.byref(m)))
        np.testing.assert_array_equal(out[:m.value], want, err_msg=f"member {i} queue")
    L.check(lib.nrg_group_close(g))


def test_queue_python_api(nrg):
    """Log + two Replica(Queue): execute_mut(Push / Pop) on one, execute(Len) on the other after
    it synced; verify sees equal contents on both."""
    from nrgpu import Len, Log, Pop, Push, Queue, Replica

    log = Log(64 * (1 << 16))
    r1 = Replica(log, Queue, 0, max_batch=4096, queue_capacity=4096)
    r2 = Replica(log, Queue, 0, max_batch=4096, queue_capacity=4096)
    t1, t2 = r1.register(), r2.register()
    assert r1.execute_mut(Pop(), t1) is None
    assert r1.execute_mut(Push(11), t1) == 11
    assert r1.execute_mut_batch([Push(2**64 - 1), Push(13), Pop(), Push(14)], t1) == [2**64 - 1, 13, 11, 14]
    assert r1.execute(Len(), t1) == 3
    r2.sync(t2)
    assert r2.execute(Len(), t2) == 3
    assert r2.execute_mut(Pop(), t2) == 2**64 - 1
    assert r1.execute(Len(), t1) == 2
    seen = []
    r1.verify(lambda q: seen.append(q))
    r2.verify(lambda q: seen.append(q))
    assert seen == [[13, 14], [13, 14]]


def test_queue_combiner_threads(nrg):
    """8 client threads, 200 calls each of up to 32 mixed Push / Pop with distinct values and Len
    reads in between. Whatever the interleaving: nothing is lost or invented (popped values plus
    the final contents are the initial plus the pushed values), every producer's values leave in
    its push order, and every Len lies in [0, capacity]."""
    T, CALLS, CAP, INIT = 8, 200, 1 << 14, 100
    dev = _open(nrg, max_batch=4096, queue_capacity=CAP, log_bytes=64 * (1 << 16))
    init = (np.arange(INIT, dtype=np.uint64) | np.uint64(0xFFFF << 32))
    dev.qu_init(init)
    comb = nrg.Combiner(dev, T)
    errors, pushed, popped, lens = [], {}, {}, []

    def client(seed):
        try:
            tok = comb.register()
            rng = np.random.default_rng(seed)
            mine, got, seq = [], [], 0
            for it in range(CALLS):
                n = int(rng.integers(1, 33))
                ops = rng.integers(0, 2, n).astype(np.uint64)
                vals = np.zeros(n, np.uint64)
                for i in range(n):
                    if ops[i]:
                        vals[i] = (tok << 32) | seq
                        seq += 1
                recs = np.zeros(n, nrg.QUEUE_OP_DTYPE)
                recs["val"], recs["op"] = vals, ops
                resp, some = comb.execute_mut(tok, recs)
                for i in range(n):
                    if ops[i]:
                        assert some[i] == 1 and resp[i] == vals[i], (tok, it, i)
                        mine.append(int(vals[i]))
                    elif some[i]:
                        got.append(int(resp[i]))
                    else:
                        assert resp[i] == 0
                if it % 2 == 0:
                    ln, sm = comb.execute(tok, n=int(rng.integers(1, 5)))
                    assert sm.all() and len(set(ln.tolist())) == 1
                    lens.append(int(ln[0]))
            pushed[tok], popped[tok] = mine, got
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=client, args=(300 + i,)) for i in range(T)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors[0]
    rounds, nops = comb.stats()
    assert nops > 0 and rounds <= 2 * T * CALLS
    comb.close()
    final = dev.qu_dump().tolist()
    assert dev.qu_len() == len(final)
    every_pop = [v for t in popped for v in popped[t]]
    every_push = [v for t in pushed for v in pushed[t]]
    assert Counter(every_pop + final) == Counter(init.tolist() + every_push)
    assert lens and all(0 <= x <= CAP for x in lens)
    # FIFO per producer: any one thread's Pops (ordered in the log) see a producer's values in its
    # push order, and what is still queued is newer than everything popped, in push order too
    last_popped = {}
    for t, got in popped.items():
        seen = {}
        for v in got:
            p, s = v >> 32, v & 0xFFFFFFFF
            assert seen.get(p, -1) < s, (t, p, s)
            seen[p] = s
            last_popped[p] = max(last_popped.get(p, -1), s)
    seen = {}
    for v in final:
        p, s = v >> 32, v & 0xFFFFFFFF
        assert seen.get(p, last_popped.get(p, -1)) < s, (p, s)
        seen[p] = s
    dev.close()
