"""Queue replay on structured Push/Pop streams and wide scans, bit-exact against the deque model.

The random walk of tests/test_gpu_queue.py gives the scan workgroup one tile per lane, takes a
Pop's element from a tile or two back and touches the empty queue briefly. The named streams of
tests/queue_streams.py reach the rest of csrc/queue.hip -- two and three tiles per scan lane with
lanes past the last tile, the first Pop of one of the chunk's own Pushes at either end of a row, a
wave and a tile, exactly as many Pops as elements from before the chunk and one more, whole tiles
of Pops on the empty queue, Pops five tiles or one lane after their Push, ring positions that pass
the physical ring's end in a later tile, a length that peaks at the capacity and one above it --
and tests/test_queue_streams_cpu.py asserts from a model that each stream does reach the arm it is
named for. Every profile goes through the ring (append + exec) and the fused round; all but the
scans also through chunks whose edges are no tile multiple and through a response window that
begins and ends inside a row, between guard words. Every response word, every `some` byte, the
length and the contents after every round must equal the model's; device buffers start out as
sentinels so an unwritten answer shows.
"""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import queue_streams as S

pytestmark = pytest.mark.gpu

PARITY = [n for n in S.PROFILES if n != "over_by_one"]  # (its own test: the round ends in an error)
SMALL = [n for n in PARITY if n not in S.SCANS]
GUARD = 64

_case = itertools.count(1)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(profile, init, rounds, per round (resp, some, contents after it)) from the deque model,
    computed once and read-only"""
    p = S.PROFILES[name]()
    init, rounds = S.values(p)
    per, cur = [], init
    for rnd in rounds:
        ((resp, some),), cur = S.deque_model(cur, [rnd])
        for a in (resp, some, cur):
            a.setflags(write=False)
        per.append((resp, some, cur))
    return p, init, rounds, per


@functools.lru_cache(maxsize=None)
def _plans(name):
    return S.plans(S.PROFILES[name]())


def _expected(name):
    """The profile and the model's answers for one test case. Every value of the case carries a
    salt of its own (k << 48, above INIT_BASE and any op index): values stay unique, and no case
    expects a number an earlier case left behind in device memory the allocator hands out again
    -- a ring slot nobody wrote, a response nobody stored -- so a read of one cannot pass."""
    p, init, rounds, per = _reference(name)
    k = np.uint64(next(_case) << 48)
    assert k < 1 << 63
    return (p, init + k, [(v + k, o) for v, o in rounds],
            [(resp + k * some.astype(np.uint64), some, dump + k) for resp, some, dump in per])


def _recs(vals, ops):
    import nrgpu

    r = np.zeros(len(ops), nrgpu.QUEUE_OP_DTYPE)
    r["val"], r["op"] = vals, ops
    return r


def _cuda(recs):
    import torch

    return torch.from_numpy(recs.view(np.int64).copy()).cuda()


def _open(nrg, p, init, **cfg):
    """a replica sized to the profile: the log holds every round, a chunk a whole round"""
    total = sum(len(o) for o in p["rounds"])
    entries = 1 << 14
    while entries < total + (1 << 14):
        entries <<= 1
    cap, mb = S.config(p)
    cfg.setdefault("queue_capacity", cap)
    cfg.setdefault("max_batch", mb)
    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_QUEUE, 0, log_bytes=64 * entries, **cfg)
    dev.qu_init(init)
    return dev


def _sentinels(n):
    import torch

    return (torch.full((n,), -1, dtype=torch.int64, device="cuda"),
            torch.full((n,), 7, dtype=torch.uint8, device="cuda"))


def _check(resp, some, want, what):
    import torch

    if isinstance(resp, torch.Tensor):
        resp, some = resp.cpu().numpy().view(np.uint64), some.cpu().numpy()
    np.testing.assert_array_equal(some, want[1], err_msg=f"{what} some")
    np.testing.assert_array_equal(resp, want[0], err_msg=f"{what} resp")


def _check_state(dev, dump, what):
    assert dev.qu_len() == len(dump), what
    np.testing.assert_array_equal(dev.qu_dump(), dump, err_msg=f"{what} contents")


def _ring_case(nrg, name, **cfg):
    p, init, rounds, per = _expected(name)
    dev = _open(nrg, p, init, **cfg)
    _check_state(dev, init, f"{name} init")
    for r, (vals, ops) in enumerate(rounds):
        first = dev.log_append(_recs(vals, ops), 1)
        resp, some = dev.log_exec(first, first + len(ops))
        _check(resp, some, per[r], f"{name} round {r}")
        _check_state(dev, per[r][2], f"{name} round {r}")
    dev.sync()  # no error was latched (at_capacity: the length reached the capacity, no more)
    dev.close()


@pytest.mark.parametrize("name", PARITY)
def test_ring(nrg, name):
    """log_append + log_exec: records from the ring, responses to the host"""
    _ring_case(nrg, name)


def test_scan_stalled_waves(nrg):
    """two tiles per scan lane with odd waves asleep wherever the scan workgroup reuses LDS
    (NRG_KNOB_STALL): a missing barrier gives a wrong start length"""
    _ring_case(nrg, S.SCANS[0], knobs={"STALL": 1})


def _ring_records(nrg, dev, first, idx):
    L = nrg._lib
    size = dev.log_state()["size"]
    rec = np.zeros(len(idx), nrg.QUEUE_OP_DTYPE)
    for k, i in enumerate(idx):
        L.check(L.load().nrg_test_ring_read(dev.handle, (first + i) & (size - 1), rec[k:].ctypes.data))
    return rec


@pytest.mark.parametrize("name", PARITY)
def test_fused(nrg, name):
    """qu_round_device: the replay reads the caller's buffer and writes the log copy. A second
    replica runs the last round without response buffers and is left in the same state."""
    import torch

    p, init, rounds, per = _expected(name)
    a, b = _open(nrg, p, init), _open(nrg, p, init)
    for r, (vals, ops) in enumerate(rounds):
        n = len(ops)
        recs = _recs(vals, ops)
        d_ops = _cuda(recs)
        first = a.log_state()["tail"]
        resp, some = _sentinels(n)
        a.qu_round_device(d_ops, n, 1, resp, some)
        bresp, bsome = _sentinels(n)
        if r == len(rounds) - 1:
            b.qu_round_device(d_ops, n, 1, None, None)
        else:
            b.qu_round_device(d_ops, n, 1, bresp, bsome)
        torch.cuda.synchronize()
        _check(resp, some, per[r], f"{name} round {r}")
        if r == len(rounds) - 1:
            assert bool((bresp == -1).all()) and bool((bsome == 7).all())
        else:
            _check(bresp, bsome, per[r], f"{name} round {r} (second replica)")
        _check_state(a, per[r][2], f"{name} round {r}")
        _check_state(b, per[r][2], f"{name} round {r} (second replica)")
        idx = [i for i in (0, 63, 64, S.T - 1, S.T, n - 1) if i < n]
        for dev in (a, b):
            assert _ring_records(nrg, dev, first, idx).tobytes() == recs[idx].tobytes(), f"{name} round {r} log copy"
        sa, sb = a.log_state(), b.log_state()
        assert (sa["tail"], sa["ltail"]) == (sb["tail"], sb["ltail"]) == (first + n, first + n)
    a.sync()
    b.sync()
    a.close()
    b.close()


@pytest.mark.parametrize("name", SMALL)
def test_chunks(nrg, name):
    """max_batch 3000 (ring_wrap: its 5000, two rounds at a time): what is appended in pieces of at
    most max_batch replays in one log_exec as several chunks whose edges are no tile multiple, each
    from the head and length the one before published"""
    p, init, rounds, per = _expected(name)
    mb, step = (5000, 2) if name == "ring_wrap" else (3000, 1)
    dev = _open(nrg, p, init, max_batch=mb)
    for g in range(0, len(rounds), step):
        group = range(g, min(g + step, len(rounds)))
        recs = np.concatenate([_recs(*rounds[r]) for r in group])
        n = len(recs)
        assert mb % S.T  # (the cross profiles of one tile or less are one chunk here too)
        firsts = [dev.log_append(recs[at:at + mb], 1) for at in range(0, n, mb)]
        assert firsts == [firsts[0] + at for at in range(0, n, mb)]
        resp, some = dev.log_exec(firsts[0], firsts[0] + n)
        want = (np.concatenate([per[r][0] for r in group]), np.concatenate([per[r][1] for r in group]))
        _check(resp, some, want, f"{name} rounds {list(group)}")
        _check_state(dev, per[group[-1]][2], f"{name} rounds {list(group)}")
    dev.sync()
    dev.close()


@pytest.mark.parametrize("name", SMALL)
def test_window(nrg, name):
    """Responses for [lo + a, lo + b) only, a and b inside a row, written into the middle of
    larger sentinel tensors: the answers are the model's, the 64 words on either side are still
    sentinels, and the state is the full round's."""
    import torch

    p, init, rounds, per = _expected(name)
    dev = _open(nrg, p, init)
    for r, ((vals, ops), pl) in enumerate(zip(rounds, _plans(name))):
        a, b = S.window(pl)
        assert 0 < a < b < len(ops) and a % S.ROW and b % S.ROW
        m = b - a
        first = dev.log_append(_recs(vals, ops), 1)
        resp, some = _sentinels(m + 2 * GUARD)
        dev.log_exec_device(first + a, first + b, resp[GUARD:GUARD + m], some[GUARD:GUARD + m])
        torch.cuda.synchronize()
        for side in (slice(0, GUARD), slice(GUARD + m, None)):
            assert bool((resp[side] == -1).all()) and bool((some[side] == 7).all()), f"{name} round {r} guard"
        _check(resp[GUARD:GUARD + m], some[GUARD:GUARD + m], (per[r][0][a:b], per[r][1][a:b]),
               f"{name} round {r} window [{a}, {b})")
        _check_state(dev, per[r][2], f"{name} round {r}")
    dev.sync()
    dev.close()


@pytest.mark.parametrize("path", ["ring", "fused"])
def test_over_by_one_latches_once(nrg, path):
    """at_capacity with one more Push at the peak, in tile 1: the length is 5001 for one op and the
    round ends at 4999. NRG_E_CAPACITY is reported once and the length stays within the capacity."""
    import torch

    p, init, rounds, _ = _expected("over_by_one")
    (vals, ops), = rounds
    cap = S.config(p)[0]
    dev = _open(nrg, p, init)
    with pytest.raises(nrg.NrgError) as e:
        if path == "ring":
            first = dev.log_append(_recs(vals, ops), 1)
            dev.log_exec(first, first + len(ops))
        else:
            d_ops = _cuda(_recs(vals, ops))
            resp, some = _sentinels(len(ops))
            dev.qu_round_device(d_ops, len(ops), 1, resp, some)
            torch.cuda.synchronize()
            dev.sync()
    assert e.value.code == nrg._lib.NRG_E_CAPACITY
    dev.sync()  # latched once: the error was reported and cleared
    ln = dev.qu_len()
    assert ln <= cap
    assert len(dev.qu_dump()) == ln
    dev.close()


def test_wrapped_ring_digest_snapshot_reserve(nrg):
    """ring_wrap up to the round that leaves 2500 elements wrapped round the end of the 8192-slot
    ring: the digest is the model's, a snapshot restored into a second replica dumps the same
    elements, qu_reserve(20000) re-lays them out (thousands of wrapped elements over many
    workgroups) keeping contents and digest, and both replicas replay the later rounds to the
    model's answers."""
    from nrgpu import digest

    p, init, rounds, per = _expected("ring_wrap")
    dev, other = _open(nrg, p, init), _open(nrg, p, init[:1])
    k = S.RING_WRAPPED_AFTER
    for r in range(k + 1):
        first = dev.log_append(_recs(*rounds[r]), 1)
        resp, some = dev.log_exec(first, first + len(rounds[r][1]))
        _check(resp, some, per[r], f"round {r}")
    dump = per[k][2]
    want = tuple(digest.queue(dump))
    assert want[0] == len(dump) == 2500
    _check_state(dev, dump, "wrapped")
    assert dev.digest() == want
    other.restore(dev.snapshot())
    _check_state(other, dump, "restored")
    assert other.digest() == want
    dev.qu_reserve(20000)
    assert dev.qu_capacity() == 20000
    _check_state(dev, dump, "after reserve")
    assert dev.digest() == want
    for what, d in (("grown", dev), ("restored", other)):
        for r in range(k + 1, len(rounds)):
            first = d.log_append(_recs(*rounds[r]), 1)
            resp, some = d.log_exec(first, first + len(rounds[r][1]))
            _check(resp, some, per[r], f"{what} round {r}")
            _check_state(d, per[r][2], f"{what} round {r}")
        d.sync()
        d.close()


@pytest.mark.parametrize("name", ["fill_drain", "saw_empty", "cross_tile_2"])
def test_group(nrg, name):
    """G = 2 over the loopback collectives, every round cut at an odd op index, one part per
    member: each member's responses for its own segment of the gathered log, and both final
    queues, equal the model's. Member 1's window starts mid-row and its pending Pops take member
    0's Pushes."""
    import torch

    L = nrg._lib
    lib = L.load()
    G = 2
    p, init, rounds, per = _expected(name)
    cfg = L.default_config(L.NRG_DS_QUEUE)
    cfg.max_batch, cfg.queue_capacity = 1 << 16, S.config(p)[0]
    cfg.log_bytes = 64 * (1 << 16)
    L.check(lib.nrg_test_loopback_collectives(1))
    g = C.c_void_p()
    try:
        L.check(lib.nrg_group_open((C.c_int * G)(*([0] * G)), G, C.byref(cfg), C.byref(g)), "nrg_group_open")
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))
    ctxs = [lib.nrg_group_replica(g, i) for i in range(G)]
    for c in ctxs:
        L.check(lib.nrg_queue_init(c, init.ctypes.data_as(C.c_void_p), len(init)))
    outs = []
    for r, (vals, ops) in enumerate(rounds):
        n = len(ops)
        cut = (n // 2) | 1
        assert cut % S.ROW and 0 < cut < n
        recs = _recs(vals, ops)
        rd = (L.Round * G)()
        keep = []
        for i, (lo, hi) in enumerate(((0, cut), (cut, n))):
            d_ops = _cuda(recs[lo:hi])
            resp, some = _sentinels(hi - lo)
            rd[i].recs, rd[i].n = d_ops.data_ptr(), hi - lo
            rd[i].resp, rd[i].some = resp.data_ptr(), some.data_ptr()
            keep.append((d_ops, resp, some, lo, hi))
        torch.cuda.synchronize()
        L.check(lib.nrg_group_round_async(g, rd, None), f"{name} group round {r}")
        outs.append(keep)
    L.check(lib.nrg_group_sync(g))
    for r, keep in enumerate(outs):
        for i, (_, resp, some, lo, hi) in enumerate(keep):
            _check(resp, some, (per[r][0][lo:hi], per[r][1][lo:hi]), f"{name} round {r} member {i}")
    want = per[-1][2]
    for i, c in enumerate(ctxs):
        n = C.c_uint64()
        L.check(lib.nrg_queue_len(c, C.byref(n)))
        assert n.value == len(want)
        out = np.zeros(max(n.value, 1), np.uint64)
        m = C.c_uint64()
        L.check(lib.nrg_queue_dump(c, out.ctypes.data_as(C.c_void_p), n.value, C.byref(m)))
        np.testing.assert_array_equal(out[:m.value], want, err_msg=f"{name} member {i} queue")
    L.check(lib.nrg_group_close(g))
