"""The file store's logged reads of any length (nrg_memfs_pread_logged*, csrc/memfs.hip mf_rfrag /
mf_rgather / mf_rcount) against the model of tests/memfs_pread_logged_model.py. Every call is checked in
every observable: the records it logged, read back from the ring; some, counts and offs; the bytes of
every slot; a guard pattern intact in every byte of data outside [offs[i], offs[i] + count[i]) and at or
past offs[n]; the files and the digest unchanged; the tail advanced by exactly T.

Shapes are the smallest at which each piece can go wrong. No test provokes a fault: every bad input is
one the host plan rejects or the replay answers with an error response."""
import ctypes as C

import numpy as np
import pytest

import memfs_grow_model as G
import memfs_model as M
import memfs_pread_logged_model as R
import memfs_pwrite_model as P
import memfs_size_model as Z

pytestmark = pytest.mark.gpu

MIN_LOG_BYTES = 2 * 32 * 256 * 64  # Log::new's floor: 16384 entries
GC_FROM_HEAD = 32 * 256
F = 3
PAST = 40  # guard bytes past offs[n]


def _open(nrg, log2_b=12, files=F, **kw):
    cfg = dict(log_bytes=MIN_LOG_BYTES, max_batch=8192, log2_slots=log2_b, queue_capacity=files)
    cfg.update(kw)
    return nrg.DeviceReplica(nrg._lib.NRG_DS_MEMFS, 0, **cfg)


def _ring(nrg, dev, lo, n):
    """records [lo, lo + n) of the log, read from the ring"""
    size = dev.log_state()["size"]
    out = np.zeros(n, nrg.MEMFS_OP_DTYPE)
    one = np.zeros(1, nrg.MEMFS_OP_DTYPE)
    for i in range(n):
        assert dev._lib.nrg_test_ring_read(dev._h, (lo + i) & (size - 1), C.c_void_p(one.ctypes.data)) == 0
        out[i] = one[0]
    return out


def _same_recs(got, want, what=""):
    for f in ("ino", "offset", "op", "len", "data"):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{what} {f}")
    assert got.tobytes() == want.tobytes(), what


def _seed(dev, files, B, seed):
    """Patterned bytes into every file (nrg_memfs_init); returns them as the plain store."""
    store = []
    for f in range(files):
        d = R.pattern(B, seed + f)
        dev.mf_init(M.FIRST_INO + f, d.tobytes())
        store.append(bytearray(d.tobytes()))
    return store


def _state(dev, files):
    return [dev.mf_dump(M.FIRST_INO + f) for f in range(files)], dev.digest()


def _call(nrg, dev, rq, store, what, sizes=None, A=None, device=False, lead=0, ring_last=None):
    """One logged pread checked against the model in every observable; returns the records it logged.
    device: nrg_memfs_pread_logged_async into a tensor that starts `lead` bytes past an aligned address;
    else the synchronous nrg_memfs_pread_logged into a numpy buffer."""
    L = nrg._lib
    files, B = dev.mf_geometry()
    A = A or B
    recs, first, offs, planned, some = R.cut(rq, files, A)
    ws, wp, want = R.pread_at(store, sizes, rq, files, A)
    assert np.array_equal(ws, some) and np.array_equal(wp, planned)
    T, n, total = len(recs), len(rq), int(offs[-1])
    cap = total + PAST
    before, st0 = _state(dev, files), dev.log_state()
    goffs = np.full(n + 1, 7, np.uint64)
    t = C.c_uint64()
    if device:
        import torch

        big = torch.full((cap + 16,), R.GUARD, dtype=torch.uint8, device="cuda")
        d = big[lead:lead + cap]
        d_counts = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        d_some = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        gotoffs, tv = dev.mf_pread_logged_device(rq, 1, d, cap, d_counts, d_some)
        dev.sync()
        data, counts, gs = big.cpu().numpy(), d_counts.cpu().numpy().astype(np.uint64), d_some.cpu().numpy()
        assert (data[:lead] == R.GUARD).all() and (data[lead + cap:] == R.GUARD).all(), what
        data, goffs = data[lead:lead + cap], gotoffs
    else:
        data = np.full(cap, R.GUARD, np.uint8)
        counts = np.full(n, 77, np.uint64)
        gs = np.full(n, 9, np.uint8)
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        L.check(dev._lib.nrg_memfs_pread_logged(dev._h, p(rq), n, 1, p(data), cap, p(counts), p(gs), p(goffs), C.byref(t)),
                what)
        tv = t.value
    assert tv == T, what
    np.testing.assert_array_equal(goffs, offs, err_msg=what + " offs")
    np.testing.assert_array_equal(gs, some, err_msg=what + " some")
    np.testing.assert_array_equal(counts, np.array([len(b) for b in want], np.uint64), err_msg=what + " counts")
    np.testing.assert_array_equal(data, R.expected_data(cap, offs, want), err_msg=what + " data and guard")
    st = dev.log_state()
    assert st["tail"] == st0["tail"] + T and st["ltail"] == st["tail"], what
    k = T if ring_last is None else min(T, ring_last)
    _same_recs(_ring(nrg, dev, st["tail"] - k, k), recs[T - k:], what + " ring")
    assert _state(dev, files) == before, what + ": a read changed the replica"
    return recs


# ---- the edge list ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2_b", [12, 7], ids=["B4096", "B128"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_edge_list_in_one_call(nrg, log2_b, device):
    B = 1 << log2_b
    rq = R.edges(F, B)
    dev = _open(nrg, log2_b)
    store = _seed(dev, F, B, 51)
    recs = _call(nrg, dev, rq, store, "edges", device=device, lead=3)
    assert len(recs) > len(rq) if B > 128 else len(recs) == len(rq)
    # unsized: the same requests through the read-only pread at this point give the same offs, some, bytes
    _, offs, planned, some = R.cut(rq, F, B)[1:]
    data, poffs, psome = dev.mf_pread(rq)
    dev.sync()
    assert poffs.cpu().numpy().astype(np.uint64).tolist() == offs.tolist()
    assert psome.cpu().numpy().tolist() == some.tolist()
    want = R.pread_at(store, None, rq, F, B)[2]
    assert data.cpu().numpy().tobytes() == b"".join(want)
    dev.close()


@pytest.mark.parametrize("log2_b", [12, 7], ids=["B4096", "B128"])
def test_edge_list_one_request_per_call(nrg, log2_b):
    B = 1 << log2_b
    rq = R.edges(F, B)
    dev = _open(nrg, log2_b)
    store = _seed(dev, F, B, 52)
    for i in range(len(rq)):
        _call(nrg, dev, rq[i:i + 1], store, f"request {i}", device=bool(i & 1), lead=i % 8)
    dev.close()


def test_every_destination_alignment_and_many_small_slots(nrg):
    """The destination at every alignment 0..7, slots of 1..19 bytes (several requests in one 8-byte word,
    empty slots between them) beside slots that cross words and lines: the byte-wise arms of mf_rgather."""
    B = 4096
    dev = _open(nrg)
    store = _seed(dev, F, B, 53)
    v = []
    for i in range(90):
        v.append((5 + i % 3, (i * 53) % 4000, i % 20))
        if i % 7 == 0:
            v.append((4, 0, 9))       # an empty slot: no file
            v.append((5, 5000, 9))    # an empty slot: past the end
    v += [(6, 121, 700), (7, 0, 4096)]
    rq = R.reqs(v)
    for lead in range(8):
        _call(nrg, dev, rq, store, f"lead {lead}", device=True, lead=lead, ring_last=64)
    dev.close()


# ---- reads between writes in one log ----------------------------------------------------------------------
def test_reads_between_writes_and_a_second_replica_replays_the_ring(nrg):
    B = 4096
    dev = _open(nrg)
    store = [bytearray(b"\x01" * B) for _ in range(F)]
    data = P.pattern(3000, 54)
    w1 = P.reqs([(5, 100, 1000, 0), (6, 0, 2048, 700)])
    rd = R.reqs([(5, 0, 1300), (6, 0, R.U64), (5, 90, 20)])
    dev.mf_pwrite(w1, data)
    P.pwrite(store, None, w1, data, F, B)
    _call(nrg, dev, rd, store, "after the first write")
    w2 = P.reqs([(5, 600, 500, 2000), (6, 1024, 1024, 1500)])  # over half of each range
    dev.mf_pwrite(w2, data)
    P.pwrite(store, None, w2, data, F, B)
    _call(nrg, dev, rd, store, "after the second write", device=True)
    # a second replica opened on nothing replays the same ring records and ends in the same state
    tail = dev.log_state()["tail"]
    recs = _ring(nrg, dev, 0, tail)
    assert set(np.unique(recs["op"]).tolist()) == {M.WRITE, M.READ}
    two = _open(nrg)
    two.log_append(recs, 1)
    two.log_exec()
    two.sync()
    assert two.digest() == dev.digest() == nrg.digest.memfs([bytes(s) for s in store], None)
    two.close()
    dev.close()


# ---- chunks and passes -------------------------------------------------------------------------------------
def test_a_request_straddles_a_replay_chunk(nrg):
    """max_batch = 64: 50 one-record requests, then a 4096-byte read whose first fragment is record 50 of
    the call, so its 32 fragments cross record 64."""
    B = 4096
    dev = _open(nrg, max_batch=64)
    store = _seed(dev, F, B, 55)
    rq = R.reqs([(5 + i % 3, 128 * (i % 32) + 3, 30) for i in range(50)] + [(6, 0, 4096), (5, 4000, 96)])
    first = R.cut(rq, F, B)[1]
    assert first[50] == 50 and first[51] == 82 and first[-1] == 83
    _call(nrg, dev, rq, store, "chunk")
    _call(nrg, dev, rq, store, "chunk, device", device=True, lead=5)
    dev.close()


def test_passes_wrap_the_smallest_ring(nrg):
    """The smallest legal log: a call whose records exceed what one append may carry goes in several
    passes and wraps the ring; requests split by a pass boundary have the right count and bytes."""
    log2_b = 16
    B = 1 << log2_b
    dev = _open(nrg, log2_b, files=2, max_batch=4096)
    store = _seed(dev, 2, B, 56)
    size = dev.log_state()["size"]
    per_pass = min(size - GC_FROM_HEAD, 4096)
    whole = B // 128
    k = size // whole + 2  # whole-file reads: more records than the ring has entries
    rq = R.reqs([(5, 7, 100)] + [(5 + i % 2, 0, B) for i in range(k)] + [(6, 1, 300)])
    first = R.cut(rq, 2, B)[1]
    T = int(first[-1])
    assert T > size > size - GC_FROM_HEAD and T > 2 * per_pass
    assert any(int(first[i]) < per_pass < int(first[i + 1]) for i in range(len(rq)))  # a request straddles passes
    _call(nrg, dev, rq, store, "passes", device=True, lead=1, ring_last=1000)
    dev.close()


# ---- sized contexts -------------------------------------------------------------------------------------------
def _round(dev, recs):
    import torch

    dev.mf_round(torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).cuda(), len(recs), 1)
    dev.sync()


def test_sized_context_counts_follow_the_size(nrg):
    B = 4096
    dev = _open(nrg)
    dev.mf_enable_sizes()
    g = G.GrowModel(F, 12)
    for f, d in enumerate(_seed(dev, F, B, 57)):
        g.init(M.FIRST_INO + f, bytes(d))
    rq = R.reqs([(5, 0, 4096), (5, 250, 100), (5, 300, 50), (6, 100, R.U64), (7, 0, 129), (5, 383, 2), (4, 0, 5)])
    for size in (333, 384, 0):  # inside a line, on a line edge, 0
        sa = np.concatenate([Z.S(5, size), Z.S(6, size)])
        _round(dev, sa)
        g.replay(sa)
        assert dev.mf_size(5) == size == g.size[0]
        recs = _call(nrg, dev, rq, g.data, f"size {size}", sizes=g.size, device=size == 384, lead=2)
        resp, rs = g.replay(recs)
        _, count, _ = R.fold(rq, R.cut(rq, F, B)[1], resp, rs)
        planned = R.cut(rq, F, B)[3]
        assert count[0] == size < planned[0] and count[4] == 129  # count < planned; file 7 keeps its bytes
    # a bound above B: planned follows the bound, count the size
    dev.set_max_capacity(4 * B)
    g.bound = 4 * B
    rq2 = R.reqs([(7, 4000, 1000), (7, 0, R.U64), (5, 0, 10), (7, 4 * B, 1), (7, 4 * B - 1, 1)])
    planned = R.cut(rq2, F, 4 * B)[3]
    assert planned.tolist() == [1000, 4 * B, 10, 0, 1]
    _call(nrg, dev, rq2, g.data, "bound", sizes=g.size, A=4 * B)
    assert dev.mf_geometry()[1] == B  # Reads grow nothing
    # read to the end after a growing write
    data = P.pattern(3000, 58)
    w = P.reqs([(7, 5000, 3000, 0)])
    dev.mf_pwrite(w, data)
    g.replay(P.cut(w, data, F, 4 * B)[0])
    assert dev.mf_geometry()[1] == 2 * B == g.B and dev.mf_size(7) == 8000
    rq3 = R.reqs([(7, 0, R.U64), (7, 4090, R.U64), (7, 7999, 2), (7, 8000, 1), (5, 0, R.U64)])
    _call(nrg, dev, rq3, g.data, "to the end", sizes=g.size, A=4 * B, device=True)
    assert dev.digest() == g.digest()
    dev.close()


# ---- capacity ------------------------------------------------------------------------------------------------
def test_capacity_is_decided_before_anything_is_logged(nrg):
    import torch

    L = nrg._lib
    B = 4096
    dev = _open(nrg)
    store = _seed(dev, F, B, 59)
    rq = R.reqs([(5, 10, 300), (6, 0, 4096), (7, 4000, 500)])
    offs = R.cut(rq, F, B)[2]
    total = int(offs[-1])
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    d = torch.full((total + 8,), R.GUARD, dtype=torch.uint8, device="cuda")
    d_c = torch.zeros(3, dtype=torch.int64, device="cuda")
    d_s = torch.zeros(3, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st0 = dev.log_state()
    t = C.c_uint64(5)
    goffs = np.zeros(4, np.uint64)
    rc = dev._lib.nrg_memfs_pread_logged_async(dev._h, p(rq), 3, 1, C.c_void_p(d.data_ptr()), total - 1,
                                               C.c_void_p(d_c.data_ptr()), C.c_void_p(d_s.data_ptr()), p(goffs), C.byref(t))
    assert rc == L.NRG_E_CAPACITY and t.value == 0 and goffs.tolist() == offs.tolist()
    dev.sync()
    assert dev.log_state() == st0 and bool((d == R.GUARD).all())
    host = np.full(total, R.GUARD, np.uint8)
    cn, sm = np.zeros(3, np.uint64), np.zeros(3, np.uint8)
    rc = dev._lib.nrg_memfs_pread_logged(dev._h, p(rq), 3, 1, p(host), total - 1, p(cn), p(sm), None, None)
    assert rc == L.NRG_E_CAPACITY and dev.log_state() == st0 and (host == R.GUARD).all()
    rc = dev._lib.nrg_memfs_pread_logged(dev._h, p(rq), 3, 1, p(host), total, p(cn), p(sm), None, C.byref(t))
    assert rc == L.NRG_OK and t.value == 3 + 32 + 1 and cn.tolist() == [300, 4096, 96]
    assert host.tobytes() == R.expected_data(total, offs, R.pread_at(store, None, rq, F, B)[2]).tobytes()
    dev.close()


# ---- the cut alone ----------------------------------------------------------------------------------------------
def test_records_only_equals_the_ring_and_touches_nothing(nrg):
    import torch

    L = nrg._lib
    B = 4096
    dev = _open(nrg)
    store = _seed(dev, F, B, 60)
    rq = R.edges(F, B)
    want = R.cut(rq, F, B)[0]
    T = len(want)
    before, st0 = _state(dev, F), dev.log_state()
    got = dev.mf_pread_logged_records(rq)
    assert got.dtype == nrg.MEMFS_OP_DTYPE
    _same_recs(got, want, "records")
    buf = torch.full((T * 152,), 0xA5, dtype=torch.uint8, device="cuda")
    t = C.c_uint64()
    torch.cuda.synchronize()
    rc = dev._lib.nrg_memfs_pread_logged_records_async(dev._h, C.c_void_p(rq.ctypes.data), len(rq), C.c_void_p(buf.data_ptr()),
                                                       T - 1, C.byref(t))
    assert rc == L.NRG_E_CAPACITY and t.value == T
    dev.sync()
    assert bool((buf == 0xA5).all())
    assert dev.log_state() == st0 and _state(dev, F) == before
    _same_recs(_call(nrg, dev, rq, store, "then logged", device=True), got, "records vs ring")
    dev.close()


# ---- groups -----------------------------------------------------------------------------------------------------
def test_two_member_group_carries_long_reads_in_rank_order(nrg):
    """Round 1: member 0's segment is long writes, member 1's long reads of the same ranges; rank order is
    log order, so member 1 reads member 0's bytes. Round 2, roles swapped: member 0's reads come first and
    do not see member 1's writes of that round."""
    import torch

    L = nrg._lib
    lib = L.load()
    Gn, B = 2, 4096
    cfg = L.default_config(L.NRG_DS_MEMFS)
    cfg.log_bytes, cfg.max_batch, cfg.log2_slots, cfg.queue_capacity = MIN_LOG_BYTES, 512, 12, F
    L.check(lib.nrg_test_loopback_collectives(1))
    g = C.c_void_p()
    try:
        L.check(lib.nrg_group_open((C.c_int * Gn)(0, 0), Gn, C.byref(cfg), C.byref(g)), "nrg_group_open")
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))
    hs = [lib.nrg_group_replica(g, i) for i in range(Gn)]
    data = [P.pattern(4200, 61), P.pattern(4200, 62)]
    writes = P.reqs([(5, 100, 300, 1), (6, 0, 4096, 9), (7, 4000, 96, 0)])
    reads = R.reqs([(5, 90, 320), (6, 0, R.U64), (7, 3990, 200), (9, 0, 4)])
    store = [bytearray(b"\x01" * B) for _ in range(F)]
    rrecs, first, offs, planned, some = R.cut(reads, F, B)
    T, total = len(rrecs), int(offs[-1])
    for rnd, (writer, reader) in enumerate(((0, 1), (1, 0))):
        if writer < reader:  # the writes come first in the log
            P.pwrite(store, None, writes, data[rnd], F, B)
        want = R.pread_at(store, None, reads, F, B)[2]
        if writer > reader:
            P.pwrite(store, None, writes, data[rnd], F, B)
        d_data = torch.from_numpy(np.array(data[rnd])).cuda()
        wrecs = P.cut(writes, data[rnd], F, B)[0]
        d_w = torch.zeros(len(wrecs) * 152, dtype=torch.uint8, device="cuda")
        d_r = torch.zeros(T * 152, dtype=torch.uint8, device="cuda")
        d_resp = torch.zeros(T * 136, dtype=torch.uint8, device="cuda")
        d_rs = torch.zeros(T, dtype=torch.uint8, device="cuda")
        t = C.c_uint64()
        torch.cuda.synchronize()
        L.check(lib.nrg_memfs_pwrite_records_async(hs[writer], C.c_void_p(writes.ctypes.data), len(writes),
                                                   C.c_void_p(d_data.data_ptr()), 4200, C.c_void_p(d_w.data_ptr()), len(wrecs),
                                                   C.byref(t)), "write records")
        L.check(lib.nrg_memfs_pread_logged_records_async(hs[reader], C.c_void_p(reads.ctypes.data), len(reads),
                                                         C.c_void_p(d_r.data_ptr()), T, C.byref(t)), "read records")
        assert t.value == T
        L.check(lib.nrg_sync(hs[0]))
        L.check(lib.nrg_sync(hs[1]))
        _same_recs(d_r.cpu().numpy().view(nrg.MEMFS_OP_DTYPE), rrecs, f"round {rnd} read records")
        rd = (L.Round * Gn)()
        rd[writer].recs, rd[writer].n = d_w.data_ptr(), len(wrecs)
        rd[reader].recs, rd[reader].n = d_r.data_ptr(), T
        rd[reader].resp, rd[reader].some = d_resp.data_ptr(), d_rs.data_ptr()
        L.check(lib.nrg_group_round_async(g, rd, None), "round")
        L.check(lib.nrg_group_sync(g), "sync")
        out = torch.full((total + PAST,), R.GUARD, dtype=torch.uint8, device="cuda")
        d_c = torch.zeros(len(reads), dtype=torch.int64, device="cuda")
        d_s = torch.zeros(len(reads), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        args = (hs[reader], C.c_void_p(reads.ctypes.data), len(reads), C.c_void_p(d_resp.data_ptr()), C.c_void_p(d_rs.data_ptr()))
        tail = (C.c_void_p(out.data_ptr()), total + PAST, C.c_void_p(d_c.data_ptr()), C.c_void_p(d_s.data_ptr()))
        assert lib.nrg_memfs_pread_logged_gather_async(*args, T - 1, *tail) == L.NRG_E_INVAL  # a wrong T
        L.check(lib.nrg_memfs_pread_logged_gather_async(*args, T, *tail), "gather")
        L.check(lib.nrg_sync(hs[reader]))
        assert d_s.cpu().numpy().tolist() == some.tolist()
        assert d_c.cpu().numpy().tolist() == [len(b) for b in want]
        np.testing.assert_array_equal(out.cpu().numpy(), R.expected_data(total + PAST, offs, want), err_msg=f"round {rnd}")
    same = C.c_int(-1)
    rows = np.zeros((Gn, 3), np.uint64)
    assert lib.nrg_group_verify(g, rows.ctypes.data_as(C.c_void_p), C.byref(same)) == L.NRG_OK
    assert same.value == 1
    assert [tuple(int(x) for x in row) for row in rows] == [nrg.digest.memfs([bytes(s) for s in store])] * Gn
    assert lib.nrg_group_close(g) == L.NRG_OK


def test_a_file_partitioned_round_carries_a_long_read_to_the_owner_and_back(nrg):
    import torch
    from nrgpu.parallel import ReplicaGroup

    L = nrg._lib
    lib = L.load()
    B = 4096
    rep = _open(nrg, max_batch=512)
    store = _seed(rep, F, B, 63)
    rq = R.reqs([(6, 100, 3000), (4, 0, 5), (7, 0, R.U64)])
    recs, first, offs, planned, some = R.cut(rq, F, B)
    T, total = len(recs), int(offs[-1])
    L.check(lib.nrg_test_loopback_collectives(1))
    try:
        grp = nrg.FilePartitionedGroup(rep, 0, 1, uid=ReplicaGroup.unique_id(), timeout_ms=20000)
        try:
            d_recs = rep.mf_pread_logged_records(rq, device=True)
            d_resp = torch.zeros(T * 136, dtype=torch.uint8, device="cuda")
            d_rs = torch.zeros(T, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            grp.round(d_recs, T, d_resp, d_rs)
            grp.sync()
            out = torch.full((total + PAST,), R.GUARD, dtype=torch.uint8, device="cuda")
            d_c = torch.zeros(len(rq), dtype=torch.int64, device="cuda")
            d_s = torch.zeros(len(rq), dtype=torch.uint8, device="cuda")
            rep.mf_pread_logged_gather_device(rq, d_resp, d_rs, T, out, total + PAST, d_c, d_s)
            rep.sync()
            want = R.pread_at(store, None, rq, F, B)[2]
            assert d_s.cpu().numpy().tolist() == some.tolist() and d_c.cpu().numpy().tolist() == [len(b) for b in want]
            np.testing.assert_array_equal(out.cpu().numpy(), R.expected_data(total + PAST, offs, want))
        finally:
            grp.close()
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))
        rep.close()


# ---- guards -----------------------------------------------------------------------------------------------------
def test_guards(nrg):
    import torch

    L = nrg._lib
    lib = L.load()
    rq = R.reqs([(5, 0, 10)])
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    d_recs = torch.zeros(152 * 4, dtype=torch.uint8, device="cuda")
    d_resp = torch.zeros(136 * 4 + 8, dtype=torch.uint8, device="cuda")
    d_c = torch.zeros(5, dtype=torch.int64, device="cuda")
    d_s = torch.zeros(4, dtype=torch.uint8, device="cuda")
    host = np.zeros(64, np.uint8)
    cn, sm = np.zeros(4, np.uint64), np.zeros(4, np.uint8)
    torch.cuda.synchronize()
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    dp = lambda t, o=0: C.c_void_p(t.data_ptr() + o)  # noqa: E731
    t = C.c_uint64()
    INV, CAPY, OK = L.NRG_E_INVAL, L.NRG_E_CAPACITY, L.NRG_OK
    hm = nrg.DeviceReplica(L.NRG_DS_HASHMAP, 0, log2_slots=10, max_batch=64)
    assert lib.nrg_memfs_pread_logged_async(hm._h, p(rq), 1, 1, dp(d), 64, dp(d_c), dp(d_s), None, None) == INV
    assert lib.nrg_memfs_pread_logged(hm._h, p(rq), 1, 1, p(host), 64, p(cn), p(sm), None, None) == INV
    assert lib.nrg_memfs_pread_logged_records_async(hm._h, p(rq), 1, dp(d_recs), 4, None) == INV
    assert lib.nrg_memfs_pread_logged_gather_async(hm._h, p(rq), 1, dp(d_resp), dp(d_s), 1, dp(d), 64, dp(d_c), dp(d_s)) == INV
    hm.close()
    dev = _open(nrg, max_batch=64)
    st0 = dev.log_state()
    # NULL and misaligned pointers; exactly one of d_counts / d_some
    assert lib.nrg_memfs_pread_logged_async(dev._h, None, 1, 1, dp(d), 64, dp(d_c), dp(d_s), None, None) == INV
    assert lib.nrg_memfs_pread_logged_async(dev._h, p(rq), 1, 1, None, 64, dp(d_c), dp(d_s), None, None) == INV
    assert lib.nrg_memfs_pread_logged_async(dev._h, p(rq), 1, 1, dp(d), 64, dp(d_c), None, None, None) == INV
    assert lib.nrg_memfs_pread_logged_async(dev._h, p(rq), 1, 1, dp(d), 64, None, dp(d_s), None, None) == INV
    assert lib.nrg_memfs_pread_logged_async(dev._h, p(rq), 1, 1, dp(d), 64, dp(d_c, 4), dp(d_s), None, None) == INV
    assert lib.nrg_memfs_pread_logged(dev._h, p(rq), 1, 1, None, 64, p(cn), p(sm), None, None) == INV
    assert lib.nrg_memfs_pread_logged(dev._h, p(rq), 1, 1, p(host), 64, p(cn), None, None, None) == INV
    assert lib.nrg_memfs_pread_logged_records_async(dev._h, p(rq), 1, dp(d_recs, 4), 4, None) == INV
    assert lib.nrg_memfs_pread_logged_records_async(dev._h, p(rq), 1, None, 4, None) == INV
    assert lib.nrg_memfs_pread_logged_gather_async(dev._h, p(rq), 1, None, dp(d_s), 1, dp(d), 64, dp(d_c), dp(d_s)) == INV
    assert lib.nrg_memfs_pread_logged_gather_async(dev._h, p(rq), 1, dp(d_resp), None, 1, dp(d), 64, dp(d_c), dp(d_s)) == INV
    assert lib.nrg_memfs_pread_logged_gather_async(dev._h, p(rq), 1, dp(d_resp, 4), dp(d_s), 1, dp(d), 64, dp(d_c), dp(d_s)) == INV
    # the gather with a wrong T, and with too little room
    assert lib.nrg_memfs_pread_logged_gather_async(dev._h, p(rq), 1, dp(d_resp), dp(d_s), 2, dp(d), 64, dp(d_c), dp(d_s)) == INV
    assert lib.nrg_memfs_pread_logged_gather_async(dev._h, p(rq), 1, dp(d_resp), dp(d_s), 1, dp(d), 9, dp(d_c), dp(d_s)) == CAPY
    # n > max_batch: the uploads are sized at open
    many = R.reqs([(5, 0, 1)] * 65)
    assert lib.nrg_memfs_pread_logged_async(dev._h, p(many), 65, 1, dp(d), 64, None, None, None, None) == CAPY
    assert lib.nrg_memfs_pread_logged(dev._h, p(many), 65, 1, p(host), 64, None, None, None, None) == CAPY
    assert lib.nrg_memfs_pread_logged_records_async(dev._h, p(many), 65, dp(d_recs), 4, None) == CAPY
    assert lib.nrg_memfs_pread_logged_gather_async(dev._h, p(many), 65, dp(d_resp), dp(d_s), 65, dp(d), 64, None, None) == CAPY
    assert dev.log_state() == st0
    # n == 0 is NRG_OK and logs nothing
    t.value = 7
    o = np.full(1, 9, np.uint64)
    assert lib.nrg_memfs_pread_logged_async(dev._h, None, 0, 1, None, 0, None, None, p(o), C.byref(t)) == OK
    assert t.value == 0 and o[0] == 0
    assert lib.nrg_memfs_pread_logged(dev._h, None, 0, 1, None, 0, None, None, None, None) == OK
    assert lib.nrg_memfs_pread_logged_records_async(dev._h, None, 0, None, 0, C.byref(t)) == OK and t.value == 0
    assert lib.nrg_memfs_pread_logged_gather_async(dev._h, None, 0, None, None, 0, None, 0, None, None) == OK
    data, offs, counts, some = dev.mf_pread_logged(np.zeros(0, nrg.MEMFS_RD_DTYPE))
    assert len(data) == 0 and offs.tolist() == [0] and len(counts) == 0 and len(some) == 0
    assert dev.log_state() == st0 and dev.mf_dump(5) == b"\x01" * 4096
    # requests of no bytes need no data at all, and counts / some may both be left out
    assert lib.nrg_memfs_pread_logged_async(dev._h, p(R.reqs([(5, 9, 0), (4, 0, 5)])), 2, 1, None, 0, None, None, None,
                                            C.byref(t)) == OK and t.value == 2
    dev.sync()
    assert dev.log_state()["tail"] == st0["tail"] + 2
    # a single MfRead of more than 128 bytes still answers EINVAL
    resp = torch.zeros(136, dtype=torch.uint8, device="cuda")
    rs = torch.zeros(1, dtype=torch.uint8, device="cuda")
    one = M.R(5, 0, 129)
    dev.mf_round(torch.from_numpy(one.view(np.uint8).reshape(-1).copy()).cuda(), 1, 1, resp, rs)
    assert lib.nrg_sync(dev._h) in (OK, INV)
    assert int(rs.cpu()[0]) == 0 and int(resp.cpu().numpy().view(nrg.MEMFS_RESP_DTYPE)["n"][0]) == L.NRG_MEMFS_EINVAL
    dev.close()


# ---- nrgpu.MfPreadLogged through two replicas on one Log ---------------------------------------------------
def test_python_replicas_carry_mfpreadlogged(nrg):
    L = nrg._lib
    log = nrg.Log(MIN_LOG_BYTES)
    a = nrg.Replica(log, nrg.MemFs, log2_slots=12, queue_capacity=F, max_batch=256)
    b = nrg.Replica(log, nrg.MemFs, log2_slots=12, queue_capacity=F, max_batch=256)
    ta, tb = a.register(), b.register()
    body = bytes(P.pattern(1000, 64))
    assert a.execute_mut(nrg.MfPwrite(5, 100, body), ta) == ("written", 1000)
    whole = b"\x01" * 100 + body + b"\x01" * (4096 - 1100)
    assert b.execute_mut(nrg.MfPreadLogged(5, 0, 4096), tb) == ("data", whole)
    assert a.execute_mut(nrg.MfPreadLogged(5, 90, 300), ta) == ("data", whole[90:390])
    assert a.execute_mut(nrg.MfPreadLogged(4, 0, 300), ta) == ("err", L.NRG_MEMFS_ENOENT)
    assert b.execute_mut(nrg.MfPreadLogged(5, 4000, 2 ** 64 - 1), tb) == ("data", whole[4000:])
    assert b.execute_mut(nrg.MfPreadLogged(5, 4096, 10), tb) == ("data", b"")
    out = b.execute_mut_batch([nrg.MfPreadLogged(5, 0, 200), nrg.MfPwrite(5, 50, b"z" * 100), nrg.MfPreadLogged(5, 0, 200),
                               nrg.MfRead(5, 98, 4)], tb)
    after = whole[:50] + b"z" * 100 + whole[150:]
    assert out == [("data", whole[:200]), ("written", 100), ("data", after[:200]), ("data", b"zzzz")]
    # MfRead stays the single-record op: more than 128 bytes is EINVAL
    assert a.execute_mut(nrg.MfRead(5, 0, 129), ta) == ("err", L.NRG_MEMFS_EINVAL)
    with pytest.raises(TypeError):
        a.execute(nrg.MfPreadLogged(5, 0, 10), ta)
    b.sync(tb)
    assert a.digest() == b.digest()
    a.dev.close()
    b.dev.close()


def test_python_replica_ops_of_many_records(nrg):
    """One op of far more records than MAX_PENDING_OPS works; an op that alone exceeds one append raises
    ValueError before anything is enqueued."""
    log = nrg.Log(MIN_LOG_BYTES)
    a = nrg.Replica(log, nrg.MemFs, log2_slots=21, queue_capacity=1, max_batch=4096)
    t = a.register()
    lim = log.size - GC_FROM_HEAD
    with pytest.raises(ValueError):
        a.execute_mut(nrg.MfPreadLogged(5, 0, lim * 128 + 1), t)
    assert a.dev.log_state()["tail"] == 0
    body = bytes(P.pattern(70000, 65))
    assert a.execute_mut(nrg.MfPwrite(5, 1000, body), t) == ("written", 70000)
    tail = a.dev.log_state()["tail"]
    assert a.execute_mut(nrg.MfPreadLogged(5, 990, 70020), t) == ("data", b"\x01" * 10 + body + b"\x01" * 10)
    assert a.dev.log_state()["tail"] == tail + 548  # far more records than MAX_PENDING_OPS
    a.dev.close()
