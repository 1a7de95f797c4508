"""The file store's logged writes of any length (nrg_memfs_pwrite*, csrc/memfs.hip mf_frag) against
the model of tests/memfs_pwrite_model.py: the answers, the record count, the log's tail, every ring
record byte for byte (zero tails included), every file against whole-request pwrite on byte arrays and
the digest; the equivalence with the model's records fed through nrg_memfs_round_async; writes that
straddle replay chunks and passes of a wrapping ring; sized contexts; the cut alone
(nrg_memfs_pwrite_records_async) and a two-member group that carries it; the guards; and nrgpu.MfPwrite
through two replicas on one Log.

Shapes are the smallest at which each piece can go wrong. No test provokes a fault: every bad input is
one the host plan rejects or the replay answers with an error response."""
import ctypes as C

import numpy as np
import pytest

import memfs_model as M
import memfs_pwrite_model as P
import memfs_size_model as Z

pytestmark = pytest.mark.gpu

MIN_LOG_BYTES = 2 * 32 * 256 * 64  # Log::new's floor: 16384 entries
GC_FROM_HEAD = 32 * 256
DATA_BYTES = 4096 + 104
F = 3


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


def _same_files(nrg, dev, store, what="", sizes=None):
    for f in range(len(store)):
        want = bytes(store[f]) if sizes is None else bytes(store[f][: sizes[f]])
        assert dev.mf_dump(M.FIRST_INO + f) == want, f"{what} file {f}"
    assert dev.digest() == nrg.digest.memfs([bytes(s) for s in store], sizes), what


def _call(nrg, dev, rq, data, store, what, sizes=None, device_data=False):
    """One mf_pwrite checked against the model in every observable: returns the records it logged."""
    files, B = dev.mf_geometry()
    recs, first, written, some = P.cut(rq, data, files, B)
    st0 = dev.log_state()
    if device_data:
        import torch

        w, s, t = dev.mf_pwrite(rq, torch.from_numpy(np.array(data)).cuda(), origin=1)
        dev.sync()
        w, s = w.cpu().numpy().astype(np.uint64), s.cpu().numpy()
    else:
        w, s, t = dev.mf_pwrite(rq, data, origin=1)
    np.testing.assert_array_equal(w, written, err_msg=what + " written")
    np.testing.assert_array_equal(s, some, err_msg=what + " some")
    assert t == int(first[-1]) == len(recs), what
    st = dev.log_state()
    assert st["tail"] == st0["tail"] + t and st["ltail"] == st["tail"], what
    _same_recs(_ring(nrg, dev, st0["tail"], t), recs, what + " ring")
    P.pwrite(store, sizes, rq, data, files, B)
    _same_files(nrg, dev, store, what, sizes)
    return recs


# ---- the edge list: one call, one request per call, and the same records through a plain round ---------
@pytest.mark.parametrize("log2_b", [12, 7], ids=["B4096", "B128"])
@pytest.mark.parametrize("device_data", [False, True], ids=["host_data", "device_data"])
def test_edge_list_in_one_call(nrg, log2_b, device_data):
    B = 1 << log2_b
    rq = P.edges(F, B, DATA_BYTES)
    data = P.pattern(DATA_BYTES, 11)
    dev = _open(nrg, log2_b)
    store = [bytearray(b"\x01" * B) for _ in range(F)]
    recs = _call(nrg, dev, rq, data, store, "edges", device_data=device_data)
    assert any(not s for s in P.cut(rq, data, F, B)[3]) and (len(recs) > len(rq) if B > 128 else len(recs) == len(rq))
    # equivalence: a second context fed the model's records through nrg_memfs_round_async
    import torch

    ref = _open(nrg, log2_b)
    ref.mf_round(torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).cuda(), len(recs), 1)
    ref.sync()
    assert ref.digest() == dev.digest()
    for f in range(F):
        assert ref.mf_dump(M.FIRST_INO + f) == dev.mf_dump(M.FIRST_INO + f)
    ref.close()
    dev.close()


@pytest.mark.parametrize("log2_b", [12, 7], ids=["B4096", "B128"])
def test_edge_list_one_request_per_call(nrg, log2_b):
    B = 1 << log2_b
    rq = P.edges(F, B, DATA_BYTES)
    data = P.pattern(DATA_BYTES, 12)
    dev = _open(nrg, log2_b)
    store = [bytearray(b"\x01" * B) for _ in range(F)]
    for i in range(len(rq)):
        _call(nrg, dev, rq[i:i + 1], data, store, f"request {i}")
    dev.close()


def test_unaligned_device_data_and_every_source_shift(nrg):
    """The source pointer itself at every alignment 0..15 (a view into a larger tensor), with requests
    whose bytes start at the head of data and end on its last byte: the byte-wise arms of mf_frag."""
    import torch

    B = 4096
    dev = _open(nrg)
    store = [bytearray(b"\x01" * B) for _ in range(F)]
    big = torch.from_numpy(P.pattern(1024 + 64, 13)).cuda()
    for lead in range(16):
        nb = 700 + lead
        d = big[lead:lead + nb]
        host = d.cpu().numpy()
        rq = P.reqs([(5, 3 + lead, 300, 0), (6, 128, nb - 100, 100), (7, 4096 - 45, 45, nb - 45), (5, 1000, 1, nb - 1)])
        recs, first, written, some = P.cut(rq, host, F, B)
        tail = dev.log_state()["tail"]
        w, s, t = dev.mf_pwrite(rq, d)
        dev.sync()
        assert t == len(recs) and s.cpu().numpy().tolist() == [1, 1, 1, 1]
        _same_recs(_ring(nrg, dev, tail, t), recs, f"lead {lead}")
        P.pwrite(store, None, rq, host, F, B)
    _same_files(nrg, dev, store, "leads")
    dev.close()


# ---- chunks and passes ---------------------------------------------------------------------------------
def test_a_request_straddles_a_replay_chunk(nrg):
    """max_batch = 64: 50 one-record requests, then a 4096-byte request whose first fragment is record
    50 of the call, so its 32 fragments lie in two replay chunks."""
    B = 4096
    dev = _open(nrg, max_batch=64)
    data = P.pattern(DATA_BYTES, 14)
    rq = P.reqs([(5 + i % 3, 128 * (i % 32) + 3, 30, i) for i in range(50)] + [(6, 0, 4096, 17), (5, 4000, 96, 1)])
    recs, first, _, _ = P.cut(rq, data, F, B)
    assert first[50] == 50 and first[51] == 82 and len(recs) == 83
    store = [bytearray(b"\x01" * B) for _ in range(F)]
    _call(nrg, dev, rq, data, store, "chunk")
    dev.close()


def test_passes_wrap_the_smallest_ring(nrg):
    """The smallest legal log: a call whose records exceed what one append may carry (the ring's
    entries less GC_FROM_HEAD, read from nrg_log_state) goes in several passes and wraps the ring; a
    request's fragments straddle the passes and stay contiguous."""
    log2_b = 16
    B = 1 << log2_b
    dev = _open(nrg, log2_b, files=2, max_batch=4096)
    size = dev.log_state()["size"]
    per_pass = size - GC_FROM_HEAD
    whole = B // 128
    k = size // whole + 2  # whole-file writes: more records than the ring has entries
    data = P.pattern(B + 64, 15)
    rq = P.reqs([(5, 7, 100, 3)] + [(5 + i % 2, 0, B, i) for i in range(k)] + [(6, 1, 300, 9)])
    recs, first, written, some = P.cut(rq, data, 2, B)
    T = len(recs)
    assert T > size > per_pass and T > 2 * per_pass  # three passes, and the ring wraps
    assert any(int(first[i]) < per_pass < int(first[i + 1]) for i in range(len(rq)))  # a request straddles the passes
    st0 = dev.log_state()
    w, s, t = dev.mf_pwrite(rq, data)
    assert t == T and np.array_equal(w, written) and np.array_equal(s, some)
    st = dev.log_state()
    assert st["tail"] == st0["tail"] + T and st["ltail"] == st["tail"]
    # the ring holds the last `size` records of the log at most: read the newest thousand
    _same_recs(_ring(nrg, dev, st["tail"] - 1000, 1000), recs[-1000:], "ring tail")
    store = [bytearray(b"\x01" * B) for _ in range(2)]
    P.pwrite(store, None, rq, data, 2, B)
    _same_files(nrg, dev, store, "passes")
    dev.close()


# ---- sized contexts -------------------------------------------------------------------------------------
def test_sized_context_grows_and_a_gap_reads_as_zero(nrg):
    B = 4096
    dev = _open(nrg)
    dev.mf_enable_sizes()
    z = Z.SizedModel(F, 12)
    store = [bytearray(b"\x01" * B) for _ in range(F)]
    sizes = [B] * F
    dev.mf_truncate(5, 10)
    z.truncate(5, 10)
    store[0][10:] = bytes(B - 10)
    sizes[0] = 10
    data = P.pattern(DATA_BYTES, 16)
    rq = P.reqs([(5, 200, 300, 33)])
    recs = _call(nrg, dev, rq, data, store, "grow", sizes)
    z.replay(recs)
    assert dev.mf_size(5) == 500 == sizes[0] == z.size[0]
    got = dev.mf_dump(5)
    assert len(got) == 500 and got[10:200] == bytes(190) and got[:10] == b"\x01" * 10
    assert got[200:] == bytes(data[33:333]) and got == z.dump(5)
    # an MfSetAttr between two pwrites, as the sized model says
    import torch

    sa = Z.S(5, 260)
    dev.mf_round(torch.from_numpy(sa.view(np.uint8).reshape(-1).copy()).cuda(), 1, 1)
    dev.sync()
    z.replay(sa)
    store[0][260:] = bytes(B - 260)
    sizes[0] = 260
    rq2 = P.reqs([(5, 250, 5, 0), (5, 700, 200, 7), (6, 4000, 96, 9), (5, 4090, 7, 0)])
    recs2 = _call(nrg, dev, rq2, data, store, "after setattr", sizes)
    z.replay(recs2)
    assert [dev.mf_size(5 + f) for f in range(F)] == sizes == z.size == [900, B, B]
    assert dev.digest() == z.digest()
    for f in range(F):
        assert dev.mf_dump(5 + f) == z.dump(5 + f)
    dev.close()


# ---- the cut alone ----------------------------------------------------------------------------------------
def test_records_only_equals_the_ring_and_touches_nothing(nrg):
    import torch

    B = 4096
    L = nrg._lib
    dev = _open(nrg)
    rq = P.edges(F, B, DATA_BYTES)
    data = P.pattern(DATA_BYTES, 17)
    want = P.cut(rq, data, F, B)[0]
    T = len(want)
    st0, dg0 = dev.log_state(), dev.digest()
    got = dev.mf_pwrite_records(rq, data)
    assert got.dtype == nrg.MEMFS_OP_DTYPE
    _same_recs(got, want, "records")
    # cap = T - 1: NRG_E_CAPACITY, n_records = T, and the prefilled buffer untouched
    d_data = torch.from_numpy(np.array(data)).cuda()
    buf = torch.full((T * 152,), 0xA5, dtype=torch.uint8, device="cuda")
    t = C.c_uint64()
    torch.cuda.synchronize()
    rc = dev._lib.nrg_memfs_pwrite_records_async(dev._h, C.c_void_p(rq.ctypes.data), len(rq), C.c_void_p(d_data.data_ptr()),
                                                 DATA_BYTES, C.c_void_p(buf.data_ptr()), T - 1, C.byref(t))
    assert rc == L.NRG_E_CAPACITY and t.value == T
    dev.sync()
    assert bool((buf == 0xA5).all())
    assert dev.log_state() == st0 and dev.digest() == dg0
    for f in range(F):
        assert dev.mf_dump(5 + f) == b"\x01" * B
    # the same call then logs exactly these records
    store = [bytearray(b"\x01" * B) for _ in range(F)]
    _same_recs(_call(nrg, dev, rq, data, store, "then logged"), got, "records vs ring")
    dev.close()


def test_two_member_group_carries_long_writes(nrg):
    """A two-member loopback group whose segments come from nrg_memfs_pwrite_records_async with different
    writes: both members replay W_0 || W_1, nrg_group_verify says identical, the dumps are the model's."""
    import torch

    L = nrg._lib
    lib = L.load()
    G, B = 2, 4096
    cfg = L.default_config(L.NRG_DS_MEMFS)
    cfg.log_bytes, cfg.max_batch, cfg.log2_slots, cfg.queue_capacity = MIN_LOG_BYTES, 512, 12, F
    L.check(lib.nrg_test_loopback_collectives(1))
    g = C.c_void_p()
    try:
        L.check(lib.nrg_group_open((C.c_int * G)(0, 0), G, C.byref(cfg), C.byref(g)), "nrg_group_open")
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))
    data = P.pattern(DATA_BYTES, 18)
    d_data = torch.from_numpy(np.array(data)).cuda()
    writes = [P.reqs([(5, 100, 300, 1), (6, 0, 4096, 9), (7, 4000, 97, 0), (5, 350, 10, 77)]),
              P.reqs([(5, 380, 700, 40), (9, 0, 5, 0), (7, 1, 127, 3), (6, 2048, 1000, 2000)])]
    store = [bytearray(b"\x01" * B) for _ in range(F)]
    rd = (L.Round * G)()
    keep = []
    for i in range(G):
        h = lib.nrg_group_replica(g, i)
        want = P.cut(writes[i], data, F, B)[0]
        T = len(want)
        d_recs = torch.zeros(T * 152, dtype=torch.uint8, device="cuda")
        t = C.c_uint64()
        torch.cuda.synchronize()
        L.check(lib.nrg_memfs_pwrite_records_async(h, C.c_void_p(writes[i].ctypes.data), len(writes[i]),
                                                   C.c_void_p(d_data.data_ptr()), DATA_BYTES, C.c_void_p(d_recs.data_ptr()),
                                                   T, C.byref(t)), "records")
        L.check(lib.nrg_sync(h))
        assert t.value == T
        _same_recs(d_recs.cpu().numpy().view(nrg.MEMFS_OP_DTYPE), want, f"member {i}")
        rd[i].recs, rd[i].n = d_recs.data_ptr(), T
        keep.append(d_recs)
        P.pwrite(store, None, writes[i], data, F, B)  # in rank order: W_0 || W_1
    L.check(lib.nrg_group_round_async(g, rd, None), "round")
    L.check(lib.nrg_group_sync(g), "sync")
    same = C.c_int(-1)
    out = np.zeros((G, 3), np.uint64)
    assert lib.nrg_group_verify(g, out.ctypes.data_as(C.c_void_p), C.byref(same)) == L.NRG_OK
    assert same.value == 1
    assert [tuple(int(x) for x in row) for row in out] == [nrg.digest.memfs([bytes(s) for s in store])] * G
    buf = np.zeros(B, np.uint8)
    n = C.c_uint64()
    for i in range(G):
        h = lib.nrg_group_replica(g, i)
        for f in range(F):
            assert lib.nrg_memfs_dump(h, 5 + f, C.c_void_p(buf.ctypes.data), B, C.byref(n)) == L.NRG_OK
            assert buf.tobytes() == bytes(store[f]), f"member {i} file {f}"
    assert lib.nrg_group_close(g) == L.NRG_OK


# ---- guards ---------------------------------------------------------------------------------------------
def test_guards(nrg):
    import torch

    L = nrg._lib
    lib = L.load()
    rq = P.reqs([(5, 0, 10, 0)])
    data = P.pattern(64, 19)
    d_data = torch.from_numpy(np.array(data)).cuda()
    d_recs = torch.zeros(152 * 4, dtype=torch.uint8, device="cuda")
    d_w = torch.zeros(4, dtype=torch.int64, device="cuda")
    d_s = torch.zeros(4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    dp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    t = C.c_uint64()
    hm = nrg.DeviceReplica(L.NRG_DS_HASHMAP, 0, log2_slots=10, max_batch=64)
    assert lib.nrg_memfs_pwrite_async(hm._h, p(rq), 1, dp(d_data), 64, 1, None, None, None) == L.NRG_E_INVAL
    assert lib.nrg_memfs_pwrite(hm._h, p(rq), 1, p(data), 64, 1, None, None, None) == L.NRG_E_INVAL
    assert lib.nrg_memfs_pwrite_records_async(hm._h, p(rq), 1, dp(d_data), 64, dp(d_recs), 4, None) == L.NRG_E_INVAL
    hm.close()
    dev = _open(nrg, max_batch=64)
    st0 = dev.log_state()
    # a valid request whose bytes are not inside data: the whole call is refused, nothing is logged
    bad = P.reqs([(5, 0, 10, 0), (5, 100, 10, 60)])
    assert lib.nrg_memfs_pwrite_async(dev._h, p(bad), 2, dp(d_data), 64, 1, None, None, C.byref(t)) == L.NRG_E_INVAL
    assert lib.nrg_memfs_pwrite(dev._h, p(bad), 2, p(data), 64, 1, None, None, None) == L.NRG_E_INVAL
    assert lib.nrg_memfs_pwrite_records_async(dev._h, p(bad), 2, dp(d_data), 64, dp(d_recs), 4, None) == L.NRG_E_INVAL
    # pointers
    assert lib.nrg_memfs_pwrite_async(dev._h, None, 1, dp(d_data), 64, 1, None, None, None) == L.NRG_E_INVAL
    assert lib.nrg_memfs_pwrite_async(dev._h, p(rq), 1, None, 64, 1, None, None, None) == L.NRG_E_INVAL
    assert lib.nrg_memfs_pwrite_async(dev._h, p(rq), 1, dp(d_data), 64, 1, dp(d_w), None, None) == L.NRG_E_INVAL
    assert lib.nrg_memfs_pwrite_async(dev._h, p(rq), 1, dp(d_data), 64, 1, None, dp(d_s), None) == L.NRG_E_INVAL
    # n > max_batch: the uploads are sized at open
    many = P.reqs([(5, 0, 1, 0)] * 65)
    assert lib.nrg_memfs_pwrite_async(dev._h, p(many), 65, dp(d_data), 64, 1, None, None, None) == L.NRG_E_CAPACITY
    assert lib.nrg_memfs_pwrite(dev._h, p(many), 65, p(data), 64, 1, None, None, None) == L.NRG_E_CAPACITY
    assert lib.nrg_memfs_pwrite_records_async(dev._h, p(many), 65, dp(d_data), 64, dp(d_recs), 4, None) == L.NRG_E_CAPACITY
    assert dev.log_state() == st0
    # n == 0 is NRG_OK and logs nothing
    t.value = 7
    assert lib.nrg_memfs_pwrite_async(dev._h, None, 0, None, 0, 1, None, None, C.byref(t)) == L.NRG_OK and t.value == 0
    assert lib.nrg_memfs_pwrite(dev._h, None, 0, None, 0, 1, None, None, None) == L.NRG_OK
    assert lib.nrg_memfs_pwrite_records_async(dev._h, None, 0, None, 0, None, 0, C.byref(t)) == L.NRG_OK and t.value == 0
    w, s, n = dev.mf_pwrite(np.zeros(0, nrg.MEMFS_WR_DTYPE), b"")
    assert len(w) == 0 and len(s) == 0 and n == 0
    assert dev.log_state() == st0 and dev.mf_dump(5) == b"\x01" * 4096
    # a request of no bytes needs no data at all
    w, s, n = dev.mf_pwrite(P.reqs([(5, 9, 0, 0), (4, 0, 5, 0)]), b"")
    assert w.tolist() == [0, L.NRG_MEMFS_ENOENT] and s.tolist() == [1, 0] and n == 2
    assert dev.log_state()["tail"] == st0["tail"] + 2
    dev.close()


# ---- nrgpu.MfPwrite through two replicas on one Log -----------------------------------------------------
def test_python_replicas_carry_mfpwrite(nrg):
    L = nrg._lib
    log = nrg.Log(MIN_LOG_BYTES)
    a = nrg.Replica(log, nrg.MemFs, log2_slots=12, queue_capacity=F, max_batch=256)
    b = nrg.Replica(log, nrg.MemFs, log2_slots=12, queue_capacity=F, max_batch=256)
    ta, tb = a.register(), b.register()
    body = bytes(P.pattern(300, 20))
    assert a.execute_mut(nrg.MfPwrite(5, 100, body), ta) == ("written", 300)
    got = b.execute(nrg.MfPread(5, 0, 4096), tb)
    assert got == ("data", b"\x01" * 100 + body + b"\x01" * (4096 - 400))
    assert a.execute_mut(nrg.MfPwrite(5, 4000, body), ta) == ("err", L.NRG_MEMFS_EFBIG)
    assert a.execute_mut(nrg.MfPwrite(4, 0, body), ta) == ("err", L.NRG_MEMFS_ENOENT)
    assert a.execute_mut(nrg.MfPwrite(6, 7, b""), ta) == ("written", 0)
    whole = bytes(P.pattern(4096, 21))
    out = b.execute_mut_batch([nrg.MfRead(5, 98, 4), nrg.MfPwrite(7, 0, whole), nrg.MfWrite(6, 0, b"ab"), nrg.MfGetAttr(7)], tb)
    assert out == [("data", b"\x01\x01" + body[:2]), ("written", 4096), ("written", 2), ("attr", 4096)]
    assert a.execute(nrg.MfPread(7, 0, 4096), ta) == ("data", whole)
    # an MfWrite of more than 128 bytes still answers EINVAL, and the replica that replays it later is not failed
    assert a.execute_mut(nrg.MfWrite(5, 0, b"x" * 129), ta) == ("err", L.NRG_MEMFS_EINVAL)
    assert b.execute(nrg.MfPread(5, 0, 4), tb) == ("data", b"\x01" * 4)
    b.sync(tb)
    assert a.digest() == b.digest()
    a.dev.close()
    b.dev.close()


def test_python_replica_ops_of_many_records(nrg):
    """One op of far more records than MAX_PENDING_OPS works; a batch of more records than one append
    carries goes in several appends, split between ops; an op that alone exceeds one append raises
    ValueError before anything is enqueued."""
    log = nrg.Log(MIN_LOG_BYTES)
    a = nrg.Replica(log, nrg.MemFs, log2_slots=21, queue_capacity=1, max_batch=4096)
    t = a.register()
    lim = log.size - GC_FROM_HEAD
    body = bytes(P.pattern(lim * 128, 22))
    with pytest.raises(ValueError):
        a.execute_mut(nrg.MfPwrite(5, 0, body + b"x"), t)
    assert a.dev.log_state()["tail"] == 0
    out = a.execute_mut_batch([nrg.MfPwrite(5, 0, body), nrg.MfPwrite(5, lim * 128 - 5, body[:70000])], t)
    assert out == [("written", lim * 128), ("written", 70000)]
    assert a.dev.log_state()["tail"] == lim + 548
    want = body[:lim * 128 - 5] + body[:70000]
    assert a.execute(nrg.MfPread(5, 0, len(want) + 1), t) == ("data", want + b"\x01")
    a.dev.close()
