"""The replicated file store (kind NRG_DS_MEMFS, csrc/memfs.hip) bit-exact against the sequential
model of tests/memfs_model.py: every response field (the zero tail of data included), every some,
the final dump of every file and the digest; then the round plumbing (chunks, response windows,
fused rounds, a wrapping log), the lifecycle (init, read, snapshot / restore, kind guards) and a
two-member replicated group on the loopback collectives.

Shapes are the smallest at which each piece can go wrong; tests/test_memfs_cpu.py checks on the CPU
that every named stream reaches the arm it is named for."""
import ctypes as C

import numpy as np
import pytest

import memfs_model as M

pytestmark = pytest.mark.gpu

MIN_LOG_BYTES = 2 * 32 * 256 * 64  # Log::new's floor: 16384 entries


def _open(nrg, s, **kw):
    cfg = dict(log_bytes=MIN_LOG_BYTES, max_batch=s.max_batch or 8192)
    cfg.update(kw)
    return nrg.DeviceReplica(nrg._lib.NRG_DS_MEMFS, 0, **s.cfg(**cfg))


def _exec(nrg, dev, lo, hi):
    """nrg_log_exec with the return code kept: (rc, resp, some). The responses are copied out before
    the error latch is read, so they are valid under NRG_E_INVAL too."""
    n = hi - lo
    resp = np.zeros(max(n, 1), nrg.MEMFS_RESP_DTYPE)
    some = np.zeros(max(n, 1), np.uint8)
    rc = dev._lib.nrg_log_exec(dev._h, lo, hi, C.c_void_p(resp.ctypes.data), C.c_void_p(some.ctypes.data))
    return rc, resp[:n], some[:n]


def _same_resp(resp, some, wresp, wsome, what=""):
    np.testing.assert_array_equal(some, wsome, err_msg=what + " some")
    np.testing.assert_array_equal(resp["n"], wresp["n"], err_msg=what + " n")
    np.testing.assert_array_equal(resp["data"], wresp["data"], err_msg=what + " data")


def _same_state(dev, model, what=""):
    for f in range(model.files):
        assert dev.mf_dump(M.FIRST_INO + f) == model.dump(M.FIRST_INO + f), f"{what} file {f}"
    assert dev.digest() == model.digest(), what


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _round(nrg, dev, recs, origin=1, want_rc=0):
    """One fused round on device buffers: (resp, some); nrg_sync afterwards must answer want_rc."""
    import torch

    n = len(recs)
    d_ops = _cuda(recs)
    d_resp = torch.full((max(n, 1) * 136,), 0xEE, dtype=torch.uint8, device="cuda")
    d_some = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    dev.mf_round(d_ops, n, origin, d_resp, d_some)
    assert dev._lib.nrg_sync(dev._h) == want_rc
    torch.cuda.synchronize()
    return d_resp.cpu().numpy().view(nrg.MEMFS_RESP_DTYPE)[:n], d_some.cpu().numpy()[:n]


# ---- every named stream, through append + exec and through a fused round -------------------------------
@pytest.mark.parametrize("s", M.all_streams(), ids=lambda s: s.name)
def test_stream_matches_the_model(nrg, s):
    L = nrg._lib
    model = M.MemFsModel(s.files, s.log2_b)
    wresp, wsome = model.replay(s.recs)
    want_rc = L.NRG_E_INVAL if model.inval else L.NRG_OK
    n = len(s.recs)
    # Log::append, then Log::exec
    dev = _open(nrg, s)
    assert dev.mf_geometry() == (s.files, 1 << s.log2_b)
    first = dev.log_append(s.recs, 1)
    rc, resp, some = _exec(nrg, dev, first, first + n)
    assert rc == want_rc  # latched exactly when an EINVAL record is present
    _same_resp(resp, some, wresp, wsome, "exec")
    _same_state(dev, model, "exec")
    assert dev._lib.nrg_sync(dev._h) == L.NRG_OK  # latched once: reading it cleared it
    dev.close()
    # the fused round: identical outputs
    dev = _open(nrg, s)
    resp2, some2 = _round(nrg, dev, s.recs, want_rc=want_rc)
    _same_resp(resp2, some2, wresp, wsome, "round")
    _same_state(dev, model, "round")
    st = dev.log_state()
    assert st["tail"] == st["ltail"] == n
    # the fused round wrote the log copy: the ring holds the records
    one = np.zeros(1, nrg.MEMFS_OP_DTYPE)
    for i in sorted({0, n // 2, n - 1}):
        assert dev._lib.nrg_test_ring_read(dev._h, i, C.c_void_p(one.ctypes.data)) == L.NRG_OK
        assert one.tobytes() == s.recs[i:i + 1].tobytes(), f"ring record {i}"
    dev.close()


def test_memfs_rs_shape_reads_see_exactly_the_writes_before_them(nrg):
    """memfs.rs's own shape: ino 5, 4096 ones, Write [3; 128] at 100, Read (90, 20) before and after."""
    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_MEMFS, 0, log_bytes=MIN_LOG_BYTES, max_batch=64)
    assert dev.mf_geometry() == (1, 4096) and dev.mf_dump(5) == b"\x01" * 4096
    recs = np.concatenate([M.R(5, 90, 20), M.W(5, 100, b"\x03" * 128), M.R(5, 90, 20), M.G(5)])
    first = dev.log_append(recs, 1)
    resp, some = dev.log_exec(first, first + 4)
    assert some.tolist() == [1, 1, 1, 1] and resp["n"].tolist() == [20, 128, 20, 4096]
    assert resp["data"][0].tobytes() == b"\x01" * 20 + bytes(108)
    assert resp["data"][2].tobytes() == b"\x01" * 10 + b"\x03" * 10 + bytes(108)
    assert not resp["data"][[1, 3]].any()
    assert dev.mf_read(5, 90, 20) == b"\x01" * 10 + b"\x03" * 10
    dev.close()


# ---- round plumbing ------------------------------------------------------------------------------------
def test_exec_spans_four_chunks_and_a_window_in_the_middle_of_one(nrg):
    """max_batch = 256 with 1000 ops: four chunks. Then the same log replayed by a second replica
    with a response window that covers only the middle of the second chunk, into device buffers
    with guard bytes on both sides."""
    import torch

    s = M.memfs_shape(1000, 77, write_pct=30)
    s.max_batch = 256
    model = M.MemFsModel(s.files, s.log2_b)
    wresp, wsome = model.replay(s.recs)
    dev = _open(nrg, s)
    first = dev.log_append(s.recs, 1)
    rc, resp, some = _exec(nrg, dev, first, first + 1000)
    assert rc == nrg._lib.NRG_OK
    _same_resp(resp, some, wresp, wsome)
    _same_state(dev, model)
    dev.close()

    dev = _open(nrg, s)
    first = dev.log_append(s.recs, 1)
    lo, hi = 300, 433  # inside chunk [256, 512)
    w = hi - lo
    d_resp = torch.full(((w + 2) * 136,), 0xEE, dtype=torch.uint8, device="cuda")
    d_some = torch.full((w + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    dev.log_exec_device(first + lo, first + hi, d_resp.data_ptr() + 136, d_some.data_ptr() + 8)
    dev.sync()
    torch.cuda.synchronize()
    r, sm = d_resp.cpu().numpy(), d_some.cpu().numpy()
    assert (r[:136] == 0xEE).all() and (r[-136:] == 0xEE).all(), "responses outside the window were written"
    assert (sm[:8] == 0xEE).all() and (sm[8 + w:] == 0xEE).all()
    _same_resp(r[136:-136].view(nrg.MEMFS_RESP_DTYPE), sm[8:8 + w], wresp[lo:hi], wsome[lo:hi], "window")
    _same_state(dev, model, "window")
    dev.close()


def test_log_wraps(nrg):
    """A log of 16384 entries and seven fused rounds of 4000 records: the ring wraps, and a round
    after the wrap is replayed by append + exec as well."""
    s = M.memfs_shape(4000, 5, files=4, log2_b=9, write_pct=40)
    dev = _open(nrg, s, max_batch=4096)
    model = M.MemFsModel(s.files, s.log2_b)
    assert dev.log_state()["size"] == 16384
    for r in range(7):
        recs = M.memfs_shape(4000, 50 + r, files=4, log2_b=9, write_pct=40).recs
        wresp, wsome = model.replay(recs)
        if r == 5:
            first = dev.log_append(recs, 1)
            rc, resp, some = _exec(nrg, dev, first, first + 4000)
            assert rc == nrg._lib.NRG_OK and first == 5 * 4000
        else:
            resp, some = _round(nrg, dev, recs)
        _same_resp(resp, some, wresp, wsome, f"round {r}")
    st = dev.log_state()
    assert st["tail"] == 28000 and st["head"] > 0  # past the ring's size: positions wrapped
    _same_state(dev, model)
    dev.close()


# ---- lifecycle -----------------------------------------------------------------------------------------
def test_init_then_replay_and_read_needs_a_synced_replica(nrg):
    L = nrg._lib
    s = M.three_files(200, 9)
    dev = _open(nrg, s)
    model = M.MemFsModel(s.files, s.log2_b)
    seed = bytes(range(1, 201))
    dev.mf_init(6, seed)
    model.init(6, seed)
    assert dev.mf_dump(6) == seed + b"\x01" * 56 and dev.mf_read(6, 190, 100) == seed[190:] + b"\x01" * 56
    assert dev._lib.nrg_memfs_init(dev._h, 8, None, 0) == L.NRG_E_INVAL  # no such ino
    assert dev._lib.nrg_memfs_init(dev._h, 5, C.c_void_p(0), 257) == L.NRG_E_INVAL  # more than the file holds
    first = dev.log_append(s.recs, 1)
    n = C.c_uint64()
    buf = np.zeros(256, np.uint8)
    assert dev._lib.nrg_memfs_read(dev._h, 5, 0, 16, C.c_void_p(buf.ctypes.data), C.byref(n)) == L.NRG_E_NOT_SYNCED
    wresp, wsome = model.replay(s.recs)
    rc, resp, some = _exec(nrg, dev, first, first + len(s.recs))
    assert rc == L.NRG_OK
    _same_resp(resp, some, wresp, wsome)
    _same_state(dev, model)
    assert dev.mf_read(7, 250, 100) == model.dump(7)[250:] and dev.mf_read(7, 256, 4) == b""
    assert dev._lib.nrg_memfs_read(dev._h, 4, 0, 16, C.c_void_p(buf.ctypes.data), C.byref(n)) == L.NRG_E_INVAL
    assert dev._lib.nrg_memfs_dump(dev._h, 5, C.c_void_p(buf.ctypes.data), 255, C.byref(n)) == L.NRG_E_CAPACITY
    assert n.value == 256
    dev.close()


def test_snapshot_restore_and_geometry_guard(nrg):
    L = nrg._lib
    s = M.three_files(300, 21)
    model = M.MemFsModel(s.files, s.log2_b)
    model.replay(s.recs)
    src = _open(nrg, s)
    _round(nrg, src, s.recs)
    info = src.snapshot_info()
    assert info.ds_kind == L.NRG_DS_MEMFS and info.items == 3 * 256 // 8 and info.bytes == 64 + 768
    img = src.snapshot()
    hinfo, data = nrg.snapshot.unpack(img)
    assert hinfo.log_idx == 300 and hinfo.digest == model.digest()
    assert data.tobytes() == b"".join(model.dump(5 + f) for f in range(3))
    assert img.tobytes() == nrg.snapshot.pack(L.NRG_DS_MEMFS, [model.dump(5 + f) for f in range(3)], 300).tobytes()
    # into a second context of the same geometry: dumps and digests equal, and it goes on from there
    dst = _open(nrg, s)
    dst.restore(img)
    _same_state(dst, model, "restored")
    assert dst.log_state()["ltail"] == 300 and dst.digest() == src.digest()
    more = M.three_files(100, 22).recs
    wresp, wsome = model.replay(more)
    for d in (src, dst):
        resp, some = _round(nrg, d, more)
        _same_resp(resp, some, wresp, wsome)
        _same_state(d, model, "after restore")
    # another geometry: another total is refused with nothing touched; the same total cut into
    # other files is refused by the digest and leaves the files as at open
    img = src.snapshot()
    for files, log2_b in ((3, 9), (1, 8), (6, 7)):
        other = nrg.DeviceReplica(L.NRG_DS_MEMFS, 0, log_bytes=MIN_LOG_BYTES, max_batch=64, log2_slots=log2_b,
                                  queue_capacity=files)
        other.mf_init(5, b"\x09" * 8)
        with pytest.raises(nrg.NrgError) as e:
            other.restore(img)
        assert e.value.code == L.NRG_E_INVAL
        want = b"\x09" * 8 if files << log2_b != 768 else b"\x01" * 8
        assert other.mf_read(5, 0, 8) == want
        other.close()
    stack = nrg.DeviceReplica(L.NRG_DS_STACK, 0, log_bytes=MIN_LOG_BYTES, max_batch=64, stack_capacity=64)
    with pytest.raises(nrg.NrgError) as e:
        stack.restore(img)
    assert e.value.code == L.NRG_E_INVAL
    stack.close()
    src.close()
    dst.close()


def test_kind_guards_both_ways_and_rejected_configs(nrg):
    L = nrg._lib
    lib = L.load()
    E = L.NRG_E_INVAL
    n = C.c_uint64()
    buf = np.zeros(4096, np.uint8)
    p = C.c_void_p(buf.ctypes.data)
    mf = nrg.DeviceReplica(L.NRG_DS_MEMFS, 0, log_bytes=MIN_LOG_BYTES, max_batch=64)
    st = nrg.DeviceReplica(L.NRG_DS_STACK, 0, log_bytes=MIN_LOG_BYTES, max_batch=64, stack_capacity=64)
    # the file store's calls on a context of another kind
    assert lib.nrg_memfs_round_async(st._h, None, 0, 1, None, None) == E
    assert lib.nrg_memfs_init(st._h, 5, p, 1) == E
    assert lib.nrg_memfs_read(st._h, 5, 0, 1, p, C.byref(n)) == E
    assert lib.nrg_memfs_dump(st._h, 5, p, 4096, C.byref(n)) == E
    assert lib.nrg_memfs_geometry(st._h, C.byref(n), C.byref(n)) == E
    # every other kind's calls on a file-store context
    assert lib.nrg_stack_round_async(mf._h, None, 0, 1, None, None) == E
    assert lib.nrg_stack_len(mf._h, C.byref(n)) == E
    assert lib.nrg_hashmap_get(mf._h, p, 0, p, p) == E
    assert lib.nrg_hashmap_round_async(mf._h, None, 0, 1, None, 0, None, None, None, None) == E
    assert lib.nrg_hashmap_size(mf._h, C.byref(n)) == E
    assert lib.nrg_queue_len(mf._h, C.byref(n)) == E
    assert lib.nrg_queue_round_async(mf._h, None, 0, 1, None, None) == E
    assert lib.nrg_synth_round_async(mf._h, None, 0, 1, None, None) == E
    assert lib.nrg_synth_dump(mf._h, p, 0, C.byref(n)) == E
    assert lib.nrg_vspace_round_async(mf._h, None, 0, 1, None, None) == E
    assert lib.nrg_vspace_tables(mf._h, C.byref(n)) == E
    assert lib.nrg_skiplist_round_async(mf._h, None, 0, 1, None, None) == E
    assert lib.nrg_skiplist_len(mf._h, C.byref(n)) == E
    # no growth bound, no combiner
    assert lib.nrg_set_max_capacity(mf._h, 1 << 20) == E and lib.nrg_set_max_capacity(mf._h, 0) == E
    comb = C.c_void_p()
    assert lib.nrg_combiner_open(mf._h, 1, C.byref(comb)) == E and not comb.value
    # a misaligned record or response buffer
    assert lib.nrg_memfs_round_async(mf._h, C.c_void_p(buf.ctypes.data + 4), 1, 1, None, None) == E
    assert mf.mf_dump(5) == b"\x01" * 4096  # and nothing of it touched the file
    mf.close()
    st.close()
    # nrg_open: the ranges of the two reused fields and of max_batch
    for bad in (dict(log2_slots=6), dict(log2_slots=27), dict(queue_capacity=0), dict(queue_capacity=(1 << 16) + 1),
                dict(log2_slots=26, queue_capacity=16), dict(max_batch=(1 << 20) + 1)):
        cfg = L.default_config(L.NRG_DS_MEMFS)
        cfg.log_bytes, cfg.max_batch = MIN_LOG_BYTES, 64
        for k, v in bad.items():
            setattr(cfg, k, v)
        h = C.c_void_p()
        assert lib.nrg_open(0, C.byref(cfg), C.byref(h)) == E and not h.value, bad
    for ok in (dict(log2_slots=7, queue_capacity=1), dict(log2_slots=7, queue_capacity=1 << 16)):
        d = nrg.DeviceReplica(L.NRG_DS_MEMFS, 0, log_bytes=MIN_LOG_BYTES, max_batch=64, **ok)
        assert d.mf_geometry() == (ok["queue_capacity"], 128)
        assert d.mf_dump(M.FIRST_INO + ok["queue_capacity"] - 1) == b"\x01" * 128
        d.close()


def test_replica_api_executes_the_three_ops(nrg):
    """Replica(log, nrgpu.MemFs): two replicas on one log; a Read through one sees the Write through
    the other (both are log records), and verify hands out the files."""
    log = nrg.Log(MIN_LOG_BYTES)
    a = nrg.Replica(log, nrg.MemFs, max_batch=64)
    b = nrg.Replica(log, nrg.MemFs, max_batch=64)
    ta, tb = a.register(), b.register()
    assert a.execute_mut(nrg.MfRead(5, 90, 20), ta) == ("data", b"\x01" * 20)
    assert a.execute_mut(nrg.MfWrite(5, 100, b"\x03" * 128), ta) == ("written", 128)
    assert b.execute_mut(nrg.MfRead(5, 90, 20), tb) == ("data", b"\x01" * 10 + b"\x03" * 10)
    assert b.execute_mut(nrg.MfGetAttr(5), tb) == ("attr", 4096)
    assert b.execute_mut(nrg.MfGetAttr(6), tb) == ("err", nrg._lib.NRG_MEMFS_ENOENT)
    assert a.execute_mut(nrg.MfWrite(5, 4000, b"\x07" * 97), ta) == ("err", nrg._lib.NRG_MEMFS_EFBIG)
    want = b"\x01" * 100 + b"\x03" * 128 + b"\x01" * (4096 - 228)
    seen = []
    a.verify(seen.append)
    b.verify(seen.append)
    assert seen == [[want], [want]]
    assert a.digest() == b.digest() == nrg.digest.memfs([want])
    a.dev.close()
    b.dev.close()


# ---- a two-member replicated group ---------------------------------------------------------------------
def test_two_member_group_replays_both_segments(nrg):
    """nrg_group_round_async over the loopback collectives: both members replay W_0 || W_1 of every
    round, each gets the responses of its own segment, nrg_group_verify says identical, and the
    digest is the model's. The file store takes the generic path (append segments + exec)."""
    import torch

    L = nrg._lib
    lib = L.load()
    G = 2
    cfg = L.default_config(L.NRG_DS_MEMFS)
    cfg.log_bytes, cfg.max_batch, cfg.log2_slots, cfg.queue_capacity = MIN_LOG_BYTES, 512, 8, 3
    L.check(lib.nrg_test_loopback_collectives(1))
    g = C.c_void_p()
    try:
        L.check(lib.nrg_group_open((C.c_int * G)(0, 0), G, C.byref(cfg), C.byref(g)), "nrg_group_open")
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))
    model = M.MemFsModel(3, 8)
    keep = []
    for r, lens in enumerate([[150, 90], [0, 70], [200, 200]]):
        rd = (L.Round * G)()
        want, got = [], []
        for i in range(G):
            n = lens[i]
            recs = M.three_files(n, 300 + 10 * r + i).recs if n else np.zeros(0, nrg.MEMFS_OP_DTYPE)
            want.append(model.replay(recs))  # in rank order: W_0 || W_1
            d_ops = _cuda(recs) if n else None
            d_resp = torch.full((max(n, 1) * 136,), 0xEE, dtype=torch.uint8, device="cuda")
            d_some = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
            rd[i].recs, rd[i].n = (d_ops.data_ptr() if n else 0), n
            rd[i].resp, rd[i].some = d_resp.data_ptr(), d_some.data_ptr()
            got.append((d_resp, d_some))
            keep.append(d_ops)
        torch.cuda.synchronize()
        L.check(lib.nrg_group_round_async(g, rd, None), f"round {r}")
        L.check(lib.nrg_group_sync(g), f"sync {r}")
        torch.cuda.synchronize()
        for i in range(G):
            n = lens[i]
            resp = got[i][0].cpu().numpy().view(nrg.MEMFS_RESP_DTYPE)[:n]
            _same_resp(resp, got[i][1].cpu().numpy()[:n], want[i][0], want[i][1], f"round {r} member {i}")
    out = np.zeros((G, 3), np.uint64)
    same = C.c_int(-1)
    assert lib.nrg_group_verify(g, out.ctypes.data_as(C.c_void_p), C.byref(same)) == L.NRG_OK
    assert same.value == 1
    assert [tuple(int(x) for x in row) for row in out] == [model.digest()] * G
    for i in range(G):
        h = lib.nrg_group_replica(g, i)
        buf = np.zeros(256, np.uint8)
        n = C.c_uint64()
        for f in range(3):
            assert lib.nrg_memfs_dump(h, 5 + f, C.c_void_p(buf.ctypes.data), 256, C.byref(n)) == L.NRG_OK
            assert buf.tobytes() == model.dump(5 + f), f"member {i} file {f}"
    # no key-partitioned rounds for this kind: the round is dropped on every rank
    assert lib.nrg_group_partitioned_round(g, (L.Round * G)()) == L.NRG_E_INVAL
    assert lib.nrg_group_verify(g, None, C.byref(same)) == L.NRG_OK and same.value == 1
    assert lib.nrg_group_close(g) == L.NRG_OK
