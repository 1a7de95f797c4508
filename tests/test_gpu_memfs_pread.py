"""The file store's read-only reads (nrg_memfs_pread / nrg_memfs_pread_async, csrc/memfs.hip) bit-exact
against the numpy model of tests/memfs_pread_model.py: data, offs and some of every request list, on a
store whose files hold random bytes and were then changed by a short logged round. Every output buffer
is followed by canary bytes: data past min(cap, total), offs past offs[n], some past some[n - 1].

tests/test_memfs_pread_cpu.py checks on the CPU that every named list reaches the arm it is named for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import memfs_model as M
import memfs_pread_model as P

pytestmark = pytest.mark.gpu

MIN_LOG_BYTES = 2 * 32 * 256 * 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = int(re.search(r"#define NRG_MF_PREAD_TILE (\d+)u", open(os.path.join(ROOT, "include", "nrgpu_testing.h")).read()).group(1))
CANARY = 0xEE
GUARD = 64  # canary bytes behind data and some; 8 words behind offs


def _store(nrg, files, log2_b, seed=1, writes=24, **kw):
    """(dev, model): every file seeded with random bytes (nrg_memfs_init), then a logged round of
    `writes` Writes and a few Reads, so that the store is what a replay left."""
    rng = np.random.default_rng(seed)
    cfg = dict(log_bytes=MIN_LOG_BYTES, max_batch=256, log2_slots=log2_b, queue_capacity=files)
    cfg.update(kw)
    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_MEMFS, 0, **cfg)
    model = M.MemFsModel(files, log2_b)
    B = 1 << log2_b
    for f in range(files):
        seedb = rng.integers(2, 256, B, dtype=np.uint8).tobytes()
        dev.mf_init(M.FIRST_INO + f, seedb)
        model.init(M.FIRST_INO + f, seedb)
    recs = []
    for i in range(writes):
        ln = int(rng.integers(1, 129))
        off = int(rng.integers(0, B - ln + 1))
        recs.append(M.W(M.FIRST_INO + int(rng.integers(0, files)), off, rng.integers(2, 256, ln, dtype=np.uint8).tobytes()))
        if i % 4 == 0:
            recs.append(M.R(M.FIRST_INO, off, ln))
    recs = np.concatenate(recs)
    first = dev.log_append(recs, 1)
    dev.log_exec(first, first + len(recs))
    model.replay(recs)
    return dev, model


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _buffers(n, room):
    import torch

    d_data = torch.full((room + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    d_offs = torch.full(((n + 1 + 8) * 8,), CANARY, dtype=torch.uint8, device="cuda")
    d_some = torch.full((n + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    return d_data, d_offs, d_some


def _check(model, rq, cap, data, offs, some, what=""):
    """data / offs / some: the whole host copies of the buffers, canaries included."""
    n = len(rq)
    wdata, woffs, wsome = P.pread(model, rq, cap)
    got_offs = offs.view(np.uint64)
    np.testing.assert_array_equal(got_offs[:n + 1], woffs, err_msg=what + " offs")
    assert (offs[(n + 1) * 8:] == CANARY).all(), what + " words behind offs[n] were written"
    np.testing.assert_array_equal(some[:n], wsome, err_msg=what + " some")
    assert (some[n:] == CANARY).all(), what + " bytes behind some[n - 1] were written"
    end = len(wdata)
    assert end == min(cap, int(woffs[-1]))
    bad = np.flatnonzero(data[:end] != wdata)
    assert bad.size == 0, f"{what} data differs at packed byte {bad[:8].tolist()} of {end}"
    assert (data[end:] == CANARY).all(), what + " data at or past min(cap, total) was written"
    return int(woffs[-1])


def _pread_async(nrg, dev, model, rq, cap=None, what="", shift=0):
    """nrg_memfs_pread_async on device buffers with canaries, checked against the model; `shift`
    misaligns d_data by that many bytes. cap=None: the exact total."""
    import torch

    n = len(rq)
    total = int(P.pread(model, rq)[1][-1])
    cap = total if cap is None else cap
    room = min(cap, total)
    d_rq = _cuda(rq) if n else None
    d_data, d_offs, d_some = _buffers(n, room + shift)
    dev.mf_pread_device(d_rq, n, d_data.data_ptr() + shift if cap else None, cap, d_offs, d_some if n else None)
    dev.sync()
    torch.cuda.synchronize()
    data = d_data.cpu().numpy()
    assert (data[:shift] == CANARY).all(), what + " bytes in front of data were written"
    return _check(model, rq, cap, data[shift:], d_offs.cpu().numpy(), d_some.cpu().numpy(), what)


def _pread_sync(nrg, dev, model, rq, cap, want_rc, what=""):
    """nrg_memfs_pread on host buffers with canaries."""
    n = len(rq)
    total = int(P.pread(model, rq)[1][-1])
    data = np.full(min(cap, total) + GUARD, CANARY, np.uint8)
    offs = np.full((n + 1 + 8) * 8, CANARY, np.uint8)
    some = np.full(n + GUARD, CANARY, np.uint8)
    rqc = np.ascontiguousarray(rq)
    rc = dev._lib.nrg_memfs_pread(dev._h, C.c_void_p(rqc.ctypes.data), n, C.c_void_p(data.ctypes.data), cap,
                                  C.c_void_p(offs.ctypes.data), C.c_void_p(some.ctypes.data))
    assert rc == want_rc, what
    _check(model, rq, cap, data, offs, some, what)


# ---- edges ---------------------------------------------------------------------------------------------
def test_edges_every_len_offset_and_ino(nrg):
    r = P.edges()
    dev, model = _store(nrg, r.files, r.log2_b, seed=2)
    before = dev.digest()
    _pread_async(nrg, dev, model, r.rq, what="edges")
    _pread_sync(nrg, dev, model, r.rq, 1 << 20, nrg._lib.NRG_OK, "edges sync")
    _pread_async(nrg, dev, model, P.reqs([]), what="n = 0")  # offs[0] = 0 and nothing else
    for one in [(5, 0, 0), (5, 3, 1), (6, 0, P.U64_MAX), (4, 0, 9), (5, 256, 1), (5, P.U64_MAX, P.U64_MAX)]:
        _pread_async(nrg, dev, model, P.reqs([one]), what=f"n = 1 {one}")
        _pread_sync(nrg, dev, model, P.reqs([one]), 256, nrg._lib.NRG_OK, f"n = 1 sync {one}")
    offs = np.full(2, 7, np.uint64)
    assert dev._lib.nrg_memfs_pread(dev._h, None, 0, None, 0, C.c_void_p(offs.ctypes.data), None) == nrg._lib.NRG_OK
    assert offs.tolist() == [0, 7]
    assert dev.digest() == before == model.digest()
    dev.close()


# ---- alignment ---------------------------------------------------------------------------------------------
def test_alignment_every_source_and_destination_pair(nrg):
    """16 lists (leading request of 0..15 bytes): every (source mod 16, packed position mod 16) with
    every length of 1, 15, 16, 17, 31, 32, 33, and the wide path at every byte shift; then the same
    with d_data itself misaligned."""
    r0 = P.alignment(0)
    dev, model = _store(nrg, r0.files, r0.log2_b, seed=3)
    for lead in range(16):
        r = P.alignment(lead)
        _pread_async(nrg, dev, model, r.rq, what=r.name)
    for shift in (1, 7, 8, 15):
        _pread_async(nrg, dev, model, P.alignment(5).rq, what=f"d_data + {shift}", shift=shift)
        _pread_async(nrg, dev, model, P.alignment(5).rq, cap=1000 + shift, what=f"d_data + {shift}, cap", shift=shift)
    dev.close()


# ---- tile boundaries, skew, the nrfs shape --------------------------------------------------------------
@pytest.fixture(scope="module")
def tile_store(nrg):
    r = P.tile_edges(T)
    dev, model = _store(nrg, r.files, r.log2_b, seed=4, max_reads=len(r.rq))
    yield r, dev, model
    dev.close()


def test_tile_boundaries(nrg, tile_store):
    r, dev, model = tile_store
    before = dev.digest()
    total = _pread_async(nrg, dev, model, r.rq, what=r.name)
    assert total == 10 * T + 100
    _pread_sync(nrg, dev, model, r.rq, total, nrg._lib.NRG_OK, r.name + " sync")
    _pread_async(nrg, dev, model, r.rq, what=r.name + " shifted", shift=9)
    assert dev.digest() == before
    for f in range(model.files):
        assert dev.mf_dump(M.FIRST_INO + f) == model.dump(M.FIRST_INO + f)


@pytest.mark.parametrize("which", ["total", "total-1", "T", "T+1", "1", "0", "huge"])
def test_cap(nrg, tile_store, which):
    """The async call leaves offs[n] the full total and writes nothing at or past cap; the sync call
    answers NRG_E_CAPACITY with offs, some and the first cap bytes valid."""
    r, dev, model = tile_store
    L = nrg._lib
    total = 10 * T + 100
    cap = {"total": total, "total-1": total - 1, "T": T, "T+1": T + 1, "1": 1, "0": 0, "huge": 1 << 62}[which]
    assert _pread_async(nrg, dev, model, r.rq, cap=cap, what="cap " + which) == total
    _pread_sync(nrg, dev, model, r.rq, cap, L.NRG_E_CAPACITY if cap < total else L.NRG_OK, "sync cap " + which)


def test_max_reads_is_the_most(nrg, tile_store):
    r, dev, model = tile_store
    L = nrg._lib
    n = len(r.rq)  # the store was opened with max_reads = n
    _pread_async(nrg, dev, model, r.rq, cap=64, what="n = max_reads")
    more = np.concatenate([r.rq, P.reqs([(5, 0, 1)])])
    d_rq = _cuda(more)
    d_data, d_offs, d_some = _buffers(n + 1, 16)
    args = (C.c_void_p(d_rq.data_ptr()), n + 1, C.c_void_p(d_data.data_ptr()), 16, C.c_void_p(d_offs.data_ptr()),
            C.c_void_p(d_some.data_ptr()))
    assert dev._lib.nrg_memfs_pread_async(dev._h, *args) == L.NRG_E_CAPACITY
    dev.sync()
    assert (d_offs.cpu().numpy() == CANARY).all() and (d_some.cpu().numpy() == CANARY).all()
    h = [np.zeros(n + 2, np.uint64) for _ in range(3)]
    assert dev._lib.nrg_memfs_pread(dev._h, C.c_void_p(more.ctypes.data), n + 1, C.c_void_p(h[0].ctypes.data), 16,
                                    C.c_void_p(h[1].ctypes.data), C.c_void_p(h[2].ctypes.data)) == L.NRG_E_CAPACITY


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_request_counts_around_the_scan_tile(nrg, tile_store, n):
    """1024 requests are one launch of the scan, 1025 are three; lengths 0..40 on random offsets."""
    _, dev, model = tile_store
    rng = np.random.default_rng(n)
    rq = P.reqs([(4 + int(rng.integers(0, 3)), int(rng.integers(0, 4 * T + 2)), int(rng.integers(0, 41))) for _ in range(n)])
    _pread_async(nrg, dev, model, rq, what=f"n = {n}")


def test_more_than_256_scan_tiles(nrg):
    """262145 requests of 0 or 1 byte: the aggregate scan takes a second step."""
    n = 256 * 1024 + 1
    dev, model = _store(nrg, 2, 8, seed=8, max_reads=n)
    rng = np.random.default_rng(9)
    rq = np.zeros(n, P.RD_DTYPE)
    rq["ino"] = rng.integers(4, 8, n)
    rq["offset"] = rng.integers(0, 258, n)
    rq["len"] = rng.integers(0, 2, n)
    _pread_async(nrg, dev, model, rq, what="262145 requests")
    dev.close()


@pytest.mark.parametrize("big_first", [True, False], ids=["big_first", "big_last"])
def test_skew_one_whole_file_beside_4096_tiny_reads(nrg, big_first):
    r = P.skew(big_first)
    dev, model = _store(nrg, r.files, r.log2_b, seed=5)
    _pread_async(nrg, dev, model, r.rq, what=r.name)
    dev.close()


def test_nrfs_shape_every_file_whole_in_shuffled_order(nrg):
    r = P.nrfs_shape()
    dev, model = _store(nrg, r.files, r.log2_b, seed=6, writes=200)
    assert _pread_async(nrg, dev, model, r.rq, what=r.name) == 64 * 4096
    _pread_sync(nrg, dev, model, r.rq, 64 * 4096, nrg._lib.NRG_OK, r.name + " sync")
    dev.close()


# ---- ordering ---------------------------------------------------------------------------------------------
def test_pread_after_a_round_on_one_stream_sees_its_writes_and_answers_as_its_reads(nrg):
    """nrg_memfs_round_async then nrg_memfs_pread_async, nothing between them: the preads see the
    round's Writes; the ranges of the round's trailing Reads (no Write after them) answer the same
    bytes through pread; the digest is the same before and after the preads."""
    import torch

    dev, model = _store(nrg, 3, 8, seed=7)
    rng = np.random.default_rng(70)
    writes = [M.W(5 + i % 3, int(rng.integers(0, 128)), rng.integers(2, 256, 128, dtype=np.uint8).tobytes()) for i in range(40)]
    ranges = [(5 + int(rng.integers(0, 3)), int(rng.integers(0, 250)), int(rng.integers(0, 129))) for _ in range(30)]
    recs = np.concatenate(writes + [M.R(*x) for x in ranges])
    n = len(recs)
    wresp, wsome = model.replay(recs)
    rq = P.reqs(ranges + [(5, 0, 256), (6, 0, 256), (7, 0, 256)])
    total = int(P.pread(model, rq)[1][-1])
    d_ops, d_rq = _cuda(recs), _cuda(rq)
    d_resp = torch.full((n * 136,), CANARY, dtype=torch.uint8, device="cuda")
    d_rsome = torch.full((n,), CANARY, dtype=torch.uint8, device="cuda")
    d_data, d_offs, d_some = _buffers(len(rq), total)
    torch.cuda.synchronize()
    L = nrg._lib
    assert dev._lib.nrg_memfs_round_async(dev._h, C.c_void_p(d_ops.data_ptr()), n, 1, C.c_void_p(d_resp.data_ptr()),
                                          C.c_void_p(d_rsome.data_ptr())) == L.NRG_OK
    assert dev._lib.nrg_memfs_pread_async(dev._h, C.c_void_p(d_rq.data_ptr()), len(rq), C.c_void_p(d_data.data_ptr()),
                                          total, C.c_void_p(d_offs.data_ptr()), C.c_void_p(d_some.data_ptr())) == L.NRG_OK
    assert dev._lib.nrg_sync(dev._h) == L.NRG_OK
    data, offs = d_data.cpu().numpy(), d_offs.cpu().numpy()
    _check(model, rq, total, data, offs, d_some.cpu().numpy(), "after the round")
    resp = d_resp.cpu().numpy().view(nrg.MEMFS_RESP_DTYPE)
    o = offs.view(np.uint64)
    for k in range(len(ranges)):  # the logged Reads answered the same bytes
        r = resp[len(writes) + k]
        assert int(r["n"]) == int(o[k + 1] - o[k]) == int(wresp["n"][len(writes) + k])
        assert r["data"][:int(r["n"])].tobytes() == data[int(o[k]):int(o[k + 1])].tobytes()
    before = dev.digest()
    assert before == model.digest()
    for _ in range(3):
        _pread_async(nrg, dev, model, rq, what="again")
    assert dev.digest() == before
    # an unreplayed append: the reads refuse until the replica is synced
    first = dev.log_append(M.W(5, 0, b"zz"), 1)
    d = [np.zeros(8, np.uint64) for _ in range(3)]
    one = P.reqs([(5, 0, 2)])
    args = (C.c_void_p(one.ctypes.data), 1, C.c_void_p(d[0].ctypes.data), 8, C.c_void_p(d[1].ctypes.data), C.c_void_p(d[2].ctypes.data))
    assert dev._lib.nrg_memfs_pread(dev._h, *args) == L.NRG_E_NOT_SYNCED
    dev.log_exec(first, first + 1)
    assert dev._lib.nrg_memfs_pread(dev._h, *args) == L.NRG_OK and d[0].tobytes()[:2] == b"zz"
    dev.close()


# ---- a two-member replicated group ---------------------------------------------------------------------------
def test_both_members_of_a_group_answer_the_same(nrg):
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
    rd = (L.Round * G)()
    keep = []
    for i in range(G):
        recs = M.three_files(120 + 30 * i, 500 + i).recs
        model.replay(recs)  # rank order: W_0 || W_1
        d_ops = _cuda(recs)
        d_resp = torch.full((len(recs) * 136,), CANARY, dtype=torch.uint8, device="cuda")
        d_rsome = torch.full((len(recs),), CANARY, dtype=torch.uint8, device="cuda")
        keep += [d_ops, d_resp, d_rsome]
        rd[i].recs, rd[i].n = d_ops.data_ptr(), len(recs)
        rd[i].resp, rd[i].some = d_resp.data_ptr(), d_rsome.data_ptr()
    torch.cuda.synchronize()
    L.check(lib.nrg_group_round_async(g, rd, None), "round")
    L.check(lib.nrg_group_sync(g), "sync")
    rng = np.random.default_rng(11)
    rq = P.reqs([(4 + int(rng.integers(0, 5)), int(rng.integers(0, 260)), int(rng.integers(0, 300))) for _ in range(500)])
    wdata, woffs, wsome = P.pread(model, rq)
    got = []
    for i in range(G):
        h = lib.nrg_group_replica(g, i)
        data = np.full(len(wdata) + GUARD, CANARY, np.uint8)
        offs = np.full((len(rq) + 9) * 8, CANARY, np.uint8)
        some = np.full(len(rq) + GUARD, CANARY, np.uint8)
        assert lib.nrg_memfs_pread(h, C.c_void_p(rq.ctypes.data), len(rq), C.c_void_p(data.ctypes.data), len(wdata),
                                   C.c_void_p(offs.ctypes.data), C.c_void_p(some.ctypes.data)) == L.NRG_OK
        _check(model, rq, len(wdata), data, offs, some, f"member {i}")
        got.append((data.tobytes(), offs.tobytes(), some.tobytes()))
    assert got[0] == got[1]
    same = C.c_int(-1)
    assert lib.nrg_group_verify(g, None, C.byref(same)) == L.NRG_OK and same.value == 1
    assert lib.nrg_group_close(g) == L.NRG_OK


# ---- refusals ---------------------------------------------------------------------------------------------
def test_refusals_another_kind_misaligned_pointers_and_nulls(nrg):
    L = nrg._lib
    lib = L.load()
    E = L.NRG_E_INVAL
    mf = nrg.DeviceReplica(L.NRG_DS_MEMFS, 0, log_bytes=MIN_LOG_BYTES, max_batch=64, max_reads=8)
    st = nrg.DeviceReplica(L.NRG_DS_STACK, 0, log_bytes=MIN_LOG_BYTES, max_batch=64, stack_capacity=64)
    d_rq = _cuda(P.reqs([(5, 0, 4), (5, 8, 4)]))
    d_data, d_offs, d_some = _buffers(2, 8)
    p = lambda t, k=0: C.c_void_p(t.data_ptr() + k)  # noqa: E731
    ok = (p(d_rq), 2, p(d_data), 8, p(d_offs), p(d_some))
    for f in (lib.nrg_memfs_pread_async, lib.nrg_memfs_pread):
        assert f(st._h, *ok) == E  # another kind
        assert f(None, *ok) == E
    a = lib.nrg_memfs_pread_async
    assert a(mf._h, p(d_rq, 4), 1, p(d_data), 8, p(d_offs), p(d_some)) == E  # requests not 8-byte aligned
    assert a(mf._h, p(d_rq), 2, p(d_data), 8, p(d_offs, 4), p(d_some)) == E  # offs not 8-byte aligned
    assert a(mf._h, None, 2, p(d_data), 8, p(d_offs), p(d_some)) == E
    assert a(mf._h, p(d_rq), 2, p(d_data), 8, None, p(d_some)) == E
    assert a(mf._h, p(d_rq), 2, p(d_data), 8, p(d_offs), None) == E
    assert a(mf._h, p(d_rq), 2, None, 8, p(d_offs), p(d_some)) == E
    assert a(mf._h, p(d_rq), 9, p(d_data), 8, p(d_offs), p(d_some)) == L.NRG_E_CAPACITY  # max_reads = 8
    h = [np.zeros(16, np.uint64) for _ in range(4)]
    hp = lambda i, k=0: C.c_void_p(h[i].ctypes.data + k)  # noqa: E731
    s = lib.nrg_memfs_pread
    assert s(mf._h, hp(0, 4), 1, hp(1), 8, hp(2), hp(3)) == E and s(mf._h, hp(0), 1, hp(1), 8, hp(2, 2), hp(3)) == E
    assert s(mf._h, None, 1, hp(1), 8, hp(2), hp(3)) == E and s(mf._h, hp(0), 1, None, 8, hp(2), hp(3)) == E
    assert s(mf._h, hp(0), 1, hp(1), 8, None, hp(3)) == E and s(mf._h, hp(0), 1, hp(1), 8, hp(2), None) == E
    mf.sync()
    assert (d_offs.cpu().numpy() == CANARY).all() and (d_some.cpu().numpy() == CANARY).all()  # nothing was launched
    assert (d_data.cpu().numpy() == CANARY).all()
    # a NULL data with cap = 0 is legal: offs and some alone
    assert a(mf._h, p(d_rq), 2, None, 0, p(d_offs), p(d_some)) == L.NRG_OK
    mf.sync()
    assert d_offs.cpu().numpy().view(np.uint64)[:3].tolist() == [0, 4, 8] and d_some.cpu().numpy()[:2].tolist() == [1, 1]
    assert mf.mf_dump(5) == b"\x01" * 4096 and lib.nrg_sync(mf._h) == L.NRG_OK  # nothing latched
    mf.close()
    st.close()


# ---- Python ---------------------------------------------------------------------------------------------
def test_mf_pread_sizes_its_buffer_and_replica_execute_reads(nrg):
    import torch

    dev, model = _store(nrg, 2, 9, seed=12)
    rq = P.reqs([(5, 500, 100), (9, 0, 4), (6, 0, 512), (5, 3, 0), (6, 17, 33), (5, 1 << 40, 5)])
    wdata, woffs, wsome = P.pread(model, rq)
    for given in (rq, np.array(rq.tolist(), np.uint64), _cuda(rq)):
        data, offs, some = dev.mf_pread(given)  # cap=None: sized on the host
        assert data.is_cuda and data.dtype == torch.uint8 and data.numel() == len(wdata) == int(woffs[-1])
        assert data.cpu().numpy().tobytes() == wdata.tobytes()
        assert offs.cpu().numpy().tolist() == woffs.tolist() and some.cpu().numpy().tolist() == wsome.tolist()
    data, offs, some = dev.mf_pread(rq, cap=40)
    assert data.numel() == 40 and data.cpu().numpy().tobytes() == wdata.tobytes()[:40] and int(offs[-1]) == int(woffs[-1])
    data, offs, some = dev.mf_pread(P.reqs([]))
    assert data.numel() == 0 and offs.cpu().tolist() == [0] and some.numel() == 0
    dev.close()
    # Replica::execute: two replicas on one log; the read through one sees the Write through the other
    log = nrg.Log(MIN_LOG_BYTES)
    a = nrg.Replica(log, nrg.MemFs, max_batch=64)
    b = nrg.Replica(log, nrg.MemFs, max_batch=64)
    ta, tb = a.register(), b.register()
    assert a.execute_mut(nrg.MfWrite(5, 100, b"\x03" * 128), ta) == ("written", 128)
    want = b"\x01" * 100 + b"\x03" * 128 + b"\x01" * (4096 - 228)
    assert b.execute(nrg.MfPread(5, 0, 4096), tb) == ("data", want)  # the whole file: 32 logged Reads' worth
    assert b.execute_batch([nrg.MfPread(5, 90, 20), nrg.MfPread(6, 0, 1), nrg.MfPread(5, 4090, 100), nrg.MfPread(5, 7, 0)],
                           tb) == [("data", want[90:110]), ("err", nrg._lib.NRG_MEMFS_ENOENT), ("data", want[4090:]), ("data", b"")]
    with pytest.raises(TypeError):
        b.execute(nrg.MfRead(5, 0, 1), tb)
    assert a.digest() == b.digest() == nrg.digest.memfs([want])
    a.dev.close()
    b.dev.close()
