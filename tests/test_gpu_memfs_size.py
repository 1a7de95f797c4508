"""The file store with sizes (nrg_memfs_enable_sizes: SetAttr as ftruncate, Writes that grow a file)
bit-exact against the sequential model of tests/memfs_size_model.py: every response field and some,
the dump of every file (up to its size), every size, every stored byte (those at and past a size are
zero), the digest against the numpy definition and the model's own, and the error latch. Then chunks
and response windows, the direct calls, snapshot / restore, a replicated group, and the gate: a
context that never enabled sizes answers as it always did.

Shapes are the smallest at which each piece can go wrong; tests/test_memfs_size_cpu.py checks on the
CPU that every named stream reaches the arms it is named for. No record is skipped or filtered."""
import ctypes as C

import numpy as np
import pytest

import memfs_model as M
import memfs_size_model as Z
from memfs_size_model import G, R, S, W

pytestmark = pytest.mark.gpu

MIN_LOG_BYTES = 2 * 32 * 256 * 64  # Log::new's floor: 16384 entries


def _open(nrg, s, sized=True, **kw):
    mb = s.max_batch or 8192
    cfg = dict(log_bytes=max(MIN_LOG_BYTES, 4 * mb * 64), max_batch=mb)
    cfg.update(kw)
    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_MEMFS, 0, **s.cfg(**cfg))
    if sized:
        dev.mf_enable_sizes()
    return dev


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _round(nrg, dev, recs, want_rc=0):
    """One fused round on device buffers: (resp, some); nrg_sync afterwards must answer want_rc."""
    import torch

    n = len(recs)
    d_ops = _cuda(recs)
    d_resp = torch.full((max(n, 1) * 136,), 0xEE, dtype=torch.uint8, device="cuda")
    d_some = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    dev.mf_round(d_ops, n, 1, d_resp, d_some)
    assert dev._lib.nrg_sync(dev._h) == want_rc
    torch.cuda.synchronize()
    return d_resp.cpu().numpy().view(nrg.MEMFS_RESP_DTYPE)[:n], d_some.cpu().numpy()[:n]


def _same_resp(resp, some, wresp, wsome, what=""):
    np.testing.assert_array_equal(some, wsome, err_msg=what + " some")
    np.testing.assert_array_equal(resp["n"], wresp["n"], err_msg=what + " n")
    np.testing.assert_array_equal(resp["data"], wresp["data"], err_msg=what + " data")


def _same_state(nrg, dev, model, what=""):
    """Dumps, sizes, every stored byte (through the snapshot's payload), and the digest three ways."""
    for f in range(model.files):
        assert dev.mf_size(M.FIRST_INO + f) == model.size[f], f"{what} size of file {f}"
        assert dev.mf_dump(M.FIRST_INO + f) == model.dump(M.FIRST_INO + f), f"{what} file {f}"
    info, data = nrg.snapshot.unpack(dev.snapshot())
    assert info.items == model.files * model.B // 8 + model.files
    raw, sizes = nrg.snapshot.memfs_split(data, model.files)
    assert raw.tobytes() == model.raw(), f"{what} stored bytes"
    assert sizes.tolist() == model.size
    dg = dev.digest()
    assert dg == info.digest == model.digest(), what
    assert dg == nrg.digest.memfs([bytes(d) for d in model.data], model.size)


# ---- every named stream, chunk by chunk through fused rounds ----------------------------------------------
@pytest.mark.parametrize("s", Z.all_streams(), ids=lambda s: s.name)
def test_stream_matches_the_model(nrg, s):
    L = nrg._lib
    model, want = Z.expected(s)
    dev = _open(nrg, s)
    latched = False
    for i, (recs, (wresp, wsome)) in enumerate(zip(s.chunks, want)):
        bad = bool(((recs["op"] > Z.SETATTR) | (recs["len"] > 128)).any())
        resp, some = _round(nrg, dev, recs, want_rc=L.NRG_E_INVAL if bad else L.NRG_OK)
        latched |= bad
        _same_resp(resp, some, wresp, wsome, f"chunk {i}")
    assert latched == model.inval
    assert dev._lib.nrg_sync(dev._h) == L.NRG_OK  # latched once: reading it cleared it
    _same_state(nrg, dev, model, s.name)
    dev.close()


def test_one_line_one_run_known_answer(nrg):
    """Old bytes, zeros, written bytes, zeros: against the bytes themselves, not the model."""
    s = Z.one_line_one_run()
    dev = _open(nrg, s)
    resp, some = _round(nrg, dev, s.chunks[0])
    want = s.old[:5] + bytes(59) + s.mid[:16] + bytes(48)
    assert some.tolist() == [1] * 6 and resp["n"].tolist() == [128, 5, 32, 80, 128, 128]
    assert resp["data"][5].tobytes() == want and dev.mf_dump(5) == want and dev.mf_size(5) == 128
    dev.close()


# ---- across chunks ------------------------------------------------------------------------------------------
def test_exec_spans_five_chunks_and_a_window_that_starts_and_ends_mid_chunk(nrg):
    """1025 records, max_batch = 256, through nrg_log_append + nrg_log_exec: every response; then a
    second replica with a response window [300, 900) into device buffers with guard bytes around."""
    import torch

    s = Z.random_stream("across_chunks", 1025, 41, 2, 9, setattr_pct=8, max_batch=256)
    model = Z.SizedModel(s.files, s.log2_b)
    wresp, wsome = model.replay(s.recs)
    dev = _open(nrg, s)
    first = dev.log_append(s.recs, 1)
    resp, some = dev.log_exec(first, first + 1025)
    _same_resp(resp, some, wresp, wsome)
    _same_state(nrg, dev, model)
    dev.close()

    dev = _open(nrg, s)
    first = dev.log_append(s.recs, 1)
    lo, hi = 300, 900
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
    _same_state(nrg, dev, model, "window")
    dev.close()


# ---- around it ------------------------------------------------------------------------------------------------
def test_direct_calls_seed_and_clip(nrg):
    """nrg_memfs_truncate / nrg_memfs_init seed files; nrg_memfs_read, nrg_memfs_dump and
    nrg_memfs_pread clip at a shrunken size; then a replay goes on from the seeded state."""
    L = nrg._lib
    s = Z.random_stream("seeded", 300, 42, 3, 8, setattr_pct=8)
    model = Z.SizedModel(3, 8)
    dev = _open(nrg, s)
    dev.mf_enable_sizes()  # idempotent
    for ino, size in ((5, 0), (6, 100), (7, 256)):
        dev.mf_truncate(ino, size)
        model.truncate(ino, size)
    seed = bytes(range(1, 41))
    dev.mf_init(5, seed)   # an empty file seeded: size 40
    model.init(5, seed)
    dev.mf_init(6, seed)   # below the size: the size stays 100
    model.init(6, seed)
    assert [dev.mf_size(5 + f) for f in range(3)] == [40, 100, 256]
    assert dev.mf_dump(5) == seed and dev.mf_dump(6) == seed + b"\x01" * 60
    assert dev.mf_read(6, 90, 50) == b"\x01" * 10 and dev.mf_read(6, 100, 8) == b"" and dev.mf_read(5, 0, 256) == seed
    dev.mf_truncate(6, 200)  # grown again: zeros, not the old bytes
    model.truncate(6, 200)
    assert dev.mf_read(6, 90, 50) == b"\x01" * 10 + bytes(40)
    reqs = np.zeros(5, nrg.MEMFS_RD_DTYPE)
    reqs["ino"], reqs["offset"], reqs["len"] = [5, 5, 6, 7, 9], [30, 40, 150, 0, 0], [100, 8, 1 << 40, 300, 8]
    data, offs, some = dev.mf_pread(reqs)
    data, offs, some = data.cpu().numpy(), offs.cpu().numpy(), some.cpu().numpy()
    assert some.tolist() == [1, 1, 1, 1, 0] and np.diff(offs).tolist() == [10, 0, 50, 256, 0]
    assert data[:10].tobytes() == seed[30:] and data[10:60].tobytes() == bytes(50) and data[60:316].tobytes() == b"\x01" * 256
    n = C.c_uint64()
    assert dev._lib.nrg_memfs_truncate(dev._h, 5, 257) == L.NRG_E_INVAL
    assert dev._lib.nrg_memfs_truncate(dev._h, 8, 0) == L.NRG_E_INVAL
    assert dev._lib.nrg_memfs_size(dev._h, 8, C.byref(n)) == L.NRG_E_INVAL
    _same_state(nrg, dev, model, "seeded")
    wresp, wsome = model.replay(s.recs)
    resp, some = _round(nrg, dev, s.recs)
    _same_resp(resp, some, wresp, wsome)
    _same_state(nrg, dev, model, "replayed")
    dev.close()


def test_snapshot_restore_sized_and_unsized_images(nrg):
    L = nrg._lib
    s = Z.random_stream("snap", 400, 43, 3, 8, setattr_pct=10)
    model = Z.SizedModel(3, 8)
    model.replay(s.recs)
    src = _open(nrg, s)
    _round(nrg, src, s.recs)
    info = src.snapshot_info()
    assert info.items == 3 * 256 // 8 + 3 and info.bytes == 64 + 768 + 24 + 40
    img = src.snapshot()
    assert img.tobytes() == nrg.snapshot.pack(L.NRG_DS_MEMFS, [bytes(d) for d in model.data], 400, model.size).tobytes()
    # into a fresh context, which becomes sized and goes on from there
    dst = _open(nrg, s, sized=False)
    n = C.c_uint64()
    assert dst._lib.nrg_memfs_size(dst._h, 5, C.byref(n)) == L.NRG_E_INVAL
    dst.restore(img)
    _same_state(nrg, dst, model, "restored")
    assert dst.log_state()["ltail"] == 400
    more = Z.random_stream("snap_more", 200, 44, 3, 8, setattr_pct=10).recs
    wresp, wsome = model.replay(more)
    for d in (src, dst):
        resp, some = _round(nrg, d, more)
        _same_resp(resp, some, wresp, wsome)
        _same_state(nrg, d, model, "after restore")
    # a sized image with a non-zero byte past a size, or a size above B: refused, the files as at open
    files = [bytearray(b"\x05" * 256) for _ in range(3)]
    sizes = [256, 100, 0]
    for f in range(3):
        files[f][sizes[f]:] = bytes(256 - sizes[f])
    good = nrg.snapshot.pack(L.NRG_DS_MEMFS, files, 7, sizes)
    dst.restore(good)
    assert [dst.mf_size(5 + f) for f in range(3)] == sizes and dst.mf_dump(6) == b"\x05" * 100
    for spoil in ("byte", "last_byte", "size"):
        f2, s2 = [bytearray(f) for f in files], list(sizes)
        if spoil == "byte":
            f2[1][100] = 9
        elif spoil == "last_byte":
            f2[2][255] = 9
        else:
            s2[0] = 257
        bad = nrg.snapshot.pack(L.NRG_DS_MEMFS, f2, 7, s2)
        with pytest.raises(nrg.NrgError) as e:
            dst.restore(bad)
        assert e.value.code == L.NRG_E_INVAL, spoil
        assert [dst.mf_size(5 + f) for f in range(3)] == [256] * 3 and dst.mf_dump(7) == b"\x01" * 256, spoil
    # an unsized image into a sized context: it stays sized, every size B
    plain = _open(nrg, s, sized=False)
    plain.mf_init(6, b"\x09" * 50)
    uimg = plain.snapshot()
    assert nrg.snapshot.header(uimg).items == 3 * 256 // 8
    dst.mf_truncate(6, 10)
    dst.restore(uimg)
    assert [dst.mf_size(5 + f) for f in range(3)] == [256] * 3
    assert dst.mf_dump(6) == b"\x09" * 50 + b"\x01" * 206
    assert dst.digest() == nrg.digest.memfs([plain.mf_dump(5 + f) for f in range(3)], [256] * 3)
    for d in (src, dst, plain):
        d.close()


def test_two_member_group_verifies_sizes(nrg):
    """nrg_group_round_async over the loopback collectives, sizes enabled on both members: after rounds
    with SetAttrs nrg_group_verify says identical and the digest is the model's; a size changed on one
    member by a direct truncate (over bytes that are zero already) makes them differ; nrg_group_resync
    carries the sizes."""
    import torch

    L = nrg._lib
    lib = L.load()
    G2 = 2
    cfg = L.default_config(L.NRG_DS_MEMFS)
    cfg.log_bytes, cfg.max_batch, cfg.log2_slots, cfg.queue_capacity = MIN_LOG_BYTES, 512, 8, 3
    L.check(lib.nrg_test_loopback_collectives(1))
    g = C.c_void_p()
    try:
        L.check(lib.nrg_group_open((C.c_int * G2)(0, 0), G2, C.byref(cfg), C.byref(g)), "nrg_group_open")
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))
    hs = [lib.nrg_group_replica(g, i) for i in range(G2)]
    for h in hs:
        assert lib.nrg_memfs_enable_sizes(h) == L.NRG_OK
    model = Z.SizedModel(3, 8)
    keep = []
    for r, lens in enumerate([[150, 90], [0, 70]]):
        rd = (L.Round * G2)()
        want, got = [], []
        for i in range(G2):
            n = lens[i]
            recs = Z.random_stream("g", n, 300 + 10 * r + i, 3, 8, setattr_pct=10).recs if n else np.zeros(0, nrg.MEMFS_OP_DTYPE)
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
        for i in range(G2):
            n = lens[i]
            resp = got[i][0].cpu().numpy().view(nrg.MEMFS_RESP_DTYPE)[:n]
            _same_resp(resp, got[i][1].cpu().numpy()[:n], want[i][0], want[i][1], f"round {r} member {i}")
    assert model.arms["shrink"] >= 5
    out = np.zeros((G2, 3), np.uint64)
    same = C.c_int(-1)
    assert lib.nrg_group_verify(g, out.ctypes.data_as(C.c_void_p), C.byref(same)) == L.NRG_OK
    assert same.value == 1
    assert [tuple(int(x) for x in row) for row in out] == [model.digest()] * G2
    # one member's size alone: shrink a file to zero (its bytes become zero), then give member 1 a size
    # of 8 over those zero bytes: the stored bytes are the same on both, only the size differs
    n = C.c_uint64()
    for h in hs:
        assert lib.nrg_memfs_truncate(h, 6, 0) == L.NRG_OK
    assert lib.nrg_group_verify(g, None, C.byref(same)) == L.NRG_OK and same.value == 1
    assert lib.nrg_memfs_truncate(hs[1], 6, 8) == L.NRG_OK
    assert lib.nrg_group_verify(g, None, C.byref(same)) == L.NRG_OK and same.value == 0
    # resync from member 1: the image carries the sizes
    assert lib.nrg_group_resync(g, 1) == L.NRG_OK
    assert lib.nrg_memfs_size(hs[0], 6, C.byref(n)) == L.NRG_OK and n.value == 8
    assert lib.nrg_group_verify(g, None, C.byref(same)) == L.NRG_OK and same.value == 1
    assert lib.nrg_group_close(g) == L.NRG_OK


def test_replica_api_executes_setattr(nrg):
    log = nrg.Log(MIN_LOG_BYTES)
    a = nrg.Replica(log, nrg.MemFs, max_batch=64)
    t = a.register()
    a.dev.mf_enable_sizes()
    assert a.execute_mut(nrg.MfSetAttr(5, 100), t) == ("attr", 100)
    assert a.execute_mut(nrg.MfGetAttr(5), t) == ("attr", 100)
    assert a.execute_mut(nrg.MfWrite(5, 120, b"\x03" * 8), t) == ("written", 8)
    assert a.execute_mut(nrg.MfRead(5, 96, 64), t) == ("data", b"\x01" * 4 + bytes(20) + b"\x03" * 8)
    assert a.execute_mut(nrg.MfSetAttr(5, 4097), t) == ("err", nrg._lib.NRG_MEMFS_EFBIG)
    assert a.dev.mf_size(5) == 128
    a.dev.close()


# ---- the gate -------------------------------------------------------------------------------------------------
def test_a_context_without_sizes_answers_as_before(nrg):
    """Op 3 is EINVAL and latches, nrg_memfs_size / nrg_memfs_truncate are NRG_E_INVAL, a Write never
    grows and GetAttr answers B: tests/memfs_model.py's unsized model, records and all."""
    L = nrg._lib
    recs = np.concatenate([W(5, 0, b"\x07" * 16), S(5, 10), G(5), R(5, 0, 32), S(5, 0), R(5, 4090, 16)])
    model = M.MemFsModel(1, 12)
    wresp, wsome = model.replay(recs)
    assert wresp["n"].tolist() == [16, M.EINVAL, 4096, 32, M.EINVAL, 6] and model.inval
    dev = nrg.DeviceReplica(L.NRG_DS_MEMFS, 0, log_bytes=MIN_LOG_BYTES, max_batch=64)
    resp, some = _round(nrg, dev, recs, want_rc=L.NRG_E_INVAL)
    _same_resp(resp, some, wresp, wsome)
    n = C.c_uint64()
    assert dev._lib.nrg_memfs_size(dev._h, 5, C.byref(n)) == L.NRG_E_INVAL
    assert dev._lib.nrg_memfs_truncate(dev._h, 5, 0) == L.NRG_E_INVAL
    assert dev.mf_dump(5) == model.dump(5) and dev.digest() == model.digest()
    assert dev.snapshot_info().items == 4096 // 8
    # and the calls are the file store's alone
    st = nrg.DeviceReplica(L.NRG_DS_STACK, 0, log_bytes=MIN_LOG_BYTES, max_batch=64, stack_capacity=64)
    assert st._lib.nrg_memfs_enable_sizes(st._h) == L.NRG_E_INVAL
    assert st._lib.nrg_memfs_size(st._h, 5, C.byref(n)) == L.NRG_E_INVAL
    assert st._lib.nrg_memfs_truncate(st._h, 5, 0) == L.NRG_E_INVAL
    st.close()
    # enabling needs a synced replica
    first = dev.log_append(recs[:1], 1)
    assert dev._lib.nrg_memfs_enable_sizes(dev._h) == L.NRG_E_NOT_SYNCED
    dev.log_exec(first, first + 1)
    dev.mf_enable_sizes()
    assert dev.mf_size(5) == 4096 and dev.mf_dump(5) == model.dump(5)
    dev.close()
