"""Removal of keys from the replicated skip list (nrg_skiplist_enable_removal, csrc/skiplist.hip)
against the sequential model of tests/skiplist_remove_model.py: every response, read, dump, length
and digest is compared bit for bit; there are no tolerances. The oracle has no Remove, so the model
is the reference; tests/test_skiplist_remove_cpu.py checks it against a plain dict and shows that
every named stream reaches the arms it is named for."""
import ctypes as C

import numpy as np
import pytest

import skiplist_remove_model as R

pytestmark = pytest.mark.gpu

U64_MAX = 2**64 - 1
LOG_BYTES = 4 * 2 * 32 * 256 * 64
PATHS = ["append_exec", "fused_round", "chunked", "window"]
NEW_KERNELS = ("sl_rm_resp", "sl_rm_state", "sl_drop_base", "sl_drop_delta")
GUARD = 64  # bytes of guard words around a response window


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def _open(nrg, s, max_batch=None, enable=True, **kw):
    kw.setdefault("max_reads", 1 << 12)
    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_SKIPLIST, 0, knobs={"SL_DELTA_MAX": s.delta_max}, log2_slots=s.log2,
                            max_batch=max_batch or s.max_batch, log_bytes=LOG_BYTES, **kw)
    if enable:
        dev.sl_enable_removal()
    return dev, s.model(max_batch)


def _round(dev, recs, origin=1):
    import torch

    n = len(recs)
    resp = torch.zeros(n, dtype=torch.int64, device="cuda")
    some = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dev.sl_round_device(_cuda(recs), n, origin, resp, some)
    dev.sync()
    return resp.cpu().numpy().view(np.uint64), some.cpu().numpy()


def _window(dev, recs):
    """append, then exec with a response window that begins and ends inside the chunk, between guards"""
    import torch

    n = len(recs)
    a, b = (n // 3, n - n // 4) if n >= 4 else (0, n)
    w = b - a
    resp = torch.full((w + 2 * GUARD // 8,), -7, dtype=torch.int64, device="cuda")
    some = torch.full((w + 2 * GUARD,), 9, dtype=torch.uint8, device="cuda")
    first = dev.log_append(recs, 1)
    dev.log_exec_device(first + a, first + b, resp.data_ptr() + GUARD, some.data_ptr() + GUARD)
    dev.sync()
    r, s = resp.cpu().numpy(), some.cpu().numpy()
    g = GUARD // 8
    assert (r[:g] == -7).all() and (r[g + w:] == -7).all() and (s[:GUARD] == 9).all() and (s[GUARD + w:] == 9).all()
    return a, b, r[g:g + w].view(np.uint64), s[GUARD:GUARD + w]


def _replay(dev, model, recs, path):
    """one chunk of the stream through the device and the model; every response compared"""
    want_r, want_s = model.replay(recs)
    a, b = 0, len(recs)
    if path == "fused_round":
        resp, some = _round(dev, recs)
    elif path == "window":
        a, b, resp, some = _window(dev, recs)
    else:
        first = dev.log_append(recs, 1)
        resp, some = dev.log_exec(first, first + len(recs))
    assert np.array_equal(some, want_s[a:b]), np.flatnonzero(some != want_s[a:b])[:8]
    assert np.array_equal(resp, want_r[a:b]), np.flatnonzero(resp != want_r[a:b])[:8]


def _queries(model, seed):
    rng = np.random.default_rng(seed)
    ks = model.keys
    pick = [ks[i] for i in rng.integers(0, len(ks), 300)] if ks else []
    pick += ks[:3] + ks[-3:] + R.BASE_KEYS[::97] + R.DELTA_KEYS[::17] + [R.absent(i) for i in range(0, 3000, 61)]
    q = set(pick) | {k + 1 for k in pick if k < U64_MAX} | {k - 1 for k in pick if k > 0} | {0, 1, U64_MAX, U64_MAX - 1}
    return np.array(sorted(q), np.uint64)


def _check(nrg, dev, model, seed=0):
    """Get, the four seeks, scans in both directions, range counts, dump, len and digest"""
    L = nrg._lib
    k, v = dev.sl_dump()
    mk, mv = model.arrays()
    assert np.array_equal(k, mk) and np.array_equal(v, mv)
    assert dev.sl_len() == len(model)
    assert dev.digest() == model.digest() == nrg.digest.skiplist(mk, mv)
    q = _queries(model, seed)
    ql = q.tolist()
    val, f = dev.sl_get(q)
    want = [model.get(x) for x in ql]
    assert f.tolist() == [int(w is not None) for w in want] and val.tolist() == [w or 0 for w in want]
    for mode in (L.NRG_SEEK_GE, L.NRG_SEEK_GT, L.NRG_SEEK_LE, L.NRG_SEEK_LT):
        ok, ov, fo = dev.sl_seek(q, mode)
        want = [model.seek(x, mode) for x in ql]
        assert fo.tolist() == [int(w is not None) for w in want], mode
        assert ok.tolist() == [w[0] if w else 0 for w in want] and ov.tolist() == [w[1] if w else 0 for w in want], mode
        sk, sv, cnt = dev.sl_scan(q[::4], mode, 6)
        for x, kr, vr, c in zip(ql[::4], sk, sv, cnt):
            assert list(zip(kr[:c].tolist(), vr[:c].tolist())) == model.scan(x, mode, 6), (mode, x)
    rng = np.random.default_rng(seed + 1)
    los, his = rng.choice(q, 200), rng.choice(q, 200)
    los[:2], his[:2] = [0, U64_MAX], [U64_MAX, 0]
    assert dev.sl_range_count(los, his).tolist() == [model.range_count(a, b) for a, b in zip(los.tolist(), his.tolist())]


def _check_launches(dev, model):
    assert dev.kernel_time("sl_drop_base")[0] == model.base_drops
    assert dev.kernel_time("sl_drop_delta")[0] == model.delta_drops
    assert dev.kernel_time("sl_compact")[0] == model.compactions


STREAMS = [n for n in R.NAMES if not R.by_name(n).error]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", STREAMS)
def test_streams_through_every_replay_path(nrg, name, path):
    s = R.by_name(name)
    dev, model = _open(nrg, s, max_batch=1024 if path == "chunked" else None)
    dev.kernel_timing(True)
    for i, recs in enumerate(s.chunks):
        _replay(dev, model, recs, path)
        assert dev.sl_len() == len(model), i
        if len(model) == 0:  # the empty map: seeks find nothing
            _check(nrg, dev, model, i)
    _check(nrg, dev, model)
    _check_launches(dev, model)
    dev.close()


def test_capacity_rule_in_one_chunk_latches(nrg):
    """a full map, then Remove(a) + Push(new b) in one chunk: b is admitted against the count before
    the chunk's removals, so NRG_E_CAPACITY is latched (the chunk after would have had the room)"""
    L = nrg._lib
    s = R.by_name("capacity_same_chunk")
    dev, model = _open(nrg, s)
    _replay(dev, model, s.chunks[0], "fused_round")
    assert dev.sl_len() == dev.sl_capacity() == 1024
    dev.sl_round_device(_cuda(s.chunks[1]), len(s.chunks[1]), 1)
    with pytest.raises(nrg.NrgError) as e:
        dev.sync()
    assert e.value.code == L.NRG_E_CAPACITY
    dev.sync()  # latched once
    model.replay(s.chunks[1])
    assert model.capacity_errors == 1 and dev.sl_len() == len(model) == 1023
    assert dev.sl_get([30, 31])[1].tolist() == [0, 0]
    dev.close()


@pytest.mark.parametrize("enabled", [True, False])
def test_snapshot_restore_into_a_fresh_context(nrg, enabled):
    s = R.by_name("sort_arms")
    src, model = _open(nrg, s)
    for recs in s.chunks:
        _replay(src, model, recs, "fused_round")
    img = src.snapshot()
    dst, _ = _open(nrg, s, enable=enabled)
    dst.restore(img)
    assert dst.digest() == src.digest() == model.digest()
    (k, v), (mk, mv) = dst.sl_dump(), model.arrays()
    assert np.array_equal(k, mk) and np.array_equal(v, mv) and dst.sl_len() == len(model)
    assert dst.sl_removal() == (R.TOMB if enabled else None)  # an image does not carry the setting
    if enabled:  # and the restored replica goes on removing
        dmodel = s.model()
        dmodel.restore(model.items())
        more = R._removes(mk[::5].tolist() + [R.absent(9999)])
        _replay(dst, dmodel, more, "append_exec")
        _check(nrg, dst, dmodel)
    src.close()
    dst.close()


def _view(nrg, h):
    d = nrg.DeviceReplica.__new__(nrg.DeviceReplica)
    d.kind, d.device, d._h, d._lib = nrg._lib.NRG_DS_SKIPLIST, 0, C.c_void_p(h), nrg._lib.load()
    return d


def _group(nrg, s, G):
    L = nrg._lib
    lib = L.load()
    cfg = L.default_config(L.NRG_DS_SKIPLIST)
    cfg.log2_slots, cfg.max_batch, cfg.log_bytes, cfg.max_reads = s.log2, s.max_batch, LOG_BYTES, 1 << 12
    L.check(lib.nrg_test_loopback_collectives(1))
    g = C.c_void_p()
    try:
        L.check(lib.nrg_group_open((C.c_int * G)(*([0] * G)), G, C.byref(cfg), C.byref(g)), "nrg_group_open")
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))
    members = [_view(nrg, lib.nrg_group_replica(g, i)) for i in range(G)]
    for m in members:
        L.check(lib.nrg_test_set_knob(m._h, L.KNOBS["SL_DELTA_MAX"], s.delta_max))
    return lib, g, members


@pytest.mark.parametrize("name", ["sort_arms", "drop_edges", "alternate_600"])
def test_replicated_group_of_two(nrg, name):
    """both members enabled; a chunk is split between the members' segments (the global log is W_0 || W_1)"""
    import torch

    L = nrg._lib
    s = R.by_name(name)
    lib, g, members = _group(nrg, s, 2)
    model = s.model()
    keep = []
    try:
        for m in members:
            m.sl_enable_removal()
        for r, recs in enumerate(s.chunks):
            cut = (len(recs) * (1 + r % 3)) // 4
            want_r, want_s = model.replay(recs)
            rd = (L.Round * 2)()
            outs = []
            for i, part in enumerate((recs[:cut], recs[cut:])):
                n = len(part)
                d_ops = _cuda(part) if n else None
                resp = torch.zeros(max(n, 1), dtype=torch.int64, device="cuda")
                some = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
                rd[i].recs, rd[i].n, rd[i].resp, rd[i].some = (d_ops.data_ptr() if n else 0), n, resp.data_ptr(), some.data_ptr()
                keep.append((d_ops, resp, some))
                outs.append((resp, some, n))
            torch.cuda.synchronize()
            L.check(lib.nrg_group_round_async(g, rd, None), f"round {r}")
            L.check(lib.nrg_group_sync(g))
            got_r = np.concatenate([o[0].cpu().numpy().view(np.uint64)[:o[2]] for o in outs])
            got_s = np.concatenate([o[1].cpu().numpy()[:o[2]] for o in outs])
            assert np.array_equal(got_s, want_s) and np.array_equal(got_r, want_r), r
            same = C.c_int(-1)
            L.check(lib.nrg_group_verify(g, None, C.byref(same)))
            assert same.value == 1
        for m in members:
            _check(nrg, m, model)
    finally:
        for m in members:
            m._h = None
        assert lib.nrg_group_close(g) == L.NRG_OK


def test_a_context_without_removal_is_as_before(nrg):
    """{k, 2^64 - 1} is an ordinary Push, and a stream's replay launches none of the new kernels"""
    import skiplist_model as M

    s = R.by_name("sort_arms")
    dev, _ = _open(nrg, s, enable=False)  # (nothing of the removal API is used here: this passes without it)
    model = M.SkipListModel(s.delta_max, s.max_batch)
    dev.kernel_timing(True)
    for recs in s.chunks:
        resp, some = _round(dev, recs)
        model.replay(recs)
        assert np.array_equal(resp, recs["key"]) and (some == 1).all()
    k, v = dev.sl_dump()
    mk, mv = model.arrays()
    assert np.array_equal(k, mk) and np.array_equal(v, mv) and dev.digest() == model.digest()
    assert (v == U64_MAX).sum() > 100  # the tombstone of the enabled contexts, stored as a value here
    probe = int(mk[np.flatnonzero(mv == U64_MAX)[0]])
    assert dev.sl_get([probe])[0].tolist() == [U64_MAX] and dev.sl_get([probe])[1].tolist() == [1]
    for name in NEW_KERNELS:
        assert dev.kernel_time(name)[0] == 0, name
    assert dev.kernel_time("sl_compact")[0] == model.compactions and dev.kernel_time("sl_resolve")[0] == len(s.chunks)
    dev.close()


def test_no_drop_pass_without_a_hit(nrg):
    """an enabled context: a chunk with no tombstone, and a chunk whose Removes all miss, drop nothing"""
    s = R.by_name("absent")
    dev, model = _open(nrg, s)
    dev.kernel_timing(True)
    for recs in s.chunks[:2]:  # the setup: Pushes only
        _replay(dev, model, recs, "fused_round")
    assert dev.kernel_time("sl_rm_state")[0] == 2  # the readback is per chunk
    _replay(dev, model, s.chunks[2], "fused_round")
    assert dev.kernel_time("sl_rm_resp")[0] == 3 and dev.kernel_time("sl_merge")[0] == 3
    assert dev.kernel_time("sl_drop_base")[0] == 0 and dev.kernel_time("sl_drop_delta")[0] == 0
    _check(nrg, dev, model)
    dev.close()


def test_prefill_and_sl_remove(nrg):
    """prefill runs the same pipeline: a tombstone value is a Remove there too; DeviceReplica.sl_remove"""
    s = R.by_name("base_every_third")
    dev, model = _open(nrg, s)
    keys = np.array(R.BASE_KEYS[:500] + R.BASE_KEYS[:500:2], np.uint64)
    vals = np.concatenate([np.arange(500, dtype=np.uint64), np.full(250, U64_MAX, np.uint64)])
    dev.sl_prefill(keys, vals)
    model.insert_many(keys.tolist(), vals.tolist())
    _check(nrg, dev, model)
    assert len(model) == 250
    gone = [R.BASE_KEYS[1], R.BASE_KEYS[0], R.BASE_KEYS[1], 7]
    prev, found = dev.sl_remove(gone)
    want_r, want_s = model.replay(R._removes(gone))
    assert prev.tolist() == want_r.tolist() == [1, 0, 0, 0] and found.tolist() == want_s.tolist() == [1, 0, 0, 0]
    _check(nrg, dev, model)
    dev.close()


def test_guards(nrg):
    import torch

    L = nrg._lib
    lib = L.load()
    s = R.by_name("absent")
    dev, model = _open(nrg, s, enable=False)
    t, on = C.c_uint64(5), C.c_int(5)
    assert lib.nrg_skiplist_removal(dev._h, C.byref(t), C.byref(on)) == L.NRG_OK and (t.value, on.value) == (0, 0)
    with pytest.raises(nrg.NrgError) as e:
        dev.sl_remove([1])  # not before removal is enabled
    assert e.value.code == L.NRG_E_INVAL and dev.log_state()["tail"] == 0
    dev.log_append(R.recs_of([1], [2]), 1)
    assert lib.nrg_skiplist_enable_removal(dev._h, R.TOMB) == L.NRG_E_NOT_SYNCED and dev.sl_removal() is None
    dev.log_exec()
    assert lib.nrg_skiplist_enable_removal(dev._h, R.TOMB) == L.NRG_OK
    assert lib.nrg_skiplist_enable_removal(dev._h, R.TOMB) == L.NRG_OK  # again, the same tombstone
    assert lib.nrg_skiplist_enable_removal(dev._h, 0) == L.NRG_E_INVAL
    assert lib.nrg_skiplist_removal(dev._h, C.byref(t), C.byref(on)) == L.NRG_OK and (t.value, on.value) == (R.TOMB, 1)
    comb = C.c_void_p()
    assert lib.nrg_combiner_open(dev._h, 4, C.byref(comb)) == L.NRG_E_INVAL
    dev.close()
    # another kind
    st = nrg.DeviceReplica(L.NRG_DS_STACK, 0, stack_capacity=1 << 10, max_batch=1024, log_bytes=LOG_BYTES)
    assert lib.nrg_skiplist_enable_removal(st._h, R.TOMB) == L.NRG_E_INVAL
    assert lib.nrg_skiplist_removal(st._h, C.byref(t), C.byref(on)) == L.NRG_E_INVAL
    st.close()
    # a partitioned round with an enabled member: refused in the local check, nothing written, no log movement
    lib, g, members = _group(nrg, s, 1)
    try:
        m = members[0]
        recs = R.recs_of([1, 2, 3], [4, 5, R.TOMB])
        d_ops = _cuda(recs)
        resp = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        some = torch.full((3,), 7, dtype=torch.uint8, device="cuda")
        rd = (L.Round * 1)()
        rd[0].recs, rd[0].n, rd[0].resp, rd[0].some = d_ops.data_ptr(), 3, resp.data_ptr(), some.data_ptr()
        torch.cuda.synchronize()
        L.check(lib.nrg_group_partitioned_round(g, rd), "before removal")
        L.check(lib.nrg_group_sync(g))
        assert some.cpu().tolist() == [1, 1, 1] and m.sl_len() == 3  # (2^64 - 1 was a value)
        m.sl_enable_removal()
        before = m.log_state()
        resp.fill_(-1)
        some.fill_(7)
        torch.cuda.synchronize()
        assert lib.nrg_group_partitioned_round(g, rd) == L.NRG_E_INVAL
        # (the pipelined form reports a round's argument errors where the round completes)
        rcs = (lib.nrg_group_partitioned_round_async(g, rd), lib.nrg_group_partitioned_flush(g))
        assert rcs in ((L.NRG_E_INVAL, L.NRG_OK), (L.NRG_OK, L.NRG_E_INVAL)), rcs
        L.check(lib.nrg_group_sync(g))
        assert m.log_state() == before and m.sl_len() == 3
        assert (resp.cpu().numpy() == -1).all() and (some.cpu().numpy() == 7).all()
    finally:
        for m in members:
            m._h = None
        assert lib.nrg_group_close(g) == L.NRG_OK


def test_python_replica_api(nrg):
    """SlPush / SlRemove / Get / Scan on two replicas of one log agree with the model"""
    L = nrg._lib
    log = nrg.Log(LOG_BYTES)
    a = nrg.Replica(log, nrg.SkipList, 0, log2_slots=12, max_batch=1024)
    b = nrg.Replica(log, nrg.SkipList, 0, log2_slots=12, max_batch=1024)
    for r in (a, b):
        r.dev.sl_enable_removal()
    ta, tb = a.register(), b.register()
    model = R.SkipListRemoveModel()
    rng = np.random.default_rng(15)
    for i in range(80):
        k = int(rng.integers(0, 25)) * 10
        rep, tok = (a, ta) if i % 2 else (b, tb)
        if rng.random() < 0.4:
            got = rep.execute_mut(nrg.SlRemove(k), tok)
            resp, some = model.replay([(k, R.TOMB)])
            assert got == (int(resp[0]) if some[0] else None), i
        else:
            v = int(rng.integers(0, U64_MAX, dtype=np.uint64))
            assert rep.execute_mut(nrg.SlPush(k, v), tok) == k
            model.replay([(k, v)])
    for rep, tok in ((a, ta), (b, tb)):
        for k in (0, 5, 10, 240, 250, U64_MAX):
            assert rep.execute(nrg.Get(k), tok) == model.get(k)
            for mode in (L.NRG_SEEK_GE, L.NRG_SEEK_LT):
                assert rep.execute(nrg.Scan(k, mode, 5), tok) == model.scan(k, mode, 5)
    seen = []
    a.verify(seen.append)
    b.verify(seen.append)
    assert seen[0] == seen[1] == model.items() and a.digest() == b.digest() == model.digest()
    c = nrg.Replica(log, nrg.SkipList, 0, log2_slots=10, max_batch=1024, clone_from=a)
    assert c.dev.sl_removal() == R.TOMB  # the clone takes the peer's setting
    c.verify(seen.append)
    assert seen[2] == model.items()
    for r in (a, b, c):
        r.dev.close()
