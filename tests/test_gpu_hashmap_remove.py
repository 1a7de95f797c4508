"""Removal of keys from the replicated hashmap (nrg_hashmap_enable_removal, csrc/hashmap.hip) against
the sequential model of tests/hashmap_remove_model.py: every response, Get, size, occupancy, dump and
digest is compared bit for bit, and the launch counts say which schedule ran; there are no tolerances.
The oracle has no Remove, so the model is the reference; tests/test_hashmap_remove_cpu.py checks it against
a plain dict and shows that every named stream reaches the arm it is named for."""
import ctypes as C

import numpy as np
import pytest

import hashmap_remove_model as R
import hashmap_streams as S

pytestmark = pytest.mark.gpu

U64 = np.uint64
LOG_BYTES = 64 * 2 * 8192
PATHS = ["append_exec", "fused_round", "chunked", "window"]
CHUNKED_BATCH = 500  # the chunked path's max_batch: smaller than the streams' larger rounds
GUARD = 64           # bytes of guard words around a response window
MARK = -0x5A5A5A5A5A5A5A5B


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def _open(nrg, st, max_batch=None, enable=True, knobs=None, **kw):
    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_HASHMAP, 0, knobs=knobs or {}, log2_slots=st.log2_slots,
                            hashmap_max_log2_slots=st.max_log2, max_batch=max_batch or st.max_batch,
                            log_bytes=LOG_BYTES, **kw)
    dev.kernel_timing(True)
    if enable:
        dev.hm_enable_removal(st.tomb)
    return dev, st.model(max_batch)


def _fused(dev, recs, gets, want_prev=True):
    """nrg_hashmap_round_async on device buffers: (prev, found, get vals, get found)"""
    import torch

    W, G = len(recs), len(gets)
    d_recs, d_gk = _cuda(recs), _cuda(gets) if G else None
    gv = torch.full((max(G, 1),), MARK, dtype=torch.int64, device="cuda")
    gf = torch.full((max(G, 1),), 7, dtype=torch.uint8, device="cuda")
    pv = torch.full((max(W, 1),), MARK, dtype=torch.int64, device="cuda") if want_prev else None
    pf = torch.full((max(W, 1),), 7, dtype=torch.uint8, device="cuda") if want_prev else None
    dev.hm_round_device(d_recs, W, 1, d_gk, G, gv if G else None, gf if G else None, pv, pf)
    dev.sync()
    prev = (pv.cpu().numpy().view(U64)[:W], pf.cpu().numpy()[:W]) if want_prev else (None, None)
    return prev[0], prev[1], gv.cpu().numpy().view(U64)[:G], gf.cpu().numpy()[:G]


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
    return a, b, r[g:g + w].view(U64), s[GUARD:GUARD + w]


def _replay(dev, model, recs, gets, path, tag=""):
    """one round of a stream through the device and the model; every response and Get compared"""
    want_p, want_f = model.replay(recs)
    want_gv, want_gf = model.get_batch(gets)
    a, b = 0, len(recs)
    if path == "fused_round":
        prev, found, gv, gf = _fused(dev, recs, gets)
    else:
        if path == "window":
            a, b, prev, found = _window(dev, recs)
        else:
            first = dev.log_append(recs, 1)
            prev, found = dev.log_exec(first, first + len(recs))
        gv, gf = dev.hm_get(gets)
    assert np.array_equal(found, want_f[a:b]), (tag, np.flatnonzero(found != want_f[a:b])[:8])
    assert np.array_equal(prev, want_p[a:b]), (tag, np.flatnonzero(prev != want_p[a:b])[:8])
    assert np.array_equal(gf, want_gf), (tag, np.flatnonzero(gf != want_gf)[:8])
    assert np.array_equal(gv, want_gv), (tag, np.flatnonzero(gv != want_gv)[:8])


def _check(nrg, dev, model):
    """size, occupancy, dump (as a set), digest"""
    k, v = dev.hm_dump()
    mk, mv = model.arrays()
    assert np.array_equal(k, mk) and np.array_equal(v, mv)
    assert dev.hm_size() == len(model)
    assert dev.hm_occupancy() == model.occupancy
    assert dev.digest() == model.digest() == nrg.digest.pairs(mk, mv)


def _launches(dev):
    return {k: dev.kernel_time(k)[0] for k in ("hm_papply", "hm_small", "hm_round", "hm_rehash")}


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", R.NAMES)
def test_streams_through_every_replay_path(nrg, name, path):
    st = R.by_name(name)
    mb = CHUNKED_BATCH if path == "chunked" else None
    dev, model = _open(nrg, st, max_batch=mb)
    chunks = 0
    for i, (recs, gets) in enumerate(st.rounds):
        _replay(dev, model, recs, gets, path, (name, i))
        chunks += -(-len(recs) // (mb or st.max_batch))
        assert dev.hm_size() == len(model) and dev.hm_occupancy() == model.occupancy, i
    _check(nrg, dev, model)
    got = _launches(dev)
    # one schedule: every chunk is a partition round with one apply launch; nothing else ever runs
    assert (got["hm_papply"], got["hm_small"], got["hm_rehash"]) == (chunks, 0, 0), got
    dev.close()


def test_never_claims_keeps_the_table(nrg):
    """5000 Removes of absent keys against a fixed 256-slot table holding 100 keys"""
    st = R.by_name("never_claims")
    dev, model = _open(nrg, st)
    for recs, gets in st.rounds:
        _replay(dev, model, recs, gets, "append_exec")
    assert dev.hm_occupancy() == dev.hm_size() == 100 and dev.hm_log2_slots() == 8
    dev.sync()  # no error latched
    v, f = dev.hm_get(st.claims["live"])
    assert f.all() and np.array_equal(v, model.get_batch(st.claims["live"])[0])
    dev.close()


def test_revival_across_an_epoch_renormalisation(nrg):
    """a dead key stays absent when the stamps are renormalised (NRG_KNOB_EPOCH_LIMIT), and is revived after"""
    st = R.by_name("revival")
    dev, model = _open(nrg, st, knobs={"EPOCH_LIMIT": 3})  # every second round renormalises
    a = st.claims["a"]
    for i, (recs, gets) in enumerate(st.rounds[:2]):
        _replay(dev, model, recs, gets, "fused_round", i)
    for i in range(4):  # rounds that do not touch the dead keys, across renormalisations
        idle = R.recs_of(a[150:160], S.mix64(np.arange(10, dtype=U64) + U64(1000 * i + 5)))
        _replay(dev, model, idle, a[:130], "fused_round", ("idle", i))
    occ = dev.hm_occupancy()
    for i, (recs, gets) in enumerate(st.rounds[2:]):
        _replay(dev, model, recs, gets, "fused_round", i + 2)
    assert dev.hm_occupancy() == occ == 200  # the slots were reused
    _check(nrg, dev, model)
    dev.close()


def test_schedule_of_an_enabled_context(nrg):
    """every round, a one-record round included, is a partition round: hm_papply once, no small round,
    whatever the knobs say; with or without responses, with or without Gets"""
    st = R.by_name("sizes_1")
    dev, model = _open(nrg, st, knobs={"SMALL_MAX": 2048, "PART": 0})
    want = 0
    for recs, gets in st.rounds:
        for want_prev, g in ((True, gets), (False, gets), (False, gets[:0])):
            p, f, gv, gf = _fused(dev, recs, g, want_prev)
            mp, mf = model.replay(recs)
            if want_prev:
                assert np.array_equal(p, mp) and np.array_equal(f, mf)
            if len(g):
                assert np.array_equal(gv, model.get_batch(g)[0]) and np.array_equal(gf, model.get_batch(g)[1])
            want += 1
            got = _launches(dev)
            assert (got["hm_papply"], got["hm_small"]) == (want, 0), got
    _check(nrg, dev, model)
    dev.close()


def test_a_context_without_removal_is_as_before(nrg, orc):
    """{k, 2^64 - 1} is an ordinary Put, and a stamp round, a partition round and a small round launch
    what they always launched (this passes without the feature, and that is its point). The counts are
    the parent commit's, measured there with this sequence: three rounds, each one hm_round launch for
    the round and, at the sync that follows, one for its deferred half (a small round defers nothing)."""
    st = R.by_name("sizes_513")
    for knobs, want_prev, want in (({"PART": 0}, False, dict(hm_papply=0, hm_small=0, hm_round=6, hm_rehash=0)),
                                   ({"PART": 2}, False, dict(hm_papply=3, hm_small=0, hm_round=6, hm_rehash=0)),
                                   ({}, True, dict(hm_papply=3, hm_small=0, hm_round=6, hm_rehash=0)),
                                   ({"SMALL_MAX": 2048}, True, dict(hm_papply=0, hm_small=3, hm_round=0, hm_rehash=0))):
        dev = nrg.DeviceReplica(nrg._lib.NRG_DS_HASHMAP, 0, knobs=knobs, log2_slots=st.log2_slots, max_batch=4096,
                                log_bytes=LOG_BYTES)
        dev.kernel_timing(True)
        om = orc.HashMap()
        for r, g in st.rounds:
            p, f, gv, gf = _fused(dev, r, g, want_prev)
            mp, mf = om.replay(r["key"], r["val"])
            if want_prev:
                assert np.array_equal(p, mp) and np.array_equal(f, mf.astype(np.uint8))
            ev, ef = om.get_batch(g)
            assert np.array_equal(gv, ev) and np.array_equal(gf, ef.astype(np.uint8))
        assert _launches(dev) == want, knobs
        k, v = dev.hm_dump()
        assert (v == R.TOMB).sum() > 100  # the tombstone of the enabled contexts, stored as a value here
        assert dev.hm_size() == len(om) and dev.hm_digest() == tuple(int(x) for x in om.digest())
        assert _launches(dev) == want, knobs  # (size, dump and digest find nothing deferred)
        dev.close()


def _churn(nrg, st, purge_every=0):
    """the churn stream; (device, model, first round at which NRG_E_TABLE_FULL was latched or None)"""
    dev, model = _open(nrg, st)
    for i, (recs, gets) in enumerate(st.rounds):
        try:
            _fused(dev, recs, gets[:0], want_prev=False)
        except nrg.NrgError as e:
            assert e.code == nrg._lib.NRG_E_TABLE_FULL
            return dev, model, i
        model.replay(recs)
        if purge_every and (i + 1) % purge_every == 0:
            dev.hm_purge()
            model.purge()
            assert dev.hm_occupancy() == dev.hm_size() == len(model)
    return dev, model, None


def test_churn_purges_a_growing_table_instead_of_growing_it(nrg):
    st = R.churn(10)
    dev, model, full = _churn(nrg, st)
    assert full is None and model.full == 0
    assert dev.hm_log2_slots() == model.log2 == 8
    assert dev.kernel_time("hm_rehash")[0] == model.purges >= 1 and model.grows == 0
    _check(nrg, dev, model)
    dev.close()


def test_growth_with_dead_slots_drops_them(nrg):
    """hm_room's grow branch on an enabled context: the target is larger than the table while dead slots
    are there (twice: 2^8 -> 2^9 -> 2^10). The rehash drops them, and the bound afterwards is live + n:
    the round after each grow decides as the model does (no count, no rehash)."""
    st = R.grow_with_dead()
    dev, model = _open(nrg, st)
    sizes = []
    for i, (recs, gets) in enumerate(st.rounds):
        _replay(dev, model, recs, gets, "fused_round", i)
        sizes.append(dev.hm_log2_slots())
        assert sizes[-1] == model.log2 and dev.kernel_time("hm_rehash")[0] == model.grows + model.purges, i
        assert dev.hm_size() == len(model) and dev.hm_occupancy() == model.occupancy, i
    assert sizes == [8, 8, 9, 9, 9, 10, 10] and (model.grows, model.purges) == (2, 0)
    _check(nrg, dev, model)
    dev.sync()  # no error
    dev.close()


def test_churn_fills_a_fixed_table_unless_it_is_purged(nrg):
    dev, model, full = _churn(nrg, R.churn(0, rounds=4))
    assert full is not None and 16 <= full < 24  # the third hundred of keys does not fit 256 slots
    dev.sync()  # latched once
    assert dev.kernel_time("hm_rehash")[0] == 0
    dev.close()
    dev, model, full = _churn(nrg, R.churn(0, rounds=8, purge_every=8), purge_every=8)
    assert full is None and dev.kernel_time("hm_rehash")[0] == model.purges >= 4
    _check(nrg, dev, model)
    before = _launches(dev)
    dev.hm_purge()  # nothing dead: nothing launched
    assert _launches(dev) == before
    dev.close()


@pytest.mark.parametrize("enabled", [True, False])
def test_snapshot_holds_live_pairs_only(nrg, enabled):
    st = R.by_name("present_absent_dead")
    src, model = _open(nrg, st)
    for recs, gets in st.rounds:
        _replay(src, model, recs, gets, "fused_round")
    assert src.hm_occupancy() > src.hm_size() > 0
    img = src.snapshot()
    info, (ik, iv) = nrg.snapshot.unpack(img)
    assert info.items == len(model) and not (iv == U64(st.tomb)).any()  # live pairs only
    dst, _ = _open(nrg, st, enable=enabled)
    dst.restore(img)
    assert dst.digest() == src.digest() == model.digest()
    k, v = dst.hm_dump()
    mk, mv = model.arrays()
    assert np.array_equal(k, mk) and np.array_equal(v, mv) and dst.hm_size() == dst.hm_occupancy() == len(model)
    assert dst.hm_removal() == (st.tomb if enabled else None)  # an image does not carry the setting
    src.close()
    dst.close()


def test_restore_refuses_an_image_with_the_tombstone_as_a_value(nrg):
    st = R.by_name("revival")
    plain = nrg.DeviceReplica(nrg._lib.NRG_DS_HASHMAP, 0, log2_slots=10, max_batch=4096, log_bytes=LOG_BYTES)
    plain.hm_prefill(np.arange(1, 50, dtype=U64), np.where(np.arange(1, 50) == 17, U64(R.TOMB), U64(5)))
    img = plain.snapshot()
    dst, model = _open(nrg, st)
    _replay(dst, model, *st.rounds[0], "fused_round")
    before = dst.log_state()
    with pytest.raises(nrg.NrgError) as e:
        dst.restore(img)
    assert e.value.code == nrg._lib.NRG_E_INVAL and dst.log_state() == before
    _check(nrg, dst, model)  # unchanged
    off, _ = _open(nrg, st, enable=False)
    off.restore(img)  # a context that never enabled takes it
    assert off.digest() == plain.digest()
    for d in (plain, dst, off):
        d.close()


def _view(nrg, h):
    d = nrg.DeviceReplica.__new__(nrg.DeviceReplica)
    d.kind, d.device, d._h, d._lib = nrg._lib.NRG_DS_HASHMAP, 0, C.c_void_p(h), nrg._lib.load()
    return d


def _group(nrg, log2, G):
    L = nrg._lib
    lib = L.load()
    cfg = L.default_config(L.NRG_DS_HASHMAP)
    cfg.log2_slots, cfg.max_batch, cfg.log_bytes, cfg.max_reads = log2, 4096, LOG_BYTES, 1 << 12
    L.check(lib.nrg_test_loopback_collectives(1))
    g = C.c_void_p()
    try:
        L.check(lib.nrg_group_open((C.c_int * G)(*([0] * G)), G, C.byref(cfg), C.byref(g)), "nrg_group_open")
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))
    return lib, g, [_view(nrg, lib.nrg_group_replica(g, i)) for i in range(G)]


def _group_round(nrg, lib, g, parts, gets, partitioned=False):
    """one round of two members; their responses and Gets"""
    import torch

    L = nrg._lib
    rd = (L.Round * 2)()
    keep = []
    for i, (part, gk) in enumerate(zip(parts, gets)):
        n, G = len(part), len(gk)
        t = dict(r=_cuda(part) if n else None, k=_cuda(gk) if G else None,
                 pv=torch.full((max(n, 1),), MARK, dtype=torch.int64, device="cuda"),
                 pf=torch.full((max(n, 1),), 7, dtype=torch.uint8, device="cuda"),
                 gv=torch.full((max(G, 1),), MARK, dtype=torch.int64, device="cuda"),
                 gf=torch.full((max(G, 1),), 7, dtype=torch.uint8, device="cuda"))
        rd[i].recs, rd[i].n = (t["r"].data_ptr() if n else 0), n
        rd[i].resp, rd[i].some = t["pv"].data_ptr(), t["pf"].data_ptr()
        rd[i].get_keys, rd[i].n_gets = (t["k"].data_ptr() if G else 0), G
        rd[i].get_vals, rd[i].get_found = t["gv"].data_ptr(), t["gf"].data_ptr()
        keep.append((t, n, G))
    torch.cuda.synchronize()
    if partitioned:
        L.check(lib.nrg_group_partitioned_round(g, rd), "partitioned round")
    else:
        L.check(lib.nrg_group_round_async(g, rd, None), "round")
    L.check(lib.nrg_group_sync(g))
    return [(t["pv"].cpu().numpy().view(U64)[:n], t["pf"].cpu().numpy()[:n], t["gv"].cpu().numpy().view(U64)[:G],
             t["gf"].cpu().numpy()[:G]) for t, n, G in keep]


def test_replicated_group_of_two_and_resync(nrg):
    """Removes from both members in one replicated round (the global log is W_0 || W_1), verify, and a
    resync after member 1 diverges"""
    import torch

    L = nrg._lib
    st = R.by_name("present_absent_dead")
    lib, g, members = _group(nrg, st.log2_slots, 2)
    model = st.model()
    try:
        for m in members:
            m.hm_enable_removal(st.tomb)
        for r, (recs, gets) in enumerate(st.rounds):
            cut = (len(recs) * (1 + r % 3)) // 4
            want_p, want_f = model.replay(recs)
            want_gv, want_gf = model.get_batch(gets)
            out = _group_round(nrg, lib, g, (recs[:cut], recs[cut:]), (gets, gets[::2]))
            assert np.array_equal(np.concatenate([out[0][1], out[1][1]]), want_f), r
            assert np.array_equal(np.concatenate([out[0][0], out[1][0]]), want_p), r
            assert np.array_equal(out[0][2], want_gv) and np.array_equal(out[0][3], want_gf), r
            assert np.array_equal(out[1][2], want_gv[::2]) and np.array_equal(out[1][3], want_gf[::2]), r
            same = C.c_int(-1)
            L.check(lib.nrg_group_verify(g, None, C.byref(same)))
            assert same.value == 1
        for m in members:
            _check(nrg, m, model)
        # member 1 alone removes a live key: the digests differ until it is resynced from member 0
        live = int(model.arrays()[0][0])
        d_op = _cuda(R.recs_of([live], [st.tomb]))
        torch.cuda.synchronize()
        L.check(lib.nrg_hashmap_round_async(members[1]._h, d_op.data_ptr(), 1, 2, None, 0, None, None, None, None))
        members[1].sync()
        assert members[1].hm_size() == len(model) - 1
        same = C.c_int(-1)
        L.check(lib.nrg_group_verify(g, None, C.byref(same)))
        assert same.value == 0
        L.check(lib.nrg_group_resync(g, 0))
        L.check(lib.nrg_group_verify(g, None, C.byref(same)))
        assert same.value == 1 and members[1].hm_removal() == st.tomb
        for m in members:
            _check_live(nrg, m, model)
        assert members[1].hm_occupancy() == len(model)  # a restored table holds no dead slot
    finally:
        for m in members:
            m._h = None
        assert lib.nrg_group_close(g) == L.NRG_OK


def _check_live(nrg, dev, model):
    k, v = dev.hm_dump()
    mk, mv = model.arrays()
    assert np.array_equal(k, mk) and np.array_equal(v, mv) and dev.hm_size() == len(model)
    assert dev.digest() == model.digest()


def test_partitioned_round_carries_removes(nrg):
    """one key-partitioned round with Removes and Gets from both members: an owner replays member 0's
    records, then member 1's, and the Gets see the round; a Remove's answer travels as a previous value"""
    L = nrg._lib
    lib, g, members = _group(nrg, 10, 2)
    model = R.HashMapRemoveModel(10)
    try:
        for m in members:
            m.hm_enable_removal()
        keys = S.free_keys(300)
        vals = S.mix64(keys + U64(77))
        first = (R.recs_of(keys[:200], vals[:200]), R.recs_of(keys[100:300], vals[100:300]))
        rm = np.full(150, R.TOMB, U64)
        second = (R.recs_of(np.concatenate([keys[:100], S.absent_keys(50)]), rm),
                  R.recs_of(np.concatenate([keys[50:150], keys[250:300]]),
                            np.concatenate([rm[:100], vals[:50] + U64(1)])))
        for parts in (first, second):
            want = [model.replay(p) for p in parts]
            gets = (keys, np.concatenate([keys[::3], S.absent_keys(20)]))
            out = _group_round(nrg, lib, g, parts, gets, partitioned=True)
            for i in range(2):
                assert np.array_equal(out[i][1], want[i][1]) and np.array_equal(out[i][0], want[i][0]), i
                gv, gf = model.get_batch(gets[i])
                assert np.array_equal(out[i][3], gf) and np.array_equal(out[i][2], gv), i
        assert sum(m.hm_size() for m in members) == len(model) == 150
        assert nrg.digest.combine([m.digest() for m in members]) == model.digest()
    finally:
        for m in members:
            m._h = None
        assert lib.nrg_group_close(g) == L.NRG_OK


def test_prefill_and_hm_remove(nrg):
    """prefill on an enabled context: a tombstone value is refused, a dead key is revived with exact
    counts; DeviceReplica.hm_remove"""
    L = nrg._lib
    st = R.by_name("revival")
    dev, model = _open(nrg, st)
    dev.hm_prefill_range(100, 1)
    model.replay(R.recs_of(np.arange(100), np.arange(100) + 1))
    prev, found = dev.hm_remove(np.array([5, 6, 5, 1000], U64))
    want_p, want_f = model.replay(R.recs_of([5, 6, 5, 1000], [st.tomb] * 4))
    assert prev.tolist() == want_p.tolist() == [6, 7, 0, 0] and found.tolist() == want_f.tolist() == [1, 1, 0, 0]
    assert (dev.hm_size(), dev.hm_occupancy()) == (98, 100)
    dev.hm_prefill_range(50, 1)  # revives keys 5 and 6
    model.replay(R.recs_of(np.arange(50), np.arange(50) + 1))
    assert (dev.hm_size(), dev.hm_occupancy()) == (100, 100)
    dev.hm_remove([7])
    model.replay(R.recs_of([7], [st.tomb]))
    dev.hm_prefill(np.array([7, 2000], U64), np.array([70, 80], U64))  # through the replay: revives 7
    model.replay(R.recs_of([7, 2000], [70, 80]))
    assert (dev.hm_size(), dev.hm_occupancy()) == (101, 101)
    _check(nrg, dev, model)
    lib = L.load()
    k2, v2 = np.array([1, 2], U64), np.array([3, st.tomb], U64)
    assert lib.nrg_hashmap_prefill(dev._h, k2.ctypes.data_as(C.c_void_p), v2.ctypes.data_as(C.c_void_p), 2) == L.NRG_E_INVAL
    assert lib.nrg_hashmap_prefill_range(dev._h, 10, st.tomb - 3) == L.NRG_E_INVAL  # key 3 would get the tombstone
    _check(nrg, dev, model)
    dev.close()


def test_gating(nrg):
    """every error return of the removal entry points, each leaving the replica usable and unchanged"""
    L = nrg._lib
    lib = L.load()
    st = R.by_name("revival")
    dev, model = _open(nrg, st, enable=False)
    t, on = C.c_uint64(5), C.c_int(5)
    assert lib.nrg_hashmap_removal(dev._h, C.byref(t), C.byref(on)) == L.NRG_OK and (t.value, on.value) == (0, 0)
    with pytest.raises(nrg.NrgError) as e:
        dev.hm_remove([1])  # not before removal is enabled
    assert e.value.code == L.NRG_E_INVAL and dev.log_state()["tail"] == 0
    dev.hm_purge()  # removal off: nothing
    assert dev.kernel_time("hm_rehash")[0] == 0
    # a present value equals the tombstone: refused, the replica as it was
    dev.log_append(R.recs_of([1, 2], [2, 77]), 1)
    assert lib.nrg_hashmap_enable_removal(dev._h, R.TOMB) == L.NRG_E_NOT_SYNCED and dev.hm_removal() is None
    dev.log_exec()
    assert lib.nrg_hashmap_enable_removal(dev._h, 77) == L.NRG_E_INVAL and dev.hm_removal() is None
    assert dev.hm_get([1, 2])[0].tolist() == [2, 77] and dev.hm_size() == dev.hm_occupancy() == 2
    # a combiner is open: refused; closed: accepted; then the combiner is refused
    comb = C.c_void_p()
    assert lib.nrg_combiner_open(dev._h, 4, C.byref(comb)) == L.NRG_OK
    assert lib.nrg_hashmap_enable_removal(dev._h, R.TOMB) == L.NRG_E_INVAL and dev.hm_removal() is None
    assert lib.nrg_combiner_close(comb) == L.NRG_OK
    assert lib.nrg_hashmap_enable_removal(dev._h, R.TOMB) == L.NRG_OK
    assert lib.nrg_hashmap_enable_removal(dev._h, R.TOMB) == L.NRG_OK  # again, the same tombstone
    assert lib.nrg_hashmap_enable_removal(dev._h, 0) == L.NRG_E_INVAL
    assert lib.nrg_hashmap_removal(dev._h, C.byref(t), C.byref(on)) == L.NRG_OK and (t.value, on.value) == (R.TOMB, 1)
    assert lib.nrg_hashmap_removal(dev._h, None, None) == L.NRG_OK
    assert lib.nrg_combiner_open(dev._h, 4, C.byref(comb)) == L.NRG_E_INVAL
    assert lib.nrg_hashmap_occupancy(dev._h, None) == L.NRG_E_INVAL
    prev, found = dev.hm_remove([2, 3])  # usable
    assert prev.tolist() == [77, 0] and found.tolist() == [1, 0] and dev.hm_get([1, 2])[1].tolist() == [1, 0]
    dev.close()
    # another kind
    stk = nrg.DeviceReplica(L.NRG_DS_STACK, 0, stack_capacity=1 << 10, max_batch=1024, log_bytes=LOG_BYTES)
    assert lib.nrg_hashmap_enable_removal(stk._h, R.TOMB) == L.NRG_E_INVAL
    assert lib.nrg_hashmap_removal(stk._h, C.byref(t), C.byref(on)) == L.NRG_E_INVAL
    assert lib.nrg_hashmap_occupancy(stk._h, C.byref(t)) == L.NRG_E_INVAL
    assert lib.nrg_hashmap_purge(stk._h) == L.NRG_E_INVAL
    stk.close()


def test_python_replica_api(nrg):
    """Put / Remove / Get on two replicas of one log agree with a dict; a clone takes the setting"""
    log = nrg.Log(LOG_BYTES)
    a = nrg.Replica(log, nrg.NrHashMap, 0, log2_slots=10, max_batch=1024)
    b = nrg.Replica(log, nrg.NrHashMap, 0, log2_slots=10, max_batch=1024)
    for r in (a, b):
        r.dev.hm_enable_removal()
    ta, tb = a.register(), b.register()
    d = {}
    rng = np.random.default_rng(15)
    for i in range(80):
        k = int(rng.integers(0, 25)) * 10
        rep, tok = (a, ta) if i % 2 else (b, tb)
        if rng.random() < 0.4:
            assert rep.execute_mut(nrg.Remove(k), tok) == d.pop(k, None), i
        else:
            v = int(rng.integers(0, 2**63, dtype=np.uint64))
            assert rep.execute_mut(nrg.Put(k, v), tok) == d.get(k), i
            d[k] = v
    for rep, tok in ((a, ta), (b, tb)):
        for k in (0, 5, 10, 240, 250, 2**64 - 1):
            assert rep.execute(nrg.Get(k), tok) == d.get(k)
    seen = []
    a.verify(seen.append)
    b.verify(seen.append)
    assert seen[0] == seen[1] == d and a.digest() == b.digest()
    # an op that would not mean on this replica what it says is refused before it reaches the log
    tail = a.dev.log_state()["tail"]
    with pytest.raises(ValueError):
        a.execute_mut(nrg.Remove(10, tombstone=R.OTHER_TOMB), ta)  # another tombstone: it would be a Put
    with pytest.raises(ValueError):
        a.execute_mut(nrg.Put(10, R.TOMB), ta)  # the replica's tombstone as a value: it would be a Remove
    assert a.dev.log_state()["tail"] == tail and a.execute(nrg.Get(10), ta) == d.get(10)
    c = nrg.Replica(log, nrg.NrHashMap, 0, log2_slots=10, max_batch=1024, clone_from=a)
    assert c.dev.hm_removal() == R.TOMB  # the clone takes the peer's setting
    c.verify(seen.append)
    assert seen[2] == d
    for r in (a, b, c):
        r.dev.close()


def test_python_remove_needs_the_replicas_tombstone(nrg):
    """nrgpu.Remove on a replica without removal, and with another tombstone than the replica's"""
    log = nrg.Log(LOG_BYTES)
    a = nrg.Replica(log, nrg.NrHashMap, 0, log2_slots=10, max_batch=1024)
    ta = a.register()
    assert a.execute_mut(nrg.Put(1, R.TOMB), ta) is None  # removal off: 2^64 - 1 is a value
    with pytest.raises(nrg.NrgError) as e:
        a.execute_mut(nrg.Remove(1), ta)
    assert e.value.code == nrg._lib.NRG_E_INVAL and a.execute(nrg.Get(1), ta) == R.TOMB
    a.dev.hm_enable_removal(R.OTHER_TOMB)
    with pytest.raises(ValueError):
        a.execute_mut(nrg.Remove(1), ta)  # the default tombstone is not this replica's
    assert a.execute(nrg.Get(1), ta) == R.TOMB
    assert a.execute_mut(nrg.Remove(1, tombstone=R.OTHER_TOMB), ta) == R.TOMB
    assert a.execute(nrg.Get(1), ta) is None and a.execute_mut(nrg.Put(1, R.TOMB), ta) is None
    a.dev.close()
