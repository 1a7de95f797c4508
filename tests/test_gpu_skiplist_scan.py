"""nrg_skiplist_scan / nrg_skiplist_scan_async (csrc/skiplist.hip sl_walk_kernel) against the scan
model of tests/skiplist_scan_model.py, bit for bit. Every output buffer is filled with a canary first
and every slot at or past a query's count must still hold it. The maps are small (at most about
2000 keys) with delta_max 8 or 64, so that the base and the delta run both hold keys where a case
wants them; tests/skiplist_model.py says which run a key is in."""
import ctypes as C

import numpy as np
import pytest

import skiplist_model as M
import skiplist_scan_model as SM

pytestmark = pytest.mark.gpu

U64_MAX = SM.U64_MAX
MIN_LOG_BYTES = 2 * 32 * 256 * 64
CANARY = 0xA5A5A5A5A5A5A5A5
CANARY32 = 0x77777777


def _val(k):
    return (int(k) * 0x9E3779B97F4A7C15 + 12345) & U64_MAX


def _recs(nrg, keys, vals):
    r = np.zeros(len(keys), nrg.PUT_DTYPE)
    r["key"], r["val"] = np.array(keys, np.uint64), np.array(vals, np.uint64)
    return r


def _push(nrg, dev, model, keys, vals=None):
    """one fused round of Push records through the device and the model"""
    import torch

    vals = [_val(k) for k in keys] if vals is None else vals
    recs = _recs(nrg, keys, vals)
    d = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
    dev.sl_round_device(d, len(recs), 1)
    dev.sync()
    model.replay(recs)


def _build(nrg, base, delta, delta_max=64, log2=11, **kw):
    """a replica whose base run holds `base` and whose delta run holds `delta`: the base keys in one
    round of more than delta_max new keys (it compacts), the delta keys in one of at most delta_max"""
    kw.setdefault("max_batch", 2048)
    kw.setdefault("log_bytes", MIN_LOG_BYTES)
    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_SKIPLIST, 0, knobs={"SL_DELTA_MAX": delta_max}, log2_slots=log2, **kw)
    model = M.SkipListModel(delta_max, kw["max_batch"])
    if len(base):
        assert len(base) > delta_max
        _push(nrg, dev, model, list(base))
    if len(delta):
        assert len(delta) <= delta_max
        _push(nrg, dev, model, list(delta))
    assert (model.nb, model.nd) == (len(base), len(delta))
    assert not set(base) & set(delta)
    return dev, model


def _spread(n, lo=1 << 20, step=997):
    return [lo + step * i for i in range(n)]


def _state(name):
    """(delta_max, base keys, delta keys, queries of the case)"""
    if name == "empty":
        return 64, [], [], []
    if name == "delta_only":  # before the first compaction
        ks = [0] + _spread(38) + [U64_MAX]
        return 64, [], ks, []
    if name == "base_only":  # right after a compaction
        ks = [0] + _spread(98) + [U64_MAX]
        return 64, ks, [], []
    if name == "alternating":  # single keys in turn: base, delta, base, ...
        ks = [0] + _spread(127) + [U64_MAX]
        return 64, ks[0::2], ks[1::2], []
    if name == "blocks_3_5":  # 3 base keys, 5 delta keys, ...: the splits leave the diagonals
        ks = _spread(96)
        base = [k for i, k in enumerate(ks) if i % 8 < 3]
        delta = [k for i, k in enumerate(ks) if i % 8 >= 3]
        fill = [0] + [(1 << 62) + 3 * i for i in range(40)] + [U64_MAX]  # the base round must pass delta_max
        return 64, base + fill, delta, []
    if name == "base_runs_out":  # from the queries on, 2 base keys are left and many delta keys
        base = _spread(70)
        top = base[-1]
        delta = [top - 997 - 10] + [top - 5] + [top + 10 * i + 1 for i in range(58)]
        # ascending from just below base[-2]: base has 2 left; descending from just above base[1]
        return 64, base, delta, [base[-2] - 1, base[-2], base[1] + 1, base[1], delta[-1], delta[0]]
    if name == "delta_runs_out":  # the reverse: 2 delta keys left inside a long stretch of base
        base = _spread(1200)
        mid = base[600]
        delta = [mid + 1, mid + 998, base[0] - 7, base[0] - 3, base[-1] + 4, base[-1] + 9, base[300] + 1, base[900] + 1]
        return 8, base, delta, [mid, mid + 1, mid + 999, base[0] - 8, base[-1] + 10, base[-1] + 5]
    if name == "big":  # 1024 entries and more from its queries, upwards from one and downwards from another
        ks = [0] + _spread(1958) + [U64_MAX]
        delta = ks[5::33][:60]
        ds = set(delta)
        return 64, [k for k in ks if k not in ds], delta, [ks[980], ks[979] + 1, ks[1024], ks[936]]
    raise KeyError(name)


STATES = ["empty", "delta_only", "base_only", "alternating", "blocks_3_5", "base_runs_out", "delta_runs_out", "big"]


def _scan_dev(dev, qs, mode, limit):
    """nrg_skiplist_scan_async into canary-filled device buffers: (keys[n, limit], vals, counts)"""
    import torch

    qs = np.ascontiguousarray(qs, np.uint64)
    n = len(qs)
    dq = torch.from_numpy(qs.view(np.int64).copy()).cuda() if n else None
    ok = torch.from_numpy(np.full(max(n, 1) * limit, CANARY, np.uint64).view(np.int64)).cuda()
    ov = ok.clone()
    cnt = torch.from_numpy(np.full(max(n, 1), CANARY32, np.uint32).view(np.int32)).cuda()
    dev.sl_scan_device(dq, n, mode, limit, ok, ov, cnt)
    dev.sync()
    return (ok.cpu().numpy().view(np.uint64).reshape(-1, limit), ov.cpu().numpy().view(np.uint64).reshape(-1, limit),
            cnt.cpu().numpy().view(np.uint32))


def _scan_host(nrg, dev, qs, mode, limit):
    """nrg_skiplist_scan into canary-filled host buffers: (rc, keys[n, limit], vals, counts)"""
    qs = np.ascontiguousarray(qs, np.uint64)
    n = len(qs)
    ok = np.full(max(n, 1) * limit, CANARY, np.uint64)
    ov = np.full(max(n, 1) * limit, CANARY, np.uint64)
    cnt = np.full(max(n, 1), CANARY32, np.uint32)
    rc = nrg._lib.load().nrg_skiplist_scan(dev.handle, qs.ctypes.data_as(C.c_void_p), n, mode, limit,
                                           ok.ctypes.data_as(C.c_void_p), ov.ctypes.data_as(C.c_void_p),
                                           cnt.ctypes.data_as(C.c_void_p))
    return rc, ok.reshape(-1, limit), ov.reshape(-1, limit), cnt


def _check(got, model, qs, mode, limit, msg):
    """entries below each count equal the model's; every slot at or past it holds the canary"""
    ok, ov, cnt = got
    n = len(qs)
    eok, eov, ecnt = SM.scan_batch(model.keys, model.m, qs, mode, limit)
    np.testing.assert_array_equal(cnt[:n], ecnt, err_msg=msg + " counts")
    live = np.arange(limit)[None, :] < ecnt[:, None]
    np.testing.assert_array_equal(ok[:n][live], eok[live], err_msg=msg + " keys")
    np.testing.assert_array_equal(ov[:n][live], eov[live], err_msg=msg + " vals")
    assert np.all(ok[:n][~live] == CANARY) and np.all(ov[:n][~live] == CANARY), msg + ": a slot past the count was written"
    assert np.all(ok[n:] == CANARY) and np.all(ov[n:] == CANARY) and np.all(cnt[n:] == CANARY32), msg + ": rows past n"


@pytest.mark.parametrize("state", STATES)
def test_states(nrg, state):
    """Every map state, all four modes, queries below, above, at and between the stored keys and at
    the ends of the key space, limits 1 .. 1024 including one above the whole map's size."""
    L = nrg._lib
    dmax, base, delta, extra = _state(state)
    dev, model = _build(nrg, base, delta, dmax)
    qs = np.concatenate([SM.edge_queries(model.keys), np.array(extra, np.uint64), SM.random_queries(model.keys, 40, 7)])
    over = min(len(model) + 5, SM.MAX_LIMIT)
    for mode in SM.MODES:
        for limit in sorted({1, 2, 3, 5, 63, 64, 65, 128, 1024, over}):
            _check(_scan_dev(dev, qs, mode, limit), model, qs, mode, limit, f"{state} mode {mode} limit {limit}")
    # the ends of the key space by name
    full = min(len(model), 8)
    has_ends = len(model) and model.keys[0] == 0 and model.keys[-1] == U64_MAX
    _, _, c = _scan_dev(dev, np.array([0, U64_MAX, U64_MAX, 0, U64_MAX - 2, 1], np.uint64), L.NRG_SEEK_GE, 8)
    assert c[0] == full and c[1] == (1 if has_ends else 0)
    _, _, c = _scan_dev(dev, np.array([U64_MAX, 0], np.uint64), L.NRG_SEEK_LE, 8)
    assert c[0] == full and c[1] == (1 if has_ends else 0)
    k, _, c = _scan_dev(dev, np.array([U64_MAX, U64_MAX - 2], np.uint64), L.NRG_SEEK_GT, 8)
    assert c[0] == 0 and c[1] == (1 if has_ends else 0) and (not has_ends or k[1, 0] == U64_MAX)
    _, _, c = _scan_dev(dev, np.array([0], np.uint64), L.NRG_SEEK_LT, 8)
    assert c[0] == 0
    dev.close()


def test_every_width_and_step_count(nrg):
    """Every limit at which the host changes the lane group's width or the number of steps a group
    takes, and that limit +- 1, on a map whose queries have 1024 entries and more ahead of them in
    one direction or the other."""
    dmax, base, delta, extra = _state("big")
    dev, model = _build(nrg, base, delta, dmax)
    ks = model.keys
    qs = np.array(extra + [0, U64_MAX, ks[3], ks[-3] + 1, ks[1000] + 1, ks[5], ks[-40]], np.uint64)
    limits = sorted(set(SM.shape_limits()) | set(SM.NAMED_LIMITS) | {SM.MAX_LIMIT - 1})
    assert {1, 2, 3, 4, 5, 9, 17, 33, 64, 65, 66, 129, 961, 1023, 1024} <= set(limits)
    for limit in limits:
        for mode in SM.MODES:
            _check(_scan_dev(dev, qs, mode, limit), model, qs, mode, limit, f"limit {limit} mode {mode}")
    dev.close()


def test_limit_equal_to_what_remains(nrg):
    """The window ends exactly at the end of the map, of the base run or of the delta run: limits of
    what remains in the direction, one less and one more."""
    L = nrg._lib
    for state in ("alternating", "base_runs_out", "delta_runs_out"):
        dmax, base, delta, _ = _state(state)
        dev, model = _build(nrg, base, delta, dmax)
        ks = model.keys
        sb, sd = sorted(base), sorted(delta)
        cases = []
        for q in (ks[-1], ks[-2], ks[-64], ks[-65], ks[len(ks) // 2], sb[-1], sb[-3], sd[-1], sd[-2]):
            cases.append((q, L.NRG_SEEK_GE, len(ks) - ks.index(q)))
        for q in (ks[0], ks[1], ks[63], ks[64], sb[0], sb[2], sd[0], sd[1]):
            cases.append((q, L.NRG_SEEK_LE, ks.index(q) + 1))
        for q, mode, remains in cases:
            for limit in sorted({remains - 1, remains, remains + 1} & set(range(1, SM.MAX_LIMIT + 1))):
                qs = np.array([q, q], np.uint64)
                got = _scan_dev(dev, qs, mode, limit)
                _check(got, model, qs, mode, limit, f"{state} q {q} mode {mode} limit {limit}")
                assert got[2][0] == min(limit, remains)
        dev.close()


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 600])
def test_batch_sizes_device_and_host_form(nrg, n):
    L = nrg._lib
    lib = L.load()
    dmax, base, delta, _ = _state("alternating")
    dev, model = _build(nrg, base, delta, dmax)
    qs = SM.random_queries(model.keys, n, 100 + n)
    for mode in SM.MODES:
        for limit in (1, 5, 64, 100):
            msg = f"n {n} mode {mode} limit {limit}"
            _check(_scan_dev(dev, qs, mode, limit), model, qs, mode, limit, msg + " device form")
            rc, *got = _scan_host(nrg, dev, qs, mode, limit)
            assert rc == L.NRG_OK
            _check(got, model, qs, mode, limit, msg + " host form")
    if n == 0:  # nothing to do: no buffer is needed
        assert lib.nrg_skiplist_scan(dev.handle, None, 0, L.NRG_SEEK_GE, 4, None, None, None) == L.NRG_OK
        assert lib.nrg_skiplist_scan_async(dev.handle, None, 0, L.NRG_SEEK_LT, 4, None, None, None) == L.NRG_OK
        k, v, c = dev.sl_scan(qs, L.NRG_SEEK_GE, 4)
        assert k.shape == (0, 4) and v.shape == (0, 4) and c.shape == (0,)
    else:
        k, v, c = dev.sl_scan(qs, L.NRG_SEEK_GT, 5)  # the Python form pads with zeros
        ek, ev, ec = SM.scan_batch(model.keys, model.m, qs, L.NRG_SEEK_GT, 5)
        assert np.array_equal(k, ek) and np.array_equal(v, ev) and np.array_equal(c, ec)
    dev.close()


def test_limit_one_is_the_seek(nrg):
    """limit = 1 answers exactly as nrg_skiplist_seek_async: the same entry where one is found, and
    counts[i] == found[i]."""
    import torch

    L = nrg._lib
    lib = L.load()
    for state in ("blocks_3_5", "base_runs_out"):  # with the keys 0 and 2^64 - 1, and without them
        dmax, base, delta, _ = _state(state)
        dev, model = _build(nrg, base, delta, dmax)
        ends = model.keys[0] == 0 and model.keys[-1] == U64_MAX
        qs = np.concatenate([SM.random_queries(model.keys, 600, 21), SM.edge_queries(model.keys)])
        n = len(qs)
        dq = torch.from_numpy(qs.view(np.int64).copy()).cuda()
        for mode in SM.MODES:
            sk, sv = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
            sf = torch.zeros(n, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            L.check(lib.nrg_skiplist_seek_async(dev.handle, dq.data_ptr(), n, mode, sk.data_ptr(), sv.data_ptr(),
                                                sf.data_ptr()))
            dev.sync()
            ok, ov, cnt = _scan_dev(dev, qs, mode, 1)
            f = sf.cpu().numpy()
            np.testing.assert_array_equal(cnt, f)
            hit = f == 1
            # with 0 and 2^64 - 1 in the map every GE and every LE finds an entry
            assert hit.any() and ((~hit).any() or (ends and mode in (L.NRG_SEEK_GE, L.NRG_SEEK_LE)))
            np.testing.assert_array_equal(ok[:, 0][hit], sk.cpu().numpy().view(np.uint64)[hit])
            np.testing.assert_array_equal(ov[:, 0][hit], sv.cpu().numpy().view(np.uint64)[hit])
            assert np.all(ok[:, 0][~hit] == CANARY) and np.all(ov[:, 0][~hit] == CANARY)
        dev.close()


@pytest.mark.parametrize("page", [1, 7, 64, 1024])
def test_pages_equal_the_dump(nrg, page):
    """GT pages from GE(0) on, concatenated, are nrg_skiplist_dump; LT pages from LE(2^64 - 1) on are
    its reverse."""
    L = nrg._lib
    name = "alternating" if page == 1 else "big"
    dmax, base, delta, _ = _state(name)
    dev, model = _build(nrg, base, delta, dmax)
    dk, dv = dev.sl_dump()
    for first, nxt, start, want in ((L.NRG_SEEK_GE, L.NRG_SEEK_GT, 0, (dk, dv)),
                                    (L.NRG_SEEK_LE, L.NRG_SEEK_LT, U64_MAX, (dk[::-1], dv[::-1]))):
        ks, vs, key, mode = [], [], start, first
        for _ in range(len(dk) // page + 2):
            k, v, c = dev.sl_scan(np.array([key], np.uint64), mode, page)
            m = int(c[0])
            ks.append(k[0, :m]), vs.append(v[0, :m])
            if m < page:
                break
            key, mode = int(k[0, m - 1]), nxt
        else:
            raise AssertionError("the walk did not end")
        assert np.array_equal(np.concatenate(ks), want[0]) and np.array_equal(np.concatenate(vs), want[1])
    dev.close()


def test_descending_is_ascending_on_the_mirrored_map(nrg):
    """LE / LT on a map are GE / GT on the map of the mirrored keys (k -> 2^64 - 1 - k), entry for
    entry, with the runs mirrored too."""
    L = nrg._lib
    dmax, base, delta, extra = _state("blocks_3_5")
    dev, model = _build(nrg, base, delta, dmax)
    mbase, mdelta = [SM.mirror(k) for k in base], [SM.mirror(k) for k in delta]
    import torch

    mdev = nrg.DeviceReplica(L.NRG_DS_SKIPLIST, 0, knobs={"SL_DELTA_MAX": dmax}, log2_slots=11, max_batch=2048,
                             log_bytes=MIN_LOG_BYTES)
    for ks in (mbase, mdelta):  # the value of a mirrored key is its original's
        recs = _recs(nrg, ks, [_val(SM.mirror(k)) for k in ks])
        mdev.sl_round_device(torch.from_numpy(recs.view(np.uint8).copy()).cuda(), len(recs), 1)
        mdev.sync()
    qs = np.concatenate([SM.edge_queries(model.keys), SM.random_queries(model.keys, 60, 4)])
    mq = np.array([SM.mirror(q) for q in qs], np.uint64)
    for down, up in ((L.NRG_SEEK_LE, L.NRG_SEEK_GE), (L.NRG_SEEK_LT, L.NRG_SEEK_GT)):
        for limit in (1, 7, 64, 200):
            ak, av, ac = _scan_dev(dev, qs, down, limit)
            bk, bv, bc = _scan_dev(mdev, mq, up, limit)
            np.testing.assert_array_equal(ac, bc)
            live = np.arange(limit)[None, :] < ac[:, None]
            np.testing.assert_array_equal(ak[live], np.uint64(U64_MAX) - bk[live])
            np.testing.assert_array_equal(av[live], bv[live])
            _check((ak, av, ac), model, qs, down, limit, f"mode {down} limit {limit}")
    dev.close()
    mdev.close()


def test_scans_show_updated_values(nrg):
    """A round that only replaces values of present keys, in both runs: no key moves, the scans show
    the new values."""
    dmax, base, delta, _ = _state("alternating")
    dev, model = _build(nrg, base, delta, dmax)
    nb, nd = model.nb, model.nd
    upd = sorted(base)[3:40:2] + sorted(delta)[1:50:3]
    _push(nrg, dev, model, upd, [(_val(k) ^ 0xFFFF) for k in upd])
    assert (model.nb, model.nd) == (nb, nd)
    qs = np.concatenate([SM.edge_queries(model.keys), np.array(upd[:10], np.uint64)])
    for mode in SM.MODES:
        for limit in (1, 16, 200):
            got = _scan_dev(dev, qs, mode, limit)
            _check(got, model, qs, mode, limit, f"after the update, mode {mode} limit {limit}")
    k, v, c = dev.sl_scan(np.array([upd[0]], np.uint64), SM.MODES[0], 1)
    assert int(k[0, 0]) == upd[0] and int(v[0, 0]) == _val(upd[0]) ^ 0xFFFF
    dev.close()


def test_replica_execute_scan(nrg):
    """Replica.execute(Scan(...)) and a batch of reads with mixed (mode, limit), Gets and Seeks."""
    L = nrg._lib
    log = nrg.Log(MIN_LOG_BYTES)
    rep = nrg.Replica(log, nrg.SkipList, 0, log2_slots=10, max_batch=1024)
    tok = rep.register()
    model = M.SkipListModel()
    ks = [0, 5, 10, 20, 40, 41, 42, 300, 1 << 40, U64_MAX]
    for k in ks:
        assert rep.execute_mut(nrg.SlPush(k, _val(k)), tok) == k
        model.replay([(k, _val(k))])
    assert rep.execute(nrg.Scan(6, L.NRG_SEEK_GE, 3), tok) == [(10, _val(10)), (20, _val(20)), (40, _val(40))]
    assert rep.execute(nrg.Scan(0, L.NRG_SEEK_LT, 3), tok) == []
    ops = [nrg.Scan(41, L.NRG_SEEK_LE, 2), nrg.Get(5), nrg.Scan(41, L.NRG_SEEK_GT, 100), nrg.Seek(6, L.NRG_SEEK_GE),
           nrg.Scan(U64_MAX, L.NRG_SEEK_LE, 2), nrg.Scan(7, L.NRG_SEEK_LE, 2), nrg.Get(6), nrg.Scan(0, L.NRG_SEEK_GE, 100)]
    want = [SM.scan(model.keys, model.m, o.key, o.mode, o.limit) if isinstance(o, nrg.Scan)
            else model.get(o.key) if isinstance(o, nrg.Get) else model.seek(o.key, o.mode) for o in ops]
    assert rep.execute_batch(ops, tok) == want
    assert want[7] == model.items() and want[0] == [(41, _val(41)), (40, _val(40))]
    rep.dev.close()


def test_refusals_leave_buffers_and_log_alone(nrg):
    """Each NRG_E_INVAL case, NRG_E_NOT_SYNCED with an unreplayed append, n > max_reads, and the host
    form's staging bound: the buffers keep their canary and the log its state."""
    import torch

    L = nrg._lib
    lib = L.load()
    E, GE = L.NRG_E_INVAL, L.NRG_SEEK_GE
    dmax, base, delta, _ = _state("alternating")
    dev, model = _build(nrg, base, delta, dmax, max_reads=1 << 15)
    n, limit = 8, 4
    qs = np.arange(n, dtype=np.uint64)
    dq = torch.from_numpy(qs.view(np.int64).copy()).cuda()
    ok = torch.from_numpy(np.full(n * limit, CANARY, np.uint64).view(np.int64)).cuda()
    ov = ok.clone()
    cnt = torch.from_numpy(np.full(n, CANARY32, np.uint32).view(np.int32)).cuda()
    hk, hv, hc = np.full(n * limit, CANARY, np.uint64), np.full(n * limit, CANARY, np.uint64), np.full(n, CANARY32, np.uint32)
    torch.cuda.synchronize()
    before = dev.log_state()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    H = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    dargs = (P(dq), P(ok), P(ov), P(cnt))
    hargs = (H(qs), H(hk), H(hv), H(hc))

    def both(n_, mode, lim, dsel=dargs, hsel=hargs, h=None):
        h = dev.handle if h is None else h
        return (lib.nrg_skiplist_scan_async(h, dsel[0], n_, mode, lim, dsel[1], dsel[2], dsel[3]),
                lib.nrg_skiplist_scan(h, hsel[0], n_, mode, lim, hsel[1], hsel[2], hsel[3]))

    assert both(n, L.NRG_SEEK_LT + 1, limit) == (E, E)
    assert both(n, GE, 0) == (E, E)
    assert both(n, GE, L.NRG_SCAN_MAX_LIMIT + 1) == (E, E)
    for drop in range(4):  # a NULL buffer with n > 0
        da = tuple(None if i == drop else a for i, a in enumerate(dargs))
        ha = tuple(None if i == drop else a for i, a in enumerate(hargs))
        assert both(n, GE, limit, da, ha) == (E, E), drop
    hm = nrg.DeviceReplica(L.NRG_DS_HASHMAP, 0, log2_slots=12, max_batch=1024, log_bytes=MIN_LOG_BYTES)
    assert both(n, GE, limit, h=hm.handle) == (E, E)  # another kind
    hm.close()
    # more queries than max_reads (checked before any buffer is looked at)
    assert both((1 << 15) + 1, GE, 1) == (L.NRG_E_CAPACITY, L.NRG_E_CAPACITY)
    # the host form's staging: n * limit <= 2^24
    big = np.zeros((1 << 14) + 1, np.uint64)
    assert lib.nrg_skiplist_scan(dev.handle, H(big), len(big), GE, 1024, H(hk), H(hv), H(hc)) == L.NRG_E_CAPACITY
    assert dev.log_state() == before
    # an append that has not been replayed
    dev.log_append(_recs(nrg, [777], [1]), 1)
    mid = dev.log_state()
    assert both(n, GE, limit) == (L.NRG_E_NOT_SYNCED, L.NRG_E_NOT_SYNCED)
    assert dev.log_state() == mid
    dev.sync()
    for t in (ok, ov):
        assert np.all(t.cpu().numpy().view(np.uint64) == CANARY)
    assert np.all(cnt.cpu().numpy().view(np.uint32) == CANARY32)
    assert np.all(hk == CANARY) and np.all(hv == CANARY) and np.all(hc == CANARY32)
    assert mid["tail"] == before["tail"] + 1 and mid["ltail"] == before["ltail"]
    dev.log_exec()
    model.replay([(777, 1)])
    assert both(n, GE, limit) == (L.NRG_OK, L.NRG_OK)
    dev.sync()
    got = (ok.cpu().numpy().view(np.uint64).reshape(n, limit), ov.cpu().numpy().view(np.uint64).reshape(n, limit),
           cnt.cpu().numpy().view(np.uint32))
    _check(got, model, qs, GE, limit, "after the refusals, device form")
    _check((hk.reshape(n, limit), hv.reshape(n, limit), hc), model, qs, GE, limit, "after the refusals, host form")
    dev.close()


def test_host_form_at_its_staging_bound(nrg):
    """n * limit = 2^24 exactly is accepted by the host form."""
    L = nrg._lib
    dmax, base, delta, _ = _state("delta_only")
    dev, model = _build(nrg, base, delta, dmax, max_reads=1 << 14)
    n, limit = 1 << 14, 1024
    qs = SM.random_queries(model.keys, n, 77)
    rc, ok, ov, cnt = _scan_host(nrg, dev, qs, L.NRG_SEEK_GT, limit)
    assert rc == L.NRG_OK
    ks = np.array(model.keys, np.uint64)
    np.testing.assert_array_equal(cnt, len(ks) - np.searchsorted(ks, qs, side="right"))
    sub = slice(0, n, 97)
    _check((ok[sub], ov[sub], cnt[sub]), model, qs[sub], L.NRG_SEEK_GT, limit, "host form at 2^24 slots")
    live = np.arange(limit)[None, :] < cnt[:, None]
    assert np.all(ok[~live] == CANARY) and np.all(ov[~live] == CANARY)
    dev.close()
