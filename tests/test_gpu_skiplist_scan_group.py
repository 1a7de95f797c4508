"""nrg_group_skiplist_scan over the loopback collectives (groups opened as
tests/test_gpu_skiplist_partitioned.py opens them): every answer equals the scan of the whole map by
the model of tests/skiplist_scan_model.py, bit for bit, and no slot at or past a query's count is
written. The members are filled by nrg_skiplist_prefill_partition (their base runs) and a partitioned
round (their delta runs)."""
import ctypes as C
import threading

import numpy as np
import pytest

import skiplist_scan_model as SM

pytestmark = pytest.mark.gpu

U64_MAX = SM.U64_MAX
LOG_BYTES = 64 * (1 << 16)
LOG2_SLOTS, MAX_BATCH, MAX_READS, DELTA_MAX = 12, 2048, 2048, 64
PREFILL, OFF = 1500, 9
CANARY = 0xA5A5A5A5A5A5A5A5
CANARY32 = 0x77777777
CASES = [(1, False), (1, True), (3, False), (8, False)]
N_ROT = (0, 1, 37, 300)  # ragged query counts per member
CLUSTER_AT = 1 << 50


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


def _cfg(L, kind=None):
    cfg = L.default_config(L.NRG_DS_SKIPLIST if kind is None else kind)
    cfg.log2_slots, cfg.max_batch, cfg.max_reads = LOG2_SLOTS, MAX_BATCH, MAX_READS
    cfg.log_bytes = LOG_BYTES
    return cfg


def _open(L, lib, G, cfg=None, exp=False):
    cfg = cfg or _cfg(L)
    L.check(lib.nrg_test_loopback_collectives(1))
    g = C.c_void_p()
    try:
        L.check(lib.nrg_group_open((C.c_int * G)(*([0] * G)), G, C.byref(cfg), C.byref(g)), "nrg_group_open")
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))
    ctxs = [lib.nrg_group_replica(g, i) for i in range(G)]
    for c in ctxs:
        if cfg.ds_kind == L.NRG_DS_SKIPLIST:
            L.check(lib.nrg_test_set_knob(c, L.KNOBS["SL_DELTA_MAX"], DELTA_MAX))
        if exp:
            L.check(lib.nrg_test_set_knob(c, L.KNOBS["EXP"], 0x10000))
    return g, ctxs


def _cluster(G):
    """six keys from 2^50 on that partition 0 of G owns: a stretch of the map that lives in one partition"""
    pool = np.arange(CLUSTER_AT, CLUSTER_AT + 400, dtype=np.uint64)
    return pool[SM.key_owner(pool, G) == 0][:6]


def _round_keys(G, seed=3):
    """the one round's records: new keys below and between the prefilled ones' span, updates of
    prefilled keys, the cluster, 0 and 2^64 - 1; at most 64 new keys, so every member's stay in delta"""
    rng = np.random.default_rng(seed)
    k = np.concatenate([rng.integers(0, 2 * PREFILL, 44, dtype=np.uint64), _cluster(G),
                        np.array([0, U64_MAX, PREFILL + 7], np.uint64)])
    v = rng.integers(0, U64_MAX, len(k), dtype=np.uint64, endpoint=True)
    return k, v


def _push_round(L, lib, g, G, k, v, member=0):
    """one partitioned round: `member` pushes (k, v), nobody reads"""
    import torch

    rd = (L.Round * G)()
    p = _cuda(np.stack([k, v], 1).astype(np.uint64))
    dummy = torch.zeros(8, dtype=torch.int64, device="cuda")
    for i in range(G):
        rd[i].get_vals, rd[i].get_found = dummy.data_ptr(), dummy.data_ptr()
    rd[member].recs, rd[member].n = p.data_ptr(), len(k)
    torch.cuda.synchronize()
    L.check(lib.nrg_group_partitioned_round(g, rd), "round")
    L.check(lib.nrg_group_sync(g))


def _model(prefill, k, v):
    """(sorted keys, dict) of the whole map: the prefill, then the round's records in order"""
    m = {i: i + OFF for i in range(prefill)}
    for a, b in zip(k.tolist(), v.tolist()):
        m[a] = b
    return sorted(m), m


def _filled(L, lib, G, exp):
    g, ctxs = _open(L, lib, G, exp=exp)
    for p, c in enumerate(ctxs):
        L.check(lib.nrg_skiplist_prefill_partition(c, PREFILL, OFF, p, G))
    k, v = _round_keys(G)
    _push_round(L, lib, g, G, k, v)
    return g, ctxs, _model(PREFILL, k, v)


def _queries(ks, G, rot, seed):
    """per member: n rotates over N_ROT; edge queries first, then random ones"""
    out = []
    for i in range(G):
        n = N_ROT[(i + rot) % 4]
        pool = np.concatenate([SM.edge_queries(ks), np.array([CLUSTER_AT, CLUSTER_AT - 1, 2 * PREFILL + 1], np.uint64),
                               SM.random_queries(ks, 300, seed + i)])
        out.append(pool[:n].copy() if n != 1 else pool[6 + i:7 + i].copy())
    return out


def _scan_all(L, lib, g, qs, mode, limit, modes=None, limits=None):
    """one nrg_group_skiplist_scan over the members' keys; (rc, per member (keys[n, limit], vals, counts))"""
    import torch

    G = len(qs)
    sc = (L.Scan * G)()
    keep = []
    for i, q in enumerate(qs):
        n = len(q)
        ok = torch.from_numpy(np.full(max(n, 1) * limit, CANARY, np.uint64).view(np.int64)).cuda()
        d = (_cuda(q) if n else None, ok, ok.clone(),
             torch.from_numpy(np.full(max(n, 1), CANARY32, np.uint32).view(np.int32)).cuda())
        sc[i].keys, sc[i].n = (d[0].data_ptr() if n else 0), n
        sc[i].out_keys, sc[i].out_vals, sc[i].counts = d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr()
        keep.append(d)
    torch.cuda.synchronize()
    rc = lib.nrg_group_skiplist_scan(g, sc, mode, limit)
    got = [(d[1].cpu().numpy().view(np.uint64).reshape(-1, limit), d[2].cpu().numpy().view(np.uint64).reshape(-1, limit),
            d[3].cpu().numpy().view(np.uint32)) for d in keep]
    return rc, got


def _check(got, ks, m, q, mode, limit, msg):
    ok, ov, cnt = got
    n = len(q)
    eok, eov, ecnt = SM.scan_batch(ks, m, q, mode, limit)
    np.testing.assert_array_equal(cnt[:n], ecnt, err_msg=msg + " counts")
    live = np.arange(limit)[None, :] < ecnt[:, None]
    np.testing.assert_array_equal(ok[:n][live], eok[live], err_msg=msg + " keys")
    np.testing.assert_array_equal(ov[:n][live], eov[live], err_msg=msg + " vals")
    assert np.all(ok[:n][~live] == CANARY) and np.all(ov[:n][~live] == CANARY), msg + ": a slot past the count was written"
    assert np.all(ok[n:] == CANARY) and np.all(ov[n:] == CANARY) and np.all(cnt[n:] == CANARY32), msg + ": rows past n"


def _check_all(L, lib, g, ks, m, G, limits, what, seed=0):
    for mode in SM.MODES:
        for j, limit in enumerate(limits):
            qs = _queries(ks, G, mode + j, seed)
            rc, got = _scan_all(L, lib, g, qs, mode, limit)
            assert rc == L.NRG_OK, (what, mode, limit, rc)
            for i, q in enumerate(qs):
                _check(got[i], ks, m, q, mode, limit, f"{what} G={G} mode {mode} limit {limit} member {i} (n = {len(q)})")


def _valid(L, lib, g, ks, m, G, what):
    """a small scan that must succeed (after a refusal the group is still usable)"""
    qs = [np.array([0, 700 + i, U64_MAX], np.uint64) for i in range(G)]
    rc, got = _scan_all(L, lib, g, qs, L.NRG_SEEK_GE, 3)
    assert rc == L.NRG_OK, what
    for i, q in enumerate(qs):
        _check(got[i], ks, m, q, L.NRG_SEEK_GE, 3, what)


@pytest.mark.parametrize("G,exp", CASES)
def test_group_scan(nrg, G, exp):
    """Ragged n per member (0, 1, 37, 300, rotating so that n = 0 visits every rank), all four modes,
    limits 1, 5, 64 and 1024; then n = 0 on every rank, and each refusal followed by a valid scan."""
    import torch

    L = nrg._lib
    lib = L.load()
    g, ctxs, (ks, m) = _filled(L, lib, G, exp)
    if G > 1:  # what the cluster is for: the whole answer in one partition, the others without a candidate
        lists = [SM.scan(pk, pv, CLUSTER_AT, L.NRG_SEEK_GE, 5) for pk, pv in SM.partition(ks, [m[k] for k in ks], G)]
        assert len(lists[0]) == 5 and SM.reduce_lists(lists, L.NRG_SEEK_GE, 5) == lists[0]
        assert sum(1 for lst in lists if not lst) >= 1
    _check_all(L, lib, g, ks, m, G, (1, 5, 64, 1024), "filled")
    E, GE = L.NRG_E_INVAL, L.NRG_SEEK_GE
    assert lib.nrg_group_skiplist_scan(g, (L.Scan * G)(), GE, 5) == L.NRG_OK  # n = 0 on every rank
    assert lib.nrg_group_skiplist_scan(g, None, GE, 5) == E
    qs = _queries(ks, G, 3, 1)
    for mode, limit in ((L.NRG_SEEK_LT + 1, 5), (GE, 0), (GE, L.NRG_SCAN_MAX_LIMIT + 1)):
        sc, keep = _raw(L, qs, 8)  # (buffers for a legal limit; the call's may not be one)
        torch.cuda.synchronize()
        assert lib.nrg_group_skiplist_scan(g, sc, mode, limit) == E, (mode, limit)
        assert all(np.all(d[1].cpu().numpy().view(np.uint64) == CANARY) for d in keep)
        assert all(np.all(d[3].cpu().numpy().view(np.uint32) == CANARY32) for d in keep)
        _valid(L, lib, g, ks, m, G, f"after mode {mode} limit {limit}")
    # a member that asks without buffers
    big = max(range(G), key=lambda i: len(qs[i]))
    sc = (L.Scan * G)()
    d = _cuda(qs[big])
    sc[big].keys, sc[big].n = d.data_ptr(), len(qs[big])
    assert lib.nrg_group_skiplist_scan(g, sc, GE, 5) == E
    _valid(L, lib, g, ks, m, G, "after a member without buffers")
    # the size bound: G * nmax * limit <= 2^27, refused on every rank before any data moves (the
    # output buffers are never looked at)
    n_over = (1 << 27) // (G * 1024) + 1
    sc, keep = _raw(L, [np.zeros(n_over if i == G - 1 else 1, np.uint64) for i in range(G)], 1024, small=True)
    torch.cuda.synchronize()
    assert lib.nrg_group_skiplist_scan(g, sc, GE, 1024) == L.NRG_E_CAPACITY
    assert all(np.all(d[1].cpu().numpy().view(np.uint64) == CANARY) for d in keep)
    _valid(L, lib, g, ks, m, G, "after the size bound")
    L.check(lib.nrg_group_sync(g))
    L.check(lib.nrg_group_close(g))


def _raw(L, qs, limit, small=False):
    """the call's structs over canary buffers; small: one row of outputs whatever n is"""
    import torch

    sc = (L.Scan * len(qs))()
    keep = []
    for i, q in enumerate(qs):
        rows = 1 if small else max(len(q), 1)
        ok = torch.from_numpy(np.full(rows * limit, CANARY, np.uint64).view(np.int64)).cuda()
        d = (_cuda(q), ok, ok.clone(), torch.from_numpy(np.full(rows, CANARY32, np.uint32).view(np.int32)).cuda())
        sc[i].keys, sc[i].n = d[0].data_ptr(), len(q)
        sc[i].out_keys, sc[i].out_vals, sc[i].counts = d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr()
        keep.append(d)
    return sc, keep


def test_empty_and_sparse_group(nrg):
    """G = 8: an empty group (every count 0, nothing written), then a map of three keys, fewer than
    G, where at least five partitions have no candidate and every limit but 1 is above the map's size."""
    L = nrg._lib
    lib = L.load()
    G = 8
    g, ctxs = _open(L, lib, G)
    _check_all(L, lib, g, [], {}, G, (1, 5), "empty group")
    k = np.array([5, 20_000, U64_MAX], np.uint64)
    v = np.array([11, 22, 33], np.uint64)
    _push_round(L, lib, g, G, k, v, member=2)
    ks, m = _model(0, k, v)
    assert len(set(SM.key_owner(k, G).tolist())) <= 3
    _check_all(L, lib, g, ks, m, G, (1, 2, 3, 5, 1024), "three keys")
    L.check(lib.nrg_group_close(g))


def test_a_hashmap_group_is_refused(nrg):
    L = nrg._lib
    lib = L.load()
    G = 3
    g, _ = _open(L, lib, G, _cfg(L, L.NRG_DS_HASHMAP))
    rc, got = _scan_all(L, lib, g, [np.arange(5, dtype=np.uint64)] * G, L.NRG_SEEK_GE, 4)
    assert rc == L.NRG_E_INVAL
    assert all(np.all(o == CANARY) and np.all(c == CANARY32) for o, _, c in got)
    L.check(lib.nrg_group_sync(g))
    L.check(lib.nrg_group_close(g))


def _run_ranks(nrg, G, body, timeout=90):
    """body(rank, uid) on G threads that form one loopback world; the first failure is raised again"""
    from nrgpu.parallel import ReplicaGroup

    L = nrg._lib
    lib = L.load()
    out, errors = [None] * G, [None] * G
    L.check(lib.nrg_test_loopback_collectives(1))
    try:
        uid = ReplicaGroup.unique_id()

        def run(rank):
            try:
                out[rank] = body(rank, uid)
            except BaseException as e:  # noqa: BLE001
                errors[rank] = e

        ts = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(G)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout)
        assert not any(t.is_alive() for t in ts), "a rank is still running (collective never matched)"
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))
    for e in errors:
        if e is not None:
            raise e
    return out


def _rank_replica(nrg, rank, G, prefill):
    from nrgpu import DeviceReplica

    L = nrg._lib
    rep = DeviceReplica(L.NRG_DS_SKIPLIST, 0, knobs={"SL_DELTA_MAX": DELTA_MAX}, log2_slots=LOG2_SLOTS,
                        max_batch=MAX_BATCH, max_reads=MAX_READS, replica_id=rank + 1, log_bytes=LOG_BYTES)
    rep.sl_prefill_partition(prefill, OFF, rank, G)
    return rep


def _rank_round(grp, rank, k, v):
    """rank 0 pushes (k, v) in one partitioned round"""
    import torch

    dummy = torch.zeros(8, dtype=torch.int64, device="cuda")
    p = _cuda(np.stack([k, v], 1).astype(np.uint64)) if rank == 0 else None
    torch.cuda.synchronize()
    grp.round(p, len(k) if rank == 0 else 0, None, 0, dummy, dummy.view(torch.uint8))
    grp.sync()


@pytest.mark.parametrize("page", [1, 7, 1024])
def test_items_walks_the_whole_map(nrg, page):
    """PartitionedGroup.items(page), G = 3 with one thread per rank iterating in step: the sorted
    model, whether a page is one entry, a few, or more than the map holds."""
    from nrgpu.parallel import PartitionedGroup

    G, prefill = 3, 150
    k, v = _round_keys(G, seed=8)
    ks, m = _model(prefill, k, v)

    def body(rank, uid):
        rep = _rank_replica(nrg, rank, G, prefill)
        grp = PartitionedGroup(rep, rank, G, uid=uid)
        _rank_round(grp, rank, k, v)
        got = list(grp.items(page))
        grp.close()
        rep.close()
        return got

    want = [(a, m[a]) for a in ks]
    assert want[0][0] == 0 and want[-1][0] == U64_MAX and len(want) > 160
    for got in _run_ranks(nrg, G, body):
        assert got == want


def test_ranks_that_disagree_are_refused_everywhere(nrg):
    """One thread per rank, G = 2: ranks that pass different limits, or different modes, get
    NRG_E_INVAL on both sides before any data moves; the same call with equal arguments then
    answers, through PartitionedGroup.scan."""
    from nrgpu.parallel import PartitionedGroup

    L = nrg._lib
    G, prefill = 2, 150
    k, v = _round_keys(G, seed=9)
    ks, m = _model(prefill, k, v)
    q = np.array([0, 77, 149, 150, CLUSTER_AT, U64_MAX], np.uint64)
    GE, LE = L.NRG_SEEK_GE, L.NRG_SEEK_LE

    def body(rank, uid):
        rep = _rank_replica(nrg, rank, G, prefill)
        grp = PartitionedGroup(rep, rank, G, uid=uid)
        _rank_round(grp, rank, k, v)
        codes = []
        for modes, limits in (((GE, GE), (4, 5)), ((GE, LE), (4, 4)), ((LE, LE), (1024, 1)), ((GE, GE), (4, 4))):
            try:
                res = grp.scan(_cuda(q), modes[rank], limits[rank])
                codes.append(tuple(t.cpu().numpy() for t in res))
            except L.NrgError as e:
                codes.append(e.code)
        grp.close()
        rep.close()
        return codes

    for codes in _run_ranks(nrg, G, body):
        assert codes[:3] == [L.NRG_E_INVAL] * 3
        ok, ov, cnt = codes[3]
        eok, eov, ecnt = SM.scan_batch(ks, m, q, GE, 4)
        assert np.array_equal(cnt.view(np.uint32), ecnt)
        assert np.array_equal(ok.view(np.uint64), eok) and np.array_equal(ov.view(np.uint64), eov)  # zeros past the counts
