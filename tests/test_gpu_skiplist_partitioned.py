"""The key-partitioned skip list (skiplist-mlnr of benches/lockfree.rs:228-317) on the GPU, over the
loopback collectives as tests/test_gpu_group_multi.py opens its groups: partitioned rounds of Push /
Get, the group-wide seeks and range counts, nrg_skiplist_prefill_partition, and the reads of a
replicated skip-list group's round. Streams, queries and expected answers come from
tests/skiplist_part_streams.py (the sequential model replaying the global log W_0 || ... || W_{G-1});
every comparison is bit for bit."""
import ctypes as C
import threading

import numpy as np
import pytest

import skiplist_part_streams as S

pytestmark = pytest.mark.gpu

U64_MAX = S.U64_MAX
LOG_BYTES = 64 * (1 << 16)


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _cfg(L, kind=None):
    cfg = L.default_config(L.NRG_DS_SKIPLIST if kind is None else kind)
    cfg.log2_slots, cfg.max_batch, cfg.max_reads = S.LOG2_SLOTS, S.MAX_BATCH, S.MAX_READS
    cfg.log_bytes = LOG_BYTES
    return cfg


def _open(L, lib, G, cfg=None, exp=False):
    """a G-member skip-list group on device 0 over the loopback collectives, delta_max set on every
    (empty) member"""
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
            L.check(lib.nrg_test_set_knob(c, L.KNOBS["SL_DELTA_MAX"], S.DELTA_MAX))
        if exp:
            L.check(lib.nrg_test_set_knob(c, L.KNOBS["EXP"], 0x10000))
    return g, ctxs


def _dump(L, lib, ctx):
    n = C.c_uint64()
    rc = lib.nrg_skiplist_dump(ctx, None, None, 0, C.byref(n))
    assert rc in (L.NRG_OK, L.NRG_E_CAPACITY)
    k, v = np.zeros(max(n.value, 1), np.uint64), np.zeros(max(n.value, 1), np.uint64)
    m = C.c_uint64()
    L.check(lib.nrg_skiplist_dump(ctx, k.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), n.value, C.byref(m)))
    return k[:m.value], v[:m.value]


def _digest(L, lib, ctx):
    out = np.zeros(3, np.uint64)
    L.check(lib.nrg_digest(ctx, out.ctypes.data_as(C.c_void_p)))
    return tuple(int(x) for x in out)


def _round_bufs(L, rd, i, k, v, gk, want):
    """device buffers of one member's part of a round, sentinels in every output"""
    import torch

    W, R = len(k), len(gk)
    d = dict(p=_cuda(np.stack([k, v], 1).astype(np.uint64)) if W else None, gk=_cuda(gk) if R else None,
             gv=torch.full((max(R, 1),), -1, dtype=torch.int64, device="cuda"),
             gf=torch.full((max(R, 1),), 7, dtype=torch.uint8, device="cuda"),
             pv=torch.full((max(W, 1),), -1, dtype=torch.int64, device="cuda"),
             pf=torch.full((max(W, 1),), 7, dtype=torch.uint8, device="cuda"))
    rd[i].recs, rd[i].n = (d["p"].data_ptr() if W else 0), W
    rd[i].resp = d["pv"].data_ptr() if want else 0
    rd[i].some = d["pf"].data_ptr() if want else 0
    rd[i].get_keys, rd[i].n_gets = (d["gk"].data_ptr() if R else 0), R
    rd[i].get_vals, rd[i].get_found = d["gv"].data_ptr(), d["gf"].data_ptr()
    return d


def _check_round(d, k, gk, want, ans, msg, dropped=False):
    W, R = len(k), len(gk)
    if dropped:  # nothing of a dropped round is written
        assert np.all(d["pf"].cpu().numpy() == 7) and np.all(d["gf"].cpu().numpy() == 7), msg
        return
    if W and want:  # Ok(Some(key))
        np.testing.assert_array_equal(_u64(d["pv"][:W]), k, err_msg=msg + " push responses")
        assert np.all(d["pf"][:W].cpu().numpy() == 1), msg
    else:  # not asked: untouched
        assert np.all(d["pf"].cpu().numpy() == 7) and np.all(d["pv"].cpu().numpy() == -1), msg
    if R:
        np.testing.assert_array_equal(d["gf"][:R].cpu().numpy(), ans[1], err_msg=msg + " found")
        np.testing.assert_array_equal(_u64(d["gv"][:R]), ans[0], err_msg=msg + " gets")


def _check_members(L, lib, ctxs, model):
    """the partitions add up to the model; every member holds only its own keys, in order"""
    G = len(ctxs)
    digs = [_digest(L, lib, c) for c in ctxs]
    from nrgpu import digest as D

    assert D.combine(digs) == model.digest()
    assert sum(d[0] for d in digs) == len(model)
    for p, c in enumerate(ctxs):
        k, _ = _dump(L, lib, c)
        assert len(k) == digs[p][0]
        assert np.all(k[1:] > k[:-1]), f"member {p} dump not strictly ascending"
        assert np.all(S.key_owner(k, G) == p) if len(k) else True, f"member {p} holds a key it does not own"


@pytest.mark.parametrize("G,skew,pipelined,exp", [c + (False,) for c in S.ROUND_CASES] +
                         [(1, False, False, True), (1, False, True, True)])
def test_partitioned_rounds(nrg, G, skew, pipelined, exp):
    """Partitioned rounds of a skip-list group: every Get equals the model's, Push responses are the
    keys where asked, the members' digests add up to the model's and every member holds exactly
    the keys it owns. skew: owner 0 receives G * 4000 Puts and all Gets of a round (replay slices
    of max_batch, read slices of max_reads). exp: the one-rank group moves its data (EXP bit 16)."""
    import torch

    L = nrg._lib
    lib = L.load()
    n = S.n_rounds(pipelined)
    rs = S.rounds(G, skew)[:n]
    model, answers = S.expected(G, skew, n)
    g, ctxs = _open(L, lib, G, exp=exp)
    for p, c in enumerate(ctxs):
        L.check(lib.nrg_skiplist_prefill_partition(c, S.PREFILL, 0, p, G))
    posted = []
    for r, parts in enumerate(rs):
        rd = (L.Round * G)()
        keep = [_round_bufs(L, rd, i, k, v, gk, want) for i, (k, v, gk, want) in enumerate(parts)]
        torch.cuda.synchronize()
        if pipelined:
            L.check(lib.nrg_group_partitioned_round_async(g, rd), f"round {r} (completes round {r - 1})")
        else:
            L.check(lib.nrg_group_partitioned_round(g, rd), f"round {r}")
            L.check(lib.nrg_group_sync(g))
        posted.append((rd, keep))
    if pipelined:
        L.check(lib.nrg_group_partitioned_flush(g), "flush")
    L.check(lib.nrg_group_sync(g))
    for r, (parts, (_, keep)) in enumerate(zip(rs, posted)):
        for i, (k, _, gk, want) in enumerate(parts):
            _check_round(keep[i], k, gk, want, answers[r][i], f"G={G} round {r} member {i}")
    _check_members(L, lib, ctxs, model)
    L.check(lib.nrg_group_close(g))


@pytest.mark.parametrize("G", [1, 3])
def test_pipelined_run_drops_a_bad_round(nrg, G):
    """Member 0 posts Puts without records in round 2 of a pipelined run: the call that moves it (of
    round 3) returns NRG_E_INVAL on the whole group, nothing of round 2 is written -- its Push
    response buffers keep their sentinel -- and the other rounds answer as the log without it."""
    import torch

    L = nrg._lib
    lib = L.load()
    rs = S.drop_rounds(G)
    model, answers = S.expected_drop(G)
    g, ctxs = _open(L, lib, G)
    for p, c in enumerate(ctxs):
        L.check(lib.nrg_skiplist_prefill_partition(c, 3000, 0, p, G))
    posted = []
    for r, parts in enumerate(rs):
        rd = (L.Round * G)()
        keep = [_round_bufs(L, rd, i, k, v, gk, want) for i, (k, v, gk, want) in enumerate(parts)]
        if r == 2:
            rd[0].recs = 0
        torch.cuda.synchronize()
        rc = lib.nrg_group_partitioned_round_async(g, rd)
        assert rc == (L.NRG_E_INVAL if r == 3 else L.NRG_OK), (r, rc)
        posted.append((rd, keep))
    L.check(lib.nrg_group_partitioned_flush(g), "flush")
    L.check(lib.nrg_group_sync(g))
    for r, (parts, (_, keep)) in enumerate(zip(rs, posted)):
        for i, (k, _, gk, want) in enumerate(parts):
            _check_round(keep[i], k, gk, want, answers[r][i] if r != 2 else None, f"G={G} round {r} member {i}",
                         dropped=r == 2)
    _check_members(L, lib, ctxs, model)
    L.check(lib.nrg_group_close(g))


def _seek_all(L, lib, g, qs, mode):
    """one nrg_group_skiplist_seek over the members' keys `qs`; (rc, per member (keys, vals, found))"""
    import torch

    G = len(qs)
    sk = (L.Seek * G)()
    keep = []
    for i, q in enumerate(qs):
        n = len(q)
        d = (_cuda(q) if n else None, torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda"),
             torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda"),
             torch.full((max(n, 1),), 7, dtype=torch.uint8, device="cuda"))
        sk[i].keys, sk[i].n = (d[0].data_ptr() if n else 0), n
        sk[i].out_keys, sk[i].out_vals, sk[i].found = d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr()
        keep.append(d)
    torch.cuda.synchronize()
    rc = lib.nrg_group_skiplist_seek(g, sk, mode)
    return rc, [(_u64(d[1])[:len(q)], _u64(d[2])[:len(q)], d[3].cpu().numpy()[:len(q)]) for d, q in zip(keep, qs)], keep


def _count_all(L, lib, g, cq):
    import torch

    G = len(cq)
    ct = (L.Count * G)()
    keep = []
    for i, (lo, hi) in enumerate(cq):
        n = len(lo)
        d = (_cuda(lo) if n else None, _cuda(hi) if n else None,
             torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda"))
        ct[i].los, ct[i].his, ct[i].n = (d[0].data_ptr() if n else 0), (d[1].data_ptr() if n else 0), n
        ct[i].counts = d[2].data_ptr()
        keep.append(d)
    torch.cuda.synchronize()
    rc = lib.nrg_group_skiplist_range_count(g, ct)
    return rc, [_u64(d[2])[:len(lo)] for d, (lo, _) in zip(keep, cq)]


def _check_reads(L, lib, g, model, keys_for_queries, G, what):
    """all four seek modes and a range count of ragged query sets, against the model"""
    for mode in S.MODES:
        qs = S.seek_queries(keys_for_queries, G, mode)
        rc, got, keep = _seek_all(L, lib, g, qs, mode)
        assert rc == L.NRG_OK, (what, mode, rc)
        for i, q in enumerate(qs):
            ok, ov, f = S.seek_expected(model, q, mode)
            msg = f"{what} G={G} mode {mode} member {i} (n = {len(q)})"
            np.testing.assert_array_equal(got[i][2], f, err_msg=msg + " found")
            np.testing.assert_array_equal(got[i][0], ok, err_msg=msg + " keys")
            np.testing.assert_array_equal(got[i][1], ov, err_msg=msg + " vals")
            if not len(q):  # nothing asked: nothing written
                assert keep[i][3].cpu().numpy()[0] == 7, msg
    cq = S.count_queries(keys_for_queries, G)
    rc, got = _count_all(L, lib, g, cq)
    assert rc == L.NRG_OK, (what, rc)
    for i, (lo, hi) in enumerate(cq):
        np.testing.assert_array_equal(got[i], S.count_expected(model, lo, hi), err_msg=f"{what} G={G} counts of member {i}")


@pytest.mark.parametrize("G,exp", [(1, False), (1, True), (3, False), (8, False)])
def test_group_wide_seek_and_range_count(nrg, G, exp):
    """nrg_group_skiplist_seek / _range_count after two partitioned rounds, the second still posted
    when the first read is called: ragged n per member (0, 1, 257, 1000), all four modes, queries
    at 0, 2^64 - 1, present keys and gaps, lo > hi. A bad mode and a member with keys but no output
    buffers are refused on the whole group, which stays usable. A one-rank group answers straight
    into the caller's buffers; exp (EXP bit 16) sends it down the general path."""
    import torch

    L = nrg._lib
    lib = L.load()
    rs = S.rounds(G, False)[:2]
    model = S.seek_state(G)
    g, ctxs = _open(L, lib, G, exp=exp)
    for p, c in enumerate(ctxs):
        L.check(lib.nrg_skiplist_prefill_partition(c, S.PREFILL, 0, p, G))
    hold = []
    for r, parts in enumerate(rs):
        rd = (L.Round * G)()
        hold.append((rd, [_round_bufs(L, rd, i, k, v, gk, want) for i, (k, v, gk, want) in enumerate(parts)]))
        torch.cuda.synchronize()
        L.check(lib.nrg_group_partitioned_round_async(g, rd), f"round {r}")  # completed by the first read below
    keys = model.arrays()[0]
    qs = S.seek_queries(keys, G, L.NRG_SEEK_LT)
    assert _seek_all(L, lib, g, qs, L.NRG_SEEK_LT + 1)[0] == L.NRG_E_INVAL
    _check_reads(L, lib, g, model, keys, G, "after two rounds")
    # a member that asks without buffers: refused everywhere, before any data moves
    big = max(range(G), key=lambda i: len(qs[i]))
    sk = (L.Seek * G)()
    d = _cuda(qs[big])
    sk[big].keys, sk[big].n = d.data_ptr(), len(qs[big])
    assert lib.nrg_group_skiplist_seek(g, sk, L.NRG_SEEK_GE) == L.NRG_E_INVAL
    ct = (L.Count * G)()
    ct[big].los, ct[big].n = d.data_ptr(), len(qs[big])
    assert lib.nrg_group_skiplist_range_count(g, ct) == L.NRG_E_INVAL
    # n = 0 on every rank
    assert lib.nrg_group_skiplist_seek(g, (L.Seek * G)(), L.NRG_SEEK_GE) == L.NRG_OK
    assert lib.nrg_group_skiplist_range_count(g, (L.Count * G)()) == L.NRG_OK
    _check_reads(L, lib, g, model, keys, G, "after the refused calls")
    _check_members(L, lib, ctxs, model)
    L.check(lib.nrg_group_close(g))


def test_seek_on_an_empty_and_on_a_sparse_group(nrg):
    """G = 8: the same queries on an empty group (nothing found, every count 0) and on a group of
    three keys, where at least five partitions are empty and answer "none" for every query."""
    import torch

    import skiplist_model as M

    L = nrg._lib
    lib = L.load()
    G = 8
    g, ctxs = _open(L, lib, G)
    keys = S.seek_state(G).arrays()[0]  # the query sets of the populated case
    model = M.SkipListModel()
    _check_reads(L, lib, g, model, keys, G, "empty group")
    rd = (L.Round * G)()
    vals = np.array([11, 22, 33], np.uint64)
    z = np.zeros(0, np.uint64)
    keep = [_round_bufs(L, rd, i, S.SPARSE_KEYS if i == 2 else z, vals if i == 2 else z, z, False) for i in range(G)]
    torch.cuda.synchronize()
    L.check(lib.nrg_group_partitioned_round(g, rd))
    model.insert_many(S.SPARSE_KEYS.tolist(), vals.tolist())
    _check_reads(L, lib, g, model, keys, G, "three keys")
    _check_reads(L, lib, g, model, S.SPARSE_KEYS, G, "three keys, queries around them")
    _check_members(L, lib, ctxs, model)
    assert keep
    L.check(lib.nrg_group_close(g))


def test_group_wide_reads_refuse_a_hashmap_group(nrg):
    L = nrg._lib
    lib = L.load()
    cfg = _cfg(L, L.NRG_DS_HASHMAP)
    g, _ = _open(L, lib, 3, cfg)
    qs = [np.arange(5, dtype=np.uint64)] * 3
    assert _seek_all(L, lib, g, qs, L.NRG_SEEK_GE)[0] == L.NRG_E_INVAL
    assert _count_all(L, lib, g, [(q, q) for q in qs])[0] == L.NRG_E_INVAL
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


def test_one_rank_per_thread(nrg):
    """nrg_group_join, G = 3, one thread per rank through nrgpu.parallel.PartitionedGroup: two
    partitioned rounds, one group-wide seek and one range count between separate callers."""
    import torch

    from nrgpu import DeviceReplica
    from nrgpu.parallel import PartitionedGroup

    L = nrg._lib
    G = 3
    rs = S.rounds(G, False)[:2]
    model = S.seek_state(G)
    _, answers = S.expected(G, False, 4)
    keys = model.arrays()[0]
    mode = L.NRG_SEEK_LE
    qs = S.seek_queries(keys, G, mode)
    cq = S.count_queries(keys, G)

    def body(rank, uid):
        rep = DeviceReplica(L.NRG_DS_SKIPLIST, 0, knobs={"SL_DELTA_MAX": S.DELTA_MAX}, log2_slots=S.LOG2_SLOTS,
                            max_batch=S.MAX_BATCH, max_reads=S.MAX_READS, replica_id=rank + 1, log_bytes=LOG_BYTES)
        rep.sl_prefill_partition(S.PREFILL, 0, rank, G)
        grp = PartitionedGroup(rep, rank, G, uid=uid)
        res = []
        for parts in rs:
            k, v, gk, want = parts[rank]
            rd = (L.Round * 1)()
            d = _round_bufs(L, rd, 0, k, v, gk, want)
            torch.cuda.synchronize()
            grp.round(d["p"], len(k), d["gk"], len(gk), d["gv"], d["gf"], d["pv"] if want else None,
                      d["pf"] if want else None)
            grp.sync()
            res.append(d)
        sk = grp.seek(_cuda(qs[rank]), mode)
        cnt = grp.range_count(_cuda(cq[rank][0]), _cuda(cq[rank][1]))
        got = (_u64(sk[0]), _u64(sk[1]), sk[2].cpu().numpy(), _u64(cnt), rep.digest(), rep.sl_dump()[0])
        grp.close()
        rep.close()
        return res, got

    out = _run_ranks(nrg, G, body)
    from nrgpu import digest as D

    assert D.combine([o[1][4] for o in out]) == model.digest()
    for rank in range(G):
        res, (ok, ov, f, cnt, _, dk) = out[rank]
        for r, parts in enumerate(rs):
            k, _, gk, want = parts[rank]
            _check_round(res[r], k, gk, want, answers[r][rank], f"round {r} rank {rank}")
        eok, eov, ef = S.seek_expected(model, qs[rank], mode)
        np.testing.assert_array_equal(f, ef, err_msg=f"rank {rank} seek found")
        np.testing.assert_array_equal(ok, eok, err_msg=f"rank {rank} seek keys")
        np.testing.assert_array_equal(ov, eov, err_msg=f"rank {rank} seek vals")
        np.testing.assert_array_equal(cnt, S.count_expected(model, *cq[rank]), err_msg=f"rank {rank} counts")
        assert np.all(S.key_owner(dk, G) == rank) and np.all(dk[1:] > dk[:-1])


def test_ranks_that_disagree_are_refused_everywhere(nrg):
    """One thread per rank, G = 2. A skip-list rank and a hashmap rank in one group: the partitioned
    round returns NRG_E_INVAL on both before any payload moves (the exchanged words carry the
    kind), and so does a group-wide seek. Two skip-list ranks that pass different seek modes: the
    same; with the same mode the group then answers."""
    import torch

    from nrgpu import DeviceReplica
    from nrgpu.parallel import PartitionedGroup

    L = nrg._lib
    G = 2
    k = np.arange(100, 164, dtype=np.uint64)

    def body_for(kinds, modes):
        def body(rank, uid):
            kw = dict(log2_slots=12, max_batch=1024, max_reads=1024, replica_id=rank + 1, log_bytes=LOG_BYTES)
            rep = DeviceReplica(kinds[rank], 0, **kw)
            grp = PartitionedGroup(rep, rank, G, uid=uid)
            rd = (L.Round * 1)()
            d = _round_bufs(L, rd, 0, k, k, k, True)
            torch.cuda.synchronize()
            codes = [0, 0, None]
            try:
                grp.round(d["p"], len(k), d["gk"], len(k), d["gv"], d["gf"], d["pv"], d["pf"])
                grp.sync()
            except L.NrgError as e:
                codes[0] = e.code
            try:
                sk = grp.seek(_cuda(k), modes[rank])
                codes[2] = (_u64(sk[0]), sk[2].cpu().numpy())
            except L.NrgError as e:
                codes[1] = e.code
            untouched = bool(np.all(d["pf"].cpu().numpy() == 7) and np.all(d["gf"].cpu().numpy() == 7))
            grp.close()
            rep.close()
            return codes, untouched

        return body

    SL, HM = L.NRG_DS_SKIPLIST, L.NRG_DS_HASHMAP
    for codes, untouched in _run_ranks(nrg, G, body_for((SL, HM), (0, 0))):
        assert codes[:2] == [L.NRG_E_INVAL, L.NRG_E_INVAL] and untouched
    for codes, untouched in _run_ranks(nrg, G, body_for((SL, SL), (L.NRG_SEEK_GE, L.NRG_SEEK_LE))):
        assert codes[:2] == [L.NRG_OK, L.NRG_E_INVAL] and not untouched
    for codes, _ in _run_ranks(nrg, G, body_for((SL, SL), (L.NRG_SEEK_GE, L.NRG_SEEK_GE))):
        assert codes[:2] == [L.NRG_OK, L.NRG_OK]
        np.testing.assert_array_equal(codes[2][0], k)  # both ranks pushed and ask for the same keys
        assert np.all(codes[2][1] == 1)


@pytest.mark.parametrize("G", [1, 8])
@pytest.mark.parametrize("n", [0, 5, 6000])
def test_prefill_partition(nrg, G, n):
    """The union of the members' dumps is 0..n-1 -> k + off, each key at its owner."""
    L = nrg._lib
    off = 7
    seen = []
    for p in range(G):
        dev = nrg.DeviceReplica(L.NRG_DS_SKIPLIST, 0, knobs={"SL_DELTA_MAX": S.DELTA_MAX}, log2_slots=S.LOG2_SLOTS,
                                max_batch=S.MAX_BATCH, log_bytes=LOG_BYTES)
        dev.sl_prefill_partition(n, off, p, G)
        k, v = dev.sl_dump()
        assert dev.sl_len() == len(k)
        dev.close()
        assert np.all(S.key_owner(k, G) == p) if len(k) else True
        assert np.array_equal(v, k + np.uint64(off)) and np.all(k[1:] > k[:-1])
        want = np.concatenate(S.prefill_slices(n, p, G) or [np.zeros(0, np.uint64)])
        assert np.array_equal(k, want)
        seen.append(k)
    assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(n, dtype=np.uint64))


def test_prefill_partition_arguments_and_growth(nrg):
    L = nrg._lib
    lib = L.load()
    dev = nrg.DeviceReplica(L.NRG_DS_SKIPLIST, 0, log2_slots=10, max_batch=S.MAX_BATCH, log_bytes=LOG_BYTES)
    for part, parts in ((1, 1), (8, 8), (0, 0), (0, L.NRG_MAX_PARTS + 1)):
        assert lib.nrg_skiplist_prefill_partition(dev.handle, 100, 0, part, parts) == L.NRG_E_INVAL
    assert dev.sl_len() == 0
    # the prefilled keys count towards automatic growth: 3000 of them into a map of 1024
    dev.set_max_capacity(1 << 14)
    dev.sl_prefill_partition(6000, 1, 0, 2)
    want = S.prefill_slices(6000, 0, 2)
    want = np.concatenate(want)
    assert len(want) > 1024 and dev.sl_capacity() >= len(want)
    k, v = dev.sl_dump()
    assert np.array_equal(k, want) and np.array_equal(v, want + np.uint64(1))
    dev.close()
    hm = nrg.DeviceReplica(L.NRG_DS_HASHMAP, 0, log2_slots=12, max_batch=1024, log_bytes=LOG_BYTES)
    assert lib.nrg_skiplist_prefill_partition(hm.handle, 100, 0, 0, 1) == L.NRG_E_INVAL
    hm.close()


def test_replicated_group_round_answers_gets(nrg):
    """A replicated skip-list group (nrg_group_round_async), G = 3: a round's Gets (3000 of one
    member, more than max_reads) are answered against the post-round state, as the model's."""
    import torch

    L = nrg._lib
    lib = L.load()
    G = 3
    rs = S.rounds(G, False)[:2]
    model = S.seek_state(G)
    _, answers = S.expected(G, False, 4)
    g, ctxs = _open(L, lib, G)
    for c in ctxs:
        L.check(lib.nrg_skiplist_prefill_range(c, S.PREFILL, 0))
    posted = []
    for r, parts in enumerate(rs):
        rd = (L.Round * G)()
        keep = [_round_bufs(L, rd, i, k, v, gk, want) for i, (k, v, gk, want) in enumerate(parts)]
        torch.cuda.synchronize()
        L.check(lib.nrg_group_round_async(g, rd, None), f"round {r}")
        posted.append((rd, keep))
    L.check(lib.nrg_group_sync(g))
    assert max(len(gk) for parts in rs for (_, _, gk, _) in parts) > S.MAX_READS
    for r, (parts, (_, keep)) in enumerate(zip(rs, posted)):
        for i, (k, _, gk, want) in enumerate(parts):
            _check_round(keep[i], k, gk, want, answers[r][i], f"replicated round {r} member {i}")
    mk, mv = model.arrays()
    for i, c in enumerate(ctxs):
        k, v = _dump(L, lib, c)
        assert np.array_equal(k, mk) and np.array_equal(v, mv), f"member {i}"
    L.check(lib.nrg_group_close(g))
