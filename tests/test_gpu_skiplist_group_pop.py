"""nrg_group_skiplist_pop and the mark-record refusal of a skip-list group that agreed on pops
(nrg_group_skiplist_enable_pops), over the loopback collectives: every rank's resp, some, packed entries and
*pop_n equal tests/skiplist_group_pop_model.py's UnionModel for the concatenated run, and the union of the
members afterwards equals the model, on the named streams of that module. Groups are opened as
tests/test_gpu_skiplist_scan_group.py opens them (log2_slots 12, max_batch 2048, SL_DELTA_MAX 64). Guard
words surround every output, and canaries sit past every count and past pop_cap."""
import ctypes as C

import numpy as np
import pytest

import skiplist_group_gpu as U
import skiplist_group_pop_model as GM

pytestmark = pytest.mark.gpu

FRONT, BACK, TOMB, U64_MAX = GM.FRONT, GM.BACK, GM.TOMB, GM.U64_MAX


def _state(L, lib, G, exp, s):
    """the stream's state on a fresh group that agreed on pops; (g, ctxs, model)"""
    g, ctxs = U.open_group(L, lib, G, exp=exp)
    if s.enable_first:
        L.check(lib.nrg_group_skiplist_enable_pops(g, FRONT, BACK), "enable_pops")
    U.prefill(L, lib, ctxs, s.prefill(G))
    for k, v in s.rounds(G):
        U.push_round(L, lib, g, G, k, v)
    if not s.enable_first:
        L.check(lib.nrg_group_skiplist_enable_pops(g, FRONT, BACK), "enable_pops")
    L.check(lib.nrg_group_skiplist_enable_pops(g, FRONT, BACK), "enable_pops again")
    return g, ctxs, s.state(G)


def _caps(reqs, length, short=None):
    caps = [sum(min(n, length) for n, _ in mine) for mine in reqs]
    if short is not None:
        caps[short[0]] = short[1]
    return caps


@pytest.mark.parametrize("G,exp", U.CASES)
@pytest.mark.parametrize("name", GM.NAMES)
def test_group_pop_streams(nrg, name, G, exp):
    L = nrg._lib
    lib = L.load()
    s = GM.by_name(name)
    g, ctxs, model = _state(L, lib, G, exp, s)
    U.check_members(L, lib, ctxs, model, f"{name} G={G} before")
    reqs = s.reqs(G, len(model.keys))
    caps = _caps(reqs, len(model.keys), s.cap(G) if s.cap else None)
    rc, keep = U.group_pop(L, lib, g, reqs, caps)
    assert rc == L.NRG_OK, (name, G, rc)
    want = U.check_pop(keep, reqs, model, f"{name} G={G} exp={exp}")
    if s.cap:
        rank, cap = s.cap(G)
        assert int(want[rank][0].sum()) > cap == keep[rank].cap
    U.check_members(L, lib, ctxs, model, f"{name} G={G} exp={exp} after")
    if name == "meet":  # the map is empty: a further pop answers None everywhere
        assert len(model.keys) == 0
        again = [[(1, 0), (2, 1)] for _ in range(G)]
        rc, keep = U.group_pop(L, lib, g, again, [3] * G)
        assert rc == L.NRG_OK
        U.check_pop(keep, again, model, f"{name} G={G} empty")
        assert all(b.resp.inner().tolist() == [0, 0] and b.some.inner().tolist() == [0, 0] for b in keep)
    L.check(lib.nrg_group_sync(g))
    L.check(lib.nrg_group_close(g))


def test_against_a_single_replica_holding_the_union(nrg):
    """ragged, G = 3: the concatenated run through nrg_skiplist_round_pops_async on one replica that holds the
    whole map gives every rank's answers (the definition of the group-wide pop)."""
    import torch

    L = nrg._lib
    lib = L.load()
    G = 3
    s = GM.by_name("ragged")
    g, ctxs, model = _state(L, lib, G, False, s)
    reqs = s.reqs(G, len(model.keys))
    caps = _caps(reqs, len(model.keys))
    rc, keep = U.group_pop(L, lib, g, reqs, caps)
    assert rc == L.NRG_OK
    one = nrg.DeviceReplica(L.NRG_DS_SKIPLIST, 0, knobs={"SL_DELTA_MAX": U.DELTA_MAX}, log2_slots=U.LOG2_SLOTS,
                            max_batch=U.MAX_BATCH, max_reads=U.MAX_READS, log_bytes=U.LOG_BYTES)
    one.sl_prefill_range(s.prefill(G), GM.OFF)
    for k, v in s.rounds(G):
        recs = np.zeros(len(k), nrg.PUT_DTYPE)
        recs["key"], recs["val"] = k, v
        one.log_exec(one.log_append(recs, 1))
    one.sl_enable_pops(FRONT, BACK)
    run = np.array([(n, BACK if back else FRONT) for mine in reqs for n, back in mine], np.uint64).reshape(-1, 2)
    n, cap = len(run), sum(caps)
    d_ops = U.cuda(run)
    resp, some = U.Guarded(n), U.Guarded(n, byte=True)
    pk, pv, total = U.Guarded(cap), U.Guarded(cap), U.Guarded(1)
    torch.cuda.synchronize()
    L.check(lib.nrg_skiplist_round_pops_async(one._h, d_ops.data_ptr(), n, 1, resp.ptr, some.ptr, pk.ptr, pv.ptr, cap,
                                              total.ptr))
    L.check(lib.nrg_sync(one._h))
    r1, off, at = resp.inner(), 0, 0
    assert int(total.inner()[0]) == int(r1.sum())
    for i, mine in enumerate(reqs):
        cnt = r1[at:at + len(mine)]
        m = int(cnt.sum())
        np.testing.assert_array_equal(keep[i].resp.inner(), cnt)
        np.testing.assert_array_equal(keep[i].some.inner(), some.inner()[at:at + len(mine)])
        np.testing.assert_array_equal(keep[i].keys.inner()[:m], pk.inner()[off:off + m])
        np.testing.assert_array_equal(keep[i].vals.inner()[:m], pv.inner()[off:off + m])
        if mine:
            assert int(keep[i].total.inner()[0]) == m
        at, off = at + len(mine), off + m
    from nrgpu import digest as D

    assert D.combine([U.digest(L, lib, c) for c in ctxs]) == one.digest()
    one.close()
    L.check(lib.nrg_group_close(g))


@pytest.mark.parametrize("G,exp", [(1, False), (3, False)])
def test_work_list_loop(nrg, G, exp):
    """Push round, pop, Push round, pop, ...: a priority queue over the partitioned map stays equal to the model"""
    L = nrg._lib
    lib = L.load()
    g, ctxs, model = _state(L, lib, G, exp, GM.by_name("single"))
    rng = np.random.default_rng(17)
    for it in range(4):
        parts = []
        for i in range(G):
            k = rng.integers(0, 4000, 30, dtype=np.uint64)
            parts.append((np.stack([k, k * np.uint64(3) + np.uint64(it)], 1), k[:5], True))
        rc, rd, keep = U.post_round(L, lib, g, parts)
        assert rc == L.NRG_OK
        L.check(lib.nrg_group_sync(g))
        U.check_round(keep, parts, model, f"G={G} push round {it}")
        reqs = [[(20 + i, 0), (3, 1)] if (i + it) % 2 == 0 else [(1, 1)] for i in range(G)]
        rc, pk = U.group_pop(L, lib, g, reqs, _caps(reqs, len(model.keys)))
        assert rc == L.NRG_OK
        U.check_pop(pk, reqs, model, f"G={G} pop {it}")
    U.check_members(L, lib, ctxs, model, f"G={G} work list")
    L.check(lib.nrg_group_close(g))


@pytest.mark.parametrize("G,exp", [(1, False), (1, True), (3, False)])
def test_a_round_with_a_mark_record_is_refused(nrg, G, exp):
    """On a pops group a round that holds a mark record on one rank gives NRG_E_INVAL on every rank, in the
    synchronous and the pipelined form: nothing written, no log moved; the next clean round works."""
    L = nrg._lib
    lib = L.load()
    g, ctxs, model = _state(L, lib, G, exp, GM.by_name("single"))
    bad = G - 1
    clean = lambda i: (np.array([(7000 + i, 1), (7100 + i, 2)], np.uint64), np.array([7000 + i, 5], np.uint64), True)
    parts = [clean(i) for i in range(G)]
    parts[bad] = (np.array([(7000, 1), (3, BACK), (7001, 2)], np.uint64), parts[bad][1], True)
    before = U.log_tails(L, lib, ctxs)
    launches = (C.c_uint64 * 4)()
    L.check(lib.nrg_test_group_launches(g, launches))
    marks_before = launches[3]
    rc, rd, keep = U.post_round(L, lib, g, parts)
    assert rc == L.NRG_E_INVAL
    rc1, rd1, keep1 = U.post_round(L, lib, g, parts, pipelined=True)
    rc2 = lib.nrg_group_partitioned_flush(g)
    assert (rc1, rc2) in ((L.NRG_E_INVAL, L.NRG_OK), (L.NRG_OK, L.NRG_E_INVAL)), (rc1, rc2)
    L.check(lib.nrg_group_sync(g))
    assert all(b.all_untouched() for b in keep + keep1)
    assert U.log_tails(L, lib, ctxs) == before
    L.check(lib.nrg_test_group_launches(g, launches))
    assert launches[3] == marks_before + 2 * G  # one mark pass per member with records and posted round
    U.check_members(L, lib, ctxs, model, f"G={G} after the refused rounds")
    parts = [clean(i) for i in range(G)]
    parts[0] = (np.array([(7000, 1), (FRONT, 9), (BACK, 8)], np.uint64), parts[0][1], True)  # marks as KEYS are Pushes
    rc, rd, keep = U.post_round(L, lib, g, parts)
    assert rc == L.NRG_OK
    L.check(lib.nrg_group_sync(g))
    U.check_round(keep, parts, model, f"G={G} the clean round")
    U.check_members(L, lib, ctxs, model, f"G={G} after the clean round")
    L.check(lib.nrg_group_close(g))


def test_refusals_of_the_pop(nrg):
    """A group that has not agreed: NRG_E_INVAL. On one that has: the bad arguments of the table, each
    refused on every rank with nothing written and the group usable; n = 0 everywhere is NRG_OK."""
    import torch

    L = nrg._lib
    lib = L.load()
    G = 3
    g, ctxs = U.open_group(L, lib, G)
    U.prefill(L, lib, ctxs, 200)
    model = GM.UnionModel()
    model.prefill(200)
    reqs = [[(2, 0)], [], [(1, 1), (3, 0)]]
    rc, keep = U.group_pop(L, lib, g, reqs, [4, 4, 4])
    assert rc == L.NRG_E_INVAL and all(b.all_untouched() for b in keep)
    # marks equal to each other: refused, nothing enabled
    assert lib.nrg_group_skiplist_enable_pops(g, FRONT, FRONT) == L.NRG_E_INVAL
    on = C.c_int(7)
    L.check(lib.nrg_skiplist_pops(ctxs[0], None, None, C.byref(on)))
    assert on.value == 0
    L.check(lib.nrg_group_skiplist_enable_pops(g, FRONT, BACK))
    assert lib.nrg_group_skiplist_enable_pops(g, BACK, FRONT) == L.NRG_E_INVAL
    assert lib.nrg_group_skiplist_enable_removal(g, FRONT) == L.NRG_E_INVAL  # a mark cannot be the tombstone
    before = U.log_tails(L, lib, ctxs)

    def refused(mutate, code=L.NRG_E_INVAL):
        q = (L.Pops * G)()
        bufs = [U.PopBufs(L, q, i, reqs[i], 4) for i in range(G)]
        mutate(q, bufs)
        torch.cuda.synchronize()
        assert lib.nrg_group_skiplist_pop(g, q) == code
        assert all(b.all_untouched() for b in bufs)

    def null_reqs(q, b):
        q[0].reqs = None

    def resp_without_some(q, b):
        q[2].some = 0

    def some_without_resp(q, b):
        q[2].resp = 0

    def null_array(q, b):
        q[0].pop_vals = 0

    def null_total(q, b):
        q[2].pop_n = 0

    def bad_end(q, b):
        b[2].arr[1].back = 2

    def too_many(q, b):
        q[0].n = 1 << 32

    for f in (null_reqs, resp_without_some, some_without_resp, null_array, null_total, bad_end):
        refused(f)
    refused(too_many, L.NRG_E_CAPACITY)

    def too_long_to_stage(q, b):  # G * nmax > 2^24 requests: agreed from the exchanged n, nothing allocated
        n = (1 << 24) // G + 1
        b[1].arr = (L.PopReq * n)()
        q[1].reqs, q[1].n = b[1].arr, n

    refused(too_long_to_stage, L.NRG_E_CAPACITY)
    assert lib.nrg_group_skiplist_pop(g, None) == L.NRG_E_INVAL
    assert U.log_tails(L, lib, ctxs) == before
    assert lib.nrg_group_skiplist_pop(g, (L.Pops * G)()) == L.NRG_OK  # n = 0 on every rank
    assert U.log_tails(L, lib, ctxs) == before
    # a member behind its log
    recs = np.zeros(1, nrg.PUT_DTYPE)
    recs["key"], recs["val"] = 900, 1
    first = C.c_uint64()
    L.check(lib.nrg_log_append(ctxs[1], recs.ctypes.data_as(C.c_void_p), 1, 2, C.byref(first)))
    rc, keep = U.group_pop(L, lib, g, reqs, [4, 4, 4])
    assert rc == L.NRG_E_NOT_SYNCED and all(b.all_untouched() for b in keep)
    L.check(lib.nrg_log_exec(ctxs[1], 0, 0, None, None))
    model.push(900, 1)  # (appended on member 1 directly, whoever owns the key: only the union is compared below)
    rc, keep = U.group_pop(L, lib, g, reqs, [4, 4, 4])
    assert rc == L.NRG_OK
    U.check_pop(keep, reqs, model, "after the refusals")
    L.check(lib.nrg_group_close(g))


@pytest.mark.parametrize("G", [1, 3])
def test_a_plain_group_launches_what_it_launched(nrg, G):
    """A Push-only round on a group that agreed on nothing: per member one fused partition and one route-back
    launch (none in the one-rank identity form), the asker-side Push response launch where responses were
    asked, no mark pass, and no removal or pop kernel in the members' replays. Then the same round on a
    group that agreed on removal launches no asker-side response kernel, and on one that agreed on pops a
    mark pass per member with records."""
    L = nrg._lib
    lib = L.load()
    k = np.arange(100, 160, dtype=np.uint64)

    def parts():
        return [(np.stack([k + np.uint64(1000 * i), k], 1), k[:4], i != 1) for i in range(G)]

    def counts(g):
        out = (C.c_uint64 * 4)()
        L.check(lib.nrg_test_group_launches(g, out))
        return list(out)

    def one_round(g, ctxs, timed):
        for c in ctxs:
            L.check(lib.nrg_kernel_timing(c, 1 if timed else 0))
        before = counts(g)
        rc, rd, keep = U.post_round(L, lib, g, parts())
        assert rc == L.NRG_OK
        L.check(lib.nrg_group_sync(g))
        return [a - b for a, b in zip(counts(g), before)]

    def kernel_launches(ctxs, name):
        tot = 0
        for c in ctxs:
            n, ms = C.c_uint64(), C.c_double()
            L.check(lib.nrg_kernel_time(c, name.encode(), C.byref(n), C.byref(ms)))
            tot += n.value
        return tot

    moved = 0 if G == 1 else G                 # the identity form moves nothing
    asked = 0 if G == 1 else G - 1             # members that passed resp / some (the identity replay answers itself)
    g, ctxs = U.open_group(L, lib, G)
    U.prefill(L, lib, ctxs, 300)
    assert one_round(g, ctxs, True) == [moved, moved, asked, 0]
    for name in ("sl_rm_resp", "sl_rm_state", "sl_pop_find", "sl_pop_plan", "sl_peek"):
        assert kernel_launches(ctxs, name) == 0, name
    L.check(lib.nrg_group_skiplist_enable_removal(g, TOMB))
    assert one_round(g, ctxs, False) == [moved, moved, 0, 0]
    L.check(lib.nrg_group_skiplist_enable_pops(g, FRONT, BACK))
    assert one_round(g, ctxs, False) == [moved, moved, 0, G]
    L.check(lib.nrg_group_close(g))


def test_python_methods_on_a_one_rank_group(nrg):
    """PartitionedGroup.enable_removal / enable_pops / pop / pop_front / pop_back, one rank over the loopback"""
    import torch

    from nrgpu.parallel import PartitionedGroup, ReplicaGroup

    L = nrg._lib
    lib = L.load()
    rep = nrg.DeviceReplica(L.NRG_DS_SKIPLIST, 0, knobs={"SL_DELTA_MAX": U.DELTA_MAX}, log2_slots=U.LOG2_SLOTS,
                            max_batch=U.MAX_BATCH, max_reads=U.MAX_READS, replica_id=1, log_bytes=U.LOG_BYTES)
    rep.sl_prefill_range(100, 5)  # keys 0 .. 99 -> k + 5
    L.check(lib.nrg_test_loopback_collectives(1))
    try:
        grp = PartitionedGroup(rep, 0, 1, uid=ReplicaGroup.unique_id())
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))
    with pytest.raises(L.NrgError) as e:
        grp.pop_front()
    assert e.value.code == L.NRG_E_INVAL
    grp.enable_removal()
    grp.enable_pops()
    assert rep.sl_removal() == TOMB and rep.sl_pops() == (FRONT, BACK)
    cnt, k, v = grp.pop_front(3)
    assert cnt.tolist() == [3] and k.tolist() == [0, 1, 2] and v.tolist() == [5, 6, 7]
    cnt, k, v = grp.pop_back()
    assert cnt.tolist() == [1] and k.tolist() == [99] and v.tolist() == [104]
    cnt, k, v = grp.pop([(2, 1), (0, 0), (2**64 - 1, 0), (1, 1)])
    assert cnt.tolist() == [2, 0, 94, 0] and k.tolist() == [98, 97] + list(range(3, 97)) and rep.sl_len() == 0
    # Remove through a partitioned round: the responses are the owners'
    recs = U.cuda(np.array([(5, 50), (5, TOMB), (5, TOMB)], np.uint64))
    resp = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    some = torch.full((3,), 7, dtype=torch.uint8, device="cuda")
    dummy = torch.zeros(8, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    grp.round(recs, 3, None, 0, dummy, dummy.view(torch.uint8), resp, some)
    grp.sync()
    assert resp.cpu().tolist() == [5, 50, 0] and some.cpu().tolist() == [1, 1, 0]
    grp.close()
    rep.close()
