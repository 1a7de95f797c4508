"""Removes in the partitioned rounds of a skip-list group that agreed on removal
(nrg_group_skiplist_enable_removal), over the loopback collectives: responses, the rounds' Gets, the union of
the members' dumps, each member holding only keys it owns and the summed digest all equal
tests/skiplist_group_pop_model.py's UnionModel replaying the records in rank order, then issue order, bit
for bit. Groups are opened as tests/test_gpu_skiplist_scan_group.py opens them (log2_slots 12, max_batch
2048, SL_DELTA_MAX 64), prefilled with 1500 keys by nrg_skiplist_prefill_partition, and one round of at most
64 new keys follows, so both runs hold entries. Guard words surround every output."""
import ctypes as C
import threading

import numpy as np
import pytest

import skiplist_group_gpu as U
import skiplist_group_pop_model as GM
import skiplist_scan_model as SM

pytestmark = pytest.mark.gpu

TOMB, U64_MAX = GM.TOMB, GM.U64_MAX
PREFILL = GM.PREFILL
OFF = U64_MAX - 7  # key 7 is prefilled with the value 2^64 - 1: a stored value equal to the tombstone


def _owned(G, p, lo, hi, n):
    """n keys of [lo, hi) that partition p of G owns"""
    pool = np.arange(lo, hi, dtype=np.uint64)
    k = pool[SM.key_owner(pool, G) == p]
    assert len(k) >= n
    return k[:n]


def _recs(pairs):
    return np.array(pairs, np.uint64).reshape(-1, 2)


def _scenario(G):
    """one round's parts. Ranks a = 0, b = the middle one, c = the last (all 0 in a one-rank group)."""
    a, b, c = 0, G // 2, G - 1
    own_a = _owned(G, a, 100, 1400, 4).tolist()        # prefilled keys rank a owns
    far = _owned(G, c, 100, 1400, 4).tolist()          # prefilled keys another rank owns (G > 1)
    fresh = [5000, 5001, 5002, 5003]                   # absent keys
    recs = [[] for _ in range(G)]
    recs[a] += [(own_a[0], TOMB), (far[0], TOMB), (fresh[0], TOMB),          # present (own, another's), absent
                (fresh[1], 11), (fresh[1], TOMB),                            # Push then Remove
                (own_a[1], TOMB), (own_a[1], 22),                            # Remove then Push
                (far[1], TOMB),                                              # the same Remove from a and c: Some ...
                (own_a[2], TOMB),                                            # a removes, b pushes: present afterwards
                (0, TOMB), (U64_MAX, TOMB), (7, TOMB)]                       # key extremes; a value equal to the tombstone
    recs[b] += [(own_a[2], 33), (fresh[2], 44)]
    recs[c] += [(far[1], TOMB), (far[2], TOMB), (U64_MAX, 55), (fresh[3], TOMB), (0, 66)]   # ... then None
    gets = [np.array(own_a[:3] + far[:3] + fresh + [0, 7, U64_MAX, 1499 - i], np.uint64) for i in range(G)]
    want = [i in (a, c) or i % 2 == 0 for i in range(G)]   # members that pass no resp beside members that do
    return [(_recs(recs[i]) if recs[i] else None, gets[i], want[i]) for i in range(G)]


def _big(G):
    """owner 0 receives 5000 Removes from the last rank, more than a replay chunk: prefilled keys (Some),
    absent keys (None) and repeats on both sides of the chunk edges (Some, then None)"""
    mine = _owned(G, 0, 8, PREFILL, 150)
    absent = _owned(G, 0, 10_000, 60_000, 2100)
    k = np.concatenate([mine[:75], absent[:1965], mine[::-1], absent, mine, absent[:560]])
    assert len(k) == 5000 and np.all(SM.key_owner(k, G) == 0)
    parts = [(None, np.array([int(mine[0]), int(mine[149]), 3], np.uint64), False) for _ in range(G)]
    parts[G - 1] = (np.stack([k, np.full(5000, TOMB, np.uint64)], 1), parts[G - 1][1], True)
    return parts


def _random_rounds(G, n_rounds=4, seed=21):
    rng = np.random.default_rng(seed)
    out = []
    for r in range(n_rounds):
        parts = []
        for i in range(G):
            n = int(rng.integers(0, 120))
            k = rng.integers(0, 2 * PREFILL, n, dtype=np.uint64)
            v = np.where(rng.random(n) < 0.5, np.uint64(TOMB), rng.integers(0, 1 << 40, n, dtype=np.uint64))
            gets = rng.integers(0, 2 * PREFILL, 40, dtype=np.uint64)
            parts.append((np.stack([k, v], 1) if n else None, gets, (i + r) % 3 != 1))
        out.append(parts)
    return out


def _filled(L, lib, G, exp):
    g, ctxs = U.open_group(L, lib, G, exp=exp)
    U.prefill(L, lib, ctxs, PREFILL, OFF)
    model = GM.UnionModel()
    model.prefill(PREFILL, OFF)
    k, v = GM.round_keys(G)
    U.push_round(L, lib, g, G, k, v)
    model.replay(zip(k.tolist(), v.tolist()))
    return g, ctxs, model


@pytest.mark.parametrize("G,exp", U.CASES)
def test_removes_in_partitioned_rounds(nrg, G, exp):
    """The scenario round, the 5000-Remove round and four pipelined rounds, each equal to the model, and the
    pipelined rounds equal to the same rounds run synchronously; the enable call is idempotent for one
    tombstone and refuses another."""
    L = nrg._lib
    lib = L.load()
    g, ctxs, model = _filled(L, lib, G, exp)
    assert model.m[7] == TOMB
    assert lib.nrg_group_skiplist_enable_removal(g, TOMB) == L.NRG_OK
    assert lib.nrg_group_skiplist_enable_removal(g, TOMB) == L.NRG_OK          # again, the same tombstone
    assert lib.nrg_group_skiplist_enable_removal(g, TOMB - 9) == L.NRG_E_INVAL  # no way back, no other value
    for c in ctxs:
        t, on = C.c_uint64(), C.c_int()
        L.check(lib.nrg_skiplist_removal(c, C.byref(t), C.byref(on)))
        assert (t.value, on.value) == (TOMB, 1)
    model.tomb = TOMB
    for name, parts in (("scenario", _scenario(G)), ("5000 removes", _big(G))):
        rc, rd, keep = U.post_round(L, lib, g, parts)
        assert rc == L.NRG_OK, (name, rc)
        L.check(lib.nrg_group_sync(g))
        U.check_round(keep, parts, model, f"G={G} exp={exp} {name}")
        U.check_members(L, lib, ctxs, model, f"G={G} exp={exp} after {name}")
    assert 7 not in model.m and model.m[0] == 66 and model.m[U64_MAX] == 55
    posted = []
    rounds = _random_rounds(G)
    for r, parts in enumerate(rounds):
        rc, rd, keep = U.post_round(L, lib, g, parts, pipelined=True)
        assert rc == L.NRG_OK, (r, rc)
        posted.append((rd, keep))
    L.check(lib.nrg_group_partitioned_flush(g), "flush")
    L.check(lib.nrg_group_sync(g))
    for r, (parts, (_, keep)) in enumerate(zip(rounds, posted)):
        U.check_round(keep, parts, model, f"G={G} exp={exp} pipelined round {r}")
    U.check_members(L, lib, ctxs, model, f"G={G} exp={exp} after the pipelined rounds")
    # the same rounds, synchronously, on a second group in the same state: every output buffer (guards and
    # unasked responses included) and every member's contents equal the pipelined run's
    g2, ctxs2, _ = _filled(L, lib, G, exp)
    L.check(lib.nrg_group_skiplist_enable_removal(g2, TOMB))
    twin = []
    for parts in [_scenario(G), _big(G)] + rounds:
        rc, rd, keep = U.post_round(L, lib, g2, parts)
        assert rc == L.NRG_OK
        L.check(lib.nrg_group_sync(g2))
        twin.append(keep)
    for r, ((_, keep), keep2) in enumerate(zip(posted, twin[2:])):
        for i, (x, y) in enumerate(zip(keep, keep2)):
            for name in ("resp", "some", "gv", "gf"):
                assert np.array_equal(getattr(x, name).host(), getattr(y, name).host()), (r, i, name)
    for p, (c, c2) in enumerate(zip(ctxs, ctxs2)):
        (k, v), (k2, v2) = U.dump(L, lib, c), U.dump(L, lib, c2)
        assert np.array_equal(k, k2) and np.array_equal(v, v2), p
        assert U.digest(L, lib, c) == U.digest(L, lib, c2), p
    L.check(lib.nrg_group_close(g2))
    L.check(lib.nrg_group_close(g))


def test_a_member_enabled_beforehand(nrg):
    """With another tombstone: NRG_E_INVAL, nothing enabled on the others, rounds still refused (that member
    enabled on its own). With the same tombstone: fine."""
    L = nrg._lib
    lib = L.load()
    G = 3
    g, ctxs, model = _filled(L, lib, G, False)
    L.check(lib.nrg_skiplist_enable_removal(ctxs[1], 5))
    assert lib.nrg_group_skiplist_enable_removal(g, TOMB) == L.NRG_E_INVAL
    for i in (0, 2):
        on = C.c_int(7)
        L.check(lib.nrg_skiplist_removal(ctxs[i], None, C.byref(on)))
        assert on.value == 0
    before = U.log_tails(L, lib, ctxs)
    parts = [(_recs([(1, 2), (3, TOMB)]), np.array([1], np.uint64), True) for _ in range(G)]
    rc, rd, keep = U.post_round(L, lib, g, parts)
    assert rc == L.NRG_E_INVAL
    L.check(lib.nrg_group_sync(g))
    assert all(b.all_untouched() for b in keep) and U.log_tails(L, lib, ctxs) == before
    assert lib.nrg_group_skiplist_enable_removal(g, 5) == L.NRG_OK  # the value that member has: every rank agrees
    model.tomb = 5
    parts = [(_recs([(10 + i, 5), (3000 + i, 9)]), np.array([10 + i, 3000 + i], np.uint64), True) for i in range(G)]
    rc, rd, keep = U.post_round(L, lib, g, parts)
    assert rc == L.NRG_OK
    L.check(lib.nrg_group_sync(g))
    U.check_round(keep, parts, model, "after agreeing on the member's tombstone")
    U.check_members(L, lib, ctxs, model, "after agreeing on the member's tombstone")
    L.check(lib.nrg_group_close(g))


def test_a_hashmap_group_is_refused(nrg):
    L = nrg._lib
    lib = L.load()
    G = 3
    g, ctxs = U.open_group(L, lib, G, U.cfg(L, L.NRG_DS_HASHMAP))
    assert lib.nrg_group_skiplist_enable_removal(g, TOMB) == L.NRG_E_INVAL
    assert lib.nrg_group_skiplist_enable_pops(g, GM.FRONT, GM.BACK) == L.NRG_E_INVAL
    for c in ctxs:
        assert lib.nrg_skiplist_removal(c, None, None) == L.NRG_E_INVAL
    # the group is as it was: a hashmap round where {k, 2^64 - 1} is a Put
    parts = [(_recs([(i + 1, TOMB), (i + 1, 4)]), np.array([i + 1], np.uint64), True) for i in range(G)]
    rc, rd, keep = U.post_round(L, lib, g, parts)
    assert rc == L.NRG_OK
    L.check(lib.nrg_group_sync(g))
    for i, b in enumerate(keep):
        assert b.some.inner().tolist() == [0, 1] and b.resp.inner().tolist() == [0, TOMB]  # previous values
        assert b.gv.inner().tolist() == [4] and b.gf.inner().tolist() == [1]
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


def test_ranks_that_pass_different_tombstones(nrg):
    """One thread per rank, G = 2: different tombstones give NRG_E_INVAL on both ranks and nothing is enabled
    (a {k, 2^64 - 1} record is still a Push); the same tombstone then enables both, twice; a Remove sent by
    rank 0 to a key rank 1 owns answers the previous value. Through PartitionedGroup."""
    import torch

    from nrgpu import DeviceReplica
    from nrgpu.parallel import PartitionedGroup

    L = nrg._lib
    G = 2
    theirs = int(_owned(G, 1, 100, 200, 1)[0])

    def round_of(grp, rank, recs):
        dummy = torch.zeros(8, dtype=torch.int64, device="cuda")
        n = len(recs) if rank == 0 else 0
        p = U.cuda(_recs(recs)) if n else None
        resp = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")
        some = torch.full((max(n, 1),), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        grp.round(p, n, None, 0, dummy, dummy.view(torch.uint8), resp if n else None, some if n else None)
        grp.sync()
        return resp.cpu().numpy().view(np.uint64)[:n].tolist(), some.cpu().numpy()[:n].tolist()

    def body(rank, uid):
        rep = DeviceReplica(L.NRG_DS_SKIPLIST, 0, knobs={"SL_DELTA_MAX": U.DELTA_MAX}, log2_slots=U.LOG2_SLOTS,
                            max_batch=U.MAX_BATCH, max_reads=U.MAX_READS, replica_id=rank + 1, log_bytes=U.LOG_BYTES)
        rep.sl_prefill_partition(300, 1, rank, G)
        grp = PartitionedGroup(rep, rank, G, uid=uid)
        res = {}
        try:
            grp.enable_removal(TOMB - rank)
            res["differ"] = L.NRG_OK
        except L.NrgError as e:
            res["differ"] = e.code
        res["enabled_after_refusal"] = rep.sl_removal()
        res["push"] = round_of(grp, rank, [(theirs, TOMB)])      # a Push of the value 2^64 - 1
        grp.enable_removal()
        grp.enable_removal()
        res["enabled"] = rep.sl_removal()
        res["remove"] = round_of(grp, rank, [(theirs, TOMB), (theirs, TOMB), (theirs, 8)])
        res["len"] = rep.sl_len()
        grp.close()
        rep.close()
        return res

    out = _run_ranks(nrg, G, body)
    for rank, res in enumerate(out):
        assert res["differ"] == L.NRG_E_INVAL and res["enabled_after_refusal"] is None and res["enabled"] == TOMB
    assert out[0]["push"] == ([theirs], [1])
    assert out[0]["remove"] == ([TOMB, 0, theirs], [1, 0, 1])
    assert out[0]["len"] + out[1]["len"] == 300
