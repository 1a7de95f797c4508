"""Table growth of the NrHashMap replica (config.hashmap_max_log2_slots, nrg_hashmap_reserve,
nrg_hashmap_capacity): the reference's HashMap<u64, u64> never runs out of room
(nr/examples/hashmap.rs starts from an empty map, benches/hashmap.rs:91-100 only pre-sizes it).

The model is a Python dict (plus the oracle's HashMap for digests). Tables are tiny: growth
starts from the 16 slots that nrg_open accepts at least, so every test crosses several rehashes.
A table that growth manages holds at most one key per two slots (common.hpp
HM_GROW_SLOTS_PER_KEY), which the size assertions below follow."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U64_MAX = 2**64 - 1
M64 = U64_MAX


def mix64(z):
    """common.hpp mix64 (splitmix64's finaliser); the home slot is its top log2_slots bits"""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def home(key, log2_slots):
    return mix64(key) >> (64 - log2_slots)


def log2_for(keys):
    """smallest table (>= 16 slots) with 2 * keys <= slots"""
    l = 4
    while (1 << l) < 2 * keys:
        l += 1
    return l


def _puts(nrg, keys, vals):
    r = np.zeros(len(keys), nrg.PUT_DTYPE)
    r["key"], r["val"] = keys, vals
    return r


def _distinct(rng, n):
    k = np.unique(rng.integers(0, 2**64 - 2, 2 * n, dtype=np.uint64))
    assert len(k) >= n
    return rng.permutation(k)[:n]


def _open(nrg, **kw):
    return nrg.DeviceReplica(nrg._lib.NRG_DS_HASHMAP, 0, **kw)


def _check_contents(dev, orc, model, absent):
    """Gets of every key and of absent ones, size, sorted dump and digest against the dict"""
    keys = np.array(sorted(model), np.uint64)
    vals = np.array([model[int(k)] for k in keys], np.uint64)
    v, f = dev.hm_get(keys)
    assert np.all(f == 1)
    np.testing.assert_array_equal(v, vals)
    if len(absent):
        v, f = dev.hm_get(absent)
        assert not np.any(f) and not np.any(v)
    assert dev.hm_size() == len(model)
    dk, dv = dev.hm_dump()
    np.testing.assert_array_equal(dk, keys)
    np.testing.assert_array_equal(dv, vals)
    om = orc.HashMap()
    om.replay(keys, vals, want_prev=False)
    assert dev.hm_digest() == om.digest()


ROUND_KINDS = {
    "stamp": {"PART": 0},      # stamp rounds wherever they can run (no previous values)
    "part": {"PART": 2},       # partition rounds everywhere
    "small": {"SMALL_MAX": 2048},  # one-launch small rounds (chunks of 64 Puts)
    "nostamp": {"STAMP_MAX": 0},   # no stamp rounds at all
}


@pytest.mark.parametrize("window", [True, False])
@pytest.mark.parametrize("kind", sorted(ROUND_KINDS))
def test_growth_through_every_round_kind(nrg, orc, kind, window):
    """3000 distinct keys through one exec in chunks of 64: the table grows between chunks, from
    16 slots to the smallest table with 2 * keys <= slots. Previous values (the response window)
    take the partition path whatever the knobs say. A second exec overwrites every key: previous
    values come from the moved slots and the table stays as it is."""
    dev = _open(nrg, log2_slots=4, max_batch=64, hashmap_max_log2_slots=14, knobs=ROUND_KINDS[kind])
    rng = np.random.default_rng(11)
    keys = _distinct(rng, 3000)
    vals = rng.integers(0, 2**64 - 1, 3000, dtype=np.uint64)
    first = dev.log_append(_puts(nrg, keys, vals), 1)
    if window:
        prev, some = dev.log_exec(first, first + 3000)
        assert not np.any(some) and not np.any(prev)  # the dict held none of them
    else:
        dev.log_exec()
    model = {int(k): int(v) for k, v in zip(keys, vals)}
    absent = np.setdiff1d(_distinct(rng, 600), keys)[:500]
    _check_contents(dev, orc, model, absent)
    assert dev.hm_log2_slots() == log2_for(3000) == 13
    vals2 = rng.integers(0, 2**64 - 1, 3000, dtype=np.uint64)
    order = rng.permutation(3000)
    first = dev.log_append(_puts(nrg, keys[order], vals2[order]), 1)
    if window:
        prev, some = dev.log_exec(first, first + 3000)
        assert np.all(some == 1)
        np.testing.assert_array_equal(prev, vals[order])
    else:
        dev.log_exec()
    model = {int(k): int(v) for k, v in zip(keys, vals2)}
    _check_contents(dev, orc, model, absent)
    assert dev.hm_log2_slots() == 13  # overwrites do not grow
    dev.close()


def test_reserve_rehashes_across_workgroups_by_a_factor_of_four(nrg, orc):
    """2000 keys in 4096 slots (load 0.49: probe chains cross any contiguous run of slots), then
    one rehash 2^12 -> 2^14."""
    L = nrg._lib
    dev = _open(nrg, log2_slots=12, max_batch=4096)  # growth off: reserve works all the same
    rng = np.random.default_rng(12)
    keys = _distinct(rng, 2000)
    vals = rng.integers(0, 2**64 - 1, 2000, dtype=np.uint64)
    dev.log_append(_puts(nrg, keys, vals), 1)
    dev.log_exec()
    assert dev.hm_log2_slots() == 12
    dev.hm_reserve(8000)
    assert dev.hm_log2_slots() == 14
    model = {int(k): int(v) for k, v in zip(keys, vals)}
    absent = np.setdiff1d(_distinct(rng, 600), keys)[:500]
    _check_contents(dev, orc, model, absent)
    dev.hm_reserve(1)  # never shrinks: nothing happens
    assert dev.hm_log2_slots() == 14
    with pytest.raises(nrg.NrgError) as e:
        dev.hm_reserve(2**40)
    assert e.value.code == L.NRG_E_INVAL
    assert dev.hm_log2_slots() == 14
    # the replica replays on in the new table
    dev.log_append(_puts(nrg, keys[:100], vals[:100] ^ np.uint64(5)), 1)
    dev.log_exec()
    model.update({int(k): int(v) ^ 5 for k, v in zip(keys[:100], vals[:100])})
    _check_contents(dev, orc, model, absent)
    dev.close()


def _keys_with_home(log2_slots, homes, n, start):
    out, k = [], start
    while len(out) < n:
        if home(k, log2_slots) in homes:
            out.append(k)
        k += 1
    return out


def test_chains_that_wrap_survive_two_grows(nrg, orc):
    """12 keys whose home is one of the last two slots of the 16-slot table and 12 whose home is
    one of the last two of the 64-slot table: their chains wrap to slot 0 in the table a rehash
    reads (16, then 64 slots) and in the tables it fills (the second set in 64 and 128 slots:
    its 12 keys share the last two, then the last four slots). 16 -> 64 -> 128, by themselves."""
    a = _keys_with_home(4, (14, 15), 12, 1000)
    b = _keys_with_home(6, (62, 63), 12, 5000)
    assert not set(a) & set(b)
    assert all(home(k, 7) >= 124 for k in b)
    dev = _open(nrg, log2_slots=4, max_batch=64, hashmap_max_log2_slots=7)
    model = {}

    def put(keys):
        keys = np.array(keys, np.uint64)
        vals = keys * np.uint64(3) + np.uint64(1)
        dev.log_append(_puts(nrg, keys, vals), 1)
        dev.log_exec()
        model.update({int(k): int(v) for k, v in zip(keys, vals)})

    put(a[:8])  # 8 keys = the limit of 16 slots: slots 14, 15, 0, 1, ... hold them
    assert dev.hm_log2_slots() == 4
    put(a[8:] + b)  # 24 keys in all: 16 -> 64 slots
    assert dev.hm_log2_slots() == 6
    _check_contents(dev, orc, model, np.arange(100, 200, dtype=np.uint64))
    put(list(range(20000, 20009)))  # 33 keys: 64 -> 128 slots
    assert dev.hm_log2_slots() == 7
    _check_contents(dev, orc, model, np.arange(100, 200, dtype=np.uint64))
    dev.close()


def test_side_key_and_its_neighbours_survive_two_grows(nrg, orc):
    """u64::MAX lives in the side slot (it is the table's empty marker) and does not move; key 0
    and u64::MAX - 1 are ordinary keys. All three keep their latest values over two grows and
    the side key counts once."""
    special = [U64_MAX, 0, U64_MAX - 1]
    dev = _open(nrg, log2_slots=4, max_batch=64, hashmap_max_log2_slots=10)
    model = {}
    rng = np.random.default_rng(14)
    fill = _distinct(rng, 60)
    fill = fill[~np.isin(fill, np.array(special, np.uint64))]
    step, sizes = 0, [dev.hm_log2_slots()]
    for lo, hi in ((0, 5), (5, 25), (25, 60)):  # 8 distinct keys, then 28, then 63: a grow each time
        step += 1
        keys = np.concatenate([np.array(special, np.uint64), fill[lo:hi], np.array(special, np.uint64)])
        vals = np.arange(len(keys), dtype=np.uint64) + np.uint64(1000 * step)
        first = dev.log_append(_puts(nrg, keys, vals), 1)
        prev, some = dev.log_exec(first, first + len(keys))
        for i, (k, v) in enumerate(zip(keys, vals)):
            want = model.get(int(k))
            assert bool(some[i]) == (want is not None), (step, i)
            if want is not None:
                assert int(prev[i]) == want, (step, i)
            model[int(k)] = int(v)
        assert dev.hm_size() == len(model)
        sizes.append(dev.hm_log2_slots())
    # (a round's Puts count before they are deduplicated, so the sizes follow the Puts, not the keys)
    assert sizes == sorted(sizes) and len(set(sizes)) >= 3 and (1 << sizes[-1]) >= 2 * len(model), sizes
    _check_contents(dev, orc, model, np.arange(1, 100, dtype=np.uint64))
    # once more without a response window: a stamp round, whose reads go by the restarted epochs
    keys = np.array(special, np.uint64)
    dev.log_append(_puts(nrg, keys, np.array([7, 8, 9], np.uint64)), 1)
    dev.log_exec()
    model.update(zip(special, (7, 8, 9)))
    assert dev.hm_size() == len(model)
    v, f = dev.hm_get(np.array(special, np.uint64))
    assert np.all(f == 1) and [int(x) for x in v] == [model[k] for k in special]
    dev.close()


@pytest.mark.parametrize("epoch_limit", [0, 5])
def test_pipelined_rounds_grow_after_the_deferred_half(nrg, epoch_limit):
    """pipeline = 1: a round's apply and reads ride in the next round's launch. 40 rounds of 48
    Puts and 64 Gets (half present, half absent), each with its own response buffers: a grow
    flushes the deferred half against the old table first, so every round's answers equal the
    dict's state after that round. With NRG_KNOB_EPOCH_LIMIT = 5 the stamps are renormalised
    every few rounds, between the grows."""
    import torch

    knobs = {"EPOCH_LIMIT": epoch_limit} if epoch_limit else None
    dev = _open(nrg, log2_slots=4, max_batch=64, max_reads=64, pipeline=1, hashmap_max_log2_slots=14, knobs=knobs)
    rng = np.random.default_rng(15)
    keys = _distinct(rng, 40 * 48 + 40 * 32)
    put_keys, absent = keys[: 40 * 48].reshape(40, 48), keys[40 * 48:].reshape(40, 32)
    model, rounds = {}, []
    for r in range(40):
        vals = rng.integers(0, 2**63, 48, dtype=np.uint64)
        pk = put_keys[r].copy()
        if r:
            pk[:8] = put_keys[r - 1][:8]  # overwrites of the round whose half is still deferred
        for k, v in zip(pk, vals):
            model[int(k)] = int(v)
        present = rng.choice(np.array(sorted(model), np.uint64), 32)
        gk = np.concatenate([present, absent[r]])
        want_v = np.array([model.get(int(k), 0) for k in gk], np.uint64)
        want_f = np.array([int(k) in model for k in gk], np.uint8)
        d_puts = torch.from_numpy(np.stack([pk, vals], 1).view(np.int64).copy()).cuda()
        d_gk = torch.from_numpy(gk.view(np.int64).copy()).cuda()
        d_gv = torch.full((64,), -1, dtype=torch.int64, device="cuda")
        d_gf = torch.full((64,), 7, dtype=torch.uint8, device="cuda")
        dev.hm_round_device(d_puts, 48, 1, d_gk, 64, d_gv, d_gf)
        rounds.append((d_puts, d_gk, d_gv, d_gf, want_v, want_f))
    dev.join()
    torch.cuda.synchronize()
    for r, (_, _, d_gv, d_gf, want_v, want_f) in enumerate(rounds):
        np.testing.assert_array_equal(d_gf.cpu().numpy(), want_f, err_msg=f"round {r} found")
        np.testing.assert_array_equal(d_gv.cpu().numpy().view(np.uint64), want_v, err_msg=f"round {r} vals")
    dev.sync()
    assert dev.hm_size() == len(model)
    assert dev.hm_log2_slots() == log2_for(len(model))
    dev.close()


def test_overwrites_do_not_grow(nrg):
    """The same 8 keys in 100 rounds: the upper bound of the key count passes the limit, the
    exact count does not, and the table stays. The 33rd distinct key doubles it."""
    dev = _open(nrg, log2_slots=6, max_batch=64, hashmap_max_log2_slots=12)
    keys = np.arange(500, 508, dtype=np.uint64)
    for r in range(100):
        dev.log_append(_puts(nrg, keys, keys + np.uint64(r)), 1)
        dev.log_exec()
    assert dev.hm_log2_slots() == 6 and dev.hm_size() == 8
    more = np.arange(600, 624, dtype=np.uint64)
    dev.log_append(_puts(nrg, more, more), 1)
    dev.log_exec()
    assert dev.hm_log2_slots() == 6 and dev.hm_size() == 32  # 32 keys in 64 slots: the limit itself
    one = np.array([700], np.uint64)
    dev.log_append(_puts(nrg, one, one), 1)
    dev.log_exec()
    assert dev.hm_size() == 33 and dev.hm_log2_slots() == 7
    v, f = dev.hm_get(np.concatenate([keys, more, one]))
    assert np.all(f == 1)
    np.testing.assert_array_equal(v, np.concatenate([keys + np.uint64(99), more, one]))
    dev.close()


def test_growth_stops_at_the_configured_maximum(nrg):
    """100 distinct keys, at most 64 slots: the table grows to the maximum and then fills like a
    fixed one: NRG_E_TABLE_FULL from the exec, once, and the replica stays usable."""
    L = nrg._lib
    dev = _open(nrg, log2_slots=4, max_batch=64, hashmap_max_log2_slots=6)
    keys = np.arange(100, 200, dtype=np.uint64)
    dev.log_append(_puts(nrg, keys, keys), 1)
    with pytest.raises(nrg.NrgError) as e:
        dev.log_exec()
    assert e.value.code == L.NRG_E_TABLE_FULL
    assert dev.hm_log2_slots() == 6
    v, f = dev.hm_get(keys)
    assert int(f.sum()) == 64 == dev.hm_size()  # every slot holds a key, each with its own value
    np.testing.assert_array_equal(v[f == 1], keys[f == 1])
    held = keys[f == 1][:10]
    dev.log_append(_puts(nrg, held, held + np.uint64(1)), 1)  # overwrites of keys it holds still work
    dev.log_exec()
    v, f = dev.hm_get(held)
    assert np.all(f == 1)
    np.testing.assert_array_equal(v, held + np.uint64(1))
    dev.close()


def test_a_fixed_table_still_fills(nrg):
    """hashmap_max_log2_slots left 0: 20 keys in 16 slots end as
    test_gpu_edge.py::test_table_full_is_an_error has it, and the table is never resized."""
    L = nrg._lib
    dev = _open(nrg, log2_slots=4, max_batch=64)
    keys = np.arange(100, 120, dtype=np.uint64)
    dev.log_append(_puts(nrg, keys, keys), 1)
    with pytest.raises(nrg.NrgError) as e:
        dev.log_exec()
    assert e.value.code == L.NRG_E_TABLE_FULL
    assert dev.hm_log2_slots() == 4
    v, f = dev.hm_get(keys)
    assert int(f.sum()) == 16 == dev.hm_size()  # every slot holds a key, each with its own value
    np.testing.assert_array_equal(v[f == 1], keys[f == 1])
    dev.close()


def test_prefill_grows_first(nrg):
    """NrHashMap::default's 5000 keys into a table that starts at 16 slots."""
    dev = _open(nrg, log2_slots=4, max_batch=64, hashmap_max_log2_slots=20)
    dev.hm_prefill_range(5000, 1)
    assert dev.hm_log2_slots() == log2_for(5000) == 14
    keys = np.arange(5000, dtype=np.uint64)
    v, f = dev.hm_get(keys)
    assert np.all(f == 1)
    np.testing.assert_array_equal(v, keys + np.uint64(1))
    v, f = dev.hm_get(np.arange(5000, 5500, dtype=np.uint64))
    assert not np.any(f)
    assert dev.hm_size() == 5000
    # host-pointer prefill (replayed in chunks) grows as well
    more = np.arange(10000, 16000, dtype=np.uint64)
    dev.hm_prefill(more, more + np.uint64(7))
    assert dev.hm_size() == 11000 and dev.hm_log2_slots() == log2_for(11000)
    v, f = dev.hm_get(more)
    assert np.all(f == 1)
    np.testing.assert_array_equal(v, more + np.uint64(7))
    dev.close()


@pytest.mark.parametrize("serve", [1, 0])
def test_combiner_grows_under_the_round_server(nrg, serve):
    """4 client threads, 100 calls of 32 Puts of distinct keys each, from 256 slots. serve = 1
    (the default): small rounds go to the resident round server, which holds the table's address
    and mask as kernel arguments; a round that needs a count or a grow stops it first."""
    T, CALLS = 4, 100
    dev = _open(nrg, log2_slots=8, max_batch=4096, max_reads=4096, hashmap_max_log2_slots=18,
                log_bytes=64 * (1 << 16))
    dev.set_knob("COMB_SERVE", serve)
    comb = nrg.Combiner(dev, T)
    errors = []

    def client(t):
        try:
            tok = comb.register()
            base = (tok + 1) << 40
            for it in range(CALLS):
                keys = np.arange(base + 32 * it, base + 32 * it + 32, dtype=np.uint64)
                prev, some = comb.put(tok, keys, keys ^ np.uint64(0xABCD))
                assert not np.any(some), (tok, it)
            for it in range(CALLS):  # this thread's keys, then (below) everyone's
                keys = np.arange(base + 32 * it, base + 32 * it + 32, dtype=np.uint64)
                got, found = comb.get(tok, keys)
                assert np.all(found == 1), (tok, it)
                np.testing.assert_array_equal(got, keys ^ np.uint64(0xABCD))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=client, args=(i,)) for i in range(T)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors[0]
    tok = 0  # every thread is done: its token is free again
    allk = np.concatenate([np.arange(((t + 1) << 40), ((t + 1) << 40) + 32 * CALLS, dtype=np.uint64) for t in range(T)])
    for i in range(0, len(allk), 32):
        got, found = comb.get(tok, allk[i:i + 32])
        assert np.all(found == 1), i
        np.testing.assert_array_equal(got, allk[i:i + 32] ^ np.uint64(0xABCD))
    comb.close()
    assert dev.hm_size() == T * CALLS * 32 == 12800
    assert dev.hm_log2_slots() >= 15
    v, f = dev.hm_get(allk)
    assert np.all(f == 1)
    np.testing.assert_array_equal(v, allk ^ np.uint64(0xABCD))
    dev.close()


def test_group_members_grow_at_the_same_round(nrg, orc):
    """Two members over the loopback collectives, growth enabled: 20 rounds of 100 distinct Puts
    per member. Both replicas replay the same log, report the same table size after every round
    and end with the model's contents."""
    import torch

    L = nrg._lib
    lib = L.load()
    cfg = L.default_config(L.NRG_DS_HASHMAP)
    cfg.log2_slots, cfg.max_batch, cfg.hashmap_max_log2_slots = 4, 1 << 12, 16
    cfg.log_bytes = 64 * (1 << 16)
    G = 2
    L.check(lib.nrg_test_loopback_collectives(1))
    g = C.c_void_p()
    try:
        L.check(lib.nrg_group_open((C.c_int * G)(0, 0), G, C.byref(cfg), C.byref(g)), "nrg_group_open")
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))
    ctxs = [lib.nrg_group_replica(g, i) for i in range(G)]

    def log2_slots(ctx):
        n = C.c_uint32()
        L.check(lib.nrg_hashmap_capacity(ctx, C.byref(n)))
        return n.value

    rng = np.random.default_rng(20)
    keys = _distinct(rng, 20 * G * 100).reshape(20, G, 100)
    om = orc.HashMap()
    sizes, keep = [], []
    for r in range(20):
        rd = (L.Round * G)()
        for i in range(G):
            v = keys[r, i] ^ np.uint64(r + 1)
            p = torch.from_numpy(np.stack([keys[r, i], v], 1).view(np.int64).copy()).cuda()
            keep.append(p)
            rd[i].recs, rd[i].n = p.data_ptr(), 100
            om.replay(keys[r, i], v, want_prev=False)
        torch.cuda.synchronize()
        L.check(lib.nrg_group_round_async(g, rd, None), f"group round {r}")
        L.check(lib.nrg_group_sync(g))
        a, b = log2_slots(ctxs[0]), log2_slots(ctxs[1])
        assert a == b, r
        sizes.append(a)
    assert sizes[-1] == log2_for(20 * G * 100) == 13 and sizes[0] < sizes[-1]
    digests = []
    for c in ctxs:
        out = np.zeros(3, np.uint64)
        L.check(lib.nrg_hashmap_digest(c, out.ctypes.data_as(C.c_void_p)))
        digests.append(tuple(int(x) for x in out))
    assert digests[0] == digests[1] == om.digest()
    L.check(lib.nrg_group_close(g))


def test_wrong_kind_is_invalid(nrg):
    L = nrg._lib
    lib = L.load()
    dev = nrg.DeviceReplica(L.NRG_DS_STACK, 0, max_batch=64, stack_capacity=1024)
    n = C.c_uint32(9)
    assert lib.nrg_hashmap_reserve(dev.handle, 100) == L.NRG_E_INVAL
    assert lib.nrg_hashmap_capacity(dev.handle, C.byref(n)) == L.NRG_E_INVAL and n.value == 9
    with pytest.raises(TypeError):
        dev.hm_reserve(100)
    with pytest.raises(TypeError):
        dev.hm_log2_slots()
    dev.close()
