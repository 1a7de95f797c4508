"""A sequential model of the hashmap with removal (nrg_hashmap_enable_removal, csrc/hashmap.hip), and
named record streams aimed at the arms of the apply kernel's removal path.

The oracle has no Remove (the reference's OpWr has none), so this is the reference: a dict, as
std::collections::HashMap::remove defines the answers -- the previous value or None, and the key is absent
afterwards. Beside the dict the model tracks which keys HOLD A SLOT: a removed key keeps its slot (dead)
until a rehash drops it, a Remove never claims one, a Put of a key without one claims one. That predicts
the occupancy, and with hm_room's policy restated below, when a growing table purges or grows.
Placement (which slot) follows tests/hashmap_streams.py place(): it is exact for keys claimed one per
round, which is how the chain streams are built; the device is never asked for a slot number.

tests/test_hashmap_remove_cpu.py checks the model against a plain dict and shows that every stream
reaches the arm it is named for; tests/test_gpu_hashmap_remove.py replays the streams. numpy alone.
"""
import numpy as np

import hashmap_streams as S

U64 = np.uint64
TOMB = 2**64 - 1
OTHER_TOMB = 0x7070707070707070
PUT_DTYPE = np.dtype([("key", "<u8"), ("val", "<u8")])
GROW_SLOTS_PER_KEY = 2  # HM_GROW_SLOTS_PER_KEY


def recs_of(keys, vals):
    r = np.zeros(len(keys), PUT_DTYPE)
    r["key"], r["val"] = np.asarray(keys, U64), np.asarray(vals, U64)
    return r


def slots_for(keys):
    """hm_slots_for: log2 of the smallest table that holds `keys` keys at the load limit."""
    l = 4
    while l < 63 and (1 << l) // GROW_SLOTS_PER_KEY < keys:
        l += 1
    return l


class HashMapRemoveModel:
    def __init__(self, log2_slots, tomb=TOMB, max_log2=0, max_batch=4096):
        self.log2, self.tomb, self.max_log2, self.max_batch = log2_slots, tomb, max_log2, max_batch
        self.map = {}      # live key -> value
        self.held = {}     # key -> slot, live or dead (the side key: -1)
        self.table = {}    # slot -> key
        self.keys_ub = 0
        self.grows = self.purges = self.full = 0
        self.arms = dict(claim=0, revive=0, die=0, remove_dead=0, remove_absent=0, overwrite=0)

    def __len__(self):
        return len(self.map)

    @property
    def occupancy(self):
        return len(self.held)

    # ---- hm_room / hm_grow on an enabled context ------------------------------------------------------
    def _rehash(self, log2):
        if log2 > self.log2:
            self.grows += 1
        else:
            self.purges += 1
        self.log2 = log2
        live = sorted((s, k) for k, s in self.held.items() if k in self.map)
        self.table, self.held = {}, {}
        for _, k in live:
            self._claim(k)

    def purge(self):
        """nrg_hashmap_purge"""
        if self.occupancy > len(self.map):
            self._rehash(self.log2)
            self.keys_ub = min(self.keys_ub, len(self.map))

    def room(self, n):
        if not n or self.max_log2 <= self.log2:
            return
        limit = (1 << self.log2) // GROW_SLOTS_PER_KEY
        if self.keys_ub + n <= limit:
            self.keys_ub += n
            return
        live, occ = len(self.map), self.occupancy
        if occ + n > limit:
            want = max(min(slots_for(live + n), self.max_log2), self.log2)
            if want > self.log2 or occ > live:
                self._rehash(want)
                occ = live
        self.keys_ub = occ + n

    # ---- one op at a time ------------------------------------------------------------------------------
    def _claim(self, k):
        if k == S.SIDE:
            self.held[k] = -1
            return True
        s = int(S.place(np.array([k], U64), self.log2, self.table)[0])
        if s < 0:
            return False
        self.held[k] = s
        return True

    def put(self, k, v):
        prev = self.map.get(k)
        if k not in self.held:
            if not self._claim(k):
                self.full += 1
                return None
            self.arms["claim"] += 1
        elif prev is None:
            self.arms["revive"] += 1
        else:
            self.arms["overwrite"] += 1
        self.map[k] = v
        return prev

    def remove(self, k):
        prev = self.map.pop(k, None)
        self.arms["die" if prev is not None else "remove_dead" if k in self.held else "remove_absent"] += 1
        return prev

    def replay(self, recs):
        """The records in log order, in replay chunks of max_batch (each asks hm_room first);
        (prev u64[n], found u8[n])."""
        n = len(recs)
        prev, found = np.zeros(n, U64), np.zeros(n, np.uint8)
        ks, vs = recs["key"].tolist(), recs["val"].tolist()
        for lo in range(0, n, self.max_batch):
            hi = min(n, lo + self.max_batch)
            self.room(hi - lo)
            for i in range(lo, hi):
                p = self.remove(ks[i]) if vs[i] == self.tomb else self.put(ks[i], vs[i])
                if p is not None:
                    prev[i], found[i] = p, 1
        return prev, found

    def get_batch(self, keys):
        ks = np.asarray(keys, U64).tolist()
        return (np.array([self.map.get(k, 0) for k in ks], U64), np.array([int(k in self.map) for k in ks], np.uint8))

    def arrays(self):
        ks = np.array(sorted(self.map), U64)
        return ks, np.array([self.map[k] for k in ks.tolist()], U64)

    def digest(self):
        k, v = self.arrays()
        if not len(k):
            return (0, 0, 0)
        h = S.mix64(k ^ S.mix64(v))
        with np.errstate(over="ignore"):
            return (len(k), int(np.add.reduce(h, dtype=U64)), int(np.bitwise_xor.reduce(h)))


# ---- streams -----------------------------------------------------------------------------------------
class Stream:
    """rounds: (records, Get keys) in order; the records of one round are one replay chunk unless the
    context's max_batch is smaller."""

    def __init__(self, name, log2_slots, tomb=TOMB, max_log2=0, max_batch=4096):
        self.name, self.log2_slots, self.tomb, self.max_log2, self.max_batch = name, log2_slots, tomb, max_log2, max_batch
        self.rounds = []
        self.claims = {}
        self._ctr = 0
        self._seed = int(S.mix64(np.frombuffer(name.encode().ljust(8, b"\0")[:8], U64)[0])) >> 20 << 20

    def vals(self, n):
        """n distinct values, none a tombstone"""
        v = S.mix64(np.arange(self._ctr, self._ctr + n, dtype=U64) + U64(self._seed))
        self._ctr += n
        assert not np.isin(v, [TOMB, OTHER_TOMB]).any()
        return v

    def add(self, keys, remove, gets=None):
        """keys[i] is removed where remove[i], else put with a fresh value"""
        keys = np.ascontiguousarray(keys, U64)
        remove = np.broadcast_to(np.asarray(remove, bool), keys.shape)
        r = recs_of(keys, np.where(remove, U64(self.tomb), self.vals(len(keys))))
        if gets is None:
            u = np.unique(keys)
            with np.errstate(over="ignore"):
                gets = np.concatenate([u, u + U64(1), np.array([S.SIDE], U64)])
        self.rounds.append((r, np.ascontiguousarray(gets, U64)))
        return len(self.rounds) - 1

    def model(self, max_batch=None):
        return HashMapRemoveModel(self.log2_slots, self.tomb, self.max_log2, max_batch or self.max_batch)


def present_absent_dead():
    """Removes of keys put in an earlier round, of keys the same round created, of absent keys, of keys
    already dead, and twice in one chunk (Some, then None)."""
    st = Stream("present_absent_dead", 10)
    a = S.free_keys(120)
    st.add(a, False)                                              # present
    b = S.free_keys(40, 120)
    keys = np.concatenate([a[:30], b, b[:20], S.absent_keys(25), a[:10], a[30:40], a[30:40]])
    rm = np.concatenate([np.ones(30, bool), np.zeros(40, bool), np.ones(20 + 25 + 10 + 10 + 10, bool)])
    st.add(keys, rm)                                              # live, created here, absent, dead in-chunk, twice
    st.add(np.concatenate([a[:30], b[:20], S.absent_keys(25)]), True)  # all dead or absent by now
    st.claims.update(a=a, b=b)
    return st


def never_claims():
    """100 live keys in a fixed 256-slot table, then 5000 Removes of distinct absent keys: occupancy
    stays 100 (a claim per Remove would fill the table after 156 of them)."""
    st = Stream("never_claims", 8, max_batch=2048)
    live = S.free_keys(100)
    st.add(live, False)
    gone = S.absent_keys(5000)
    for lo in range(0, 5000, 2000):
        st.add(gone[lo:lo + 2000], True, np.concatenate([live, gone[lo:lo + 50]]))
    st.claims.update(live=live, gone=gone)
    return st


def in_chunk_order():
    """Put-then-Remove of new keys (a slot each, no key), Remove-then-Put of present keys (the Put
    answers None), and 600 alternating records of one key."""
    st = Stream("in_chunk_order", 10)
    base = S.free_keys(50)
    st.add(base, False)
    new = S.free_keys(20, 50)
    st.add(np.concatenate([new, new]), np.concatenate([np.zeros(20, bool), np.ones(20, bool)]))
    st.add(np.concatenate([base[:20], base[:20]]), np.concatenate([np.ones(20, bool), np.zeros(20, bool)]))
    one = S.free_keys(1, 70)
    st.add(np.repeat(one, 600), np.arange(600) % 2 == 1)
    st.add(np.repeat(one, 600), np.arange(600) % 2 == 0)
    st.claims.update(base=base, new=new, one=one)
    return st


EDGE_AT = (62, 63, 64, 65, 510, 511, 512, 513, 1022, 1023, 1024, 1025, 1599)
EDGE_REMOVE = (63, 64, 511, 512, 1023, 1024, 1599)  # the other edge positions are Puts of the same key


def one_bucket_edges():
    """One apply bucket taken in four chunks of 512 (the layout of hashmap_streams.prev_one_bucket): every
    record of the 1600 is of bucket 0, so a record's position in the bucket is its index. One key has
    Puts at 62, 65, 510, 513, 1022, 1025 and Removes at 63, 64, 511, 512, 1023, 1024, 1599: a Remove on
    either side of a walk step (63 | 64) and of a chunk (511 | 512, 1023 | 1024), and as the last record."""
    st = Stream("one_bucket_edges", 12)
    _, _, nb_log, bk_shift, C = S.round_geometry(S.PREV_N, 12, True)
    ks = S.keys_with_home(lambda h: (h >> bk_shift) == 0, 104, 12)
    edge, fill = ks[0], ks[8:]
    st.add(np.concatenate([[edge], fill[::3]]), False)
    rng = np.random.default_rng(1601)
    keys = fill[rng.integers(0, len(fill), S.PREV_N)]
    rm = rng.random(S.PREV_N) < 0.3
    keys[list(EDGE_AT)] = edge
    rm[list(EDGE_AT)] = False
    rm[list(EDGE_REMOVE)] = True
    st.add(keys, rm)
    st.add(keys[::-1], rm[::-1])
    st.claims.update(edge=edge, bk_shift=bk_shift, C=C)
    return st


def revival():
    """Remove in one chunk, Put in a later one: None, the slot reused, the new value read."""
    st = Stream("revival", 10)
    a = S.free_keys(200)
    st.add(a, False)
    st.add(a[:120], True)
    st.add(a[:60], False)                      # revived
    st.add(np.concatenate([a[60:120], a[:30]]), np.concatenate([np.zeros(60, bool), np.ones(30, bool)]))
    st.claims.update(a=a)
    return st


CHAIN_HOMES = {"chain": 517 * 4 + 1, "chain_wrap": (1 << 12) - 2}  # the second: its next group is group 0


def chain(name):
    """Five keys of one home group, one per round, so the fifth lives in the next group. The first four are
    removed: the fifth must still be found by Get, Put and Remove through four dead slots, and a new key
    of that home must still land somewhere (past the dead slots) and be found."""
    st = Stream(name, 12)
    g = CHAIN_HOMES[name] >> 2
    ks = S.keys_with_home(lambda h: (h >> 2) == g, 8, 12)
    for k in ks[:5]:
        st.add([k], False, ks)
    st.add(ks[:4], True, ks)
    st.add([ks[4]], False, ks)                 # Put finds the fifth
    st.add([ks[5]], False, ks)                 # a new key of that home
    st.add([ks[4], ks[5]], True, ks)           # Remove finds both
    st.add([ks[4], ks[0], ks[6]], False, ks)   # revived in the second group and in the first; one more new
    st.claims.update(keys=ks, group=g)
    return st


def side(name, tomb):
    """The key 2^64 - 1 (the side slot): Put, Remove, Get, Put."""
    st = Stream(name, 8, tomb=tomb)
    k = np.array([S.SIDE], U64)
    other = S.free_keys(3)
    st.add(np.concatenate([other, k]), False)
    st.add(k, True)
    st.add(k, True)                            # dead already
    st.add(k, False)
    st.add(np.concatenate([k, k, k]), [True, False, True])
    st.add(np.concatenate([k, k]), [False, False])
    return st


SIZES = (1, 63, 64, 65, 511, 512, 513, 2049)


def sizes(n):
    """A round of n records, about a third Removes, over live, dead and absent keys."""
    st = Stream(f"sizes_{n}", 14)
    base = S.free_keys(600)
    st.add(base, False)
    st.add(base[:200], True)                   # dead
    rng = np.random.default_rng(n)
    pool = np.concatenate([base, S.free_keys(300, 600)])  # live, dead, absent
    keys = pool[rng.integers(0, len(pool), n)]
    rm = rng.permutation(np.arange(n) % 3 == 0)  # a third, to the record
    if n == 1:
        rm[:] = True
        keys[0] = base[300]
    st.add(keys, rm)
    st.claims.update(n=n)
    return st


CHURN_ROUND = 25  # records per round: live + n stays within a 2^8 table's 128 keys (hm_room's target)


def churn(max_log2, rounds=50, purge_every=0):
    """100 new keys put, then removed, `rounds` times, CHURN_ROUND records a round. With growth on, hm_room's
    target is the table that holds live + n keys: at most 100 + 25 here, so a 2^8 table purges and never
    grows (whole rounds of 100 would have it grow to 2^9 for live + n = 200)."""
    st = Stream(f"churn_{max_log2}_{purge_every}", 8, max_log2=max_log2)
    for r in range(rounds):
        ks = S.free_keys(100, 100 * r)
        for rm in (False, True):
            for lo in range(0, 100, CHURN_ROUND):
                st.add(ks[lo:lo + CHURN_ROUND], rm, ks[::7])
    st.claims.update(purge_every=purge_every)
    return st


def full_exact():
    """A fixed 256-slot table filled to its last slot, 40 of the slots then dead: no probe of an absent key
    meets an empty slot any more. A Remove of an absent key walks the whole table and answers None, as a
    Get of it answers absent, and latches nothing; dead keys are still found for revival and for another
    Remove."""
    st = Stream("full_exact", 8)
    ks = S.keys_with_home(lambda h: h >= 0, 256, 8)
    for lo in range(0, 256, 64):
        st.add(ks[lo:lo + 64], False)
    gone = S.absent_keys(30)
    st.add(np.concatenate([ks[:40], gone]), True, np.concatenate([ks[:60], gone]))
    st.add(np.concatenate([gone[:10], ks[:20], ks[20:40], S.absent_keys(10, 30)]),
           np.concatenate([np.ones(10, bool), np.zeros(20, bool), np.ones(30, bool)]),
           np.concatenate([ks[:60], gone, S.absent_keys(10, 30)]))
    st.claims.update(keys=ks, gone=gone)
    return st


def grow_with_dead():
    """A 2^8 table that may grow to 2^10, with rounds whose records do not fit beside the live keys while
    dead slots are there: hm_room's target is larger than the table, the rehash drops the dead slots on
    the way, and keys_ub = live + n afterwards. Twice: 2^8 -> 2^9 with 30 dead slots, 2^9 -> 2^10 with 50."""
    st = Stream("grow_with_dead", 8, max_log2=10)
    a, b, c, d = (S.free_keys(n, lo) for n, lo in ((60, 0), (100, 60), (100, 160), (100, 260)))
    st.add(a, False)
    st.add(a[:30], True)
    st.add(b, False, np.concatenate([a, b]))       # 30 live + 100 > 128: grows, 30 dead slots dropped
    st.add(b[:50], True)
    st.add(c, False)                               # occupancy 130 + 100 fits 2^9's 256: nothing happens
    st.add(d, False, np.concatenate([a, b, c, d]))  # 180 live + 100 > 256: grows, 50 dead slots dropped
    st.add(np.concatenate([a[:10], d[:10]]), [False] * 10 + [True] * 10)
    return st


NAMES = (["present_absent_dead", "never_claims", "in_chunk_order", "one_bucket_edges", "revival", "chain",
          "chain_wrap", "side_default", "side_other", "full_exact"] + [f"sizes_{n}" for n in SIZES])
_built = {}


def by_name(name):
    """The stream of that name (built once; treat it as read-only)."""
    if name not in _built:
        if name.startswith("sizes_"):
            st = sizes(int(name[6:]))
        elif name.startswith("chain"):
            st = chain(name)
        elif name.startswith("side_"):
            st = side(name, TOMB if name == "side_default" else OTHER_TOMB)
        else:
            st = {"present_absent_dead": present_absent_dead, "never_claims": never_claims,
                  "in_chunk_order": in_chunk_order, "one_bucket_edges": one_bucket_edges, "revival": revival,
                  "full_exact": full_exact}[name]()
        assert st.name == name
        _built[name] = st
    return _built[name]
