"""A sequential model of the skip list with removal (nrg_skiplist_enable_removal, csrc/skiplist.hip),
and the named streams the CPU and the GPU tests replay.

The model is tests/skiplist_model.py's dict plus sorted key list, with ops applied one by one: a
record whose val is the tombstone is Remove(key) (SkipMap::remove: the previous value or None, the
key absent afterwards), every other record Push(key, val) (the key, Some). It knows nothing of the
kernels. It carries the device's two-run policy as the parent does, stated once: per chunk, a key that
was absent before the chunk and is present after it goes to the delta run, a key that was present and
is absent leaves its run, a key present before and after stays where it was; the delta run is merged
into the base run when nd > delta_max after the chunk. With a capacity, a chunk's new keys are admitted
against the key count before the chunk's own removals: the largest ones that do not fit are left out
and the error is counted.

A stream is a list of chunks (PUT_DTYPE records) for one configuration; plan() counts, from the
records alone (its own bookkeeping of which run holds which key, no model), the arms its name
promises (`needs`: arm -> the least count).
"""
from __future__ import annotations

import bisect
import functools
from collections import Counter

import numpy as np

import skiplist_model as M
from nrgpu import _lib as L

U64_MAX = M.U64_MAX
TOMB = U64_MAX                 # DeviceReplica.sl_enable_removal's default
SL_DROP_PART = 2048            # csrc/skiplist.hip: inputs per drop workgroup (test_skiplist_remove_cpu.py pins it)
SL_RES_TILE = M.SL_RES_TILE
SL_SORT_WG = M.SL_SORT_WG


PUT_DTYPE = np.dtype([("key", "<u8"), ("val", "<u8")])  # nrg_put (nrgpu.PUT_DTYPE)


def recs_of(keys, vals) -> np.ndarray:
    r = np.zeros(len(keys), PUT_DTYPE)
    r["key"], r["val"] = np.array(keys, np.uint64), np.array(vals, np.uint64)
    return r


class SkipListRemoveModel(M.SkipListModel):
    def __init__(self, delta_max: int = M.DELTA_DEFAULT, max_batch: int = 1 << 20, tombstone: int = TOMB,
                 capacity: int | None = None):
        super().__init__(delta_max, max_batch)
        self.tombstone = tombstone
        self.capacity = capacity
        self.capacity_errors = 0
        self.base_drops = 0    # chunks that removed a key of the base run
        self.delta_drops = 0   # chunks that removed a key of the delta run
        self._out = None

    def _apply(self, k, v, banned=()):
        """one op; (response, some)"""
        if v == self.tombstone:
            if k not in self.m:
                return 0, 0
            prev = self.m.pop(k)
            del self.keys[bisect.bisect_left(self.keys, k)]
            return prev, 1
        if k not in banned:
            if k not in self.m:
                bisect.insort(self.keys, k)
            self.m[k] = v
        return k, 1

    def _chunk(self, keys, vals):
        keys, vals = [int(k) for k in keys], [int(v) for v in vals]
        before = set(self.m)
        banned = ()
        if self.capacity is not None:
            # the chunk's new keys: absent before it, and its last record of the key is a Push
            last = {}
            for k, v in zip(keys, vals):
                last[k] = v
            new = sorted(k for k, v in last.items() if v != self.tombstone and k not in before)
            room = max(0, self.capacity - len(before))
            if len(new) > room:
                self.capacity_errors += 1
                banned = set(new[room:])  # contents are unspecified from here on; this is what the device does
        for k, v in zip(keys, vals):
            r, s = self._apply(k, v, banned)
            if self._out is not None:
                self._out.append((r, s))
        after = set(self.m)
        gone = before - after
        gone_delta = gone & self.delta
        if gone - gone_delta:
            self.base_drops += 1
        if gone_delta:
            self.delta_drops += 1
        self.delta -= gone_delta
        self.delta |= after - before
        if self.nd > self.delta_max:
            self.delta.clear()
            self.compactions += 1

    def replay(self, recs):
        """recs: PUT_DTYPE records or (key, val) pairs. Returns (resp u64, some u8), one per record."""
        if isinstance(recs, np.ndarray) and recs.dtype.names:
            keys, vals = recs["key"].tolist(), recs["val"].tolist()
        else:
            keys, vals = [int(r[0]) for r in recs], [int(r[1]) for r in recs]
        self._out = []
        try:
            self.insert_many(keys, vals)
            out = self._out
        finally:
            self._out = None
        return np.array([r for r, _ in out], np.uint64), np.array([s for _, s in out], np.uint8)

    def scan(self, k, mode, limit):
        """SkipMap::range from a bound, the first `limit` pairs: ascending for GE / GT, descending for LE / LT"""
        ks = self.keys
        if mode in (L.NRG_SEEK_GE, L.NRG_SEEK_GT):
            i = bisect.bisect_left(ks, k) if mode == L.NRG_SEEK_GE else bisect.bisect_right(ks, k)
            out = ks[i:i + limit]
        else:
            i = bisect.bisect_right(ks, k) if mode == L.NRG_SEEK_LE else bisect.bisect_left(ks, k)
            out = ks[max(0, i - limit):i][::-1]
        return [(x, self.m[x]) for x in out]


def plain_dict(chunks, tombstone=TOMB):
    """The same ops on a plain dict: (the dict, the responses of every chunk)."""
    d, out = {}, []
    for c in chunks:
        resp, some = [], []
        for k, v in zip(c["key"].tolist(), c["val"].tolist()):
            if v == tombstone:
                some.append(int(k in d))
                resp.append(d.pop(k, 0))
            else:
                d[k] = v
                resp.append(k)
                some.append(1)
        out.append((np.array(resp, np.uint64), np.array(some, np.uint8)))
    return d, out


# ---- streams ---------------------------------------------------------------------------------------------
class Stream:
    """A named stream: the context's shape, its chunks, and the arms its name promises."""

    def __init__(self, name, chunks, needs, log2=14, delta_max=256, max_batch=8192, capacity=None, error=False):
        self.name, self.chunks, self.needs = name, chunks, needs
        self.log2, self.delta_max, self.max_batch = log2, delta_max, max_batch
        self.capacity = capacity  # the model checks the capacity rule only where a stream is about it
        self.error = error        # the stream ends with NRG_E_CAPACITY latched
        assert all(len(c) <= max_batch for c in chunks)

    def model(self, max_batch=None) -> SkipListRemoveModel:
        return SkipListRemoveModel(self.delta_max, max_batch or self.max_batch, TOMB, self.capacity)

    def plan(self) -> Counter:
        """The arms the chunks reach, each replayed as one chunk, from the records alone."""
        a = Counter()
        run = {}           # key -> "b" | "d"
        for c in self.chunks:
            keys, vals = c["key"].tolist(), c["val"].tolist()
            n = len(keys)
            a["sort_wg" if n <= SL_SORT_WG else "sort_radix"] += 1
            order = sorted(range(n), key=lambda i: (keys[i], i))
            base = sorted(k for k, r in run.items() if r == "b")
            delta = sorted(k for k, r in run.items() if r == "d")
            deadb, deadd, new = [], [], []
            tomb_seen = False
            s = 0
            while s < n:
                e = s
                while e + 1 < n and keys[order[e + 1]] == keys[order[s]]:
                    e += 1
                k = keys[order[s]]
                ops = [vals[order[i]] == TOMB for i in range(s, e + 1)]  # True: Remove
                tomb_seen |= any(ops)
                a["tiles_of_one_key"] = max(a["tiles_of_one_key"], e // SL_RES_TILE - s // SL_RES_TILE + 1)
                for i, rm in enumerate(ops):
                    if rm:
                        a["resp_from_chunk" if i else "resp_from_state"] += 1
                        if i and ops[i - 1] and s + i == 256:
                            a["rr_straddle_256"] += 1
                present = k in run
                if ops[-1]:
                    if not present:
                        a["rm_absent"] += 1
                        if not all(ops):
                            a["push_then_remove_new"] += 1
                    elif run[k] == "b":
                        a["rm_base_hit"] += 1
                        deadb.append(bisect.bisect_left(base, k))
                    else:
                        a["rm_delta_hit"] += 1
                        deadd.append(bisect.bisect_left(delta, k))
                else:
                    if present and any(ops):
                        a["remove_then_push_present"] += 1
                    if not present:
                        new.append(k)
                s = e + 1
            for dead, nrun, tag in ((deadb, len(base), "base"), (deadd, len(delta), "delta")):
                if not dead:
                    continue
                a["drop_%s_chunks" % tag] += 1
                a["dead_first"] += dead[0] == 0
                a["dead_last"] += dead[-1] == nrun - 1
                a["dead_at_part_edge"] += sum(1 for x in dead if x >= SL_DROP_PART - 1 and (x + 1) % SL_DROP_PART <= 2)
                longest = cur = 1
                for x, y in zip(dead, dead[1:]):
                    cur = cur + 1 if y == x + 1 else 1
                    longest = max(longest, cur)
                a["dead_run_longer_than_part"] += longest > SL_DROP_PART
                a["all_%s_dead" % tag] += len(dead) == nrun
            if tomb_seen and not deadb and not deadd:
                a["no_drop_rm_chunks"] += 1
            if not tomb_seen:
                a["no_tombstone_chunks"] += 1
            if self.capacity is not None and len(new) > self.capacity - len(run):
                a["capacity_error_chunks"] += 1
                new = new[:max(0, self.capacity - len(run))]
            for k in (base[i] for i in deadb):
                del run[k]
            for k in (delta[i] for i in deadd):
                del run[k]
            if deadd and len(deadd) == len(delta):
                a["drop_empties_delta"] += 1
            if (deadb or deadd) and not run:
                a["map_emptied"] += 1
            for k in new:
                run[k] = "d"
            nd = sum(1 for r in run.values() if r == "d")
            if nd > self.delta_max:
                a["compactions"] += 1
                a["compaction_with_base_drop"] += bool(deadb)
                for k in run:
                    run[k] = "b"
        return a


NBASE, NDELTA = 6000, 200
BASE_KEYS = [1000 + 3 * i for i in range(NBASE)]        # = 1 (mod 3)
DELTA_KEYS = [1002 + 90 * i for i in range(NDELTA)]     # = 0 (mod 3)


def absent(i):                                          # = 2 (mod 3): in neither run after the setup
    return 1001 + 3 * i


def _vals(rng, n):
    return rng.integers(0, U64_MAX, n, dtype=np.uint64)  # (never the tombstone: the bound is exclusive)


def _one(rng):
    return int(rng.integers(0, U64_MAX, dtype=np.uint64))


def _setup(rng, nbase=NBASE, ndelta=NDELTA):
    """two chunks: nbase keys that compact into base (nbase > delta_max), ndelta that stay in delta"""
    out = [recs_of(BASE_KEYS[:nbase][::-1], _vals(rng, nbase))]
    if ndelta:
        out.append(recs_of(DELTA_KEYS[:ndelta], _vals(rng, ndelta)))
    return out


def _removes(keys):
    return recs_of(keys, [TOMB] * len(keys))


def _shuffled(rng, r):
    return r[rng.permutation(len(r))]


def _mixed(rng, n):
    """n records over keys of both runs and absent ones, about a third of them Removes"""
    pool = np.array(BASE_KEYS[:400] + DELTA_KEYS[:60] + [absent(i) for i in range(300)], np.uint64)
    keys = pool[rng.integers(0, len(pool), n)]
    vals = _vals(rng, n)
    vals[rng.random(n) < 0.35] = TOMB
    return recs_of(keys, vals)


@functools.lru_cache(maxsize=None)
def streams():
    out = []

    def add(name, chunks, needs, **kw):
        out.append(Stream(name, chunks, needs, **kw))

    rng = np.random.default_rng(2024)
    add("base_every_third", _setup(rng) + [_shuffled(rng, _removes(BASE_KEYS[::3]))],
        dict(rm_base_hit=NBASE // 3, drop_base_chunks=1))
    new = [absent(7 * i) for i in range(40)]  # (200 + 40 <= delta_max: they stay in delta)
    add("delta_previous_chunk", _setup(rng) + [recs_of(new, _vals(rng, 40)), _shuffled(rng, _removes(new))],
        dict(rm_delta_hit=40, drop_delta_chunks=1))
    gone = [absent(i) for i in range(300)] + [0, U64_MAX, 5]
    add("absent", _setup(rng) + [_removes(gone + gone[:40])],
        dict(rm_absent=303, no_drop_rm_chunks=1, resp_from_chunk=40))
    k, v = [], []
    for i in range(50):
        k += [absent(1000 + i), BASE_KEYS[i], absent(1000 + i)]
        v += [_one(rng), _one(rng), TOMB]
    add("push_then_remove", _setup(rng) + [recs_of(k, v)], dict(push_then_remove_new=50, no_drop_rm_chunks=1))
    k, v = [], []
    for i in range(50):
        for key in (BASE_KEYS[11 * i], DELTA_KEYS[3 * i]):
            k += [key, absent(i), key]
            v += [TOMB, _one(rng), _one(rng)]
    add("remove_then_push", _setup(rng) + [recs_of(k, v)], dict(remove_then_push_present=100, resp_from_state=100))
    # 255 smaller keys, then one base key removed twice: sorted positions 255 and 256
    small = list(range(1, 256))
    k = small[:100] + [BASE_KEYS[500]] + small[100:] + [BASE_KEYS[500]] + [absent(3000 + i) for i in range(40)]
    v = _vals(rng, len(k))
    v[100] = v[256] = TOMB
    add("remove_remove_straddle", _setup(rng) + [recs_of(k, v)], dict(rr_straddle_256=1, rm_base_hit=1))
    alt = [_one(rng) if i % 2 == 0 else TOMB for i in range(600)]
    add("alternate_600", _setup(rng) + [recs_of([absent(77)] * 600, alt), recs_of([BASE_KEYS[9]] * 600, alt[1:] + [123]),
                                        recs_of([DELTA_KEYS[9]] * 600, alt[1:] + [TOMB])],
        dict(tiles_of_one_key=3, resp_from_chunk=598, rm_absent=1, rm_delta_hit=1))
    ends = [0, U64_MAX]
    add("ends", _setup(rng) + [recs_of(ends, [10, 11]), _removes(ends), _removes(ends), recs_of(ends, [12, 13]),
                               recs_of(ends + ends + ends, [TOMB, TOMB, 14, 15, TOMB, 16])],
        dict(rm_delta_hit=3, rm_absent=2, remove_then_push_present=1))
    edges = [0, NBASE - 1] + [p * SL_DROP_PART + d for p in (1, 2) for d in (-1, 0, 1)]
    add("drop_edges", _setup(rng) + [_removes([BASE_KEYS[i] for i in edges] + [DELTA_KEYS[0], DELTA_KEYS[-1]]),
                                     _removes(BASE_KEYS[100:2400])],
        dict(dead_first=2, dead_last=2, dead_at_part_edge=6, dead_run_longer_than_part=1, drop_delta_chunks=1))
    add("every_base_key", _setup(rng) + [_shuffled(rng, _removes(BASE_KEYS)), recs_of(BASE_KEYS[:30], _vals(rng, 30))],
        dict(all_base_dead=1, rm_base_hit=NBASE))
    add("every_delta_key", _setup(rng, 3000, 0) + [recs_of(DELTA_KEYS[:1] + [absent(i) for i in range(2998)], _vals(rng, 2999))]
        + [_removes(DELTA_KEYS[:1] + [absent(i) for i in range(2998)]), recs_of([absent(5)], [5])],
        dict(all_delta_dead=1, drop_empties_delta=1, dead_run_longer_than_part=1), delta_max=2999)
    add("every_key", _setup(rng) + [_shuffled(rng, _removes(BASE_KEYS + DELTA_KEYS)), _removes([5, BASE_KEYS[0]]),
                                    recs_of([7, U64_MAX, BASE_KEYS[3]], [1, 2, 3])],
        dict(all_base_dead=1, all_delta_dead=1, map_emptied=1))
    add("sort_arms", _setup(rng) + [_mixed(rng, n) for n in (1, 255, 256, 257, 1024, 1025, 2049, 4097)],
        dict(sort_wg=6, sort_radix=4, rm_base_hit=100, rm_delta_hit=20, rm_absent=100, resp_from_chunk=100))
    few = [absent(2000 + i) for i in range(10)]
    add("compaction_interplay", _setup(rng) + [recs_of([absent(3000 + i) for i in range(100)] + BASE_KEYS[40:90],
                                                       _vals(rng, 100).tolist() + [TOMB] * 50),
                                               recs_of(few, _vals(rng, 10)), _removes(few)],
        dict(compaction_with_base_drop=1, drop_empties_delta=1, compactions=2))
    # the capacity rule, on a full map of 2^10 keys
    full = recs_of(range(0, 3 * 1024, 3), _vals(rng, 1024))
    add("capacity_room_next_chunk", [full, _removes([3 * i for i in range(10)]), recs_of([3 * i + 1 for i in range(10)], _vals(rng, 10))],
        dict(rm_delta_hit=10, capacity_error_chunks=0), log2=10, delta_max=1024, capacity=1024)
    add("capacity_same_chunk", [full, recs_of([30, 31], [TOMB, 1])],
        dict(rm_delta_hit=1, capacity_error_chunks=1), log2=10, delta_max=1024, capacity=1024, error=True)
    return out


def by_name(name) -> Stream:
    return next(s for s in streams() if s.name == name)


NAMES = [s.name for s in streams()]
