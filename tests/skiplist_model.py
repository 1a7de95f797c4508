"""A sequential model of the replicated skip list (ordered map u64 -> u64, csrc/skiplist.hip).

The contents are a dict plus a sorted key list (bisect): insert replaces the value of a present key
and answers the key (SkipMap::insert behind SkipListWrapper, benches/lockfree_partitioned.rs:86-118).
The model also carries the device's two-run policy, stated once: a chunk's new keys go to the delta
run, and the delta run is merged into the base run (a compaction) when nd > delta_max after a chunk's
merge. It mirrors the kernels' tile constants, so the tests can place chunk sizes around them.
"""
from __future__ import annotations

import bisect

import numpy as np

from nrgpu import _lib as L
from nrgpu import digest as _digest

# csrc/skiplist.hip constexpr values (test_skiplist_cpu.py pins them to the source)
SL_SORT_WG = 1024     # chunks up to here sort in one workgroup
SL_SORT_TILE = 2048   # keys per tile of the radix sort's passes
SL_RES_TILE = 256     # records per resolve / scatter workgroup
SL_MERGE_PART = 2048  # outputs per merge workgroup
TILE_CONSTANTS = {"SL_SORT_WG": SL_SORT_WG, "SL_SORT_TILE": SL_SORT_TILE, "SL_RES_TILE": SL_RES_TILE,
                  "SL_MERGE_PART": SL_MERGE_PART}
LOG2_MIN, LOG2_MAX, LOG2_DEFAULT = 4, 28, 24
DELTA_DEFAULT = 1 << 22
U64_MAX = 2**64 - 1


class SkipListModel:
    def __init__(self, delta_max: int = DELTA_DEFAULT, max_batch: int = 1 << 20):
        self.m = {}
        self.keys = []        # sorted
        self.delta = set()    # the keys of the delta run
        self.delta_max = delta_max
        self.max_batch = max_batch
        self.compactions = 0

    # -- the two-run policy ----------------------------------------------------------------
    @property
    def nd(self) -> int:
        return len(self.delta)

    @property
    def nb(self) -> int:
        return len(self.keys) - len(self.delta)

    def _chunk(self, keys, vals):
        for k, v in zip(keys, vals):
            k, v = int(k), int(v)
            if k not in self.m:
                bisect.insort(self.keys, k)
                self.delta.add(k)
            self.m[k] = v
        if self.nd > self.delta_max:  # compact when nd > delta_max after a chunk's merge
            self.delta.clear()
            self.compactions += 1

    def insert_many(self, keys, vals):
        """Records in order, cut into chunks of max_batch as a replay or a prefill cuts them."""
        keys, vals = list(keys), list(vals)
        for at in range(0, len(keys), self.max_batch):
            self._chunk(keys[at:at + self.max_batch], vals[at:at + self.max_batch])

    def replay(self, recs):
        """recs: PUT_DTYPE records or (key, val) pairs. Returns (resp, some): the key, 1."""
        if isinstance(recs, np.ndarray) and recs.dtype.names:
            keys, vals = recs["key"].tolist(), recs["val"].tolist()
        else:
            keys, vals = [int(r[0]) for r in recs], [int(r[1]) for r in recs]
        self.insert_many(keys, vals)
        return np.array(keys, np.uint64), np.ones(len(keys), np.uint8)

    def restore(self, pairs):
        """The state after nrg_restore: everything in the base run."""
        self.m = {int(k): int(v) for k, v in pairs}
        self.keys = sorted(self.m)
        self.delta = set()

    # -- reads -------------------------------------------------------------------------------
    def __len__(self):
        return len(self.keys)

    def get(self, k):
        return self.m.get(int(k))

    def seek(self, k, mode):
        """(key, value) or None; mode L.NRG_SEEK_GE / GT / LE / LT."""
        k = int(k)
        ks = self.keys
        if mode == L.NRG_SEEK_GE:
            i = bisect.bisect_left(ks, k)
        elif mode == L.NRG_SEEK_GT:
            i = bisect.bisect_right(ks, k)
        elif mode == L.NRG_SEEK_LE:
            i = bisect.bisect_right(ks, k) - 1
        elif mode == L.NRG_SEEK_LT:
            i = bisect.bisect_left(ks, k) - 1
        else:
            raise ValueError("seek mode")
        if i < 0 or i >= len(ks):
            return None
        return ks[i], self.m[ks[i]]

    def range(self, lo, hi):
        """The pairs with lo <= key <= hi, ascending."""
        lo, hi = int(lo), int(hi)
        if lo > hi:
            return []
        ks = self.keys[bisect.bisect_left(self.keys, lo):bisect.bisect_right(self.keys, hi)]
        return [(k, self.m[k]) for k in ks]

    def range_count(self, lo, hi):
        lo, hi = int(lo), int(hi)
        if lo > hi:
            return 0
        return bisect.bisect_right(self.keys, hi) - bisect.bisect_left(self.keys, lo)

    def items(self):
        return [(k, self.m[k]) for k in self.keys]

    def arrays(self):
        k = np.array(self.keys, np.uint64)
        return k, np.array([self.m[x] for x in self.keys], np.uint64)

    def digest(self):
        return _digest.skiplist(*self.arrays())
