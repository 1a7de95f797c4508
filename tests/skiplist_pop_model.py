"""A sequential model of the skip list with pops (nrg_skiplist_enable_pops, csrc/skiplist.hip), and the
named streams the CPU and the GPU tests replay.

The model is tests/skiplist_remove_model.py's (a dict plus a sorted key list, ops applied one by one)
with two more ops: a record {n, FRONT} is PopFront x n and {n, BACK} is PopBack x n, pop_front()
(pop_back()) called n times: the response is (m, m >= 1), m the entries popped, and the entries are kept
in the order popped (the packed output of nrg_skiplist_round_pops_async). It knows nothing of the
kernels. It carries the device's policy as its parents do, stated once: a chunk is cut at its maximal
runs of consecutive pop records; every ordinary stretch between them is a chunk of the parent's (its new
keys go to delta, delta is merged into base when nd > delta_max after it); every run is one pop step,
after which a run (base or delta) that lost a prefix has been shifted. With `tombstone` None the context
has no removal and every non-pop record is a Push.

A stream is a list of chunks (PUT_DTYPE records) for one configuration. Builder keeps a model beside the
chunks it collects, so a stream can ask for len - 1 entries or re-push the key it has just popped; the
properties a stream is named for are counted from the steps the model logs (`needs`: tag -> the least
count), and tests/test_skiplist_pop_cpu.py checks the model itself against a heap restatement.
"""
from __future__ import annotations

import functools
from collections import Counter

import numpy as np

import skiplist_model as M
import skiplist_remove_model as R

U64_MAX = M.U64_MAX
TOMB = R.TOMB
FRONT, BACK = U64_MAX - 1, U64_MAX - 2   # DeviceReplica.sl_enable_pops' defaults
PUT_DTYPE = R.PUT_DTYPE
recs_of = R.recs_of
CHUNKED_MAX_BATCH = 500                  # the chunked path's max_batch (a pop run of "cut_500" straddles it)


class SkipListPopModel(R.SkipListRemoveModel):
    def __init__(self, delta_max: int = M.DELTA_DEFAULT, max_batch: int = 1 << 20, tombstone=None,
                 front: int = FRONT, back: int = BACK):
        super().__init__(delta_max, max_batch, tombstone)
        self.front, self.back = front, back
        self.finds = 0        # chunks searched for pop records (every non-empty chunk)
        self.steps = []       # one dict per pop step
        self.segments = []    # per chunk that has a pop record: the number of segments
        self.shifts = 0       # runs that lost a prefix, over all steps
        self.popped = []      # (key, val) of every entry popped since clear_popped(), in the order popped

    def clear_popped(self):
        self.popped = []

    def _is_pop(self, v):
        return v == self.front or v == self.back

    def _pop_step(self, ns, vals):
        nb, nd = self.nb, self.nd
        st = dict(records=len(ns), nb=nb, nd=nd, f=0, b=0, fb=0, fd=0, bb=0, bd=0, zero_after_meet=0, clipped=0)
        for n, v in zip(ns, vals):
            m = min(n, len(self.keys))
            st["clipped"] += 0 < m < n
            st["zero_after_meet"] += n > 0 and m == 0 and st["f"] + st["b"] > 0
            if v == self.front:
                take = self.keys[:m]
                del self.keys[:m]
                st["f"] += m
            else:
                take = self.keys[len(self.keys) - m:][::-1]
                del self.keys[len(self.keys) - m:]
                st["b"] += m
            for k in take:
                tag = "d" if k in self.delta else "b"
                st[("f" if v == self.front else "b") + tag] += 1
                self.delta.discard(k)
                self.popped.append((k, self.m.pop(k)))
            if self._out is not None:
                self._out.append((m, 1 if m else 0))
        self.shifts += (st["fb"] > 0) + (st["fd"] > 0)
        self.steps.append(st)

    def _chunk(self, keys, vals):
        keys, vals = [int(k) for k in keys], [int(v) for v in vals]
        if not keys:
            return
        self.finds += 1
        n, at, segs, any_pop = len(keys), 0, 0, False
        while at < n:
            e = at
            pop = self._is_pop(vals[at])
            while e < n and self._is_pop(vals[e]) == pop:
                e += 1
            if pop:
                self._pop_step(keys[at:e], vals[at:e])
                any_pop = True
            else:
                super()._chunk(keys[at:e], vals[at:e])
            segs += 1
            at = e
        if any_pop:
            self.segments.append(segs)


def heap_restatement(chunks, tombstone=None, front=FRONT, back=BACK):
    """The same ops with a dict and two heaps with lazy deletion in place of the sorted list: (the final
    dict, per chunk (resp, some), every popped (key, val) in order). No runs, no steps, no segments."""
    import heapq

    d, lo, hi, out, popped = {}, [], [], [], []
    for c in chunks:
        resp, some = [], []
        for k, v in zip(c["key"].tolist(), c["val"].tolist()):
            if v == front or v == back:
                heap, sign = (lo, 1) if v == front else (hi, -1)
                m = 0
                while m < k and d:
                    x = sign * heapq.heappop(heap)
                    if x in d:  # (else: a stale entry of a key that left by the other end or by a Remove)
                        popped.append((x, d.pop(x)))
                        m += 1
                resp.append(m)
                some.append(1 if m else 0)
            elif tombstone is not None and v == tombstone:
                some.append(int(k in d))
                resp.append(d.pop(k, 0))
            else:
                if k not in d:  # (a key that comes back may sit in a heap twice: the second pop finds it gone)
                    heapq.heappush(lo, k)
                    heapq.heappush(hi, -k)
                d[k] = v
                resp.append(k)
                some.append(1)
        out.append((np.array(resp, np.uint64), np.array(some, np.uint8)))
    return d, out, popped


# ---- streams ---------------------------------------------------------------------------------------------
class Stream:
    """A named stream: the context's shape, its chunks, and the properties its name promises."""

    def __init__(self, name, chunks, needs, log2=14, delta_max=256, max_batch=8192, removal=False):
        self.name, self.chunks, self.needs = name, chunks, needs
        self.log2, self.delta_max, self.max_batch, self.removal = log2, delta_max, max_batch, removal
        assert all(len(c) <= max_batch for c in chunks)

    def model(self, max_batch=None) -> SkipListPopModel:
        return SkipListPopModel(self.delta_max, max_batch or self.max_batch, TOMB if self.removal else None)

    def plan(self, max_batch=None) -> Counter:
        """What the stream reaches, from the steps the model logs while it replays the chunks."""
        m = self.model(max_batch)
        a = Counter()
        for c in self.chunks:
            before = m.compactions
            nsteps = len(m.steps)
            m.replay(c)
            if m.compactions > before and len(m.steps) > nsteps and m.steps[nsteps]["nd"] == 0:
                a["pop_after_compaction"] += 1
        for s in m.steps:
            f, b = s["f"], s["b"]
            a["steps"] += 1
            a["front_all_base"] += f > 0 and s["fd"] == 0
            a["front_all_delta"] += f > 0 and s["fb"] == 0
            a["front_both_runs"] += s["fb"] > 0 and s["fd"] > 0
            a["back_all_base"] += b > 0 and s["bd"] == 0
            a["back_all_delta"] += b > 0 and s["bb"] == 0
            a["back_both_runs"] += s["bb"] > 0 and s["bd"] > 0
            a["empties_delta_only"] += s["nd"] > 0 and s["fd"] + s["bd"] == s["nd"] and s["fb"] + s["bb"] < s["nb"]
            a["empties_base_only"] += s["nb"] > 0 and s["fb"] + s["bb"] == s["nb"] and s["fd"] + s["bd"] < s["nd"]
            a["empties_both"] += s["nb"] > 0 and s["nd"] > 0 and f + b == s["nb"] + s["nd"]
            a["grants_meet_mid_record"] += s["clipped"] > 0 and f > 0 and b > 0
            a["zero_after_meet"] += s["zero_after_meet"]
            a["noop_steps"] += f + b == 0
            a["mixed_ends"] += f > 0 and b > 0
            a["longest_run"] = max(a["longest_run"], s["records"])
            a["largest_step"] = max(a["largest_step"], f + b)
        a["max_segments"] = max(m.segments, default=0)
        a["shifts"] = m.shifts
        a["compactions"] = m.compactions
        return a


class Builder:
    def __init__(self, rng, removal=False, delta_max=256):
        self.rng, self.chunks = rng, []
        self.m = SkipListPopModel(delta_max, 1 << 20, TOMB if removal else None)

    def chunk(self, recs):
        self.chunks.append(recs)
        self.m.replay(recs)
        return self

    def push(self, keys):
        return self.chunk(pushes(self.rng, keys))

    def setup(self, base, delta):
        """base (more than delta_max keys: they compact into the base run), then delta (they stay)"""
        assert len(base) > self.m.delta_max >= len(delta)
        self.push(list(base)[::-1])
        if delta:
            self.push(list(delta))
        assert self.m.nb == len(base) and self.m.nd == len(delta)
        return self

    @property
    def len(self):
        return len(self.m)


def pushes(rng, keys):
    return recs_of(list(keys), rng.integers(0, 1 << 62, len(keys), dtype=np.uint64))  # (never a mark or the tombstone)


def pops(*pairs):
    """pairs of ('f' | 'b', n)"""
    return recs_of([n for _, n in pairs], [FRONT if e == "f" else BACK for e, _ in pairs])


def cat(*parts):
    return np.concatenate(parts)


LOW = [100 + 3 * i for i in range(3000)]            # a base run below ...
HIGH = [20000 + 7 * i for i in range(200)]          # ... a delta run
EVEN = [2 * i for i in range(3000)]                 # a base run interleaved key by key, at both ends, with
ODD = [2 * i + 1 for i in range(100)] + [2 * i + 1 for i in range(2900, 3000)]  # this delta run


def fresh(i):                                       # keys no setup holds: above LOW and EVEN, below HIGH
    return 10000 + 2 * i


@functools.lru_cache(maxsize=None)
def streams():
    out = []
    rng = np.random.default_rng(4242)

    def add(name, b, needs, **kw):
        out.append(Stream(name, b.chunks, needs, removal=b.m.tombstone is not None, **kw))

    # counts: 0, 1, len - 1, len, len + 1, 2^63 (and 2^64 - 1), each a chunk of its own, refilled in between
    b = Builder(rng).setup(LOW[:300], HIGH[:50])
    b.chunk(pops(("f", 0))).chunk(pops(("b", 0))).chunk(pops(("f", 1))).chunk(pops(("b", 1)))
    b.chunk(pops(("f", b.len - 1)))
    assert b.len == 1
    b.push(LOW[:300]).chunk(pops(("b", b.len)))
    assert b.len == 0
    b.chunk(pops(("f", 1), ("b", 1)))  # the empty map: None
    b.push(LOW[:300]).chunk(pops(("f", b.len + 1)))
    b.push(LOW[:300]).chunk(pops(("b", 1 << 63)))
    b.push(LOW[:300]).chunk(pops(("f", U64_MAX), ("b", 1 << 63), ("f", U64_MAX)))
    assert b.len == 0
    add("counts", b, dict(noop_steps=3, steps=10))

    b = Builder(rng).setup(LOW, HIGH)
    b.chunk(pops(("f", 50))).chunk(pops(("b", 50))).chunk(pops(("f", 7), ("b", 9), ("f", 1)))
    add("front_base_back_delta", b, dict(front_all_base=2, back_all_delta=2, mixed_ends=1))
    b = Builder(rng).setup(HIGH[:1] + [30000 + 3 * i for i in range(2999)], LOW[:200])
    b.chunk(pops(("f", 50))).chunk(pops(("b", 50))).chunk(pops(("b", 7), ("f", 9), ("b", 1)))
    add("front_delta_back_base", b, dict(front_all_delta=2, back_all_base=2, mixed_ends=1))
    b = Builder(rng).setup(EVEN, ODD)
    b.chunk(pops(("f", 151))).chunk(pops(("b", 151))).chunk(pops(("f", 1), ("b", 1), ("f", 2), ("b", 2), ("f", 30), ("b", 30)))
    add("interleaved", b, dict(front_both_runs=2, back_both_runs=2))

    b = Builder(rng).setup(LOW, HIGH)
    b.chunk(pops(("b", 200)))
    add("empties_delta_only", b, dict(empties_delta_only=1, shifts=0))
    b = Builder(rng).setup(LOW[:300], HIGH)
    b.chunk(pops(("f", 300))).push([5]).chunk(pops(("f", 1)))
    add("empties_base_only", b, dict(empties_base_only=1))
    b = Builder(rng).setup(EVEN, ODD)
    b.chunk(pops(("f", 1000), ("b", 3000))).push(EVEN[:10])
    add("empties_both", b, dict(empties_both=1))

    # 350 entries: 100 + 100 + 100 granted whole, then 50 of 100, then nothing
    b = Builder(rng).setup(LOW[:300], HIGH[:50])
    b.chunk(pops(("f", 100), ("b", 100), ("f", 100), ("b", 100), ("f", 5), ("b", 1), ("f", 0), ("b", 1 << 63)))
    b.push(LOW[:5])
    add("exhaustion", b, dict(grants_meet_mid_record=1, zero_after_meet=3, empties_both=1))

    b = Builder(rng).setup(LOW[:300], [0, U64_MAX])
    b.chunk(pops(("f", 1), ("b", 1))).push([0, U64_MAX]).chunk(pops(("b", 2))).chunk(pops(("f", 2)))
    add("key_extremes", b, dict(front_all_delta=1, back_all_delta=1, front_both_runs=1, back_both_runs=1))

    b = Builder(rng).setup(LOW, HIGH)
    b.chunk(cat(pops(("f", 3), ("b", 3)), pushes(rng, [fresh(i) for i in range(40)])))
    b.chunk(cat(pushes(rng, [fresh(100 + i) for i in range(40)]), pops(("b", 3), ("f", 3))))
    b.chunk(pops(*[("f" if i % 3 else "b", i % 5) for i in range(300)]))
    nine = []
    for i in range(4):
        nine += [pushes(rng, [fresh(200 + 10 * i + q) for q in range(10)] + LOW[50 * i:50 * i + 3]), pops(("f", 2), ("b", 1))]
    b.chunk(cat(*nine, pushes(rng, [fresh(300)])))
    add("run_placement", b, dict(max_segments=9, longest_run=300, steps=7))

    # runs at [450, 560) and [990, 1010): the chunked path's max_batch of 500 cuts both
    b = Builder(rng).setup(LOW, HIGH)
    b.chunk(cat(pushes(rng, [fresh(i) for i in range(450)]), pops(*[("f" if i % 2 else "b", 1 + i % 3) for i in range(110)]),
                pushes(rng, [fresh(1000 + i) for i in range(430)]), pops(*[("f", 2)] * 20), pushes(rng, LOW[500:690])))
    add("cut_500", b, dict(steps=2, longest_run=110))

    b = Builder(rng).setup(LOW, HIGH)
    parts, at = [], 0
    for n in (255, 256, 257, 1024, 1025):
        keys = [fresh(at + i) for i in range(n - n // 4)] + LOW[at:at + n // 4]
        parts += [pushes(rng, [keys[i] for i in rng.permutation(n)]), pops(("f", 3), ("b", 2))]
        at += n
    b.chunk(cat(*parts, pushes(rng, [fresh(at + i) for i in range(255)])))
    add("segment_edges", b, dict(max_segments=11, compactions=3))

    b = Builder(rng).setup(LOW, HIGH)
    b.chunk(cat(pushes(rng, [fresh(i) for i in range(100)] + [1, 2]), pops(("f", 4), ("b", 4))))  # 200 + 102 > 256
    first = b.m.keys[:6]
    b.chunk(cat(pops(("f", 6)), pushes(rng, first[::2]), pops(("f", 2)), pushes(rng, first)))
    add("pipeline_interplay", b, dict(pop_after_compaction=1, compactions=2))

    b = Builder(rng, removal=True).setup(LOW, HIGH)
    b.chunk(cat(recs_of([LOW[0], HIGH[-1]], [TOMB, TOMB]), pops(("f", 1), ("b", 1))))
    k0, k1 = b.m.keys[0], b.m.keys[1]
    b.chunk(cat(recs_of([k1, 7], [TOMB, 70]), pops(("f", 3)), recs_of([7, k0], [TOMB, TOMB]), pops(("f", 1))))
    add("with_removal", b, dict(steps=3, mixed_ends=1))

    b = Builder(rng).setup(LOW + [fresh(i) for i in range(3000)], HIGH)
    b.chunk(pops(("f", 4096)))
    add("one_4096", b, dict(largest_step=4096, steps=1))
    b = Builder(rng).setup(LOW + [fresh(i) for i in range(3000)], HIGH)
    b.chunk(pops(*[("f", 1)] * 4096)).chunk(pops(*[("b" if i % 7 == 0 else "f", 1) for i in range(4096)]))
    add("many_ones", b, dict(longest_run=4096, largest_step=4096, steps=2))
    return out


def by_name(name) -> Stream:
    return next(s for s in streams() if s.name == name)


NAMES = [s.name for s in streams()]
