"""Models and named streams for removal and pops in a partitioned skip-list group
(nrg_group_skiplist_enable_removal / _enable_pops, nrg_group_skiplist_pop), shared by
tests/test_skiplist_group_pop_cpu.py and the GPU tests.

UnionModel is one map holding the whole key space, ops applied one at a time: a round's records in rank
order, then issue order (Push answers (key, 1), Remove (previous value, 1) or (0, 0)); a group pop's
requests, concatenated in rank order, as pop_front() / pop_back() called n times each. It knows nothing
of partitions, candidates or kernels. cut() is the other side: what each member loses, computed per
member from the candidate lists alone by the rank formula of the select step.

A stream names a state (a prefill by nrg_skiplist_prefill_partition and partitioned Push rounds on top of
it, so both runs hold entries) and the requests of every rank.
"""
from __future__ import annotations

import bisect

import numpy as np

import skiplist_pop_model as P
import skiplist_scan_model as SM

U64_MAX = SM.U64_MAX
TOMB, FRONT, BACK = P.TOMB, P.FRONT, P.BACK
OFF = 9                      # the prefill's value offset
PREFILL = 1500
NRG_SCAN_MAX_LIMIT = 1024
N_ROT = (0, 1, 37, 300)      # ragged request counts per member
CLUSTER_AT = 1 << 50
GS = (1, 3, 8)


class UnionModel:
    def __init__(self, tombstone=None):
        self.m, self.keys, self.tomb = {}, [], tombstone

    def prefill(self, n, off=OFF):
        for k in range(n):
            self.push(k, (k + off) & U64_MAX)  # (u64 arithmetic, as the device's)

    def push(self, k, v):
        if k not in self.m:
            bisect.insort(self.keys, k)
        self.m[k] = v

    def replay(self, recs):
        """records (key, val) one at a time: (resp u64[n], some u8[n])"""
        resp, some = [], []
        for k, v in recs:
            k, v = int(k), int(v)
            if self.tomb is not None and v == self.tomb:
                if k in self.m:
                    resp.append(self.m.pop(k))
                    some.append(1)
                    del self.keys[bisect.bisect_left(self.keys, k)]
                else:
                    resp.append(0)
                    some.append(0)
            else:
                self.push(k, v)
                resp.append(k)
                some.append(1)
        return np.array(resp, np.uint64), np.array(some, np.uint8)

    def get(self, keys):
        return (np.array([self.m.get(int(k), 0) for k in keys], np.uint64),
                np.array([int(k) in self.m for k in keys], np.uint8))

    def pop_run(self, reqs):
        """reqs[r]: rank r's (n, back) list. Per rank: (counts u64, keys u64, vals u64), the entries packed
        in request order, each request's in the order popped."""
        out = []
        for mine in reqs:
            cnt, ks, vs = [], [], []
            for n, back in mine:
                m = min(int(n), len(self.keys))
                take = self.keys[len(self.keys) - m:][::-1] if back else self.keys[:m]
                if m:
                    if back:
                        del self.keys[len(self.keys) - m:]
                    else:
                        del self.keys[:m]
                cnt.append(m)
                for k in take:
                    ks.append(k)
                    vs.append(self.m.pop(k))
            out.append((np.array(cnt, np.uint64), np.array(ks, np.uint64), np.array(vs, np.uint64)))
        return out

    def items(self):
        return [(k, self.m[k]) for k in self.keys]

    def members(self, G):
        """per member: the sorted keys it owns"""
        k = np.array(self.keys, np.uint64)
        own = SM.key_owner(k, G) if len(k) else np.zeros(0, np.int64)
        return [k[own == p] for p in range(G)]


def totals(reqs, length):
    """(F, Bk) of the concatenated run against a map of `length` entries"""
    left, F, B = length, 0, 0
    for mine in reqs:
        for n, back in mine:
            m = min(int(n), left)
            left -= m
            if back:
                B += m
            else:
                F += m
    return F, B


def cut(members, F, Bk):
    """What the select step computes: per member (c_f, c_b, candidates contributed at the front, at the
    back). Member o contributes its min(F, len_o) smallest keys; a candidate's rank is its index in its own
    list plus the candidates of every other list below its key; rank < F is popped. Backs from the top."""
    cf_list = [np.asarray(k[:min(F, len(k))]) for k in members]
    cb_list = [np.asarray(k[len(k) - min(Bk, len(k)):][::-1]) for k in members]
    c_f, c_b = [], []
    for o in range(len(members)):
        rank = np.arange(len(cf_list[o]), dtype=np.int64)
        for q, other in enumerate(cf_list):
            if q != o:
                rank = rank + np.searchsorted(other, cf_list[o], side="left")
        c_f.append(int(np.count_nonzero(rank < F)))
        rank = np.arange(len(cb_list[o]), dtype=np.int64)
        for q, other in enumerate(cb_list):
            if q != o:  # keys of `other` above the candidate: descending list, so count from its ascending reverse
                rank = rank + (len(other) - np.searchsorted(other[::-1], cb_list[o], side="right"))
        c_b.append(int(np.count_nonzero(rank < Bk)))
    return c_f, c_b, [len(c) for c in cf_list], [len(c) for c in cb_list]


def cut_by_sorting(members, F, Bk):
    """the same by sorting the union and taking the ends"""
    allk = np.sort(np.concatenate(members)) if members else np.zeros(0, np.uint64)
    front, back = allk[:F], allk[len(allk) - Bk:]
    return ([int(np.isin(k, front).sum()) for k in members], [int(np.isin(k, back).sum()) for k in members])


# ---- streams ---------------------------------------------------------------------------------------------
def cluster_keys(G):
    """six keys from 2^50 on that partition 0 of G owns"""
    pool = np.arange(CLUSTER_AT, CLUSTER_AT + 400, dtype=np.uint64)
    return pool[SM.key_owner(pool, G) == 0][:6]


def round_keys(G, seed=3):
    """one round on top of the prefill: new keys below and between the prefilled ones' span, updates of
    prefilled keys, 0 and 2^64 - 1; at most 64 new keys, so every member's stay in delta"""
    rng = np.random.default_rng(seed)
    k = np.concatenate([rng.integers(0, 2 * PREFILL, 44, dtype=np.uint64), cluster_keys(G),
                        np.array([0, U64_MAX, PREFILL + 7], np.uint64)])
    v = rng.integers(0, U64_MAX - 8, len(k), dtype=np.uint64)  # (no tombstone, no mark)
    return k, v


class Stream:
    def __init__(self, name, prefill, rounds, reqs, cap=None, enable_first=True):
        self.name = name
        self.prefill = prefill    # G -> n of nrg_skiplist_prefill_partition
        self.rounds = rounds      # G -> [(keys, vals)] pushed by rank 0, one partitioned round each
        self.reqs = reqs          # (G, length) -> per rank [(n, back)]
        self.cap = cap            # G -> (rank, pop_cap) of the one rank whose arrays are short, or None
        self.enable_first = enable_first  # the group agrees on pops before the rounds (else after them)

    def state(self, G):
        m = UnionModel()
        m.prefill(self.prefill(G))
        for k, v in self.rounds(G):
            m.replay(zip(k.tolist(), v.tolist()))
        return m


def _ragged(G, length):
    rng = np.random.default_rng(11)
    out = []
    for r in range(G):
        n = N_ROT[(r + 1) % 4] if G > 1 else 37
        c = rng.integers(0, 6, n)
        b = rng.integers(0, 2, n)
        if n >= 2:
            c[0], c[1] = 0, 1
        out.append([(int(x), int(y)) for x, y in zip(c, b)])
    return out


def _cluster_rounds(G):
    """no prefill: a first round of 120 keys per member (above delta_max, so each member's go to base), a
    second of a few (delta); the six smallest keys of the map are partition 0's, three in each round"""
    rng = np.random.default_rng(5)
    c = cluster_keys(G)
    a = np.unique(rng.integers(CLUSTER_AT + 1000, CLUSTER_AT + 10**6, 120 * G, dtype=np.uint64))
    b = np.unique(rng.integers(CLUSTER_AT + 10**6, CLUSTER_AT + 2 * 10**6, 8 * G, dtype=np.uint64))
    ka, kb = np.concatenate([c[:3], a]), np.concatenate([c[3:], b])
    return [(ka, ka ^ np.uint64(0x55)), (kb, kb ^ np.uint64(0xAA))]


def _empty_member_rounds(G):
    """no prefill; keys that the last member does not own (one rank: none at all)"""
    if G == 1:
        return []
    pool = np.arange(100, 1300, dtype=np.uint64)
    k = pool[SM.key_owner(pool, G) != G - 1][:700]
    return [(k, k + np.uint64(3))]


def _marks_rounds(G):
    k, v = round_keys(G, seed=4)
    v = v.copy()
    v[::3] = FRONT
    v[1::3] = BACK
    return [(k, v)]


def _meet(G, length):
    f = length // 3
    out = [[] for _ in range(G)]
    out[0].append((f, 0))
    out[G - 1].append((length - f - 5, 1))
    out[G // 2].append((3, 0))
    out[G - 1].append((3, 1))   # the last record of the run asks for 3 with 2 left: short
    return out


_STD = dict(prefill=lambda G: PREFILL, rounds=lambda G: [round_keys(G)])
STREAMS = [
    Stream("single", reqs=lambda G, n: [[(1, 0)]] + [[] for _ in range(G - 1)], **_STD),
    Stream("ragged", reqs=_ragged, **_STD),
    Stream("cluster", prefill=lambda G: 0, rounds=_cluster_rounds,
           reqs=lambda G, n: [[(2, 0)]] + [[] for _ in range(G - 2)] + ([[(4, 0)]] if G > 1 else [])),
    Stream("wide", prefill=lambda G: 1300 * G, rounds=lambda G: [round_keys(G)],
           reqs=lambda G, n: [[] for _ in range(G - 1)] + [[(1000, 0), (7, 1), (2000, 0)]]),
    Stream("meet", reqs=_meet, **_STD),
    Stream("empty_member", prefill=lambda G: 0, rounds=_empty_member_rounds,
           reqs=lambda G, n: [[(5, r & 1), (40, 1 - (r & 1))] for r in range(G)]),
    Stream("marks_as_values", reqs=lambda G, n: [[(30, 0), (30, 1)] for _ in range(G)], enable_first=False,
           prefill=lambda G: 100, rounds=_marks_rounds),
    Stream("cap", reqs=lambda G, n: [[(20, 0), (9, 1), (15, 0)] for _ in range(G)], cap=lambda G: (G // 2, 25), **_STD),
]
NAMES = [s.name for s in STREAMS]


def by_name(name) -> Stream:
    return next(s for s in STREAMS if s.name == name)
