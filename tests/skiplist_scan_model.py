"""A sequential model of the skip list's range scans (nrg_skiplist_scan / nrg_group_skiplist_scan):
SkipMap::range from a bound, the first `limit` entries, ascending for GE / GT and descending for
LE / LT. `scan` answers one query by bisect over the sorted keys; `reduce_lists` mirrors the group's
reduce kernel (a candidate's place is its place in its own list plus the candidates of the other
lists that precede it); the named query sets and limits are the ones the GPU tests use.
"""
from __future__ import annotations

import bisect

import numpy as np

from nrgpu import _lib as L
from nrgpu.parallel import key_owner

U64_MAX = 2**64 - 1
MODES = (L.NRG_SEEK_GE, L.NRG_SEEK_GT, L.NRG_SEEK_LE, L.NRG_SEEK_LT)
UP = (L.NRG_SEEK_GE, L.NRG_SEEK_GT)
MAX_LIMIT = 1024  # NRG_SCAN_MAX_LIMIT


def log2_width(limit: int) -> int:
    """csrc/skiplist.hip sl_walk_log2_width: the lane group is the power of two at or above
    `limit`, up to a wave of 64."""
    lw = 0
    while lw < 6 and (1 << lw) < limit:
        lw += 1
    return lw


def steps(limit: int) -> int:
    w = 1 << log2_width(limit)
    return (limit + w - 1) // w


def shape_limits():
    """Every limit at which the group width or the step count changes, and that limit +- 1."""
    out = set()
    for lim in range(2, MAX_LIMIT + 1):
        if (log2_width(lim), steps(lim)) != (log2_width(lim - 1), steps(lim - 1)):
            out.update(x for x in (lim - 1, lim, lim + 1) if 1 <= x <= MAX_LIMIT)
    return sorted(out)


NAMED_LIMITS = (1, 2, 3, 63, 64, 65, 128, 1024)


def scan(sorted_keys, vals, k: int, mode: int, limit: int):
    """The first `limit` (key, value) pairs from the bound k in the mode's direction. `vals` is a
    sequence parallel to sorted_keys or a dict key -> value."""
    k = int(k)
    val = (lambda i: vals[sorted_keys[i]]) if isinstance(vals, dict) else (lambda i: vals[i])
    if mode == L.NRG_SEEK_GE:
        i = bisect.bisect_left(sorted_keys, k)
    elif mode == L.NRG_SEEK_GT:
        i = bisect.bisect_right(sorted_keys, k)
    elif mode == L.NRG_SEEK_LE:
        i = bisect.bisect_right(sorted_keys, k) - 1
    elif mode == L.NRG_SEEK_LT:
        i = bisect.bisect_left(sorted_keys, k) - 1
    else:
        raise ValueError("scan mode")
    if mode in UP:
        idx = range(i, min(len(sorted_keys), i + limit))
    else:
        idx = range(i, max(-1, i - limit), -1)
    return [(int(sorted_keys[j]), int(val(j))) for j in idx]


def scan_batch(sorted_keys, vals, qs, mode: int, limit: int):
    """(keys[n, limit], vals[n, limit], counts[n]) with `fill` nowhere: rows are padded with zeros;
    compare only the first counts[i] columns of a row."""
    n = len(qs)
    ok = np.zeros((n, limit), np.uint64)
    ov = np.zeros((n, limit), np.uint64)
    cnt = np.zeros(n, np.uint32)
    for i, q in enumerate(qs):
        r = scan(sorted_keys, vals, int(q), mode, limit)
        cnt[i] = len(r)
        if r:
            ok[i, :len(r)] = [p[0] for p in r]
            ov[i, :len(r)] = [p[1] for p in r]
    return ok, ov, cnt


def reduce_lists(lists, mode: int, limit: int):
    """The group's reduce (csrc/group.cpp grp_scan_reduce_kernel): G candidate lists of (key, value),
    each in the scan's order and of disjoint keys, to the first `limit` of their merge, by counting:
    the place of candidate t of list o is t + the candidates of every other list that precede it."""
    up = mode in UP
    out = [None] * limit
    for o, lst in enumerate(lists):
        for t, (k, v) in enumerate(lst):
            place = t
            for p, other in enumerate(lists):
                if p != o:
                    place += sum(1 for (x, _) in other if (x < k if up else x > k))
            if place < limit:
                assert out[place] is None, "two candidates at one place"
                out[place] = (k, v)
    total = min(limit, sum(len(lst) for lst in lists))
    assert all(x is not None for x in out[:total]) and all(x is None for x in out[total:])
    return out[:total]


def partition(sorted_keys, vals, G: int):
    """The map split by nrg_key_owner: per partition (sorted keys, values)."""
    ks = np.array(sorted_keys, np.uint64)
    vs = np.array(vals, np.uint64)
    own = key_owner(ks, G) if len(ks) else np.zeros(0, np.int64)
    return [(ks[own == p].tolist(), vs[own == p].tolist()) for p in range(G)]


def edge_queries(sorted_keys) -> np.ndarray:
    """Below the smallest key, above the largest, equal to stored keys, between stored keys, and the
    ends of the key space."""
    qs = {0, 1, U64_MAX, U64_MAX - 1, U64_MAX - 2, 1 << 63}
    ks = [int(k) for k in sorted_keys]
    if ks:
        pick = sorted({0, 1, 2, len(ks) // 3, len(ks) // 2, len(ks) - 3, len(ks) - 2, len(ks) - 1} & set(range(len(ks))))
        for i in pick:
            k = ks[i]
            qs.update(x for x in (k - 1, k, k + 1) if 0 <= x <= U64_MAX)
        qs.add(max(ks[0] - 1, 0))
        qs.add(min(ks[-1] + 1, U64_MAX))
    return np.array(sorted(qs), np.uint64)


def random_queries(sorted_keys, n: int, seed: int) -> np.ndarray:
    """n queries: stored keys, their neighbours and uniform u64s, shuffled."""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    if len(sorted_keys):
        ks = np.array(sorted_keys, np.uint64)
        hit = ks[rng.integers(0, len(ks), size=n)]
        d = rng.integers(0, 3, size=n).astype(np.uint64)  # k - 1, k, k + 1 (wrapping is fine: any u64 is a query)
        with np.errstate(over="ignore"):
            near = hit + d - np.uint64(1)
        take = rng.random(n) < 0.7
        out = np.where(take, near, out)
    return out


def mirror(k: int) -> int:
    """The order-reversing bijection of u64: LE / LT on the keys are GE / GT on the mirrored keys."""
    return U64_MAX - int(k)
