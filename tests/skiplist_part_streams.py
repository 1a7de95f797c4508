"""Round streams and query sets of the key-partitioned skip list (nrg_group_partitioned_round on a
group of NRG_DS_SKIPLIST replicas, nrg_group_skiplist_seek / _range_count), built once for the CPU
and the GPU tests.

A stream is a list of rounds, a round one (keys, vals, get_keys, wants_resp) per member. Expected
answers come from tests/skiplist_model.py replaying the global log W_0 || ... || W_{G-1} round by
round (rank order is the NR global-log order of every key), the Gets of a round against the state
after it. The per-member view -- what each owner receives, in which slices it replays it, when it
compacts -- is modelled too, so that the CPU tests can show a stream reaches what it is named for.
"""
from __future__ import annotations

import functools

import numpy as np

import skiplist_model as M
from nrgpu import _lib as L
from nrgpu.parallel import key_owner

U64_MAX = M.U64_MAX
# the GPU tests' configuration
LOG2_SLOTS, MAX_BATCH, MAX_READS, DELTA_MAX = 16, 4096, 2048, 512
CAPACITY = 1 << LOG2_SLOTS
PREFILL, SPAN = 6000, 30_000
W_ROT, R_ROT = (0, 1, 2500, 4000), (3000, 0, 1700)
# (G, skew, pipelined): the round cases; the one-rank data-moving form (NRG_KNOB_EXP bit 16) reuses (1, F)
ROUND_CASES = [(1, False, False), (1, False, True), (3, False, False), (3, True, False), (3, False, True),
               (8, False, False), (8, True, True)]
COMMON = 12_345  # one key pushed by every member that pushes in a round
MODES = (L.NRG_SEEK_GE, L.NRG_SEEK_GT, L.NRG_SEEK_LE, L.NRG_SEEK_LT)
N_ROT = (0, 1, 257, 1000)  # ragged query counts per member


def n_rounds(pipelined) -> int:
    return 5 if pipelined else 4


@functools.lru_cache(maxsize=None)
def owned0(G: int) -> np.ndarray:
    """keys below SPAN that partition 0 of G owns"""
    pool = np.arange(SPAN, dtype=np.uint64)
    return pool[key_owner(pool, G) == 0]


@functools.lru_cache(maxsize=None)
def rounds(G: int, skew: bool, n: int = 5):
    """skew: every Put and Get of every member (but the keys 0 and 2^64 - 1) belongs to partition 0"""
    own = owned0(G)
    out = []
    for r in range(n):
        parts = []
        for i in range(G):
            rng = np.random.default_rng(1000 * r + 10 * i + (5 if skew else 0) + 100_000 * G)
            W = 4000 if skew else W_ROT[(i + r) % 4]
            R = R_ROT[(i + r) % 3]
            if skew:
                k = own[rng.integers(0, len(own), W)].copy()
                gk = own[rng.integers(0, len(own), R)].copy()
            else:
                k = rng.integers(0, SPAN, W, dtype=np.uint64)
                gk = rng.integers(0, SPAN + 2000, R, dtype=np.uint64)
            if W:
                k[::40] = COMMON
            if W > 10:
                k[5], k[7] = 0, U64_MAX
            if R > 10:
                gk[3], gk[4], gk[5] = 0, U64_MAX, COMMON
            v = rng.integers(0, U64_MAX, W, dtype=np.uint64, endpoint=True)
            parts.append((k, v, gk, bool((i + r) % 2 == 1 or skew)))
        out.append(parts)
    return out


@functools.lru_cache(maxsize=None)
def drop_rounds(G: int):
    """five rounds of the dropped-bad-round test (round 2 is the bad one)"""
    out = []
    for r in range(5):
        parts = []
        for i in range(G):
            rng = np.random.default_rng(7000 + 40 * r + i)
            W, R = 700 + 50 * i, 900
            parts.append((rng.integers(0, 12_000, W, dtype=np.uint64),
                          rng.integers(0, U64_MAX, W, dtype=np.uint64, endpoint=True),
                          rng.integers(0, 12_000, R, dtype=np.uint64), True))
        out.append(parts)
    return out


def prefilled(n: int = PREFILL, off: int = 0) -> M.SkipListModel:
    m = M.SkipListModel()
    m.insert_many(range(n), range(off, n + off))
    return m


def replay(model: M.SkipListModel, rs, skip=()):
    """The global log of the rounds `rs` (but those in `skip`) into `model`; per round and member the
    Gets' (vals, found), None for a skipped round."""
    out = []
    for r, parts in enumerate(rs):
        if r in skip:
            out.append(None)
            continue
        for (k, v, _, _) in parts:
            model.insert_many(k.tolist(), v.tolist())
        ans = []
        for (_, _, gk, _) in parts:
            got = [model.get(x) for x in gk.tolist()]
            ans.append((np.array([0 if g is None else g for g in got], np.uint64),
                        np.array([g is not None for g in got], np.uint8)))
        out.append(ans)
    return out


@functools.lru_cache(maxsize=None)
def expected(G: int, skew: bool, n: int):
    """(model after the n rounds, the Gets' answers per round and member)"""
    m = prefilled()
    return m, replay(m, rounds(G, skew)[:n])


@functools.lru_cache(maxsize=None)
def expected_drop(G: int):
    m = prefilled(3000)
    return m, replay(m, drop_rounds(G), skip=(2,))


# ---- the per-member view -------------------------------------------------------------------------------
def prefill_slices(n: int, part: int, parts: int, max_batch: int = MAX_BATCH):
    """nrg_skiplist_prefill_partition's chunks: the owned keys of each slice of max_batch keys"""
    out = []
    for at in range(0, n, max_batch):
        k = np.arange(at, min(n, at + max_batch), dtype=np.uint64)
        out.append(k[key_owner(k, parts) == part])
    return out


def member_view(G: int, rs, prefill: int = PREFILL):
    """Per member: its model (delta policy at DELTA_MAX, replay slices of MAX_BATCH), and per round the
    Puts and Gets it received and the most keys it ever held."""
    views = []
    for p in range(G):
        m = M.SkipListModel(DELTA_MAX, MAX_BATCH)
        for k in prefill_slices(prefill, p, G):
            m.insert_many(k.tolist(), k.tolist())
        views.append(dict(model=m, rput=[], rget=[], peak=len(m)))
    for parts in rs:
        for p, vw in enumerate(views):
            ks = [k[key_owner(k, G) == p] if len(k) else k for (k, _, _, _) in parts]
            vs = [v[key_owner(k, G) == p] if len(k) else v for (k, v, _, _) in parts]
            rk = np.concatenate(ks) if ks else np.zeros(0, np.uint64)
            rv = np.concatenate(vs) if vs else np.zeros(0, np.uint64)
            vw["model"].insert_many(rk.tolist(), rv.tolist())  # rank order, cut at MAX_BATCH
            vw["rput"].append(len(rk))
            vw["rget"].append(sum(int((key_owner(gk, G) == p).sum()) if len(gk) else 0 for (_, _, gk, _) in parts))
            vw["peak"] = max(vw["peak"], len(vw["model"]))
    return views


# ---- group-wide seeks and range counts -----------------------------------------------------------------
def _pool(keys_sorted, seed: int) -> np.ndarray:
    """queries at 0, 2^64 - 1, present keys, their neighbours (gaps or present) and far gaps"""
    rng = np.random.default_rng(seed)
    ks = np.asarray(keys_sorted, np.uint64)
    fixed = np.array([0, U64_MAX, 1, U64_MAX - 1, COMMON, 1 << 63, SPAN + 5000], np.uint64)
    if len(ks) == 0:
        return np.concatenate([fixed, rng.integers(0, SPAN, 1200, dtype=np.uint64)])
    pres = ks[rng.integers(0, len(ks), 400)]
    with np.errstate(over="ignore"):
        near = np.concatenate([pres + np.uint64(1), pres - np.uint64(1)])
    gaps = rng.integers(0, SPAN + 4000, 400, dtype=np.uint64)
    return np.concatenate([fixed, pres, near, gaps])


def seek_queries(keys_sorted, G: int, mode: int, seed: int = 0):
    """per member: its keys; n rotates over N_ROT with the member and the mode"""
    pool = _pool(keys_sorted, 17 + seed)
    out = []
    for i in range(G):
        n = N_ROT[(i + mode) % 4]
        rng = np.random.default_rng(100 * mode + i + seed)
        q = pool[rng.integers(0, len(pool), n)] if n > 7 else pool[:n].copy()
        if n > 7:
            q[:7] = pool[:7]
        out.append(q)
    return out


def count_queries(keys_sorted, G: int, seed: int = 0):
    """per member: (los, his); some with lo > hi, the whole key space, single present keys"""
    pool = _pool(keys_sorted, 29 + seed)
    out = []
    for i in range(G):
        n = N_ROT[(i + 1) % 4] if G > 1 else N_ROT[3]
        rng = np.random.default_rng(900 + i + seed)
        a = pool[rng.integers(0, len(pool), n)]
        b = pool[rng.integers(0, len(pool), n)]
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        if n > 7:
            lo[0], hi[0] = 0, U64_MAX
            lo[1], hi[1] = U64_MAX, 0          # lo > hi
            lo[2], hi[2] = a[2], a[2]          # one key
            lo[3], hi[3] = hi[3], lo[3]        # swapped: lo > hi unless they are equal
            lo[4], hi[4] = U64_MAX, U64_MAX
            lo[5], hi[5] = 0, 0
        elif n == 1:
            lo[0], hi[0] = 0, U64_MAX
        out.append((lo, hi))
    return out


def seek_expected(model: M.SkipListModel, q: np.ndarray, mode: int):
    ok, ov, f = np.zeros(len(q), np.uint64), np.zeros(len(q), np.uint64), np.zeros(len(q), np.uint8)
    for j, k in enumerate(q.tolist()):
        hit = model.seek(k, mode)
        if hit is not None:
            ok[j], ov[j], f[j] = hit[0], hit[1], 1
    return ok, ov, f


def count_expected(model: M.SkipListModel, lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    return np.array([model.range_count(a, b) for a, b in zip(lo.tolist(), hi.tolist())], np.uint64)


def candidates(keys_sorted, G: int, q: np.ndarray, mode: int):
    """found[p][j], key[p][j]: partition p's candidate for query j (the per-member seek)"""
    ks = np.asarray(keys_sorted, np.uint64)
    own = key_owner(ks, G) if len(ks) else np.zeros(0, np.int64)
    found = np.zeros((G, len(q)), bool)
    key = np.zeros((G, len(q)), np.uint64)
    for p in range(G):
        part = ks[own == p]
        if mode in (L.NRG_SEEK_GE, L.NRG_SEEK_GT):
            idx = np.searchsorted(part, q, side="left" if mode == L.NRG_SEEK_GE else "right")
            ok = idx < len(part)
        else:
            idx = np.searchsorted(part, q, side="right" if mode == L.NRG_SEEK_LE else "left") - 1
            ok = idx >= 0
        found[p] = ok
        if len(part):
            key[p][ok] = part[idx[ok]]
    return found, key


SPARSE_KEYS = np.array([5, 20_000, U64_MAX], np.uint64)  # the three keys of the sparse group


@functools.lru_cache(maxsize=None)
def seek_state(G: int):
    """the model after the first two rounds of the plain stream of G members"""
    m = prefilled()
    replay(m, rounds(G, False)[:2])
    return m
