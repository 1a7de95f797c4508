"""The key-partitioned skip list without a GPU: the C ABI declares and exports the new calls, NULL
groups are refused, and the shared streams of tests/skiplist_part_streams.py reach what the GPU tests
(tests/test_gpu_skiplist_partitioned.py) rely on them for -- shown with the sequential model and
nrgpu.parallel.key_owner alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import skiplist_part_streams as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["nrg_skiplist_prefill_partition", "nrg_group_skiplist_seek", "nrg_group_skiplist_range_count"]


@pytest.fixture(scope="module")
def lib():
    import nrgpu

    return nrgpu.load()


def test_header_declares_and_library_exports(lib):
    from nrgpu import _lib as L

    with open(os.path.join(ROOT, "include", "nrgpu.h")) as f:
        h = f.read()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, h, re.M), name
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    assert re.search(r"\}\s*nrg_seek;", h) and re.search(r"\}\s*nrg_count;", h)
    # the structs as the header lays them out
    assert [f[0] for f in L.Seek._fields_] == ["keys", "n", "out_keys", "out_vals", "found"]
    assert [f[0] for f in L.Count._fields_] == ["los", "his", "n", "counts"]
    assert C.sizeof(L.Seek) == 40 and C.sizeof(L.Count) == 32


def test_null_groups_are_refused(lib):
    from nrgpu import _lib as L

    q, c = L.Seek(), L.Count()
    assert lib.nrg_group_skiplist_seek(None, C.byref(q), L.NRG_SEEK_GE) == L.NRG_E_INVAL
    assert lib.nrg_group_skiplist_range_count(None, C.byref(c)) == L.NRG_E_INVAL
    assert lib.nrg_skiplist_prefill_partition(None, 10, 0, 0, 1) == L.NRG_E_INVAL


def test_key_owner_is_the_librarys(lib):
    keys = np.concatenate([np.arange(2000, dtype=np.uint64), np.array([S.U64_MAX, S.COMMON], np.uint64)])
    for G in (1, 3, 8):
        own = S.key_owner(keys, G)
        assert [lib.nrg_key_owner(int(k), G) for k in keys[::37]] == own[::37].tolist()


@pytest.mark.parametrize("G,skew,pipelined", S.ROUND_CASES)
def test_round_streams_reach_their_cases(G, skew, pipelined):
    n = S.n_rounds(pipelined)
    rs = S.rounds(G, skew)[:n]
    assert 4 <= len(rs) <= 5
    views = S.member_view(G, rs)
    if skew:  # owner 0 replays at least two slices in every round
        assert all(x > S.MAX_BATCH for x in views[0]["rput"])
        assert all(k.size == 4000 for parts in rs for (k, _, _, _) in parts)
    if skew or G == 1:  # some owner answers its Gets in more than one slice
        assert any(x > S.MAX_READS for vw in views for x in vw["rget"])
    for p, vw in enumerate(views):
        assert vw["model"].compactions >= 1, f"member {p} never compacts at delta_max {S.DELTA_MAX}"
        assert vw["peak"] <= S.CAPACITY, f"member {p} would be clipped"
    # the sizes rotate through every W and R, the ends of the key space and the shared key are there
    ws = {len(k) for parts in rs for (k, _, _, _) in parts}
    rr = {len(gk) for parts in rs for (_, _, gk, _) in parts}
    assert rr == set(S.R_ROT)
    assert ws == ({4000} if skew else set(S.W_ROT))
    allk = np.concatenate([k for parts in rs for (k, _, _, _) in parts])
    assert 0 in allk and S.U64_MAX in allk
    if skew or G == 1:  # some round in which every member pushes the shared key
        assert any(all(S.COMMON in k for (k, _, _, _) in parts) for parts in rs)
    else:  # (members with W = 0 push nothing) every member that pushes, pushes it
        assert all(S.COMMON in k for parts in rs for (k, _, _, _) in parts if len(k))
    # the members' final key sets are disjoint and add up to the global model's
    m, answers = S.expected(G, skew, n)
    assert sum(len(vw["model"]) for vw in views) == len(m)
    assert len(answers) == n and all(len(a) == G for a in answers)
    # the shared key: the highest rank that pushed it in the last round it was pushed wins
    last = [parts for parts in rs if any(S.COMMON in k for (k, _, _, _) in parts)][-1]
    k, v = [(k, v) for (k, v, _, _) in last if S.COMMON in k][-1]
    assert m.get(S.COMMON) == int(v[np.nonzero(k == S.COMMON)[0][-1]])


@pytest.mark.parametrize("G", [1, 3])
def test_drop_stream(G):
    rs = S.drop_rounds(G)
    m, answers = S.expected_drop(G)
    assert answers[2] is None and all(a is not None for r, a in enumerate(answers) if r != 2)
    full = S.prefilled(3000)
    S.replay(full, rs)
    assert full.arrays()[1].tolist() != m.arrays()[1].tolist()  # dropping round 2 is visible in the contents


@pytest.mark.parametrize("G", [3, 8])
def test_seek_queries_cross_ranks(G):
    m = S.seek_state(G)
    keys = m.arrays()[0]
    for mode in S.MODES:
        qs = S.seek_queries(keys, G, mode)
        assert {len(q) for q in qs} <= set(S.N_ROT) and len({len(q) for q in qs}) >= 3  # ragged
        elsewhere = multi = False
        for asker, q in enumerate(qs):
            if not len(q):
                continue
            found, key = S.candidates(keys, G, q, mode)
            ok, _, f = S.seek_expected(m, q, mode)
            for j in np.nonzero(f)[0]:
                win = [p for p in range(G) if found[p][j] and key[p][j] == ok[j]]
                assert len(win) == 1  # disjoint partitions: no ties
                elsewhere |= win[0] != asker
                multi |= int(found[:, j].sum()) >= 3 and win[0] != 0
            assert len(q) < 7 or (0 in q and S.U64_MAX in q)
        assert elsewhere and multi, mode
    ragged = {tuple(len(q) for q in S.seek_queries(keys, G, mode)) for mode in S.MODES}
    assert len(ragged) == 4  # every member asks 0, 1, 257 and 1000 keys over the four modes


def test_one_rank_asks_every_size():
    keys = S.seek_state(1).arrays()[0]
    assert sorted(len(S.seek_queries(keys, 1, mode)[0]) for mode in S.MODES) == sorted(S.N_ROT)


def test_sparse_group_leaves_partitions_empty():
    own = set(S.key_owner(S.SPARSE_KEYS, 8).tolist())
    assert len(own) <= 3 and len(set(range(8)) - own) >= 5
    # and a query set against it gets "none" for every query from at least five ranks
    q = S.seek_queries(S.SPARSE_KEYS, 8, 0)[3]
    found, _ = S.candidates(S.SPARSE_KEYS, 8, q, 0)
    assert len(q) == 1000 and (~found).all(axis=1).sum() >= 5 and found.any()


def test_count_queries_have_their_edges():
    for G in (1, 3, 8):
        m = S.seek_state(G)
        cq = S.count_queries(m.arrays()[0], G)
        assert {len(lo) for lo, _ in cq} <= set(S.N_ROT)
        big = [(lo, hi) for lo, hi in cq if len(lo) == 1000][0]
        exp = S.count_expected(m, *big)
        assert (big[0] > big[1]).any() and exp[0] == len(m) and exp[1] == 0 and exp[2] in (0, 1)
        assert exp.max() > 1000
