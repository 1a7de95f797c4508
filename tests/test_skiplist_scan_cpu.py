"""The skip list's range scans without a GPU: the scan model (tests/skiplist_scan_model.py) against a
brute-force filter, sort and slice; the mirror of the group's reduce over nrg_key_owner partitions
against the whole-map scan; limit = 1 against SkipListModel.seek; and the C ABI: the header
declares and the library exports the three calls, and NULL handles are refused."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import skiplist_model as M
import skiplist_scan_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["nrg_skiplist_scan", "nrg_skiplist_scan_async", "nrg_group_skiplist_scan"]
U64_MAX = SM.U64_MAX


@pytest.fixture(scope="module")
def lib():
    import nrgpu

    return nrgpu.load()


def _maps():
    """(name, sorted keys, values): empty, one key, the ends of the key space, a dense stretch, random"""
    rng = np.random.default_rng(5)
    rnd = sorted(set(rng.integers(0, 1 << 64, size=300, dtype=np.uint64).tolist()) | {0, U64_MAX})
    dense = list(range(10, 200, 3))
    out = [("empty", []), ("one", [77]), ("ends", [0, U64_MAX]), ("dense", dense), ("random", rnd)]
    return [(name, ks, [(k * 0x9E3779B97F4A7C15 + 1) & U64_MAX for k in ks]) for name, ks in out]


def _brute(ks, vs, k, mode, limit):
    from nrgpu import _lib as L

    keep = {L.NRG_SEEK_GE: lambda x: x >= k, L.NRG_SEEK_GT: lambda x: x > k, L.NRG_SEEK_LE: lambda x: x <= k,
            L.NRG_SEEK_LT: lambda x: x < k}[mode]
    pairs = sorted(((x, v) for x, v in zip(ks, vs) if keep(x)), reverse=mode not in SM.UP)
    return pairs[:limit]


@pytest.mark.parametrize("name,ks,vs", _maps(), ids=[m[0] for m in _maps()])
def test_model_is_filter_sort_slice(name, ks, vs):
    qs = SM.edge_queries(ks).tolist() + SM.random_queries(ks, 40, 3).tolist()
    for mode in SM.MODES:
        for limit in (1, 2, 3, 7, 64, 65, 1024):
            for q in qs:
                assert SM.scan(ks, vs, q, mode, limit) == _brute(ks, vs, q, mode, limit), (name, mode, limit, q)
    # a dict of values answers the same
    d = dict(zip(ks, vs))
    assert SM.scan(ks, d, 50, SM.MODES[0], 5) == SM.scan(ks, vs, 50, SM.MODES[0], 5)


def test_edges_of_the_key_space():
    from nrgpu import _lib as L

    ks = [0, 5, U64_MAX]
    vs = [1, 2, 3]
    assert SM.scan(ks, vs, 0, L.NRG_SEEK_GE, 8) == [(0, 1), (5, 2), (U64_MAX, 3)]
    assert SM.scan(ks, vs, U64_MAX, L.NRG_SEEK_LE, 8) == [(U64_MAX, 3), (5, 2), (0, 1)]
    assert SM.scan(ks, vs, U64_MAX, L.NRG_SEEK_GT, 8) == []
    assert SM.scan(ks, vs, 0, L.NRG_SEEK_LT, 8) == []
    assert SM.scan(ks, vs, U64_MAX - 1, L.NRG_SEEK_GT, 8) == [(U64_MAX, 3)]
    ok, ov, cnt = SM.scan_batch(ks, vs, [0, 6], L.NRG_SEEK_GT, 2)
    assert cnt.tolist() == [2, 1] and ok.tolist() == [[5, U64_MAX], [U64_MAX, 0]] and ov.tolist() == [[2, 3], [3, 0]]


@pytest.mark.parametrize("G", [1, 2, 3, 8])
def test_reduce_over_partitions_is_the_whole_map_scan(G):
    """Every partition scans its own keys; the reduce mirror of the G candidate lists equals the scan
    of the whole map, whether a partition has `limit` candidates, fewer or none."""
    for name, ks, vs in _maps():
        parts = SM.partition(ks, vs, G)
        assert sorted(k for p in parts for k in p[0]) == ks
        qs = SM.edge_queries(ks).tolist()[:24] + SM.random_queries(ks, 6, G).tolist()
        for mode in SM.MODES:
            for limit in (1, 5, 64):
                for q in qs:
                    lists = [SM.scan(pk, pv, q, mode, limit) for pk, pv in parts]
                    assert SM.reduce_lists(lists, mode, limit) == SM.scan(ks, vs, q, mode, limit), (name, G, mode, limit, q)


def test_limit_one_is_the_seek():
    m = M.SkipListModel()
    _, ks, vs = _maps()[-1]
    m.insert_many(ks, vs)
    for mode in SM.MODES:
        for q in SM.edge_queries(ks).tolist() + SM.random_queries(ks, 100, 9).tolist():
            s = m.seek(q, mode)
            assert SM.scan(m.keys, m.m, q, mode, 1) == ([s] if s else []), (mode, q)


def test_descending_is_ascending_on_the_mirrored_keys():
    from nrgpu import _lib as L

    _, ks, vs = _maps()[-1]
    mk = [SM.mirror(k) for k in reversed(ks)]
    mv = list(reversed(vs))
    for down, up in ((L.NRG_SEEK_LE, L.NRG_SEEK_GE), (L.NRG_SEEK_LT, L.NRG_SEEK_GT)):
        for q in SM.edge_queries(ks).tolist():
            a = SM.scan(ks, vs, q, down, 9)
            b = SM.scan(mk, mv, SM.mirror(q), up, 9)
            assert [(SM.mirror(k), v) for k, v in b] == a


def test_widths_and_shape_limits():
    assert [SM.log2_width(x) for x in (1, 2, 3, 4, 5, 8, 9, 32, 33, 64, 65, 1024)] == [0, 1, 2, 2, 3, 3, 4, 5, 6, 6, 6, 6]
    assert [SM.steps(x) for x in (1, 64, 65, 128, 129, 1024)] == [1, 1, 2, 2, 3, 16]
    lims = SM.shape_limits()
    for x in (1, 2, 3, 4, 5, 6, 8, 9, 10, 32, 33, 34, 64, 65, 66, 128, 129, 130, 960, 961, 962):
        assert x in lims, x
    with open(os.path.join(ROOT, "node-replication_amd", "csrc", "skiplist.hip")) as f:
        src = f.read()
    # the mirror above is of this source: the width doubles up to 2^6 while it is below the limit
    assert re.search(r"while \(lw < 6 && \(1u << lw\) < limit\) lw\+\+;", src)


def test_header_declares_and_library_exports(lib):
    from nrgpu import _lib as L

    with open(os.path.join(ROOT, "include", "nrgpu.h")) as f:
        h = f.read()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, h, re.M), name
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    assert re.search(r"#define NRG_SCAN_MAX_LIMIT 1024u", h) and L.NRG_SCAN_MAX_LIMIT == 1024
    assert re.search(r"\}\s*nrg_scan;", h)
    assert [f[0] for f in L.Scan._fields_] == ["keys", "n", "out_keys", "out_vals", "counts"]
    assert C.sizeof(L.Scan) == 40


def test_null_handles_are_refused(lib):
    from nrgpu import _lib as L

    k = np.zeros(4, np.uint64)
    ok, ov, cnt = np.full(8, 7, np.uint64), np.full(8, 7, np.uint64), np.full(4, 7, np.uint32)
    p = [a.ctypes.data_as(C.c_void_p) for a in (k, ok, ov, cnt)]
    assert lib.nrg_skiplist_scan(None, p[0], 4, L.NRG_SEEK_GE, 2, p[1], p[2], p[3]) == L.NRG_E_INVAL
    assert lib.nrg_skiplist_scan_async(None, p[0], 4, L.NRG_SEEK_GE, 2, p[1], p[2], p[3]) == L.NRG_E_INVAL
    q = L.Scan()
    assert lib.nrg_group_skiplist_scan(None, C.byref(q), L.NRG_SEEK_GE, 2) == L.NRG_E_INVAL
    assert np.all(ok == 7) and np.all(ov == 7) and np.all(cnt == 7)


def test_python_read_op_is_exported():
    import nrgpu

    s = nrgpu.Scan(5, 0, 16)
    assert (s.key, s.mode, s.limit) == (5, 0, 16) and "Scan" in nrgpu.__all__
