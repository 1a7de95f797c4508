"""Skip-list pops without a device: the model of tests/skiplist_pop_model.py against a heap
restatement on every named stream, every stream's plan() against what its name promises, the new entry
points on a NULL handle and their declaration in the header (tests/test_abi.py then checks that every
declared symbol is exported), and the Python ops."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import skiplist_pop_model as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64_MAX = 2**64 - 1


@pytest.mark.parametrize("name", P.NAMES)
def test_model_equals_the_heap_restatement(name):
    s = P.by_name(name)
    m = s.model()
    d, want, popped = P.heap_restatement(s.chunks, P.TOMB if s.removal else None)
    for c, (wr, ws) in zip(s.chunks, want):
        resp, some = m.replay(c)
        assert np.array_equal(resp, wr) and np.array_equal(some, ws)
    assert m.popped == popped and dict(m.items()) == d and m.keys == sorted(d)
    assert m.delta <= set(d) and m.nb + m.nd == len(d)


@pytest.mark.parametrize("name", P.NAMES)
def test_model_is_the_same_at_any_chunking(name):
    """contents, responses and popped entries do not depend on where a replay cuts its chunks (the
    steps and the two-run policy do)"""
    s = P.by_name(name)
    a, b = s.model(), s.model(max_batch=P.CHUNKED_MAX_BATCH)
    for c in s.chunks:
        ra, rb = a.replay(c), b.replay(c)
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1])
    assert a.items() == b.items() and a.popped == b.popped


@pytest.mark.parametrize("name", P.NAMES)
def test_plan_meets_the_streams_needs(name):
    s = P.by_name(name)
    p = s.plan()
    for tag, least in s.needs.items():
        assert p[tag] >= least, (tag, p[tag], least)


def test_the_named_properties_are_where_the_names_say():
    plans = {n: P.by_name(n).plan() for n in P.NAMES}
    a = plans["front_base_back_delta"]
    assert a["front_all_delta"] == a["front_both_runs"] == a["back_all_base"] == a["back_both_runs"] == 0
    a = plans["front_delta_back_base"]
    assert a["front_all_base"] == a["front_both_runs"] == a["back_all_delta"] == a["back_both_runs"] == 0
    a = plans["interleaved"]
    assert a["front_all_base"] == a["front_all_delta"] == a["back_all_base"] == a["back_all_delta"] == 0
    # the interleaving is key by key: the first 151 of the front come alternately from the two runs
    m = P.by_name("interleaved").model()
    for c in P.by_name("interleaved").chunks[:3]:
        m.replay(c)
    assert [k for k, _ in m.popped] == list(range(151)) and (m.steps[0]["fb"], m.steps[0]["fd"]) == (76, 75)
    a = plans["empties_delta_only"]
    assert a["shifts"] == 0 and a["empties_base_only"] == a["empties_both"] == 0  # back pops alone: nothing moves
    assert plans["empties_base_only"]["empties_delta_only"] == plans["empties_base_only"]["empties_both"] == 0
    # exhaustion: 100 + 100 + 100 + 50 of 350; the record the grants meet in, then (0, None)
    s = P.by_name("exhaustion")
    m = s.model()
    for c in s.chunks[:2]:
        m.replay(c)
    resp, some = m.replay(s.chunks[2])
    assert resp.tolist() == [100, 100, 100, 50, 0, 0, 0, 0] and some.tolist() == [1, 1, 1, 1, 0, 0, 0, 0]
    assert plans["exhaustion"]["steps"] == 1
    assert plans["run_placement"]["max_segments"] == 9
    c0, c1 = P.by_name("run_placement").chunks[2:4]
    assert c0["val"][0] in (P.FRONT, P.BACK) and c0["val"][-1] not in (P.FRONT, P.BACK)   # a pop run first
    assert c1["val"][-1] in (P.FRONT, P.BACK) and c1["val"][0] not in (P.FRONT, P.BACK)   # a pop run last
    assert np.isin(P.by_name("run_placement").chunks[4]["val"], (P.FRONT, P.BACK)).all()  # a whole chunk
    # cut_500: two runs as one chunk, four when max_batch = 500 cuts both
    assert plans["cut_500"]["steps"] == 2 and P.by_name("cut_500").plan(P.CHUNKED_MAX_BATCH)["steps"] == 4
    # segment_edges: the ordinary segments around the pop runs
    v = P.by_name("segment_edges").chunks[2]["val"]
    pop = np.isin(v, (P.FRONT, P.BACK))
    edges = np.flatnonzero(np.diff(np.concatenate([[1], pop.astype(np.int8), [1]])))
    assert np.diff(edges)[::2].tolist() == [255, 256, 257, 1024, 1025, 255]
    assert plans["one_4096"]["largest_step"] == 4096 and plans["one_4096"]["longest_run"] == 1
    assert plans["many_ones"]["longest_run"] == 4096
    keys = {k for k, _ in _popped("key_extremes")}
    assert {0, U64_MAX} <= keys
    for s in P.streams():  # the sizes stay small
        assert sum(len(c) for c in s.chunks) < 30_000 and s.log2 <= 14 and max(len(c) for c in s.chunks) <= 6000


def _popped(name):
    s = P.by_name(name)
    m = s.model()
    for c in s.chunks:
        m.replay(c)
    return m.popped


def test_pop_semantics_one_op_at_a_time():
    F, B = P.FRONT, P.BACK
    m = P.SkipListPopModel()
    resp, some = m.replay([(5, 50), (3, 30), (9, 90), (1, F), (1, B), (0, F), (2, F), (1, B), (7, 70), (1 << 63, B)])
    assert resp.tolist() == [5, 3, 9, 1, 1, 0, 1, 0, 7, 1] and some.tolist() == [1, 1, 1, 1, 1, 0, 1, 0, 1, 1]
    assert m.popped == [(3, 30), (9, 90), (5, 50), (7, 70)] and len(m) == 0
    assert [s["records"] for s in m.steps] == [5, 1] and m.segments == [4]
    # a removal tombstone beside the marks, and other marks: 2^64 - 2 is then an ordinary value
    m = P.SkipListPopModel(tombstone=P.TOMB, front=0, back=1)
    resp, some = m.replay([(4, F), (6, B), (4, P.TOMB), (9, 0), (9, 1)])
    assert resp.tolist() == [4, 6, F, 1, 0] and some.tolist() == [1, 1, 1, 1, 0] and m.popped == [(6, B)]


# ---- the library, without a device ---------------------------------------------------------------------
def test_null_handle_is_einval():
    import nrgpu
    from nrgpu import _lib as L

    lib = nrgpu.load()
    for s in ("nrg_skiplist_enable_pops", "nrg_skiplist_pops", "nrg_skiplist_round_pops_async", "nrg_skiplist_pop"):
        assert s in L.SIGNATURES and hasattr(lib, s)
    f, b, on, m = C.c_uint64(7), C.c_uint64(7), C.c_int(7), C.c_uint64(7)
    assert lib.nrg_skiplist_enable_pops(None, P.FRONT, P.BACK) == L.NRG_E_INVAL
    assert lib.nrg_skiplist_pops(None, C.byref(f), C.byref(b), C.byref(on)) == L.NRG_E_INVAL
    assert lib.nrg_skiplist_round_pops_async(None, None, 0, 1, None, None, None, None, 0, None) == L.NRG_E_INVAL
    assert lib.nrg_skiplist_pop(None, 0, 1, 1, None, None, C.byref(m)) == L.NRG_E_INVAL
    assert (f.value, b.value, on.value, m.value) == (7, 7, 7, 7)


def test_header_declares_the_entry_points_and_names_the_cost():
    with open(os.path.join(ROOT, "include", "nrgpu.h")) as f:
        h = f.read()
    assert re.search(r"^int nrg_skiplist_enable_pops\(nrg_ctx\* ctx, uint64_t front_mark, uint64_t back_mark\);", h, re.M)
    assert re.search(r"^int nrg_skiplist_pops\(nrg_ctx\* ctx, uint64_t\* front_mark, uint64_t\* back_mark, int\* enabled\);",
                     h, re.M)
    assert re.search(r"^int nrg_skiplist_round_pops_async\(", h, re.M) and re.search(r"^int nrg_skiplist_pop\(", h, re.M)
    sec = h[h.index("---- Skip list:"):h.index("---- file store")]
    assert "no\n * pop_front / pop_back" not in sec and "one segment per\n * record" in sec and "pop_cap covers" in sec
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        with open(os.path.join(ROOT, doc)) as f:
            assert "nrg_skiplist_enable_pops" in f.read(), doc


def test_python_ops():
    import nrgpu

    r = nrgpu.SkipList.encode([nrgpu.SlPush(3, 4), nrgpu.SlPopFront(), nrgpu.SlPopBack(5), nrgpu.SlPopFront(2, mark=0)])
    assert r["key"].tolist() == [3, 1, 5, 2] and r["val"].tolist() == [4, P.FRONT, P.BACK, 0]
    assert nrgpu.SkipList.decode([3, 2, 0], [1, 1, 0]) == [3, 2, None]

    class Dev:
        def __init__(self, marks):
            self.marks = marks

        def sl_pops(self):
            return self.marks

    chk = nrgpu.SkipList.check_ops
    chk(Dev((P.FRONT, P.BACK)), [nrgpu.SlPopFront(3), nrgpu.SlPopBack(), nrgpu.SlPush(1, 2), nrgpu.SlRemove(1)])
    chk(Dev(None), [nrgpu.SlPush(1, P.FRONT)])  # without pops a mark is a value
    with pytest.raises(nrgpu.NrgError):
        chk(Dev(None), [nrgpu.SlPopFront()])
    with pytest.raises(ValueError):
        chk(Dev((5, 6)), [nrgpu.SlPopBack()])
    with pytest.raises(ValueError):
        chk(Dev((P.FRONT, P.BACK)), [nrgpu.SlPush(1, P.BACK)])


def test_constants_match_the_source():
    with open(os.path.join(ROOT, "node-replication_amd", "csrc", "skiplist.hip")) as f:
        src = f.read()
    for name in ("SL_FIND_PART", "SL_TAKE_PART"):
        got = re.search(r"constexpr u32 %s = (\d+);" % name, src)
        assert got and int(got.group(1)) == 2048
    for kernel in ("sl_pop_find", "sl_pop_plan", "sl_pop_take", "sl_pop_shift"):
        assert 'NRG_LAUNCH(c, "%s"' % kernel in src
    with open(os.path.join(ROOT, "node-replication_amd", "nrgpu", "replica.py")) as f:
        py = f.read()
    assert "SL_FRONT_MARK, SL_BACK_MARK = 2**64 - 2, 2**64 - 3" in py and (P.FRONT, P.BACK) == (2**64 - 2, 2**64 - 3)
