"""Skip-list removal without a device: the model of tests/skiplist_remove_model.py against a plain
dict on every named stream, every stream's plan() against what its name promises, the two new entry
points on a NULL handle, and their declaration in the header (tests/test_abi.py then checks that
every declared symbol is exported)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import skiplist_remove_model as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64_MAX = 2**64 - 1


@pytest.mark.parametrize("name", R.NAMES)
def test_model_equals_a_plain_dict(name):
    s = R.by_name(name)
    m = s.model()
    d, want = R.plain_dict(s.chunks)
    for c, (wr, ws) in zip(s.chunks, want):
        resp, some = m.replay(c)
        if not s.error:
            assert np.array_equal(resp, wr) and np.array_equal(some, ws)
    assert m.capacity_errors == (1 if s.error else 0)
    if s.error:  # the dict has no capacity: the model leaves the key that did not fit out
        assert len(m) == len(d) - 1 and len(m) <= s.capacity
        return
    assert dict(m.items()) == d and m.keys == sorted(d) and len(m) == len(d)
    assert m.delta <= set(d) and m.nb + m.nd == len(d)


@pytest.mark.parametrize("name", R.NAMES)
def test_model_is_the_same_at_any_chunking(name):
    """contents and responses do not depend on where a replay cuts its chunks (the two-run policy does)"""
    s = R.by_name(name)
    if s.capacity is not None:
        return  # (the capacity rule is per chunk: section "Capacity" of the header)
    a, b = s.model(), s.model(max_batch=300)
    for c in s.chunks:
        ra, rb = a.replay(c), b.replay(c)
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1])
    assert a.items() == b.items()


@pytest.mark.parametrize("name", R.NAMES)
def test_plan_meets_the_streams_needs(name):
    s = R.by_name(name)
    p = s.plan()
    for arm, least in s.needs.items():
        assert p[arm] >= least, (arm, p[arm], least)
    # the plan's bookkeeping of the runs and the model's agree on what a chunk drops and compacts
    m = s.model()
    for c in s.chunks:
        m.replay(c)
    assert (p["drop_base_chunks"], p["drop_delta_chunks"], p["compactions"]) == (m.base_drops, m.delta_drops, m.compactions)
    assert p["capacity_error_chunks"] == m.capacity_errors


def test_the_named_arms_are_where_the_names_say():
    P = {n: R.by_name(n).plan() for n in R.NAMES}
    assert P["absent"]["drop_base_chunks"] == P["absent"]["drop_delta_chunks"] == 0
    assert P["push_then_remove"]["drop_base_chunks"] == P["push_then_remove"]["drop_delta_chunks"] == 0
    assert P["capacity_room_next_chunk"]["capacity_error_chunks"] == 0
    assert P["capacity_same_chunk"]["capacity_error_chunks"] == 1
    assert P["alternate_600"]["tiles_of_one_key"] == 3
    sizes = [len(c) for c in R.by_name("sort_arms").chunks[2:]]
    assert sizes == [1, 255, 256, 257, 1024, 1025, 2049, 4097]
    for s in R.streams():  # the sizes stay small
        assert sum(len(c) for c in s.chunks) < 30_000 and s.log2 <= 14
    assert R.SL_SORT_WG == 1024 and R.SL_RES_TILE == 256


def test_remove_semantics_one_op_at_a_time():
    m = R.SkipListRemoveModel()
    T = R.TOMB
    resp, some = m.replay([(5, 50), (5, T), (5, T), (6, T), (7, 70), (7, 71), (7, T), (8, T), (8, 80)])
    assert resp.tolist() == [5, 50, 0, 0, 7, 7, 71, 0, 8] and some.tolist() == [1, 1, 0, 0, 1, 1, 1, 0, 1]
    assert m.items() == [(8, 80)] and m.get(5) is None and len(m) == 1
    GE, LT = R.L.NRG_SEEK_GE, R.L.NRG_SEEK_LT
    assert m.seek(0, GE) == (8, 80) and m.seek(8, LT) is None
    m.replay([(8, T)])
    assert len(m) == 0 and m.seek(0, GE) is None and m.digest() == (0, 0, 0)
    assert m.scan(0, GE, 4) == [] and m.scan(U64_MAX, R.L.NRG_SEEK_LE, 4) == []
    # another tombstone: 2^64 - 1 is then an ordinary value
    m = R.SkipListRemoveModel(tombstone=0)
    resp, some = m.replay([(1, U64_MAX), (1, 0), (1, 0)])
    assert resp.tolist() == [1, U64_MAX, 0] and some.tolist() == [1, 1, 0]


# ---- the library, without a device ---------------------------------------------------------------------
def test_null_handle_is_einval():
    import nrgpu
    from nrgpu import _lib as L

    lib = nrgpu.load()
    for s in ("nrg_skiplist_enable_removal", "nrg_skiplist_removal"):
        assert s in L.SIGNATURES and hasattr(lib, s)
    t, on = C.c_uint64(7), C.c_int(7)
    assert lib.nrg_skiplist_enable_removal(None, U64_MAX) == L.NRG_E_INVAL
    assert lib.nrg_skiplist_removal(None, C.byref(t), C.byref(on)) == L.NRG_E_INVAL
    assert lib.nrg_skiplist_removal(None, None, None) == L.NRG_E_INVAL
    assert (t.value, on.value) == (7, 7)


def test_header_declares_the_entry_points_and_names_what_is_missing():
    with open(os.path.join(ROOT, "include", "nrgpu.h")) as f:
        h = f.read()
    assert re.search(r"^int nrg_skiplist_enable_removal\(nrg_ctx\* ctx, uint64_t tombstone\);", h, re.M)
    assert re.search(r"^int nrg_skiplist_removal\(nrg_ctx\* ctx, uint64_t\* tombstone, int\* enabled\);", h, re.M)
    assert "no removal of keys (the" not in h
    for word in ("partitioned", "nrg_combiner_open", "pop_front"):
        assert word in h[h.index("---- Skip list:"):h.index("---- file store")]
    with open(os.path.join(ROOT, "README.md")) as f:
        readme = f.read()
    assert "no removal of keys" not in readme and "nrg_skiplist_enable_removal" in readme


def test_python_ops():
    import nrgpu

    r = nrgpu.SkipList.encode([nrgpu.SlPush(3, 4), nrgpu.SlRemove(3), nrgpu.SlRemove(9, tombstone=0)])
    assert r["key"].tolist() == [3, 3, 9] and r["val"].tolist() == [4, U64_MAX, 0]
    assert nrgpu.SkipList.decode([3, 4, 0], [1, 1, 0]) == [3, 4, None]


def test_drop_constants_match_the_source():
    with open(os.path.join(ROOT, "node-replication_amd", "csrc", "skiplist.hip")) as f:
        src = f.read()
    got = re.search(r"constexpr u32 SL_DROP_PART = (\d+);", src)
    assert got and int(got.group(1)) == R.SL_DROP_PART
    assert "SL_DROP_PART == SL_TPB * SL_DROP_ITEMS" in src
