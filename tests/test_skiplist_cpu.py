"""The replicated skip list without a device: the sequential model (tests/skiplist_model.py), the
library's ABI for the kind, and the constants the model mirrors from csrc/skiplist.hip."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import skiplist_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64_MAX = 2**64 - 1


@pytest.fixture(scope="module")
def nrgpu_mod():
    import nrgpu

    nrgpu.load()
    return nrgpu


def _modes(L):
    return L.NRG_SEEK_GE, L.NRG_SEEK_GT, L.NRG_SEEK_LE, L.NRG_SEEK_LT


# ---- the model -----------------------------------------------------------------------------------
def test_insert_replaces_and_answers_the_key():
    m = M.SkipListModel()
    resp, some = m.replay([(5, 50), (7, 70), (5, 51)])
    assert resp.tolist() == [5, 7, 5] and some.tolist() == [1, 1, 1]
    assert m.items() == [(5, 51), (7, 70)] and len(m) == 2 and m.get(5) == 51 and m.get(6) is None


def test_seek_on_empty_and_single_key_maps(nrgpu_mod):
    GE, GT, LE, LT = _modes(nrgpu_mod._lib)
    m = M.SkipListModel()
    for mode in (GE, GT, LE, LT):
        for k in (0, 1, U64_MAX):
            assert m.seek(k, mode) is None
    m.replay([(0, 9)])
    assert m.seek(0, GE) == (0, 9) and m.seek(0, LE) == (0, 9) and m.seek(0, GT) is None and m.seek(0, LT) is None
    assert m.seek(1, LT) == (0, 9) and m.seek(U64_MAX, LE) == (0, 9) and m.seek(1, GE) is None
    m = M.SkipListModel()
    m.replay([(U64_MAX, 3)])
    assert m.seek(U64_MAX, GE) == (U64_MAX, 3) and m.seek(U64_MAX, LE) == (U64_MAX, 3)
    assert m.seek(U64_MAX, GT) is None and m.seek(U64_MAX, LT) is None
    assert m.seek(0, GE) == (U64_MAX, 3) and m.seek(0, GT) == (U64_MAX, 3) and m.seek(0, LE) is None
    assert m.seek(U64_MAX - 1, GT) == (U64_MAX, 3) and m.seek(U64_MAX - 1, LT) is None


def test_seek_between_at_and_beyond_keys(nrgpu_mod):
    GE, GT, LE, LT = _modes(nrgpu_mod._lib)
    m = M.SkipListModel()
    m.replay([(10, 1), (20, 2), (30, 3)])
    assert m.seek(15, GE) == (20, 2) and m.seek(15, GT) == (20, 2) and m.seek(15, LE) == (10, 1) and m.seek(15, LT) == (10, 1)
    assert m.seek(20, GE) == (20, 2) and m.seek(20, GT) == (30, 3) and m.seek(20, LE) == (20, 2) and m.seek(20, LT) == (10, 1)
    assert m.seek(31, GE) is None and m.seek(30, GT) is None and m.seek(9, LE) is None and m.seek(10, LT) is None
    assert m.seek(0, GE) == (10, 1) and m.seek(U64_MAX, LE) == (30, 3)  # front and back


def test_range_and_range_count():
    m = M.SkipListModel()
    m.replay([(0, 1), (10, 2), (20, 3), (U64_MAX, 4)])
    assert m.range(11, 10) == [] and m.range_count(11, 10) == 0
    assert m.range(10, 10) == [(10, 2)] and m.range_count(10, 10) == 1 and m.range(11, 11) == []
    assert m.range(0, U64_MAX) == m.items() and m.range_count(0, U64_MAX) == 4
    assert m.range(1, U64_MAX - 1) == [(10, 2), (20, 3)] and m.range(20, U64_MAX) == [(20, 3), (U64_MAX, 4)]


def test_digest_is_the_hashmaps_for_the_same_pairs(nrgpu_mod):
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 500, 2000, dtype=np.uint64)
    vals = rng.integers(0, U64_MAX, 2000, dtype=np.uint64)
    m = M.SkipListModel()
    m.insert_many(keys.tolist(), vals.tolist())
    d = dict(zip(keys.tolist(), vals.tolist()))  # last wins
    assert m.digest() == nrgpu_mod.digest.pairs(list(d.keys()), list(d.values()))
    assert M.SkipListModel().digest() == (0, 0, 0)


def test_two_run_policy():
    m = M.SkipListModel(delta_max=4, max_batch=3)
    m.insert_many([1, 2, 3], [0, 0, 0])
    assert (m.nb, m.nd, m.compactions) == (0, 3, 0)
    m.insert_many([1, 2, 4], [9, 9, 9])  # one new key: nd = 4, not above delta_max
    assert (m.nb, m.nd, m.compactions) == (0, 4, 0)
    m.insert_many([5], [0])  # nd = 5 > 4
    assert (m.nb, m.nd, m.compactions) == (5, 0, 1)
    m.insert_many([6, 7, 8, 9, 10, 11], [0] * 6)  # two chunks of 3: 3, then 6 > 4
    assert (m.nb, m.nd, m.compactions) == (11, 0, 2)
    m.insert_many([1, 5, 9], [7, 7, 7])  # updates only
    assert (m.nb, m.nd, m.compactions) == (11, 0, 2) and m.get(5) == 7


# ---- the library, without a device ---------------------------------------------------------------
def test_kind_seek_modes_and_knob(nrgpu_mod):
    L = nrgpu_mod._lib
    assert L.NRG_DS_SKIPLIST == 6
    assert (L.NRG_SEEK_GE, L.NRG_SEEK_GT, L.NRG_SEEK_LE, L.NRG_SEEK_LT) == (0, 1, 2, 3)
    assert L.KNOBS["SL_DELTA_MAX"] == 20


def test_config_defaults(nrgpu_mod):
    L = nrgpu_mod._lib
    cfg = L.default_config(L.NRG_DS_SKIPLIST)
    other = L.default_config(L.NRG_DS_QUEUE)
    assert cfg.ds_kind == 6 and cfg.log2_slots == M.LOG2_DEFAULT == 24
    assert cfg.max_batch == other.max_batch == 1 << 20 and cfg.max_reads == other.max_reads
    assert cfg.log_bytes == other.log_bytes and cfg.pipeline == 0 and cfg.replica_id == 1
    assert C.sizeof(L.Config) == 88  # the struct keeps its size


SYMBOLS = ["round_async", "get", "get_async", "seek", "seek_async", "range", "range_count", "range_count_async",
           "dump", "len", "prefill", "prefill_range", "reserve", "capacity"]


def test_every_symbol_is_exported_and_rejects_a_null_handle(nrgpu_mod):
    L = nrgpu_mod._lib
    lib = nrgpu_mod.load()
    for s in SYMBOLS:
        assert "nrg_skiplist_" + s in L.SIGNATURES
        assert hasattr(lib, "nrg_skiplist_" + s)
    n = C.c_uint64()
    E = L.NRG_E_INVAL
    assert lib.nrg_skiplist_round_async(None, None, 0, 1, None, None) == E
    assert lib.nrg_skiplist_get(None, None, 0, None, None) == E
    assert lib.nrg_skiplist_get_async(None, None, 0, None, None) == E
    assert lib.nrg_skiplist_seek(None, None, 0, 0, None, None, None) == E
    assert lib.nrg_skiplist_seek_async(None, None, 0, 0, None, None, None) == E
    assert lib.nrg_skiplist_range(None, 0, 1, None, None, 0, C.byref(n)) == E
    assert lib.nrg_skiplist_range_count(None, None, None, 0, None) == E
    assert lib.nrg_skiplist_range_count_async(None, None, None, 0, None) == E
    assert lib.nrg_skiplist_dump(None, None, None, 0, C.byref(n)) == E
    assert lib.nrg_skiplist_len(None, C.byref(n)) == E
    assert lib.nrg_skiplist_prefill(None, None, None, 0) == E
    assert lib.nrg_skiplist_prefill_range(None, 0, 0) == E
    assert lib.nrg_skiplist_reserve(None, 1) == E
    assert lib.nrg_skiplist_capacity(None, C.byref(n)) == E


def test_snapshot_payload_is_16_bytes_per_item_in_key_order(nrgpu_mod):
    S, L = nrgpu_mod.snapshot, nrgpu_mod._lib
    for items in (0, 1, 3, 4, 1000):
        assert S.image_bytes(L.NRG_DS_SKIPLIST, items) == (64 + 16 * items + 63) & ~63
    img = S.pack(L.NRG_DS_SKIPLIST, {30: 3, 10: 1, U64_MAX: 9, 0: 5}, 77)
    info, (k, v) = S.unpack(img)
    assert info.ds_kind == 6 and info.items == 4 and info.log_idx == 77 and info.bytes == 128
    assert k.tolist() == [0, 10, 30, U64_MAX] and v.tolist() == [5, 1, 3, 9]
    assert info.digest == nrgpu_mod.digest.skiplist(k, v)


# ---- the constants the model mirrors ---------------------------------------------------------------
def test_tile_constants_match_the_source():
    src = open(os.path.join(ROOT, "node-replication_amd", "csrc", "skiplist.hip")).read()
    for name, val in M.TILE_CONSTANTS.items():
        got = re.search(r"constexpr \w+ %s = (\d+);" % name, src)
        assert got, f"skiplist.hip no longer defines {name}: revisit tests/skiplist_model.py"
        assert int(got.group(1)) == val, name
    m = re.search(r"SL_LOG2_MIN = (\d+), SL_LOG2_MAX = (\d+), SL_LOG2_DEFAULT = (\d+);", src)
    assert m and tuple(map(int, m.groups())) == (M.LOG2_MIN, M.LOG2_MAX, M.LOG2_DEFAULT)
    assert "SL_DELTA_DEFAULT = 1ull << 22;" in src and M.DELTA_DEFAULT == 1 << 22
    assert "SL_MERGE_PART == SL_TPB * SL_MERGE_ITEMS" in src
