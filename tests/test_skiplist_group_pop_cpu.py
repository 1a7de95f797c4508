"""The group-wide pop without a device: the cut every member computes from the candidate lists alone
(tests/skiplist_group_pop_model.py cut(): the select step's rank formula) equals "sort the union, take
the ends" on every named stream, the model's pop run removes exactly that from every partition, every
stream has the property it is named for, and the new entry points answer a NULL handle and are declared
in the header (tests/test_abi.py then checks that every declared symbol is exported)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import skiplist_group_pop_model as GM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("G", GM.GS)
@pytest.mark.parametrize("name", GM.NAMES)
def test_the_cut_equals_sorting_the_union(name, G):
    s = GM.by_name(name)
    m = s.state(G)
    before = m.members(G)
    reqs = s.reqs(G, len(m.keys))
    assert len(reqs) == G
    F, Bk = GM.totals(reqs, len(m.keys))
    assert F + Bk <= len(m.keys)
    c_f, c_b, nf, nb = GM.cut(before, F, Bk)
    assert (c_f, c_b) == GM.cut_by_sorting(before, F, Bk)
    assert sum(c_f) == F and sum(c_b) == Bk
    assert nf == [min(F, len(k)) for k in before] and nb == [min(Bk, len(k)) for k in before]
    # the model's run, one pop at a time, takes exactly that from every partition: a prefix and a suffix
    got = m.pop_run(reqs)
    assert sum(int(c.sum()) for c, _, _ in got) == F + Bk
    for o, (was, now) in enumerate(zip(before, m.members(G))):
        assert np.array_equal(now, was[c_f[o]:len(was) - c_b[o]]), (name, G, o)
    for (cnt, ks, vs), mine in zip(got, reqs):
        assert len(cnt) == len(mine) and len(ks) == len(vs) == int(cnt.sum())
        at = 0
        for c, (n, back) in zip(cnt.tolist(), mine):  # each request's entries in the order popped
            part = ks[at:at + c].astype(object)
            assert c <= n and all((a > b) if back else (a < b) for a, b in zip(part[:-1], part[1:]))
            at += c


def test_the_named_properties_are_where_the_names_say():
    s = GM.by_name("single")
    assert [len(r) for r in s.reqs(3, 99)] == [1, 0, 0] and s.reqs(1, 99) == [[(1, 0)]]
    r = GM.by_name("ragged").reqs(8, 1500)
    assert sorted(len(x) for x in r) == [0, 0, 1, 1, 37, 37, 300, 300]
    flat = [q for x in r for q in x]
    assert {0, 1} <= {n for n, _ in flat} and {b for _, b in flat} == {0, 1}
    # cluster: the six smallest keys are partition 0's and live in both of its runs' rounds
    s = GM.by_name("cluster")
    m = s.state(3)
    F, Bk = GM.totals(s.reqs(3, len(m.keys)), len(m.keys))
    assert (F, Bk) == (6, 0) and GM.cut(m.members(3), F, Bk)[:2] == ([6, 0, 0], [0, 0, 0])
    (ka, _), (kb, _) = s.rounds(3)
    assert set(m.keys[:3]) <= set(ka.tolist()) and set(m.keys[3:6]) <= set(kb.tolist())
    for G in (3, 8):  # the first round goes to base on every member (delta_max 64), the second stays in delta
        own = GM.SM.key_owner(s.rounds(G)[0][0], G)
        assert np.bincount(own, minlength=G).min() > 64
        own = GM.SM.key_owner(s.rounds(G)[1][0], G)
        assert 0 < np.bincount(own, minlength=G).max() <= 64
    # wide: F = 3000 where the map has it, and a member contributes more than NRG_SCAN_MAX_LIMIT candidates
    s = GM.by_name("wide")
    for G in GM.GS:
        m = s.state(G)
        F, Bk = GM.totals(s.reqs(G, len(m.keys)), len(m.keys))
        assert F == min(3000, len(m.keys) - 7) and Bk == 7
        assert max(GM.cut(m.members(G), F, Bk)[2]) > GM.NRG_SCAN_MAX_LIMIT
        assert max(len(k) for k in m.members(G)) < 4096  # (a member's capacity in the GPU tests)
    # meet: fronts and backs ask for len + 1, so the last record is short and the map is empty afterwards
    s = GM.by_name("meet")
    for G in GM.GS:
        m = s.state(G)
        n = len(m.keys)
        reqs = s.reqs(G, n)
        asked = sum(c for x in reqs for c, _ in x)
        assert asked == n + 1 and sum(GM.totals(reqs, n)) == n
        got = m.pop_run(reqs)
        assert got[G - 1][0].tolist()[-1] == 2 and len(m.keys) == 0
        assert all(c.sum() == 0 for c, _, _ in m.pop_run([[(1, 0), (1, 1)] for _ in range(G)]))
    s = GM.by_name("empty_member")
    for G in (3, 8):
        mem = s.state(G).members(G)
        assert len(mem[G - 1]) == 0 and min(len(k) for k in mem[:G - 1]) > 40
    assert len(s.state(1).keys) == 0
    s = GM.by_name("marks_as_values")
    m = s.state(3)
    vals = np.concatenate([v for _, _, v in m.pop_run(s.reqs(3, len(m.keys)))])
    assert GM.FRONT in vals and GM.BACK in vals and not s.enable_first
    s = GM.by_name("cap")
    for G in GM.GS:
        rank, cap = s.cap(G)
        m = s.state(G)
        got = m.pop_run(s.reqs(G, len(m.keys)))
        assert 0 <= rank < G and int(got[rank][0].sum()) > cap > 20  # the cut falls inside the second request
    for s in GM.STREAMS:  # the sizes stay small
        for G in GM.GS:
            assert s.prefill(G) <= 10_400 and sum(len(k) for k, _ in s.rounds(G)) < 1100
            assert all(len(k) <= 2048 for k, _ in s.rounds(G))


def test_union_model_semantics_one_op_at_a_time():
    m = GM.UnionModel(tombstone=GM.TOMB)
    resp, some = m.replay([(5, 50), (3, 30), (5, GM.TOMB), (5, GM.TOMB), (9, 90), (3, 31), (7, GM.TOMB)])
    assert resp.tolist() == [5, 3, 50, 0, 9, 3, 0] and some.tolist() == [1, 1, 1, 0, 1, 1, 0]
    assert m.items() == [(3, 31), (9, 90)]
    m = GM.UnionModel()  # without removal the tombstone is a value
    m.replay([(1, GM.TOMB), (2, 20), (4, 40), (8, 80)])
    got = m.pop_run([[(1, 0), (0, 1)], [], [(2, 1), (5, 0)]])
    assert [g[0].tolist() for g in got] == [[1, 0], [], [2, 1]]
    assert got[0][1].tolist() == [1] and got[0][2].tolist() == [GM.TOMB]
    assert got[2][1].tolist() == [8, 4, 2] and len(m.keys) == 0


# ---- the library, without a device ---------------------------------------------------------------------
NEW = ["nrg_group_skiplist_enable_removal", "nrg_group_skiplist_enable_pops", "nrg_group_skiplist_pop"]


def test_null_handle_is_einval():
    import nrgpu
    from nrgpu import _lib as L

    lib = nrgpu.load()
    for s in NEW:
        assert s in L.SIGNATURES and hasattr(lib, s)
    assert lib.nrg_group_skiplist_enable_removal(None, GM.TOMB) == L.NRG_E_INVAL
    assert lib.nrg_group_skiplist_enable_pops(None, GM.FRONT, GM.BACK) == L.NRG_E_INVAL
    q = L.Pops()
    assert lib.nrg_group_skiplist_pop(None, C.byref(q)) == L.NRG_E_INVAL
    assert C.sizeof(L.PopReq) == 16 and C.sizeof(L.Pops) == 64


def test_header_and_documents_name_the_calls():
    with open(os.path.join(ROOT, "include", "nrgpu.h")) as f:
        h = f.read()
    assert re.search(r"^int nrg_group_skiplist_enable_removal\(nrg_group\* g, uint64_t tombstone\);", h, re.M)
    assert re.search(r"^int nrg_group_skiplist_enable_pops\(nrg_group\* g, uint64_t front_mark, uint64_t back_mark\);", h, re.M)
    assert re.search(r"^int nrg_group_skiplist_pop\(nrg_group\* g, const nrg_pops\* pops\);", h, re.M)
    assert h.count("unless the group agreed on it") >= 3
    for doc in ("README.md", "DESIGN.md"):
        with open(os.path.join(ROOT, doc)) as f:
            text = f.read()
        assert all(s in text for s in NEW), doc
    with open(os.path.join(ROOT, "README.md")) as f:
        assert "Still missing: removal and pops in partitioned rounds" not in f.read()


def test_python_methods_exist():
    from nrgpu.parallel import PartitionedGroup

    for name in ("enable_removal", "enable_pops", "pop", "pop_front", "pop_back"):
        assert callable(getattr(PartitionedGroup, name))
