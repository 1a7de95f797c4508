"""The sequential model of tests/hashmap_remove_model.py against a plain dict, and every named stream
against the arm it is named for, counted from the records and the geometry model of
tests/hashmap_streams.py alone. No GPU and no library."""
import numpy as np
import pytest

import hashmap_remove_model as R
import hashmap_streams as S

U64 = np.uint64


def _plain(st):
    """The stream through a plain dict: every response, and the arm of every record. `slotted` is the
    set of keys ever put (no stream here rehashes, so a key put once holds a slot from then on)."""
    d, slotted = {}, set()
    arms = dict(claim=0, revive=0, die=0, remove_dead=0, remove_absent=0, overwrite=0)
    out = []
    for recs, gets in st.rounds:
        prev, found = [], []
        for k, v in zip(recs["key"].tolist(), recs["val"].tolist()):
            p = d.get(k)
            if v == st.tomb:
                arms["die" if p is not None else "remove_dead" if k in slotted else "remove_absent"] += 1
                d.pop(k, None)
            else:
                arms["overwrite" if p is not None else "revive" if k in slotted else "claim"] += 1
                d[k] = v
                slotted.add(k)
            prev.append(p or 0)
            found.append(int(p is not None))
        out.append((prev, found, [d.get(k, 0) for k in gets.tolist()], [int(k in d) for k in gets.tolist()]))
    return d, slotted, arms, out


@pytest.mark.parametrize("name", R.NAMES)
def test_model_is_a_dict(name):
    st = R.by_name(name)
    d, slotted, arms, out = _plain(st)
    for max_batch in (None, 500):
        m = st.model(max_batch)
        for (recs, gets), (prev, found, gv, gf) in zip(st.rounds, out):
            p, f = m.replay(recs)
            assert p.tolist() == prev and f.tolist() == found
            v, g = m.get_batch(gets)
            assert v.tolist() == gv and g.tolist() == gf
        assert m.map == d and m.occupancy == len(slotted) and m.arms == arms and m.full == 0
        k, v = m.arrays()
        assert m.digest()[0] == len(d) and dict(zip(k.tolist(), v.tolist())) == d
    assert not any(v in (R.TOMB, R.OTHER_TOMB) for v in d.values())


def test_digest_is_the_library_definition():
    from nrgpu import digest

    m = R.by_name("revival").model()
    for recs, _ in R.by_name("revival").rounds:
        m.replay(recs)
    assert m.digest() == digest.pairs(*m.arrays())


def _arms(name):
    return _plain(R.by_name(name))[2]


def test_present_absent_dead_reaches_every_remove_arm():
    st = R.by_name("present_absent_dead")
    a = _arms(st.name)
    assert a["die"] >= 60 and a["remove_absent"] >= 50 and a["remove_dead"] >= 60 and a["claim"] == 160
    recs = st.rounds[1][0]
    k, rm = recs["key"], recs["val"] == st.tomb
    twice = st.claims["a"][30:40]
    for x in twice:  # removed twice in one chunk
        assert rm[k == x].tolist() == [True, True]
    created = st.claims["b"][:20]
    for x in created:  # put and removed in one chunk
        assert rm[k == x].tolist() == [False, True]


def test_never_claims_would_fill_the_table():
    st = R.by_name("never_claims")
    assert st.max_log2 == 0 and st.log2_slots == 8
    gone = np.concatenate([r["key"] for r, _ in st.rounds[1:]])
    assert len(np.unique(gone)) == 5000 and len(st.rounds) >= 4  # several chunks
    assert all((r["val"] == st.tomb).all() for r, _ in st.rounds[1:])
    assert not np.isin(gone, st.claims["live"]).any()
    assert 5000 > (1 << 8) - 100  # a claim per Remove would run out of slots
    m = st.model()
    for recs, _ in st.rounds:
        m.replay(recs)
    assert m.occupancy == len(m) == 100 and m.full == 0


def test_in_chunk_order_patterns():
    st = R.by_name("in_chunk_order")
    d, slotted, arms, out = _plain(st)
    new = st.claims["new"]
    assert np.isin(new, list(slotted)).all() and not any(k in d for k in new.tolist())  # occupancy + 1, size + 0
    recs = st.rounds[2][0]
    prev, found = out[2][0], out[2][1]
    assert (recs["val"][:20] == st.tomb).all() and found[:20] == [1] * 20 and found[20:] == [0] * 20
    for r in (3, 4):
        recs = st.rounds[r][0]
        assert len(recs) == 600 and len(np.unique(recs["key"])) == 1
        rm = recs["val"] == st.tomb
        assert (rm[1:] != rm[:-1]).all()  # alternating: more than one chunk of 512 and nine walk steps
    assert out[3][1] == [0] + [1, 0] * 299 + [1]   # Put answers None after a Remove, a Remove Some after a Put
    assert out[4][1][:3] == [0, 0, 1]              # the key is dead when round 4 starts with a Remove


def test_one_bucket_edges_layout():
    st = R.by_name("one_bucket_edges")
    recs = st.rounds[1][0]
    _, tile, nb_log, bk_shift, C = S.round_geometry(len(recs), st.log2_slots, True)
    assert (len(recs), C, bk_shift) == (S.PREV_N, S.PA_PREV_C, st.claims["bk_shift"])
    assert (S.bucket(recs["key"], st.log2_slots, bk_shift) == 0).all()  # position in the bucket = index
    assert -(-len(recs) // C) == 4
    at = np.flatnonzero(recs["key"] == st.claims["edge"])
    assert at.tolist() == list(R.EDGE_AT)
    rm = (recs["val"] == st.tomb)
    assert np.flatnonzero(rm[at]).tolist() == [R.EDGE_AT.index(p) for p in R.EDGE_REMOVE]
    for a, b in ((63, 64), (511, 512), (1023, 1024)):  # Removes on both sides of a step and of two chunk edges
        assert rm[a] and rm[b] and a // S.WALK != b // S.WALK
    assert 511 // C != 512 // C and 1023 // C != 1024 // C and rm[1599]
    assert 0.2 < rm.mean() < 0.4


def test_revival_reuses_slots():
    st = R.by_name("revival")
    d, slotted, arms, out = _plain(st)
    assert arms["revive"] == 120 and arms["claim"] == 200 and len(slotted) == 200
    assert out[2][1] == [0] * 60  # the reviving Puts answer None


@pytest.mark.parametrize("name", ["chain", "chain_wrap"])
def test_chain_fifth_key_lives_in_the_next_group(name):
    st = R.by_name(name)
    ks, g = st.claims["keys"], st.claims["group"]
    groups = 1 << (st.log2_slots - 2)
    assert (S.home(ks, st.log2_slots) >> U64(2) == g).all()
    m = st.model()
    for recs, _ in st.rounds[:5]:
        m.replay(recs)
    assert sorted(m.held[k] >> 2 for k in ks[:4].tolist()) == [g] * 4
    assert m.held[int(ks[4])] >> 2 == (g + 1) % groups
    if name == "chain_wrap":
        assert g == groups - 1  # the next group is the table's first
    for recs, _ in st.rounds[5:]:
        m.replay(recs)
    assert m.held[int(ks[5])] >> 2 == (g + 1) % groups and m.held[int(ks[6])] >> 2 == (g + 1) % groups
    assert m.occupancy == 7 and len(m) == 3
    assert (st.rounds[5][0]["val"] == st.tomb).all() and len(st.rounds[5][0]) == 4


def test_side_streams():
    for name, tomb in (("side_default", R.TOMB), ("side_other", R.OTHER_TOMB)):
        st = R.by_name(name)
        assert st.tomb == tomb
        a = _arms(name)
        side = [r["val"][r["key"] == U64(S.SIDE)] == U64(tomb) for r, _ in st.rounds]
        assert [x.tolist() for x in side[:4]] == [[False], [True], [True], [False]]  # Put, Remove, (dead), Put
        assert a["revive"] >= 2 and a["remove_dead"] >= 1 and a["die"] >= 2


def test_sizes():
    assert R.SIZES == (1, 63, 64, 65, 511, 512, 513, 2049)
    for n in R.SIZES:
        st = R.by_name(f"sizes_{n}")
        recs = st.rounds[2][0]
        assert len(recs) == n
        assert int((recs["val"] == st.tomb).sum()) == -(-n // 3)
        a1 = _arms(st.name)
        if n >= 511:  # the round itself meets live, dead and absent keys with both ops
            assert a1["remove_dead"] and a1["remove_absent"] and a1["die"] > 200 and a1["revive"] and a1["claim"] > 600


def _run(st, purge_every=0):
    m = st.model()
    for i, (recs, _) in enumerate(st.rounds):
        m.replay(recs)
        if purge_every and (i + 1) % purge_every == 0:
            m.purge()
    return m


def test_churn_policy():
    """hm_room on an enabled context, restated: a growing 2^8 table under 100-key churn purges and
    never grows; a fixed one fills with dead slots unless it is purged."""
    m = _run(R.churn(10))
    assert (m.log2, m.grows, m.full) == (8, 0, 0) and m.purges >= 10 and len(m) == 0
    m = _run(R.churn(0, rounds=4))
    assert m.full > 0 and m.purges == 0
    m = _run(R.churn(0, rounds=8, purge_every=8), purge_every=8)
    assert m.full == 0 and m.purges >= 4
    # whole rounds of 100 would grow: live + n = 200 keys do not fit 2^8 slots at the load limit
    assert R.slots_for(200) == 9 and R.slots_for(125) == 8 and R.slots_for(128) == 8 and R.slots_for(129) == 9


def test_full_exact_leaves_no_empty_slot():
    st = R.by_name("full_exact")
    m = st.model()
    for recs, _ in st.rounds[:4]:
        m.replay(recs)
    assert sorted(m.table) == list(range(256)) and m.occupancy == 256  # every slot taken
    arms0 = dict(m.arms)
    for recs, _ in st.rounds[4:]:
        m.replay(recs)
    a = {k: m.arms[k] - arms0[k] for k in m.arms}
    assert a["remove_absent"] == 30 + 10 + 10 and a["die"] == 40 and a["revive"] == 20 and a["remove_dead"] == 20
    assert a["claim"] == 0 and m.full == 0 and m.occupancy == 256 and len(m) == 256 - 40 + 20


def test_grow_with_dead_reaches_the_grow_branch():
    """both grows happen with dead slots present, and the bound afterwards is live + n"""
    st = R.grow_with_dead()
    m = st.model()
    seen = []
    for recs, _ in st.rounds:
        before = (m.log2, m.occupancy - len(m), len(m))
        m.replay(recs)
        if m.log2 != before[0]:
            seen.append((before, m.log2, m.keys_ub, len(recs)))
    assert [(b[0], b[1], l) for b, l, _, _ in seen] == [(8, 30, 9), (9, 50, 10)]
    assert all(ub == b[2] + n for b, _, ub, n in seen)  # keys_ub = live + n
    assert (m.grows, m.purges, m.full) == (2, 0, 0) and m.occupancy == len(m) + 10
