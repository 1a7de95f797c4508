"""The hashmap Put streams (tests/hashmap_streams.py) without a device: the constants the host model
mirrors are pinned to the text of csrc/hashmap.hip and csrc/common.hpp, the round geometry is checked
against values written out by hand from hm_replay_chunk, every stream is checked for the property it
is named for, and the oracle is pinned against a Python dict on these shapes."""
import os
import re

import numpy as np
import pytest

import hashmap_streams as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64


def _src(name):
    return open(os.path.join(ROOT, "node-replication_amd", "csrc", name)).read()


# ---- the constants the model mirrors ---------------------------------------------------------------
def test_constants_match_the_source():
    hm, co = _src("hashmap.hip"), _src("common.hpp")
    assert f"constexpr int TPB = {S.TPB};" in hm
    assert f"constexpr u32 SM_W = {S.SM_W}, SM_R = {S.SM_R}, SM_HT = {S.SM_HT};" in hm
    assert "n <= c->hm.small_max && n <= SM_W && R <= SM_R" in hm
    assert f"static constexpr int C = PREV ? {S.PA_PREV_C} : {S.PA_C_PER_THREAD} * T;" in hm
    assert f"static constexpr int HT = {S.PA_HT_PER_C} * C;" in hm
    m = re.search(r"NB_LOG = T == 1024 \? (\d+) : T == 512 \? (\d+) : (\d+);", hm)
    assert m and {1024: int(m.group(1)), 512: int(m.group(2)), 256: int(m.group(3))} == S.PA_NB_LOG
    assert re.search(r"struct StampLds \{[^}]*static constexpr int HT = %d \* TILE;" % S.STAMP_HT_PER_TILE, hm)
    assert "constexpr u64 PART_MIN = 3ull << 17;" in hm and S.PART_MIN == 3 << 17
    assert "constexpr u64 PA_WIDE_MIN = 1ull << 16;" in hm and S.PA_WIDE_MIN == 1 << 16
    assert f"constexpr u32 HM_BK_MAX = {S.HM_BK_MAX};" in co
    m = re.search(r"const u32 K1 = n <= \(1u << (\d+)\) \? 1u : n <= \(1u << (\d+)\) \? 2u : n <= \(1u << (\d+)\) \? 4u : 8u;", hm)
    assert m and tuple(1 << int(g) for g in m.groups()) == S.TILE_THRESHOLDS
    assert "const u32 tile = TPB * K1;" in hm
    assert "while ((64ull << nb_log) < n && (1u << nb_log) < HM_BK_MAX) nb_log++;" in hm
    assert "if (nb_log > pa_nb_log) nb_log = pa_nb_log;" in hm and "if (nb_log > log2_slots) nb_log = log2_slots;" in hm
    assert "const u32 pa_t = want_prev ? 256u : c->hm.pa_tpb ? c->hm.pa_tpb : n >= PA_WIDE_MIN ? 512u : 256u;" in hm
    assert "ij.bk_shift = log2_slots - nb_log;" in hm
    assert "rec[q].key == EMPTY_KEY ? 0u : (u32)(table_home(rec[q].key, shift) >> j.bk_shift)" in hm  # the side key: bucket 0
    assert f"for (u32 s0 = 0; s0 < cn; s0 += {S.WALK})" in hm
    assert "if (n <= (1u << 18)) return 1u;" in hm and "return n >= 655360 && R >= n ? 4u : 2u;" in hm
    assert "constexpr u64 EMPTY_KEY = ~0ull;" in co and S.SIDE == 2**64 - 1
    for c in ("0xbf58476d1ce4e5b9ull", "0x94d049bb133111ebull", "z ^ (z >> 30)", "z ^ (z >> 27)", "z ^ (z >> 31)"):
        assert c in co
    assert "return mix64(key) >> shift;" in co
    assert "return ((((home >> 2) + (p >> 2)) << 2) | ((home + p) & 3)) & tmask;" in co


def test_mix64_matches_the_oracle(orc):
    ks = np.array([0, 1, 2, 12345, 2**63, 2**64 - 1], U64)
    assert [int(x) for x in S.mix64(ks)] == [orc.mix64(int(k)) for k in ks]


def test_probe_slot_examples_and_cover():
    ex = re.findall(r"probe_slot\((\d+), (\d+), (\d+)\) == (\d+)", _src("common.hpp"))
    assert len(ex) == 6
    for h, p, tmask, want in ex:
        assert S.probe_slot(int(h), int(p), int(tmask)) == int(want)
    for h in range(64):  # a 64-slot table: every slot once from every home, the first four in the home's group
        seq = [S.probe_slot(h, p, 63) for p in range(64)]
        assert sorted(seq) == list(range(64)) and all(s >> 2 == h >> 2 for s in seq[:4])


def test_place_follows_the_probe_sequence():
    ks = S.keys_with_home(lambda h: h == 62, 6, 6)
    assert S.place(ks, 6).tolist() == [62, 63, 60, 61, 2, 3]  # round the last group, then the first one
    table = {}
    S.place(S.keys_with_home(lambda h: h >= 0, 64, 6), 6, table)
    assert sorted(table) == list(range(64))
    assert S.place(S.keys_with_home(lambda h: h >= 0, 1, 6, skip=64), 6, table).tolist() == [-1]


# (n, log2_slots, want_prev, pa_tpb) -> (K1, tile, nb_log, bk_shift, C), by hand from hm_replay_chunk
GEOMETRY = [
    ((64, 12, False, 0), (1, 256, 0, 12, 1024)),
    ((64, 12, True, 0), (1, 256, 0, 12, 512)),
    ((65, 12, False, 0), (1, 256, 1, 11, 1024)),
    ((65, 12, True, 0), (1, 256, 1, 11, 512)),
    ((65, 12, False, 512), (1, 256, 1, 11, 2048)),
    ((65, 12, False, 1024), (1, 256, 1, 11, 4096)),
    ((1 << 14, 20, False, 0), (1, 256, 8, 12, 1024)),
    ((1 << 14, 20, True, 0), (1, 256, 8, 12, 512)),
    (((1 << 14) + 1, 20, False, 0), (2, 512, 9, 11, 1024)),
    (((1 << 14) + 1, 20, True, 0), (2, 512, 9, 11, 512)),
    (((1 << 14) + 1, 20, False, 1024), (2, 512, 8, 12, 4096)),
    ((1 << 16, 20, False, 0), (2, 512, 9, 11, 2048)),   # PA_WIDE_MIN: 512 threads, at most 512 buckets
    ((1 << 16, 20, False, 256), (2, 512, 10, 10, 1024)),
    ((1 << 16, 20, True, 0), (2, 512, 10, 10, 512)),
    (((1 << 16) + 1, 20, False, 0), (4, 1024, 9, 11, 2048)),
    (((1 << 16) + 1, 20, True, 0), (4, 1024, 10, 10, 512)),  # 64 << 10 = 2^16 < n, but HM_BK_MAX buckets
    (((1 << 16) + 1, 20, False, 1024), (4, 1024, 8, 12, 4096)),
    (((1 << 18) + 1, 20, False, 0), (8, 2048, 9, 11, 2048)),
    (((1 << 18) + 1, 20, True, 0), (8, 2048, 10, 10, 512)),
    (((1 << 18) + 1, 20, False, 256), (8, 2048, 10, 10, 1024)),
    (((1 << 18) + 1, 20, False, 512), (8, 2048, 9, 11, 2048)),
    (((1 << 18) + 1, 20, False, 1024), (8, 2048, 8, 12, 4096)),
    ((2000, 12, False, 0), (1, 256, 5, 7, 1024)),
    ((1600, 12, True, 0), (1, 256, 5, 7, 512)),
    ((100_000, 8, False, 0), (4, 1024, 8, 0, 2048)),     # never more buckets than slots
]


@pytest.mark.parametrize("args,want", GEOMETRY)
def test_round_geometry_at_the_thresholds(args, want):
    assert S.round_geometry(*args) == want


def test_stamp_k1_choice():
    assert [S.stamp_k1(n, R) for n, R in ((1 << 18, 0), ((1 << 18) + 1, 0), (655360, 655359), (655360, 655360))] == [1, 2, 2, 4]
    assert [S.stamp_k1(5, 0, k) for k in (1, 2, 3, 4)] == [1, 2, 2, 4]


# ---- every stream has the property it is named for ---------------------------------------------------
def _new_in(st, r):
    """Put keys of round r that no earlier round put."""
    before = np.concatenate([pk for pk, _, _ in st.rounds[:r]] + [np.zeros(0, U64)])
    return np.setdiff1d(st.rounds[r][0], before)


def test_the_catalogue_is_complete():
    names = S.names()
    assert len(set(names)) == len(names)
    for p in S.W_PATTERNS:
        sizes = [n for n in S.W_SIZES if f"w{n}_{p}" in names]
        assert sizes == [n for n in S.W_SIZES if p != "straddle" or n >= 63]  # (below 63 no straddle position exists)
    assert S.W_SIZES == (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049)


@pytest.mark.parametrize("name", S.w_names())
def test_w_streams(name):
    st = S.get(name)
    n, pattern, present = st.claims["n"], st.claims["pattern"], st.claims["present"]
    assert st.log2_slots == 12 and len(st.rounds) == 2
    assert len(st.rounds[0][0]) == 300 and len(np.unique(st.rounds[0][0])) == 300
    pk, _, gk = st.rounds[1]
    assert len(pk) == n
    u = np.unique(pk)
    assert set(u) | {int(k) + 1 for k in u if k != S.SIDE} | {S.SIDE} <= set(gk.tolist())
    is_present, is_side = np.isin(pk, present), pk == U64(S.SIDE)
    if pattern == "new":
        assert len(u) == n and not is_present.any() and not is_side.any()
    elif pattern == "equal":
        assert len(u) == 1 and not is_present.any() and not is_side.any()
    elif pattern == "twice":
        assert np.array_equal(pk[0:n - 1:2], pk[1:n:2]) and len(u) == (n + 1) // 2 and not is_present.any()
    elif pattern == "hits":
        assert is_present.all()
    elif pattern == "mix":
        i = np.arange(n)
        assert is_side[i % 3 == 2].all() and is_present[i % 3 == 1].all()
        assert not (is_present | is_side)[i % 3 == 0].any() and len(np.unique(pk[i % 3 == 0])) == (n + 2) // 3
    elif pattern == "side_ends":
        assert is_side[0] and is_side[n - 1] and is_present[1:n - 1].all() and len(np.unique(pk[1:n - 1])) <= 1
    elif pattern == "straddle":
        at = st.claims["straddle_at"]
        assert at == [p for p in (62, 63, 64, 254, 255, 256, 510, 511, 512, 1022, 1023, 1024) if p < n] and at
        key = pk[at[0]]
        assert np.array_equal(np.nonzero(pk == key)[0], at) and len(u) == n - len(at) + 1 and not is_present.any()
        for edge in (63, 255, 511, 1023):  # both sides of every edge the round reaches
            if edge + 1 < n:
                assert pk[edge] == key and pk[edge + 1] == key


@pytest.mark.parametrize("name", list(S.TILE_MIX))
def test_tile_mix_streams(name):
    st = S.get(name)
    n, tile = st.claims["n"], st.claims["tile"]
    assert (n, tile) in (((1 << 14) + 513, 512), ((1 << 16) + 1025, 1024), ((1 << 18) + 2049, 2048))
    assert S.round_geometry(n, 20, True)[1] == tile and st.log2_slots == 20 and len(st.rounds) == 1
    pk = st.rounds[0][0]
    assert len(pk) == n and pk[tile - 1] == pk[tile] and (pk == pk[tile]).sum() == 2
    i = np.arange(n)
    body = (i != tile - 1) & (i != tile)
    assert (pk[body & (i % 3 == 2)] == U64(S.SIDE)).all()
    first = {}
    for j, k in enumerate(pk.tolist()):
        first.setdefault(k, j)
    fresh = np.array([first[k] == j for j, k in enumerate(pk.tolist())])
    assert fresh[body & (i % 3 == 0)].all() and not fresh[body & (i % 3 == 1)].any()
    assert len(first) <= n // 2


def _chunk_step(p):
    return p // S.PA_PREV_C, p % S.PA_PREV_C // S.WALK


@pytest.mark.parametrize("name", ["prev_one_bucket", "prev_window"])
def test_prev_streams_sit_in_one_bucket_at_the_named_positions(name):
    st = S.get(name)
    _, _, nb_log, bk_shift, C = S.round_geometry(S.PREV_N, 12, True)
    assert (nb_log, C) == (5, 512)
    named, at = st.claims["named"], st.claims["at"]
    for pk, _, _ in st.rounds[1:]:
        assert len(pk) == 1600 and (S.bucket(pk, 12, bk_shift) == 0).all()  # 3 chunks of 512 and 64
    pk = st.rounds[1][0]
    for key, pos in at.items():
        k = S.SIDE if key == "side" else named[key]
        assert np.array_equal(np.nonzero(pk == U64(k))[0], pos), key
    assert at["edge"] == [0, 511, 512, 513, 1023, 1024, 1535, 1536, 1599] and at["side"] == [5]
    assert named["before"] in st.rounds[0][0] and _chunk_step(at["before"][0])[0] == 2
    assert named["claimed"] not in st.rounds[0][0]
    assert [_chunk_step(p)[0] for p in at["claimed"]] == [0, 2]
    assert {_chunk_step(p) for p in at["step"]} == {(1, 2)} and len(at["step"]) == 64
    assert [_chunk_step(p) for p in at["step1"]].count((1, 3)) == 64 and _chunk_step(at["step1"][-1]) == (1, 4)
    assert {_chunk_step(p) for p in at["alt0"] + at["alt1"]} == {(1, 5)}
    assert sorted(at["alt0"] + at["alt1"]) == list(range(832, 896)) and all(p % 2 == 0 for p in at["alt0"])
    new, old = _new_in(st, 1), np.intersect1d(st.rounds[1][0], st.rounds[0][0])
    assert len(new) > 60 and len(old) > 30  # claims and table values both feed the walk
    if name == "prev_one_bucket":
        a2 = st.claims["at_side_wins"]
        pk2 = st.rounds[2][0]
        assert np.array_equal(np.nonzero(pk2 == U64(S.SIDE))[0], [5, 511, 512, 1599]) and a2["side"] == [5, 511, 512, 1599]
        assert np.array_equal(np.nonzero(pk2 == named["edge"])[0], [0, 513, 1023, 1024, 1535, 1536])
        assert np.array_equal(st.rounds[3][0], pk[::-1]) and np.array_equal(st.rounds[4][0], pk2[::-1])
    else:
        assert st.window == [(0, 1600), (511, 513), (512, 1024), (600, 601), (1599, 1600)]


def test_dedup_tiles_has_pairs_inside_and_across_tiles():
    st = S.get("dedup_tiles")
    pk = st.rounds[0][0]
    assert len(pk) == 2000 and S.round_geometry(2000, 12, False)[1] == 256
    for a, b in st.claims["pairs"]["in_tile"]:
        assert pk[a] == pk[b] and a // 256 == b // 256 and (pk == pk[a]).sum() == 2
    assert [(a, b) for a, b in st.claims["pairs"]["across"]] == [(255, 256), (1023, 1024)]
    for a, b in st.claims["pairs"]["across"]:
        assert pk[a] == pk[b] and a // 256 + 1 == b // 256 and (pk == pk[a]).sum() == 2
    every = st.claims["every"]
    assert [p // 256 for p in every] == list(range(8)) and len(set(pk[every])) == 1 and (pk == pk[every[0]]).sum() == 8
    side = np.nonzero(pk == U64(S.SIDE))[0]
    assert side.tolist() == [400, 450, 767, 768]
    assert np.array_equal(st.rounds[1][0], pk[::-1])


@pytest.mark.parametrize("T", S.PA_WIDTHS)
def test_dedup_chunks_one_bucket_and_chunk_edges(T):
    st = S.get(f"dedup_chunks_{T}")
    c = st.claims
    pk = st.rounds[0][0]
    _, tile, nb_log, bk_shift, C = S.round_geometry(len(pk), 12, False, T)
    assert C == 4 * T == c["C"] and len(pk) == 3 * C - 64 and tile == 256
    assert (S.bucket(pk, 12, bk_shift) == c["bucket"]).all() and 0 < c["bucket"] < (1 << nb_log)
    for t0 in range(0, len(pk), 256):  # no duplicate inside an index tile: the dedup index keeps every Put
        assert len(np.unique(pk[t0:t0 + 256])) == len(pk[t0:t0 + 256])
    assert c["at"] == [C - 1, C, 2 * C] and (pk[c["at"]] == c["key"]).all()


@pytest.mark.parametrize("tile", S.STAMP_TILES)
def test_stamp_blocks_layout(tile):
    st = S.get(f"stamp_blocks_{tile}")
    c = st.claims
    pk = st.rounds[0][0]
    n = 4 * tile + 7
    assert len(pk) == n and n < S.PART_MIN
    assert (pk[:tile] == c["hot"]).all() and pk[n - 1] == c["hot"]
    lo, hi = c["distinct"]
    assert (lo, hi) == (tile, 2 * tile)
    slots = S.place(pk[lo:hi], 12)
    assert len(np.unique(slots)) == tile == len(np.unique(pk[lo:hi])) and (slots >= 0).all()
    assert tile * S.STAMP_HT_PER_TILE == 2 * tile  # the combine table at load 1 / 2
    b2 = pk[2 * tile:3 * tile]
    b2 = b2[(b2 != U64(S.SIDE)) & (b2 != c["once"])]
    assert len(b2) == tile - 2 and (S.home(b2, 12) >> U64(2) == U64(c["group"])).all()
    once = np.nonzero(pk == c["once"])[0]
    assert sorted(int(p) // tile for p in once) == [1, 2, 3, 4]
    side = np.nonzero(pk == U64(S.SIDE))[0]
    assert side.tolist() == c["side"] and len({int(p) // tile for p in side}) == 2
    again = np.isin(pk[3 * tile:4 * tile], pk[lo:hi])  # block 3 takes the stamps of block 1's keys
    assert again.sum() >= tile - 2
    assert np.array_equal(st.rounds[1][0], pk[::-1])


@pytest.mark.parametrize("homes", S.FULL_HOMES)
def test_full_streams_fill_every_slot(homes):
    st = S.get(f"full_{homes}")
    keys, extra = st.claims["keys"], st.claims["extra"]
    assert st.log2_slots == 8 and len(np.unique(keys)) == 256 and extra not in keys
    assert [len(_new_in(st, r)) for r in range(6)] == [100, 100, 57, 0, 1, 0]  # (57: 56 keys and the side key)
    assert len(st.rounds[2][0]) == 101 and S.SIDE in st.rounds[2][0]
    assert np.array_equal(st.rounds[3][0], keys[::-1]) and st.rounds[4][0].tolist() == [extra] and st.refused == {4: [0]}
    assert set(st.rounds[5][0].tolist()) == set(keys.tolist()) | {S.SIDE}
    table, order = {}, np.concatenate([pk[pk != U64(S.SIDE)] for pk, _, _ in st.rounds[:4]])
    _, first = np.unique(order, return_index=True)
    order = order[np.sort(first)]
    slots = S.place(order, 8, table)
    assert sorted(table) == list(range(256)) and (slots >= 0).all()
    assert S.place(np.array([extra], U64), 8, table).tolist() == [-1]
    h = S.home(order, 8).astype(np.int64)
    chain = ((slots >> 2) - (h >> 2)) % 64 * 4 + 4  # slots of the probe sequence up to the key's group
    if homes == "last_group":
        assert (h >= 252).all() and chain.max() >= 250
    elif homes == "one_slot":
        assert len(set(h.tolist())) == 1 and chain.max() == 256
    for r, (pk, _, gk) in enumerate(st.rounds):
        sofar = np.unique(np.concatenate([p for p, _, _ in st.rounds[:min(r, 3) + 1]]))
        assert set(sofar.tolist()) <= set(gk.tolist()) and len(gk) >= 2 * len(sofar)


def test_border_race_chains_cross_their_borders():
    st = S.get("border_race")
    c = st.claims
    _, _, nb_log, bk_shift, _ = S.round_geometry(2000, 12, False)
    per, nb = 1 << bk_shift, 1 << nb_log
    assert per == c["per"] and c["borders"][-1] == (nb - 1, 0) and len(c["borders"]) == 3
    assert [len(pk) for pk, _, _ in st.rounds] == [600, 2000, 2000]
    table = {}
    S.place(st.rounds[0][0], 12, table)
    for r, cnt in ((1, 24), (2, 36)):
        new = _new_in(st, r)
        order = st.rounds[r][0][np.sort(np.unique(st.rounds[r][0], return_index=True)[1])]
        order = order[np.isin(order, new)]
        slots = dict(zip(order.tolist(), S.place(order, 12, table).tolist()))
        for (b, b1), over, first in zip(c["borders"], c["over"], c["first"]):
            ov, fi = over[:cnt], first[:cnt]
            assert np.isin(ov, st.rounds[r][0]).all() and np.isin(fi, st.rounds[r][0]).all()
            assert (S.home(ov, 12).astype(np.int64) >> 2 == (b * per + per - 4) >> 2).all()
            hf = S.home(fi, 12).astype(np.int64)
            assert ((hf >= b1 * per) & (hf < b1 * per + 24)).all()
            if r == 1:  # the chains of bucket b's keys end in bucket b + 1, among its own keys' groups
                crossed = [k for k in ov.tolist() if slots[k] >> bk_shift == b1]
                assert len(crossed) >= 16
                assert max(slots[k] for k in crossed) - b1 * per >= 16
    assert len(_new_in(st, 1)) == 6 * 24 and len(_new_in(st, 2)) == 6 * 12


def test_chain_handover_overflow_keys_sit_behind_an_empty_slot():
    st = S.get("chain_handover")
    sizes = [len(pk) for pk, _, _ in st.rounds]
    assert [n <= S.HANDOVER_SMALL for n in sizes] == [True, False, True, False] and max(sizes) <= S.SM_W
    table = {}
    for r, (pk, _, _) in enumerate(st.rounds):
        S.place(_new_in(st, r), 12, table)
    where = {k: s for s, k in table.items()}
    for hm, keys in zip(st.claims["homes"], st.claims["clusters"]):
        assert (S.home(keys, 12) == U64(hm)).all() and len(keys) == 6
        slots = [where[k] for k in keys.tolist()]
        g0, g1 = hm >> 2, ((hm >> 2) + 1) & 1023
        assert sorted(slots[:4]) == [4 * g0 + i for i in range(4)]  # the home group, full
        assert slots[4:] == [4 * g1 + (hm & 3), 4 * g1 + ((hm + 1) & 3)]  # then the home's offset of the next group
        assert 4 * g1 + ((hm + 3) & 3) not in table and 4 * g1 + ((hm + 2) & 3) not in table
    assert {hm & 3 for hm in st.claims["homes"]} == {0, 1, 2, 3} and st.claims["homes"][-1] >> 2 == 1023
    first_small, first_large = set(st.rounds[0][0].tolist()), set(_new_in(st, 1).tolist())
    assert first_small <= set(st.rounds[1][0].tolist())  # a large round finds what a small one placed
    assert set(np.concatenate(st.claims["clusters"][4:]).tolist()) <= first_large & set(st.rounds[2][0].tolist())  # and back


# ---- the oracle on these shapes, against a dict -------------------------------------------------------
def _dict_replay(d, pk, pv):
    prev, found = np.zeros(len(pk), U64), np.zeros(len(pk), np.uint8)
    for i, (k, v) in enumerate(zip(pk.tolist(), pv.tolist())):
        if k in d:
            prev[i], found[i] = d[k], 1
        d[k] = v
    return prev, found


@pytest.mark.parametrize("name", S.names())
def test_oracle_matches_a_dict_and_sizes_are_bounded(orc, name):
    st = S.get(name)
    assert st.ops() <= S.MAX_OPS or name in S.LARGE
    assert st.log2_slots <= 12 or name in S.LARGE
    om, d, allv = orc.HashMap(), {}, []
    for pk, pv, gk in st.rounds:
        allv.append(pv)
        oprev, of = om.replay(pk, pv)
        dprev, df = _dict_replay(d, pk, pv)
        np.testing.assert_array_equal(of, df)
        np.testing.assert_array_equal(oprev, dprev)
        gv, gf = om.get_batch(gk)
        np.testing.assert_array_equal(gf, np.array([k in d for k in gk.tolist()], np.uint8))
        np.testing.assert_array_equal(gv, np.array([d.get(k, 0) for k in gk.tolist()], U64))
    allv = np.concatenate(allv)
    assert len(np.unique(allv)) == len(allv)  # a wrong previous value cannot pass by coincidence
    ok, ov = om.dump_sorted()
    assert len(om) == len(d) and ok.tolist() == sorted(d) and ov.tolist() == [d[k] for k in sorted(d)]
