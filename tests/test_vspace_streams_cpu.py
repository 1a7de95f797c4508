"""The page-table streams reach the arms of csrc/vspace.hip they are named for (no GPU).

tests/vspace_streams.py builds the streams; plan() restates the replay's classification and counting
over the model. Here: the constants the streams mirror are still those of vspace.hip; every stream
at every size meets the condition that puts it into its arm (which path ran is what the GPU file
cannot see: a chunk replayed sequentially gives the same answers as one replayed in parallel); the
plan's flags agree with the definition; the capped replay agrees with the GPU file's deep-copying
one; and check_pool rejects what it is there to reject.
"""
import os
import re

import numpy as np
import pytest

import vspace_streams as S
from vspace_model import KB4, VSpaceModel

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "node-replication_amd", "csrc",
                   "vspace.hip")


@pytest.mark.parametrize("name,value", [("VS_TPB", 256), ("VS_ALLOC_TPB", 1024), ("VS_SEQ_TPB", 1024),
                                        ("VS_SEQ_SLICE", 4096), ("VS_MAXG", 513)])
def test_kernel_constants(name, value):
    src = open(HIP).read()
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, src)
    assert m, f"{name} not found in vspace.hip: revisit tests/vspace_streams.py"
    assert int(m.group(1)) == value == getattr(S, name), (
        f"{name} is now {m.group(1)}, the streams assume {value}: revisit the sizes of tests/vspace_streams.py "
        "(256-op dep tiles, ceil(n / 1024) ops per vs_alloc lane, 1024-op stretches, 4096-op launches)")


def test_max_batch_bound_and_dtype():
    src = re.sub(r"\s+", " ", open(HIP).read())
    assert "cf.max_batch > (1ull << 16)" in src and S.MAX_BATCH == 1 << 16
    assert "cfg->max_batch = 1u << 16;" in src
    import nrgpu

    assert S.OP_DTYPE == nrgpu.VSPACE_OP_DTYPE


def _plan(name, n):
    log2, setup, chunk = S.stream(name, n)
    m = VSpaceModel()
    for b in setup:
        _, _, s = m.replay(b)
        assert s.all(), "a setup op failed"
    return m, S.plan(m, chunk, 1 << log2), log2, chunk


def _fields_unique(chunk):
    assert len(np.unique(chunk["pbase"])) == len(chunk)
    assert set(np.unique(chunk["rights"]).tolist()) == set(range(1, 9)) and set(chunk["op"].tolist()) == {0, 1}


@pytest.mark.parametrize("name,n", S.CASES, ids=lambda v: str(v))
def test_stream_reaches_its_arm(name, n):
    m, p, log2, chunk = _plan(name, n)
    assert len(chunk) == n <= S.MAX_BATCH and log2 <= 16
    _fields_unique(chunk)
    tiles = -(-n // S.VS_TPB)
    first = p.flag.count(S.FIRST)
    later = p.flag.count(S.LATER)
    assert p.per_lane == -(-n // 1024) and (p.per_lane >= 2) == (n > 1024)
    if name not in ("tight_fit", "overflow") and n != S.MAX_BATCH:
        assert not p.fallback, "the stream is meant to replay in parallel"
    if name in ("independent", "independent_desc"):
        assert first == n and later == 0 and p.nlater == 0
        assert p.npt_total == n  # a PT each
        if name == "independent":
            assert p.n4 == 1 and p.npd == 1 + -(-(n - 100) // 512)
            assert p.pd_share == min(512, max(100, n - 100)) and p.pdpt_share == n
            assert p.pd_share >= 256 or n <= 256 + 100
        else:
            assert p.n4 == 5 and p.need4_words == {0, 1, 3, 7}
            assert p.pd_share >= min(256, n // 5 - 100)
            # rank order against log order: the first op of the log has the highest address
            assert int(chunk["vbase"][0]) == int(chunk["vbase"].max())
            assert (np.diff(chunk["vbase"].astype(np.int64) >> 21) < 0).all()
    elif name == "chain":
        assert first == 1 and later == n - 1 and p.flag[0] == S.FIRST
        assert p.stretches == -(-n // 1024) >= 2 or n < 1024
        assert p.slices == -(-n // 4096)
        a, b, s, left = S.replay_capped(m, chunk, 1 << log2)
        assert not left and s.tolist() == [1 - i % 2 for i in range(n)]  # success, failure, success, ...
        assert m.tables() == 4 and len(m.dump()[0]) == 1 + (n - 1) // 64 + 2 * ((n + 62) // 128)
    elif name == "far_dep":
        tgt = S.far_dep_targets(n)
        assert [i for i in range(n) if p.flag[i] == S.LATER] == sorted(tgt)
        assert all(p.near[i] == j for i, j in tgt.items())  # "overlaps only": the nearest is the target
        assert p.tile_dist == tiles - 1
        if tiles >= 2:
            assert p.tile_dist >= 1 and any(i // 256 - j // 256 == 1 for i, j in tgt.items())
        if n > 1024:
            assert p.stretches >= 2
        if n > 4096:
            assert p.slices >= 2
    elif name == "octets":
        assert first == n // 8 and later == n - first
        if n > 256:
            assert p.tile_dist >= 1
        assert p.stretches == -(-n // 1024) and p.slices == -(-n // 4096)
        assert p.pd_share >= min(256, n // 8 - 100)
        assert p.fallback == (n == S.MAX_BATCH)  # 2^14 tables hold the chunk, but not vs_alloc's bound
        if n == S.MAX_BATCH:
            assert log2 == 14 and p.bound > 1 << 14
    elif name in ("edges", "edges_inval"):
        assert p.tile_dist == (4 if n == 1100 else 1)
        assert (p.flag.count(S.INVALID) == 1) == (name == "edges_inval")
        lo = np.array([S.granules(int(r["vbase"]), int(r["len"])) for r in chunk])
        big = int(np.argmax(lo[:, 1] - lo[:, 0]))
        assert lo[big, 1] - lo[big, 0] + 1 == S.VS_MAXG and p.flag[big] == S.LATER and p.reach2[big] is False
        # its followers: first, middle and last granule are later ops, the granule after it is first wave
        tail = [i for i in range(n - 30, n) if lo[big, 0] <= lo[i, 0] <= lo[big, 1] + 1]
        assert [p.flag[i] for i in tail] == [S.LATER, S.LATER, S.LATER, S.FIRST]
        assert [p.near[i] for i in tail[:3]] == [big] * 3
    elif name == "cross_pd":
        ops = S.cross_pd_ops(n)
        assert all(p.flag[i] == S.FIRST for i in ops) and later == 0
        assert [p.reach2[i] for i in ops] == [True, True, True, True, True, False, True, False]
        assert [p.npt[i] for i in ops] == [2, 2, 2, 2, 2, 1, 1, 0]
        # new PDPTs: slots 21, 22, 23 (the op into slot 24 starts in 23), 25, 26 and the padding's
        assert p.n4 == 6
        a, b, s, left = S.replay_capped(m, chunk, 1 << log2)
        assert not left and [int(s[i]) for i in ops] == [1, 1, 1, 1, 1, 1, 1, 0]
    elif name in ("tight_fit", "overflow"):
        cap = 1 << log2
        assert p.fallback and later == 10 and p.stretches == -(-n // 1024) and p.slices == -(-n // 4096)
        # without the later ops' bound the first wave alone would be let through
        assert m.tables() + p.n4 + p.npd + p.npt_total <= cap
        a, b, s, left = S.replay_capped(m, chunk, cap)
        if name == "tight_fit":
            assert not left and m.tables() == cap and s.all()
        else:
            assert len(left) >= 1 and m.tables() <= cap
            kept_later = [i for i in range(left[0], n) if p.flag[i] == S.LATER and i not in left]
            assert len(kept_later) >= 1 and all(s[i] == 1 for i in kept_later)
            assert all(p.flag[i] == S.FIRST for i in left)
            assert (a[left] == chunk["vbase"][left]).all() and not s[left].any() and not b[left].any()
    if name not in ("chain", "cross_pd", "tight_fit", "overflow"):  # (those have replayed the chunk above)
        S.replay_capped(m, chunk, 1 << log2)
    assert m.tables() <= 1 << 14


@pytest.mark.parametrize("name,n", [c for c in S.CASES if c[1] <= 1100], ids=lambda v: str(v))
def test_plan_flags_match_the_definition(name, n):
    _, p, _, chunk = _plan(name, n)
    assert p.flag == S.brute_flags(chunk)


def test_plan_does_not_touch_the_model():
    log2, setup, chunk = S.stream("cross_pd", 300)
    m = VSpaceModel()
    for b in setup:
        m.replay(b)
    before = S.model_pool(m).copy()
    S.plan(m, chunk, 1 << log2)
    np.testing.assert_array_equal(S.model_pool(m), before)


def test_capped_replay_equals_the_deep_copying_one():
    import copy

    import nrgpu
    import test_gpu_vspace as G

    for name, (log2, more, rows) in G.EXHAUST.items():
        ok = G._recs(nrgpu, [(G.V0, 0x1000, 4 * KB4, G.M, 3), (2 * G.SLOT4, 0x9000, 2 * KB4, G.M, 3)] + more)
        m1 = VSpaceModel()
        m1.replay(ok)
        m2 = copy.deepcopy(m1)
        recs = G._recs(nrgpu, rows)
        a1, b1, s1, left_out = G._replay_capped(m1, recs, 1 << log2)
        a2, b2, s2, left = S.replay_capped(m2, recs, 1 << log2)
        assert s2.tolist() == G.EXHAUST_SOME[name] and len(left) == left_out, name
        for x, y in ((a1, a2), (b1, b2), (s1, s2), (S.model_pool(m1), S.model_pool(m2))):
            np.testing.assert_array_equal(x, y, err_msg=name)


def test_check_pool_accepts_the_model_and_rejects_aliases():
    log2, setup, chunk = S.stream("cross_pd", 300)
    m = VSpaceModel()
    for b in setup:
        m.replay(b)
    m.replay(chunk)
    pool = S.model_pool(m)
    level = S.check_pool(pool, m.tables())
    assert level[0] == 3 and sorted(set(level.tolist())) == [0, 1, 2, 3]
    # two PD slots that name one PT
    pd = max(np.flatnonzero(level == 1), key=lambda t: int((pool[t] & np.uint64(0x81) == np.uint64(1)).sum()))
    slots = np.flatnonzero(pool[pd] & np.uint64(0x81) == np.uint64(1))  # its PTs
    assert len(slots) >= 2
    bad = pool.copy()
    bad[pd, slots[1]] = bad[pd, slots[0]]
    with pytest.raises(AssertionError, match="referenced 2 times"):
        S.check_pool(bad, m.tables())
    # ... seen as a table nothing references when the walk is cut short of it
    bad = pool.copy()
    bad[pd, slots[1]] = 0
    with pytest.raises(AssertionError, match="referenced by nothing"):
        S.check_pool(bad, m.tables())
    # an index >= ntables
    bad = pool.copy()
    bad[pd, slots[0]] = np.uint64((m.tables() << 12) | 7)
    with pytest.raises(AssertionError, match="not in"):
        S.check_pool(bad, m.tables())
    # an entry that is not index << 12 | P|RW|US; the PML4 named by an entry
    bad = pool.copy()
    bad[pd, slots[0]] = np.uint64(int(bad[pd, slots[0]]) & ~2)
    with pytest.raises(AssertionError, match="is not index"):
        S.check_pool(bad, m.tables())
    bad = pool.copy()
    bad[pd, slots[0]] = np.uint64(7)
    with pytest.raises(AssertionError, match="not in"):
        S.check_pool(bad, m.tables())
