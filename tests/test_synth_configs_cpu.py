"""The synthetic structure's configuration matrix on the CPU (no GPU).

tests/synth_model.py holds a Python model of AbstractDataStructure written from its definition,
a restatement of the bucket replay's layout, and the named op streams that
tests/test_gpu_synthetic_configs.py replays on the GPU. Here: the layout's constants and the
eligibility rule are still those of csrc/synthetic.hip; the C oracle (what the GPU is judged by)
equals the model at every configuration of the matrix, not only at the defaults; every stream
reaches the kernel arm it is named for, by the model's indices and the layout restatement; and the
defaults with the suite's random stream reach none of them.
"""
import os
import re

import numpy as np
import pytest

import synth_model as S

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "node-replication_amd", "csrc",
                   "synthetic.hip")
MATRIX = S.matrix()
BY_NAME = {name: cfg for name, cfg, _ in MATRIX}
CASES = [(name, st) for name, _, streams in MATRIX for st in streams]
SORT_ONLY = {"hr17", f"span{S.MAX_ELIGIBLE_SPAN + 1}", "cw0_hw3", "cw9", "cw63_hw1"}


def _src():
    return re.sub(r"\s+", " ", open(HIP).read())


@pytest.mark.parametrize("name,value", [("SYB_SHIFT", 9), ("SYA_TPB", 512), ("SYA_OROUNDS", 4), ("SY_MAX_NB", 512),
                                        ("SY_MAX_HOT", 16), ("SY_MAX_TILES", 4096), ("SY_MAX_CW", 8),
                                        ("SY_B0_PARTS", 4), ("SYB_TPB", 512), ("SYB_PER", 10), ("SYF_PER", 10)])
def test_kernel_constants(name, value):
    m = re.search(r"constexpr [^;]*\b%s = (\d+)u?\b" % name, _src())
    assert m, f"{name} not found in synthetic.hip: revisit tests/synth_model.py"
    assert int(m.group(1)) == value, f"{name} is now {m.group(1)}, tests/synth_model.py assumes {value}"


def test_derived_constants_and_eligibility():
    src = _src()
    for text in ("SYB_WORDS = 1u << SYB_SHIFT;", "SYA_WAVES = SYA_TPB / 64,", "SYA_OPS = SYA_WAVES * SYA_OROUNDS * 64;",
                 "SYB_PASS = SYB_TPB * PER;",
                 # sy_bucket_words and sy_bucket_eligible, which bucket_words / bucket_eligible restate
                 "const u64 nbw = SY_MAX_NB - SY_B0_PARTS; return span > 1 ? (span - 1 + nbw - 1) / nbw : 1;",
                 "return cf.synth_cold_writes >= 1 && cf.synth_cold_writes <= SY_MAX_CW && cf.synth_hot_reads <= "
                 "SY_MAX_HOT && span <= 1 + (u64)(SY_MAX_NB - SY_B0_PARTS) * SYB_WORDS && cf.max_batch <= "
                 "(u64)SY_MAX_TILES * SYA_OPS;"):
        assert text in src, f"synthetic.hip no longer says `{text}`: revisit tests/synth_model.py"
    assert S.SYB_WORDS == 1 << 9 and S.SYA_OPS == 512 // 64 * 4 * 64 and S.SYA_WAVE_OPS == 4 * 64
    assert S.SYB_PASS == 512 * 10 and S.MAX_ELIGIBLE_SPAN == 260097
    assert S.ROUND_OPS == 3 * S.SYA_OPS + 77 and S.SYA_OPS < S.MAX_BATCH < S.ROUND_OPS


def test_layout_restatement():
    for span, W, NB in ((1, 1, 1), (2, 1, 2), (3, 1, 3), (509, 1, 509), (510, 2, 256), (4096, 9, 456), (49999, 99, 507),
                        (199998, 394, 509), (260097, 512, 509)):
        assert (S.bucket_words(span), S.num_buckets(span)) == (W, NB), span
        assert NB + S.SY_B0_PARTS - 1 <= S.SY_MAX_NB and W <= S.SYB_WORDS
        # every cold word has a bucket below NB and a word below W; the last word is in the last bucket
        for x in {0, 1, 2, W, W + 1, span - 2, span - 1} & set(range(span)):
            b = S.bucket_of(x, W)
            assert 0 <= b < NB and 0 <= S.word_in_bucket(x, W) < W
            assert x == 0 or 1 + (b - 1) * W + S.word_in_bucket(x, W) == x
        assert S.bucket_of(span - 1, W) == NB - 1
    assert all(p * p != 49999 and 49999 % p for p in range(2, 224))  # the matrix's prime span


def test_eligibility_verdicts():
    got = {name for name, cfg, _ in MATRIX if not S.bucket_eligible(cfg, S.MAX_BATCH)}
    assert got == SORT_ONLY
    assert len(MATRIX) - len(got) >= 30  # both verdicts occur
    assert not S.bucket_eligible(S.Cfg(), S.SY_MAX_TILES * S.SYA_OPS + 1) and S.bucket_eligible(S.Cfg(), 1 << 20)
    for name, cfg, _ in MATRIX:  # what nrg_open accepts
        assert 0 < cfg.hot_reads < cfg.n and 0 < cfg.hot_writes + cfg.cold_writes <= 64, name
    names = [name for name, _, _ in MATRIX]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("name,stream", CASES)
def test_oracle_against_model(orc, name, stream):
    """replay (every response), read and dump of the C oracle equal the model's"""
    cfg = BY_NAME[name]
    os_, mod = orc.Synthetic(*cfg), S.SynthModel(*cfg)
    for r, ops in enumerate(S.STREAMS[stream](cfg, 7, n=300)):
        np.testing.assert_array_equal(os_.replay(ops), mod.replay(ops), err_msg=f"round {r}")
        rd = S.reads(cfg, r, 40)
        np.testing.assert_array_equal(os_.read(rd), mod.read(rd), err_msg=f"reads after round {r}")
    np.testing.assert_array_equal(os_.dump(), mod.dump())


def test_model_from_the_definition():
    """the model on a case small enough to work out by hand: n = 5, hot_reads = 2, hot_writes = 3,
    cold_writes = 2 (span 3)"""
    m = S.SynthModel(5, 2, 2, 2, 3)
    # ReadWrite(tid 2, r1 2, r2 1): hot 1, 0, 1 -> words 0, 1 = 1, 3; cold 4 % 3 + 2 = 3 and 5 % 3 + 2 = 4: sum 3 + 4
    assert m.replay([(2, 2, 1, S.RW)])[0] == 7 and m.words == [1, 3, 2, 4, 5]
    # WriteOnly(tid 9, r1 1, r2 2^64 - 1): hot range wraps (empty); cold 9 % 3 + 2 = 2 and (9 - 1) % 3 + 2 = 4
    assert m.replay([(9, 1, S.M64, S.WO)])[0] == 0 and m.words == [1, 3, 9, 4, 9]
    # ReadOnly(tid 1, r1 2^64 - 1, r2 2): hot 0, 1, 0 -> 1 + 3 + 1; cold (2^64 - 1) % 3 = 0 -> word 2, then
    # 2^64 - 1 + 2 wraps to 1 -> word 3
    assert m.read([(1, S.M64, 2)])[0] == 5 + 9 + 4
    assert list(m.dump()) == [1, 3, 9, 4, 9]


@pytest.mark.parametrize("name", [n for n, _, st in MATRIX if "one_word" in st])
def test_one_word_fills_bucket_0(name):
    cfg = BY_NAME[name]
    rounds = S.one_word(cfg, 3)
    for ops in rounds[:2]:
        st = S.round_stats(cfg, ops)
        assert st["word0"] == len(ops) * cfg.cold_writes and st["buckets"] == {0}
        assert st["wave_max"] == S.SYA_WAVE_OPS * cfg.cold_writes and st["tile_max"] == S.SYA_OPS * cfg.cold_writes
    if cfg.cold_writes == 8:
        assert st["wave_max"] == 2048 and st["tile_max"] == 16384  # the packed fields' limits
        assert len(ops) * 8 > 9 * S.SYB_PASS  # several bucket passes
    assert not (rounds[0][:, 3] == S.WO).any() and (rounds[1][:, 3] == S.WO).any()


@pytest.mark.parametrize("name", [n for n, _, st in MATRIX if "sweep" in st])
def test_sweep_reaches_every_bucket(name):
    cfg = BY_NAME[name]
    W, NB = S.bucket_words(cfg.span), S.num_buckets(cfg.span)
    rounds = S.sweep(cfg, 11)
    st = S.round_stats(cfg, rounds[0])
    assert st["buckets"] == set(range(NB)) and cfg.span - 1 in st["words"] and 0 in st["words"]
    for b in range(1, NB):  # first and last word of every bucket
        assert 1 + (b - 1) * W in st["words"] and min(b * W, cfg.span - 1) in st["words"]
    if S.ROUND_OPS * cfg.cold_writes >= cfg.span + 2 * NB * cfg.cold_writes:
        assert st["words"] == set(range(cfg.span))
    assert (rounds[0][:, 3] == S.WO).all() and (rounds[1][:, 3] == S.RW).all()


@pytest.mark.parametrize("name", [n for n, _, st in MATRIX if "edges" in st])
def test_edges_wrap(name):
    cfg = BY_NAME[name]
    ops = S.edges(cfg, 5)[0]
    assert len({(int(a), int(b)) for a, b in ops[:, 1:3]}) == len(set(S.edge_values(cfg.span))) ** 2  # every pairing
    assert S.round_stats(cfg, ops)["wraps"] >= 1
    assert ((1 << 64) % cfg.span == 0) == (cfg.span & (cfg.span - 1) == 0)
    assert any(not S.hot_indices(cfg, int(r2)) for r2 in ops[:, 2])  # the wrapping hot range


def test_power_of_two_spans_are_the_wrap_controls():
    """2^64 mod span = 0 at spans 1, 2 and 4096: the stepped index needs no correction when the u64 sum
    wraps, so a replay without it is still right there, and wrong at every other span of the matrix"""
    spans = [cfg.span for name, cfg, _ in MATRIX if name.startswith("span")]
    assert sorted(s for s in spans if (1 << 64) % s == 0) == [1, 2, 4096]
    assert sorted(s for s in spans if (1 << 64) % s) == [3, 509, 510, 49999, S.MAX_ELIGIBLE_SPAN, S.MAX_ELIGIBLE_SPAN + 1]


@pytest.mark.parametrize("name", [n for n, _, st in MATRIX if "hot_repeat" in st])
def test_hot_repeat(name):
    cfg = BY_NAME[name]
    ops = S.hot_repeat(cfg, 9)[0]
    st = S.round_stats(cfg, ops)
    assert (st["hot_twice"] > 0) == (cfg.hot_writes > cfg.hot_reads)
    assert (st["hot_steps"] > 0) == (cfg.hot_writes >= 2)
    assert {int(r2) % cfg.hot_reads for r2 in ops[:, 2] if int(r2) < 1 << 63} == set(range(cfg.hot_reads))
    # per 64-op run: WriteOnly in the last lane only, WriteOnly followed by ReadWrites, both kinds lane by lane
    kinds = ops[: len(ops) // 64 * 64, 3].reshape(-1, 64)
    assert any(k[63] == S.WO and k[:63].all() for k in kinds)
    assert any(k[63] == S.RW and (k == S.WO).sum() == 1 for k in kinds)
    assert any((k[0::2] != k[1::2]).all() for k in kinds)
    tail = ops[-77:]  # ReadWrite only, a wrapping hot range among them
    assert (tail[:, 3] == S.RW).all()
    assert not cfg.hot_writes or any(not S.hot_indices(cfg, int(r2)) for r2 in tail[:, 2])
    if cfg.hot_writes > cfg.hot_reads:  # a WriteOnly that sets one hot word twice: the SET search's tie
        assert any(int(o[3]) == S.WO and len(set(S.hot_indices(cfg, int(o[2])))) < cfg.hot_writes for o in ops)


def test_wo_runs():
    ops0, ops1 = S.wo_runs(S.Cfg(), 1)[:2]
    wo = np.flatnonzero(ops0[:, 3] == S.WO)
    edges_ = np.flatnonzero(np.diff(wo) > 1)
    starts, ends = wo[np.r_[0, edges_ + 1]], wo[np.r_[edges_, len(wo) - 1]] + 1
    assert len(starts) == 4 and all(s % 64 and e % 64 for s, e in zip(starts, ends))
    assert any(s // S.SYA_OPS != (e - 1) // S.SYA_OPS for s, e in zip(starts, ends))  # a run across a tile edge
    assert any(s < S.MAX_BATCH <= e for s, e in zip(starts, ends))  # ... and across the chunk edge
    assert (ops0[wo, 0] >= 1 << 31).all() and (ops1[ops1[:, 3] == S.WO, 0] < 1 << 31).all()


def test_salt():
    for name, f in S.STREAMS.items():
        a, b = f(S.Cfg(hot_writes=3), 1), f(S.Cfg(hot_writes=3), 2)
        assert len(a) == 4 and all(x.shape == (S.ROUND_OPS, 4) for x in a), name
        assert any((x != y).any() for x, y in zip(a, b)), name


def test_defaults_with_random_reach_none_of_it():
    cfg = S.Cfg()
    assert tuple(cfg) == S.DEFAULTS
    st = S.round_stats(cfg, S.random(cfg, 1)[0])
    assert st["hot_twice"] == 0 and st["hot_steps"] == 0
    # the fullest bucket is cold word 0, with one touch per tid-0 op (a quarter of the ops): about 512
    # per tile and 64 per wave, against the 16384 and 2048 the packed fields are sized for
    assert st["tile_max"] < 1024 and st["wave_max"] < 256
    assert len(st["buckets"]) == S.num_buckets(cfg.span) and S.bucket_words(cfg.span) == 394  # one W, one NB
