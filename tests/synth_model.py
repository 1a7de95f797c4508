"""A sequential model of AbstractDataStructure (the reference's benches/synthetic.rs:60-195), a
restatement of the bucket replay's layout, and the named op streams of the configuration tests.

The model is written from the definition with Python ints, every u64 operation masked by hand
(release-build wrapping arithmetic): storage starts at words[i] = i; an op's hot range
r2 .. r2 + hot_writes is empty when the addition wraps, else it touches words (r2 + j) % hot_reads;
its cold touches are words (r1 * tid + k * r2 mod 2^64) % (n - hot_reads) + hot_reads. WriteOnly
sets every touched word to tid and answers 0; ReadWrite answers the sum of the cold words as read
and adds 1 to every touched word; ReadOnly sums hot_writes hot and cold_reads cold words.

The layout part restates, from the cold span alone, what csrc/synthetic.hip's partition computes:
cold word 0 alone in bucket 0, words 1.. in buckets of W = ceil((span - 1) / 508) words.
tests/test_synth_configs_cpu.py pins its constants against the source.

The streams are functions of (configuration, seed, ops per round) and return a list of rounds,
each an (n, 4) uint64 array of {tid, r1, r2, op} rows (op 0 = WriteOnly, 1 = ReadWrite). The
seed is a salt: it moves values, op kinds or the order, so memory left by another run cannot
pass as an answer.
"""
import numpy as np

M64 = (1 << 64) - 1
WO, RW = 0, 1
DEFAULTS = (200_000, 20, 5, 2, 1)  # n, cold_reads, cold_writes, hot_reads, hot_writes

# ---- csrc/synthetic.hip's layout constants -------------------------------------------------
SY_MAX_NB = 512
SY_B0_PARTS = 4
SYB_WORDS = 512
SYA_OPS = 2048  # ops per partition tile: 8 waves x 4 rounds x 64 lanes
SYA_WAVE_OPS = 256  # ops of one tile ranked by one wave
SY_MAX_HOT = 16
SY_MAX_CW = 8
SY_MAX_TILES = 4096
SYB_PASS = 512 * 10  # touches per bucket pass: SYB_TPB * SYB_PER
MAX_ELIGIBLE_SPAN = 1 + (SY_MAX_NB - SY_B0_PARTS) * SYB_WORDS  # 260097

ROUND_OPS = 3 * SYA_OPS + 77  # three tiles and a part


class Cfg(tuple):
    """(n, cold_reads, cold_writes, hot_reads, hot_writes)"""
    __slots__ = ()

    def __new__(cls, n=DEFAULTS[0], cold_reads=DEFAULTS[1], cold_writes=DEFAULTS[2], hot_reads=DEFAULTS[3],
                hot_writes=DEFAULTS[4]):
        return tuple.__new__(cls, (n, cold_reads, cold_writes, hot_reads, hot_writes))

    n = property(lambda s: s[0])
    cold_reads = property(lambda s: s[1])
    cold_writes = property(lambda s: s[2])
    hot_reads = property(lambda s: s[3])
    hot_writes = property(lambda s: s[4])
    span = property(lambda s: s[0] - s[3])

    def nrg(self, **more):
        """the nrg_config fields"""
        return dict(synth_n=self.n, synth_cold_reads=self.cold_reads, synth_cold_writes=self.cold_writes,
                    synth_hot_reads=self.hot_reads, synth_hot_writes=self.hot_writes, **more)


def with_span(span, **kw):
    c = Cfg(**kw)
    return Cfg(span + c.hot_reads, *c[1:])


# ---- the model ------------------------------------------------------------------------------
def hot_indices(cfg, r2):
    if ((r2 + cfg.hot_writes) & M64) < r2:  # `begin..end` with a wrapped end is empty
        return []
    return [(r2 + j) % cfg.hot_reads for j in range(cfg.hot_writes)]


def cold_indices(cfg, tid, r1, r2, count=None):
    span, hr = cfg.span, cfg.hot_reads
    begin = (r1 * tid) & M64
    out = []
    for _ in range(cfg.cold_writes if count is None else count):
        out.append(begin % span + hr)
        begin = (begin + r2) & M64
    return out


class SynthModel:
    def __init__(self, n=DEFAULTS[0], cold_reads=DEFAULTS[1], cold_writes=DEFAULTS[2], hot_reads=DEFAULTS[3],
                 hot_writes=DEFAULTS[4]):
        self.cfg = Cfg(n, cold_reads, cold_writes, hot_reads, hot_writes)
        assert 0 < hot_reads < n
        self.words = list(range(n))

    def replay(self, ops):
        cfg, w = self.cfg, self.words
        resp = np.zeros(len(ops), np.uint64)
        for i, row in enumerate(ops):
            tid, r1, r2, op = (int(v) for v in row)
            hot, cold = hot_indices(cfg, r2), cold_indices(cfg, tid, r1, r2)
            if op == WO:
                for x in hot:
                    w[x] = tid
                for x in cold:
                    w[x] = tid
            else:
                for x in hot:
                    w[x] = (w[x] + 1) & M64
                s = 0
                for x in cold:
                    s = (s + w[x]) & M64
                    w[x] = (w[x] + 1) & M64
                resp[i] = s
        return resp

    def read(self, rd):
        cfg, w = self.cfg, self.words
        out = np.zeros(len(rd), np.uint64)
        for i, row in enumerate(rd):
            tid, r1, r2 = (int(v) for v in row)
            s = 0
            for x in hot_indices(cfg, r2):
                s = (s + w[x]) & M64
            for x in cold_indices(cfg, tid, r1, r2, cfg.cold_reads):
                s = (s + w[x]) & M64
            out[i] = s
        return out

    def dump(self):
        return np.array(self.words, np.uint64)


# ---- the bucket layout, from the span --------------------------------------------------------
def bucket_words(span):
    """W: words per bucket from cold word 1 on"""
    nbw = SY_MAX_NB - SY_B0_PARTS
    return -(-(span - 1) // nbw) if span > 1 else 1


def num_buckets(span):
    return 1 + -(-(span - 1) // bucket_words(span))


def bucket_of(x, W):
    """bucket of cold word x (x relative to hot_reads)"""
    return 0 if x == 0 else 1 + (x - 1) // W


def word_in_bucket(x, W):
    return 0 if x == 0 else (x - 1) % W


def bucket_eligible(cfg, max_batch):
    """sy_bucket_eligible: the bucket replay takes the configuration, else the sort path does"""
    return (1 <= cfg.cold_writes <= SY_MAX_CW and cfg.hot_reads <= SY_MAX_HOT and cfg.span <= MAX_ELIGIBLE_SPAN
            and max_batch <= SY_MAX_TILES * SYA_OPS)


def round_stats(cfg, ops):
    """What one round does to the layout, from the model's indices alone: touches per cold word 0,
    the set of touched buckets and cold words, the largest count one wave (256 consecutive ops of
    a tile) and one tile (2048 ops) put into one bucket, the number of cold steps whose u64 sum
    wraps, ops that touch one hot word at least twice, and hot steps taken (j >= 1)."""
    W, hr = bucket_words(cfg.span), cfg.hot_reads
    st = dict(word0=0, buckets=set(), words=set(), wave_max=0, tile_max=0, wraps=0, hot_twice=0, hot_steps=0)
    wave, tile = {}, {}
    for i, row in enumerate(ops):
        tid, r1, r2, _ = (int(v) for v in row)
        if i % SYA_WAVE_OPS == 0:
            wave = {}
        if i % SYA_OPS == 0:
            tile = {}
        begin = (r1 * tid) & M64
        for k, x in enumerate(cold_indices(cfg, tid, r1, r2)):
            x -= hr
            b = bucket_of(x, W)
            st["word0"] += x == 0
            st["buckets"].add(b)
            st["words"].add(x)
            wave[b] = wave.get(b, 0) + 1
            tile[b] = tile.get(b, 0) + 1
            st["wave_max"] = max(st["wave_max"], wave[b])
            st["tile_max"] = max(st["tile_max"], tile[b])
            st["wraps"] += k + 1 < cfg.cold_writes and begin + r2 > M64  # a wrap the next index depends on
            begin = (begin + r2) & M64
        hot = hot_indices(cfg, r2)
        st["hot_twice"] += len(set(hot)) < len(hot)
        st["hot_steps"] += max(len(hot) - 1, 0)
    return st


# ---- streams ----------------------------------------------------------------------------------
def sm64(seed, n):
    """n splitmix64 outputs of stream `seed`"""
    with np.errstate(over="ignore"):
        z = (np.arange(1, n + 1, dtype=np.uint64) + np.uint64(seed & M64)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _rows(tid, r1, r2, op, n):
    a = np.zeros((n, 4), np.uint64)
    a[:, 0], a[:, 1], a[:, 2], a[:, 3] = tid, r1, r2, op
    return a


def random(cfg, seed, n=ROUND_OPS, rounds=4, wo=10, tids=(0, 1, 5, 63)):
    """full-range r1 and r2, tids from a small set with 0 in it, `wo` percent WriteOnly"""
    out = []
    for r in range(rounds):
        raw = sm64(seed * 1000 + r, 4 * n)
        out.append(_rows(np.asarray(tids, np.uint64)[raw[0::4] % np.uint64(len(tids))], raw[1::4], raw[2::4],
                         (raw[3::4] % np.uint64(100) >= np.uint64(wo)).astype(np.uint64), n))
    return out


def random30(cfg, seed, n=ROUND_OPS, rounds=4):
    return random(cfg, seed, n, rounds, wo=30, tids=(0, 2, 9, 31))


def one_word(cfg, seed, n=ROUND_OPS, rounds=4):
    """r1 * tid = 0 and r2 = 0: every cold touch of every op lands on cold word 0, every hot touch
    on words j % hot_reads. ReadWrite ops have tid 0; rounds 1 and 3 hold a few WriteOnly ops (which
    put bucket 0 back into one workgroup), with a salted tid and r1 = 0 in round 3."""
    out = []
    for r in range(rounds):
        raw = sm64(seed * 1000 + 100 + r, 2 * n)
        a = _rows(0, raw[0::2], 0, RW, n)
        if r & 1:
            w = raw[1::2] % np.uint64(29) == 0
            a[w, 3] = WO
            if r == 3:
                a[w, 0] = np.uint64(2 + seed % 1000)
                a[w, 1] = 0
        out.append(a)
    return out


def sweep(cfg, seed, n=ROUND_OPS, rounds=4):
    """tid = 1, r2 = 1: op i touches cold words r1 .. r1 + CW - 1 (mod span). Cold word 0, the
    first and the last word of every bucket (the last of them is the last word of the storage)
    start an op each, and the rest of the round walks on with r1 = start + CW * i, which is
    every cold word when n * CW reaches the span. Round 0 is WriteOnly, round 1 ReadWrite, then
    the kinds alternate op by op; the seed rotates the order and moves the walk's start."""
    span, W, cw = cfg.span, bucket_words(cfg.span), max(cfg.cold_writes, 1)
    starts = [0]
    for b in range(1, num_buckets(span)):
        starts += [1 + (b - 1) * W, min(b * W, span - 1)]
    starts = starts[:n]
    off = seed % span
    walk = [(off + cw * i) % span for i in range(n - len(starts))]
    r1 = np.array(starts + walk, np.uint64)
    out = []
    for r in range(rounds):
        kind = WO if r == 0 else RW if r == 1 else (np.arange(n) + r + seed) % 2
        out.append(np.roll(_rows(1, r1, 1, kind, n), (seed + 17 * r) % n, axis=0))
    return out


def edge_values(span):
    return [v & M64 for v in (0, 1, span - 1, span, span + 1, 2 * span - 1, 1 << 63, (1 << 64) - span, (1 << 64) - 2,
                              (1 << 64) - 1)]


def edges(cfg, seed, n=ROUND_OPS, rounds=4):
    """tid = 1, r1 and r2 from edge_values(span) in every pairing (100 pairs, repeated to the round's
    length): reciprocal quotient estimates low by one and by two, the wrapping hot range, and a
    u64 wrap at every cold step. A fifth of the ops are WriteOnly, by the seed."""
    ev = np.array(edge_values(cfg.span), np.uint64)
    i = np.arange(n)
    out = []
    for r in range(rounds):
        raw = sm64(seed * 1000 + 200 + r, n)
        j = (i + seed + 7 * r) % 100
        out.append(_rows(1, ev[j // 10], ev[j % 10], (raw % np.uint64(5) != 0).astype(np.uint64), n))
    return out


def hot_repeat(cfg, seed, n=ROUND_OPS, rounds=4):
    """For hot_writes > hot_reads (an op then touches a hot word more than once). r2 = m * hot_reads + i
    takes every residue; one op in 50 has an r2 whose hot range wraps. The kinds go by 64-op run
    (a wave round): run % 4 = 0 alternates WriteOnly and ReadWrite lane by lane, 1 has its only
    WriteOnly in the last lane, 2 has one mid-run followed by ReadWrites, 3 is ReadWrite
    only; the seed shifts the pattern by whole runs and picks the tids. The round's last 77 ops (its
    partial tile) are ReadWrite with a wrapping r2 among them, so no later SET covers what the
    hot words took from them."""
    tids = np.array([0, 1, 5, 63, 2 + seed % 1000], np.uint64)
    i = np.arange(n)
    lane, run = i % 64, (i // 64 + seed) % 4
    out = []
    for r in range(rounds):
        raw = sm64(seed * 1000 + 300 + r, 3 * n)
        r2 = (raw[0::3] % np.uint64(1 << 32)) * np.uint64(cfg.hot_reads) + (i % cfg.hot_reads).astype(np.uint64)
        wr = (i + r) % 50 == 49  # r2 > 2^64 - 1 - hot_writes: the hot range wraps
        r2[wr] = np.uint64(M64) - (i[wr] % min(3, max(cfg.hot_writes, 1))).astype(np.uint64)
        kind = np.where(run == 0, (lane + r) % 2, np.where(run == 1, lane != 63, np.where(run == 2, lane != 20 + r, 1)))
        kind[n - min(77, n // 4):] = RW
        out.append(_rows(tids[raw[1::3] % np.uint64(len(tids))], raw[2::3], r2, kind, n))
    return out


def wo_runs(cfg, seed, n=ROUND_OPS, rounds=4):
    """Runs of WriteOnly that start and end mid-wave and mid-tile (one crosses a tile edge, one a
    chunk edge at 4096), the rest ReadWrite. Round 0's WriteOnly tids are >= 2^31 (8-B seen values
    in that chunk and, through the words they leave, the next); later rounds write small tids."""
    runs = [(37, 140), (SYA_OPS - 30, SYA_OPS + 45), (2 * SYA_OPS - 700, 2 * SYA_OPS + 3), (3 * SYA_OPS + 5, 3 * SYA_OPS + 70)]
    big = np.array([(1 << 40) + 3, 1 << 31, M64 - 15, (1 << 63) + seed % 1000], np.uint64)
    small = np.array([0, 1, 7, 2 + seed % 1000], np.uint64)
    out = []
    for r in range(rounds):
        raw = sm64(seed * 1000 + 400 + r, 3 * n)
        a = _rows(small[raw[0::3] % np.uint64(4)], raw[1::3], raw[2::3], RW, n)
        for lo, hi in runs:
            lo, hi = min(lo + 11 * r, n), min(hi + 11 * r, n)
            a[lo:hi, 3] = WO
            if r == 0:
                a[lo:hi, 0] = big[raw[0::3][lo:hi] % np.uint64(4)]
        out.append(a)
    return out


def sentinel(cfg, seed, n=ROUND_OPS, rounds=4):
    """random30 with r2 = 2^64 - 1 on every third op: the hot range wraps, and the sort path emits
    its sentinel key for each of the op's hot touches"""
    out = random30(cfg, seed + 5, n, rounds)
    for a in out:
        a[seed % 3::3, 2] = M64
    return out


STREAMS = dict(random=random, random30=random30, one_word=one_word, sweep=sweep, edges=edges, hot_repeat=hot_repeat,
               wo_runs=wo_runs, sentinel=sentinel)


def reads(cfg, seed, n=200):
    """a batch of ReadOnly ops, (n, 3) {tid, r1, r2}: random, with wrapping hot ranges and r2 = 0"""
    raw = sm64(seed * 1000 + 500, 3 * n)
    a = np.zeros((n, 3), np.uint64)
    a[:, 0], a[:, 1], a[:, 2] = raw[0::3] % np.uint64(8), raw[1::3], raw[2::3]
    a[::13, 2] = np.uint64(M64) - np.arange(len(a[::13]), dtype=np.uint64) % np.uint64(3)
    a[::17, 2] = 0
    return a


# ---- the matrix ------------------------------------------------------------------------------
MAX_BATCH = 2 * SYA_OPS  # a ROUND_OPS exec spans two chunks


def matrix():
    """[(name, Cfg, stream names)]: one thing at a time away from the defaults, plus the listed
    combinations. The expected path of each is bucket_eligible(cfg, MAX_BATCH)."""
    m = []
    for cw in (1, 2, 3, 4, 6, 7, 8):
        m.append((f"cw{cw}", Cfg(cold_writes=cw), ("random", "one_word", "sweep", "wo_runs")))
    # fewer than 512 buckets: W = 1, 1 + 299 buckets
    for cw in (1, 8):
        m.append((f"cw{cw}_n302", Cfg(n=302, cold_writes=cw), ("random", "one_word", "sweep", "wo_runs")))
    for hr in (7, 17):
        m.append((f"hr{hr}", Cfg(hot_reads=hr), ("hot_repeat", "random30")))
    for hr in (1, 3, 16):
        for hw in sorted({0, 1, hr, hr + 1, 2 * hr + 1}):
            m.append((f"hr{hr}_hw{hw}", Cfg(hot_reads=hr, hot_writes=hw), ("hot_repeat", "random30")))
    for span in (1, 2, 3, 509, 510, 4096, 49999, MAX_ELIGIBLE_SPAN, MAX_ELIGIBLE_SPAN + 1):
        m.append((f"span{span}", with_span(span), ("random", "sweep", "edges")))
    m.append(("cw0_hw3", Cfg(cold_writes=0, hot_writes=3), ("random30", "hot_repeat")))
    m.append(("cw9", Cfg(cold_writes=9), ("random", "one_word")))
    m.append(("cw63_hw1", Cfg(cold_writes=63), ("random", "wo_runs")))
    m.append(("n1023", Cfg(n=1023), ("sentinel", "sweep")))
    m.append(("n1024", Cfg(n=1024), ("sentinel", "sweep")))
    return m
