"""Named Put streams for the write side of the hashmap replay, and a host model of where they land.

The seeded uniform and Zipf rounds of tests/test_gpu_hashmap.py replay a few round sizes in roomy
tables. Every stream here is aimed at one constant of csrc/hashmap.hip instead: a round size at a
tile, wave or chunk edge, one apply bucket taken in several chunks with previous values (and the
state the walk carries between its 64-entry steps and 512-entry chunks), duplicates on either side
of an index tile, the stamp rounds' block combine table and their election across blocks, a table
filled to its last slot through the replay's own claims, two apply workgroups claiming in the
same groups, and keys one kind of round placed in a chain's second group found by another kind.

The model restates, in numpy, what decides where a Put goes: mix64, a key's home slot, the probe
sequence, a sequential placement, and the partition round's geometry as hm_replay_chunk derives
it. tests/test_hashmap_streams_cpu.py pins the mirrored constants to the source text and checks
that every stream has the property it is named for; tests/test_gpu_hashmap_streams.py replays the
streams on the GPU, path by path. Values are distinct over a stream (mix64 of a counter), so a
wrong previous value never passes by coincidence. No GPU and no library: numpy alone.
"""
import numpy as np

U64 = np.uint64
SIDE = 0xFFFFFFFFFFFFFFFF  # EMPTY_KEY: the one key that lives in the side slot

# ---- constants mirrored from csrc/hashmap.hip and csrc/common.hpp ------------------------------------
TPB = 256
SM_W, SM_R, SM_HT = 2048, 8192, 4096
PA_WIDTHS = (256, 512, 1024)
PA_PREV_C = 512                            # PaGeo<true, 256>::C
PA_C_PER_THREAD = 4                        # PaGeo<false, T>::C = 4 * T
PA_HT_PER_C = 2                            # PaGeo::HT = 2 * C
PA_NB_LOG = {256: 10, 512: 9, 1024: 8}     # PaGeo<., T>::NB_LOG
STAMP_HT_PER_TILE = 2                      # StampLds<K1>::HT = 2 * TILE
PART_MIN = 3 << 17
PA_WIDE_MIN = 1 << 16
HM_BK_MAX = 1024
TILE_THRESHOLDS = (1 << 14, 1 << 16, 1 << 18)  # partition tile 256 / 512 / 1024 / 2048 Puts
WALK = 64                                  # entries per step of the previous-value walk (one wave)


def pa_c(want_prev, pa_t):
    return PA_PREV_C if want_prev else PA_C_PER_THREAD * pa_t


# ---- host model ----------------------------------------------------------------------------------
def mix64(x):
    x = np.asarray(x, U64)
    with np.errstate(over="ignore"):
        x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
        return x ^ (x >> U64(31))


def home(key, log2_slots):
    return mix64(key) >> U64(64 - log2_slots)


def probe_slot(h, p, tmask):
    return ((((h >> 2) + (p >> 2)) << 2) | ((h + p) & 3)) & tmask


def place(keys, log2_slots, table=None):
    """Insert `keys` (distinct, none the side key) in order into `table` (slot -> key, a dict; a
    new one if None); the slot of each, -1 where no slot is left."""
    table = {} if table is None else table
    tmask = (1 << log2_slots) - 1
    homes = home(keys, log2_slots)
    out = np.full(len(keys), -1, np.int64)
    for i, (k, h) in enumerate(zip(np.asarray(keys, U64).tolist(), homes.tolist())):
        for p in range(tmask + 1):
            s = probe_slot(h, p, tmask)
            if table.get(s, k) == k:
                table[s] = k
                out[i] = s
                break
    return out


def round_geometry(n, log2_slots, want_prev, pa_tpb=0):
    """(K1, tile, nb_log, bk_shift, C) of a partition round of n Puts, as hm_replay_chunk has them."""
    t0, t1, t2 = TILE_THRESHOLDS
    K1 = 1 if n <= t0 else 2 if n <= t1 else 4 if n <= t2 else 8
    nb_log = 0
    while (64 << nb_log) < n and (1 << nb_log) < HM_BK_MAX:
        nb_log += 1
    pa_t = 256 if want_prev else pa_tpb if pa_tpb else 512 if n >= PA_WIDE_MIN else 256
    nb_log = min(nb_log, PA_NB_LOG[pa_t], log2_slots)
    return K1, TPB * K1, nb_log, log2_slots - nb_log, pa_c(want_prev, pa_t)


def bucket(key, log2_slots, bk_shift):
    """Apply bucket of every key (the side key: bucket 0)."""
    key = np.asarray(key, U64)
    return np.where(key == U64(SIDE), U64(0), home(key, log2_slots) >> U64(bk_shift)).astype(np.int64)


def stamp_k1(n, R, knob=0):
    if knob:
        return 4 if knob >= 4 else 2 if knob >= 2 else 1
    return 1 if n <= (1 << 18) else 4 if n >= 655360 and R >= n else 2


# ---- key picking ---------------------------------------------------------------------------------
N_CAND = 4_000_000
_cand = {}


def _candidates():
    if not _cand:
        _cand["k"] = np.arange(1, N_CAND, dtype=U64)
        _cand["m"] = mix64(_cand["k"])
    return _cand["k"], _cand["m"]


def keys_with_home(pred, count, log2_slots, skip=0):
    """The first `count` candidate keys (after `skip` matches) whose home slot satisfies `pred`."""
    k, m = _candidates()
    sel = k[pred((m >> U64(64 - log2_slots)).astype(np.int64))][skip:skip + count]
    assert len(sel) == count, "not enough candidates"
    return sel


FREE_BASE = 1 << 23  # keys of any home: FREE_BASE + 3 j (above every candidate; key + 1 is never a key)


def free_keys(count, skip=0):
    return (FREE_BASE + 3 * np.arange(skip, skip + count)).astype(U64)


def absent_keys(count, skip=0):
    return (FREE_BASE + 3 * np.arange(skip, skip + count) + 2).astype(U64)


class Stream:
    def __init__(self, name, log2_slots, max_batch=4096):
        self.name = name
        self.log2_slots = log2_slots
        self.max_batch = max_batch
        self.rounds = []     # (put_keys, put_vals, get_keys)
        self.window = None   # list of (a, b): response windows of the last round (prev_window)
        self.refused = {}    # round -> indices of Puts the full table cannot take
        self.claims = {}     # what the stream is built to have (checked on the host model)
        self._ctr = 0
        self._seed = int(mix64(np.frombuffer(name.encode().ljust(8, b"\0")[:8], U64)[0])) >> 20 << 20

    def vals(self, n):
        v = mix64(np.arange(self._ctr, self._ctr + n, dtype=U64) + U64(self._seed))
        self._ctr += n
        return v

    def add(self, put_keys, get_keys=None):
        pk = np.ascontiguousarray(put_keys, U64)
        if get_keys is None:  # every Put key, each key + 1, the side key
            u = np.unique(pk)
            with np.errstate(over="ignore"):
                get_keys = np.concatenate([u, u + U64(1), np.array([SIDE], U64)])
        self.rounds.append((pk, self.vals(len(pk)), np.ascontiguousarray(get_keys, U64)))
        return len(self.rounds) - 1

    def ops(self):
        return sum(len(pk) + len(gk) for pk, _, gk in self.rounds)


# ---- w<N>_<pattern>: round sizes at the wave, block and tile edges -------------------------------------
W_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049)
W_PATTERNS = ("new", "equal", "twice", "hits", "mix", "side_ends", "straddle")
STRADDLE_AT = (62, 63, 64, 254, 255, 256, 510, 511, 512, 1022, 1023, 1024)
W_PRESENT = 300


def w_names():
    return [f"w{n}_{p}" for p in W_PATTERNS for n in W_SIZES if p != "straddle" or n > STRADDLE_AT[0]]


def w_stream(n, pattern):
    st = Stream(f"w{n}_{pattern}", 12)
    present = free_keys(W_PRESENT)
    st.add(present)
    new = free_keys(n, W_PRESENT)
    i = np.arange(n)
    if pattern == "new":
        pk = new
    elif pattern == "equal":
        pk = np.repeat(new[:1], n)
    elif pattern == "twice":
        pk = np.repeat(new[:(n + 1) // 2], 2)[:n]
    elif pattern == "hits":
        pk = present[i % W_PRESENT]
    elif pattern == "mix":
        pk = np.where(i % 3 == 0, new[i // 3], np.where(i % 3 == 1, present[(i // 3) % W_PRESENT], U64(SIDE)))
    elif pattern == "side_ends":
        pk = np.repeat(present[7:8], n)
        pk[0] = pk[n - 1] = SIDE
    elif pattern == "straddle":
        pk = new.copy()
        at = [p for p in STRADDLE_AT if p < n]
        pk[at] = free_keys(1, W_PRESENT + n)[0]
        st.claims["straddle_at"] = at
    else:
        raise KeyError(pattern)
    st.add(pk)
    st.claims.update(n=n, pattern=pattern, present=present)
    return st


# ---- tile<K>_mix: the larger partition tiles -------------------------------------------------------
TILE_MIX = {"tile512_mix": (1 << 14) + 513, "tile1024_mix": (1 << 16) + 1025, "tile2048_mix": (1 << 18) + 2049}


def tile_mix(name):
    n = TILE_MIX[name]
    st = Stream(name, 20, max_batch=1 << n.bit_length())
    _, tile, _, _, _ = round_geometry(n, 20, False)
    i = np.arange(n)
    span = free_keys(n // 2)  # a new key (its first Put), a key Put earlier in the round, the side key
    pk = np.where(i % 3 == 0, span[i // 3], np.where(i % 3 == 1, span[(i // 3) // 2], U64(SIDE)))
    x = free_keys(1, n // 2)[0]
    lost = pk[[p for p in (tile - 1, tile) if p % 3 == 0]]
    pk[tile - 1] = pk[tile] = x  # one key on each side of the first tile edge
    pk[np.isin(pk, lost)] = span[0]  # (the later Puts of a key whose first Put made way)
    st.add(pk)
    st.claims.update(n=n, tile=tile, straddle_at=[tile - 1, tile])
    return st


# ---- prev_one_bucket / prev_window: one apply bucket in four chunks, with previous values -------------
PREV_N = 1600
PREV_EDGES = (0, 511, 512, 513, 1023, 1024, 1535, 1536, 1599)
PREV_SIDE = (5, 511, 512, 1599)
PREV_WINDOWS = ((0, 1600), (511, 513), (512, 1024), (600, 601), (1599, 1600))


def _prev_layout(side_wins):
    """One round of PREV_N Puts, all of apply bucket 0 (where the side key goes too), so a Put's
    position in its bucket is its index in the round. The edge key and the side key both want
    positions 511, 512 and 1599: `side_wins` says which of them gets those three."""
    _, _, nb_log, bk_shift, C = round_geometry(PREV_N, 12, True)
    assert (nb_log, C) == (5, 512)
    ks = keys_with_home(lambda h: (h >> bk_shift) == 0, 104, 12)
    named = dict(edge=ks[0], before=ks[1], claimed=ks[2], step=ks[3], step1=ks[4], alt0=ks[5], alt1=ks[6])
    fill = ks[8:]
    rng = np.random.default_rng(1600)
    pk = fill[rng.integers(0, len(fill), PREV_N)]
    at = {}
    at["before"] = [1100, 1300]                # present before the round, first Put in chunk 2
    at["claimed"] = [100, 1200]                # new, claimed in chunk 0, next written in chunk 2
    at["step"] = list(range(640, 704))         # a whole walk step
    at["step1"] = list(range(704, 769))        # a step and one more: crosses 767 | 768
    at["alt0"] = list(range(832, 896, 2))      # two keys lane by lane across a step
    at["alt1"] = list(range(833, 896, 2))
    contested = set(PREV_EDGES) & set(PREV_SIDE)
    at["edge"] = [p for p in PREV_EDGES if not (side_wins and p in contested)]
    at["side"] = [p for p in PREV_SIDE if side_wins or p not in contested]
    for name, pos in at.items():
        pk[pos] = SIDE if name == "side" else named[name]
    return pk, named, at, fill


def _prev_first(st):
    pk, named, at, fill = _prev_layout(False)
    # `before` and a third of the filler keys are present when the round starts
    st.add(np.concatenate([[named["before"]], fill[::3]]))
    st.add(pk)
    st.claims.update(named=named, at=at, fill=fill)
    return pk


def prev_one_bucket():
    st = Stream("prev_one_bucket", 12)
    pk = _prev_first(st)
    pk2, _, at2, _ = _prev_layout(True)
    st.add(pk2)
    st.add(pk[::-1])
    st.add(pk2[::-1])
    st.claims["at_side_wins"] = at2
    return st


def prev_window():
    st = Stream("prev_window", 12)
    _prev_first(st)
    st.window = list(PREV_WINDOWS)
    return st


# ---- dedup_tiles / dedup_chunks_<T>: duplicates round the index tiles and the apply chunks -------------
DEDUP_N = 2000


def dedup_tiles():
    st = Stream("dedup_tiles", 12)
    n = DEDUP_N
    pk = free_keys(n)
    extra = free_keys(8, n)
    pairs = {"in_tile": [(10, 200), (300, 301)], "across": [(255, 256), (1023, 1024)]}
    for j, (a, b) in enumerate(pairs["in_tile"] + pairs["across"]):
        pk[a] = pk[b] = extra[j]
    every = [TPB * t + 17 for t in range((n + TPB - 1) // TPB)]
    pk[every] = extra[4]
    side = [400, 450, 767, 768]  # the side key inside a tile and across an edge
    pk[side] = SIDE
    st.add(pk)
    st.add(pk[::-1])
    st.claims.update(pairs=pairs, every=every, side=side)
    return st


def dedup_chunks(T):
    """One bucket of 64 Puts fewer than three chunks of the T-thread apply, every index tile a
    permutation of the same 256 keys (the dedup index drops nothing, so chunk positions are round
    positions), and one key at chunk positions C - 1, C and 2 C."""
    C = pa_c(False, T)
    n = 3 * C - 64
    st = Stream(f"dedup_chunks_{T}", 12, max_batch=1 << n.bit_length())  # (one round: larger than 4096 for T > 256)
    _, tile, nb_log, bk_shift, c = round_geometry(n, 12, False, T)
    assert tile == TPB and c == C
    b = (1 << nb_log) - 2
    pool = keys_with_home(lambda h: (h >> bk_shift) == b, TPB, 12)
    rng = np.random.default_rng(T)
    pk = np.concatenate([rng.permutation(pool) for _ in range((n + TPB - 1) // TPB)])[:n]
    z = pool[0]
    at = [C - 1, C, 2 * C]
    for p in at:
        t0 = p // TPB * TPB
        q = t0 + int(np.nonzero(pk[t0:t0 + TPB] == z)[0][0])
        pk[q], pk[p] = pk[p], pk[q]
    st.add(pk, np.concatenate([pool, absent_keys(TPB)]))
    st.claims.update(T=T, C=C, n=n, bucket=b, key=z, at=at)
    return st


# ---- stamp_blocks_<tile>: the stamp rounds' block combine table and election across blocks -------------
STAMP_TILES = (256, 512, 1024)


def stamp_blocks(tile):
    n = 4 * tile + 7
    st = Stream(f"stamp_blocks_{tile}", 12, max_batch=1 << n.bit_length())  # (4 * 1024 + 7 is above 4096)
    hot, once = free_keys(2)
    distinct = free_keys(tile, 2)
    tail = free_keys(5, 2 + tile)
    g = 517  # one group of four slots
    grp = keys_with_home(lambda h: (h >> 2) == g, 8, 12)
    j = np.arange(tile)
    b0 = np.repeat(hot, tile)          # block 0: one key
    b1 = distinct.copy()               # block 1: all distinct and new (combine table at load 1/2)
    b2 = grp[j % len(grp)]             # block 2: every Put homes to one group
    b3 = distinct[(j * 7) % tile]      # block 3: block 1's keys again, in another order
    b3[1::2] = distinct[j[1::2] // 2]
    b1[3] = b2[9] = b3[tile - 2] = once    # one key once per block after block 0
    b2[40] = b3[41] = SIDE                  # the side key in two blocks
    b4 = np.concatenate([[once], tail, [hot]])  # block 0's key is the round's last record
    pk = np.concatenate([b0, b1, b2, b3, b4]).astype(U64)
    st.add(pk)
    st.add(pk[::-1])
    st.claims.update(tile=tile, n=n, hot=hot, once=once, group=g, distinct=(tile, 2 * tile), side=[2 * tile + 40, 3 * tile + 41])
    return st


# ---- full_<homes>: a 256-slot table filled to its last slot, and one key more --------------------------
FULL_HOMES = ("uniform", "last_group", "one_slot")
FULL_LOG2 = 8


def full(homes):
    st = Stream(f"full_{homes}", FULL_LOG2)
    S = 1 << FULL_LOG2
    pred = {"uniform": lambda h: h >= 0, "last_group": lambda h: h >= S - 4, "one_slot": lambda h: h == 77}[homes]
    ks = keys_with_home(pred, S + 1, FULL_LOG2)
    keys, extra = ks[:S], ks[S]
    side = np.array([SIDE], U64)
    seen = []

    def gets():
        k = np.concatenate(seen)
        return np.concatenate([k, absent_keys(len(k))])

    seen.append(keys[:100])
    st.add(keys[:100], gets())
    seen.append(keys[100:200])
    st.add(keys[100:200], gets())
    third = np.concatenate([keys[200:228], keys[:22], side, keys[228:256], keys[100:122]])  # 56 new, 44 present
    seen += [keys[200:256], side]
    st.add(third, gets())
    st.add(keys[::-1], gets())
    r = st.add(np.array([extra], U64), np.concatenate([gets(), [extra]]))  # the table is full
    st.refused[r] = [0]
    st.add(np.concatenate([keys, side]), np.concatenate([gets(), [extra]]))
    st.claims.update(keys=keys, extra=extra, homes=homes)
    return st


# ---- border_race: two apply workgroups claiming in the same groups -------------------------------------
BORDER_N = 2000


def border_race():
    st = Stream("border_race", 12)
    _, _, nb_log, bk_shift, _ = round_geometry(BORDER_N, 12, False)
    nb, per = 1 << nb_log, 1 << bk_shift  # buckets, slots per bucket
    borders = [(5, 6), (nb // 2 + 1, nb // 2 + 2), (nb - 1, 0)]  # the last one wraps the table's end
    present = free_keys(600)
    st.add(present)
    rng = np.random.default_rng(31)
    over, first = [], []
    for b, b1 in borders:
        # homed in the last group of bucket b: the chain runs on into bucket b + 1
        over.append(keys_with_home(lambda h: (h >> 2) == (b * per + per - 4) >> 2, 36, 12))
        # homed in the first six groups of bucket b + 1
        first.append(keys_with_home(lambda h: (h >= b1 * per) & (h < b1 * per + 24), 36, 12))

    def rnd(lo, hi):
        new = np.concatenate([a[lo:hi] for a in over + first])
        pk = present[rng.integers(0, len(present), BORDER_N)]
        pk[rng.choice(BORDER_N, len(new), replace=False)] = new
        return pk

    st.add(rnd(0, 24))
    st.add(rnd(0, 36)[::-1])
    st.claims.update(borders=borders, per=per, over=over, first=first, present=present)
    return st


# ---- chain_handover: keys placed by one round kind, found again by another -----------------------------
# The small rounds walk a chain by probe_slot(home, p), the stamp and partition rounds step by step
# with probe_next. Six keys per home slot: four fill the home group, two go on to the next group and
# sit at the home's offset and the one after it, with the slot before them empty -- a walker that
# entered that group anywhere else would meet the empty slot first and claim a second slot for a key
# the table holds. Rounds alternate between at most HANDOVER_SMALL Puts and more, so with SMALL_MAX =
# HANDOVER_SMALL each kind of round finds what the other one placed.
HANDOVER_SMALL = 64
HANDOVER_HOMES = (65, 130, 195, 260, 1001, 2002, 3003, 4092)  # offsets 1, 2, 3, 0, 1, 2, 3, 0; the last wraps


def chain_handover():
    st = Stream("chain_handover", 12)
    a = [keys_with_home(lambda h: h == hm, 6, 12) for hm in HANDOVER_HOMES[:4]]
    b = [keys_with_home(lambda h: h == hm, 6, 12) for hm in HANDOVER_HOMES[4:]]
    fill = free_keys(HANDOVER_SMALL + 1 - 24)
    ka, kb = np.concatenate(a), np.concatenate(b)
    st.add(ka)                                   # small: places a
    st.add(np.concatenate([ka, kb, fill]))       # large: finds a, places b
    st.add(np.concatenate([kb, ka[::-1][:16]]))  # small: finds b
    st.add(np.concatenate([fill, kb[::-1], ka]))  # large
    st.claims.update(clusters=a + b, homes=HANDOVER_HOMES)
    return st


# ---- the catalogue ---------------------------------------------------------------------------------
def names():
    return (w_names() + list(TILE_MIX) + ["prev_one_bucket", "prev_window", "dedup_tiles"] +
            [f"dedup_chunks_{T}" for T in PA_WIDTHS] + [f"stamp_blocks_{t}" for t in STAMP_TILES] +
            [f"full_{h}" for h in FULL_HOMES] + ["border_race", "chain_handover"])


LARGE = tuple(TILE_MIX)  # the only streams above MAX_OPS
MAX_OPS = 20_000
_built = {}


def get(name):
    """The stream of that name (built once; treat it as read-only)."""
    if name not in _built:
        head, _, tail = name.partition("_")
        if name in TILE_MIX:
            st = tile_mix(name)
        elif head[0] == "w" and head[1:].isdigit():
            st = w_stream(int(head[1:]), tail)
        elif name.startswith("dedup_chunks_"):
            st = dedup_chunks(int(name.rsplit("_", 1)[1]))
        elif name.startswith("stamp_blocks_"):
            st = stamp_blocks(int(name.rsplit("_", 1)[1]))
        elif name.startswith("full_"):
            st = full(tail)
        else:
            st = {"prev_one_bucket": prev_one_bucket, "prev_window": prev_window, "dedup_tiles": dedup_tiles,
                  "border_race": border_race, "chain_handover": chain_handover}[name]()
        assert st.name == name
        _built[name] = st
    return _built[name]
