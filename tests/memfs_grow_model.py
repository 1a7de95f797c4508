"""Sequential model of the file store WITH SIZES AND A GROWTH BOUND (include/nrgpu.h "File store: capacity
growth": nrg_set_max_capacity in bytes per file, nrg_memfs_reserve) and the named record streams the CPU
and GPU tests share.

The model is tests/memfs_size_model.py's SizedModel with the definition of growth read literally, record
by record: a record is admitted against max(B, the bound); an admitted Write of len > 0 or SetAttr whose
end lies past B first extends every file's bytearray with zeros to the power of two at or above that end.
So the capacity after any prefix is max(the capacity at open or the last reserve, pow2ceil(the largest
admitted end so far)), whatever chunks the device replays the prefix in. Nothing of the device's plan
(the need kernel, the relayout, the readback) is restated here.

need() / grow_log2() restate csrc/memfs_plan.hpp's mf_rec_need / mf_grow_log2; tests/memfs_grow_policy.cpp
checks the header's own against a third, independent statement in C++.
"""
import numpy as np

import memfs_model as M
import memfs_size_model as Z
from memfs_model import ENOENT, EFBIG, EINVAL, FIRST_INO, G, R, W
from memfs_size_model import S, SETATTR, WRITE

U64 = (1 << 64) - 1


def pow2ceil(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def need(ino, offset, op, length, files, max_bytes):
    """The end a record asks the store to hold under a bound of max_bytes, or 0 (mf_rec_need)."""
    if op > SETATTR or length > 128 or not FIRST_INO <= ino < FIRST_INO + files:
        return 0
    if op == WRITE:
        return offset + length if length and offset + length <= max_bytes else 0
    if op == SETATTR:
        return offset if offset <= max_bytes else 0
    return 0


def grow_log2(log2_b, need_bytes, max_log2):
    """mf_grow_log2: log2 of the capacity that holds need_bytes, from log2_b, never past max_log2."""
    l = log2_b
    while l < max_log2 and (1 << l) < need_bytes:
        l += 1
    return l


class GrowModel(Z.SizedModel):
    """SizedModel whose files grow: `bound` bytes per file (0: none, a fixed capacity)."""

    def __init__(self, files=1, log2_b=12, bound=0):
        super().__init__(files, log2_b)
        self.bound = bound
        self.grows = 0  # times the capacity changed

    def adm(self):
        return max(self.B, self.bound)

    def _extend(self, to):
        if to > self.B:
            for d in self.data:
                d.extend(bytes(to - self.B))
            self.B = to
            self.grows += 1

    def reserve(self, file_bytes):
        self._extend(pow2ceil(file_bytes))

    def truncate(self, ino, size):
        assert size <= self.adm()
        self._extend(pow2ceil(size))
        super().truncate(ino, size)

    def apply(self, ino, offset, op, length, data=b""):
        zero = bytes(128)
        if op <= SETATTR and length <= 128 and FIRST_INO <= ino < FIRST_INO + self.files:
            if op == WRITE and offset + length > self.adm():
                return 0, EFBIG, zero
            if op == WRITE and length == 0:  # within the bound: valid, touches nothing, grows nothing
                return 1, 0, zero
            if op == SETATTR and offset > self.adm():
                return 0, EFBIG, zero
            self._extend(pow2ceil(need(ino, offset, op, length, self.files, self.adm())))
        return super().apply(ino, offset, op, length, data)


class Stream(Z.Stream):
    """A named stream with a bound, what is done before the records (`seed(model_or_dev_adapter)`), and
    the geometry it must end with."""

    def __init__(self, name, files, log2_b, bound, recs, end_b, seed=None):
        super().__init__(name, files, log2_b, [recs], {})
        self.bound, self.end_b, self.seed = bound, end_b, seed or (lambda t: None)


_cache = {}


def expected(s):
    """(model after the stream, (resp, some) of the whole stream); computed once per stream and shared."""
    if s.name not in _cache:
        m = GrowModel(s.files, s.log2_b, s.bound)
        s.seed(m)
        _cache[s.name] = (m, m.replay(s.recs))
    return _cache[s.name]


def _pat(rng, n):
    return M._pattern(rng, n)


def append():
    """fxmark's append shape: one file grows write by write from 128 bytes to 4096."""
    rng = np.random.default_rng(11)
    recs = [W(5, 128 * k, _pat(rng, 128)) for k in range(32)]
    return Stream("append", 1, 7, 4096, recs, 4096, seed=lambda t: t.truncate(5, 0))


def straddle():
    """One Write over the old end: its first line is in the old store, its second in the new; a logged
    Read of the range later in the same chunk sees it."""
    rng = np.random.default_rng(12)
    B = 256
    recs = [W(5, 0, _pat(rng, 128)), W(5, B - 64, _pat(rng, 128)), G(5), R(5, B - 64, 128), R(5, B - 128, 128),
            R(5, B, 128), G(5)]
    return Stream("straddle", 1, 8, 1024, recs, 512)


def _seed3(B):
    def seed(t):
        for f in range(3):
            t.init(5 + f, bytes(((7 + 31 * f + i) % 251) + 1 for i in range(B)))
    return seed


def stride():
    """Three seeded files; only file 1 is written past B: files 0 and 2 intact at the new stride."""
    rng = np.random.default_rng(13)
    B = 256
    recs = [W(6, 700, _pat(rng, 100)), R(5, 128, 128), R(7, 128, 128), R(6, 672, 128), G(5), G(6), G(7),
            W(5, 10, _pat(rng, 20)), W(7, 200, _pat(rng, 56)), R(7, 128, 128)]
    return Stream("stride", 3, 8, 2048, recs, 1024, seed=_seed3(B))


def edges():
    """Ends at max and max + 1, SetAttr to max and max + 1, offsets near 2^64, a bad ino with a huge
    offset, len = 129 with a huge offset: the refused records change and grow nothing. The admitted
    ones alone end at 1024 = max."""
    rng = np.random.default_rng(14)
    mx = 1024
    recs = [W(5, 300, _pat(rng, 50)),                       # grows 128 -> 512
            W(5, mx - 127, _pat(rng, 128)),                 # ends at max + 1: EFBIG
            S(6, mx + 1), S(6, 1 << 40), S(6, U64),         # EFBIG
            W(5, U64, _pat(rng, 1)), W(5, U64 - 5, _pat(rng, 128)), W(5, U64, b""),  # wraps / past max: EFBIG
            W(9, mx - 128, _pat(rng, 128)), W(4, 1 << 50, _pat(rng, 8)), S(9, mx),    # ENOENT with any offset
            M.rec(5, 1 << 60, WRITE, 129), M.rec(5, 600, WRITE, 129), S(5, 700, 129),  # EINVAL first
            W(5, 600, b""), W(5, mx, b""), W(5, mx + 1, b""),  # no bytes: valid within max, grows nothing
            G(5), G(6), R(5, 256, 128)]
    mid = list(recs)
    recs += [W(5, mx - 128, _pat(rng, 128)),                # ends at max: 512 -> 1024
             S(6, mx), G(6), R(6, mx - 64, 128), S(6, 100), G(6), R(5, mx - 128, 128), G(5)]
    s = Stream("edges", 2, 7, mx, recs, mx)
    s.mid = len(mid)  # B after this many records is 512: what the first admitted record alone gives
    return s


def extend():
    """ftruncate past B, a Read of the hole (zeros), then a shrink: the capacity stays."""
    rng = np.random.default_rng(15)
    recs = [W(5, 0, _pat(rng, 128)), S(5, 3000), G(5), R(5, 2000, 128), R(5, 100, 128), R(5, 2990, 128),
            S(5, 64), G(5), R(5, 0, 128), S(5, 200), R(5, 0, 128), R(5, 100, 128)]
    return Stream("extend", 1, 8, 4096, recs, 4096)


def mid():
    """Three files of random bytes from 4096 to 2^20 bytes each: the relayout's grid-stride and tails."""
    rng = np.random.default_rng(16)
    B, mx = 4096, 1 << 20
    blobs = [rng.integers(1, 256, B, dtype=np.uint8).tobytes() for _ in range(3)]

    def seed(t):
        for f in range(3):
            t.init(5 + f, blobs[f])
    recs = [W(6, mx - 128, _pat(rng, 128)), R(5, 4000, 128), R(7, 0, 128), R(6, mx - 100, 128), R(6, 4090, 64), G(6)]
    return Stream("mid", 3, 12, mx, recs, mx, seed=seed)


def all_streams():
    return [append(), straddle(), stride(), edges(), extend(), mid()]
