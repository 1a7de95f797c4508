"""Sequential model of the file store WITH SIZES (include/nrgpu.h, nrg_memfs_enable_sizes: SetAttr as
ftruncate, Writes that grow a file) and the named record streams the CPU and GPU tests share.

The model is the definition read literally: a bytearray of B bytes and a size per file, every byte
0x01 and every size B when sizes are enabled, the records applied one by one in log order. Bytes at
and past a file's size are kept zero, as the device keeps them, so that the raw bytes compare too.
Nothing of the GPU's plan (sort by file, scan of composed functions, line runs) decides an answer
here. The model does count, beside the answers, which arms of the definition and which positions of
the replay plan a stream reaches (`arms`), so that a stream named for an arm can be checked on the
CPU to still reach it; those counters read the plan's geometry (128-byte lines, chunks) and nothing
else.

then() / apply_fn() are the scan element of csrc/memfs.hip (mfs_then) written out in Python:
tests/test_memfs_size_cpu.py folds them over random op lists against this model.
"""
from collections import Counter

import numpy as np

import memfs_model as M
from memfs_model import ENOENT, EFBIG, EINVAL, FIRST_INO, G, LINE, OP_DTYPE, R, RESP_DTYPE, W, rec

WRITE, READ, GETATTR, SETATTR = 0, 1, 2, 3
_M = 0xFFFFFFFFFFFFFFFF


def S(ino, size, length=0):
    """SetAttr: offset carries the new size."""
    return rec(ino, size, SETATTR, length)


class SizedModel:
    def __init__(self, files=1, log2_b=12):
        self.files, self.B = files, 1 << log2_b
        self.data = [bytearray(b"\x01" * self.B) for _ in range(files)]
        self.size = [self.B] * files
        self.inval = False
        self.arms = Counter()
        self.new_chunk()

    # -- the direct calls ---------------------------------------------------------------------
    def init(self, ino, data):
        f = ino - FIRST_INO
        self.data[f][: len(data)] = data
        self.size[f] = max(self.size[f], len(data))

    def truncate(self, ino, size):
        f = ino - FIRST_INO
        if size < self.size[f]:
            self.data[f][size:self.size[f]] = bytes(self.size[f] - size)
        self.size[f] = size

    # -- plan counters (no answer depends on them) ----------------------------------------------
    def new_chunk(self):
        """A chunk of the replay begins: close the line runs of the last one."""
        for (f, line), pos in getattr(self, "_runpos", {}).items():
            if self._shrinks[f] > self._seen[(f, line)]:
                self.arms["shrink_after_run"] += 1
        for f, n in enumerate(getattr(self, "_shrinks", [])):
            if n:
                touched = sum(1 for (g, _) in self._runpos if g == f)
                self.arms["shrink_on_empty_line"] += self.B // LINE - touched
        self._runpos, self._seen, self._shrinks = {}, {}, [0] * self.files

    def _touch(self, f, off, n):
        for line in range(off // LINE, (off + n - 1) // LINE + 1):
            k = (f, line)
            pos = self._runpos.get(k, 0)
            if self._shrinks[f] > self._seen.get(k, 0):
                self.arms["shrink_before_run_pos_%d" % pos] += 1
            self._seen[k] = self._shrinks[f]
            self._runpos[k] = pos + 1

    # -- one record -----------------------------------------------------------------------------
    def apply(self, ino, offset, op, length, data=b""):
        """(some, n, the 128 response data bytes)."""
        zero = bytes(128)
        a = self.arms
        if op > SETATTR or length > 128:
            self.inval = True
            a["einval"] += 1
            return 0, EINVAL, zero
        if not FIRST_INO <= ino < FIRST_INO + self.files:
            a["enoent"] += 1
            return 0, ENOENT, zero
        f = ino - FIRST_INO
        d, size = self.data[f], self.size[f]
        if op == GETATTR:
            a["getattr"] += 1
            return 1, size, zero
        if op == SETATTR:
            s = offset
            if s > self.B:
                a["efbig_setattr"] += 1
                return 0, EFBIG, zero
            if s < size:
                d[s:size] = bytes(size - s)
                a["shrink"] += 1
                a["shrink_mid_line" if s % LINE else "shrink_to_line_edge"] += 1
                if s == 0:
                    a["shrink_to_0"] += 1
                self._shrinks[f] += 1
            elif s == size:
                a["setattr_same"] += 1
            else:
                a["grow_setattr"] += 1
                if s == self.B:
                    a["setattr_to_B"] += 1
            self.size[f] = s
            return 1, s, zero
        if op == WRITE:
            if offset + length > self.B:
                a["efbig_write"] += 1
                return 0, EFBIG, zero
            a["write"] += 1
            if length:
                d[offset:offset + length] = bytes(data[:length])
                if offset + length > size:
                    a["grow_write"] += 1
                    if offset > size:
                        a["gap_write"] += 1
                    if offset + length == self.B:
                        a["write_to_B"] += 1
                    self.size[f] = offset + length
                self._touch(f, offset, length)
            elif offset > size:
                a["len0_write_past_size"] += 1
            return 1, length, zero
        a["read"] += 1
        n = 0 if offset >= size else min(length, size - offset)
        if length and offset == size:
            a["read_at_size"] += 1
        elif length and size < offset < self.B:
            a["read_past_size"] += 1
        elif n < length:
            a["read_clipped"] += 1
        if n:
            self._touch(f, offset, n)
        return 1, n, bytes(d[offset:offset + n]) + bytes(128 - n)

    def replay(self, recs):
        """(responses, some) of one chunk's records applied in order."""
        resp = np.zeros(len(recs), RESP_DTYPE)
        some = np.zeros(len(recs), np.uint8)
        self.new_chunk()
        for i, r in enumerate(recs):
            s, n, d = self.apply(int(r["ino"]), int(r["offset"]), int(r["op"]), int(r["len"]), r["data"].tobytes())
            some[i], resp["n"][i] = s, n
            resp["data"][i] = np.frombuffer(d, np.uint8)
        return resp, some

    def dump(self, ino):
        """nrg_memfs_dump: the file up to its size."""
        f = ino - FIRST_INO
        return bytes(self.data[f][: self.size[f]])

    def raw(self):
        """Every stored byte, file after file: the payload of a snapshot before the sizes."""
        return b"".join(bytes(d) for d in self.data)

    def digest(self):
        """(count, sum, xor) of mix64(k ^ mix64(v)): the unsized items (every aligned 8-byte word,
        k = file << 32 | word index) plus (file << 32 | 0xFFFFFFFF, size) per file; plain integers."""
        c = s = x = 0
        for f, d in enumerate(self.data):
            items = [((f << 32) | w, int.from_bytes(d[8 * w:8 * w + 8], "little")) for w in range(self.B // 8)]
            items.append(((f << 32) | 0xFFFFFFFF, self.size[f]))
            for k, v in items:
                h = M._mix64(k ^ M._mix64(v))
                c, s, x = c + 1, (s + h) & _M, x ^ h
        return c, s, x


# ---- the scan element (csrc/memfs.hip mfs_then), for the CPU test -----------------------------------------
NONE = 0xFFFFFFFF
IDENT = (False, 0, 0, NONE, NONE)  # (const, v, decided shrinks k, undecided target t, smallest decided target m)


def element(op, offset, length, B, valid_file=True):
    """A record's function on its file's size."""
    if not valid_file or length > 128:
        return IDENT
    if op == WRITE and length and offset + length <= B:
        return (False, offset + length, 0, NONE, NONE)
    if op == SETATTR and offset <= B:
        return (True, offset, 0, offset, NONE)
    return IDENT


def then(F, G):
    """F, then G."""
    fc, fv, fk, ft, fm = F
    gc, gv, gk, gt, gm = G
    k, t, m = fk + gk, ft, min(fm, gm)
    if gt != NONE:
        if gt < fv:
            k, m = k + 1, min(m, gt)
        elif not fc:
            t = gt
    return (fc or gc, gv if gc else max(fv, gv), k, t, m)


def apply_fn(F, x):
    """(size, shrinks, smallest shrink target or NONE) of F on a file of size x."""
    c, v, k, t, m = F
    pend = t != NONE and t < x
    return (v if c else max(x, v)), k + (1 if pend else 0), (min(m, t) if pend else m)


# ---- streams ----------------------------------------------------------------------------------------------
class Stream:
    """A named stream: geometry, its chunks (each replayed as one round) and the arms its name
    promises (`needs`: arm -> the least count the model must report)."""

    def __init__(self, name, files, log2_b, chunks, needs, max_batch=None):
        self.name, self.files, self.log2_b = name, files, log2_b
        self.chunks = [np.concatenate(c) if isinstance(c, list) else c for c in chunks]
        self.needs, self.max_batch = needs, max_batch

    @property
    def recs(self):
        return np.concatenate(self.chunks)

    def cfg(self, **kw):
        return dict(log2_slots=self.log2_b, queue_capacity=self.files, **kw)


_cache = {}


def expected(s):
    """(model after the stream, [(resp, some) per chunk]); computed once per stream and shared."""
    if s.name not in _cache:
        m = SizedModel(s.files, s.log2_b)
        out = [m.replay(c) for c in s.chunks]
        m.new_chunk()
        _cache[s.name] = (m, out)
    return _cache[s.name]


def _pat(rng, n):
    return M._pattern(rng, n)


def one_line_one_run():
    rng = np.random.default_rng(1)
    old, mid = _pat(rng, 128), _pat(rng, 32)
    s = Stream("one_line_one_run", 1, 7, [[W(5, 0, old), S(5, 5), W(5, 64, mid), S(5, 80), S(5, 128), R(5, 0, 128)]],
               {"shrink": 2, "grow_setattr": 1, "gap_write": 1, "setattr_to_B": 1})
    s.old, s.mid = old, mid
    return s


def shrink_targets():
    rng = np.random.default_rng(2)
    B = 512
    out = []
    for ino in (5, 6):
        out += [W(ino, o, _pat(rng, 128)) for o in range(0, B, 128)]
        out += [S(ino, 200), R(ino, 128, 128), G(ino), S(ino, B), R(ino, 128, 128)]       # mid-line
        out += [W(ino, 200, _pat(rng, 128)), S(ino, 256), R(ino, 200, 128), G(ino)]       # a line boundary
        out += [S(ino, 256), G(ino)]                                                      # the current size
        out += [S(ino, 0), R(ino, 0, 128), G(ino), S(ino, B), R(ino, 0, 128), R(ino, B - 128, 128), G(ino)]
        out += [S(ino, B + 1), G(ino), S(ino, 1 << 40), S(ino, (1 << 64) - 1)]            # EFBIG
        out += [S(ino, 10, 129), G(ino)]                                                  # EINVAL first
        out += [S(ino + 2, 10), S(4, 0), G(ino)]                                          # ENOENT
    return Stream("shrink_targets", 2, 9, [out], {"shrink_mid_line": 2, "shrink_to_line_edge": 4, "shrink_to_0": 2,
                                                  "setattr_same": 2, "setattr_to_B": 4, "efbig_setattr": 6,
                                                  "einval": 2, "enoent": 4})


def growing_writes():
    rng = np.random.default_rng(3)
    B = 512
    out = []
    for ino in (5, 6):
        out += [S(ino, 100), W(ino, 150, _pat(rng, 20)), R(ino, 90, 100), G(ino)]  # a gap of 50 zeros
        out += [W(ino, B - 28, _pat(rng, 28)), G(ino), R(ino, 160, 128), R(ino, B - 64, 64)]  # ends exactly at B
        out += [S(ino, 50), W(ino, 300, b""), G(ino), R(ino, 0, 128)]  # len 0 past the size: no growth
        out += [W(ino, 50, _pat(rng, 1)), G(ino), W(ino, 52, _pat(rng, 128)), G(ino), R(ino, 40, 128)]
    return Stream("growing_writes", 2, 9, [out], {"gap_write": 4, "grow_write": 8, "write_to_B": 2,
                                                  "len0_write_past_size": 2, "shrink": 4})


def reads_at_the_end():
    out = []
    for ino in (5, 6):
        out += [S(ino, 300), R(ino, 290, 20), G(ino), R(ino, 300, 8), G(ino), R(ino, 400, 16), G(ino),
                R(ino, 299, 1), R(ino, 172, 128), R(ino, 173, 128), R(ino, 511, 1), R(ino, 512, 1), G(ino)]
    return Stream("reads_at_the_end", 2, 9, [out], {"read_clipped": 4, "read_at_size": 2, "read_past_size": 4,
                                                    "getattr": 8})


def untouched_lines(one_chunk):
    rng = np.random.default_rng(4)
    B = 4096
    fill = [W(5, o, _pat(rng, 128)) for o in range(0, B, 128)]
    reads = [R(5, o, 128) for o in range(0, B, 128)]
    if one_chunk:
        chunks = [fill, [S(5, 10), S(5, B)] + reads + [G(5)]]
        needs = {"shrink": 1, "setattr_to_B": 1, "shrink_before_run_pos_0": 32}
    else:
        chunks = [fill, [S(5, 10)], [S(5, B)] + reads + [G(5)]]
        needs = {"shrink": 1, "setattr_to_B": 1, "shrink_on_empty_line": 32}
    return Stream("untouched_lines_%s" % ("one_chunk" if one_chunk else "three_chunks"), 1, 12, chunks, needs)


RUN_SHRINKS = (7, 8, 9, 63, 64, 65)


def run_positions():
    """One line, a run of 70 ops; a SetAttr that shrinks sits before the run's ops 7, 8, 9, 63, 64, 65
    (the look-ahead group of 8 and the batch of 64) and after its last. Every target is at least 8 and
    every Read starts below 8, so every op of the run covers a byte and the positions are exact."""
    rng = np.random.default_rng(5)
    out = [W(5, 0, _pat(rng, 128))]
    for pos in range(1, 70):
        if pos in RUN_SHRINKS:
            t = int(rng.integers(8, 100))
            out += [S(5, 128), S(5, t)]  # (grown to B first, so that t is below the size: a shrink)
            out.append(W(5, t + 5, _pat(rng, int(rng.integers(1, 128 - t - 5)))))  # a gap, then bytes
        elif pos % 3 == 0:
            off = int(rng.integers(0, 100))
            out.append(W(5, off, _pat(rng, int(rng.integers(1, 128 - off)))))
        else:
            out.append(R(5, int(rng.integers(0, 8)), 128))
    out += [S(5, 128), S(5, 33)]
    needs = {"shrink_before_run_pos_%d" % p: 1 for p in RUN_SHRINKS}
    needs.update(shrink_after_run=1, shrink=7)
    return Stream("run_positions", 1, 7, [out, [R(5, 0, 128), G(5)]], needs)


def chunk_edges():
    rng = np.random.default_rng(6)
    fill = [W(5, o, _pat(rng, 128)) for o in range(0, 512, 128)]
    c1 = [S(5, 40), W(5, 100, _pat(rng, 60)), R(5, 0, 128), R(5, 100, 128)]       # a shrink first
    c2 = [R(5, 128, 64), W(5, 300, _pat(rng, 100)), R(5, 256, 128), S(5, 130)]    # a shrink last
    c3 = [R(5, o, 128) for o in range(0, 512, 128)] + [G(5)]
    return Stream("chunk_edges", 2, 9, [fill, c1, c2, c3], {"shrink": 2, "shrink_before_run_pos_0": 2,
                                                            "shrink_after_run": 1, "shrink_on_empty_line": 3})


def random_stream(name, n, seed, files, log2_b, setattr_pct=5, max_batch=None, chunk=None):
    """n random records: setattr_pct % SetAttr (to 0, B, or anywhere in 0 .. B), 35 % Writes, 10 %
    GetAttr, the rest Reads that may start past the end; now and then a bad ino or a range past B.
    No EINVAL: nothing may be latched."""
    rng = np.random.default_rng(seed)
    B = 1 << log2_b
    out = []
    for _ in range(n):
        ino = FIRST_INO + int(rng.integers(0, files))
        if rng.random() < 0.002:
            ino = FIRST_INO + files
        k = rng.random() * 100
        if k < setattr_pct:
            z = rng.random()
            out.append(S(ino, 0 if z < 0.05 else (B if z < 0.15 else (B + 1 if z < 0.17 else int(rng.integers(0, B + 1))))))
        elif k < setattr_pct + 35:
            ln = int(rng.integers(0, 129))
            off = int(rng.integers(0, B - ln + (2 if rng.random() < 0.02 else 1)))
            out.append(W(ino, off, _pat(rng, ln)))
        elif k < setattr_pct + 45:
            out.append(G(ino))
        else:
            out.append(R(ino, int(rng.integers(0, B + 16)), int(rng.integers(0, 129))))
    recs = np.concatenate(out)
    chunks = [recs] if not chunk else [recs[i:i + chunk] for i in range(0, n, chunk)]
    share = max(1, n * setattr_pct // 400)
    return Stream(name, files, log2_b, chunks, {"shrink": share, "grow_write": 1, "read_clipped": 1, "getattr": 1},
                  max_batch=max_batch)


def hot_file(n):
    """memfs.rs's own shape, every op on ino 5: one segment of the scan is the whole chunk."""
    return random_stream("hot_file_%d" % n, n, 1000 + n, 1, 12, max_batch=max(8192, 1 << (n - 1).bit_length()))


def all_streams():
    """Every named stream the GPU test replays."""
    s = [one_line_one_run(), shrink_targets(), growing_writes(), reads_at_the_end(), untouched_lines(False),
         untouched_lines(True), run_positions(), chunk_edges()]
    s += [hot_file(n) for n in (255, 256, 257, 1025, 4097, 65537)]
    s += [random_stream("three_files_4097", 4097, 31, 3, 9), random_stream("files_300_4097", 4097, 32, 300, 7),
          random_stream("one_line_file_1025", 1025, 33, 1, 7, setattr_pct=10)]
    return s
