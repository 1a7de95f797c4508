"""Sequential model of the replicated file store (include/nrgpu.h, kind NRG_DS_MEMFS) and the named
record streams the CPU and GPU tests share.

The model is the definition read literally: one bytearray per file, every byte 0x01 at open
(benches/memfs.rs:118), the records applied one by one in log order, each answering (some, n, data)
exactly as the header states. Nothing of the GPU's plan (lines, slots, sort) appears in it; the
streams' plan() does know about lines, so that a stream named for an arm of the kernels (a run that
ends at a batch edge, an op that crosses a line) can say on the CPU whether it still reaches it.
"""
from collections import Counter

import numpy as np

OP_DTYPE = np.dtype([("ino", "<u8"), ("offset", "<u8"), ("op", "<u4"), ("len", "<u4"), ("data", "u1", (128,))])
RESP_DTYPE = np.dtype([("n", "<u8"), ("data", "u1", (128,))])
WRITE, READ, GETATTR = 0, 1, 2
FIRST_INO = 5
ENOENT, EFBIG, EINVAL = 1, 2, 3
LINE = 128  # bytes of a line of the replay; also the most bytes a record carries
BATCH = 64  # slots of a line's run that mf_lines walks at a time

_M = 0xFFFFFFFFFFFFFFFF


def _mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
    return z ^ (z >> 31)


class MemFsModel:
    def __init__(self, files=1, log2_b=12):
        self.files, self.B = files, 1 << log2_b
        self.data = [bytearray(b"\x01" * self.B) for _ in range(files)]
        self.inval = False  # an EINVAL record was applied: the device latches NRG_E_INVAL

    def init(self, ino, data):
        self.data[ino - FIRST_INO][: len(data)] = data

    def apply(self, ino, offset, op, length, data=b""):
        """One record: (some, n, the 128 response data bytes)."""
        zero = bytes(128)
        if op > GETATTR or length > 128:
            self.inval = True
            return 0, EINVAL, zero
        if not FIRST_INO <= ino < FIRST_INO + self.files:
            return 0, ENOENT, zero
        f = self.data[ino - FIRST_INO]
        if op == GETATTR:
            return 1, self.B, zero
        if op == WRITE:
            if offset + length > self.B:
                return 0, EFBIG, zero
            f[offset:offset + length] = bytes(data[:length])
            return 1, length, zero
        n = 0 if offset >= self.B else min(length, self.B - offset)
        return 1, n, bytes(f[offset:offset + n]) + bytes(128 - n)

    def replay(self, recs):
        """(responses, some) of the records applied in order."""
        resp = np.zeros(len(recs), RESP_DTYPE)
        some = np.zeros(len(recs), np.uint8)
        for i, r in enumerate(recs):
            s, n, d = self.apply(int(r["ino"]), int(r["offset"]), int(r["op"]), int(r["len"]), r["data"].tobytes())
            some[i], resp["n"][i] = s, n
            resp["data"][i] = np.frombuffer(d, np.uint8)
        return resp, some

    def dump(self, ino):
        return bytes(self.data[ino - FIRST_INO])

    def digest(self):
        """(count, sum, xor) of mix64(k ^ mix64(v)) over every aligned 8-byte little-endian word of
        every file, k = file << 32 | word index: written out in plain integers, independent of
        nrgpu.digest."""
        c = s = x = 0
        for f, d in enumerate(self.data):
            for w in range(self.B // 8):
                h = _mix64(((f << 32) | w) ^ _mix64(int.from_bytes(d[8 * w:8 * w + 8], "little")))
                c, s, x = c + 1, (s + h) & _M, x ^ h
        return c, s, x


# ---- records ---------------------------------------------------------------------------------------
def rec(ino, offset, op, length, data=b""):
    r = np.zeros(1, OP_DTYPE)
    r["ino"], r["offset"], r["op"], r["len"] = ino, offset, op, length
    d = bytes(data)[:128]
    r["data"][0, : len(d)] = np.frombuffer(d, np.uint8)
    return r


def W(ino, offset, data):
    return rec(ino, offset, WRITE, len(data), data)


def R(ino, offset, size):
    return rec(ino, offset, READ, size)


def G(ino):
    return rec(ino, 0, GETATTR, 0)


def _pattern(rng, n):
    """n bytes that are neither the initial 0x01 nor zero, so a byte from the wrong place shows."""
    return rng.integers(2, 256, n, dtype=np.uint8).tobytes()


class Stream:
    """A named stream: its geometry, its records and the arms its name promises (`needs`: arm ->
    the least count plan() must report)."""

    def __init__(self, name, files, log2_b, recs, needs, max_batch=None):
        self.name, self.files, self.log2_b = name, files, log2_b
        self.recs = np.concatenate(recs) if isinstance(recs, list) else recs
        self.needs, self.max_batch = needs, max_batch

    def cfg(self, **kw):
        return dict(log2_slots=self.log2_b, queue_capacity=self.files, **kw)

    def plan(self):
        """Which arms of the definition and of the replay plan the records reach, counted from the
        records alone (no file contents): ops by kind and outcome, shapes of the byte ranges against
        the 128-byte lines, and the lengths of the lines' runs in slots."""
        B, F = 1 << self.log2_b, self.files
        a = Counter()
        runs = Counter()
        for r in self.recs:
            ino, off, op, ln = int(r["ino"]), int(r["offset"]), int(r["op"]), int(r["len"])
            if op > GETATTR:
                a["einval_op"] += 1
                continue
            if ln > 128:
                a["einval_len"] += 1
                continue
            if not FIRST_INO <= ino < FIRST_INO + F:
                a["enoent"] += 1
                continue
            if op == GETATTR:
                a["getattr"] += 1
                continue
            if op == WRITE:
                if off + ln > B:
                    a["efbig"] += 1
                    continue
                a["write"] += 1
                cover = ln
            else:
                a["read"] += 1
                cover = 0 if off >= B else min(ln, B - off)
                if off >= B:
                    a["read_past_end"] += 1
                elif cover < ln:
                    a["read_clipped"] += 1
            if ln == 0:
                a["len0"] += 1
            if cover == 0:
                continue
            if cover == 1:
                a["len1"] += 1
            if cover == 128 and off % 2:
                a["len128_odd_offset"] += 1
            if off + cover == B and cover == 128:
                a["last_128_of_file"] += 1
            if off % LINE == 0:
                a["starts_at_line"] += 1
            if (off + cover) % LINE == 0:
                a["ends_at_line"] += 1
            start = (ino - FIRST_INO) * B + off
            first, last = start // LINE, (start + cover - 1) // LINE
            runs[first] += 1
            if last != first:
                a["crosses_line"] += 1
                runs[last] += 1
        lines = F * B // LINE
        a["lines"] = lines
        a["lines_touched"] = len(runs)
        a["lines_empty"] = lines - len(runs)
        a["runs_of_1"] = sum(1 for v in runs.values() if v == 1)
        a["max_run"] = max(runs.values(), default=0)
        a["slots"] = 2 * len(self.recs)
        a["records"] = len(self.recs)
        for v in runs.values():
            a["run_%d" % v] += 1
        return a


# ---- the named streams ------------------------------------------------------------------------------
def memfs_shape(n, seed, files=1, log2_b=12, write_pct=10):
    """generate_fs_operations (benches/memfs.rs:294-322): write_pct % Writes of 128 bytes, Reads of
    0..127 bytes, offsets in 0..B-256, on random files; shuffled. The Writes carry distinct bytes
    (the benchmark's [3; 128] would hide which Write a Read saw)."""
    rng = np.random.default_rng(seed)
    B = 1 << log2_b
    out = []
    for i in range(n):
        ino = FIRST_INO + int(rng.integers(0, files))
        off = int(rng.integers(0, B - 256))
        if i % 100 < write_pct:
            out.append(W(ino, off, _pattern(rng, 128)))
        else:
            out.append(R(ino, off, int(rng.integers(0, 128))))
    order = rng.permutation(n)
    recs = np.concatenate(out)[order]
    return Stream("memfs_shape_%d" % n, files, log2_b, recs, {"records": n})


def one_line(run, seed):
    """One file of 128 bytes: a single line, every op serialises, the run is exactly `run` slots
    (every op covers at least one byte and can touch no second line)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(run):
        off = int(rng.integers(0, 128))
        ln = int(rng.integers(1, 128 - off + 1))
        out.append(W(5, off, _pattern(rng, ln)) if rng.random() < 0.4 else R(5, off, ln))
    return Stream("one_line_%d" % run, 1, 7, out, {"run_%d" % run: 1, "lines": 1, "write": 1, "read": 1})


def three_files(n, seed):
    """3 files of 256 bytes, ops on the three interleaved, many of them crossing the middle line edge."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ino = FIRST_INO + i % 3
        ln = int(rng.integers(0, 129))
        off = int(rng.integers(0, 256 - ln + 1))
        k = rng.random()
        out.append(W(ino, off, _pattern(rng, ln)) if k < 0.45 else (R(ino, off, ln) if k < 0.95 else G(ino)))
    return Stream("three_files", 3, 8, out, {"write": n // 4, "read": n // 4, "getattr": 1, "crosses_line": n // 8,
                                             "lines": 6, "lines_touched": 6})


def thousand_files(n, seed):
    """1000 files of 128 bytes and far fewer ops than lines: most runs are empty or of length 1."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ino = FIRST_INO + int(rng.integers(0, 1000))
        off = int(rng.integers(0, 100))
        ln = int(rng.integers(1, 29))
        out.append(W(ino, off, _pattern(rng, ln)) if i % 2 == 0 else R(ino, off, ln))
    return Stream("thousand_files", 1000, 7, out, {"lines": 1000, "lines_empty": 500, "runs_of_1": 200, "run_2": 10})


def boundaries(seed):
    """2 files of 512 bytes: ops that end exactly at a line boundary, start exactly at one or cross
    one; len 128 at an odd offset, len 1, len 0, the last 128 bytes, a Read clipped to 5 bytes and
    Reads at and past the end; each Write is followed by Reads of its neighbourhood."""
    rng = np.random.default_rng(seed)
    B = 512
    out = []

    def wr(ino, off, ln):
        out.append(W(ino, off, _pattern(rng, ln)))
        lo = max(0, off - 3)
        out.append(R(ino, lo, min(128, ln + 6)))

    for ino in (5, 6):
        wr(ino, 100, 28)        # ends at 128
        wr(ino, 128, 50)        # starts at 128
        wr(ino, 120, 20)        # crosses 128
        wr(ino, 77, 128)        # a full record at an odd offset: two lines, neither whole
        wr(ino, 255, 1)         # one byte, the last of a line
        wr(ino, 256, 1)         # one byte, the first of a line
        wr(ino, 300, 0)         # nothing
        out.append(R(ino, 300, 0))
        wr(ino, B - 128, 128)   # the last line whole
        wr(ino, 256, 128)       # a whole line, aligned
        out.append(R(ino, B - 5, 20))   # n = 5
        out.append(R(ino, B, 20))       # n = 0
        out.append(R(ino, B + 1000, 1))
        out.append(R(ino, 1 << 40, 128))
        out.append(R(ino, 0, 128))
        out.append(R(ino, 127, 2))
        out.append(W(ino, B, b""))      # len 0 at the very end: valid
        out.append(G(ino))
    return Stream("boundaries", 2, 9, out, {"ends_at_line": 4, "starts_at_line": 4, "crosses_line": 4,
                                            "len128_odd_offset": 2, "len1": 4, "len0": 6, "last_128_of_file": 2,
                                            "read_clipped": 2, "read_past_end": 6, "getattr": 2})


def last_writer(n, seed):
    """100 % Writes of one byte range (then one Read of it): the last writer wins."""
    rng = np.random.default_rng(seed)
    out = [W(5, 60, _pattern(rng, 100)) for _ in range(n)]
    out.append(R(5, 60, 100))
    return Stream("last_writer", 1, 8, out, {"write": n, "read": 1, "crosses_line": n, "max_run": n + 1})


def wrwr(pad, seed):
    """One line. `pad` filler ops, then Write, Read, Write, Read of the same bytes: with pad = 10 the
    four sit inside the run's first 64-slot batch, with pad = 62 the batch edge falls between the
    first Read and the second Write."""
    rng = np.random.default_rng(seed)
    out = [R(5, int(rng.integers(0, 100)), 8) if i % 3 else W(5, int(rng.integers(0, 20)), _pattern(rng, 4))
           for i in range(pad)]
    out += [W(5, 40, _pattern(rng, 30)), R(5, 38, 34), W(5, 40, _pattern(rng, 30)), R(5, 38, 34)]
    out += [R(5, 0, 128)]
    s = Stream("wrwr_%d" % pad, 1, 7, out, {"run_%d" % (pad + 5): 1, "write": 2, "read": 3})
    s.tail_at = pad  # slot of the first of the four in the line's run
    return s


def errors(seed, einval=True):
    """2 files of 256 bytes: a valid stream with every error arm mixed in (without the EINVAL records
    if einval is False: then nothing may be latched)."""
    rng = np.random.default_rng(seed)
    bad = [W(5, 200, _pattern(rng, 57)),              # EFBIG: one byte too far
           W(6, 256, _pattern(rng, 1)),               # EFBIG: starts at the end
           W(5, 1 << 33, _pattern(rng, 8)),           # EFBIG: far past the end
           W(5, (1 << 64) - 4, _pattern(rng, 8)),     # EFBIG: offset + len wraps in u64
           W(4, 0, _pattern(rng, 8)), R(7, 0, 8), G(0), R((1 << 64) - 1, 0, 1), W(7 + (1 << 32), 0, b"x")]  # ENOENT
    if einval:
        bad += [rec(5, 0, WRITE, 129, _pattern(rng, 128)), rec(5, 0, READ, 129), rec(5, 0, 3, 8), rec(6, 10, 0xFFFFFFFF, 0),
                rec(5, 0, READ, 0xFFFFFFFF), rec(99, 0, 7, 500)]
    out = []
    for b in bad:  # each bad record between a Write and a Read of bytes it would have touched
        out += [W(5, 0, _pattern(rng, 128)), W(6, 100, _pattern(rng, 100)), b, R(5, 0, 128), R(6, 128, 128), R(5, 190, 66)]
    needs = {"efbig": 4, "enoent": 5, "write": 18, "read": 27}
    if einval:
        needs.update(einval_len=3, einval_op=3)
    return Stream("errors" if einval else "errors_no_einval", 2, 8, out, needs)


def all_streams():
    """Every named stream the GPU test replays, small ones first."""
    s = [boundaries(1), errors(2), errors(3, einval=False), three_files(400, 4), thousand_files(600, 5),
         last_writer(300, 6), wrwr(10, 7), wrwr(62, 8)]
    s += [one_line(r, 10 + r) for r in (63, 64, 65, 128, 129)]
    s += [memfs_shape(n, 100 + n) for n in (1, 2, 255, 256, 257, 1024, 1025, 4097)]
    return s
