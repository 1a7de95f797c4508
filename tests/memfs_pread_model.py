"""Model of the file store's read-only reads (include/nrgpu.h nrg_memfs_pread*) and the named
request lists the CPU and GPU tests share.

pread() is the definition read literally over a MemFsModel's files: request i answers some[i] and
count_i bytes, the bytes are concatenated in request order, offs is the running sum, and a cap cuts
the concatenation. Nothing of the GPU's plan appears in it. plan() does know the copy kernel's plan
(the packed output cut into tiles of `tile` bytes, each tile into aligned 16-byte chunks), so that a
request list named for an arm of the kernels can say on the CPU whether it still reaches it.
"""
from collections import Counter

import numpy as np

from memfs_model import FIRST_INO

RD_DTYPE = np.dtype([("ino", "<u8"), ("offset", "<u8"), ("len", "<u8")])
U64_MAX = (1 << 64) - 1


def reqs(items):
    """[(ino, offset, len), ...] -> an array of RD_DTYPE."""
    r = np.zeros(len(items), RD_DTYPE)
    for i, (ino, off, ln) in enumerate(items):
        r[i] = (ino, off, ln)
    return r


def counts(rq, files, B):
    """(count, some) of every request."""
    ino, off, ln = rq["ino"], rq["offset"], rq["len"]
    some = (ino >= np.uint64(FIRST_INO)) & (ino < np.uint64(FIRST_INO + files))
    left = np.uint64(B) - np.minimum(off, np.uint64(B))  # 0 at and past the end
    return np.where(some, np.minimum(ln, left), np.uint64(0)).astype(np.uint64), some.astype(np.uint8)


def pread(model, rq, cap=None):
    """(data, offs, some): data holds the first min(cap, total) packed bytes; offs[n] is the total."""
    cnt, some = counts(rq, model.files, model.B)
    offs = np.zeros(len(rq) + 1, np.uint64)
    offs[1:] = np.cumsum(cnt, dtype=np.uint64)
    total = int(offs[-1])
    end = total if cap is None else min(int(cap), total)
    store = np.frombuffer(b"".join(bytes(d) for d in model.data), np.uint8)
    # packed byte q of request i is the store's byte src_i + (q - offs[i])
    src = (rq["ino"] - np.uint64(FIRST_INO)) * np.uint64(model.B) + rq["offset"]
    keep = cnt > 0
    delta = (src[keep] - offs[:-1][keep]).astype(np.int64)  # (wraps where offs is larger: int64 undoes it)
    idx = np.repeat(delta, cnt[keep].astype(np.int64)) + np.arange(total, dtype=np.int64)
    return store[idx[:end]], offs, some


def plan(rq, files, log2_b, tile, cap=None):
    """Which arms the requests reach, counted from the requests alone: outcomes of the clip, the
    requests per tile and tiles per request, where requests end against the tile edges, runs of
    requests without bytes, and how the 16-byte chunks of the output fall (inside one request: the
    wide path, with the source's misalignment against the chunk's; otherwise byte by byte). `pairs`
    is the set of (source address mod 16, packed position mod 16, length) of the requests with bytes."""
    B = 1 << log2_b
    cnt, some = counts(rq, files, B)
    n = len(rq)
    offs = [0]
    for c in cnt:
        offs.append(offs[-1] + int(c))
    total = offs[-1]
    end = total if cap is None else min(int(cap), total)
    a = Counter(requests=n, total=total, end=end, tiles=-(-end // tile))
    pairs = set()
    per_tile = Counter()
    run = 0
    for i, r in enumerate(rq):
        ino, off, ln, c = int(r["ino"]), int(r["offset"]), int(r["len"]), int(cnt[i])
        if not some[i]:
            a["enoent"] += 1
        elif off >= B:
            a["past_end"] += 1
        elif c < ln:
            a["clipped"] += 1
        if some[i] and ln == 0:
            a["len0"] += 1
        if c == 0:
            run += 1
            a["max_zero_run"] = max(a["max_zero_run"], run)
            if 0 < offs[i] < end and offs[i] % tile == 0:
                a["zero_at_tile_edge"] += 1  # the run it belongs to sits on a tile boundary
            if i == 0:
                a["zero_first"] += 1
            if i == n - 1:
                a["zero_last"] += 1
            continue
        run = 0
        lo, hi = offs[i], offs[i + 1]
        src = (ino - FIRST_INO) * B + off
        pairs.add((src % 16, lo % 16, c))
        if lo >= end:
            a["wholly_past_cap"] += 1
            continue
        if hi > end:
            a["cut_by_cap"] += 1
            hi = end
        for k in (-1, 0, 1):
            if hi > 1 and (hi - k) % tile == 0:
                a["ends_at_T%+d" % k if k else "ends_at_T"] += 1
        t0, t1 = lo // tile, (hi - 1) // tile
        a["max_tiles_per_req"] = max(a["max_tiles_per_req"], t1 - t0 + 1)
        if t1 - t0 + 1 >= 3 and (lo % 16 or src % 16):
            a["spans_3_tiles_misaligned"] += 1
        for t in range(t0, t1 + 1):
            per_tile[t] += 1
        # the 16-byte chunks that lie wholly inside this request take the wide path
        c0, c1 = -(-lo // 16), hi // 16
        if c1 > c0:
            a["wide_chunks"] += c1 - c0
            a["wide_shift_%d" % ((src + c0 * 16 - lo) % 16)] += 1
    a["byte_chunks"] = -(-end // 16) - a["wide_chunks"]
    a["max_reqs_in_tile"] = max(per_tile.values(), default=0)
    a["tiles_gt_64_reqs"] = sum(1 for v in per_tile.values() if v > 64)
    a["tiles_gt_1024_reqs"] = sum(1 for v in per_tile.values() if v > 1024)
    a["pairs"] = pairs
    return a


# ---- the named request lists -------------------------------------------------------------------------
class Reads:
    """A named request list: its geometry, the requests and the arms its name promises (`needs`: arm ->
    the least count plan() must report)."""

    def __init__(self, name, files, log2_b, rq, needs, cap=None):
        self.name, self.files, self.log2_b, self.needs, self.cap = name, files, log2_b, needs, cap
        self.rq = rq if isinstance(rq, np.ndarray) else reqs(rq)

    def plan(self, tile):
        return plan(self.rq, self.files, self.log2_b, tile, self.cap)


EDGE_LENS = (0, 1, 127, 128, 129, 255, 256, 257, U64_MAX)
EDGE_OFFS = (0, 1, 255, 256, 257, 1 << 33, U64_MAX)
EDGE_INOS = (4, 5, 6, 7, U64_MAX)
ALIGN_LENS = (1, 15, 16, 17, 31, 32, 33)


def edges():
    """2 files of 256 bytes: every (ino, offset, len) of the three edge lists."""
    rq = [(i, o, ln) for i in EDGE_INOS for o in EDGE_OFFS for ln in EDGE_LENS]
    return Reads("edges", 2, 8, rq, {"enoent": 3 * 63, "past_end": 2 * 4 * 9, "clipped": 20, "len0": 2 * 7,
                                     "max_zero_run": 63})


def alignment(lead):
    """One file of 4096 bytes. A leading request of `lead` bytes, then for every source misalignment s
    and every length of ALIGN_LENS a request at a source address = s mod 16, followed by a filler that
    brings the packed position back to `lead` mod 16: over lead = 0..15 every (source mod 16, packed
    mod 16, length) is reached. Then 16 longer requests, one per source misalignment."""
    rq = [(5, 3, lead)]
    k = 0
    for s in range(16):
        for ln in ALIGN_LENS:
            rq.append((5, 16 * (k % 250) + s, ln))
            rq.append((5, 7 * k % 4000, -ln % 16))
            k += 1
    for s in range(16):  # and one long enough for whole chunks: the wide path at every byte shift
        rq.append((5, 160 * s + s, 64 + s))
    return Reads("alignment_%d" % lead, 1, 12, rq, {"requests": 1 + 2 * 16 * 7 + 16, "wide_chunks": 16 * 3})


def tile_edges(T):
    """One file of 4T bytes: requests ending at T - 1, T and T + 1, one spanning three tiles from a
    misaligned start, a tile of more than 1024 one-byte requests and one of more than 64, 300
    requests without bytes (empty and unknown inos alternating) on a tile boundary, and an empty
    request first and last."""
    B = 4 * T
    rq = [(5, 9, 0)]                                   # empty, first
    rq += [(5, 100, T - 1)]                            # packed [0, T - 1)
    rq += [(5, 5, 1)]                                  # ends at T
    rq += [(5, 77, T + 1)]                             # [T, 2T + 1): ends at T + 1 of its tile
    rq += [(5, 3 * T - 7, 0), (9, 0, 50)] * 2          # a short run inside a tile
    rq += [(5, T - 5, 3 * T)]                          # [2T + 1, 5T + 1): three tiles and more, misaligned
    rq += [(5, 31 * i % B, 1) for i in range(T - 1)]   # one-byte requests up to 6T: a tile of > 1024
    assert T >= 2048
    rq += [(5, 13, 0), (3, 0, 9)] * 150                # 300 without bytes, exactly at 6T
    rq += [(5, 1000 + i, 1) for i in range(100)]       # > 64 in the next tile
    rq += [(5, 0, B)]                                  # the whole file
    rq += [(5, B, 1)]                                  # empty (past the end), last
    return Reads("tile_edges", 1, (4 * T).bit_length() - 1, rq,
                 {"ends_at_T-1": 1, "ends_at_T": 1, "ends_at_T+1": 1, "spans_3_tiles_misaligned": 1, "tiles_gt_64_reqs": 2,
                  "tiles_gt_1024_reqs": 1, "max_zero_run": 300, "zero_at_tile_edge": 300, "zero_first": 1, "zero_last": 1,
                  "enoent": 152})


def skew(big_first, seed=5):
    """One file of 1 MiB: one whole-file read beside 4096 reads of 0..3 bytes."""
    rng = np.random.default_rng(seed)
    small = [(5, int(rng.integers(0, 1 << 20)), int(rng.integers(0, 4))) for _ in range(4096)]
    big = [(5, 0, 1 << 20)]
    return Reads("skew_big_%s" % ("first" if big_first else "last"), 1, 20, big + small if big_first else small + big,
                 {"max_tiles_per_req": 64, "tiles_gt_1024_reqs": 1, "len0": 500, "requests": 4097})


def nrfs_shape(files=64, seed=6):
    """benches/nrfs.rs: files of 4096 bytes, every file read whole, in a shuffled order."""
    order = np.random.default_rng(seed).permutation(files)
    return Reads("nrfs_shape", files, 12, [(FIRST_INO + int(f), 0, 4096) for f in order],
                 {"total": files * 4096, "wide_chunks": files * 256, "requests": files})


def all_reads(T):
    return [edges()] + [alignment(d) for d in range(16)] + [tile_edges(T), skew(True), skew(False), nrfs_shape()]
