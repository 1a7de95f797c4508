"""Model of the file store's logged reads of any length (include/nrgpu.h, nrg_memfs_pread_logged*) and
the request lists the CPU and GPU tests share.

Three things, written from the header and none by calling the library:
  pread_at()  the definition read literally, on byte arrays: request i reads min(len, A - offset) bytes
              of file `ino` from `offset`, clipped at the file's size (B in an unsized store);
  cut()       the 128-byte Read records a call logs: one per line of what the request plans to read, or
              the single record of a request that names no file or plans no bytes, with first[], offs[],
              planned and some;
  fold()      the way back: the fragments' responses to (count, bytes) per request.
The records go to the sequential models of the replay (memfs_model.MemFsModel, memfs_size_model.
SizedModel, memfs_grow_model.GrowModel), which know nothing of requests: that their folded answers equal
pread_at()'s is the cut's proof.
"""
import numpy as np

import memfs_model as M

RD_DTYPE = np.dtype([("ino", "<u8"), ("offset", "<u8"), ("len", "<u8")])
FIRST_INO, ENOENT, LINE = M.FIRST_INO, M.ENOENT, M.LINE
U64 = (1 << 64) - 1
GUARD = 0xA5  # what the tests fill `data` with before a call: the store's 0x01, the sized zero and
              # the patterns below never produce it


def reqs(items):
    """[(ino, offset, len), ...] as an array of RD_DTYPE."""
    a = np.zeros(len(items), RD_DTYPE)
    for i, (ino, off, ln) in enumerate(items):
        a["ino"][i], a["offset"][i], a["len"][i] = ino, off, ln
    return a


def plan_one(r, files, A):
    """(some, planned) of one request, checked in the replay's order: the ino, then the range."""
    ino, off, ln = int(r["ino"]), int(r["offset"]), int(r["len"])
    if not FIRST_INO <= ino < FIRST_INO + files:
        return 0, 0
    if ln == 0 or off >= A:
        return 1, 0
    return 1, min(ln, A - off)  # (Python integers: no overflow)


def pread_at(store, sizes, rq, files, A):
    """The answers of the requests against `store` (a bytes-like per file; `sizes` a list, or None for
    an unsized store whose files end at len(store[f])): (some, planned, [bytes per request])."""
    some = np.zeros(len(rq), np.uint8)
    planned = np.zeros(len(rq), np.uint64)
    out = []
    for i, r in enumerate(rq):
        some[i], p = plan_one(r, files, A)
        planned[i] = p
        b = b""
        if p:
            f, off = int(r["ino"]) - FIRST_INO, int(r["offset"])
            size = len(store[f]) if sizes is None else sizes[f]
            b = bytes(store[f][off:min(off + p, max(size, off))])
        out.append(b)
    return some, planned, out


def cut(rq, files, A):
    """(records, first, offs, planned, some): what one call logs and where its answers go."""
    out, first, offs = [], [0], [0]
    some = np.zeros(len(rq), np.uint8)
    planned = np.zeros(len(rq), np.uint64)
    for i, r in enumerate(rq):
        ino, off = int(r["ino"]), int(r["offset"])
        some[i], p = plan_one(r, files, A)
        planned[i] = p
        if p == 0:
            out.append(M.R(ino, off, 0))
        else:
            # the cuts: the range's ends and every multiple of 128 strictly between them
            edges = [off] + list(range((off // LINE + 1) * LINE, off + p, LINE)) + [off + p]
            for lo, hi in zip(edges[:-1], edges[1:]):
                out.append(M.R(ino, lo, hi - lo))
        first.append(len(out))
        offs.append(offs[-1] + p)
    recs = np.concatenate(out) if out else np.zeros(0, M.OP_DTYPE)
    return recs, np.array(first, np.uint64), np.array(offs, np.uint64), planned, some


def fold(rq, first, resp, rsome):
    """(some, count, [bytes per request]) from the responses of a call's records: some from the first
    fragment, each fragment's data[:n] concatenated (a request that names no file has no bytes)."""
    n = len(rq)
    some = np.zeros(n, np.uint8)
    count = np.zeros(n, np.uint64)
    out = []
    for i in range(n):
        lo, hi = int(first[i]), int(first[i + 1])
        some[i] = rsome[lo]
        b = b""
        if some[i]:
            b = b"".join(resp["data"][t][: int(resp["n"][t])].tobytes() for t in range(lo, hi))
        count[i] = len(b)
        out.append(b)
    return some, count, out


def expected_data(cap, offs, chunks):
    """`data` after a call into a buffer of cap GUARD bytes: request i's bytes at offs[i], nothing else."""
    d = np.full(cap, GUARD, np.uint8)
    for i, b in enumerate(chunks):
        o = int(offs[i])
        d[o:o + len(b)] = np.frombuffer(b, np.uint8)
    return d


def pattern(n, seed):
    """n bytes, none of them the store's 0x01, 0 nor GUARD."""
    v = np.random.default_rng(seed).integers(2, 255, n, dtype=np.uint16).astype(np.uint8)
    v[v == GUARD] = 0x5A
    return v


def edges(files, B):
    """The edge list of the feature, for `files` (>= 3) files of B bytes."""
    F = FIRST_INO
    v = [(F, 0, 0), (F, 0, 1), (F, B - 1, 1)]
    for off in (0, 1, 127, 128):
        v += [(F + 1, off % B, ln) for ln in (127, 128, 129)]
    v += [(F + 2, 100 % B, 128),            # across two lines (one when B = 128: clipped)
          (F + 2, 60 % B, 300),             # across three
          (F, 0, B),                        # the whole file
          (F + 1, 0, U64),                  # read to the end
          (4, 0, 10),                       # an ino below the first, between valid requests
          (F + 2, 67 % B, U64),             # read to the end from the middle of a line
          (F, B, 5), (F, B + 1, 5), (F, 1 << 63, U64), (F, U64, U64),
          (F + files, 3, 10),               # an ino above the last
          (F + 1, 40 % B, 200), (F + 1, 40 % B, 200)]  # the same range twice
    return reqs(v)
