"""Model of the file store's logged writes of any length (include/nrgpu.h, nrg_memfs_pwrite*) and the
request lists the CPU and GPU tests share.

Two things, both written from the header and neither by calling the library:
  pwrite()  the definition read literally, on byte arrays: request i writes data[data_off, data_off +
            len) to file `ino` at `offset`, whole or not at all, the requests applied in order;
  cut()     the 128-byte Write records a call logs: one per line the request touches, or the single
            record of a request that fails or has no bytes, with first[], written and some.
The records go to the sequential models of the replay (memfs_model.MemFsModel, memfs_size_model.
SizedModel), which know nothing of requests: that their files equal pwrite()'s is the cut's proof.
"""
import numpy as np

import memfs_model as M

WR_DTYPE = np.dtype([("ino", "<u8"), ("offset", "<u8"), ("len", "<u8"), ("data_off", "<u8")])
FIRST_INO, ENOENT, EFBIG, LINE = M.FIRST_INO, M.ENOENT, M.EFBIG, M.LINE


def reqs(items):
    """[(ino, offset, len, data_off), ...] as an array of WR_DTYPE."""
    a = np.zeros(len(items), WR_DTYPE)
    for i, (ino, off, ln, doff) in enumerate(items):
        a["ino"][i], a["offset"][i], a["len"][i], a["data_off"][i] = ino, off, ln, doff
    return a


def answer(r, files, B):
    """(some, written) of one request, checked in the replay's order: the ino, then the range."""
    ino, off, ln = int(r["ino"]), int(r["offset"]), int(r["len"])
    if not FIRST_INO <= ino < FIRST_INO + files:
        return 0, ENOENT
    if off + ln > B:  # (Python integers: no overflow)
        return 0, EFBIG
    return 1, ln


def pwrite(store, sizes, rq, data, files, B):
    """The requests applied in order to `store` (a bytearray per file) as whole pwrites; `sizes` (a
    list, or None for an unsized store) grows as POSIX says. Returns (written, some)."""
    written = np.zeros(len(rq), np.uint64)
    some = np.zeros(len(rq), np.uint8)
    for i, r in enumerate(rq):
        some[i], written[i] = answer(r, files, B)
        ln = int(r["len"])
        if some[i] and ln:
            f, off, doff = int(r["ino"]) - FIRST_INO, int(r["offset"]), int(r["data_off"])
            store[f][off:off + ln] = bytes(data[doff:doff + ln])
            if sizes is not None:
                sizes[f] = max(sizes[f], off + ln)
    return written, some


def cut(rq, data, files, B):
    """(records, first, written, some): what one call logs. A request that fails logs one record the
    replay answers with the same error; one of no bytes logs {ino, offset, WRITE, 0}."""
    out, first = [], [0]
    written = np.zeros(len(rq), np.uint64)
    some = np.zeros(len(rq), np.uint8)
    for i, r in enumerate(rq):
        ino, off, ln, doff = int(r["ino"]), int(r["offset"]), int(r["len"]), int(r["data_off"])
        some[i], written[i] = answer(r, files, B)
        if not some[i]:
            out.append(M.rec(ino, B, M.WRITE, 1) if written[i] == EFBIG else M.rec(ino, off, M.WRITE, 0))
        elif ln == 0:
            out.append(M.rec(ino, off, M.WRITE, 0))
        else:
            # the cuts: the request's ends and every multiple of 128 strictly between them
            edges = [off] + list(range((off // LINE + 1) * LINE, off + ln, LINE)) + [off + ln]
            for lo, hi in zip(edges[:-1], edges[1:]):
                out.append(M.W(ino, lo, bytes(data[doff + lo - off:doff + hi - off])))
        first.append(len(out))
    recs = np.concatenate(out) if out else np.zeros(0, M.OP_DTYPE)
    return recs, np.array(first, np.uint64), written, some


def pattern(n, seed):
    """n bytes, none of them the store's 0x01 nor 0."""
    return (np.random.default_rng(seed).integers(2, 256, n, dtype=np.uint16)).astype(np.uint8)


def edges(files, B, data_bytes):
    """The edge list of the feature, for `files` files of B bytes over data_bytes (>= 4200) bytes of data."""
    F = FIRST_INO
    v = [(F, 0, 0, 0), (F, 9, 1, 5), (F, 0, 128, 3), (F + 1, 0, B, 0)]  # len 0, 1, 128, a whole file
    if B >= 512:
        v += [(F, 1, 128, 7), (F, 127, 2, 9), (F + 2, 100, 300, 11)]  # the last: 28 / 128 / 128 / 16
    v += [(F, B - 77, 77, 1),      # ends exactly at B
          (F, B, 0, 0),            # valid
          (F, B - 1, 2, 0),        # offset + len = B + 1: EFBIG
          (F, B + 1, 0, 0),        # EFBIG
          (F, 1 << 63, 1 << 63, 0),  # EFBIG, and no overflow
          (4, 0, 10, 1 << 60),     # ENOENT; a failing request's data_off is not looked at
          (F + files, 3, 10, 0)]   # ENOENT
    v += [(F + a % files, (a * 37) % (B - 40), 33 + a % 7, 32 + a) for a in range(16)]  # data_off & 15: every value
    v += [(F, 5, 40, data_bytes - 40),  # a fragment that ends on the last byte of data
          (F + 1, 10, 50, 64), (F + 2, 20, 50, 64),  # two requests share one data_off
          (F + 1, 30, 60, 200)]    # overlaps (F + 1, 10, 50): the later wins
    return reqs(v)
