"""The snapshot image of nrg_snapshot_async / nrg_restore (include/nrgpu.h), in numpy.

One buffer, the same on the device, on the host and on disk: a 64-byte header of eight
little-endian u64 words

  0     magic, the ASCII bytes NRGSNAP1
  1     ds_kind | version << 32
  2     items
  3     bytes = 64 + payload, rounded up to a multiple of 64 (zero padding)
  4     log_idx: the state is the replay of [0, log_idx)
  5-7   the nrg_digest triple (count, sum, xor) of the state

and the payload: hashmap `items` {key, value} records in any order; stack `items` u32, bottom
first; queue `items` u64, front first; synthetic synth_n u64 words; vspace the `items` allocated
pool tables of 512 u64, inner entries as stored (table_index * 4096 | flags); skip list `items`
{key, value} records in strictly ascending key order; file store `items` = F * B / 8 u64 words, the
files' bytes in inode order, and from a sized context (nrg_memfs_enable_sizes) the F sizes as u64
after them, `items` = F * B / 8 + F (memfs_split() tells the two apart).

unpack() reads an image of any kind; pack() builds one for the four flat kinds from a host model,
its digest words from nrgpu.digest, so that a model can seed a GPU replica (DeviceReplica.restore).
Needs no GPU and no library.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from . import _lib as L
from . import digest as _digest

MAGIC = int.from_bytes(b"NRGSNAP1", "little")
VERSION = 1
HEADER_BYTES = 64

Info = namedtuple("Info", "ds_kind version items bytes log_idx digest")

_ITEM_BYTES = {L.NRG_DS_HASHMAP: 16, L.NRG_DS_STACK: 4, L.NRG_DS_SYNTHETIC: 8, L.NRG_DS_QUEUE: 8,
               L.NRG_DS_VSPACE: 4096, L.NRG_DS_SKIPLIST: 16, L.NRG_DS_MEMFS: 8}
_ADDR = 0x000FFFFFFFFFF000  # x86 ADDRESS_MASK: bits 12..51


def as_u8(buf) -> np.ndarray:
    """An image held as bytes or as an array of any dtype, as a flat u8 array."""
    b = np.frombuffer(buf, np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else np.asarray(buf)
    return np.ascontiguousarray(b).view(np.uint8).reshape(-1)


def image_bytes(kind: int, items: int) -> int:
    """Header word 3 of an image of `items` items."""
    return (HEADER_BYTES + items * _ITEM_BYTES[kind] + 63) & ~63


def header(buf) -> Info:
    """The validated header of the image in `buf` (u8 array or bytes), as nrg_snapshot_info_read
    validates it; ValueError otherwise."""
    b = as_u8(buf)
    if b.size < HEADER_BYTES:
        raise ValueError("snapshot: shorter than its header")
    h = [int(x) for x in b[:HEADER_BYTES].view("<u8")]
    if h[0] != MAGIC:
        raise ValueError("snapshot: bad magic")
    kind, version = h[1] & 0xFFFFFFFF, h[1] >> 32
    if version != VERSION:
        raise ValueError(f"snapshot: version {version}, not {VERSION}")
    if kind not in _ITEM_BYTES:
        raise ValueError(f"snapshot: unknown kind {kind}")
    items = h[2]
    if items > 1 << 40 or h[3] != image_bytes(kind, items):
        raise ValueError(f"snapshot: {h[3]} bytes do not hold {items} items of kind {kind}")
    if h[3] > b.size:
        raise ValueError(f"snapshot: truncated ({b.size} of {h[3]} bytes)")
    return Info(kind, version, items, h[3], h[4], (h[5], h[6], h[7]))


def unpack(buf):
    """(info, state) of an image: hashmap (keys, vals) u64 arrays in the image's order; stack a u32
    array, bottom first; queue a u64 array, front first; synthetic the u64 words; vspace the pool
    tables, a u64 array [items, 512] (leaves() walks it); file store the files' bytes in inode order
    as one u8 array (the image does not carry the geometry: reshape it to [F, B])."""
    info = header(buf)
    b = as_u8(buf)
    pay = b[HEADER_BYTES:HEADER_BYTES + info.items * _ITEM_BYTES[info.ds_kind]]
    k = info.ds_kind
    if k in (L.NRG_DS_HASHMAP, L.NRG_DS_SKIPLIST):  # (the skip list's in ascending key order)
        r = pay.view("<u8").reshape(-1, 2)
        return info, (r[:, 0].copy(), r[:, 1].copy())
    if k == L.NRG_DS_STACK:
        return info, pay.view("<u4").copy()
    if k == L.NRG_DS_VSPACE:
        return info, pay.view("<u8").reshape(-1, 512).copy()
    if k == L.NRG_DS_MEMFS:
        return info, pay.copy()
    return info, pay.view("<u8").copy()  # queue, synthetic


def memfs_split(data, files: int):
    """The payload of a file-store image (unpack's u8 array) of `files` files: (bytes, sizes) with
    bytes a u8 array [F, B] and sizes a u64 array [F], or None for an unsized image. B is a power
    of two, so F * B and F * B + 8 F cannot be confused; ValueError if the payload is neither."""
    d = as_u8(data)
    per, rem = divmod(d.size, files)
    for b, sized in ((per, False), (per - 8, True)):
        if rem == 0 and b >= 128 and b & (b - 1) == 0:
            body = d[:files * b].reshape(files, b).copy()
            return body, (d[files * b:].view("<u8").copy() if sized else None)
    raise ValueError(f"snapshot: {d.size} bytes are not {files} files of a power-of-two size")


def leaves(tables) -> np.ndarray:
    """nrg_vspace_dump's list from the pool tables of a vspace image: every leaf entry as
    (vaddr, entry), in ascending vaddr. Slots are walked in index order from the PML4 (table 0)
    down, so nothing depends on the order in which the tables were allocated; an inner entry whose
    table index is not in the image is skipped."""
    t = np.asarray(tables, dtype=np.uint64).reshape(-1, 512)
    out = []

    def walk(tab, level, va):
        for i in np.flatnonzero(t[tab] & np.uint64(1)):
            e = int(t[tab, i])
            v = va | (int(i) << (12 + 9 * level))
            if level == 0 or (level == 1 and e & 0x80):
                out.append((v, e))
            else:
                nxt = (e & _ADDR) >> 12
                if nxt < len(t):
                    walk(nxt, level - 1, v)

    if len(t):
        walk(0, 3, 0)
    return np.array(out, dtype=L.VSPACE_LEAF_DTYPE)


def pack(kind: int, state, log_idx: int, sizes=None) -> np.ndarray:
    """The image (u8 array) of a host model's state after replaying [0, log_idx): hashmap a
    (keys, vals) pair or a dict; stack the elements, bottom first; queue the elements, front first;
    synthetic the words; skip list as the hashmap (the records are written in ascending key order);
    file store the files in inode order, each a bytes-like of the same length (the B stored bytes),
    with sizes= one size per file for a sized image.
    The digest words are nrgpu.digest's."""
    if kind in (L.NRG_DS_HASHMAP, L.NRG_DS_SKIPLIST):
        if isinstance(state, dict):
            keys, vals = list(state.keys()), list(state.values())
        else:
            keys, vals = state
        keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
        vals = np.asarray(vals, dtype=np.uint64).reshape(-1)
        if keys.shape != vals.shape:
            raise ValueError("keys and vals differ in length")
        if np.unique(keys).size != keys.size:
            raise ValueError("a key appears twice")
        if kind == L.NRG_DS_SKIPLIST:
            order = np.argsort(keys, kind="stable")
            keys, vals = keys[order], vals[order]
        pay = np.stack([keys, vals], 1).astype("<u8").view(np.uint8).reshape(-1)
        items, dg = keys.size, _digest.pairs(keys, vals)
    elif kind == L.NRG_DS_STACK:
        v = np.asarray(state, dtype=np.uint32).reshape(-1)
        pay, items, dg = v.astype("<u4").view(np.uint8), v.size, _digest.stack(v)
    elif kind in (L.NRG_DS_QUEUE, L.NRG_DS_SYNTHETIC):
        v = np.asarray(state, dtype=np.uint64).reshape(-1)
        pay, items = v.astype("<u8").view(np.uint8), v.size
        dg = _digest.queue(v) if kind == L.NRG_DS_QUEUE else _digest.synthetic(v)
    elif kind == L.NRG_DS_MEMFS:
        files = [bytes(f) for f in state]
        if not files or len({len(f) for f in files}) != 1 or len(files[0]) % 8:
            raise ValueError("files of one length, a multiple of 8")
        pay = np.frombuffer(b"".join(files), np.uint8)
        if sizes is not None:
            pay = np.concatenate([pay, np.asarray(sizes, dtype="<u8").reshape(len(files)).view(np.uint8)])
        items, dg = pay.size // 8, _digest.memfs(files, sizes)
    else:
        raise ValueError(f"pack: kind {kind} has no flat state")
    nbytes = image_bytes(kind, items)
    out = np.zeros(nbytes, np.uint8)
    out[:HEADER_BYTES].view("<u8")[:] = [MAGIC, kind | VERSION << 32, items, nbytes, log_idx, *dg]
    out[HEADER_BYTES:HEADER_BYTES + pay.size] = pay
    return out
