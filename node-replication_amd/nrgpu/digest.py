"""The state digest of nrg_digest / nrg_group_verify (include/nrgpu.h), mirrored in numpy.

A replica's digest is the triple (count, sum, xor) over the structure's items of
h = mix64(k ^ mix64(v)), the sum wrapping in u64. What (k, v) is depends on the kind:

  hashmap    (key, value)
  stack      (index from the bottom, element)
  queue      (index from the front, element)
  synthetic  (word index, word)
  vspace     (the leaf's first virtual address, the leaf entry)
  skip list  (key, value), the hashmap's definition
  file store (file index << 32 | word index, the word) over every aligned 8-byte word of every file

With these a caller that holds a host snapshot or a CPU model of the structure computes the triple
the device must report, without the device's state ever leaving the GPU.
"""
from __future__ import annotations

import numpy as np

_U64 = np.uint64


def mix64(a) -> np.ndarray:
    """The splitmix64 finaliser (csrc/common.hpp mix64, oracle orc_mix64), elementwise on u64."""
    z = np.array(a, dtype=_U64, copy=True)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
        return z ^ (z >> _U64(31))


def pairs(keys, vals):
    """(count, sum, xor) of mix64(k ^ mix64(v)) over the (k, v) pairs, as three Python ints."""
    k = np.ascontiguousarray(np.asarray(keys, dtype=_U64)).reshape(-1)
    v = np.ascontiguousarray(np.asarray(vals, dtype=_U64)).reshape(-1)
    if k.shape != v.shape:
        raise ValueError("keys and vals differ in length")
    if k.size == 0:
        return (0, 0, 0)
    h = mix64(k ^ mix64(v))
    with np.errstate(over="ignore"):
        s = np.add.reduce(h, dtype=_U64)
    return (int(k.size), int(s), int(np.bitwise_xor.reduce(h)))


def _positional(values):
    v = np.asarray(values, dtype=_U64).reshape(-1)
    return pairs(np.arange(v.size, dtype=_U64), v)


def stack(values):
    """A stack holding `values`, bottom first."""
    return _positional(values)


def queue(values_front_first):
    """A queue holding these values, front first."""
    return _positional(values_front_first)


def synthetic(words):
    """The synthetic structure's words, in index order."""
    return _positional(words)


def vspace(vaddrs, entries):
    """A page table's leaves: each leaf's first virtual address (raw, bits 48..63 clear) and its
    entry, in any order."""
    return pairs(vaddrs, entries)


def skiplist(keys, vals):
    """An ordered map's (key, value) pairs, in any order: the hashmap's triple for the same pairs."""
    return pairs(keys, vals)


def memfs(files, sizes=None):
    """A file store's files in inode order, each a bytes-like of the same length B (a multiple of
    8): the items are the aligned little-endian 8-byte words, keyed (file index << 32 | word index).
    sizes: a sized context's (nrg_memfs_enable_sizes) file sizes, one more item per file, keyed
    (file index << 32 | 0xFFFFFFFF); `files` are still the B stored bytes, zero at and past the size."""
    keys, vals = [], []
    for f, data in enumerate(files):
        w = np.frombuffer(bytes(data), dtype="<u8")
        keys.append((_U64(f) << _U64(32)) | np.arange(w.size, dtype=_U64))
        vals.append(w)
    if sizes is not None:
        if len(sizes) != len(files):
            raise ValueError("one size per file")
        keys.append((np.arange(len(files), dtype=_U64) << _U64(32)) | _U64(0xFFFFFFFF))
        vals.append(np.asarray(sizes, dtype=_U64))
    if not keys:
        return (0, 0, 0)
    return pairs(np.concatenate(keys), np.concatenate(vals))


def combine(triples):
    """The digest of a structure split into disjoint parts (a partitioned group's members): counts
    and sums add, xors xor."""
    c = s = x = 0
    for t in triples:
        c += int(t[0])
        s = (s + int(t[1])) & 0xFFFFFFFFFFFFFFFF
        x ^= int(t[2])
    return (c, s, x)
