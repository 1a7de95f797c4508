"""The snapshot image without a GPU: the library exports the snapshot / restore / resync calls and
refuses a NULL context without touching a device; nrgpu.snapshot packs and unpacks the image of
every flat kind with the header of include/nrgpu.h and nrgpu.digest's triple, refuses what
nrg_snapshot_info_read refuses, and walks a page-table image's leaves."""
import ctypes as C

import numpy as np
import pytest

from nrgpu import _lib as L
from nrgpu import digest, snapshot

MAGIC = int.from_bytes(b"NRGSNAP1", "little")
SYMBOLS = ["nrg_snapshot_size", "nrg_snapshot_async", "nrg_snapshot_info_read", "nrg_restore", "nrg_group_resync"]


def test_symbols_exported_and_null_context_refused():
    import nrgpu

    lib = nrgpu.load()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in L.SIGNATURES
    info = L.SnapshotInfo()
    buf = (C.c_uint8 * 128)()
    assert C.sizeof(L.SnapshotInfo) == 56
    assert lib.nrg_snapshot_size(None, C.byref(info)) == L.NRG_E_INVAL
    assert lib.nrg_snapshot_async(None, buf, 128) == L.NRG_E_INVAL
    assert lib.nrg_snapshot_info_read(None, buf, 128, C.byref(info)) == L.NRG_E_INVAL
    assert lib.nrg_restore(None, buf, 128) == L.NRG_E_INVAL
    assert lib.nrg_group_resync(None, 0) == L.NRG_E_INVAL


def _states():
    rng = np.random.default_rng(7)
    keys = rng.choice(1 << 40, 1500, replace=False).astype(np.uint64)
    keys[17] = 0xFFFFFFFFFFFFFFFF  # the side key is a key like any other in the image
    vals = rng.integers(0, 2**64 - 1, 1500, dtype=np.uint64)
    return {
        "hashmap": (L.NRG_DS_HASHMAP, (keys, vals), digest.pairs(keys, vals), 16),
        "stack": (L.NRG_DS_STACK, rng.integers(0, 2**32 - 1, 50_001, dtype=np.uint32), None, 4),
        "queue": (L.NRG_DS_QUEUE, rng.integers(0, 2**64 - 1, 777, dtype=np.uint64), None, 8),
        "synthetic": (L.NRG_DS_SYNTHETIC, rng.integers(0, 2**64 - 1, 1000, dtype=np.uint64), None, 8),
    }


@pytest.mark.parametrize("name", ["hashmap", "stack", "queue", "synthetic"])
def test_pack_unpack_roundtrip(name):
    kind, state, dg, item = _states()[name]
    if dg is None:
        dg = getattr(digest, name)(state)
    img = snapshot.pack(kind, state, 12345)
    assert img.dtype == np.uint8 and img.size % 64 == 0
    n = len(state[0]) if name == "hashmap" else len(state)
    w = [int(x) for x in img[:64].view("<u8")]
    assert w[0] == MAGIC and bytes(img[:8]) == b"NRGSNAP1"
    assert w[1] == kind | 1 << 32
    assert w[2] == n
    assert w[3] == img.size == (64 + n * item + 63) // 64 * 64
    assert w[4] == 12345
    assert tuple(w[5:8]) == tuple(dg)
    assert not img[64 + n * item:].any()  # zero padding
    info, got = snapshot.unpack(img)
    assert info == snapshot.Info(kind, 1, n, img.size, 12345, tuple(dg))
    if name == "hashmap":
        np.testing.assert_array_equal(got[0], state[0])
        np.testing.assert_array_equal(got[1], state[1])
        info2, got2 = snapshot.unpack(snapshot.pack(kind, dict(zip(state[0].tolist(), state[1].tolist())), 12345))
        assert info2 == info and sorted(zip(got2[0].tolist(), got2[1].tolist())) == sorted(
            zip(state[0].tolist(), state[1].tolist()))
    else:
        assert got.dtype == state.dtype
        np.testing.assert_array_equal(got, state)
    assert snapshot.unpack(img.tobytes())[0] == info  # bytes as read from a file


@pytest.mark.parametrize("name", ["hashmap", "stack", "queue", "synthetic"])
def test_empty_state(name):
    kind = _states()[name][0]
    empty = (np.zeros(0, np.uint64), np.zeros(0, np.uint64)) if name == "hashmap" else np.zeros(0, np.uint64)
    img = snapshot.pack(kind, empty, 0)
    info, got = snapshot.unpack(img)
    assert img.size == 64 and info.items == 0 and info.bytes == 64 and info.digest == (0, 0, 0)
    assert (len(got[0]) if name == "hashmap" else len(got)) == 0


def test_unpack_refuses_bad_headers():
    img = snapshot.pack(L.NRG_DS_STACK, np.arange(100, dtype=np.uint32), 5)

    def words(**kw):
        b = img.copy()
        for i, v in kw.items():
            b[:64].view("<u8")[int(i[1:])] = v
        return b

    snapshot.unpack(img)
    for bad in (words(w0=MAGIC ^ 1), words(w0=0),                       # magic
                words(w1=L.NRG_DS_STACK | 2 << 32),                     # version
                words(w1=99 | 1 << 32), words(w1=0 | 1 << 32),          # kind
                words(w2=113), words(w2=96), words(w3=img.size + 64),  # (97..112 u32 round to these bytes) words(w3=img.size - 64), words(w3=img.size + 1),
                words(w1=L.NRG_DS_QUEUE | 1 << 32),                     # 100 u64 do not take these bytes
                img[:-64], img[:32]):                                   # truncated
        with pytest.raises(ValueError):
            snapshot.unpack(bad)
    with pytest.raises(ValueError):
        snapshot.pack(L.NRG_DS_VSPACE, np.zeros(512, np.uint64), 0)
    with pytest.raises(ValueError):
        snapshot.pack(L.NRG_DS_HASHMAP, ([1, 1], [2, 3]), 0)


def test_vspace_leaves_of_a_hand_built_pool():
    """PML4 (table 0) -> PDPT (table 2) -> PD (table 1) with one 2 MiB leaf: the numbering is not
    the walk's order, and the leaf's vaddr comes from the three slot indices."""
    inner = 1 | 2 | 4
    t = np.zeros((3, 512), np.uint64)
    t[0, 3] = 2 * 4096 | inner
    t[2, 5] = 1 * 4096 | inner
    leaf = 0x40000000 | 1 | 0x80 | 2
    t[1, 7] = leaf
    t[1, 9] = 7 * 4096 | inner  # a PT the image does not hold: skipped
    got = snapshot.leaves(t)
    assert got.dtype == L.VSPACE_LEAF_DTYPE
    assert got.tolist() == [((3 << 39) | (5 << 30) | (7 << 21), leaf)]
    # the same through an image's bytes
    img = np.zeros(64 + 3 * 4096, np.uint8)
    dg = digest.vspace(got["vaddr"], got["entry"])
    img[:64].view("<u8")[:] = [MAGIC, L.NRG_DS_VSPACE | 1 << 32, 3, img.size, 9, *dg]
    img[64:].view("<u8")[:] = t.reshape(-1)
    info, tables = snapshot.unpack(img)
    assert info.items == 3 and info.log_idx == 9 and tables.shape == (3, 512)
    np.testing.assert_array_equal(snapshot.leaves(tables), got)
    assert snapshot.leaves(np.zeros((1, 512), np.uint64)).size == 0
