"""The file store without a GPU: the sequential model (tests/memfs_model.py) against answers written
out by hand, the ABI side (kind, defaults, struct sizes, symbols), the numpy mirrors of the digest
and the snapshot image, and every named stream's plan(): a stream that stops reaching the arm it is
named for fails here, instead of passing vacuously on the GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import memfs_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nrgpu_mod():
    import nrgpu

    nrgpu.load()
    return nrgpu


# ---- the model against hand-written answers ---------------------------------------------------------
def test_initial_file_is_4096_ones():
    m = M.MemFsModel()
    assert m.files == 1 and m.B == 4096
    assert m.dump(5) == b"\x01" * 4096
    assert m.apply(5, 0, M.GETATTR, 0) == (1, 4096, bytes(128))


def test_write_then_read_sees_it_and_a_read_logged_before_does_not():
    m = M.MemFsModel()
    before = m.apply(5, 90, M.READ, 20)  # logged before the Write
    assert before == (1, 20, b"\x01" * 20 + bytes(108))
    assert m.apply(5, 100, M.WRITE, 128, b"\x03" * 128) == (1, 128, bytes(128))
    after = m.apply(5, 90, M.READ, 20)
    assert after == (1, 20, b"\x01" * 10 + b"\x03" * 10 + bytes(108))
    assert m.dump(5) == b"\x01" * 100 + b"\x03" * 128 + b"\x01" * (4096 - 228)
    assert not m.inval


def test_read_is_clipped_at_the_end():
    m = M.MemFsModel(1, 8)
    m.apply(5, 250, M.WRITE, 6, bytes([9, 8, 7, 6, 5, 4]))
    assert m.apply(5, 251, M.READ, 20) == (1, 5, bytes([8, 7, 6, 5, 4]) + bytes(123))
    assert m.apply(5, 256, M.READ, 20) == (1, 0, bytes(128))
    assert m.apply(5, 1 << 50, M.READ, 128) == (1, 0, bytes(128))
    assert m.apply(5, 128, M.READ, 128) == (1, 128, b"\x01" * 122 + bytes([9, 8, 7, 6, 5, 4]))


def test_error_answers_change_nothing():
    m = M.MemFsModel(2, 8)
    want = m.dump(5), m.dump(6)
    assert m.apply(5, 200, M.WRITE, 57, b"\x07" * 57) == (0, M.EFBIG, bytes(128))  # one byte too far
    assert m.apply(5, 200, M.WRITE, 56, b"\x01" * 56) == (1, 56, bytes(128))       # exactly to the end
    assert m.apply(5, 257, M.WRITE, 0) == (0, M.EFBIG, bytes(128))
    assert m.apply(4, 0, M.WRITE, 4, b"abcd") == (0, M.ENOENT, bytes(128))
    assert m.apply(7, 0, M.READ, 4) == (0, M.ENOENT, bytes(128))
    assert m.apply(7, 0, M.GETATTR, 0) == (0, M.ENOENT, bytes(128))
    assert not m.inval
    assert m.apply(5, 0, M.WRITE, 129, b"\x07" * 128) == (0, M.EINVAL, bytes(128)) and m.inval
    m.inval = False
    assert m.apply(5, 0, 3, 0) == (0, M.EINVAL, bytes(128)) and m.inval
    assert m.apply(99, 0, M.READ, 200) == (0, M.EINVAL, bytes(128))  # EINVAL is checked before the ino
    assert (m.dump(5), m.dump(6)) == want


def test_len_zero_is_a_valid_no_op():
    m = M.MemFsModel(1, 7)
    assert m.apply(5, 17, M.WRITE, 0) == (1, 0, bytes(128))
    assert m.apply(5, 128, M.WRITE, 0) == (1, 0, bytes(128))  # at the very end too
    assert m.apply(5, 17, M.READ, 0) == (1, 0, bytes(128))
    assert m.dump(5) == b"\x01" * 128


def test_replay_fills_the_response_arrays_and_digest_counts_words():
    m = M.MemFsModel(2, 7)
    recs = np.concatenate([M.W(6, 3, b"xyz"), M.R(6, 2, 5), M.G(5), M.R(9, 0, 1)])
    resp, some = m.replay(recs)
    assert some.tolist() == [1, 1, 1, 0] and resp["n"].tolist() == [3, 5, 128, M.ENOENT]
    assert resp["data"][1].tobytes() == b"\x01xyz\x01" + bytes(123)
    assert not resp["data"][[0, 2, 3]].any()
    c, s, x = m.digest()
    assert c == 2 * 128 // 8
    other = M.MemFsModel(2, 7)
    other.apply(5, 3, M.WRITE, 3, b"xyz")  # the same bytes in the other file: another digest
    assert other.digest()[0] == c and other.digest() != (c, s, x)


# ---- the ABI side ------------------------------------------------------------------------------------
def test_kind_constants_and_struct_sizes(nrgpu_mod):
    L = nrgpu_mod._lib
    assert L.NRG_DS_MEMFS == 7 and L.NRG_MEMFS_FIRST_INO == M.FIRST_INO == 5
    assert (L.NRG_MEMFS_WRITE, L.NRG_MEMFS_READ, L.NRG_MEMFS_GETATTR) == (M.WRITE, M.READ, M.GETATTR) == (0, 1, 2)
    assert (L.NRG_MEMFS_ENOENT, L.NRG_MEMFS_EFBIG, L.NRG_MEMFS_EINVAL) == (M.ENOENT, M.EFBIG, M.EINVAL) == (1, 2, 3)
    assert L.MEMFS_OP_DTYPE.itemsize == 152 and L.MEMFS_RESP_DTYPE.itemsize == 136
    assert L.MEMFS_OP_DTYPE == M.OP_DTYPE and L.MEMFS_RESP_DTYPE == M.RESP_DTYPE
    assert [L.MEMFS_OP_DTYPE.fields[f][1] for f in ("ino", "offset", "op", "len", "data")] == [0, 8, 16, 20, 24]
    assert [L.MEMFS_RESP_DTYPE.fields[f][1] for f in ("n", "data")] == [0, 8]
    hdr = open(os.path.join(ROOT, "include", "nrgpu.h")).read()
    assert re.search(r"#define NRG_DS_MEMFS 7u", hdr)
    assert re.search(r"uint8_t data\[128\];\s*\} nrg_memfs_op; /\* 152 B \*/", hdr)
    assert re.search(r"uint8_t data\[128\];\s*\} nrg_memfs_resp; /\* 136 B \*/", hdr)
    src = open(os.path.join(ROOT, "node-replication_amd", "csrc", "memfs.hip")).read()
    assert "sizeof(nrg_memfs_op) == MF_REC_WORDS * 8 && sizeof(nrg_memfs_resp) == MF_RESP_WORDS * 8" in src
    assert "MF_REC_WORDS = 19;" in src and "MF_RESP_WORDS = 17;" in src  # 152 and 136 bytes


def test_config_defaults(nrgpu_mod):
    L = nrgpu_mod._lib
    cfg = L.default_config(L.NRG_DS_MEMFS)
    other = L.default_config(L.NRG_DS_QUEUE)
    assert cfg.ds_kind == 7 and cfg.log2_slots == 12 and cfg.queue_capacity == 1  # one 4096-byte file
    assert cfg.max_batch == 1 << 20 and cfg.max_reads == other.max_reads and cfg.log_bytes == other.log_bytes
    assert cfg.pipeline == 0 and cfg.replica_id == 1
    assert C.sizeof(L.Config) == 88  # the struct keeps its size
    assert other.queue_capacity == 1 << 24 and L.default_config(L.NRG_DS_SKIPLIST).log2_slots == 24  # untouched


def test_every_symbol_is_exported_and_rejects_a_null_handle(nrgpu_mod):
    L = nrgpu_mod._lib
    lib = nrgpu_mod.load()
    for s in ("round_async", "init", "read", "dump", "geometry"):
        assert "nrg_memfs_" + s in L.SIGNATURES and hasattr(lib, "nrg_memfs_" + s)
    n = C.c_uint64()
    E = L.NRG_E_INVAL
    assert lib.nrg_memfs_round_async(None, None, 0, 1, None, None) == E
    assert lib.nrg_memfs_init(None, 5, None, 0) == E
    assert lib.nrg_memfs_read(None, 5, 0, 0, None, C.byref(n)) == E
    assert lib.nrg_memfs_dump(None, 5, None, 0, C.byref(n)) == E
    assert lib.nrg_memfs_geometry(None, C.byref(n), C.byref(n)) == E


def test_plugin_encodes_the_three_ops_and_decodes_their_answers(nrgpu_mod):
    N = nrgpu_mod
    ops = [N.MfWrite(5, 100, b"\x03" * 128), N.MfRead(5, 90, 20), N.MfGetAttr(6), N.MfWrite(5, 0, b"z" * 200)]
    recs = N.MemFs.encode(ops)
    assert recs.dtype == N.MEMFS_OP_DTYPE and recs["op"].tolist() == [0, 1, 2, 0]
    assert recs["len"].tolist() == [128, 20, 0, 200] and recs["offset"].tolist() == [100, 90, 0, 0]
    assert recs["data"][0].tobytes() == b"\x03" * 128 and not recs["data"][1:].any()
    m = M.MemFsModel(2, 12)
    resp, some = m.replay(recs)
    got = N.MemFs.decode_ops(ops, resp, some)
    assert got == [("written", 128), ("data", b"\x01" * 10 + b"\x03" * 10), ("attr", 4096), ("err", M.EINVAL)]
    assert N.MemFs.decode(resp, some)[3] == ("err", M.EINVAL)
    with pytest.raises(TypeError):
        N.MemFs.read_batch(None, [N.MfRead(5, 0, 1)])
    with pytest.raises(TypeError):
        N.MemFs.encode([N.Put(1, 2)])


def test_digest_and_snapshot_mirrors(nrgpu_mod):
    D, S, L = nrgpu_mod.digest, nrgpu_mod.snapshot, nrgpu_mod._lib
    m = M.MemFsModel(3, 7)
    m.replay(np.concatenate([M.W(5, 3, b"abc"), M.W(7, 120, b"12345678")]))
    files = [m.dump(5 + f) for f in range(3)]
    assert D.memfs(files) == m.digest()
    assert D.memfs([]) == (0, 0, 0)
    for items in (16, 48, 1000):
        assert S.image_bytes(L.NRG_DS_MEMFS, items) == (64 + 8 * items + 63) & ~63
    img = S.pack(L.NRG_DS_MEMFS, files, 9)
    info, data = S.unpack(img)
    assert info.ds_kind == 7 and info.items == 48 and info.log_idx == 9 and info.digest == m.digest()
    assert data.tobytes() == b"".join(files)
    with pytest.raises(ValueError):
        S.pack(L.NRG_DS_MEMFS, [b"12345678", b"1234"], 0)


# ---- the named streams reach what they are named for ---------------------------------------------------
@pytest.mark.parametrize("s", M.all_streams(), ids=lambda s: s.name)
def test_stream_reaches_its_arms(s):
    plan = s.plan()
    assert plan["records"] == len(s.recs) and plan["slots"] == 2 * len(s.recs)
    assert plan["lines"] == s.files * (1 << s.log2_b) // 128
    for arm, least in s.needs.items():
        assert plan[arm] >= least, f"{s.name} no longer reaches {arm}: {plan[arm]} < {least}"
    if s.name == "errors_no_einval":
        assert plan["einval_len"] == plan["einval_op"] == 0
    if s.name.startswith("one_line") or s.name.startswith("wrwr"):
        assert plan["max_run"] == len(s.recs)  # the whole stream is one run


def test_record_counts_sit_on_both_sides_of_the_sort_tile_and_the_grid():
    """2n slots against the radix sort's 2048-key tile (1024 | 1025 records), the expand workgroup
    of 256 records (255 | 256 | 257) and one record; 4097 records are more than two sort tiles."""
    src = open(os.path.join(ROOT, "node-replication_amd", "csrc", "memfs.hip")).read()
    assert "constexpr int MF_TPB = 256;" in src and "MF_AHEAD = 8;" in src
    hdr = open(os.path.join(ROOT, "node-replication_amd", "csrc", "internal.hpp")).read()
    assert "constexpr u32 SORT_TILE = 2048;" in hdr
    counts = sorted(len(s.recs) for s in M.all_streams() if s.name.startswith("memfs_shape"))
    assert counts == [1, 2, 255, 256, 257, 1024, 1025, 4097]
    runs = sorted(len(s.recs) for s in M.all_streams() if s.name.startswith("one_line"))
    assert runs == [M.BATCH - 1, M.BATCH, M.BATCH + 1, 2 * M.BATCH, 2 * M.BATCH + 1]
    a, b = (s for s in M.all_streams() if s.name.startswith("wrwr"))
    assert a.tail_at + 4 <= M.BATCH and b.tail_at + 2 == M.BATCH  # inside one batch; split W R | W R
