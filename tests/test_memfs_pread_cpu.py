"""The file store's read-only reads without a GPU: the ABI of nrg_memfs_pread* (the 24-byte request,
both symbols exported and bound, a NULL context refused), the tile size shared with the kernel, the
numpy model of tests/memfs_pread_model.py on hand-worked answers, and that every named request list
of the GPU test reaches the arm it is named for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import memfs_model as M
import memfs_pread_model as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tile():
    hdr = open(os.path.join(ROOT, "include", "nrgpu_testing.h")).read()
    return int(re.search(r"#define NRG_MF_PREAD_TILE (\d+)u", hdr).group(1))


@pytest.fixture(scope="module")
def nrgpu_mod():
    import nrgpu

    nrgpu.load()
    return nrgpu


# ---- ABI ---------------------------------------------------------------------------------------------
def test_request_is_24_bytes_and_both_symbols_are_exported(nrgpu_mod):
    L = nrgpu_mod._lib
    lib = nrgpu_mod.load()
    assert L.MEMFS_RD_DTYPE.itemsize == 24 and L.MEMFS_RD_DTYPE == P.RD_DTYPE == nrgpu_mod.MEMFS_RD_DTYPE
    assert [L.MEMFS_RD_DTYPE.fields[f][1] for f in ("ino", "offset", "len")] == [0, 8, 16]
    hdr = open(os.path.join(ROOT, "include", "nrgpu.h")).read()
    assert re.search(r"uint64_t ino, offset, len;\s*\} nrg_memfs_rd; /\* 24 B \*/", hdr)
    for name in ("nrg_memfs_pread", "nrg_memfs_pread_async"):
        assert hasattr(lib, name) and name in L.SIGNATURES
        res, args = L.SIGNATURES[name]
        assert res is C.c_int and len(args) == 7 and args[2] is C.c_uint64 and args[4] is C.c_uint64
        assert getattr(lib, name)(None, None, 0, None, 0, None, None) == L.NRG_E_INVAL
        assert re.search(r"int %s\(nrg_ctx\* ctx, const nrg_memfs_rd\*" % name, hdr)
    assert "nr/src/replica.rs" in hdr[hdr.index("nrg_memfs_geometry(nrg_ctx*"):hdr.index("} nrg_memfs_rd;")]
    assert "nrfs.rs:16-18, :88-101" in hdr[hdr.index("nrg_memfs_geometry(nrg_ctx*"):hdr.index("} nrg_memfs_rd;")]


def test_tile_size_is_one_constant():
    T = _tile()
    assert T >= 4096 and T & (T - 1) == 0
    src = open(os.path.join(ROOT, "node-replication_amd", "csrc", "memfs.hip")).read()
    assert "constexpr u32 MF_PREAD_TILE = %d;" % T in src
    assert "static_assert(MF_PREAD_TILE == NRG_MF_PREAD_TILE" in src
    assert "constexpr u32 MF_PR_ITEMS = 4;" in src  # 1024 requests per scan tile: test_gpu_memfs_pread's counts


def test_python_surface(nrgpu_mod):
    N = nrgpu_mod
    assert callable(N.DeviceReplica.mf_pread) and callable(N.DeviceReplica.mf_pread_device)
    assert N.MfPread(5, 0, 4096).size == 4096
    with pytest.raises(TypeError):  # the logged Read stays an execute_mut op
        N.MemFs.read_batch(None, [N.MfPread(5, 0, 1), N.MfRead(5, 0, 1)])
    with pytest.raises(TypeError):
        N.MemFs.read_batch(None, [N.Get(1)])
    assert N.MemFs.read_batch(None, []) == []


# ---- the model on answers worked by hand ----------------------------------------------------------------
def test_model_clips_packs_and_truncates():
    m = M.MemFsModel(2, 8)
    m.replay(M.W(5, 3, b"abcdefgh"))
    rq = P.reqs([(5, 0, 5), (4, 0, 3), (6, 250, 100), (5, 256, 3), (5, 2, 4), (7, 0, 1), (5, 255, P.U64_MAX),
                 (5, P.U64_MAX, P.U64_MAX)])
    data, offs, some = P.pread(m, rq)
    assert offs.tolist() == [0, 5, 5, 11, 11, 15, 15, 16, 16] and some.tolist() == [1, 0, 1, 1, 1, 0, 1, 1]
    assert data.tobytes() == b"\x01\x01\x01ab" + b"\x01" * 6 + b"\x01abc" + b"\x01"
    for cap in (0, 1, 7, 15, 16, 17, 1 << 40):
        d, o, s = P.pread(m, rq, cap)
        assert d.tobytes() == data.tobytes()[:cap] and o.tolist() == offs.tolist() and s.tolist() == some.tolist()
    d, o, s = P.pread(m, P.reqs([]))
    assert len(d) == 0 and o.tolist() == [0] and len(s) == 0


def test_plan_counts_a_hand_worked_list():
    # tile 32: [0, 31) ends at T - 1; [31, 32) ends at T; two empty ones at 32; [32, 65) ends at T + 1 of
    # the third tile and spans two tiles
    rq = P.reqs([(5, 1, 31), (5, 0, 1), (5, 9, 0), (9, 0, 4), (5, 16, 33)])
    a = P.plan(rq, 1, 8, 32)
    assert (a["total"], a["tiles"], a["enoent"], a["len0"], a["max_zero_run"], a["zero_at_tile_edge"]) == (65, 3, 1, 1, 2, 2)
    assert a["ends_at_T-1"] == 1 and a["ends_at_T"] == 1 and a["ends_at_T+1"] == 1
    assert a["max_tiles_per_req"] == 2 and a["max_reqs_in_tile"] == 2
    assert a["wide_chunks"] == 1 + 2 and a["wide_shift_1"] == 1 and a["wide_shift_0"] == 1 and a["byte_chunks"] == 2
    assert a["pairs"] == {(1, 0, 31), (0, 15, 1), (0, 0, 33)}
    b = P.plan(rq, 1, 8, 32, cap=40)
    assert b["end"] == 40 and b["tiles"] == 2 and b["cut_by_cap"] == 1 and b["total"] == 65


# ---- the named lists reach what they are named for ---------------------------------------------------------
@pytest.mark.parametrize("r", P.all_reads(_tile()), ids=lambda r: r.name)
def test_list_reaches_its_arms(r):
    plan = r.plan(_tile())
    for arm, least in r.needs.items():
        assert plan[arm] >= least, f"{r.name} no longer reaches {arm}: {plan[arm]} < {least}"


def test_edges_hold_every_listed_value():
    r = P.edges()
    assert len(r.rq) == 5 * 7 * 9
    assert set(r.rq["len"].tolist()) == {0, 1, 127, 128, 129, 255, 256, 257, P.U64_MAX}
    assert set(r.rq["offset"].tolist()) == {0, 1, 255, 256, 257, 1 << 33, P.U64_MAX}
    assert set(r.rq["ino"].tolist()) == {4, 5, 6, 7, P.U64_MAX}


def test_alignment_lists_reach_every_pair_with_every_length_and_every_wide_shift():
    T = _tile()
    pairs, shifts = set(), set()
    for lead in range(16):
        a = P.alignment(lead).plan(T)
        pairs |= a["pairs"]
        shifts |= {k for k in range(16) if a["wide_shift_%d" % k]}
    for s in range(16):
        for d in range(16):
            for ln in P.ALIGN_LENS:
                assert (s, d, ln) in pairs, (s, d, ln)
    assert shifts == set(range(16))


def test_tile_edges_and_skew_sit_where_the_kernel_changes_path():
    T = _tile()
    a = P.tile_edges(T).plan(T)
    assert a["tiles"] == 11 and a["max_tiles_per_req"] >= 4 and a["max_reqs_in_tile"] > 1024
    assert a["requests"] > 1024  # more than one scan tile: the three-launch scan
    for big_first in (True, False):
        s = P.skew(big_first)
        b = s.plan(T)
        assert b["max_reqs_in_tile"] > 1024 and b["max_tiles_per_req"] >= (1 << 20) // T
        assert (int(s.rq["len"][0]) == 1 << 20) == big_first and (int(s.rq["len"][-1]) == 1 << 20) != big_first
