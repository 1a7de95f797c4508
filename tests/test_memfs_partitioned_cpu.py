"""File-partitioned rounds of a file-store group (nrg_group_file_round) without a GPU: the owner
function in C against its numpy mirror, the ABI of the four new symbols and their NULL arguments, the
Python surface, and the order argument on the sequential models alone: for every case of
tests/memfs_part_streams.py, one model replaying W_0 || ... || W_{G-1} and G models each replaying only
the records of the files it owns give the same response for every record and the same bytes for every
file on its owner; the sized case with memfs_size_model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import memfs_model as M
import memfs_part_streams as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = (1, 2, 3, 7, 8, 64)


@pytest.fixture(scope="module")
def nrgpu_mod():
    import nrgpu

    nrgpu.load()
    return nrgpu


def _inos():
    return np.array(list(range(0, 5)) + list(range(5, 5 + 2001)) + [1 << 63, (1 << 64) - 1], dtype=np.uint64)


def test_owner_in_c_equals_the_numpy_mirror(nrgpu_mod):
    from nrgpu.parallel import memfs_owner

    lib = nrgpu_mod.load()
    inos = _inos()
    for parts in PARTS:
        got = np.array([lib.nrg_memfs_owner(int(i), parts) for i in inos], np.int64)
        np.testing.assert_array_equal(got, memfs_owner(inos, parts), err_msg=f"parts {parts}")
        # the definition, written out: the file index modulo parts, 0 below the first ino
        want = [(int(i) - 5) % parts if int(i) >= 5 else 0 for i in inos]
        assert got.tolist() == want
        assert got.tolist() == [PS.owner(i, parts) for i in inos]
    assert lib.nrg_memfs_owner(12345, 0) == 0 and memfs_owner(inos[:3], 0).tolist() == [0, 0, 0]


def test_abi_and_python_surface(nrgpu_mod):
    N = nrgpu_mod
    L = N._lib
    lib = N.load()
    hdr = open(os.path.join(ROOT, "include", "nrgpu.h")).read()
    for name, res, nargs in (("nrg_memfs_owner", C.c_uint32, 2), ("nrg_memfs_partition_async", C.c_int, 7),
                             ("nrg_memfs_route_back_async", C.c_int, 7), ("nrg_group_file_round", C.c_int, 2)):
        assert hasattr(lib, name) and name in L.SIGNATURES
        got_res, args = L.SIGNATURES[name]
        assert got_res is res and len(args) == nargs
        assert re.search(r"(uint32_t|int) %s\(" % name, hdr)
    assert L.SIGNATURES["nrg_group_file_round"][1][1] == C.POINTER(L.Round)
    assert re.search(r"#define NRG_MEMFS_PARTITION_TILE %d\b" % L.NRG_MEMFS_PARTITION_TILE, hdr)
    # NULL group / NULL context
    rd = (L.Round * 1)()
    assert lib.nrg_group_file_round(None, rd) == L.NRG_E_INVAL
    assert lib.nrg_memfs_partition_async(None, None, 0, 1, None, None, None) == L.NRG_E_INVAL
    assert lib.nrg_memfs_route_back_async(None, None, None, None, 0, None, None) == L.NRG_E_INVAL
    # the Python surface
    from nrgpu import parallel

    assert issubclass(parallel.FilePartitionedGroup, parallel.ReplicaGroup)
    assert callable(parallel.FilePartitionedGroup.round) and callable(parallel.FilePartitionedGroup.owner)
    assert N.FilePartitionedGroup is parallel.FilePartitionedGroup and N.memfs_owner is parallel.memfs_owner
    assert "FilePartitionedGroup" in N.__all__ and "memfs_owner" in N.__all__


def test_the_three_out_of_scope_places_are_true_as_worded():
    hdr = open(os.path.join(ROOT, "include", "nrgpu.h")).read()
    src = open(os.path.join(ROOT, "node-replication_amd", "csrc", "memfs.hip")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "no partitioned groups" not in readme and "nrg_group_file_round" in readme
    assert "key-partitioned group rounds" in hdr and "nrg_group_file_round" in hdr
    assert "Out of scope: the combiner, partitioned groups and growth" in src
    assert "key-partitioned entry points" in src and "group_files.cpp" in src and "nrg_group_file_round" in src


CASES = [c for G in (1, 2, 3, 8) for c in PS.cases(G)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_owners_replaying_their_own_records_answer_as_the_one_log_does(case):
    x = PS.expected(case)
    G = case.G
    assert len(case.rounds) in (3, 4)
    lens = [[len(r) for r in rnd] for rnd in case.rounds]
    assert any(all(n == 0 for n in row) for row in lens)  # n = 0 on all ranks, and on some
    assert G == 1 or any(0 < sum(n == 0 for n in row) < G for row in lens)
    for e, rnd in enumerate(case.rounds):
        for r in range(G):
            (wr, ws), (br, bs) = x.want[e][r], x.back[e][r]
            np.testing.assert_array_equal(bs, ws, err_msg=f"round {e} rank {r} some")
            np.testing.assert_array_equal(br["n"], wr["n"], err_msg=f"round {e} rank {r} n")
            np.testing.assert_array_equal(br["data"], wr["data"], err_msg=f"round {e} rank {r} data")
    touched = set()
    for f in range(case.files):
        ino = M.FIRST_INO + f
        p = PS.owner(ino, G)
        assert x.part[p].dump(ino) == x.rep.dump(ino), f"file {f} on its owner {p}"
        if case.sized:
            assert x.part[p].size[f] == x.rep.size[f]
        if x.rep.dump(ino) != x.initial.dump(ino):
            touched.add(p)
        for q in range(G):  # a member's copy of a file it does not own is as it was seeded
            if q != p and (case.files <= 16 or f % 41 == 0):
                assert x.part[q].dump(ino) == x.initial.dump(ino), f"file {f} on member {q}"
    assert touched, "the case changes no file"
    assert not x.rep.inval and not any(m.inval for m in x.part)  # nothing to latch in these cases


def test_the_cases_reach_what_they_are_named_for():
    for G in (1, 2, 3, 8):
        by = {c.name: c for c in PS.cases(G)}
        sk = by["skewed_pwrite"]
        for rnd in sk.rounds:
            got0 = sum(int((PS.owners(recs, G) == 0).sum()) for recs in rnd)
            assert got0 == 0 or got0 > PS.MAX_BATCH  # owner 0 replays in slices
            first = next((recs for recs in rnd if len(recs)), None)
            if first is not None:  # a run of Writes of ino 5 at consecutive lines straddles record 64
                mine = first[PS.owners(first, G) == 0]
                a, b = mine[PS.MAX_BATCH - 1], mine[PS.MAX_BATCH]
                assert a["op"] == b["op"] == M.WRITE and a["ino"] == b["ino"] == 5
                assert int(b["offset"]) == int(a["offset"]) + int(a["len"]) and int(b["offset"]) % 128 == 0
        assert by["one_file"].files == 1 and by["three_files"].files == 3 and by["thousand_files"].files == 1000
        assert by["three_files"].quiet == {0: {G - 1}}
        sz = np.concatenate([r for rnd in by["sized"].rounds for r in rnd])
        assert (sz["op"] == 3).sum() > 10 and by["sized"].sized
        er = np.concatenate([r for rnd in by["errors"].rounds for r in rnd])
        assert (er["ino"] < 5).any() and (er["ino"] > 7).any()
        if G > 1:  # every owner gets records in the thousand-files case
            th = np.concatenate([r for rnd in by["thousand_files"].rounds for r in rnd])
            assert set(PS.owners(th, G).tolist()) == set(range(G))
