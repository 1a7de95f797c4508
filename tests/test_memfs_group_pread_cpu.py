"""The group-wide pread of a file-partitioned group (nrg_group_memfs_pread) on the models alone
(tests/memfs_group_pread_model.py): the protocol restated in numpy (partition, owner answers, T, re-pack)
equals the literal definition for every rank, after every round of every case of memfs_part_streams at
G = 1, 2, 3 and 8; the request lists the GPU test uses do tell a local read from the group's; and the
repack_alignment list reaches every (source mod 16, output mod 16, length). Then the ABI and the Python
surface, which need the library but no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import memfs_group_pread_model as GM
import memfs_model as M
import memfs_part_streams as PS
import memfs_pread_model as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS = (1, 2, 3, 8)
CASES = [pytest.param(c, id=c.id) for G in GS for c in PS.cases(G)]


def _same(got, want, what):
    for g, w, part in zip(got, want, ("data", "offs", "some")):
        np.testing.assert_array_equal(np.asarray(g).astype(np.uint64), np.asarray(w).astype(np.uint64), err_msg=f"{what} {part}")


def test_the_literal_definition_is_memfs_pread_on_the_owners_files():
    """On an unsized group: a model whose every file is the owner's dump, read by memfs_pread_model.pread."""
    for case in [c for G in GS for c in PS.cases(G) if not c.sized]:
        G = case.G
        owner_files, _ = GM.states(case)[-1]
        assert all(len(b) == 1 << case.log2_b for b in owner_files)
        view = M.MemFsModel(case.files, case.log2_b)
        for f, b in enumerate(owner_files):
            view.init(M.FIRST_INO + f, b)
        for r in range(G):
            rq = GM.ragged(case, len(case.rounds) - 1, r, GM.ragged_n(r))
            _same(GM.literal(owner_files, rq), P.pread(view, rq), f"G={G} rank {r}")
            _same(GM.literal(owner_files, rq, cap=100), P.pread(view, rq, cap=100), f"G={G} rank {r} cap")


def test_a_sized_group_clips_at_the_owners_size():
    case = next(c for c in PS.cases(3) if c.name == "sized")
    x = PS.expected(case)
    owner_files, member_files = GM.states(case)[-1]
    sizes = [len(b) for b in owner_files]
    assert sizes == [x.part[PS.owner(M.FIRST_INO + f, 3)].size[f] for f in range(case.files)]
    assert any(s < 1 << case.log2_b for s in sizes), "no file is shorter than B: nothing would be clipped at a size"
    rq = P.reqs([(M.FIRST_INO + f, o, P.U64_MAX) for f in range(case.files) for o in (0, 1, sizes[f], sizes[f] + 1)])
    data, offs, some = GM.literal(owner_files, rq)
    want = [max(sizes[f] - o, 0) for f in range(case.files) for o in (0, 1, sizes[f], sizes[f] + 1)]
    assert np.diff(offs.astype(np.int64)).tolist() == want and some.all()
    assert bytes(data[: sizes[0]]) == owner_files[0]


def test_the_owners_files_are_the_replicated_models():
    """What the definition reads is what one replica replaying W_0 || W_1 || ... would hold."""
    for G in GS:
        for case in PS.cases(G):
            x = PS.expected(case)
            owner_files, _ = GM.states(case)[-1]
            assert owner_files == [x.rep.dump(M.FIRST_INO + f) for f in range(case.files)], case.id


@pytest.mark.parametrize("case", CASES)
def test_protocol_equals_the_definition_for_every_rank(case):
    G = case.G
    st = GM.states(case)
    for e, per_call in enumerate(GM.answers(case)):
        owner_files, member_files = st[e + 1]
        for name, reqs, want in per_call:
            got, T, given = GM.protocol(member_files, G, reqs)
            for r in range(G):
                _same(got[r], want[r], f"{case.id} round {e} {name} rank {r}")
                assert int(want[r][1][-1]) == T[:, r].sum()
                # the re-pack's input is a permutation of the answer: same bytes, other order
                assert sorted(given[r]["pos"].tolist()) == list(range(len(reqs[r])))
            if name == "all_idle":
                assert not T.any() and all(len(w[0]) == 0 and w[1].tolist() == [0] for w in want)
            if name == "heavy_owner0":
                assert sum(GM.partition(rq, G)[2][0] for rq in reqs) > 1024 and not T[1:].any()
            if name == "whole_files":
                assert all(len(rq) == 64 for rq in reqs)


@pytest.mark.parametrize("case", [p for p in CASES if p.values[0].G > 1 and p.values[0].files > 1])
def test_a_local_read_would_fail_the_gpu_test(case):
    """For every member, after every round with records, the ragged list has a request whose answer from
    the member's own files differs from the group's: a library that read locally would not pass."""
    st = GM.states(case)
    for e, per_call in enumerate(GM.answers(case)):
        if not any(len(s) for s in case.rounds[e]):
            continue
        _, reqs, want = per_call[0]
        for r in range(case.G):
            local = GM.literal(st[e + 1][1][r], reqs[r])
            differs = [i for i in range(len(reqs[r]))
                       if bytes(local[0][int(local[1][i]):int(local[1][i + 1])]) != bytes(want[r][0][int(want[r][1][i]):int(want[r][1][i + 1])])]
            assert differs, f"{case.id} round {e} rank {r}: the local answer equals the group's"


def test_ragged_lists_hold_the_edge_requests():
    case = next(c for c in PS.cases(3) if c.name == "sized")
    B, F = 1 << case.log2_b, case.files
    rq = np.concatenate([GM.ragged(case, e, r, GM.ragged_n(r)) for e in range(4) for r in range(3)])
    assert (rq["len"] == 0).any() and (rq["len"] == P.U64_MAX).any()
    assert (rq["offset"] == B).any() and (rq["offset"] > B).any()
    assert (rq["ino"] < M.FIRST_INO).any() and (rq["ino"] >= M.FIRST_INO + F).any()
    assert [GM.ragged_n(r) for r in range(3)] == [37, 87, 137]


def test_repack_alignment_reaches_every_triple():
    rq = GM.repack_alignment()
    assert len(rq) == 5376 and int(rq["len"].sum()) == 49152
    assert set(rq["ino"].tolist()) == {5, 6} and int((rq["offset"] + rq["len"]).max()) <= 4096
    want = {(s, d, ln) for s in range(16) for d in range(16) for ln in P.ALIGN_LENS}
    assert GM.reached(rq) == want and len(want) == 1792
    # and the numpy re-pack of it equals the literal pread
    m = M.MemFsModel(2, 12)
    for f in range(2):
        m.init(M.FIRST_INO + f, PS.init_bytes(f, 4096))
    files = [m.dump(5), m.dump(6)]
    got, T, _ = GM.protocol([files, files], 2, [rq, P.reqs([])])
    _same(got[0], P.pread(m, rq), "repack_alignment")
    assert T[:, 0].sum() == 49152 and T[0][0] and T[1][0]


# ---- the ABI and the Python surface (the library, no GPU) ----------------------------------------------
@pytest.fixture(scope="module")
def nrgpu_mod():
    import nrgpu

    nrgpu.load()
    return nrgpu


def test_abi_of_the_three_entry_points(nrgpu_mod):
    L = nrgpu_mod._lib
    lib = nrgpu_mod.load()
    hdr = open(os.path.join(ROOT, "include", "nrgpu.h")).read()
    assert C.sizeof(L.Pread) == 48 and [f[0] for f in L.Pread._fields_] == ["reqs", "n", "data", "cap", "offs", "some"]
    assert re.search(r"\} nrg_pread;\s*int nrg_group_memfs_pread\(nrg_group\* g, const nrg_pread\* reads\);", hdr)
    for name, nargs in (("nrg_group_memfs_pread", 2), ("nrg_memfs_rd_partition_async", 7), ("nrg_memfs_pread_repack_async", 10)):
        assert hasattr(lib, name) and len(L.SIGNATURES[name][1]) == nargs
    assert lib.nrg_group_memfs_pread(None, None) == L.NRG_E_INVAL
    assert lib.nrg_memfs_rd_partition_async(None, None, 0, 2, None, None, None) == L.NRG_E_INVAL
    assert lib.nrg_memfs_pread_repack_async(None, None, None, None, None, 0, None, 0, None, None) == L.NRG_E_INVAL
    # every entry point cites the reference
    doc = hdr[hdr.index("The building blocks of the group-wide pread"):hdr.index("} nrg_pread;")]
    assert doc.count("nrfs.rs") >= 3 and doc.count("cnr/src/replica.rs:430-445") >= 3
    assert "a group-wide pread, a pipelined form" not in hdr  # the old "Not for this mode" sentence
    assert callable(nrgpu_mod.parallel.FilePartitionedGroup.pread)
    assert nrgpu_mod.MfPread(5, 0, 4096).size == 4096  # still the local read


def test_the_request_partition_and_the_copy_are_shared_code():
    part = open(os.path.join(ROOT, "node-replication_amd", "csrc", "partition.hip")).read()
    mem = open(os.path.join(ROOT, "node-replication_amd", "csrc", "memfs.hip")).read()
    assert "fp_count_kernel<RD_REQ_WORDS>" in part and "pt_scan_kernel" in part[part.index("rd_partition("):]
    # one copy kernel, two sources
    assert mem.count("void mf_pread_copy_kernel(") == 1
    assert "mf_pread_copy_kernel<PACKED>" in mem
