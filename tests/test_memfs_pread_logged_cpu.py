"""The file store's logged reads of any length without a GPU: the numpy model of the cut
(tests/memfs_pread_logged_model.py) through the sequential replay models and back through fold() against
pread on byte arrays, unsized, sized (a size inside a line, on a line edge, 0) and with a growth bound
above B; nrg_memfs_pread_logged_plan, which touches no device, against the model; the ABI of the five
symbols; the Python codec (MemFs.encode_counts / decode_ops) that turns an MfPreadLogged into its fragment
records and folds them; and the header's statement of the cut."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import memfs_grow_model as G
import memfs_model as M
import memfs_pread_logged_model as R
import memfs_size_model as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nrgpu_mod():
    import nrgpu

    nrgpu.load()
    return nrgpu


def _random(files, A, n, seed):
    rng = np.random.default_rng(seed)
    v = []
    for _ in range(n):
        ino, off = R.FIRST_INO + int(rng.integers(files)), int(rng.integers(A + 1))
        k = int(rng.integers(8))
        if k == 0:
            ln = 0
        elif k == 1:
            ln = A - off
        elif k == 2:
            ln = A - off + 1 + int(rng.integers(3))  # clipped at A
        elif k == 3:
            ino, ln = int(rng.integers(12)), int(rng.integers(200))  # sometimes ENOENT
        elif k == 4:
            ln = R.U64 - int(rng.integers(3))  # read to the end
        else:
            ln = int(rng.integers(A - off + 1))
        v.append((ino, off, ln))
    return R.reqs(v)


def _lists():
    out = []
    for log2_b in (12, 7):
        B = 1 << log2_b
        out.append(("edges_B%d" % B, 3, log2_b, R.edges(3, B)))
        out.append(("random_B%d" % B, 3, log2_b, _random(3, B, 120, 7 + log2_b)))
    out.append(("random_one_file_B1024", 1, 10, _random(1, 1024, 120, 3)))
    return out


LISTS = _lists()


def _check_cut(rq, files, A):
    recs, first, offs, planned, some = R.cut(rq, files, A)
    assert first[0] == 0 and first[-1] == len(recs) and np.all(np.diff(first) >= 1)
    assert offs[0] == 0 and np.array_equal(np.diff(offs), planned)
    assert np.all(recs["op"] == M.READ) and np.all(recs["len"] <= 128) and not recs["data"].any()
    nz = recs[recs["len"] > 0]
    assert np.all(nz["offset"] // 128 == (nz["offset"] + nz["len"] - 1) // 128)  # one line each
    return recs, first, offs, planned, some


def _fill(models, files, B, seed):
    """The same patterned bytes into every model's files; returns them as the plain store."""
    store = []
    for f in range(files):
        d = R.pattern(B, seed + f)
        for m in models:
            m.init(R.FIRST_INO + f, d.tobytes())
        store.append(bytearray(d.tobytes()))
    return store


@pytest.mark.parametrize("name,files,log2_b,rq", LISTS, ids=[l[0] for l in LISTS])
def test_the_cut_replayed_and_folded_equals_pread(name, files, log2_b, rq):
    B = 1 << log2_b
    recs, first, offs, planned, some = _check_cut(rq, files, B)
    m = M.MemFsModel(files, log2_b)
    store = _fill([m], files, B, 11)
    before = m.digest()
    resp, rs = m.replay(recs)
    assert not m.inval and m.digest() == before  # Reads change nothing
    fs, count, got = R.fold(rq, first, resp, rs)
    ws, wp, want = R.pread_at(store, None, rq, files, B)
    assert np.array_equal(fs, ws) and np.array_equal(fs, some) and np.array_equal(wp, planned)
    assert got == want and np.array_equal(count, planned)  # unsized: count == planned
    # ... and packed as the read-only pread packs the same requests: the same clip, the same offsets
    assert [len(b) for b in want] == np.diff(offs).tolist()
    # a request that names no file: one record, which the replay answers with ENOENT
    for i in np.flatnonzero(some == 0):
        a = int(first[i])
        assert int(first[i + 1]) - a == 1 and rs[a] == 0 and int(resp["n"][a]) == R.ENOENT


@pytest.mark.parametrize("sizes", [(10, 0, 2048), (128, 4096, 129), (0, 0, 0), (4095, 1, 256)],
                         ids=["inside_a_line", "on_a_line_edge", "zero", "mixed"])
def test_sized_counts_follow_the_size_and_slots_follow_the_plan(sizes):
    files, log2_b, B = 3, 12, 4096
    rq = np.concatenate([R.edges(files, B), _random(files, B, 80, 5)])
    recs, first, offs, planned, some = _check_cut(rq, files, B)
    z = Z.SizedModel(files, log2_b)
    store = _fill([z], files, B, 21)
    for f, s in enumerate(sizes):
        z.truncate(R.FIRST_INO + f, s)
        store[f][s:] = bytes(B - s)
    resp, rs = z.replay(recs)
    fs, count, got = R.fold(rq, first, resp, rs)
    ws, wp, want = R.pread_at(store, list(sizes), rq, files, B)
    assert np.array_equal(fs, ws) and got == want and np.array_equal(wp, planned)
    want_count = [min(int(p), max(sizes[int(r["ino"]) - R.FIRST_INO] - int(r["offset"]), 0)) if p else 0
                  for r, p in zip(rq, planned)]
    assert count.tolist() == want_count and any(c < p for c, p in zip(want_count, planned.tolist()))
    # the fragments' n along a run: full, at most one partial, then zero
    for i in range(len(rq)):
        n = resp["n"][int(first[i]):int(first[i + 1])].astype(np.int64)
        full = recs["len"][int(first[i]):int(first[i + 1])].astype(np.int64)
        if some[i]:
            k = int(np.argmax(n < full)) if (n < full).any() else len(n)
            assert np.array_equal(n[:k], full[:k]) and not n[k + 1:].any()


def test_with_a_bound_above_B_the_plan_follows_the_bound_and_the_count_the_size():
    files, log2_b, B, A = 3, 9, 512, 4096
    rq = np.concatenate([R.edges(files, A), _random(files, A, 80, 9)])
    recs, first, offs, planned, some = _check_cut(rq, files, A)
    g = G.GrowModel(files, log2_b, bound=A)
    store = _fill([g], files, B, 31)
    resp, rs = g.replay(recs)
    assert g.B == B and g.grows == 0  # Reads ask for no growth
    fs, count, got = R.fold(rq, first, resp, rs)
    ws, wp, want = R.pread_at(store, [B] * files, rq, files, A)
    assert np.array_equal(fs, ws) and got == want and np.array_equal(wp, planned)
    assert int(planned.max()) == A and int(count.max()) == B


@pytest.mark.parametrize("name,files,log2_b,rq", LISTS, ids=[l[0] for l in LISTS])
def test_the_plan_function_equals_the_model(nrgpu_mod, name, files, log2_b, rq):
    first, offs, some = nrgpu_mod.memfs_pread_logged_plan(log2_b, files, rq)
    _, mf, mo, _, ms = R.cut(rq, files, 1 << log2_b)
    assert np.array_equal(first, mf) and np.array_equal(offs, mo) and np.array_equal(some, ms)
    with pytest.raises(ValueError):
        nrgpu_mod.memfs_pread_logged_plan(6, files, rq)
    f0, o0, s0 = nrgpu_mod.memfs_pread_logged_plan(log2_b, files, rq[:0])
    assert f0.tolist() == [0] and o0.tolist() == [0] and len(s0) == 0


def test_request_is_24_bytes_and_the_symbols_are_exported(nrgpu_mod):
    L = nrgpu_mod._lib
    lib = nrgpu_mod.load()
    assert L.MEMFS_RD_DTYPE.itemsize == 24 and L.MEMFS_RD_DTYPE == R.RD_DTYPE
    hdr = open(os.path.join(ROOT, "include", "nrgpu.h")).read()
    for name, nargs in (("nrg_memfs_pread_logged_plan", 7), ("nrg_memfs_pread_logged_async", 10),
                        ("nrg_memfs_pread_logged", 10), ("nrg_memfs_pread_logged_records_async", 6),
                        ("nrg_memfs_pread_logged_gather_async", 10)):
        assert hasattr(lib, name) and name in L.SIGNATURES
        res, args = L.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs
        assert re.search(r"int %s\(" % name, hdr)
    # a NULL context is refused before anything else
    assert lib.nrg_memfs_pread_logged_async(None, None, 0, 1, None, 0, None, None, None, None) == L.NRG_E_INVAL
    assert lib.nrg_memfs_pread_logged(None, None, 0, 1, None, 0, None, None, None, None) == L.NRG_E_INVAL
    assert lib.nrg_memfs_pread_logged_records_async(None, None, 0, None, 0, None) == L.NRG_E_INVAL
    assert lib.nrg_memfs_pread_logged_gather_async(None, None, 0, None, None, 0, None, 0, None, None) == L.NRG_E_INVAL


def test_the_header_states_the_four_cases_and_cites_the_reference():
    hdr = open(os.path.join(ROOT, "include", "nrgpu.h")).read()
    doc = hdr[hdr.index("/* Logged reads of any length"):hdr.index("int nrg_memfs_pread_logged_plan(")]
    assert "memfs.rs:73-78, :267-282" in doc
    flat = " ".join(doc.replace("*", " ").split())
    assert "ino outside the range one record {ino, offset, READ, len 0}; some = 0, planned = 0" in flat
    assert "len == 0 or offset >= A one record {ino, offset, READ, len 0}; some = 1, planned = 0" in flat
    assert "planned = min(len, A - offset)" in flat and "len may be 2^64 - 1" in flat
    assert "[max(offset, line_k 128), min(offset + planned, (line_k + 1) 128))" in flat
    assert "count[i] = min(planned[i], max(size - offset, 0))" in flat
    assert "offs[n] > cap is NRG_E_CAPACITY from the call WITH NOTHING LOGGED" in flat
    src = open(os.path.join(ROOT, "node-replication_amd", "csrc", "memfs.hip")).read()
    for k in ("mf_rfrag_kernel", "mf_rgather_kernel", "mf_rcount_kernel"):
        assert k in src
    plan = open(os.path.join(ROOT, "node-replication_amd", "csrc", "memfs_plan.hpp")).read()
    assert "NRG_MFP_HD inline RCut rcut_of(" in plan and "mfp::rcut_of(" in src  # the kernels use the host's functions
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert design.index("Writes of any length") < design.index("Logged reads of any length")


# ---- the Python codec ----------------------------------------------------------------------------------
def test_python_surface(nrgpu_mod):
    N = nrgpu_mod
    for m in ("mf_pread_logged", "mf_pread_logged_device", "mf_pread_logged_records", "mf_pread_logged_records_device",
              "mf_pread_logged_gather_device"):
        assert callable(getattr(N.DeviceReplica, m))
    assert N.MfPreadLogged(5, 0, 4096).size == 4096
    with pytest.raises(TypeError):
        N.MemFs.encode([N.MfPreadLogged(5, 0, 4096)])
    with pytest.raises(TypeError, match="execute_mut op"):
        N.MemFs.read_batch(None, [N.MfPreadLogged(5, 0, 4096)])
    # MfRead stays the single-record op
    r = N.MemFs.encode([N.MfRead(5, 0, 300)])
    assert len(r) == 1 and int(r["len"][0]) == 300


@pytest.mark.parametrize("name,files,log2_b,rq", LISTS, ids=[l[0] for l in LISTS])
def test_encode_counts_equals_the_models_cut_and_decode_ops_folds(nrgpu_mod, name, files, log2_b, rq):
    N = nrgpu_mod
    B = 1 << log2_b
    ops = [N.MfPreadLogged(int(r["ino"]), int(r["offset"]), int(r["len"])) for r in rq]
    recs, counts = N.MemFs.encode_counts(ops, log2_b, files)
    mrecs, first, offs, planned, some = R.cut(rq, files, B)
    assert counts == np.diff(first).astype(np.int64).tolist() == N.MemFs.record_counts(ops, log2_b, files)
    assert recs.tobytes() == mrecs.tobytes()
    m = M.MemFsModel(files, log2_b)
    store = _fill([m], files, B, 41)
    resp, rs = m.replay(recs)
    out = N.MemFs.decode_ops(ops, resp, rs, counts)
    _, _, want = R.pread_at(store, None, rq, files, B)
    assert out == [("data", b) if s else ("err", R.ENOENT) for b, s in zip(want, some)]


def test_a_mixed_batch_keeps_every_ops_records_in_place(nrgpu_mod):
    N = nrgpu_mod
    files, log2_b, B = 3, 12, 4096
    data = R.pattern(700, 3).tobytes()
    ops = [N.MfWrite(5, 0, b"abc"), N.MfPreadLogged(5, 0, 300), N.MfPwrite(6, 100, data), N.MfPreadLogged(6, 90, 720),
           N.MfRead(5, 1, 2), N.MfPreadLogged(9, 0, 5), N.MfPreadLogged(7, 5000, 5), N.MfGetAttr(7)]
    recs, counts = N.MemFs.encode_counts(ops, log2_b, files)
    assert counts == [1, 3, 7, 7, 1, 1, 1, 1] and len(recs) == sum(counts)
    m = M.MemFsModel(files, log2_b)
    resp, rs = m.replay(recs)
    out = N.MemFs.decode_ops(ops, resp, rs, counts)
    want6 = bytearray(b"\x01" * B)
    want6[100:800] = data
    assert out == [("written", 3), ("data", b"abc" + b"\x01" * 297), ("written", 700), ("data", bytes(want6[90:810])),
                   ("data", b"bc"), ("err", R.ENOENT), ("data", b""), ("attr", B)]
