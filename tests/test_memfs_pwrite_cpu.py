"""The file store's logged writes of any length without a GPU: the numpy model of the cut
(tests/memfs_pwrite_model.py) through the sequential replay models against whole-request pwrite on
byte arrays, sized and unsized; nrg_memfs_pwrite_plan, which touches no device, against the model; the
ABI of the request and the four symbols; and the Python codec (MemFs.encode_counts / decode_ops) that
turns an MfPwrite into its fragment records."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import memfs_model as M
import memfs_pwrite_model as P
import memfs_size_model as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA_BYTES = 4096 + 104


@pytest.fixture(scope="module")
def nrgpu_mod():
    import nrgpu

    nrgpu.load()
    return nrgpu


def _random(files, B, data_bytes, n, seed):
    rng = np.random.default_rng(seed)
    v = []
    for _ in range(n):
        ino, off = P.FIRST_INO + int(rng.integers(files)), int(rng.integers(B + 1))
        k = int(rng.integers(8))
        if k == 0:
            ln = 0
        elif k == 1:
            ln = B - off
        elif k == 2:
            ln = B - off + 1 + int(rng.integers(3))  # EFBIG
        elif k == 3:
            ino, ln = int(rng.integers(12)), int(rng.integers(200))  # sometimes ENOENT
        else:
            ln = int(rng.integers(B - off + 1))
        ln = min(ln, data_bytes) if P.answer({"ino": ino, "offset": off, "len": ln}, files, B)[0] else ln
        v.append((ino, off, ln, int(rng.integers(data_bytes - min(ln, data_bytes) + 1))))
    return P.reqs(v)


def _lists():
    out = []
    for log2_b in (12, 7):
        B = 1 << log2_b
        out.append(("edges_B%d" % B, 3, log2_b, P.edges(3, B, DATA_BYTES)))
        out.append(("random_B%d" % B, 3, log2_b, _random(3, B, DATA_BYTES, 120, 7 + log2_b)))
    out.append(("random_one_file_B1024", 1, 10, _random(1, 1024, DATA_BYTES, 120, 3)))
    return out


LISTS = _lists()


@pytest.mark.parametrize("name,files,log2_b,rq", LISTS, ids=[l[0] for l in LISTS])
def test_the_cut_replayed_equals_whole_pwrite(name, files, log2_b, rq):
    B = 1 << log2_b
    data = P.pattern(DATA_BYTES, 1)
    recs, first, written, some = P.cut(rq, data, files, B)
    assert first[0] == 0 and first[-1] == len(recs) and np.all(np.diff(first) >= 1)
    assert np.all(recs["op"] == M.WRITE) and np.all(recs["len"] <= 128)
    # every fragment with bytes lies in one line; bytes past len are zero
    nz = recs[recs["len"] > 0]
    assert np.all(nz["offset"] // 128 == (nz["offset"] + nz["len"] - 1) // 128)
    assert all(not r["data"][int(r["len"]):].any() for r in recs)
    store = [bytearray(b"\x01" * B) for _ in range(files)]
    w, s = P.pwrite(store, None, rq, data, files, B)
    assert np.array_equal(w, written) and np.array_equal(s, some)
    m = M.MemFsModel(files, log2_b)
    resp, rs = m.replay(recs)
    assert not m.inval
    for f in range(files):
        assert m.dump(P.FIRST_INO + f) == bytes(store[f]), (name, f)
    # a request's answer folds from its records': the sum of Written, or the single record's error
    for i in range(len(rq)):
        a, b = int(first[i]), int(first[i + 1])
        if some[i]:
            assert rs[a:b].all() and int(resp["n"][a:b].sum()) == int(written[i])
        else:
            assert b - a == 1 and rs[a] == 0 and int(resp["n"][a]) == int(written[i])


@pytest.mark.parametrize("name,files,log2_b,rq", LISTS, ids=[l[0] for l in LISTS])
def test_the_cut_replayed_by_the_sized_model_grows_files_as_pwrite_does(name, files, log2_b, rq):
    B = 1 << log2_b
    data = P.pattern(DATA_BYTES, 2)
    recs = P.cut(rq, data, files, B)[0]
    z = Z.SizedModel(files, log2_b)
    store = [bytearray(b"\x01" * B) for _ in range(files)]
    sizes = [B] * files
    for f, size in enumerate((10, 0, B // 2)[:files]):  # short files first: writes past the size grow them
        z.truncate(P.FIRST_INO + f, size)
        store[f][size:] = bytes(B - size)
        sizes[f] = size
    half = len(rq) // 2
    P.pwrite(store, sizes, rq[:half], data, files, B)
    cut_at = int(P.cut(rq[:half], data, files, B)[1][-1])
    z.replay(recs[:cut_at])
    if files > 1:  # a SetAttr between two calls: both sides cut file 1 at 20
        z.replay(Z.S(P.FIRST_INO + 1, 20))
        if sizes[1] > 20:
            store[1][20:] = bytes(B - 20)
        sizes[1] = 20
    P.pwrite(store, sizes, rq[half:], data, files, B)
    z.replay(recs[cut_at:])
    assert not z.inval
    for f in range(files):
        assert z.size[f] == sizes[f], (name, f)
        assert z.dump(P.FIRST_INO + f) == bytes(store[f][: sizes[f]]), (name, f)
    assert z.raw() == b"".join(bytes(s) for s in store)


def test_hand_worked_cut():
    data = np.arange(2, 2 + 200, dtype=np.uint8)
    recs, first, written, some = P.cut(P.reqs([(7, 100, 300, 0)]), np.resize(data, 400), 3, 4096)
    assert [(int(r["offset"]), int(r["len"])) for r in recs] == [(100, 28), (128, 128), (256, 128), (384, 16)]
    assert list(first) == [0, 4] and list(written) == [300] and list(some) == [1]
    assert recs["data"][1][0] == data[28] and recs["data"][3][15] == np.resize(data, 400)[299] and recs["data"][3][16] == 0
    recs, first, written, some = P.cut(P.reqs([(5, 127, 2, 0), (5, 4095, 2, 0), (4, 77, 2, 0), (5, 4096, 0, 0)]), data, 3, 4096)
    assert [(int(r["ino"]), int(r["offset"]), int(r["len"])) for r in recs] == [
        (5, 127, 1), (5, 128, 1), (5, 4096, 1), (4, 77, 0), (5, 4096, 0)]
    assert list(first) == [0, 2, 3, 4, 5] and list(written) == [2, P.EFBIG, P.ENOENT, 0] and list(some) == [1, 0, 0, 1]
    assert not recs["data"][2].any()


# ---- the library's plan: fails without the feature (the symbol is missing) ------------------------------
def _plan(lib, log2_b, files, rq, data_bytes):
    n = len(rq)
    first = np.full(n + 1, 99, np.uint64)
    written = np.full(n, 99, np.uint64)
    some = np.full(n, 99, np.uint8)
    code = lib.nrg_memfs_pwrite_plan(log2_b, files, C.c_void_p(rq.ctypes.data), n, data_bytes, C.c_void_p(first.ctypes.data),
                                     C.c_void_p(written.ctypes.data), C.c_void_p(some.ctypes.data))
    return code, first, written, some


@pytest.mark.parametrize("name,files,log2_b,rq", LISTS, ids=[l[0] for l in LISTS])
def test_plan_agrees_with_the_model(nrgpu_mod, name, files, log2_b, rq):
    lib = nrgpu_mod.load()
    B = 1 << log2_b
    data = P.pattern(DATA_BYTES, 1)
    _, first, written, some = P.cut(rq, data, files, B)
    code, f, w, s = _plan(lib, log2_b, files, rq, DATA_BYTES)
    assert code == 0
    assert np.array_equal(f, first) and np.array_equal(w, written) and np.array_equal(s, some)
    for i in range(len(rq)):  # and one request per call
        code, f, w, s = _plan(lib, log2_b, files, rq[i:i + 1], DATA_BYTES)
        assert code == 0 and f[0] == 0 and f[1] == first[i + 1] - first[i] and w[0] == written[i] and s[0] == some[i]


def test_plan_errors(nrgpu_mod):
    lib, L = nrgpu_mod.load(), nrgpu_mod._lib
    ok = P.reqs([(5, 0, 10, 0)])
    for log2_b, files in ((6, 1), (27, 1), (12, 0), (12, (1 << 16) + 1), (26, 16)):
        assert _plan(lib, log2_b, files, ok, 10)[0] == L.NRG_E_INVAL
    assert _plan(lib, 26, 8, ok, 10)[0] == 0
    first = np.zeros(2, np.uint64)
    assert lib.nrg_memfs_pwrite_plan(12, 1, None, 1, 10, C.c_void_p(first.ctypes.data), None, None) == L.NRG_E_INVAL
    assert lib.nrg_memfs_pwrite_plan(12, 1, C.c_void_p(ok.ctypes.data), 1, 10, None, None, None) == L.NRG_E_INVAL
    assert lib.nrg_memfs_pwrite_plan(12, 1, C.c_void_p(ok.ctypes.data), 1, 10, C.c_void_p(first.ctypes.data), None, None) == 0
    assert list(first) == [0, 1]
    assert lib.nrg_memfs_pwrite_plan(12, 1, None, 0, 0, None, None, None) == 0
    # a valid request's bytes lie inside data; a failing or empty request's data_off is not looked at
    assert _plan(lib, 12, 1, ok, 9)[0] == L.NRG_E_INVAL
    assert _plan(lib, 12, 1, P.reqs([(5, 0, 10, 1)]), 10)[0] == L.NRG_E_INVAL
    assert _plan(lib, 12, 1, P.reqs([(5, 0, 10, (1 << 64) - 4)]), 1000)[0] == L.NRG_E_INVAL
    assert _plan(lib, 12, 1, P.reqs([(5, 7, 0, 1000), (9, 0, 10, 1000), (5, 4090, 10, 1000)]), 0)[0] == 0


# ---- ABI ---------------------------------------------------------------------------------------------
def test_request_is_32_bytes_and_the_symbols_are_exported(nrgpu_mod):
    L = nrgpu_mod._lib
    lib = nrgpu_mod.load()
    assert L.MEMFS_WR_DTYPE.itemsize == 32 and L.MEMFS_WR_DTYPE == P.WR_DTYPE == nrgpu_mod.MEMFS_WR_DTYPE
    assert [L.MEMFS_WR_DTYPE.fields[f][1] for f in ("ino", "offset", "len", "data_off")] == [0, 8, 16, 24]
    hdr = open(os.path.join(ROOT, "include", "nrgpu.h")).read()
    assert re.search(r"uint64_t ino, offset, len, data_off;\s*\} nrg_memfs_wr; /\* 32 B \*/", hdr)
    for name, nargs in (("nrg_memfs_pwrite_plan", 8), ("nrg_memfs_pwrite_async", 9), ("nrg_memfs_pwrite", 9),
                        ("nrg_memfs_pwrite_records_async", 8)):
        assert hasattr(lib, name) and name in L.SIGNATURES
        res, args = L.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs
        assert re.search(r"int %s\(" % name, hdr)
    # a NULL context is refused before anything else
    assert lib.nrg_memfs_pwrite_async(None, None, 0, None, 0, 1, None, None, None) == L.NRG_E_INVAL
    assert lib.nrg_memfs_pwrite(None, None, 0, None, 0, 1, None, None, None) == L.NRG_E_INVAL
    assert lib.nrg_memfs_pwrite_records_async(None, None, 0, None, 0, None, 0, None) == L.NRG_E_INVAL


def test_the_out_of_scope_lines_are_gone_and_the_others_stay():
    hdr = open(os.path.join(ROOT, "include", "nrgpu.h")).read()
    src = open(os.path.join(ROOT, "node-replication_amd", "csrc", "memfs.hip")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "whole-file 4096-byte ops" not in hdr
    assert "Out of scope: benches/nrfs.rs" not in src
    assert "no `nrfs.rs` whole-file `FileWrite`" not in readme
    assert "capacity growth past B" in hdr and "directories" in hdr and "partitioned" in hdr and "combiner" in hdr
    assert "Out of scope: the combiner, partitioned groups and growth" in src


# ---- the Python codec ----------------------------------------------------------------------------------
def test_python_surface(nrgpu_mod):
    N = nrgpu_mod
    for m in ("mf_pwrite", "mf_pwrite_records", "mf_pwrite_device", "mf_pwrite_records_device"):
        assert callable(getattr(N.DeviceReplica, m))
    assert N.MfPwrite(5, 0, b"x").data == b"x"
    assert callable(N.MemFs.encode_for) and callable(N.MemFs.encode_counts)


def test_encode_counts_is_the_models_cut(nrgpu_mod):
    N = nrgpu_mod
    B, files = 4096, 3
    rq = P.edges(files, B, DATA_BYTES)
    data = P.pattern(DATA_BYTES, 4)
    ops = []
    for r in rq:
        some, _ = P.answer(r, files, B)
        ln, doff = int(r["len"]), int(r["data_off"])
        body = bytes(data[doff:doff + ln]) if some else bytes(min(ln, 300))  # a failing op's bytes do not matter
        if not some and ln > 300:
            continue  # (an op carries its bytes: 2^63 of them cannot be made)
        ops.append(N.MfPwrite(int(r["ino"]), int(r["offset"]), body))
    ops.insert(3, N.MfRead(5, 0, 16))
    ops.append(N.MfWrite(5, 0, b"y" * 129))
    recs, counts = N.MemFs.encode_counts(ops, 12, files)
    want, pos = [], 0
    for o in ops:
        if isinstance(o, N.MfPwrite):
            want.append(P.cut(P.reqs([(o.ino, o.offset, len(o.data), 0)]), np.frombuffer(o.data, np.uint8), files, B)[0])
        else:
            want.append(N.MemFs.encode([o]))
    assert counts == [len(w) for w in want] and sum(counts) == len(recs)
    assert np.concatenate(want).tobytes() == recs.tobytes()
    # the responses fold into one answer per op
    m = M.MemFsModel(files, 12)
    resp, some = m.replay(recs)
    got = N.MemFs.decode_ops(ops, resp, some, counts)
    ref = M.MemFsModel(files, 12)
    for o, g in zip(ops, got):
        if isinstance(o, N.MfPwrite):
            s, w = P.answer({"ino": o.ino, "offset": o.offset, "len": len(o.data)}, files, B)
            assert g == (("written", w) if s else ("err", w))
            if s and o.data:
                ref.data[o.ino - 5][o.offset:o.offset + len(o.data)] = o.data
        elif isinstance(o, N.MfRead):
            assert g == ("data", bytes(ref.data[0][:16]))
        else:
            assert g == ("err", M.EINVAL)  # an MfWrite of more than 128 bytes still answers EINVAL
    with pytest.raises(TypeError):
        N.MemFs.encode([N.MfPwrite(5, 0, b"x")])
