"""The replicated skip list (ordered map, csrc/skiplist.hip) against the sequential model of
tests/skiplist_model.py: every response, dump, length, digest and read is compared bit for bit.
There are no tolerances. Chunk sizes sit at 1, 2, 63, 64, 65 and around every tile constant the
model mirrors from the kernels."""
import ctypes as C

import numpy as np
import pytest

import skiplist_model as M

pytestmark = pytest.mark.gpu

U64_MAX = 2**64 - 1
MIN_LOG_BYTES = 2 * 32 * 256 * 64
SIZES = sorted({1, 2, 63, 64, 65} | {t + d for t in M.TILE_CONSTANTS.values() for d in (-1, 0, 1)})
BASE = 1 << 32
BASE_KEYS = [BASE + 1000 * i for i in range(100)]       # what the populated map holds in its base run
DELTA_KEYS = [BASE + 1000 * i + 500 for i in range(40)]  # and in its delta run


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def _recs(nrg, keys, vals):
    r = np.zeros(len(keys), nrg.PUT_DTYPE)
    r["key"], r["val"] = np.array(keys, np.uint64), np.array(vals, np.uint64)
    return r


def _open(nrg, log2=13, delta_max=64, **kw):
    kw.setdefault("max_batch", 4096)
    kw.setdefault("log_bytes", MIN_LOG_BYTES)
    knobs = {"SL_DELTA_MAX": delta_max} if delta_max else None
    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_SKIPLIST, 0, knobs=knobs, log2_slots=log2, **kw)
    model = M.SkipListModel(delta_max or min(1 << log2, M.DELTA_DEFAULT), kw["max_batch"])
    return dev, model


def _round(nrg, dev, recs, origin=1):
    """one fused round; (resp, some) of its records"""
    import torch

    n = len(recs)
    d_ops = _cuda(recs) if n else None
    resp = torch.zeros(max(n, 1), dtype=torch.int64, device="cuda")
    some = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
    dev.sl_round_device(d_ops, n, origin, resp, some)
    dev.sync()
    return resp.cpu().numpy().view(np.uint64)[:n], some.cpu().numpy()[:n]


def _both(nrg, dev, model, keys, vals):
    """the same records through the device and the model; the responses are (key, 1)"""
    recs = _recs(nrg, keys, vals)
    resp, some = _round(nrg, dev, recs)
    mresp, msome = model.replay(recs)
    assert np.array_equal(resp, mresp) and np.array_equal(some, msome)
    assert np.array_equal(resp, recs["key"]) and (some == 1).all()


def _check(dev, model):
    k, v = dev.sl_dump()
    mk, mv = model.arrays()
    assert np.array_equal(k, mk) and np.array_equal(v, mv)
    assert dev.sl_len() == len(model)
    assert dev.digest() == model.digest()


def _populate(nrg, dev, model, ends=False):
    """base and delta both hold keys (delta_max = 64): 100 keys compact into base, 40 stay in delta"""
    rng = np.random.default_rng(1)
    _both(nrg, dev, model, BASE_KEYS[::-1], rng.integers(0, U64_MAX, 100, dtype=np.uint64))
    _both(nrg, dev, model, DELTA_KEYS, rng.integers(0, U64_MAX, 40, dtype=np.uint64))
    if ends:
        _both(nrg, dev, model, [U64_MAX, 0], [11, 12])
    assert model.compactions == 1 and model.nb == 100 and model.nd == (42 if ends else 40)


def _pattern(name, n):
    new = [BASE + 2 * i + 1 for i in range(n)]  # odd offsets: in neither run, between their keys
    if name == "asc":
        return new
    if name == "desc":
        return new[::-1]
    if name == "equal":
        return [BASE + 77] * n
    if name == "twice":
        h = n // 2
        return (new[:h] + new[:h] + new[h:h + 1])[:n] if h else new
    if name == "hits_base":
        return [BASE_KEYS[(7 * i) % 100] for i in range(n)]
    if name == "hits_delta":
        return [DELTA_KEYS[(3 * i) % 40] for i in range(n)]
    if name == "mix":
        return [(BASE_KEYS[i % 100], DELTA_KEYS[i % 40], new[i])[i % 3] for i in range(n)]
    if name == "below":
        return [n - i for i in range(n)]
    if name == "above":
        return [(1 << 63) + 5 * i for i in range(n)]
    if name == "ends":
        return [(0, U64_MAX, new[i])[i % 3] for i in range(n)]
    raise KeyError(name)


PATTERNS = ["asc", "desc", "equal", "twice", "hits_base", "hits_delta", "mix", "below", "above", "ends"]


@pytest.mark.parametrize("n", SIZES)
def test_chunk_shapes(nrg, n):
    rng = np.random.default_rng(n)
    for populated in (False, True):
        for name in PATTERNS:
            dev, model = _open(nrg)
            if populated:
                _populate(nrg, dev, model, ends=name == "ends")
            _both(nrg, dev, model, _pattern(name, n), rng.integers(0, U64_MAX, n, dtype=np.uint64))
            _check(dev, model)
            dev.close()


# ---- policy -------------------------------------------------------------------------------------------
def test_compaction_threshold_and_update_rounds(nrg):
    dev, model = _open(nrg, delta_max=64)
    dev.kernel_timing(True)
    _both(nrg, dev, model, range(100, 140), range(40))
    _both(nrg, dev, model, range(200, 224), range(24))  # nd = 64 exactly: no compaction
    _check(dev, model)
    assert (model.nd, model.compactions) == (64, 0) and dev.kernel_time("sl_compact")[0] == 0
    _both(nrg, dev, model, list(range(100, 140)) * 10, range(400))  # updates only: nd unchanged
    assert (model.nd, model.compactions) == (64, 0) and dev.kernel_time("sl_compact")[0] == 0
    _check(dev, model)
    _both(nrg, dev, model, [7], [7])  # nd = 65: one compaction
    assert (model.nb, model.nd, model.compactions) == (65, 0, 1) and dev.kernel_time("sl_compact")[0] == 1
    _check(dev, model)
    _both(nrg, dev, model, list(range(100, 140)) + [7], range(41))  # updates of base keys
    assert dev.kernel_time("sl_compact")[0] == 1
    _check(dev, model)
    assert dev.kernel_time("sl_sort")[0] == 5 and dev.kernel_time("sl_merge")[0] == 5
    dev.close()


def test_twenty_mixed_rounds_follow_the_models_compactions(nrg):
    dev, model = _open(nrg, delta_max=64)
    dev.kernel_timing(True)
    rng = np.random.default_rng(20)
    sizes = [1, 30, 70, 2, 257, 64, 65, 10, 1025, 3, 40, 20, 5, 2049, 63, 1, 33, 31, 500, 17]
    for i, n in enumerate(sizes):
        span = 300 if i % 3 else 1 << 62  # small spans bring updates, large ones new keys
        _both(nrg, dev, model, rng.integers(0, span, n, dtype=np.uint64), rng.integers(0, U64_MAX, n, dtype=np.uint64))
        _check(dev, model)
        assert dev.kernel_time("sl_compact")[0] == model.compactions, f"round {i}"
    assert model.compactions >= 2
    dev.close()


# ---- chunking, entry points, log wrap -------------------------------------------------------------------
def _dup_stream(n, seed):
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 400, n, dtype=np.uint64)
    keys[250:262] = 5  # one key across the 256 boundary, others across 512 and 768
    keys[510:515] = 6
    keys[767:770] = U64_MAX
    return keys, rng.integers(0, U64_MAX, n, dtype=np.uint64)


@pytest.mark.parametrize("window", [(0, 1000), (350, 650)])
def test_chunked_exec_equals_one_chunk(nrg, window):
    keys, vals = _dup_stream(1000, 3)
    recs = _recs(nrg, keys, vals)
    out = []
    for mb in (256, 4096):
        dev, model = _open(nrg, max_batch=mb)
        first = dev.log_append(recs, 1)
        assert first == 0
        resp, some = dev.log_exec(first + window[0], first + window[1])
        model.replay(recs)
        _check(dev, model)
        assert np.array_equal(resp, keys[window[0]:window[1]]) and (some == 1).all()
        out.append((dev.sl_dump(), resp.copy()))
        dev.close()
    assert np.array_equal(out[0][0][0], out[1][0][0]) and np.array_equal(out[0][0][1], out[1][0][1])


def test_round_equals_append_plus_exec_and_segments(nrg):
    import torch

    keys, vals = _dup_stream(900, 4)
    recs = _recs(nrg, keys, vals)
    a, model = _open(nrg)
    b, _ = _open(nrg)
    s, _ = _open(nrg)
    ra, sa = _round(nrg, a, recs, origin=2)
    d = _cuda(recs)
    rb = torch.zeros(900, dtype=torch.int64, device="cuda")
    sb = torch.zeros(900, dtype=torch.uint8, device="cuda")
    first = b.log_append_device(d, 900, 2)
    b.log_exec_device(first, first + 900, rb, sb)
    b.sync()
    assert np.array_equal(ra, rb.cpu().numpy().view(np.uint64)) and np.array_equal(sa, sb.cpu().numpy())
    # two segments of two origins: 500 records of origin 1, then 400 of origin 2, stride 512
    seg = np.zeros(1024, nrg.PUT_DTYPE)
    seg[:500], seg[512:912] = recs[:500], recs[500:]
    ds = _cuda(seg)
    firsts = s.log_append_segments(ds, 512, [500, 400], [1, 2])
    assert firsts == [0, 500]
    rs = torch.zeros(400, dtype=torch.int64, device="cuda")
    ss = torch.zeros(400, dtype=torch.uint8, device="cuda")
    s.log_exec_device(500, 900, rs, ss)
    s.sync()
    assert np.array_equal(rs.cpu().numpy().view(np.uint64), keys[500:]) and (ss.cpu().numpy() == 1).all()
    model.replay(recs)
    for dev in (a, b, s):
        _check(dev, model)
        assert dev.log_state()["tail"] == 900 and dev.log_state()["ltail"] == 900
        dev.close()


def test_log_wraps_twice(nrg):
    dev, model = _open(nrg, max_batch=2048)
    size = dev.log_state()["size"]
    rng = np.random.default_rng(6)
    rounds = 0
    while dev.log_state()["tail"] <= 2 * size + 1000:
        n = 1500 + 97 * (rounds % 5)
        _both(nrg, dev, model, rng.integers(0, 3000, n, dtype=np.uint64), rng.integers(0, U64_MAX, n, dtype=np.uint64))
        rounds += 1
        if rounds % 6 == 0:
            _check(dev, model)
    _check(dev, model)
    assert dev.log_state()["tail"] > 2 * size
    dev.close()


# ---- reads ----------------------------------------------------------------------------------------------
def _queries(model, seed):
    ks = model.keys
    q = set(ks) | {k + 1 for k in ks if k < U64_MAX} | {k - 1 for k in ks if k > 0} | {0, U64_MAX}
    rng = np.random.default_rng(seed)
    q |= set(rng.integers(0, U64_MAX, 200, dtype=np.uint64).tolist()) | set(rng.integers(0, 3 * BASE, 200, dtype=np.uint64).tolist())
    return np.array(sorted(q), np.uint64)


def _check_reads(nrg, dev, model, seed):
    L = nrg._lib
    q = _queries(model, seed)
    v, f = dev.sl_get(q)
    want = [model.get(k) for k in q.tolist()]
    assert f.tolist() == [int(w is not None) for w in want] and v.tolist() == [w or 0 for w in want]
    for mode in (L.NRG_SEEK_GE, L.NRG_SEEK_GT, L.NRG_SEEK_LE, L.NRG_SEEK_LT):
        ok, ov, fo = dev.sl_seek(q, mode)
        want = [model.seek(k, mode) for k in q.tolist()]
        assert fo.tolist() == [int(w is not None) for w in want], mode
        assert ok.tolist() == [w[0] if w else 0 for w in want] and ov.tolist() == [w[1] if w else 0 for w in want], mode
    rng = np.random.default_rng(seed + 1)
    los, his = rng.choice(q, 300), rng.choice(q, 300)
    los[:3], his[:3] = [0, U64_MAX, 5], [U64_MAX, 0, 5]
    assert dev.sl_range_count(los, his).tolist() == [model.range_count(a, b) for a, b in zip(los.tolist(), his.tolist())]


@pytest.mark.parametrize("state", ["empty", "base", "delta", "both"])
def test_reads(nrg, state):
    dev, model = _open(nrg, max_reads=1 << 14)
    rng = np.random.default_rng(8)
    if state in ("base", "both"):
        _both(nrg, dev, model, [0] + BASE_KEYS, rng.integers(1, U64_MAX, 101, dtype=np.uint64))
        assert model.nd == 0 and model.nb == 101
    if state in ("delta", "both"):
        _both(nrg, dev, model, DELTA_KEYS + [U64_MAX], rng.integers(1, U64_MAX, 41, dtype=np.uint64))
        assert model.nd == 41
    _check_reads(nrg, dev, model, 30)
    if state == "both":
        # range windows inside one run and across both; cap one short copies nothing
        for lo, hi in ((BASE, BASE + 400), (BASE + 500, BASE + 500), (BASE + 1, BASE + 39999), (0, U64_MAX),
                       (BASE + 5000, U64_MAX), (9, 3)):
            k, v = dev.sl_range(lo, hi)
            assert list(zip(k.tolist(), v.tolist())) == model.range(lo, hi), (lo, hi)
        lib, n = dev._lib, C.c_uint64()
        kb, vb = np.full(200, 7, np.uint64), np.full(200, 7, np.uint64)
        want = len(model.range(BASE, BASE + 39999))
        rc = lib.nrg_skiplist_range(dev._h, BASE, BASE + 39999, kb.ctypes.data, vb.ctypes.data, want - 1, C.byref(n))
        assert rc == nrg._lib.NRG_E_CAPACITY and n.value == want and (kb == 7).all() and (vb == 7).all()
        rc = lib.nrg_skiplist_dump(dev._h, kb.ctypes.data, vb.ctypes.data, len(model) - 1, C.byref(n))
        assert rc == nrg._lib.NRG_E_CAPACITY and n.value == len(model) and (kb == 7).all()
    dev.close()


def test_read_rules(nrg):
    L = nrg._lib
    dev, model = _open(nrg, max_reads=64)
    _both(nrg, dev, model, [1, 2, 3], [4, 5, 6])
    dev.log_append(_recs(nrg, [9], [9]), 1)
    q = np.arange(10, dtype=np.uint64)
    for call in (lambda: dev.sl_get(q), lambda: dev.sl_seek(q, L.NRG_SEEK_GE), lambda: dev.sl_range_count(q, q),
                 lambda: dev.sl_range(0, 10)):
        with pytest.raises(nrg.NrgError) as e:
            call()
        assert e.value.code == L.NRG_E_NOT_SYNCED
    dev.log_exec()
    assert dev.sl_get(q)[1].tolist() == [0, 1, 1, 1, 0, 0, 0, 0, 0, 1]
    q = np.arange(65, dtype=np.uint64)
    for call in (lambda: dev.sl_get(q), lambda: dev.sl_seek(q, L.NRG_SEEK_LT), lambda: dev.sl_range_count(q, q)):
        with pytest.raises(nrg.NrgError) as e:
            call()
        assert e.value.code == L.NRG_E_CAPACITY
    with pytest.raises(nrg.NrgError) as e:
        dev.sl_seek(q[:4], 4)
    assert e.value.code == L.NRG_E_INVAL
    dev.close()


# ---- prefill ----------------------------------------------------------------------------------------------
def test_prefill_range_is_the_references_default(nrg):
    n = 5000  # more than one chunk of 4096
    dev, model = _open(nrg)
    dev.sl_prefill_range(n, 0)
    model.insert_many(range(n), range(n))
    _check(dev, model)
    q = np.array([0, 1, n - 1, n, n + 1, U64_MAX], np.uint64)
    v, f = dev.sl_get(q)
    assert v.tolist() == [0, 1, n - 1, 0, 0, 0] and f.tolist() == [1, 1, 1, 0, 0, 0]
    assert dev.log_state()["tail"] == 0  # no log traffic
    dev.sl_prefill_range(10, 3)  # on a non-empty map: values replaced
    model.insert_many(range(10), range(3, 13))
    _check(dev, model)
    dev.close()


def test_prefill_unsorted_with_duplicates(nrg):
    dev, model = _open(nrg, max_batch=512)
    rng = np.random.default_rng(9)
    for n in (1300, 700):  # on the empty map, then on what that left
        keys = rng.integers(0, 900, n, dtype=np.uint64)
        keys[::50] = U64_MAX
        vals = rng.integers(0, U64_MAX, n, dtype=np.uint64)
        dev.sl_prefill(keys, vals)
        model.insert_many(keys.tolist(), vals.tolist())
        _check(dev, model)
    dev.close()


def test_merges_beyond_one_grid(nrg):
    """More merge partitions than workgroups are launched (the merge strides over them), and chunks of
    max_batch = 2^20 through the radix sort: 9M keys, the digest and spot reads against numpy."""
    L = nrg._lib
    n, off = 9_000_000, 5
    dev, _ = _open(nrg, log2=24, delta_max=1 << 20, max_batch=1 << 20)
    dev.sl_prefill_range(n, off)
    assert dev.sl_len() == n
    keys = np.arange(n, dtype=np.uint64)
    assert dev.digest() == nrg.digest.pairs(keys, keys + np.uint64(off))
    q = np.array([0, 1, M.SL_MERGE_PART - 1, M.SL_MERGE_PART, 4096 * M.SL_MERGE_PART - 1, 4096 * M.SL_MERGE_PART,
                  n - 1, n, U64_MAX], np.uint64)
    v, f = dev.sl_get(q)
    assert f.tolist() == [1] * 7 + [0, 0] and v[:7].tolist() == (q[:7] + np.uint64(off)).tolist()
    ok, ov, fo = dev.sl_seek(q, L.NRG_SEEK_LT)
    assert fo.tolist() == [0] + [1] * 8 and ok[1:].tolist() == [0, 2046, 2047, 8388606, 8388607, n - 2, n - 1, n - 1]
    lo = 4096 * M.SL_MERGE_PART - 3
    k, vv = dev.sl_range(lo, lo + 5)
    assert k.tolist() == list(range(lo, lo + 6)) and vv.tolist() == [x + off for x in range(lo, lo + 6)]
    assert dev.sl_range_count([0, 7], [U64_MAX, n + 9]).tolist() == [n, n - 7]
    dev.close()


# ---- capacity ---------------------------------------------------------------------------------------------
def test_fixed_capacity_latches_once(nrg):
    L = nrg._lib
    dev, model = _open(nrg, log2=10, delta_max=0)
    assert dev.sl_capacity() == 1024
    for at in range(0, 1024, 300):
        ks = list(range(3 * at, 3 * min(at + 300, 1024), 3))
        _both(nrg, dev, model, ks, ks)
    _both(nrg, dev, model, [0, 3, 6], [1, 1, 1])  # updates at capacity are fine
    _check(dev, model)
    assert dev.sl_len() == 1024
    one = _cuda(_recs(nrg, [1], [1]))
    dev.sl_round_device(one, 1, 1)
    with pytest.raises(nrg.NrgError) as e:
        dev.sync()
    assert e.value.code == L.NRG_E_CAPACITY
    dev.sync()  # latched once
    assert dev.sl_len() <= 1024
    dev.close()


def test_reserve(nrg):
    L = nrg._lib
    dev, model = _open(nrg, log2=10)
    _populate(nrg, dev, model)
    dev.sl_reserve(3000)
    assert dev.sl_capacity() == 3000
    _check(dev, model)
    dev.sl_reserve(100)  # never shrinks
    assert dev.sl_capacity() == 3000
    ks = [BASE + 2 * i + 1 for i in range(2800)]
    _both(nrg, dev, model, ks, ks)
    _check(dev, model)
    with pytest.raises(nrg.NrgError) as e:
        dev.sl_reserve((1 << 28) + 1)
    assert e.value.code == L.NRG_E_INVAL and dev.sl_capacity() == 3000
    dev.close()


def test_automatic_growth(nrg):
    L = nrg._lib
    dev, model = _open(nrg, log2=10, max_batch=1024)
    with pytest.raises(nrg.NrgError) as e:
        dev.set_max_capacity(1000)  # below the capacity
    assert e.value.code == L.NRG_E_INVAL
    dev.set_max_capacity(1 << 13)
    rng = np.random.default_rng(12)
    for r in range(8):  # 4800 distinct keys and some updates: four times the open capacity and more
        ks = np.concatenate([np.arange(600 * r, 600 * (r + 1), dtype=np.uint64) * 7, rng.integers(0, 4000, 100, dtype=np.uint64) * 7])
        rng.shuffle(ks)
        _both(nrg, dev, model, ks, rng.integers(0, U64_MAX, len(ks), dtype=np.uint64))
        _check(dev, model)
    assert len(model) >= 4 * 1024 and 4096 < dev.sl_capacity() <= 1 << 13
    dev.close()
    # a stream of updates never reallocates
    dev, model = _open(nrg, log2=10, max_batch=1024)
    dev.set_max_capacity(1 << 13)
    _both(nrg, dev, model, range(500), range(500))
    for r in range(10):
        _both(nrg, dev, model, range(500), range(r, r + 500))
    _check(dev, model)
    assert dev.sl_capacity() == 1024
    dev.close()


# ---- digest, snapshot, restore -------------------------------------------------------------------------
def test_digest_equals_a_hashmaps(nrg):
    L = nrg._lib
    dev, model = _open(nrg)
    _populate(nrg, dev, model, ends=True)
    hm = nrg.DeviceReplica(L.NRG_DS_HASHMAP, 0, log2_slots=12, max_batch=4096, log_bytes=MIN_LOG_BYTES)
    k, v = model.arrays()
    first = hm.log_append(_recs(nrg, k[::-1], v[::-1]), 1)
    hm.log_exec()
    assert dev.digest() == model.digest() == hm.digest()
    hm.close()
    dev.close()


def test_snapshot_restore_into_another_shape(nrg):
    L = nrg._lib
    src, model = _open(nrg, log2=12, delta_max=64)
    _populate(nrg, src, model, ends=True)
    img = src.snapshot()
    info, (k, v) = nrg.snapshot.unpack(img)
    mk, mv = model.arrays()
    assert info.ds_kind == L.NRG_DS_SKIPLIST and info.items == len(model) and info.digest == model.digest()
    assert np.array_equal(k, mk) and np.array_equal(v, mv) and info.log_idx == src.log_state()["ltail"]
    assert info.bytes == nrg.snapshot.image_bytes(L.NRG_DS_SKIPLIST, len(model))
    dst, dmodel = _open(nrg, log2=10, delta_max=16)
    _both(nrg, dst, dmodel, [1, 2, 3], [1, 2, 3])  # replaced by the restore
    dst.restore(img)
    dmodel.restore(model.items())
    _check(dst, dmodel)
    a, b = src.log_state(), dst.log_state()
    assert all(b[f] == info.log_idx for f in ("head", "tail", "ctail", "ltail")) and a["ltail"] == b["ltail"]
    assert dst.log_append(_recs(nrg, [5], [5]), 1) == info.log_idx
    dst.log_exec()
    dmodel.replay([(5, 5)])
    _both(nrg, src, model, [5], [5])
    ks = DELTA_KEYS[:10] + [BASE + 2 * i + 1 for i in range(30)] + [0]
    _both(nrg, src, model, ks, range(len(ks)))
    _both(nrg, dst, dmodel, ks, range(len(ks)))
    _check(src, model)
    _check(dst, dmodel)
    assert src.digest() == dst.digest()
    src.close()
    dst.close()


def test_restore_rejects_bad_images(nrg):
    L = nrg._lib
    S = nrg.snapshot
    dev, model = _open(nrg, log2=10)
    _both(nrg, dev, model, [1, 2], [3, 4])
    good = S.pack(L.NRG_DS_SKIPLIST, {10 * i: i for i in range(50)}, 9)
    swapped = good.copy()
    pay = swapped[64:64 + 50 * 16].view("<u8").reshape(-1, 2)
    pay[[20, 21]] = pay[[21, 20]]  # the digest words still match: only the order check sees it
    with pytest.raises(nrg.NrgError) as e:
        dev.restore(swapped)
    assert e.value.code == L.NRG_E_INVAL
    wrong = S.pack(L.NRG_DS_HASHMAP, {1: 1}, 0)
    with pytest.raises(nrg.NrgError) as e:
        dev.restore(wrong)
    assert e.value.code == L.NRG_E_INVAL
    big = S.pack(L.NRG_DS_SKIPLIST, {i: i for i in range(1025)}, 0)
    with pytest.raises(nrg.NrgError) as e:
        dev.restore(big)
    assert e.value.code == L.NRG_E_CAPACITY
    dev.restore(good)
    model.restore([(10 * i, i) for i in range(50)])
    _check(dev, model)
    assert dev.log_state()["tail"] == 9
    dev.set_max_capacity(2048)  # with a bound the larger image is taken, growing first
    dev.restore(big)
    model.restore([(i, i) for i in range(1025)])
    _check(dev, model)
    assert dev.sl_capacity() >= 1025
    dev.close()


# ---- group ------------------------------------------------------------------------------------------------
def _view(nrg, h):
    """a DeviceReplica over a handle the group owns (never closed from here)"""
    d = nrg.DeviceReplica.__new__(nrg.DeviceReplica)
    d.kind, d.device, d._h, d._lib = nrg._lib.NRG_DS_SKIPLIST, 0, C.c_void_p(h), nrg._lib.load()
    return d


def test_group_rounds_verify_and_resync(nrg):
    import torch

    L = nrg._lib
    lib = L.load()
    cfg = L.default_config(L.NRG_DS_SKIPLIST)
    cfg.log2_slots, cfg.max_batch, cfg.log_bytes = 12, 2048, MIN_LOG_BYTES
    L.check(lib.nrg_test_loopback_collectives(1))
    g = C.c_void_p()
    try:
        L.check(lib.nrg_group_open((C.c_int * 2)(0, 0), 2, C.byref(cfg), C.byref(g)), "nrg_group_open")
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))
    members = [_view(nrg, lib.nrg_group_replica(g, i)) for i in range(2)]
    model = M.SkipListModel(min(1 << 12, M.DELTA_DEFAULT), 2048)
    rng = np.random.default_rng(14)
    keep = []
    try:
        for r, lens in enumerate([(300, 70), (0, 1100), (45, 9)]):
            rd = (L.Round * 2)()
            want = []
            for i, n in enumerate(lens):
                recs = _recs(nrg, rng.integers(0, 800, n, dtype=np.uint64), rng.integers(0, U64_MAX, n, dtype=np.uint64))
                model.replay(recs)  # rank order: W_0 || W_1
                d_ops = _cuda(recs) if n else None
                resp = torch.zeros(max(n, 1), dtype=torch.int64, device="cuda")
                some = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
                rd[i].recs, rd[i].n, rd[i].resp, rd[i].some = (d_ops.data_ptr() if n else 0), n, resp.data_ptr(), some.data_ptr()
                keep.append((d_ops, resp, some))
                want.append((recs["key"], resp, some, n))
            torch.cuda.synchronize()
            L.check(lib.nrg_group_round_async(g, rd, None), f"round {r}")
            L.check(lib.nrg_group_sync(g))
            for key, resp, some, n in want:
                assert np.array_equal(resp.cpu().numpy().view(np.uint64)[:n], key) and (some.cpu().numpy()[:n] == 1).all()
            same = C.c_int(-1)
            L.check(lib.nrg_group_verify(g, None, C.byref(same)))
            assert same.value == 1
            _check(members[0], model)
        _check(members[1], model)
        # a foreign Put on member 1 alone
        _round(nrg, members[1], _recs(nrg, [U64_MAX], [1]), origin=2)
        same = C.c_int(-1)
        L.check(lib.nrg_group_verify(g, None, C.byref(same)))
        assert same.value == 0
        L.check(lib.nrg_group_resync(g, 0))
        L.check(lib.nrg_group_verify(g, None, C.byref(same)))
        assert same.value == 1
        _check(members[1], model)
        _check(members[0], model)
    finally:
        for m in members:
            m._h = None
        assert lib.nrg_group_close(g) == L.NRG_OK


# ---- kind guards, Python API, configurations -----------------------------------------------------------
def test_kind_guards(nrg):
    L = nrg._lib
    lib = L.load()
    st = nrg.DeviceReplica(L.NRG_DS_STACK, 0, stack_capacity=1 << 10, max_batch=1024, log_bytes=MIN_LOG_BYTES)
    ops = np.zeros(4, nrg.STACK_OP_DTYPE)
    ops["val"], ops["op"] = [1, 2, 3, 4], 1
    st.log_append(ops, 1)
    before = st.log_state()
    h, n, E = st._h, C.c_uint64(), L.NRG_E_INVAL
    buf = np.zeros(64, np.uint64)
    p = buf.ctypes.data
    d = _cuda(buf)
    dp = d.data_ptr()
    assert lib.nrg_skiplist_round_async(h, dp, 1, 1, dp, dp) == E
    assert lib.nrg_skiplist_get(h, p, 1, p, p) == E and lib.nrg_skiplist_get_async(h, dp, 1, dp, dp) == E
    assert lib.nrg_skiplist_seek(h, p, 1, 0, p, p, p) == E and lib.nrg_skiplist_seek_async(h, dp, 1, 0, dp, dp, dp) == E
    assert lib.nrg_skiplist_range(h, 0, 9, p, p, 8, C.byref(n)) == E
    assert lib.nrg_skiplist_range_count(h, p, p, 1, p) == E and lib.nrg_skiplist_range_count_async(h, dp, dp, 1, dp) == E
    assert lib.nrg_skiplist_dump(h, p, p, 8, C.byref(n)) == E and lib.nrg_skiplist_len(h, C.byref(n)) == E
    assert lib.nrg_skiplist_prefill(h, p, p, 1) == E and lib.nrg_skiplist_prefill_range(h, 4, 0) == E
    assert lib.nrg_skiplist_reserve(h, 1 << 12) == E and lib.nrg_skiplist_capacity(h, C.byref(n)) == E
    assert lib.nrg_test_set_knob(h, L.KNOBS["SL_DELTA_MAX"], 8) == E
    assert st.log_state() == before and (buf == 0).all()
    st.log_exec()
    assert st.st_dump().tolist() == [1, 2, 3, 4]
    st.close()
    dev, model = _open(nrg)
    _both(nrg, dev, model, [1], [2])
    assert lib.nrg_hashmap_get(dev._h, p, 1, p, p) == E
    comb = C.c_void_p()
    assert lib.nrg_combiner_open(dev._h, 4, C.byref(comb)) == E
    # the knob: only on an empty context, 1 .. capacity
    assert lib.nrg_test_set_knob(dev._h, L.KNOBS["SL_DELTA_MAX"], 8) == E
    _check(dev, model)
    dev.close()
    dev, _ = _open(nrg, log2=10, delta_max=0)
    assert lib.nrg_test_set_knob(dev._h, L.KNOBS["SL_DELTA_MAX"], 0) == E
    assert lib.nrg_test_set_knob(dev._h, L.KNOBS["SL_DELTA_MAX"], 1025) == E
    assert lib.nrg_test_set_knob(dev._h, L.KNOBS["SL_DELTA_MAX"], 1024) == L.NRG_OK
    dev.close()


def test_python_replica_api(nrg):
    L = nrg._lib
    log = nrg.Log(MIN_LOG_BYTES)
    a = nrg.Replica(log, nrg.SkipList, 0, log2_slots=12, max_batch=1024)
    b = nrg.Replica(log, nrg.SkipList, 0, log2_slots=12, max_batch=1024)
    ta, tb = a.register(), b.register()
    model = M.SkipListModel()
    rng = np.random.default_rng(15)
    for i in range(40):
        k, v = int(rng.integers(0, 25)) * 10, int(rng.integers(0, U64_MAX, dtype=np.uint64))
        rep, tok = (a, ta) if i % 2 else (b, tb)
        assert rep.execute_mut(nrg.SlPush(k, v), tok) == k
        model.replay([(k, v)])
    for rep, tok in ((a, ta), (b, tb)):
        for k in (0, 5, 10, 240, 250, U64_MAX):
            assert rep.execute(nrg.Get(k), tok) == model.get(k)
            for mode in (L.NRG_SEEK_GE, L.NRG_SEEK_GT, L.NRG_SEEK_LE, L.NRG_SEEK_LT):
                assert rep.execute(nrg.Seek(k, mode), tok) == model.seek(k, mode)
    seen = []
    a.verify(seen.append)
    b.verify(seen.append)
    assert seen[0] == seen[1] == model.items()
    assert a.digest() == b.digest() == model.digest()
    c = nrg.Replica(log, nrg.SkipList, 0, log2_slots=10, max_batch=1024, clone_from=a)
    c.verify(seen.append)
    assert seen[2] == model.items()
    for r in (a, b, c):
        r.dev.close()


def test_smallest_and_rejected_configurations(nrg):
    L = nrg._lib
    lib = L.load()
    dev, model = _open(nrg, log2=M.LOG2_MIN, delta_max=0, max_batch=16, max_reads=16)
    assert dev.sl_capacity() == 16
    _both(nrg, dev, model, [9, 3, U64_MAX, 0, 9, 5, 6, 7, 8, 1, 2, 4, 10, 11, 12, 3], range(16))
    _check(dev, model)
    assert dev.sl_seek([4], L.NRG_SEEK_GT)[0].tolist() == [5]
    dev.close()
    for bad in (dict(log2_slots=M.LOG2_MIN - 1), dict(log2_slots=M.LOG2_MAX + 1), dict(max_batch=(1 << 24) + 1)):
        cfg = L.default_config(L.NRG_DS_SKIPLIST)
        cfg.log2_slots, cfg.log_bytes = 10, MIN_LOG_BYTES
        for k, v in bad.items():
            setattr(cfg, k, v)
        h = C.c_void_p()
        assert lib.nrg_open(0, C.byref(cfg), C.byref(h)) == L.NRG_E_INVAL and not h.value
    dev = nrg.DeviceReplica(L.NRG_DS_SKIPLIST, 0, log2_slots=10, max_batch=0, pipeline=1, log_bytes=MIN_LOG_BYTES)
    assert dev.cfg.max_batch == 0 and dev.sl_len() == 0  # 0: the default of the other kinds; pipeline accepted
    dev.close()
