"""pop_front / pop_back on the replicated skip list (nrg_skiplist_enable_pops, csrc/skiplist.hip) against
the sequential model of tests/skiplist_pop_model.py: every response, popped entry, dump, length and
digest is compared bit for bit; there are no tolerances. The oracle has no pops, so the model is the
reference; tests/test_skiplist_pop_cpu.py checks it against a heap restatement and shows that every
named stream has the property it is named for."""
import ctypes as C

import numpy as np
import pytest

import skiplist_pop_model as P

pytestmark = pytest.mark.gpu

U64_MAX = 2**64 - 1
LOG_BYTES = 4 * 2 * 32 * 256 * 64
PATHS = ["append_exec", "fused_round", "chunked", "window"]
POP_KERNELS = ("sl_pop_find", "sl_pop_plan", "sl_pop_take", "sl_pop_shift")
GUARD = 64  # bytes of guard words around a response window and behind the popped entries


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def _open(nrg, s, max_batch=None, enable=True, **kw):
    kw.setdefault("max_reads", 1 << 12)
    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_SKIPLIST, 0, knobs={"SL_DELTA_MAX": s.delta_max}, log2_slots=s.log2,
                            max_batch=max_batch or s.max_batch, log_bytes=LOG_BYTES, **kw)
    if s.removal:
        dev.sl_enable_removal()
    if enable:
        dev.sl_enable_pops()
    return dev, s.model(max_batch)


def _round_pops(dev, recs, cap, origin=1):
    """nrg_skiplist_round_pops_async with room for `cap` entries between guard words:
    (resp, some, keys[:min(total, cap)], vals[...], total)"""
    import torch

    n, g = len(recs), GUARD // 8
    resp = torch.zeros(n, dtype=torch.int64, device="cuda")
    some = torch.zeros(n, dtype=torch.uint8, device="cuda")
    pk = torch.full((cap + 2 * g,), -7, dtype=torch.int64, device="cuda")
    pv = torch.full((cap + 2 * g,), -7, dtype=torch.int64, device="cuda")
    pn = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    dev.sl_round_pops_device(_cuda(recs), n, origin, resp, some, pk.data_ptr() + GUARD, pv.data_ptr() + GUARD, cap,
                             pn.data_ptr() + 8)
    dev.sync()
    k, v, t = pk.cpu().numpy(), pv.cpu().numpy(), pn.cpu().numpy()
    assert t[0] == t[2] == -7
    total = int(t[1])
    got = min(total, cap)
    for a in (k, v):  # nothing before the arrays, nothing at or past min(total, pop_cap)
        assert (a[:g] == -7).all() and (a[g + got:] == -7).all(), np.flatnonzero(a != -7)[[0, -1]]
    return (resp.cpu().numpy().view(np.uint64), some.cpu().numpy(), k[g:g + got].view(np.uint64),
            v[g:g + got].view(np.uint64), total)


def _window(dev, recs, a, b):
    """append, then exec with the response window [a, b) of the chunk between guards"""
    import torch

    w = b - a
    resp = torch.full((w + 2 * GUARD // 8,), -7, dtype=torch.int64, device="cuda")
    some = torch.full((w + 2 * GUARD,), 9, dtype=torch.uint8, device="cuda")
    first = dev.log_append(recs, 1)
    dev.log_exec_device(first + a, first + b, resp.data_ptr() + GUARD, some.data_ptr() + GUARD)
    dev.sync()
    r, s = resp.cpu().numpy(), some.cpu().numpy()
    g = GUARD // 8
    assert (r[:g] == -7).all() and (r[g + w:] == -7).all() and (s[:GUARD] == 9).all() and (s[GUARD + w:] == 9).all()
    return r[g:g + w].view(np.uint64), s[GUARD:GUARD + w]


def _window_of(recs):
    """a window that begins and ends inside a pop run where the chunk has one of three records or more
    (else inside the chunk)"""
    n = len(recs)
    pop = np.isin(recs["val"], (P.FRONT, P.BACK))
    edges = np.flatnonzero(np.diff(np.concatenate([[0], pop.astype(np.int8), [0]])))
    runs = [(int(a), int(b)) for a, b in zip(edges[::2], edges[1::2]) if b - a >= 3]
    if len(runs) >= 2:
        return runs[0][0] + 1, runs[-1][1] - 1
    if runs:
        return runs[0][0] + 1, runs[0][1] - 1
    return (n // 3, n - n // 4) if n >= 4 else (0, n)


def _replay(dev, model, recs, path):
    """one chunk of the stream through the device and the model; every response and popped entry compared"""
    model.clear_popped()
    want_r, want_s = model.replay(recs)
    a, b = 0, len(recs)
    if path == "fused_round":
        resp, some, pk, pv, total = _round_pops(dev, recs, len(model.popped) + 5)
        assert total == len(model.popped)
        assert pk.tolist() == [k for k, _ in model.popped] and pv.tolist() == [v for _, v in model.popped]
    elif path == "window":
        a, b = _window_of(recs)
        resp, some = _window(dev, recs, a, b)
    else:
        first = dev.log_append(recs, 1)
        resp, some = dev.log_exec(first, first + len(recs))
    assert np.array_equal(some, want_s[a:b]), np.flatnonzero(some != want_s[a:b])[:8]
    assert np.array_equal(resp, want_r[a:b]), np.flatnonzero(resp != want_r[a:b])[:8]


def _state(nrg, dev, model):
    k, v = dev.sl_dump()
    mk, mv = model.arrays()
    assert np.array_equal(k, mk) and np.array_equal(v, mv)
    assert dev.sl_len() == len(model)
    assert dev.digest() == model.digest() == nrg.digest.skiplist(mk, mv)


def _reads(nrg, dev, model):
    """the read kernels on the runs the pops left: Get, the four seeks, a scan each way, range counts"""
    L = nrg._lib
    ks = model.keys
    pick = ks[:4] + ks[-4:] + ks[::max(1, len(ks) // 50)] + [0, 1, 99, 100, 10000, 19999, U64_MAX - 3, U64_MAX]
    q = np.array(sorted(set(pick) | {k + 1 for k in pick if k < U64_MAX} | {k - 1 for k in pick if k > 0}), np.uint64)
    ql = q.tolist()
    val, f = dev.sl_get(q)
    want = [model.get(x) for x in ql]
    assert f.tolist() == [int(w is not None) for w in want] and val.tolist() == [w or 0 for w in want]
    for mode in (L.NRG_SEEK_GE, L.NRG_SEEK_GT, L.NRG_SEEK_LE, L.NRG_SEEK_LT):
        ok, ov, fo = dev.sl_seek(q, mode)
        want = [model.seek(x, mode) for x in ql]
        assert fo.tolist() == [int(w is not None) for w in want], mode
        assert ok.tolist() == [w[0] if w else 0 for w in want] and ov.tolist() == [w[1] if w else 0 for w in want], mode
        sk, sv, cnt = dev.sl_scan(q[::4], mode, 6)
        for x, kr, vr, c in zip(ql[::4], sk, sv, cnt):
            assert list(zip(kr[:c].tolist(), vr[:c].tolist())) == model.scan(x, mode, 6), (mode, x)
    assert dev.sl_range_count(q[:-1], q[1:]).tolist() == [model.range_count(a, b) for a, b in zip(ql[:-1], ql[1:])]


def _check_launches(dev, model, delivered):
    assert dev.kernel_time("sl_pop_find")[0] == model.finds
    assert dev.kernel_time("sl_pop_plan")[0] == len(model.steps)
    assert dev.kernel_time("sl_pop_shift")[0] == model.shifts
    assert dev.kernel_time("sl_pop_take")[0] == (sum(1 for s in model.steps if s["f"] + s["b"]) if delivered else 0)
    assert dev.kernel_time("sl_compact")[0] == model.compactions


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", P.NAMES)
def test_streams_through_every_replay_path(nrg, name, path):
    s = P.by_name(name)
    dev, model = _open(nrg, s, max_batch=P.CHUNKED_MAX_BATCH if path == "chunked" else None)
    dev.kernel_timing(True)
    for i, recs in enumerate(s.chunks):
        _replay(dev, model, recs, path)
        _state(nrg, dev, model)
    _reads(nrg, dev, model)
    _check_launches(dev, model, path == "fused_round")
    img = dev.snapshot()
    dst, _ = _open(nrg, s, enable=False)
    dst.restore(img)
    assert dst.digest() == dev.digest() == model.digest() and dst.sl_pops() is None  # an image does not carry the setting
    dst.close()
    dev.close()


def test_a_chunk_without_pop_records_on_an_enabled_context(nrg):
    """sl_pop_find once per chunk and no other sl_pop_* launch; the pipeline's launches as without pops"""
    s = P.by_name("front_base_back_delta")
    dev, model = _open(nrg, s)
    dev.kernel_timing(True)
    for recs in s.chunks[:2]:  # the setup: Pushes only
        _replay(dev, model, recs, "fused_round")
    assert dev.kernel_time("sl_pop_find")[0] == 2
    for name in POP_KERNELS[1:]:
        assert dev.kernel_time(name)[0] == 0, name
    for name in ("sl_stream", "sl_resolve", "sl_scan", "sl_scatter", "sl_merge"):
        assert dev.kernel_time(name)[0] == 2, name
    _state(nrg, dev, model)
    dev.close()


@pytest.mark.parametrize("name", ["one_4096", "many_ones", "exhaustion", "run_placement"])
def test_pop_cap_smaller_than_the_total(nrg, name):
    """the stored prefix, the exact total, and nothing written past pop_cap (the guards of _round_pops)"""
    s = P.by_name(name)
    dev, model = _open(nrg, s)
    for recs in s.chunks:
        model.clear_popped()
        want_r, want_s = model.replay(recs)
        total = len(model.popped)
        cap = total // 2
        resp, some, pk, pv, got = _round_pops(dev, recs, cap)
        assert got == total and len(pk) == min(cap, total)
        assert pk.tolist() == [k for k, _ in model.popped[:cap]] and pv.tolist() == [v for _, v in model.popped[:cap]]
        assert np.array_equal(resp, want_r) and np.array_equal(some, want_s)
    _state(nrg, dev, model)
    dev.close()


def test_counts_without_entries_through_the_plain_round(nrg):
    """nrg_skiplist_round_async on an enabled context replays pops and answers counts; sl_pop_take never runs"""
    import torch

    s = P.by_name("interleaved")
    dev, model = _open(nrg, s)
    dev.kernel_timing(True)
    for recs in s.chunks:
        n = len(recs)
        resp = torch.zeros(n, dtype=torch.int64, device="cuda")
        some = torch.zeros(n, dtype=torch.uint8, device="cuda")
        dev.sl_round_device(_cuda(recs), n, 1, resp, some)
        dev.sync()
        want_r, want_s = model.replay(recs)
        assert np.array_equal(resp.cpu().numpy().view(np.uint64), want_r) and np.array_equal(some.cpu().numpy(), want_s)
    _state(nrg, dev, model)
    _check_launches(dev, model, False)
    dev.close()


def test_a_context_without_pops_is_as_before(nrg):
    """{k, mark} is an ordinary Push, and a fixed sequence launches what the parent commit launches: measured
    there with this sequence (the chunks of "run_placement", 6 rounds): sl_stream, sl_resolve, sl_scan,
    sl_scatter and sl_merge 6 each, sl_compact 2, and no kernel named sl_pop_*, sl_rm_* or sl_drop_*.
    (Nothing of the pops API is used here: this passes without it, and that is its point.)"""
    import torch

    import skiplist_model as M

    s = P.by_name("run_placement")
    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_SKIPLIST, 0, knobs={"SL_DELTA_MAX": s.delta_max}, log2_slots=s.log2,
                            max_batch=s.max_batch, log_bytes=LOG_BYTES, max_reads=1 << 12)
    model = M.SkipListModel(s.delta_max, s.max_batch)
    dev.kernel_timing(True)
    for recs in s.chunks:
        n = len(recs)
        resp = torch.zeros(n, dtype=torch.int64, device="cuda")
        some = torch.zeros(n, dtype=torch.uint8, device="cuda")
        dev.sl_round_device(_cuda(recs), n, 1, resp, some)
        dev.sync()
        model.replay(recs)
        assert np.array_equal(resp.cpu().numpy().view(np.uint64), recs["key"]) and (some.cpu().numpy() == 1).all()
    k, v = dev.sl_dump()
    mk, mv = model.arrays()
    assert np.array_equal(k, mk) and np.array_equal(v, mv) and dev.digest() == model.digest()
    assert (v == P.FRONT).sum() >= 1 and (v == P.BACK).sum() >= 1  # the marks of the enabled contexts, stored as values
    assert dev.sl_get([2, 1])[0].tolist() == [P.FRONT, P.BACK]  # the last chunk's {2, FRONT} and {1, BACK}
    rounds = len(s.chunks)
    assert rounds == 6 and model.compactions == 2
    for name in ("sl_stream", "sl_resolve", "sl_scan", "sl_scatter", "sl_merge"):
        assert dev.kernel_time(name)[0] == rounds, name
    assert dev.kernel_time("sl_compact")[0] == model.compactions
    for name in POP_KERNELS + ("sl_rm_resp", "sl_rm_state", "sl_drop_base", "sl_drop_delta"):
        assert dev.kernel_time(name)[0] == 0, name
    dev.close()


def _view(nrg, h):
    d = nrg.DeviceReplica.__new__(nrg.DeviceReplica)
    d.kind, d.device, d._h, d._lib = nrg._lib.NRG_DS_SKIPLIST, 0, C.c_void_p(h), nrg._lib.load()
    return d


def _group(nrg, s, G):
    L = nrg._lib
    lib = L.load()
    cfg = L.default_config(L.NRG_DS_SKIPLIST)
    cfg.log2_slots, cfg.max_batch, cfg.log_bytes, cfg.max_reads = s.log2, s.max_batch, LOG_BYTES, 1 << 12
    L.check(lib.nrg_test_loopback_collectives(1))
    g = C.c_void_p()
    try:
        L.check(lib.nrg_group_open((C.c_int * G)(*([0] * G)), G, C.byref(cfg), C.byref(g)), "nrg_group_open")
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))
    members = [_view(nrg, lib.nrg_group_replica(g, i)) for i in range(G)]
    for m in members:
        L.check(lib.nrg_test_set_knob(m._h, L.KNOBS["SL_DELTA_MAX"], s.delta_max))
    return lib, g, members


@pytest.mark.parametrize("name", ["interleaved", "run_placement", "exhaustion"])
def test_replicated_group_of_two(nrg, name):
    """both members enabled; a chunk is split between the members' segments (the global log is W_0 || W_1), so
    pop records come from both members in one round. Counts as responses, identical digests."""
    import torch

    L = nrg._lib
    s = P.by_name(name)
    lib, g, members = _group(nrg, s, 2)
    model = s.model()
    keep = []
    try:
        for m in members:
            m.sl_enable_pops()
        for r, recs in enumerate(s.chunks):
            pop = np.flatnonzero(np.isin(recs["val"], (P.FRONT, P.BACK)))
            # inside the first pop run where there is one: both members then contribute pop records
            cut = int(pop[0]) + 1 if len(pop) >= 2 else (len(recs) * (1 + r % 3)) // 4
            want_r, want_s = model.replay(recs)
            rd = (L.Round * 2)()
            outs = []
            for i, part in enumerate((recs[:cut], recs[cut:])):
                n = len(part)
                d_ops = _cuda(part) if n else None
                resp = torch.zeros(max(n, 1), dtype=torch.int64, device="cuda")
                some = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
                rd[i].recs, rd[i].n, rd[i].resp, rd[i].some = (d_ops.data_ptr() if n else 0), n, resp.data_ptr(), some.data_ptr()
                keep.append((d_ops, resp, some))
                outs.append((resp, some, n))
            torch.cuda.synchronize()
            L.check(lib.nrg_group_round_async(g, rd, None), f"round {r}")
            L.check(lib.nrg_group_sync(g))
            got_r = np.concatenate([o[0].cpu().numpy().view(np.uint64)[:o[2]] for o in outs])
            got_s = np.concatenate([o[1].cpu().numpy()[:o[2]] for o in outs])
            assert np.array_equal(got_s, want_s) and np.array_equal(got_r, want_r), r
            same = C.c_int(-1)
            L.check(lib.nrg_group_verify(g, None, C.byref(same)))
            assert same.value == 1
        for m in members:
            _state(nrg, m, model)
        assert members[0].digest() == members[1].digest()
    finally:
        for m in members:
            m._h = None
        assert lib.nrg_group_close(g) == L.NRG_OK


def test_abi_rules(nrg):
    import torch

    L = nrg._lib
    lib = L.load()
    F, B, T = P.FRONT, P.BACK, P.TOMB
    s = P.by_name("exhaustion")
    dev, model = _open(nrg, s, enable=False)
    f, b, on = C.c_uint64(5), C.c_uint64(5), C.c_int(5)
    assert lib.nrg_skiplist_pops(dev._h, C.byref(f), C.byref(b), C.byref(on)) == L.NRG_OK
    assert (f.value, b.value, on.value) == (0, 0, 0) and dev.sl_pops() is None
    m = C.c_uint64(9)
    assert lib.nrg_skiplist_pop(dev._h, 0, 1, 1, None, None, C.byref(m)) == L.NRG_E_INVAL and m.value == 9
    with pytest.raises(nrg.NrgError) as e:
        dev.sl_pop_front()  # not before pops are enabled
    assert e.value.code == L.NRG_E_INVAL and dev.log_state()["tail"] == 0
    pn = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert lib.nrg_skiplist_round_pops_async(dev._h, None, 0, 1, None, None, None, None, 0, pn.data_ptr()) == L.NRG_E_INVAL
    dev.log_append(P.recs_of([1, 2], [2, F]), 1)  # {2, F} is a Push while pops are off
    assert lib.nrg_skiplist_enable_pops(dev._h, F, B) == L.NRG_E_NOT_SYNCED and dev.sl_pops() is None
    dev.log_exec()
    assert lib.nrg_skiplist_enable_pops(dev._h, F, F) == L.NRG_E_INVAL  # equal marks
    assert lib.nrg_skiplist_enable_pops(dev._h, F, B) == L.NRG_OK
    assert lib.nrg_skiplist_enable_pops(dev._h, F, B) == L.NRG_OK  # again, the same marks
    assert lib.nrg_skiplist_enable_pops(dev._h, B, F) == L.NRG_E_INVAL and lib.nrg_skiplist_enable_pops(dev._h, F, 0) == L.NRG_E_INVAL
    assert dev.sl_pops() == (F, B)
    for tomb in (F, B):  # pops first: a tombstone equal to a mark is refused, another one taken
        assert lib.nrg_skiplist_enable_removal(dev._h, tomb) == L.NRG_E_INVAL and dev.sl_removal() is None
    assert lib.nrg_skiplist_enable_removal(dev._h, T) == L.NRG_OK
    # the stored value that equals a mark stays a value, and comes out of a pop as one
    k, v = dev.sl_pop_back()
    assert (k.tolist(), v.tolist()) == ([2], [F]) and dev.sl_len() == 1
    assert lib.nrg_skiplist_round_pops_async(dev._h, None, 0, 1, None, None, None, None, 0, None) == L.NRG_E_INVAL
    assert lib.nrg_skiplist_round_pops_async(dev._h, None, 0, 1, None, None, None, None, 4, pn.data_ptr()) == L.NRG_E_INVAL
    comb = C.c_void_p()
    assert lib.nrg_combiner_open(dev._h, 4, C.byref(comb)) == L.NRG_E_INVAL
    dev.close()
    dev, _ = _open(nrg, s, enable=False)  # removal first: marks equal to the tombstone are refused
    dev.sl_enable_removal(T)
    assert lib.nrg_skiplist_enable_pops(dev._h, T, B) == L.NRG_E_INVAL and lib.nrg_skiplist_enable_pops(dev._h, F, T) == L.NRG_E_INVAL
    assert dev.sl_pops() is None and lib.nrg_skiplist_enable_pops(dev._h, F, B) == L.NRG_OK
    dev.close()
    # another kind
    st = nrg.DeviceReplica(L.NRG_DS_STACK, 0, stack_capacity=1 << 10, max_batch=1024, log_bytes=LOG_BYTES)
    assert lib.nrg_skiplist_enable_pops(st._h, F, B) == L.NRG_E_INVAL
    assert lib.nrg_skiplist_pops(st._h, C.byref(f), C.byref(b), C.byref(on)) == L.NRG_E_INVAL
    assert lib.nrg_skiplist_pop(st._h, 0, 1, 1, None, None, C.byref(m)) == L.NRG_E_INVAL
    st.close()


def test_partitioned_round_with_an_enabled_member(nrg):
    """refused in the local check: NRG_E_INVAL, nothing written, no log movement"""
    import torch

    L = nrg._lib
    s = P.by_name("exhaustion")
    lib, g, members = _group(nrg, s, 1)
    try:
        m = members[0]
        recs = P.recs_of([1, 2, 3], [4, 5, P.FRONT])
        d_ops = _cuda(recs)
        resp = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        some = torch.full((3,), 7, dtype=torch.uint8, device="cuda")
        rd = (L.Round * 1)()
        rd[0].recs, rd[0].n, rd[0].resp, rd[0].some = d_ops.data_ptr(), 3, resp.data_ptr(), some.data_ptr()
        torch.cuda.synchronize()
        L.check(lib.nrg_group_partitioned_round(g, rd), "before pops")
        L.check(lib.nrg_group_sync(g))
        assert some.cpu().tolist() == [1, 1, 1] and m.sl_len() == 3  # (the mark was a value)
        m.sl_enable_pops()
        before = m.log_state()
        resp.fill_(-1)
        some.fill_(7)
        torch.cuda.synchronize()
        assert lib.nrg_group_partitioned_round(g, rd) == L.NRG_E_INVAL
        # (the pipelined form reports a round's argument errors where the round completes)
        rcs = (lib.nrg_group_partitioned_round_async(g, rd), lib.nrg_group_partitioned_flush(g))
        assert rcs in ((L.NRG_E_INVAL, L.NRG_OK), (L.NRG_OK, L.NRG_E_INVAL)), rcs
        L.check(lib.nrg_group_sync(g))
        assert m.log_state() == before and m.sl_len() == 3
        assert (resp.cpu().numpy() == -1).all() and (some.cpu().numpy() == 7).all()
    finally:
        for m in members:
            m._h = None
        assert lib.nrg_group_close(g) == L.NRG_OK


def test_python_api(nrg):
    """DeviceReplica.sl_pop_front / sl_pop_back, and SlPopFront / SlPopBack through two replicas of one log"""
    s = P.by_name("interleaved")
    dev, model = _open(nrg, s)
    for recs in s.chunks[:2]:
        _replay(dev, model, recs, "append_exec")
    for back, n in ((0, 1), (1, 1), (0, 7), (1, 300), (0, 0), (1, 1 << 63), (0, 1)):
        model.clear_popped()
        model.replay(P.pops(("b" if back else "f", n)))
        k, v = dev.sl_pop_back(n) if back else dev.sl_pop_front(n)
        assert k.tolist() == [x for x, _ in model.popped] and v.tolist() == [y for _, y in model.popped], (back, n)
    assert dev.sl_len() == len(model) == 0
    dev.close()

    log = nrg.Log(LOG_BYTES)
    a = nrg.Replica(log, nrg.SkipList, 0, log2_slots=12, max_batch=1024)
    b = nrg.Replica(log, nrg.SkipList, 0, log2_slots=12, max_batch=1024)
    ta, tb = a.register(), b.register()
    with pytest.raises(nrg.NrgError):
        a.execute_mut(nrg.SlPopFront(), ta)  # not before the replica enabled pops
    for r in (a, b):
        r.dev.sl_enable_pops()
    model = P.SkipListPopModel()
    rng = np.random.default_rng(16)
    for i in range(80):
        rep, tok = (a, ta) if i % 2 else (b, tb)
        x = rng.random()
        if x < 0.4:
            n = int(rng.integers(0, 4))
            op, mark = (nrg.SlPopFront(n), P.FRONT) if x < 0.2 else (nrg.SlPopBack(n), P.BACK)
            resp, some = model.replay([(n, mark)])
            assert rep.execute_mut(op, tok) == (int(resp[0]) if some[0] else None), i
        else:
            k, v = int(rng.integers(0, 25)) * 10, int(rng.integers(0, 1 << 62))
            assert rep.execute_mut(nrg.SlPush(k, v), tok) == k
            model.replay([(k, v)])
    assert a.execute_mut(nrg.SlPopFront(3), ta) == int(model.replay([(3, P.FRONT)])[0][0])
    with pytest.raises(ValueError):
        a.execute_mut(nrg.SlPopBack(1, mark=5), ta)
    seen = []
    a.verify(seen.append)
    b.verify(seen.append)
    assert seen[0] == seen[1] == model.items() and a.digest() == b.digest() == model.digest()
    c = nrg.Replica(log, nrg.SkipList, 0, log2_slots=10, max_batch=1024, clone_from=a)
    assert c.dev.sl_pops() == (P.FRONT, P.BACK)  # the clone takes the peer's setting
    c.verify(seen.append)
    assert seen[2] == model.items()
    for r in (a, b, c):
        r.dev.close()
