"""What the GPU tests of removal and pops in a partitioned skip-list group share
(tests/test_gpu_skiplist_group_remove.py, tests/test_gpu_skiplist_group_pop.py): groups opened over the
loopback collectives as tests/test_gpu_skiplist_scan_group.py opens them, device buffers with guard words
on both sides of every output, one partitioned round, one group pop, and the comparison of the members
with tests/skiplist_group_pop_model.py's UnionModel."""
import ctypes as C

import numpy as np

import skiplist_group_pop_model as GM
import skiplist_scan_model as SM

U64_MAX = GM.U64_MAX
LOG_BYTES = 64 * (1 << 16)
LOG2_SLOTS, MAX_BATCH, MAX_READS, DELTA_MAX = 12, 2048, 2048, 64
CANARY, CANARY8, PAD = 0xA5A5A5A5A5A5A5A5, 0x5A, 8
CASES = [(1, False), (1, True), (3, False), (8, False)]


def cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


class Guarded:
    """n words (or bytes) on the device with PAD guard words (bytes) before and after, canaries all over"""

    def __init__(self, n, byte=False):
        import torch

        self.n, self.byte = n, byte
        fill = np.full(n + 2 * PAD, CANARY8, np.uint8) if byte else np.full(n + 2 * PAD, CANARY, np.uint64).view(np.int64)
        self.t = torch.from_numpy(fill).cuda()
        self.ptr = self.t.data_ptr() + PAD * (1 if byte else 8)

    def host(self):
        a = self.t.cpu().numpy()
        return a if self.byte else a.view(np.uint64)

    def inner(self):
        return self.host()[PAD:PAD + self.n]

    def guards_intact(self):
        a, c = self.host(), (CANARY8 if self.byte else CANARY)
        return bool(np.all(a[:PAD] == c) and np.all(a[PAD + self.n:] == c))

    def untouched(self):
        return bool(np.all(self.host() == (CANARY8 if self.byte else CANARY)))


def cfg(L, kind=None):
    c = L.default_config(L.NRG_DS_SKIPLIST if kind is None else kind)
    c.log2_slots, c.max_batch, c.max_reads = LOG2_SLOTS, MAX_BATCH, MAX_READS
    c.log_bytes = LOG_BYTES
    return c


def open_group(L, lib, G, config=None, exp=False):
    config = config or cfg(L)
    L.check(lib.nrg_test_loopback_collectives(1))
    g = C.c_void_p()
    try:
        L.check(lib.nrg_group_open((C.c_int * G)(*([0] * G)), G, C.byref(config), C.byref(g)), "nrg_group_open")
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))
    ctxs = [lib.nrg_group_replica(g, i) for i in range(G)]
    for c in ctxs:
        if config.ds_kind == L.NRG_DS_SKIPLIST:
            L.check(lib.nrg_test_set_knob(c, L.KNOBS["SL_DELTA_MAX"], DELTA_MAX))
        if exp:
            L.check(lib.nrg_test_set_knob(c, L.KNOBS["EXP"], 0x10000))
    return g, ctxs


def dump(L, lib, ctx):
    n = C.c_uint64()
    rc = lib.nrg_skiplist_dump(ctx, None, None, 0, C.byref(n))
    assert rc in (L.NRG_OK, L.NRG_E_CAPACITY)
    k, v = np.zeros(max(n.value, 1), np.uint64), np.zeros(max(n.value, 1), np.uint64)
    m = C.c_uint64()
    L.check(lib.nrg_skiplist_dump(ctx, k.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), n.value, C.byref(m)))
    return k[:m.value], v[:m.value]


def digest(L, lib, ctx):
    out = np.zeros(3, np.uint64)
    L.check(lib.nrg_digest(ctx, out.ctypes.data_as(C.c_void_p)))
    return tuple(int(x) for x in out)


def log_tails(L, lib, ctxs):
    out = []
    for c in ctxs:
        info = L.LogInfo()
        L.check(lib.nrg_log_state(c, C.byref(info)))
        out.append({f: getattr(info, f) for f, _ in L.LogInfo._fields_})
    return out


def check_members(L, lib, ctxs, model, msg=""):
    """the union of the members' dumps is the model, every member holds only keys it owns, in order, and
    the digests add up to the model's"""
    from nrgpu import digest as D

    G = len(ctxs)
    ks, vs = [], []
    for p, c in enumerate(ctxs):
        k, v = dump(L, lib, c)
        assert np.all(k[1:] > k[:-1]), f"{msg}: member {p} dump not strictly ascending"
        assert len(k) == 0 or np.all(SM.key_owner(k, G) == p), f"{msg}: member {p} holds a key it does not own"
        ks.append(k)
        vs.append(v)
    k, v = np.concatenate(ks), np.concatenate(vs)
    order = np.argsort(k, kind="stable")
    items = model.items()
    mk = np.array([a for a, _ in items], np.uint64)
    mv = np.array([b for _, b in items], np.uint64)
    np.testing.assert_array_equal(k[order], mk, err_msg=msg + " keys of the union")
    np.testing.assert_array_equal(v[order], mv, err_msg=msg + " values of the union")
    assert D.combine([digest(L, lib, c) for c in ctxs]) == D.skiplist(mk, mv), msg + " digest"


def prefill(L, lib, ctxs, n, off=GM.OFF):
    for p, c in enumerate(ctxs):
        L.check(lib.nrg_skiplist_prefill_partition(c, n, off, p, len(ctxs)))


class RoundBufs:
    """one member's part of a partitioned round: recs (n, 2) u64 or None, Get keys, guarded outputs"""

    def __init__(self, L, rd, i, recs, gets, want):
        W = 0 if recs is None else len(recs)
        R = 0 if gets is None else len(gets)
        self.W, self.R, self.want = W, R, want
        self.p = cuda(np.ascontiguousarray(recs, np.uint64)) if W else None
        self.gk = cuda(np.asarray(gets, np.uint64)) if R else None
        self.gv, self.gf = Guarded(R), Guarded(R, byte=True)
        self.resp, self.some = Guarded(W), Guarded(W, byte=True)
        rd[i].recs, rd[i].n = (self.p.data_ptr() if W else 0), W
        rd[i].resp, rd[i].some = (self.resp.ptr, self.some.ptr) if want else (0, 0)
        rd[i].get_keys, rd[i].n_gets = (self.gk.data_ptr() if R else 0), R
        rd[i].get_vals, rd[i].get_found = self.gv.ptr, self.gf.ptr

    def all_untouched(self):
        return self.gv.untouched() and self.gf.untouched() and self.resp.untouched() and self.some.untouched()


def post_round(L, lib, g, parts, pipelined=False):
    """parts[i] = (recs, gets, want); returns (rc, the round struct, [RoundBufs]): keep both alive until synced"""
    import torch

    G = len(parts)
    rd = (L.Round * G)()
    keep = [RoundBufs(L, rd, i, *parts[i]) for i in range(G)]
    torch.cuda.synchronize()
    rc = (lib.nrg_group_partitioned_round_async if pipelined else lib.nrg_group_partitioned_round)(g, rd)
    return rc, rd, keep


def check_round(keep, parts, model, msg):
    """after the sync: the model replays the round's records in rank order, then answers its Gets"""
    want = [model.replay(recs if recs is not None else []) for recs, _, _ in parts]
    for i, ((recs, gets, asked), b) in enumerate(zip(parts, keep)):
        m = f"{msg} member {i}"
        if asked and b.W:
            np.testing.assert_array_equal(b.resp.inner(), want[i][0], err_msg=m + " responses")
            np.testing.assert_array_equal(b.some.inner(), want[i][1], err_msg=m + " some")
        else:
            assert b.resp.untouched() and b.some.untouched(), m + ": responses written where none were asked"
        if b.R:
            gv, gf = model.get(gets)
            np.testing.assert_array_equal(b.gf.inner(), gf, err_msg=m + " found")
            np.testing.assert_array_equal(b.gv.inner(), gv, err_msg=m + " gets")
        for buf in (b.resp, b.some, b.gv, b.gf):
            assert buf.guards_intact(), m + ": a guard word was written"


def push_round(L, lib, g, G, k, v, member=0):
    parts = [(np.stack([k, v], 1) if i == member else None, None, False) for i in range(G)]
    rc, rd, keep = post_round(L, lib, g, parts)
    L.check(rc, "push round")
    L.check(lib.nrg_group_sync(g))


class PopBufs:
    def __init__(self, L, q, i, reqs, cap, extra=PAD):
        n = len(reqs)
        self.n, self.cap = n, cap
        self.arr = (L.PopReq * max(n, 1))(*[L.PopReq(int(c), int(b), 0) for c, b in reqs])
        self.resp, self.some = Guarded(n), Guarded(n, byte=True)
        self.keys, self.vals, self.total = Guarded(cap), Guarded(cap), Guarded(1)
        q[i].reqs, q[i].n = self.arr, n
        q[i].resp, q[i].some = self.resp.ptr, self.some.ptr
        q[i].pop_keys, q[i].pop_vals, q[i].pop_cap, q[i].pop_n = self.keys.ptr, self.vals.ptr, cap, self.total.ptr

    def all_untouched(self):
        return all(b.untouched() for b in (self.resp, self.some, self.keys, self.vals, self.total))


def group_pop(L, lib, g, reqs, caps):
    """one nrg_group_skiplist_pop; (rc, [PopBufs])"""
    import torch

    G = len(reqs)
    q = (L.Pops * G)()
    keep = [PopBufs(L, q, i, reqs[i], caps[i]) for i in range(G)]
    torch.cuda.synchronize()
    rc = lib.nrg_group_skiplist_pop(g, q)
    return rc, keep


def check_pop(keep, reqs, model, msg):
    """every rank's resp, some, packed entries and *pop_n against the model's run; canaries past every count
    and past pop_cap. Returns the model's answer."""
    want = model.pop_run(reqs)
    for i, (b, (cnt, ks, vs)) in enumerate(zip(keep, want)):
        m = f"{msg} member {i}"
        np.testing.assert_array_equal(b.resp.inner(), cnt, err_msg=m + " resp")
        np.testing.assert_array_equal(b.some.inner(), (cnt >= 1).astype(np.uint8), err_msg=m + " some")
        total = int(cnt.sum())
        if b.n:
            assert int(b.total.inner()[0]) == total, m + " *pop_n"
        else:
            assert b.total.untouched() or int(b.total.inner()[0]) == 0, m + " *pop_n of a member without requests"
        stored = min(total, b.cap)
        np.testing.assert_array_equal(b.keys.inner()[:stored], ks[:stored], err_msg=m + " popped keys")
        np.testing.assert_array_equal(b.vals.inner()[:stored], vs[:stored], err_msg=m + " popped values")
        assert np.all(b.keys.inner()[stored:] == CANARY) and np.all(b.vals.inner()[stored:] == CANARY), m + ": past the count"
        for buf in (b.resp, b.some, b.keys, b.vals, b.total):
            assert buf.guards_intact(), m + ": a guard word was written"
    return want
