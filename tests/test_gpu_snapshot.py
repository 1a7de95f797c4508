"""Snapshot and restore on the GPU, every kind: a replica restored from another's snapshot into a
different geometry is indistinguishable from one that replayed the log (dumps, digests, log
positions, and the responses and final state of further rounds); what nrg_restore refuses leaves
the replica as it was; a corrupted payload fails the digest check; nrg_snapshot_async never stores
past cap; a host model seeds a replica; a late replica joins a garbage-collected log through
clone_from; nrg_group_resync brings a diverged group back."""
import ctypes as C
from collections import deque

import numpy as np
import pytest

from nrgpu import digest, snapshot
from test_gpu_group_verify import _HashMapKind, _StackKind, _VSpaceKind, _cuda, _open_group, _run_ranks, _verify

pytestmark = pytest.mark.gpu

MIN_LOG_BYTES = 2 * 32 * 256 * 64
SIDE = 0xFFFFFFFFFFFFFFFF


def _rounds(dev, batches):
    """append + exec each batch through the log; [(responses, some)] of every batch"""
    out = []
    for recs in batches:
        first = dev.log_append(recs, 1)
        out.append(dev.log_exec(first, first + len(recs)))
    return out


def _same_responses(a, b):
    assert len(a) == len(b)
    for (ra, sa), (rb, sb) in zip(a, b):
        np.testing.assert_array_equal(sa, sb)
        np.testing.assert_array_equal(ra, rb)


# ---- per kind: configs of the source A and the destination B, the log A replays, further rounds,
# ---- and the observable state ----------------------------------------------------------------
class _Hm:
    def __init__(self, nrg, nkeys, b_cfg):
        self.kind = nrg._lib.NRG_DS_HASHMAP
        self.a_cfg = dict(log2_slots=12, max_batch=1 << 12, log_bytes=MIN_LOG_BYTES)
        self.b_cfg = dict(max_batch=1 << 11, log_bytes=2 * MIN_LOG_BYTES, **b_cfg)
        rng = np.random.default_rng(nkeys)
        keys = rng.choice(1 << 20, nkeys, replace=False).astype(np.uint64)
        if nkeys > 1:
            keys[3] = SIDE
        first = np.zeros(nkeys, nrg.PUT_DTYPE)
        first["key"], first["val"] = keys, rng.integers(0, 2**63, nkeys, dtype=np.uint64)
        again = first[: nkeys // 2].copy()  # overwritten in a second round: values of a replay round
        again["val"] += np.uint64(1)
        self.log = [b for b in (first[: nkeys // 3], first[nkeys // 3:], again) if len(b)]
        self.more = []
        for r in range(3):  # known keys (the side key among them) and new ones, some twice in a round
            m = np.zeros(600, nrg.PUT_DTYPE)
            known = rng.choice(keys, 600) if nkeys else rng.integers(0, 50, 600, dtype=np.uint64)
            m["key"] = np.where(rng.random(600) < 0.5, known, rng.integers(0, 1 << 20, 600, dtype=np.uint64))
            m["key"][5] = SIDE
            m["val"] = rng.integers(0, 2**63, 600, dtype=np.uint64)
            self.more.append(m)

    def state(self, d):
        k, v = d.hm_dump()
        return [k.tolist(), v.tolist(), d.hm_size()]

    def unpacked(self, st):
        o = np.argsort(st[0], kind="stable")
        return [st[0][o].tolist(), st[1][o].tolist(), len(st[0])]


class _St:
    def __init__(self, nrg, n, b_cfg=None):
        self.kind = nrg._lib.NRG_DS_STACK
        self.a_cfg = dict(stack_capacity=1 << 17, max_batch=1 << 16, log_bytes=1 << 23)
        self.b_cfg = dict(stack_capacity=1 << 16, max_batch=1 << 13, log_bytes=1 << 23)
        rng = np.random.default_rng(n + 1)
        push = np.zeros(n, nrg.STACK_OP_DTYPE)
        push["val"], push["op"] = rng.integers(0, 2**32, n, dtype=np.uint32), 1
        self.log = [push] if n else []
        self.more = []
        for r in range(2):
            m = np.zeros(5000, nrg.STACK_OP_DTYPE)
            m["val"], m["op"] = rng.integers(0, 2**32, 5000, dtype=np.uint32), rng.integers(0, 2, 5000)
            self.more.append(m)

    def state(self, d):
        return [d.st_dump().tolist(), d.st_len()]

    def unpacked(self, st):
        return [st.tolist(), len(st)]


class _Qu:
    """capacity 2^10 and max_batch 2^8 make a ring of 2^11: 2560 Pops take the front past the
    ring's end once, to ring position 512"""

    def __init__(self, nrg):
        self.kind = nrg._lib.NRG_DS_QUEUE
        self.a_cfg = dict(queue_capacity=1 << 10, max_batch=1 << 8, log_bytes=MIN_LOG_BYTES)
        self.b_cfg = dict(queue_capacity=1 << 12, max_batch=1 << 9, log_bytes=MIN_LOG_BYTES)
        rng = np.random.default_rng(5)
        self.model = deque()

        def batch(ops):
            m = np.zeros(len(ops), nrg.QUEUE_OP_DTYPE)
            m["op"], m["val"] = ops, rng.integers(0, 2**63, len(ops), dtype=np.uint64)
            for v, o in zip(m["val"].tolist(), m["op"].tolist()):
                if o:
                    self.model.append(v)
                elif self.model:
                    self.model.popleft()
            return m

        self.log = [batch([1] * 200)] + [batch([1, 0] * 128) for _ in range(20)]
        self.front_first = list(self.model)
        self.more = [batch((rng.random(256) < 0.55).astype(np.uint64)) for _ in range(3)]

    def state(self, d):
        return [d.qu_dump().tolist(), d.qu_len()]

    def unpacked(self, st):
        return [st.tolist(), len(st)]


class _Sy:
    def __init__(self, nrg):
        self.kind = nrg._lib.NRG_DS_SYNTHETIC
        self.a_cfg = dict(synth_n=1000, max_batch=1 << 10, log_bytes=MIN_LOG_BYTES)
        self.b_cfg = dict(synth_n=1000, max_batch=1 << 9, log_bytes=2 * MIN_LOG_BYTES)
        rng = np.random.default_rng(9)

        def batch(n):
            m = np.zeros(n, nrg.SYNTH_OP_DTYPE)
            m["tid"], m["op"] = rng.integers(0, 8, n), rng.integers(0, 2, n)
            m["r1"], m["r2"] = rng.integers(0, 2**63, n, dtype=np.uint64), rng.integers(0, 2**63, n, dtype=np.uint64)
            return m

        self.log = [batch(700), batch(300)]
        self.more = [batch(500), batch(200)]

    def state(self, d):
        return [d.sy_dump().tolist()]

    def unpacked(self, st):
        return [st.tolist()]


class _Vs:
    def __init__(self, nrg, orc):
        gen = _VSpaceKind(nrg, orc)
        self.kind = gen.kind
        self.a_cfg = dict(gen.cfg)
        self.b_cfg = dict(max_batch=64, log2_slots=10, log_bytes=2 * MIN_LOG_BYTES)
        self.log = [gen.segment(50, s) for s in range(4)]
        self.more = [gen.segment(50, 40 + s) for s in range(2)]
        self.other = gen.segment(30, 99)  # what B holds before the restore

    def state(self, d):
        lv = d.vs_dump()
        return [lv["vaddr"].tolist(), lv["entry"].tolist(), d.vs_tables()]

    def unpacked(self, tables):
        lv = snapshot.leaves(tables)
        return [lv["vaddr"].tolist(), lv["entry"].tolist(), len(tables)]


def _case(nrg, orc, name):
    if name == "hm-fixed":
        return _Hm(nrg, 1500, dict(log2_slots=16))
    if name == "hm-grow":
        return _Hm(nrg, 1500, dict(log2_slots=8, hashmap_max_log2_slots=16))
    if name == "hm-empty":
        return _Hm(nrg, 0, dict(log2_slots=16))
    if name == "hm-one":
        return _Hm(nrg, 1, dict(log2_slots=16))
    if name.startswith("st-"):
        return _St(nrg, int(name[3:]))
    return {"queue": lambda: _Qu(nrg), "synthetic": lambda: _Sy(nrg), "vspace": lambda: _Vs(nrg, orc)}[name]()


CASES = ["hm-fixed", "hm-grow", "hm-empty", "hm-one", "st-0", "st-1", "st-50001", "queue", "synthetic", "vspace"]


@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("name", CASES)
def test_restored_replica_is_a_replayed_one(nrg, orc, name, pipeline):
    L = nrg._lib
    k = _case(nrg, orc, name)
    a = nrg.DeviceReplica(k.kind, 0, pipeline=pipeline, **k.a_cfg)
    b = nrg.DeviceReplica(k.kind, 0, pipeline=pipeline, **k.b_cfg)
    try:
        _rounds(a, k.log)
        a.sync()
        if name == "queue":
            assert a.qu_dump().tolist() == k.front_first
        if name == "vspace":  # B holds another table first, and a digest's tags of it
            _rounds(b, [k.other])
            stale = b.digest()
        want = a.snapshot_info()
        img = a.snapshot()
        info, st = snapshot.unpack(img)
        a_state, a_log, a_dg = k.state(a), a.log_state(), a.digest()
        print(name, pipeline, info)
        assert info == want._replace(digest=a_dg) and info.ds_kind == k.kind and info.bytes == img.size
        assert info.log_idx == a_log["ltail"] == sum(len(x) for x in k.log)
        assert k.unpacked(st) == a_state  # the image itself is the state
        if name == "hm-fixed":
            assert info.items == 1500 and SIDE in st[0].tolist()
        if pipeline:  # straight from the device buffer
            p, nbytes, dinfo = a.snapshot_device()
            assert dinfo == info
            b.restore(p, nbytes)
        else:
            b.restore(img)
        assert k.state(b) == a_state
        assert b.digest() == a_dg == info.digest
        if name == "vspace":
            assert stale != a_dg
        if name == "hm-grow":
            assert b.hm_log2_slots() == 12  # sized for 1500 keys at one key per two slots
        lb = b.log_state()
        assert lb["head"] == lb["tail"] == lb["ctail"] == lb["ltail"] == a_log["ltail"]
        probe = k.more[0][:0]
        assert b.log_append(probe, 1) == a_log["ltail"]
        # the same further rounds: bit-equal responses and final state
        ra, rb = _rounds(a, k.more), _rounds(b, k.more)
        _same_responses(ra, rb)
        assert any(s.any() for _, s in ra) or name == "st-0"
        assert k.state(b) == k.state(a)
        assert b.digest() == a.digest()
        assert b.log_state()["tail"] == a.log_state()["tail"]
        if name == "vspace":
            lv = a.vs_dump()
            rng = np.random.default_rng(3)
            va = np.concatenate([lv["vaddr"][::7] + rng.integers(0, 4096, len(lv["vaddr"][::7])).astype(np.uint64),
                                 rng.integers(0, 1 << 47, 200).astype(np.uint64)])
            pa, fa = a.vs_resolve(va)
            pb, fb = b.vs_resolve(va)
            assert fa.any() and not fa.all()
            np.testing.assert_array_equal(fa, fb)
            np.testing.assert_array_equal(pa, pb)
    finally:
        a.close()
        b.close()


# ---- refusals ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vspace_image(nrg, orc):
    k = _Vs(nrg, orc)
    a = nrg.DeviceReplica(k.kind, 0, **k.a_cfg)
    _rounds(a, k.log)
    img = a.snapshot()
    a.close()
    return img


def _refusal_cases(nrg, L):
    st_img = snapshot.pack(L.NRG_DS_STACK, np.arange(3000, dtype=np.uint32), 3000)
    bad_magic = st_img.copy()
    bad_magic[2] ^= 1
    keys = np.arange(1500, dtype=np.uint64) * np.uint64(977)
    return {
        "wrong-kind": (L.NRG_DS_QUEUE, dict(queue_capacity=1 << 12, max_batch=256), st_img, L.NRG_E_INVAL),
        "truncated": (L.NRG_DS_STACK, dict(stack_capacity=1 << 12), st_img[:-64], L.NRG_E_INVAL),
        "magic": (L.NRG_DS_STACK, dict(stack_capacity=1 << 12), bad_magic, L.NRG_E_INVAL),
        "stack-capacity": (L.NRG_DS_STACK, dict(stack_capacity=2999), st_img, L.NRG_E_CAPACITY),
        "queue-capacity": (L.NRG_DS_QUEUE, dict(queue_capacity=1 << 10, max_batch=256),
                           snapshot.pack(L.NRG_DS_QUEUE, np.arange(1025, dtype=np.uint64), 7), L.NRG_E_CAPACITY),
        "vspace-capacity": (L.NRG_DS_VSPACE, dict(log2_slots=2, max_batch=64), None, L.NRG_E_CAPACITY),
        "synth-n": (L.NRG_DS_SYNTHETIC, dict(synth_n=1000, max_batch=256),
                    snapshot.pack(L.NRG_DS_SYNTHETIC, np.arange(999, dtype=np.uint64), 1), L.NRG_E_INVAL),
        "table-full": (L.NRG_DS_HASHMAP, dict(log2_slots=10, max_batch=256),
                       snapshot.pack(L.NRG_DS_HASHMAP, (keys, keys), 1500), L.NRG_E_TABLE_FULL),
        "grow-limit": (L.NRG_DS_HASHMAP, dict(log2_slots=8, hashmap_max_log2_slots=11, max_batch=256),
                       snapshot.pack(L.NRG_DS_HASHMAP, (keys, keys), 1500), L.NRG_E_TABLE_FULL),
    }


def _own_content(nrg, L, kind):
    """a small log for B, so that 'unchanged' is about something"""
    if kind == L.NRG_DS_HASHMAP:
        r = np.zeros(40, nrg.PUT_DTYPE)
        r["key"], r["val"] = np.arange(40), np.arange(40) + 5
    elif kind == L.NRG_DS_STACK:
        r = np.zeros(40, nrg.STACK_OP_DTYPE)
        r["val"], r["op"] = np.arange(40), 1
    elif kind == L.NRG_DS_QUEUE:
        r = np.zeros(40, nrg.QUEUE_OP_DTYPE)
        r["val"], r["op"] = np.arange(40), 1
    elif kind == L.NRG_DS_SYNTHETIC:
        r = np.zeros(40, nrg.SYNTH_OP_DTYPE)
        r["tid"], r["r1"], r["r2"] = 1, np.arange(40), np.arange(40) * 3
    else:
        r = np.zeros(1, nrg.VSPACE_OP_DTYPE)
        r[0] = (1 << 30, 1 << 21, 8192, 0, 3)
    return r


_DUMPS = {1: lambda d: [x.tolist() for x in d.hm_dump()], 2: lambda d: d.st_dump().tolist(),
          3: lambda d: d.sy_dump().tolist(), 4: lambda d: d.qu_dump().tolist(), 5: lambda d: d.vs_dump().tolist()}


@pytest.mark.parametrize("name", ["wrong-kind", "truncated", "magic", "stack-capacity", "queue-capacity",
                                  "vspace-capacity", "synth-n", "table-full", "grow-limit"])
def test_refused_restore_leaves_the_replica_untouched(nrg, vspace_image, name):
    L = nrg._lib
    kind, cfg, img, code = _refusal_cases(nrg, L)[name]
    if img is None:
        img = vspace_image
        assert snapshot.header(img).items > 4
    b = nrg.DeviceReplica(kind, 0, log_bytes=MIN_LOG_BYTES, **cfg)
    try:
        _rounds(b, [_own_content(nrg, L, kind)])
        before = (_DUMPS[kind](b), b.log_state(), b.digest())
        with pytest.raises(nrg.NrgError) as e:
            b.restore(img)
        assert e.value.code == code
        assert (_DUMPS[kind](b), b.log_state(), b.digest()) == before
        b.sync()  # nothing latched
    finally:
        b.close()


def test_restore_null_arguments(nrg):
    L = nrg._lib
    b = nrg.DeviceReplica(L.NRG_DS_STACK, 0, stack_capacity=1 << 10, log_bytes=MIN_LOG_BYTES)
    lib = L.load()
    info = L.SnapshotInfo()
    assert lib.nrg_snapshot_size(b.handle, None) == L.NRG_E_INVAL
    assert lib.nrg_snapshot_async(b.handle, None, 4096) == L.NRG_E_INVAL
    assert lib.nrg_snapshot_info_read(b.handle, None, 4096, C.byref(info)) == L.NRG_E_INVAL
    assert lib.nrg_restore(b.handle, None, 4096) == L.NRG_E_INVAL
    b.close()


@pytest.mark.parametrize("name", ["hashmap", "stack"])
def test_corrupted_payload_fails_the_digest_check(nrg, name):
    L = nrg._lib
    if name == "hashmap":
        keys = np.arange(1500, dtype=np.uint64) * np.uint64(977)
        kind, cfg, img = L.NRG_DS_HASHMAP, dict(log2_slots=12), snapshot.pack(L.NRG_DS_HASHMAP, (keys, keys + 1), 10)
    else:
        kind, cfg = L.NRG_DS_STACK, dict(stack_capacity=1 << 12)
        img = snapshot.pack(kind, np.arange(3000, dtype=np.uint32), 10)
    bad = img.copy()
    bad[64 + 8 * 101] ^= 0x10  # one payload word
    b = nrg.DeviceReplica(kind, 0, log_bytes=MIN_LOG_BYTES, **cfg)
    try:
        with pytest.raises(nrg.NrgError) as e:
            b.restore(bad)
        assert e.value.code == L.NRG_E_INVAL
        b.restore(img)  # "restore again"
        assert b.digest() == snapshot.header(img).digest and b.log_state()["tail"] == 10
    finally:
        b.close()


@pytest.mark.parametrize("name", ["hashmap", "stack"])
def test_snapshot_async_never_stores_past_cap(nrg, name):
    import torch

    L = nrg._lib
    lib = L.load()
    if name == "hashmap":  # 16 tiles of 4096 slots: most fit, the last ones would pass cap
        a = nrg.DeviceReplica(L.NRG_DS_HASHMAP, 0, log2_slots=16, log_bytes=MIN_LOG_BYTES)
        a.hm_prefill_range(20000, 1)
    else:
        a = nrg.DeviceReplica(L.NRG_DS_STACK, 0, stack_capacity=1 << 12, log_bytes=MIN_LOG_BYTES)
        a.st_init(np.arange(3000, dtype=np.uint32))
    try:
        need = a.snapshot_info().bytes
        buf = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        cap = need - 64
        assert lib.nrg_snapshot_async(a.handle, buf.data_ptr(), cap) == L.NRG_OK
        assert lib.nrg_sync(a.handle) == L.NRG_E_CAPACITY
        assert lib.nrg_sync(a.handle) == L.NRG_OK  # latched once
        host = buf.cpu().numpy()
        assert (host[cap:] == 0xA5).all(), "stored past cap"
        assert not host[:8].any()  # magic = 0
        info = L.SnapshotInfo()
        assert lib.nrg_snapshot_info_read(a.handle, buf.data_ptr(), need, C.byref(info)) == L.NRG_E_INVAL
        # and with room: the image, nothing behind it
        buf.fill_(0xA5)
        torch.cuda.synchronize()
        assert lib.nrg_snapshot_async(a.handle, buf.data_ptr(), need) == L.NRG_OK
        assert lib.nrg_sync(a.handle) == L.NRG_OK
        host = buf.cpu().numpy()
        assert (host[need:] == 0xA5).all()
        assert snapshot.header(host[:need]).digest == a.digest()
        # a buffer too short for the header: nothing at all
        buf.fill_(0xA5)
        torch.cuda.synchronize()
        assert lib.nrg_snapshot_async(a.handle, buf.data_ptr(), 48) == L.NRG_OK
        assert lib.nrg_sync(a.handle) == L.NRG_E_CAPACITY
        assert (buf.cpu().numpy() == 0xA5).all()
    finally:
        a.close()


def test_host_model_seeds_a_replica(nrg, orc):
    L = nrg._lib
    om = orc.HashMap()
    keys = np.concatenate([orc.gen_uniform(4000, 1, 3000), np.array([SIDE], np.uint64)])
    om.replay(keys, orc.gen_raw(len(keys), 2), want_prev=False)
    mk, mv = om.dump_sorted()
    b = nrg.DeviceReplica(L.NRG_DS_HASHMAP, 0, log2_slots=13, log_bytes=MIN_LOG_BYTES)
    b.restore(snapshot.pack(L.NRG_DS_HASHMAP, (mk, mv), 4001))
    k, v = b.hm_dump()
    np.testing.assert_array_equal(k, mk)
    np.testing.assert_array_equal(v, mv)
    assert b.hm_size() == len(mk) and b.digest() == om.digest() and b.log_state()["ltail"] == 4001
    got, found = b.hm_get(np.array([SIDE, int(mk[0]), 1 << 50], np.uint64))
    assert found.tolist() == [1, 1, 0] and int(got[0]) == int(mv[-1])
    b.close()
    st = orc.Stack(np.arange(7, dtype=np.uint32))
    st.replay(*orc.gen_stack_ops(5001, 3))
    s = nrg.DeviceReplica(L.NRG_DS_STACK, 0, stack_capacity=1 << 14, log_bytes=MIN_LOG_BYTES)
    s.restore(snapshot.pack(L.NRG_DS_STACK, st.dump(), 5001).tobytes())
    np.testing.assert_array_equal(s.st_dump(), st.dump())
    assert s.digest() == digest.stack(st.dump())
    s.close()


def test_late_replica_after_gc_joins_through_clone_from(nrg):
    """test_late_replica_after_gc_is_refused's scenario with clone_from=a: registration succeeds,
    both replicas see a round executed through either, and their digests agree."""
    log = nrg.Log(2 * 64 * 8192)
    a = nrg.Replica(log, nrg.NrHashMap, 0, log2_slots=16, max_batch=4096, log_bytes=log.bytes)
    ta = a.register()
    for r in range(4):
        a.execute_mut_batch([nrg.Put(k, r) for k in range(3000)], ta)
    assert log.head > 0
    with pytest.raises(RuntimeError, match="garbage-collected"):  # still refused without it
        nrg.Replica(log, nrg.NrHashMap, 0, log2_slots=16, max_batch=4096)
    b = nrg.Replica(log, nrg.NrHashMap, 0, clone_from=a, log2_slots=14, max_batch=4096)
    assert b.idx == 2 and b.dev.log_state()["ltail"] == log.tail == a.dev.log_state()["ltail"]
    tb = b.register()
    assert b.execute(nrg.Get(2999), tb) == 3
    assert a.execute_mut(nrg.Put(7, 100), ta) == 3
    assert b.execute_mut(nrg.Put(7, 200), tb) == 100
    assert b.execute_mut(nrg.Put(1 << 40, 1), tb) is None
    assert a.execute(nrg.Get(7), ta) == 200 and a.execute(nrg.Get(1 << 40), ta) == 1
    assert b.execute(nrg.Get(7), tb) == 200
    assert a.digest() == b.digest()
    a.dev.close()
    b.dev.close()


# ---- nrg_group_resync --------------------------------------------------------------------------
def _diverge(nrg, lib, L, name, ctx):
    """one extra record into this replica alone, through a direct call"""
    import torch

    if name == "stack":
        op = np.zeros(1, nrg.STACK_OP_DTYPE)
        op["val"], op["op"] = 4242, L.NRG_STACK_PUSH
        d_op = _cuda(op)
        torch.cuda.synchronize()
        L.check(lib.nrg_stack_round_async(ctx, d_op.data_ptr(), 1, 2, None, None))
    else:
        op = np.zeros(1, nrg.PUT_DTYPE)
        op["key"], op["val"] = 1 << 45, 4242
        d_op = _cuda(op)
        torch.cuda.synchronize()
        L.check(lib.nrg_hashmap_round_async(ctx, d_op.data_ptr(), 1, 2, None, 0, None, None, None, None))
    L.check(lib.nrg_sync(ctx))
    return d_op


@pytest.mark.parametrize("name", ["hashmap", "stack"])
def test_group_resync_single_process(nrg, orc, name):
    import torch

    L = nrg._lib
    lib = L.load()
    G = 3
    k = {"hashmap": _HashMapKind, "stack": _StackKind}[name](nrg, orc)
    g = _open_group(nrg, k.kind, G, **k.cfg)
    keep = []

    def round_(r, lens):
        rd = (L.Round * G)()
        for i in range(G):
            recs = k.segment(lens[i], 100 * r + i)
            d = _cuda(recs) if lens[i] else None
            rd[i].recs, rd[i].n = (d.data_ptr() if d is not None else 0), lens[i]
            keep.append(d)
        torch.cuda.synchronize()
        L.check(lib.nrg_group_round_async(g, rd, None), f"round {r}")

    try:
        round_(0, [50, 23, 41])
        round_(1, [0, 37, 19])
        rc, same, _ = _verify(nrg, g, G)
        assert rc == L.NRG_OK and same == 1
        keep.append(_diverge(nrg, lib, L, name, lib.nrg_group_replica(g, 1)))
        rc, same, out = _verify(nrg, g, G)
        assert rc == L.NRG_OK and same == 0 and out[0].tolist() == out[2].tolist() != out[1].tolist()
        assert lib.nrg_group_resync(g, 3) == L.NRG_E_INVAL and lib.nrg_group_resync(g, -1) == L.NRG_E_INVAL
        assert lib.nrg_group_resync(g, 0) == L.NRG_OK
        rc, same, out = _verify(nrg, g, G)
        assert rc == L.NRG_OK and same == 1 and tuple(int(x) for x in out[1]) == tuple(k.triple())
        info = [L.LogInfo() for _ in range(G)]
        for i in range(G):
            L.check(lib.nrg_log_state(lib.nrg_group_replica(g, i), C.byref(info[i])))
        assert info[0].tail == info[1].tail == info[2].tail == info[1].ltail == info[1].head
        round_(2, [61, 5, 19])
        rc, same, out = _verify(nrg, g, G)
        assert rc == L.NRG_OK and same == 1
        assert [tuple(int(x) for x in row) for row in out] == [tuple(k.triple())] * G
        assert (lib.nrg_group_last_error(g) or b"") == b""
    finally:
        assert lib.nrg_group_close(g) == L.NRG_OK


@pytest.mark.parametrize("name", ["hashmap", "stack"])
def test_group_resync_thread_ranks(nrg, orc, name):
    """one rank per thread (nrg_group_join): rank 1 diverges, every rank calls resync(0)"""
    import torch

    from nrgpu import DeviceReplica
    from nrgpu.parallel import ReplicaGroup

    L = nrg._lib
    lib = L.load()
    G = 3
    k = {"hashmap": _HashMapKind, "stack": _StackKind}[name](nrg, orc)
    plan, triples = [], []
    for r, lens in enumerate([[50, 23, 41], [0, 37, 19], [61, 5, 19]]):
        plan.append([k.segment(lens[i], 100 * r + i) for i in range(G)])
        triples.append(tuple(k.triple()))

    def body(rank, uid):
        rep = DeviceReplica(k.kind, 0, replica_id=rank + 1, **k.cfg)
        grp = ReplicaGroup(rep, rank, G, uid=uid)
        keep = []

        def round_(parts):
            recs = parts[rank]
            d = _cuda(recs) if len(recs) else None
            keep.append(d)
            torch.cuda.synchronize()
            grp.round_async(d, len(recs))

        round_(plan[0])
        round_(plan[1])
        grp.sync()
        if rank == 1:
            keep.append(_diverge(nrg, lib, L, name, rep.handle))
        same0, d0 = grp.verify()
        grp.resync(0)
        same1, d1 = grp.verify()
        round_(plan[2])
        same2, d2 = grp.verify()
        tail = rep.log_state()["tail"]
        grp.close()
        rep.close()
        return same0, d0, same1, d1, same2, d2, tail

    out = _run_ranks(nrg, G, body)
    for rank in range(G):
        same0, d0, same1, d1, same2, d2, tail = out[rank]
        assert same0 is False and d0[0].tolist() == d0[2].tolist() != d0[1].tolist()
        assert same1 is True and tuple(int(x) for x in d1[rank]) == triples[1]
        assert same2 is True and [tuple(int(x) for x in row) for row in d2] == [triples[2]] * G
        assert tail == out[0][6]
