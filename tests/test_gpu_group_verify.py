"""nrg_group_verify over the loopback collectives: every rank's digest triple all-gathered, equal
on replicas that replayed the same log and equal to nrgpu.digest (the numpy mirror) of the model's
replay of W_0 || ... || W_{G-1}; a partitioned group's triples add up to the whole map's; a replica
that diverged is a result (identical = 0), not an error."""
import ctypes as C
import threading
from collections import deque

import numpy as np
import pytest

from nrgpu import digest
from vspace_model import KB4, MB2, VSpaceModel

pytestmark = pytest.mark.gpu

MIN_LOG_BYTES = 2 * 32 * 256 * 64
SLOT4 = 1 << 39


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def _open_group(nrg, kind, G, **cfgkw):
    L = nrg._lib
    lib = L.load()
    cfg = L.default_config(kind)
    for k, v in cfgkw.items():
        setattr(cfg, k, v)
    L.check(lib.nrg_test_loopback_collectives(1))
    g = C.c_void_p()
    try:
        L.check(lib.nrg_group_open((C.c_int * G)(*([0] * G)), G, C.byref(cfg), C.byref(g)), "nrg_group_open")
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))
    return g


def _verify(nrg, g, G):
    L = nrg._lib
    out = np.full((G, 3), 0x77, np.uint64)
    same = C.c_int(-1)
    rc = L.load().nrg_group_verify(g, out.ctypes.data_as(C.c_void_p), C.byref(same))
    return rc, same.value, out


# per kind: (config, records of a segment, the model's replay of one segment, the model's triple)
class _StackKind:
    def __init__(self, nrg, orc):
        self.kind, self.dtype = nrg._lib.NRG_DS_STACK, nrg.STACK_OP_DTYPE
        self.cfg = dict(max_batch=1 << 12, stack_capacity=1 << 16, log_bytes=MIN_LOG_BYTES)
        self.orc, self.model = orc, orc.Stack()

    def segment(self, n, seed):
        vals, ops = self.orc.gen_stack_ops(n, seed)
        ops[: n // 3] = 1
        r = np.zeros(n, self.dtype)
        r["val"], r["op"] = vals, ops
        if n:
            self.model.replay(vals, ops)
        return r

    def triple(self):
        return digest.stack(self.model.dump())


class _QueueKind:
    def __init__(self, nrg, orc):
        self.kind, self.dtype = nrg._lib.NRG_DS_QUEUE, nrg.QUEUE_OP_DTYPE
        self.cfg = dict(max_batch=1 << 12, queue_capacity=1 << 14, log_bytes=MIN_LOG_BYTES)
        self.q = deque()

    def segment(self, n, seed):
        rng = np.random.default_rng(seed)
        r = np.zeros(n, self.dtype)
        r["val"] = rng.integers(0, 2**64 - 1, n, dtype=np.uint64)
        r["op"] = (rng.random(n) < 0.6).astype(np.uint64)
        for v, o in zip(r["val"].tolist(), r["op"].tolist()):
            if o:
                self.q.append(v)
            elif self.q:
                self.q.popleft()
        return r

    def triple(self):
        return digest.queue(list(self.q))


class _VSpaceKind:
    def __init__(self, nrg, orc):
        self.kind, self.dtype = nrg._lib.NRG_DS_VSPACE, nrg.VSPACE_OP_DTYPE
        self.cfg = dict(max_batch=64, log2_slots=8, log_bytes=MIN_LOG_BYTES)
        self.model = VSpaceModel()

    def segment(self, n, seed):
        rng = np.random.default_rng(seed)
        lo = SLOT4 - 64 * (1 << 20)
        r = np.zeros(n, self.dtype)
        for i in range(n):
            if rng.random() < 0.2:
                r[i] = (lo + int(rng.integers(0, 64)) * MB2, int(rng.integers(0, 1 << 20)) * MB2,
                        int(rng.integers(1, 3)) * MB2 + int(rng.integers(0, 8)) * KB4, 0, int(rng.integers(1, 9)))
            else:
                r[i] = (lo + int(rng.integers(0, 1 << 15)) * KB4, int(rng.integers(0, 1 << 36)) * KB4,
                        int(rng.integers(0, 33)) * KB4, int(rng.integers(0, 2)), int(rng.integers(1, 9)))
        if n:
            self.model.replay(r)
        return r

    def triple(self):
        return digest.vspace(*self.model.dump())


class _HashMapKind:
    def __init__(self, nrg, orc):
        self.kind, self.dtype = nrg._lib.NRG_DS_HASHMAP, nrg.PUT_DTYPE
        self.cfg = dict(max_batch=1 << 12, log2_slots=14, log_bytes=MIN_LOG_BYTES)
        self.orc, self.model = orc, orc.HashMap()

    def segment(self, n, seed):
        r = np.zeros(n, self.dtype)
        r["key"], r["val"] = self.orc.gen_uniform(n, seed, 3000), self.orc.gen_raw(n, seed + 1)
        if n > 10:
            r["key"][7] = 0xFFFFFFFFFFFFFFFF
        if n:
            self.model.replay(r["key"].copy(), r["val"].copy())
        return r

    def triple(self):
        return self.model.digest()


KINDS = {"stack": _StackKind, "queue": _QueueKind, "vspace": _VSpaceKind, "hashmap": _HashMapKind}
CASES = [("stack", 2), ("stack", 3), ("queue", 2), ("queue", 3), ("vspace", 2), ("vspace", 3), ("hashmap", 3)]


@pytest.mark.parametrize("name,G", CASES, ids=[f"{n}-G{g}" for n, g in CASES])
def test_group_verify_replicated_rounds(nrg, orc, name, G):
    """Three replicated rounds with ragged segments, one of them empty: identical = 1 and every
    rank's triple is the mirror of the model's replay of W_0 || ... || W_{G-1}. For the stack a
    last step applies one Push to member 1 alone: NRG_OK, identical = 0, and the group still closes."""
    import torch

    L = nrg._lib
    lib = L.load()
    k = KINDS[name](nrg, orc)
    g = _open_group(nrg, k.kind, G, **k.cfg)
    rc, same, out = _verify(nrg, g, G)  # before any round
    assert rc == L.NRG_OK and same == 1
    assert [tuple(int(x) for x in row) for row in out] == [tuple(k.triple())] * G
    keep = []
    for r, lens in enumerate([[50, 23, 41], [0, 37, 0], [0, 0, 0], [61, 0, 19]]):
        rd = (L.Round * G)()
        for i in range(G):
            n = lens[i]
            recs = k.segment(n, 100 * r + i)  # (in rank order: the model replays W_0 || W_1 || ...)
            d_ops = _cuda(recs) if n else None
            rd[i].recs, rd[i].n = (d_ops.data_ptr() if n else 0), n
            if name == "hashmap":
                gk = torch.zeros(1, dtype=torch.int64, device="cuda")
                gv = torch.zeros(1, dtype=torch.int64, device="cuda")
                gf = torch.zeros(1, dtype=torch.uint8, device="cuda")
                rd[i].get_keys, rd[i].n_gets, rd[i].get_vals, rd[i].get_found = gk.data_ptr(), 1, gv.data_ptr(), gf.data_ptr()
                keep.append((gk, gv, gf))
            keep.append(d_ops)
        torch.cuda.synchronize()
        L.check(lib.nrg_group_round_async(g, rd, None), f"round {r}")
        if r == 1:  # mid-way, with the round still queued: verify completes it first
            rc, same, out = _verify(nrg, g, G)
            assert rc == L.NRG_OK and same == 1 and tuple(int(x) for x in out[0]) == tuple(k.triple())
    rc, same, out = _verify(nrg, g, G)
    print(name, G, out.tolist())
    assert rc == L.NRG_OK and same == 1
    want = tuple(k.triple())
    assert want[0] > 0
    for i in range(G):
        assert tuple(int(x) for x in out[i]) == want, f"rank {i}"
    # digests is nullable
    same = C.c_int(-1)
    assert lib.nrg_group_verify(g, None, C.byref(same)) == L.NRG_OK and same.value == 1
    assert lib.nrg_group_verify(g, None, None) == L.NRG_E_INVAL
    if name == "stack":
        # divergence: one direct Push on member 1 alone
        op = np.zeros(1, nrg.STACK_OP_DTYPE)
        op["val"], op["op"] = 4242, L.NRG_STACK_PUSH
        d_op = _cuda(op)
        torch.cuda.synchronize()
        L.check(lib.nrg_stack_round_async(lib.nrg_group_replica(g, 1), d_op.data_ptr(), 1, 2, None, None))
        rc, same, out = _verify(nrg, g, G)
        assert rc == L.NRG_OK and same == 0
        assert out[0].tolist() != out[1].tolist() and tuple(int(x) for x in out[0]) == want
        assert int(out[1][0]) == want[0] + 1
        assert (lib.nrg_group_last_error(g) or b"") == b""
    assert lib.nrg_group_close(g) == L.NRG_OK


def _run_ranks(nrg, G, body, timeout=90):
    """body(rank, uid) on G threads that form one loopback world; re-raise the first failure"""
    from nrgpu.parallel import ReplicaGroup

    L = nrg._lib
    lib = L.load()
    L.check(lib.nrg_test_loopback_collectives(1))
    errors, out = [None] * G, [None] * G
    try:
        uid = ReplicaGroup.unique_id()

        def run(rank):
            try:
                out[rank] = body(rank, uid)
            except BaseException as e:  # noqa: BLE001
                errors[rank] = e

        ts = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(G)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout)
        assert not any(t.is_alive() for t in ts), "a rank is still running (collective never matched)"
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))
    for e in errors:
        if e is not None:
            raise e
    return out


def test_group_verify_thread_ranks(nrg, orc):
    """One rank per thread, joined by unique id (nrg_group_join), G = 2, stack rounds with ragged
    segments: every rank gets the same digests array, identical, equal to the oracle's stack."""
    import torch

    from nrgpu import DeviceReplica
    from nrgpu.parallel import ReplicaGroup

    L = nrg._lib
    G = 2
    init = np.arange(300, dtype=np.uint32)
    st = orc.Stack(init)
    plan = []
    for r, lens in enumerate([[700, 300], [0, 450], [128, 0]]):
        parts = []
        for i in range(G):
            vals, ops = orc.gen_stack_ops(lens[i], 50 * r + i)
            st.replay(vals, ops)
            recs = np.zeros(lens[i], nrg.STACK_OP_DTYPE)
            recs["val"], recs["op"] = vals, ops
            parts.append(recs)
        plan.append(parts)
    want = digest.stack(st.dump())

    def body(rank, uid):
        rep = DeviceReplica(L.NRG_DS_STACK, 0, max_batch=1 << 12, stack_capacity=1 << 16, pipeline=1,
                            log_bytes=MIN_LOG_BYTES, replica_id=rank + 1)
        rep.st_init(init)
        grp = ReplicaGroup(rep, rank, G, uid=uid)
        keep = []
        for parts in plan:
            recs = parts[rank]
            d_ops = _cuda(recs) if len(recs) else None
            keep.append(d_ops)
            torch.cuda.synchronize()
            grp.round_async(d_ops, len(recs))
        same, digs = grp.verify()
        mine = rep.digest()
        dump = rep.st_dump()
        grp.close()
        rep.close()
        return same, digs, mine, dump

    out = _run_ranks(nrg, G, body)
    for rank in range(G):
        same, digs, mine, dump = out[rank]
        assert same is True and digs.shape == (G, 3) and digs.dtype == np.uint64
        np.testing.assert_array_equal(digs, out[0][1])
        assert tuple(int(x) for x in digs[rank]) == mine == want
        np.testing.assert_array_equal(dump, st.dump())


def test_group_verify_partitioned(nrg, orc):
    """A partitioned hashmap group, G = 3: each member holds one partition, so identical = 0 by
    design; the triples combine (count and sum add, xor xors) to the whole map's digest."""
    import torch

    from nrgpu import DeviceReplica
    from nrgpu.parallel import PartitionedGroup

    L = nrg._lib
    G, prefill, span = 3, 3000, 20_000
    om = orc.HashMap()
    om.prefill_range(prefill, 1)
    plan = []
    for r in range(2):
        parts = []
        for i in range(G):
            W = [1500, 0, 900][(i + r) % 3]
            k, v = orc.gen_uniform(W, 300 * r + i, span), orc.gen_raw(W, 300 * r + i + 100)
            om.replay(k, v)
            parts.append((k, v))
        plan.append(parts)
    want = om.digest()

    def body(rank, uid):
        rep = DeviceReplica(L.NRG_DS_HASHMAP, 0, log2_slots=15, max_batch=4096, replica_id=rank + 1)
        rep.hm_prefill_partition(prefill, 1, rank, G)
        grp = PartitionedGroup(rep, rank, G, uid=uid)
        keep = []
        for parts in plan:
            k, v = parts[rank]
            W = len(k)
            p = _cuda(np.stack([k, v], 1).astype(np.uint64)) if W else None
            gv = torch.zeros(1, dtype=torch.int64, device="cuda")
            gf = torch.zeros(1, dtype=torch.uint8, device="cuda")
            keep.append((p, gv, gf))
            torch.cuda.synchronize()
            grp.round_async(p, W, None, 0, gv, gf)  # posted: verify completes it
        same, digs = grp.verify()
        mine = rep.digest()
        grp.close()
        rep.close()
        return same, digs, mine

    out = _run_ranks(nrg, G, body)
    digs = out[0][1]
    for rank in range(G):
        same, d, mine = out[rank]
        assert same is False
        np.testing.assert_array_equal(d, digs)
        assert tuple(int(x) for x in d[rank]) == mine
    assert all(int(digs[i][0]) > 0 for i in range(G))
    assert digest.combine(digs) == want
