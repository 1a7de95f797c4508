"""nrg_digest / nrg_digest_async on every kind: the device's triple against nrgpu.digest (the numpy
mirror of the definition) applied to the CPU oracle's or the sequential model's state, never to
the device's own dump alone; the device's dump is checked against the same model beside it."""
import ctypes as C

import numpy as np
import pytest

from nrgpu import digest
from vspace_model import KB4, MB2, VSpaceModel, bench_ops

pytestmark = pytest.mark.gpu

EMPTY = 0xFFFFFFFFFFFFFFFF
MIN_LOG_BYTES = 2 * 32 * 256 * 64
GB1 = 1 << 30
SLOT4 = 1 << 39
V0 = (3 << 39) | (5 << 30) | (7 << 21)
M, D = 0, 1
SENTINEL = 0x5A5A5A5A5A5A5A5A
# the reduction kernels cap themselves at 1024 workgroups of 256 lanes (common.hpp DG_MAX_GRID, DG_TPB)
GRID_ITEMS = 1024 * 256


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


def _async_digest(dev):
    """nrg_digest_async into a device tensor pre-filled with a sentinel, read after sync"""
    import torch

    t = torch.full((3,), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    dev.digest_device(t)
    dev.sync()
    return tuple(int(x) for x in t.cpu().numpy().view(np.uint64))


def _both(dev):
    d = dev.digest()
    print("digest", d)
    assert _async_digest(dev) == d
    return d


# ---- hashmap ------------------------------------------------------------------------------------
def _hm_check(dev, om):
    want = om.digest()
    k, v = om.dump_sorted()
    assert digest.pairs(k, v) == want  # (the mirror, on the oracle alone)
    dk, dv = dev.hm_dump()
    np.testing.assert_array_equal(dk, k)
    np.testing.assert_array_equal(dv, v)
    assert dev.digest() == dev.hm_digest() == want


@pytest.mark.parametrize("knobs", [{}, {"PART": 2}], ids=["stamp", "partition"])
def test_hashmap_digest(nrg, orc, knobs):
    """after a prefill, a round without previous values (a stamp round, or a partition round with
    PART = 2), a round with the side key, and a round with previous values"""
    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_HASHMAP, 0, knobs=knobs, log2_slots=14, max_batch=8192)
    om = orc.HashMap()
    assert _both(dev) == (0, 0, 0)
    dev.hm_prefill_range(1000, 1)
    om.prefill_range(1000, 1)
    _hm_check(dev, om)
    for r, side in enumerate([False, True, True]):
        keys = orc.gen_uniform(3000, 20 + r, 2500)
        vals = orc.gen_raw(3000, 30 + r)
        if side:
            keys[5::301] = EMPTY
        recs = np.zeros(3000, nrg.PUT_DTYPE)
        recs["key"], recs["val"] = keys, vals
        first = dev.log_append(recs, 1)
        if r == 2:
            dev.log_exec(first, first + 3000)
        else:
            dev.log_exec()
        om.replay(keys, vals)
        _hm_check(dev, om)
    assert _async_digest(dev) == om.digest()
    dev.close()


def test_hashmap_digest_after_growth(nrg, orc):
    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_HASHMAP, 0, log2_slots=10, hashmap_max_log2_slots=14, max_batch=4096)
    om = orc.HashMap()
    for r in range(2):
        keys = orc.gen_uniform(2000, 70 + r, 1 << 40)
        vals = orc.gen_raw(2000, 80 + r)
        recs = np.zeros(2000, nrg.PUT_DTYPE)
        recs["key"], recs["val"] = keys, vals
        dev.log_append(recs, 1)
        dev.log_exec()
        om.replay(keys, vals)
        _hm_check(dev, om)
    assert dev.hm_log2_slots() > 10
    assert _async_digest(dev) == om.digest()
    dev.close()


# ---- stack --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, GRID_ITEMS + 7])
def test_stack_digest_lengths(nrg, orc, n):
    """nrg_stack_init of n values; the last length takes some lanes round the grid-stride loop twice"""
    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_STACK, 0, max_batch=4096)
    assert dev.cfg.stack_capacity >= GRID_ITEMS * 16  # (so the kernel's grid is at its cap)
    init = (orc.gen_raw(n, 5) >> np.uint64(32)).astype(np.uint32) if n else np.zeros(0, np.uint32)
    dev.st_init(init)
    os_ = orc.Stack(init)
    want = digest.stack(os_.dump())
    assert want[0] == n and (n > 0 or want == (0, 0, 0))
    np.testing.assert_array_equal(dev.st_dump(), os_.dump())
    assert _both(dev) == want
    dev.close()


def test_stack_digest_flushes_a_deferred_finish(nrg, orc):
    """pipeline = 1: a 4097-op round (three tiles) whose finish is still deferred, then the digest
    without a join: it is the oracle's stack after the round"""
    import torch

    n = 4097
    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_STACK, 0, max_batch=8192, stack_capacity=1 << 16, pipeline=1)
    init = np.arange(100, dtype=np.uint32)
    dev.st_init(init)
    os_ = orc.Stack(init)
    vals, ops = orc.gen_stack_ops(n, 41)
    ops[:300] = 0  # Pops past the bottom, then a net rise
    recs = np.zeros(n, nrg.STACK_OP_DTYPE)
    recs["val"], recs["op"] = vals, ops
    d_ops = _cuda(recs)
    resp = torch.zeros(n, dtype=torch.int32, device="cuda")
    some = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dev.st_round_device(d_ops, n, 1, resp, some)
    os_.replay(vals, ops)
    want = digest.stack(os_.dump())
    assert dev.digest() == want and want[0] == len(os_) > 0
    assert _async_digest(dev) == want
    np.testing.assert_array_equal(dev.st_dump(), os_.dump())
    dev.close()


# ---- queue --------------------------------------------------------------------------------------
def test_queue_digest_round_the_ring(nrg):
    """capacity 8 and chunks of 8: a ring of 16 slots. Rounds of Push and Pop until the front has
    passed slot 16 more than twice; the digest is the list model's after every round, one of
    which leaves the queue empty."""
    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_QUEUE, 0, queue_capacity=8, max_batch=8, log_bytes=MIN_LOG_BYTES)
    rng = np.random.default_rng(12)
    q, popped, emptied, rounds = [], 0, 0, 0
    assert _both(dev) == (0, 0, 0)
    while popped <= 40 or not emptied:
        drain = rounds % 5 == 4
        vals = rng.integers(0, 2**64 - 1, 8, dtype=np.uint64)
        ops = np.zeros(8, np.uint64)
        for i in range(8):
            push = (not drain) and (len(q) == 0 or (len(q) < 8 and rng.random() < 0.55))
            if push:
                ops[i] = 1
                q.append(int(vals[i]))
            elif q:
                q.pop(0)
                popped += 1
        recs = np.zeros(8, nrg.QUEUE_OP_DTYPE)
        recs["val"], recs["op"] = vals, ops
        first = dev.log_append(recs, 1)
        dev.log_exec(first, first + 8)
        want = digest.queue(q)
        assert dev.digest() == want, f"round {rounds}"
        np.testing.assert_array_equal(dev.qu_dump(), np.array(q, np.uint64))
        if not q:
            emptied += 1
            assert want == (0, 0, 0)
        rounds += 1
    assert popped > 32 and emptied
    assert _async_digest(dev) == digest.queue(q)
    dev.close()


def test_queue_digest_default_capacity(nrg):
    """70,000 elements from nrg_queue_init_range, then a round that pops 5 and pushes 3"""
    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_QUEUE, 0, max_batch=4096)
    dev.qu_init_range(70_000)
    q = list(range(70_000))
    assert _both(dev) == digest.queue(q)
    recs = np.zeros(8, nrg.QUEUE_OP_DTYPE)
    recs["op"] = [0, 0, 0, 0, 0, 1, 1, 1]
    recs["val"] = [0, 0, 0, 0, 0, 11, EMPTY, 13]
    first = dev.log_append(recs, 1)
    dev.log_exec(first, first + 8)
    q = q[5:] + [11, EMPTY, 13]
    np.testing.assert_array_equal(dev.qu_dump(), np.array(q, np.uint64))
    assert _both(dev) == digest.queue(q)
    dev.close()


# ---- synthetic ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0])
def test_synthetic_digest(nrg, orc, fused):
    """pipeline = 1: after a round whose sums and hot-word fold are still deferred (one launch per
    round, and SY_FUSED = 0), the digest without a join is the oracle's storage"""
    import torch

    n = 20_000
    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_SYNTHETIC, 0, knobs={"SY_FUSED": fused}, max_batch=1 << 15, pipeline=1)
    os_ = orc.Synthetic()
    want0 = digest.synthetic(os_.dump())
    assert want0[0] == 200_000 and dev.digest() == want0
    keep = []
    for r in range(2):
        raw = orc.gen_raw(4 * n, 600 + r)
        ops = np.zeros(n, nrg.SYNTH_OP_DTYPE)
        ops["tid"], ops["r1"], ops["r2"] = raw[0::4] % 64, raw[1::4], raw[2::4]
        ops["op"] = (raw[3::4] % 100 >= 10).astype(np.uint64)
        d_ops = _cuda(ops)
        resp = torch.zeros(n, dtype=torch.int64, device="cuda")
        some = torch.zeros(n, dtype=torch.uint8, device="cuda")
        dev.sy_round_device(d_ops, n, 1, resp, some)
        keep.append((d_ops, resp, some))
        os_.replay(np.stack([ops["tid"], ops["r1"], ops["r2"], ops["op"]], axis=1))
        want = digest.synthetic(os_.dump())
        assert dev.digest() == want != want0, f"round {r}"
    assert _async_digest(dev) == want
    np.testing.assert_array_equal(dev.sy_dump(), os_.dump())
    dev.close()


# ---- vspace -------------------------------------------------------------------------------------
def _recs(nrg, rows):
    r = np.zeros(len(rows), nrg.VSPACE_OP_DTYPE)
    for i, row in enumerate(rows):
        r[i] = row
    return r


def _vs_open(nrg, **kw):
    kw.setdefault("log2_slots", 8)
    kw.setdefault("max_batch", 64)
    kw.setdefault("log_bytes", MIN_LOG_BYTES)
    return nrg.DeviceReplica(nrg._lib.NRG_DS_VSPACE, 0, **kw)


def _vs_check(dev, model):
    va, en = model.dump()
    want = digest.vspace(va, en)
    d = dev.vs_dump()
    np.testing.assert_array_equal(d["vaddr"], va)
    np.testing.assert_array_equal(d["entry"], en)
    assert dev.vs_tables() == model.tables()
    got = dev.digest()
    print("vspace digest", got, "tables", model.tables(), "leaves", len(va))
    assert got == want
    return want


VS_CASES = {
    "empty": [],
    "four_pages": [(V0 + 3 * KB4, 0x10_0000, 4 * KB4, M, 3)],
    # a PD holding three 2 MiB leaves and a PT
    "large_and_pt": [(V0, 0x4000_0000, 3 * MB2 + 5 * KB4, M, 7), (V0 + 8 * MB2, 0x4000_1000, MB2, M, 3)],
    # into a second PD (a 1 GiB boundary) and into a second PDPT (a 512 GiB boundary)
    "second_pd": [(6 * GB1 - 3 * KB4, 0x70_0000, 9 * KB4, D, 0)],
    "second_pdpt": [(2 * SLOT4 - 2 * KB4, 0x1_0000_0000, 5 * KB4, M, 7)],
    "large_across_pd": [(9 * GB1 - 2 * MB2, 0x8000_0000, 5 * MB2, D, 0)],
    # PML4 slot 511: the vaddr is raw, not sign-extended
    "top_slot": [(0xFF80_0000_3000, 0x9000, 2 * KB4, M, 3)],
    "zero_length": [(V0 + 5 * KB4, 0x1000, 0, M, 3)],
}


@pytest.mark.parametrize("name", list(VS_CASES))
def test_vspace_digest_cases(nrg, name):
    dev = _vs_open(nrg)
    model = VSpaceModel()
    recs = _recs(nrg, VS_CASES[name])
    if len(recs):
        first = dev.log_append(recs, 1)
        _, some = dev.log_exec(first, first + len(recs))
        _, _, s = model.replay(recs)
        np.testing.assert_array_equal(some, s)
        assert s.all()
    want = _vs_check(dev, model)
    assert _async_digest(dev) == want
    if name in ("empty", "zero_length"):
        assert want == (0, 0, 0)
    if name == "zero_length":
        assert model.tables() >= 2  # a PT with no present entry, and the tables above it
    if name == "top_slot":
        assert model.dump()[0].tolist() == [0xFF80_0000_3000, 0xFF80_0000_4000]
    if name == "large_and_pt":
        en = model.dump()[1]
        assert int(((en & np.uint64(0x80)) != 0).sum()) == 3 and len(en) == 3 + 5 + 512
    dev.close()


def test_vspace_digest_then_map_more(nrg):
    """digest, map more (new tables under tables an earlier digest tagged, and a new PML4 slot),
    digest again: the mirror of the new model each time"""
    dev = _vs_open(nrg)
    model = VSpaceModel()
    seen = []
    for rows in ([(V0 + 3 * KB4, 0x10_0000, 4 * KB4, M, 3), (2 * SLOT4, 0x9000, 2 * KB4, M, 3)],
                 [(V0 + 5 * MB2, 0x4000_0000, 2 * MB2, M, 7), (V0 + 40 * KB4, 0x7000, 600 * KB4, D, 0)],
                 [(7 * SLOT4 + GB1, 0x1000, KB4, M, 1), (V0 + 3 * KB4, 0x1000, KB4, M, 3)]):
        recs = _recs(nrg, rows)
        first = dev.log_append(recs, 1)
        _, some = dev.log_exec(first, first + len(recs))
        np.testing.assert_array_equal(some, model.replay(recs)[2])
        seen.append(_vs_check(dev, model))
        assert _async_digest(dev) == seen[-1]
    assert len(set(seen)) == 3
    dev.close()


def _replay_capped(model, recs, cap):
    """the sequential replay in a pool of `cap` tables: an op whose tables do not fit changes nothing"""
    import copy

    s = np.zeros(len(recs), np.uint8)
    for i in range(len(recs)):
        trial = copy.deepcopy(model)
        si = trial.replay(recs[i:i + 1])[2]
        if trial.tables() <= cap:
            model.t = trial.t
            s[i] = si[0]
    return s


def test_vspace_digest_after_pool_exhaustion(nrg):
    """A pool of 16 tables with 10 taken, then a chunk whose third op is left out for lack of
    tables (tests/test_gpu_vspace.py first_wave_after_dependent): the digest is that of the
    sequential replay that leaves out exactly that op."""
    L = nrg._lib
    big = (5 * SLOT4 + KB4, 0x5000, KB4, M, 3)
    dev = _vs_open(nrg, log2_slots=4)
    model = VSpaceModel()
    ok = _recs(nrg, [(V0, 0x1000, 4 * KB4, M, 3), (2 * SLOT4, 0x9000, 2 * KB4, M, 3), (7 * SLOT4, 0x1000, KB4, M, 3)])
    first = dev.log_append(ok, 1)
    dev.log_exec(first, first + len(ok))
    model.replay(ok)
    assert model.tables() == 10
    _vs_check(dev, model)
    recs = _recs(nrg, [(9 * SLOT4, 0xA000, KB4, M, 3), (9 * SLOT4 + 511 * KB4, 0xB000, 2 * KB4, M, 1), big,
                       (V0 + 6 * KB4, 0x2000, KB4, M, 3)])
    s = _replay_capped(model, recs, 16)
    assert s.tolist() == [1, 1, 0, 1]
    dev.log_append(recs, 1)
    with pytest.raises(nrg.NrgError) as e:
        dev.log_exec()
        dev.sync()
    assert e.value.code == L.NRG_E_CAPACITY
    dev.sync()
    want = _vs_check(dev, model)
    assert _async_digest(dev) == want and want[0] == 4 + 2 + 1 + 1 + 2 + 1
    dev.close()


def test_vspace_digest_bench_shaped(nrg):
    """48 ops drawn as generate_operations draws them: about 3,100 tables and 1M leaves"""
    recs = bench_ops(np.random.default_rng(11), 48, nrg.VSPACE_OP_DTYPE)
    dev = _vs_open(nrg, log2_slots=12, max_batch=48)
    model = VSpaceModel()
    first = dev.log_append(recs, 1)
    _, some = dev.log_exec(first, first + 48)
    assert model.replay(recs)[2].all() and some.all() and 2000 < model.tables() <= 4096
    want = _vs_check(dev, model)
    assert want[0] > 900_000 and _async_digest(dev) == want
    dev.close()


def _table(dev, t):
    out = np.zeros(512, np.uint64)
    nrgl = dev._lib
    assert nrgl.nrg_test_vspace_table(dev.handle, t, out.ctypes.data_as(C.c_void_p)) == 0
    return out


def test_vspace_digest_does_not_depend_on_allocation_order(nrg):
    """40 ops on pairwise distinct 2 MiB granules spread over PML4 slots, PDPTs and PDs, replayed
    one op per chunk in order on one replica and in reverse order on another: equal digests and
    dumps, although the tables were handed out in different orders (the PML4s' entries differ)."""
    rows = []
    for i in range(40):
        v = (1 + i % 4) * SLOT4 + (i % 5) * GB1 + (3 * i + 1) * MB2 + (i % 7) * KB4
        if i % 3 == 0:
            rows.append(((1 + i % 4) * SLOT4 + (i % 5) * GB1 + (3 * i + 1) * MB2, i * MB2, MB2, M, 1 + i % 8))
        else:
            rows.append((v, 0x1000 * (i + 1), (1 + i % 9) * KB4, i % 2, 1 + i % 8))
    recs = _recs(nrg, rows)
    gr = recs["vbase"] >> np.uint64(21)
    assert len(set(gr.tolist())) == 40 and np.all((recs["vbase"] + recs["len"] - np.uint64(1)) >> np.uint64(21) == gr)
    model = VSpaceModel()
    assert model.replay(recs)[2].all()
    devs = []
    for order in (recs, recs[::-1].copy()):
        dev = _vs_open(nrg, max_batch=1)
        first = dev.log_append(order, 1)
        _, some = dev.log_exec(first, first + 40)
        assert some.all() and dev.log_state()["ltail"] == 40
        devs.append(dev)
    a, b = devs
    want = _vs_check(a, model)
    assert _vs_check(b, model) == want
    assert _async_digest(a) == _async_digest(b) == want
    assert not np.array_equal(_table(a, 0), _table(b, 0))  # not vacuous: inner entries differ
    a.close()
    b.close()
