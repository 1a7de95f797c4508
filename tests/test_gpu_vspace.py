"""Replicated page table parity: the HIP replay (vspace.hip) against the sequential model of
tests/vspace_model.py (benches/vspace.rs:177-381 map_generic, :436-467 resolve_addr, :499-526
VSpaceDispatcher).

Every case compares, bit for bit, each response (a, b, some), the number of tables, the full leaf
dump, and Identify of every touched page boundary, its neighbours, offsets inside pages and
addresses with bits 48..63 set. Pools hold 2^2 .. 2^12 tables and chunks 64 ops unless said.
"""
import ctypes as C

import numpy as np
import pytest

from vspace_model import KB4, MB2, VSpaceModel, bench_ops

pytestmark = pytest.mark.gpu

MIN_LOG_BYTES = 2 * 32 * 256 * 64  # Log::new's floor: 2 * GC_FROM_HEAD entries of 64 bytes
GB1 = 1 << 30
SLOT4 = 1 << 39                     # one PML4 slot: 512 GiB
V0 = (3 << 39) | (5 << 30) | (7 << 21)  # PML4 slot 3, PDPT slot 5, PD slot 7: 2 MiB-aligned
M, D = 0, 1                         # NRG_VSPACE_MAP, NRG_VSPACE_MAP_DEVICE


def _recs(nrg, rows):
    """rows of (vbase, pbase, len, op, rights)"""
    r = np.zeros(len(rows), nrg.VSPACE_OP_DTYPE)
    for i, row in enumerate(rows):
        r[i] = row
    return r


def _open(nrg, **kw):
    kw.setdefault("log2_slots", 8)
    kw.setdefault("max_batch", 64)
    kw.setdefault("log_bytes", MIN_LOG_BYTES)
    return nrg.DeviceReplica(nrg._lib.NRG_DS_VSPACE, 0, **kw)


def _probes(recs):
    """every touched page boundary and 2 MiB boundary inside a range, the pages next to them,
    offsets inside those pages, and the same with bits 48..63 set"""
    a = []
    for r in recs:
        v, n = int(r["vbase"]), int(r["len"])
        edges = [v, v + n] + list(range((v | (MB2 - 1)) + 1, v + n, MB2))
        for e in edges:
            a += [e - KB4, e, e + KB4]
    a = np.array([x for x in a if 0 <= x < 1 << 48], np.uint64)
    a = np.unique(a)
    return np.concatenate([a, a + np.uint64(0x123), a + np.uint64(KB4 - 1), a | np.uint64(0xFFFF << 48),
                           a | np.uint64(0x8000 << 48) | np.uint64(0x7)])


def _check_state(dev, model, recs):
    assert dev.vs_tables() == model.tables()
    d = dev.vs_dump()
    va, en = model.dump()
    np.testing.assert_array_equal(d["vaddr"], va)
    np.testing.assert_array_equal(d["entry"], en)
    probes = _probes(recs)
    pa, found = dev.vs_resolve(probes)
    want = [model.resolve(int(x)) for x in probes]
    np.testing.assert_array_equal(pa, np.array([w[0] for w in want], np.uint64))
    np.testing.assert_array_equal(found, np.array([w[1] for w in want], np.uint8))


def _exec(dev, model, recs):
    """append + exec of one batch with every response wanted, against the model"""
    first = dev.log_append(recs, 1)
    resp, some = dev.log_exec(first, first + len(recs))
    a, b, s = model.replay(recs)
    np.testing.assert_array_equal(some, s)
    np.testing.assert_array_equal(resp["a"], a)
    np.testing.assert_array_equal(resp["b"], b)
    return s


def _play(nrg, batches, **kw):
    """the batches one exec call each; state checked after every one"""
    dev = _open(nrg, **kw)
    model = VSpaceModel()
    seen, somes = [], []
    for rows in batches:
        recs = _recs(nrg, rows)
        seen.append(recs)
        somes.append(_exec(dev, model, recs))
        _check_state(dev, model, np.concatenate(seen))
    dev.sync()
    dev.close()
    return model, somes


def test_vspace_one_map_of_four_pages(nrg):
    model, somes = _play(nrg, [[(V0 + 3 * KB4, 0x10_0000, 4 * KB4, M, 3)]])
    assert model.tables() == 4 and somes[0].tolist() == [1]


def test_vspace_table_boundaries(nrg):
    """ranges crossing a PT boundary, a PD boundary (1 GiB) and a PML4-slot boundary (512 GiB)"""
    rows = [(V0 + 509 * KB4, 0x5000, 7 * KB4, M, 3),
            (6 * GB1 - 3 * KB4, 0x70_0000, 9 * KB4, D, 0),
            (2 * SLOT4 - 2 * KB4, 0x1_0000_0000, 5 * KB4, M, 7)]
    model, somes = _play(nrg, [rows])
    assert somes[0].all()
    # PML4; four PDPTs (slots 3, 0, 1, 2); five PDs; six PTs
    assert model.tables() == 1 + 4 + 5 + 6
    _play(nrg, [[r] for r in rows])


def test_vspace_large_pages(nrg):
    # aligned 3 x 2 MiB + 5 pages; vbase aligned but pbase not: 512 PTEs; a run across a PD boundary
    rows = [(V0, 0x4000_0000, 3 * MB2 + 5 * KB4, M, 7),
            (V0 + 8 * MB2, 0x4000_1000, MB2, M, 3),
            (9 * GB1 - 2 * MB2, 0x8000_0000, 5 * MB2, D, 0)]
    model, somes = _play(nrg, [rows])
    assert somes[0].all()
    va, en = model.dump()
    assert int(((en & np.uint64(0x80)) != 0).sum()) == 3 + 5 and len(va) == 8 + 5 + 512
    dev = _open(nrg)
    _exec(dev, VSpaceModel(), _recs(nrg, rows[:1]))
    pa, found = dev.vs_resolve(np.array([V0 + MB2 + 0x12345, V0 + 3 * MB2 - 1, V0 + 3 * MB2 + 5 * KB4], np.uint64))
    assert pa.tolist() == [0x4000_0000 + MB2 + 0x12345, 0x4000_0000 + 3 * MB2 - 1, 0] and found.tolist() == [1, 1, 0]
    dev.close()


def test_vspace_rights_and_map_device(nrg):
    """each of the 8 rights, 4 KiB and 2 MiB, and MapDevice: the flags through the dump"""
    rows = [(V0 + r * KB4, r * 0x10_0000, KB4, M, r) for r in range(1, 9)]
    rows += [(V0 + (4 + r) * MB2, r * MB2, MB2, M, r) for r in range(1, 9)]
    rows += [(V0 + 20 * KB4, 0x7000, KB4, D, 5), (V0 + 20 * MB2, 64 * MB2, MB2, D, 0)]
    model, somes = _play(nrg, [rows])
    assert somes[0].all()
    en = dict(zip(*[x.tolist() for x in model.dump()]))
    P, RW, US, PS, XD = 1, 2, 4, 0x80, 1 << 63
    assert en[V0 + 2 * KB4] == 2 * 0x10_0000 | P | US | XD and en[V0 + 7 * KB4] == 7 * 0x10_0000 | P | RW
    assert en[V0 + 9 * MB2] == 5 * MB2 | P | PS and en[V0 + 12 * MB2] == 8 * MB2 | P | PS | RW | US
    assert en[V0 + 20 * KB4] == 0x7000 | P | RW | XD and en[V0 + 20 * MB2] == 64 * MB2 | P | PS | RW | XD


CONFLICTS = {
    # an exact remap
    "remap": [(V0, 0x1000, 4 * KB4, M, 3), (V0, 0x9000, 4 * KB4, M, 3)],
    # starts free, meets a mapped page mid-PT: the prefix stays, at = the frame's start
    "mid_pt": [(V0 + 8 * KB4, 0x1000, 2 * KB4, M, 3), (V0 + 4 * KB4, 0x20_0000, 8 * KB4, M, 1)],
    # the same with the failure in the op's second frame
    "second_frame": [(V0 + MB2 + 3 * KB4, 0x1000, KB4, M, 3), (V0 + 510 * KB4, 0x30_0000, 10 * KB4, D, 0)],
    # a run of large pages meets a PT
    "run_meets_pt": [(V0 + 2 * MB2, 0x1000, KB4, M, 3), (V0, 0x4000_0000, 4 * MB2, M, 7)],
    # an aligned request whose first granule already has a PT: 4 KiB there, large pages after it
    "pt_then_large": [(V0, 0, 0, M, 3), (V0, 0x4000_0000, 3 * MB2, M, 7)],
    # a 4 KiB map into a granule that holds a large page
    "into_large": [(V0, 0x4000_0000, MB2, M, 7), (V0 + 3 * KB4, 0x1000, KB4, M, 3)],
}
CONFLICT_OK = {"remap": [1, 0], "mid_pt": [1, 0], "second_frame": [1, 0], "run_meets_pt": [1, 0],
               "pt_then_large": [1, 1], "into_large": [1, 0]}


@pytest.mark.parametrize("together", [False, True], ids=["separate_execs", "one_chunk"])
@pytest.mark.parametrize("name", list(CONFLICTS))
def test_vspace_conflicts(nrg, name, together):
    rows = CONFLICTS[name]
    _, somes = _play(nrg, [rows] if together else [[r] for r in rows])
    assert np.concatenate(somes).tolist() == CONFLICT_OK[name]


def test_vspace_chain_on_one_granule(nrg):
    """8 ops on one granule in one chunk: each sees what the ones before it left"""
    rows = [(V0 + 10 * KB4, 0x1000, 4 * KB4, M, 3),    # ok
            (V0 + 12 * KB4, 0x2000, 4 * KB4, M, 3),    # err at once
            (V0 + 14 * KB4, 0x3000, 4 * KB4, M, 1),    # ok (the second op wrote nothing)
            (V0 + 6 * KB4, 0x4000, 6 * KB4, D, 0),     # 4 pages, then err
            (V0, 0x4000_0000, MB2, M, 7),              # aligned, but the granule has a PT: 6 pages, err
            (V0 + 18 * KB4, 0x5000, 0, M, 3),          # len 0: ok
            (V0 + 511 * KB4, 0x6000, 2 * KB4, M, 8),   # crosses into the next granule: ok
            (V0 + 500 * KB4, 0x7000, 20 * KB4, M, 2)]  # 11 pages, then err
    _, somes = _play(nrg, [rows])
    assert somes[0].tolist() == [1, 0, 1, 0, 0, 1, 1, 0]
    _play(nrg, [[r] for r in rows])


def test_vspace_zero_length(nrg):
    rows = [(V0 + 5 * KB4, 0x1000, 0, M, 3), (V0 + MB2, 0, 0, D, 0), (2 * SLOT4, 0x5000, 0, M, 1)]
    model, somes = _play(nrg, [rows])
    assert somes[0].all() and model.tables() == 1 + 2 + 2 + 3 and len(model.dump()[0]) == 0


def _mix(nrg, seed, n=300):
    """20 % aligned requests of 1..3 x 2 MiB + 0..7 pages, 80 % 4 KiB-aligned ones of 0..64 pages,
    vbase in a 128 MiB window that straddles a PML4-slot boundary"""
    rng = np.random.default_rng(seed)
    lo = SLOT4 - 64 * (1 << 20)
    rows = []
    for _ in range(n):
        if rng.random() < 0.2:
            v = lo + int(rng.integers(0, 64)) * MB2
            p = int(rng.integers(0, 1 << 20)) * MB2
            ln = int(rng.integers(1, 4)) * MB2 + int(rng.integers(0, 8)) * KB4
        else:
            v = lo + int(rng.integers(0, 1 << 15)) * KB4
            p = int(rng.integers(0, 1 << 36)) * KB4
            ln = int(rng.integers(0, 65)) * KB4
        rows.append((v, p, ln, int(rng.integers(0, 2)), int(rng.integers(1, 9))))
    return _recs(nrg, rows)


MIX_SEED = 7


def _cuda_bytes(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def _resp_of(t):
    return t.cpu().numpy().view(np.uint64).reshape(-1, 2)


def test_vspace_random_mix_three_ways(nrg):
    """300 seeded ops: append + exec in chunks of 64 with a response sub-window, the same through
    nrg_vspace_round_async, the same as segments: the model's answers and state each time."""
    import torch

    recs = _mix(nrg, MIX_SEED)
    n = len(recs)
    model = VSpaceModel()
    a, b, s = model.replay(recs)
    assert int(s.sum()) >= n // 4 and int((s == 0).sum()) >= n // 4  # (on the model alone)
    mva, men = model.dump()
    # append, then one exec call that replays five chunks; responses for [50, 250) only
    dev = _open(nrg)
    first = dev.log_append(recs, 1)
    resp, some = dev.log_exec(first + 50, first + 250)
    np.testing.assert_array_equal(some, s[50:250])
    np.testing.assert_array_equal(resp["a"], a[50:250])
    np.testing.assert_array_equal(resp["b"], b[50:250])
    _check_state(dev, model, recs)
    dev.close()
    # fused rounds of at most 64
    dev = _open(nrg)
    outs = []
    for lo in range(0, n, 64):
        k = min(64, n - lo)
        d_ops = _cuda_bytes(recs[lo:lo + k])
        r = torch.full((k, 2), -1, dtype=torch.int64, device="cuda")
        sm = torch.full((k,), 7, dtype=torch.uint8, device="cuda")
        dev.vs_round_device(d_ops, k, 1, r, sm)
        outs.append((d_ops, r, sm))
    dev.sync()
    got = np.concatenate([_resp_of(r) for _, r, _ in outs])
    np.testing.assert_array_equal(np.concatenate([sm.cpu().numpy() for _, _, sm in outs]), s)
    np.testing.assert_array_equal(got[:, 0], a)
    np.testing.assert_array_equal(got[:, 1], b)
    _check_state(dev, model, recs)
    st = dev.log_state()
    assert (st["tail"], st["ltail"]) == (n, n)
    dev.close()
    # three segments of unequal length; responses for the middle one
    dev = _open(nrg)
    lens, stride = [100, 37, 163], 163
    buf = np.zeros(3 * stride, nrg.VSPACE_OP_DTYPE)
    off = [0, 100, 137]
    for i in range(3):
        buf[i * stride: i * stride + lens[i]] = recs[off[i]: off[i] + lens[i]]
    d_base = _cuda_bytes(buf)
    firsts = dev.log_append_segments(d_base, stride, lens, [3, 1, 2])
    assert firsts == off
    r = torch.full((37, 2), -1, dtype=torch.int64, device="cuda")
    sm = torch.full((37,), 7, dtype=torch.uint8, device="cuda")
    dev.log_exec_device(100, 137, r, sm)
    dev.sync()
    np.testing.assert_array_equal(sm.cpu().numpy(), s[100:137])
    np.testing.assert_array_equal(_resp_of(r)[:, 0], a[100:137])
    np.testing.assert_array_equal(_resp_of(r)[:, 1], b[100:137])
    _check_state(dev, model, recs)
    d = dev.vs_dump()
    np.testing.assert_array_equal(d["vaddr"], mva)
    np.testing.assert_array_equal(d["entry"], men)
    dev.close()


def test_vspace_bench_shaped(nrg):
    """48 ops drawn as generate_operations draws them: about 3,100 tables and 1M leaves"""
    recs = bench_ops(np.random.default_rng(11), 48, nrg.VSPACE_OP_DTYPE)
    dev = _open(nrg, log2_slots=12, max_batch=48)
    model = VSpaceModel()
    s = _exec(dev, model, recs)
    assert s.all() and 2000 < model.tables() <= 4096
    _check_state(dev, model, recs)
    dev.close()


def _replay_capped(model, recs, cap):
    """the sequential replay in a pool of `cap` tables: an op whose tables do not fit changes
    nothing and answers some = 0, a = vbase, b = 0; the ops after it go on"""
    import copy

    a = np.zeros(len(recs), np.uint64)
    b = np.zeros(len(recs), np.uint64)
    s = np.zeros(len(recs), np.uint8)
    left_out = 0
    for i in range(len(recs)):
        trial = copy.deepcopy(model)
        ai, bi, si = trial.replay(recs[i:i + 1])
        if trial.tables() > cap:
            a[i], left_out = recs["vbase"][i], left_out + 1
        else:
            model.t = trial.t
            a[i], b[i], s[i] = ai[0], bi[0], si[0]
    return a, b, s, left_out


BIG = (5 * SLOT4 + KB4, 0x5000, KB4, M, 3)  # three new tables wherever it comes
EXHAUST = {
    # alone in its chunk: a first-wave op
    "first_wave": (3, [], [BIG]),
    # behind a zero-length op on its own granule, which does not fit either; the op before them does
    "in_log_order": (3, [], [(V0 + 6 * KB4, 0x2000, KB4, M, 3), (5 * SLOT4, 0x3000, 0, M, 3), BIG]),
    # 10 of 16 tables taken. The first op takes 3; the second depends on it and takes 1; the third is
    # independent of both, needs 3 and is the one log order leaves out, though it and the first
    # would fit without the second; the fourth needs none and goes on
    "first_wave_after_dependent": (4, [(7 * SLOT4, 0x1000, KB4, M, 3)],
                                   [(9 * SLOT4, 0xA000, KB4, M, 3), (9 * SLOT4 + 511 * KB4, 0xB000, 2 * KB4, M, 1),
                                    BIG, (V0 + 6 * KB4, 0x2000, KB4, M, 3)]),
}
EXHAUST_SOME = {"first_wave": [0], "in_log_order": [1, 0, 0], "first_wave_after_dependent": [1, 1, 0, 1]}


@pytest.mark.parametrize("name", list(EXHAUST))
def test_vspace_pool_exhaustion_latches_capacity_once(nrg, name):
    """A pool of 8 (16) tables with 7 (10) taken, then one chunk that needs more than are left:
    every response, the left-out ops' included (some = 0, a = vbase, b = 0), the table count, the
    dump and Identify are those of the sequential replay that leaves out exactly the ops whose
    tables do not fit; NRG_E_CAPACITY is reported once."""
    import torch

    L = nrg._lib
    log2, more, rows = EXHAUST[name]
    cap = 1 << log2
    dev = _open(nrg, log2_slots=log2)
    model = VSpaceModel()
    ok = _recs(nrg, [(V0, 0x1000, 4 * KB4, M, 3), (2 * SLOT4, 0x9000, 2 * KB4, M, 3)] + more)
    _exec(dev, model, ok)
    assert dev.vs_tables() == model.tables() == 7 + 3 * len(more)
    recs = _recs(nrg, rows)
    a, b, s, left_out = _replay_capped(model, recs, cap)
    assert s.tolist() == EXHAUST_SOME[name] and left_out == s.tolist().count(0)  # (on the model alone)
    first = dev.log_append(recs, 1)
    r = torch.full((len(rows), 2), -1, dtype=torch.int64, device="cuda")
    sm = torch.full((len(rows),), 7, dtype=torch.uint8, device="cuda")
    dev.log_exec_device(first, first + len(rows), r, sm)
    with pytest.raises(nrg.NrgError) as e:
        dev.sync()
    assert e.value.code == L.NRG_E_CAPACITY
    dev.sync()  # latched once: reported and cleared
    np.testing.assert_array_equal(sm.cpu().numpy(), s)
    np.testing.assert_array_equal(_resp_of(r)[:, 0], a)
    np.testing.assert_array_equal(_resp_of(r)[:, 1], b)
    assert dev.vs_tables() == model.tables() <= cap
    _check_state(dev, model, np.concatenate([ok, recs]))
    dev.close()


def test_vspace_out_of_domain_records(nrg):
    """a misaligned vbase, rights = 0, len = 2^30 (and more): state unchanged, some = 0 with
    a = vbase, NRG_E_INVAL latched once"""
    import torch

    L = nrg._lib
    dev = _open(nrg)
    model = VSpaceModel()
    rows = [(V0, 0x1000, 2 * KB4, M, 3),
            (V0 + 0x10, 0x1000, KB4, M, 3), (V0 + MB2, 0x1000, KB4, M, 0), (V0 + 2 * MB2, 0, GB1, D, 0),
            (V0 + 3 * MB2, 0x1001, KB4, M, 3), (V0 + 4 * MB2, 0x1000, KB4, 2, 3), (V0 + 5 * MB2, 0x1000, KB4, M, 9),
            ((1 << 48) - KB4, 0, 2 * KB4, M, 3), (1 << 48, 0, 0, M, 3),
            (V0 + 2 * KB4, 0x8000, KB4, D, 0)]
    recs = _recs(nrg, rows)
    a, b, s = model.replay(recs)
    assert s.tolist() == [1] + [0] * 8 + [1] and a[1:9].tolist() == [r[0] for r in rows[1:9]]
    first = dev.log_append(recs, 1)
    r = torch.full((len(rows), 2), -1, dtype=torch.int64, device="cuda")
    sm = torch.full((len(rows),), 7, dtype=torch.uint8, device="cuda")
    dev.log_exec_device(first, first + len(rows), r, sm)
    with pytest.raises(nrg.NrgError) as e:
        dev.sync()
    assert e.value.code == L.NRG_E_INVAL
    dev.sync()  # latched once
    np.testing.assert_array_equal(sm.cpu().numpy(), s)
    np.testing.assert_array_equal(_resp_of(r)[:, 0], a)
    np.testing.assert_array_equal(_resp_of(r)[:, 1], b)
    assert model.tables() == 4
    _check_state(dev, model, recs[[0, 9]])
    dev.close()


def test_vspace_log_wrap(nrg):
    """The minimum log (16384 entries) and 20 rounds of 1024 small ops on a 1 GiB window: the tail
    passes the ring's size, the head follows it (GC), and every round's answers are the model's."""
    dev = _open(nrg, log2_slots=10, max_batch=1024)
    model = VSpaceModel()
    rng = np.random.default_rng(5)
    base = 7 * SLOT4 + 3 * GB1
    every = []
    for rnd in range(20):
        recs = np.zeros(1024, nrg.VSPACE_OP_DTYPE)
        recs["vbase"] = np.uint64(base) + rng.integers(0, 1 << 18, 1024).astype(np.uint64) * np.uint64(KB4)
        recs["pbase"] = rng.integers(0, 1 << 36, 1024).astype(np.uint64) * np.uint64(KB4)
        recs["len"] = rng.integers(0, 5, 1024).astype(np.uint64) * np.uint64(KB4)
        recs["op"] = rng.integers(0, 2, 1024)
        recs["rights"] = rng.integers(1, 9, 1024)
        s = _exec(dev, model, recs)
        every.append(recs[::16])
        assert int(s.sum()) > 0
    st = dev.log_state()
    assert st["size"] == MIN_LOG_BYTES // 64 and st["tail"] == 20 * 1024 > st["size"] and st["head"] > 0
    _check_state(dev, model, np.concatenate(every))
    dev.sync()
    dev.close()


def test_vspace_group_members(nrg):
    """A two-member group over the loopback collectives: each member's responses for its own
    segment of the gathered log, and both members' final tables, are the model's replay of
    W_0 || W_1 round by round."""
    import torch

    L = nrg._lib
    lib = L.load()
    G = 2
    cfg = L.default_config(L.NRG_DS_VSPACE)
    cfg.max_batch, cfg.log2_slots, cfg.log_bytes = 64, 8, MIN_LOG_BYTES
    L.check(lib.nrg_test_loopback_collectives(1))
    g = C.c_void_p()
    try:
        L.check(lib.nrg_group_open((C.c_int * G)(*([0] * G)), G, C.byref(cfg), C.byref(g)), "nrg_group_open")
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))
    ctxs = [lib.nrg_group_replica(g, i) for i in range(G)]
    model = VSpaceModel()
    allrecs = _mix(nrg, 21, 200)
    outs, pos = [], 0
    for r, lens in enumerate([[30, 30], [0, 25], [17, 0], [0, 0], [40, 18], [20, 20]]):
        rd = (L.Round * G)()
        keep = []
        for i in range(G):
            n = lens[i]
            recs = allrecs[pos:pos + n]
            pos += n
            d_ops = _cuda_bytes(recs) if n else None
            resp = torch.full((max(n, 1), 2), -1, dtype=torch.int64, device="cuda")
            some = torch.full((max(n, 1),), 7, dtype=torch.uint8, device="cuda")
            rd[i].recs, rd[i].n = (d_ops.data_ptr() if n else 0), n
            rd[i].resp, rd[i].some = resp.data_ptr(), some.data_ptr()
            keep.append((d_ops, resp, some, n, model.replay(recs)))
        torch.cuda.synchronize()
        L.check(lib.nrg_group_round_async(g, rd, None), f"vspace group round {r}")
        outs.append(keep)
    L.check(lib.nrg_group_sync(g))
    for r, keep in enumerate(outs):
        for i, (_, resp, some, n, (a, b, s)) in enumerate(keep):
            if n:
                np.testing.assert_array_equal(some[:n].cpu().numpy(), s, err_msg=f"round {r} member {i} some")
                np.testing.assert_array_equal(_resp_of(resp[:n])[:, 0], a, err_msg=f"round {r} member {i} a")
                np.testing.assert_array_equal(_resp_of(resp[:n])[:, 1], b, err_msg=f"round {r} member {i} b")
    va, en = model.dump()
    for i, c in enumerate(ctxs):
        n = C.c_uint64()
        L.check(lib.nrg_vspace_tables(c, C.byref(n)))
        assert n.value == model.tables()
        assert lib.nrg_vspace_dump(c, None, 0, C.byref(n)) == L.NRG_E_CAPACITY and n.value == len(va)
        out = np.zeros(n.value, nrg.VSPACE_LEAF_DTYPE)
        m = C.c_uint64()
        L.check(lib.nrg_vspace_dump(c, out.ctypes.data_as(C.c_void_p), n.value, C.byref(m)))
        np.testing.assert_array_equal(out["vaddr"], va, err_msg=f"member {i}")
        np.testing.assert_array_equal(out["entry"], en, err_msg=f"member {i}")
    L.check(lib.nrg_group_close(g))


def test_vspace_has_no_combiner(nrg):
    L = nrg._lib
    dev = _open(nrg)
    out = C.c_void_p()
    assert L.load().nrg_combiner_open(dev.handle, 1, C.byref(out)) == L.NRG_E_INVAL
    assert not out.value
    dev.close()


def test_vspace_reads_need_a_synced_replica(nrg):
    L = nrg._lib
    dev = _open(nrg, max_reads=8)
    dev.log_append(_recs(nrg, [(V0, 0x1000, KB4, M, 3)]), 1)
    buf = np.zeros(16, np.uint64)
    f = np.zeros(16, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert dev._lib.nrg_vspace_resolve(dev.handle, p, 1, p, f.ctypes.data_as(C.c_void_p)) == L.NRG_E_NOT_SYNCED
    dev.log_exec()
    assert dev.vs_resolve([V0 + 5])[0].tolist() == [0x1005]
    assert dev._lib.nrg_vspace_resolve(dev.handle, p, 9, p, f.ctypes.data_as(C.c_void_p)) == L.NRG_E_CAPACITY
    dev.close()


def test_vspace_python_api(nrg):
    """Log + two Replica(VSpace): execute_mut(Map / MapDevice) on one, execute(Identify) on the
    other after it synced; verify sees equal leaves on both."""
    from nrgpu import Identify, Log, Map, MapDevice, Replica, VSpace

    log = Log(MIN_LOG_BYTES)
    r1 = Replica(log, VSpace, 0, max_batch=64, log2_slots=6)
    r2 = Replica(log, VSpace, 0, max_batch=64, log2_slots=6)
    t1, t2 = r1.register(), r2.register()
    assert r1.execute_mut(Map(V0, 2 * KB4, 3, 0x5000), t1) == ("ok", 0x5000, 2 * KB4)
    assert r1.execute_mut_batch([MapDevice(V0 + MB2, 0x9000, KB4), Map(V0 + KB4, KB4, 1, 0)], t1) == \
        [("ok", 0, 0), ("err", V0 + KB4)]
    assert r1.execute(Identify(V0 + KB4 + 7), t1) == 0x6007
    r2.sync(t2)
    assert r2.execute(Identify(V0 + MB2), t2) == 0x9000 and r2.execute(Identify(V0 + 2 * KB4), t2) == 0
    seen = []
    r1.verify(lambda v: seen.append(v))
    r2.verify(lambda v: seen.append(v))
    assert seen[0] == seen[1] and [x[0] for x in seen[0]] == [V0, V0 + KB4, V0 + MB2]


# ---- open / close, after tests/test_gpu_open_config.py ---------------------------------------
SMALLEST = dict(log_bytes=MIN_LOG_BYTES, max_batch=64, log2_slots=2)


def test_vspace_smallest_config_opens_answers_and_closes(nrg):
    """A pool of four tables, 64-op chunks and a log of the minimum size: open, one 16-op round on
    one granule against the model, close; then the same again."""
    rng = np.random.default_rng(3)
    rows = [(V0 + int(rng.integers(0, 24)) * KB4, int(rng.integers(0, 1 << 30)) * KB4, int(rng.integers(0, 4)) * KB4,
             int(rng.integers(0, 2)), int(rng.integers(1, 9))) for _ in range(16)]
    for _ in range(2):
        dev = _open(nrg, **SMALLEST)
        st = dev.log_state()
        assert st["size"] == MIN_LOG_BYTES // 64 and st["ds_kind"] == nrg._lib.NRG_DS_VSPACE
        model = VSpaceModel()
        recs = _recs(nrg, rows)
        s = _exec(dev, model, recs)
        assert 0 < int(s.sum()) < 16 and model.tables() == 4
        _check_state(dev, model, recs)
        dev.sync()
        assert dev._lib.nrg_close(dev._h) == nrg._lib.NRG_OK
        dev._h = None


@pytest.mark.parametrize("bad", [dict(log2_slots=1), dict(log2_slots=23), dict(max_batch=(1 << 16) + 1)],
                         ids=lambda v: ",".join(f"{k}={x}" for k, x in v.items()))
def test_vspace_rejected_config_is_invalid(nrg, bad):
    L = nrg._lib
    cfg = L.default_config(L.NRG_DS_VSPACE)
    for k, v in dict(SMALLEST, **bad).items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    assert L.load().nrg_open(0, C.byref(cfg), C.byref(h)) == L.NRG_E_INVAL
    assert not h.value
    _open(nrg, **SMALLEST).close()


def test_vspace_zero_max_batch_takes_the_default(nrg):
    """max_batch = 0 means the kind's default, 2^16 here, as it means 2^20 for the other kinds"""
    dev = _open(nrg, log2_slots=6, max_batch=0)
    model = VSpaceModel()
    recs = _recs(nrg, [(V0, 0x1000, 2 * KB4, M, 3), (V0 + KB4, 0x9000, KB4, D, 0)])
    assert _exec(dev, model, recs).tolist() == [1, 0]
    _check_state(dev, model, recs)
    dev.close()
