"""The page-table replay (vspace.hip) at real chunk sizes: the named streams of tests/vspace_streams.py,
one chunk each (max_batch = n), against the sequential model of tests/vspace_model.py, or against the
capped sequential replay where the pool runs out.

Every case compares, bit for bit: each response (a, b, some); the number of tables; the full leaf
dump; nrg_digest against nrgpu.digest.vspace of the model's leaves; Identify of a seeded sample of at
most 4096 addresses (the probes of the chunk's first 32, last 32 and 64 random ops); and it checks
the structure of the device's pool image (every table referenced exactly once: two entries numbered
onto one table show here before their leaves collide). vs_seq is launched ceil(n / 4096) times a
chunk. Which path a chunk took (parallel or the sequential fallback) cannot be seen from here: the
answers are the same. tests/test_vspace_streams_cpu.py pins it per stream through the plan model.
"""
import ctypes as C

import numpy as np
import pytest

import vspace_streams as S
from nrgpu import NrgError, digest, snapshot
from test_gpu_vspace import MIN_LOG_BYTES, _cuda_bytes, _probes, _resp_of
from vspace_model import VSpaceModel

pytestmark = pytest.mark.gpu


def _open(nrg, log2, max_batch, total):
    entries = max(MIN_LOG_BYTES // 64, 1 << int(2 * total).bit_length())
    return nrg.DeviceReplica(nrg._lib.NRG_DS_VSPACE, 0, log2_slots=log2, max_batch=max_batch, max_reads=4096,
                             log_bytes=64 * entries)


def _sample(recs, seed):
    rng = np.random.default_rng(seed)
    n = len(recs)
    pick = np.unique(np.concatenate([np.arange(min(32, n)), np.arange(max(0, n - 32), n),
                                     rng.integers(0, n, 64)]))
    probes = _probes(recs[pick])
    if len(probes) > 4096:  # (an op of 513 granules has that many boundaries of its own)
        probes = probes[np.sort(rng.choice(len(probes), 4096, replace=False))]
    return probes


def _check_state(dev, model, recs, seed):
    assert dev.vs_tables() == model.tables()
    d = dev.vs_dump()
    va, en = model.dump()
    np.testing.assert_array_equal(d["vaddr"], va)
    np.testing.assert_array_equal(d["entry"], en)
    assert dev.digest() == tuple(digest.vspace(va, en))
    info, tables = snapshot.unpack(dev.snapshot())
    assert info.items == model.tables()
    S.check_pool(tables, model.tables())
    probes = _sample(recs, seed)
    pa, found = dev.vs_resolve(probes)
    want = [model.resolve(int(x)) for x in probes]
    np.testing.assert_array_equal(pa, np.array([w[0] for w in want], np.uint64))
    np.testing.assert_array_equal(found, np.array([w[1] for w in want], np.uint8))


def _exec(dev, recs, want, error=None):
    """append + exec of `recs` with every response wanted; `error`: the code the chunk latches, once"""
    import torch

    a, b, s = want
    n = len(recs)
    first = dev.log_append(recs, 1)
    if error is None:
        resp, some = dev.log_exec(first, first + n)
        ra, rb = resp["a"], resp["b"]
    else:
        r = torch.full((n, 2), -1, dtype=torch.int64, device="cuda")
        sm = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        dev.log_exec_device(first, first + n, r, sm)
        with pytest.raises(NrgError) as e:
            dev.sync()
        assert e.value.code == error
        dev.sync()  # latched once: reported and cleared
        some, ra, rb = sm.cpu().numpy(), _resp_of(r)[:, 0], _resp_of(r)[:, 1]
    np.testing.assert_array_equal(some, s)
    np.testing.assert_array_equal(ra, a)
    np.testing.assert_array_equal(rb, b)


def _setup(nrg, name, n, max_batch=None):
    """the replica and the model after the stream's setup batches"""
    log2, setup, chunk = S.stream(name, n)
    dev = _open(nrg, log2, max_batch or n, sum(len(b) for b in setup) + n)
    model = VSpaceModel()
    for b in setup:
        _exec(dev, b, model.replay(b))
    return dev, model, log2, chunk


@pytest.mark.parametrize("name,n", S.CASES, ids=lambda v: str(v))
def test_vspace_stream(nrg, name, n):
    L = nrg._lib
    dev, model, log2, chunk = _setup(nrg, name, n)
    a, b, s, left = S.replay_capped(model, chunk, 1 << log2)
    error = None
    if name == "overflow":
        assert left
        error = L.NRG_E_CAPACITY
    else:
        assert not left
        if name == "edges_inval":
            error = L.NRG_E_INVAL
    dev.kernel_timing(True, only="vs_seq")
    _exec(dev, chunk, (a, b, s), error)
    assert dev.kernel_time("vs_seq")[0] == -(-n // S.VS_SEQ_SLICE)
    dev.kernel_timing(False)
    _check_state(dev, model, chunk, seed=n)
    dev.sync()  # nothing (else) latched
    dev.close()


def test_vspace_octets_through_the_fused_round(nrg):
    """octets at 4097 through nrg_vspace_round_async: vs_prep writes the log copy"""
    import torch

    n = 4097
    dev, model, log2, chunk = _setup(nrg, "octets", n)
    a, b, s = model.replay(chunk)
    d_ops = _cuda_bytes(chunk)
    r = torch.full((n, 2), -1, dtype=torch.int64, device="cuda")
    sm = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    dev.vs_round_device(d_ops, n, 1, r, sm)
    dev.sync()
    np.testing.assert_array_equal(sm.cpu().numpy(), s)
    np.testing.assert_array_equal(_resp_of(r)[:, 0], a)
    np.testing.assert_array_equal(_resp_of(r)[:, 1], b)
    _check_state(dev, model, chunk, seed=1)
    st = dev.log_state()
    assert (st["tail"], st["ltail"]) == (n, n)
    rec = np.zeros(1, nrg.VSPACE_OP_DTYPE)
    nrg._lib.check(nrg._lib.load().nrg_test_ring_read(dev.handle, (n - 1) & (st["size"] - 1),
                                                       rec.ctypes.data_as(C.c_void_p)))
    assert rec[0] == chunk[n - 1]
    dev.close()


def test_vspace_far_dep_in_five_chunks(nrg):
    """far_dep at 4097 appended once and replayed 1000 ops a chunk, responses for [900, 3100): the
    window's answers and the final state are those of one chunk"""
    n = 4097
    dev, model, log2, chunk = _setup(nrg, "far_dep", n, max_batch=1000)
    a, b, s = model.replay(chunk)
    first = dev.log_append(chunk, 1)
    resp, some = dev.log_exec(first + 900, first + 3100)
    np.testing.assert_array_equal(some, s[900:3100])
    np.testing.assert_array_equal(resp["a"], a[900:3100])
    np.testing.assert_array_equal(resp["b"], b[900:3100])
    _check_state(dev, model, chunk, seed=2)
    dev.close()


def test_vspace_independent_after_reserve_and_after_restore(nrg):
    """independent at 2049 in a pool opened with 2^4 tables and grown to 2^13 (vs_reserve): the first
    1024 ops, a snapshot, and a fresh replica that restores it; both replay the other 1025 ops as
    one chunk and both equal the model"""
    n, half = 2049, 1024
    log2, setup, chunk = S.stream("independent", n)
    assert not setup
    model = VSpaceModel()
    dev = _open(nrg, 4, n, n)
    dev.vs_reserve(1 << 13)
    assert dev.vs_capacity() == 1 << 13
    _exec(dev, chunk[:half], model.replay(chunk[:half]))
    assert model.tables() > 1 << 4
    _check_state(dev, model, chunk[:half], seed=3)
    img = dev.snapshot()
    fresh = _open(nrg, 13, n, n)
    fresh.restore(img)
    assert fresh.log_state()["tail"] == half
    want = model.replay(chunk[half:])
    for d in (dev, fresh):
        _exec(d, chunk[half:], want)
        _check_state(d, model, chunk, seed=4)
        d.close()
