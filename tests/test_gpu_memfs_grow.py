"""Capacity growth of the file store (include/nrgpu.h "File store: capacity growth": nrg_set_max_capacity
in bytes per file, nrg_memfs_reserve) bit-exact against the sequential model of tests/memfs_grow_model.py.

Every named stream is replayed three ways: as one fused round, in fused rounds of 3 records, and by a
replica that is given the whole log in its ring and follows it (nrg_log_exec in chunks of its own
max_batch, then nrg_sync). Each is compared with the model on responses, some, dumps, sizes, every stored
byte, geometry and digest, and the three must agree on geometry and digest: the capacity is a pure
function of the log prefix, not of its chunks. Then the gates (no bound, B == max: none of the growth
kernels is launched), the entry points' checks, pwrite, snapshots, and groups over the loopback
collectives. F <= 5 and B from 128 bytes; tests/test_memfs_grow_cpu.py checks the streams on the CPU."""
import copy
import ctypes as C

import numpy as np
import pytest

import memfs_grow_model as GM
import memfs_model as M
from memfs_model import EFBIG, G, R, W
from memfs_size_model import S

pytestmark = pytest.mark.gpu

MIN_LOG_BYTES = 2 * 32 * 256 * 64  # Log::new's floor: 16384 entries
GROW_KERNELS = ("mf_need", "mf_room", "mf_grow")


class _Seed:
    """What a stream's seed() calls, on a device replica."""

    def __init__(self, dev):
        self.dev = dev

    def init(self, ino, data):
        self.dev.mf_init(ino, data)

    def truncate(self, ino, size):
        self.dev.mf_truncate(ino, size)


def _open(nrg, files, log2_b, bound=0, max_batch=64, sized=True, seed=None, timing=False):
    dev = nrg.DeviceReplica(nrg._lib.NRG_DS_MEMFS, 0, log2_slots=log2_b, queue_capacity=files,
                            log_bytes=max(MIN_LOG_BYTES, 4 * max_batch * 64), max_batch=max_batch)
    if sized:
        dev.mf_enable_sizes()
    if seed:
        seed(_Seed(dev))
    if bound:
        dev.set_max_capacity(bound)
    if timing:
        dev.kernel_timing(True)
    return dev


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _bad(recs):
    return bool(((recs["op"] > 3) | (recs["len"] > 128)).any())


def _round(nrg, dev, recs):
    """One fused round on device buffers: (resp, some). nrg_sync afterwards answers NRG_E_INVAL exactly
    when the round held a record outside the domain."""
    import torch

    L = nrg._lib
    n = len(recs)
    d_ops = _cuda(recs)
    d_resp = torch.full((max(n, 1) * 136,), 0xEE, dtype=torch.uint8, device="cuda")
    d_some = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    dev.mf_round(d_ops, n, 1, d_resp, d_some)
    assert dev._lib.nrg_sync(dev._h) == (L.NRG_E_INVAL if _bad(recs) else L.NRG_OK)
    torch.cuda.synchronize()
    return d_resp.cpu().numpy().view(nrg.MEMFS_RESP_DTYPE)[:n], d_some.cpu().numpy()[:n]


def _same_resp(resp, some, want, what=""):
    wresp, wsome = want
    np.testing.assert_array_equal(some, wsome, err_msg=what + " some")
    np.testing.assert_array_equal(resp["n"], wresp["n"], err_msg=what + " n")
    np.testing.assert_array_equal(resp["data"], wresp["data"], err_msg=what + " data")


def _same_state(nrg, dev, model, what=""):
    """Geometry, sizes, dumps, every stored byte (the snapshot's payload) and the digest."""
    assert dev.mf_geometry() == (model.files, model.B), what
    for f in range(model.files):
        assert dev.mf_size(M.FIRST_INO + f) == model.size[f], f"{what} size of file {f}"
        assert dev.mf_dump(M.FIRST_INO + f) == model.dump(M.FIRST_INO + f), f"{what} file {f}"
    info, data = nrg.snapshot.unpack(dev.snapshot())
    assert info.items == model.files * model.B // 8 + model.files
    raw, sizes = nrg.snapshot.memfs_split(data, model.files)
    assert raw.shape == (model.files, model.B) and raw.tobytes() == model.raw(), f"{what} stored bytes"
    assert sizes.tolist() == model.size
    dg = dev.digest()
    assert dg == info.digest == nrg.digest.memfs([bytes(d) for d in model.data], model.size), what
    if model.B <= 4096:
        assert dg == model.digest(), what
    return dg


# ---- every named stream, three ways ---------------------------------------------------------------------------
@pytest.mark.parametrize("s", GM.all_streams(), ids=lambda s: s.name)
def test_stream_three_ways(nrg, s):
    L = nrg._lib
    model, want = GM.expected(s)
    n = len(s.recs)
    # one fused round
    a = _open(nrg, s.files, s.log2_b, s.bound, seed=s.seed)
    resp, some = _round(nrg, a, s.recs)
    _same_resp(resp, some, want, "fused")
    da = _same_state(nrg, a, model, "fused")
    # fused rounds of 3 records
    b = _open(nrg, s.files, s.log2_b, s.bound, seed=s.seed)
    parts = [_round(nrg, b, s.recs[i:i + 3]) for i in range(0, n, 3)]
    _same_resp(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), want, "chunks of 3")
    db = _same_state(nrg, b, model, "chunks of 3")
    # a follower: the whole log in its ring, replayed in chunks of its own max_batch
    c = _open(nrg, s.files, s.log2_b, s.bound, max_batch=16 if n > 16 else 5, seed=s.seed)
    first = c.log_append(s.recs, 2)
    rc, resp, some = c.log_exec_rc(first, first + n)
    assert rc == (L.NRG_E_INVAL if _bad(s.recs) else L.NRG_OK)
    c.sync()
    _same_resp(resp, some, want, "follower")
    dc = _same_state(nrg, c, model, "follower")
    assert da == db == dc and a.mf_geometry() == b.mf_geometry() == c.mf_geometry() == (s.files, s.end_b)
    for d in (a, b, c):
        d.close()


def test_append_equals_a_store_opened_large(nrg):
    """The appended file is, in dump and digest, the file of a context opened at log2_slots = 12 and given
    the same truncate and Writes."""
    s = GM.append()
    grown = _open(nrg, 1, 7, 4096, seed=s.seed, timing=True)
    large = _open(nrg, 1, 12, seed=s.seed)
    for d in (grown, large):
        _round(nrg, d, s.recs)
    assert grown.mf_geometry() == large.mf_geometry() == (1, 4096)
    assert grown.mf_dump(5) == large.mf_dump(5) == b"".join(r["data"].tobytes() for r in s.recs)
    assert grown.digest() == large.digest()
    assert grown.kernel_time("mf_grow")[0] == 1  # one fused round: the chunk's whole need at once
    assert grown.kernel_time("mf_need")[0] == 1 and grown.kernel_time("mf_room")[0] == 1
    grown.close()
    large.close()


def test_refused_records_grow_nothing(nrg):
    """edges: after the records up to the first admitted end at max, B is what the one admitted Write
    before them gives (512), however large the refused records' offsets were."""
    s = GM.edges()
    dev = _open(nrg, s.files, s.log2_b, s.bound, timing=True)
    half = GM.GrowModel(s.files, s.log2_b, s.bound)
    want = half.replay(s.recs[:s.mid])
    resp, some = _round(nrg, dev, s.recs[:s.mid])
    _same_resp(resp, some, want)
    assert dev.mf_geometry() == (2, 512) and dev.kernel_time("mf_grow")[0] == 1
    _same_state(nrg, dev, half)
    dev.close()


# ---- the gates ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", [0, 256], ids=["no_bound", "B_equals_max"])
def test_a_fixed_store_launches_nothing_of_growth(nrg, bound):
    """Without a bound, and at B == max, the EFBIG answers are today's and none of mf_need, mf_room and
    mf_grow is launched or read."""
    import memfs_size_model as Z

    recs = np.concatenate([W(5, 200, b"\x07" * 56), W(5, 200, b"\x07" * 57), S(6, 256), S(6, 257), W(6, 256, b""),
                           W(6, 257, b""), S(5, 1 << 40), W(7, (1 << 64) - 1, b"\x09"), G(5), R(5, 192, 128)])
    model = Z.SizedModel(3, 8)
    want = model.replay(recs)
    assert want[0]["n"].tolist()[:8] == [56, EFBIG, 256, EFBIG, 0, EFBIG, EFBIG, EFBIG]
    dev = _open(nrg, 3, 8, bound, timing=True)
    for _ in range(2):
        resp, some = _round(nrg, dev, recs)
        _same_resp(resp, some, want)
    first = dev.log_append(recs, 1)
    resp, some = dev.log_exec(first, first + len(recs))
    _same_resp(resp, some, want)
    assert dev.mf_geometry() == (3, 256)
    for k in GROW_KERNELS:
        assert dev.kernel_time(k) == (0, 0.0), k
    assert dev.kernel_time("mfs_expand")[0] == 3  # (the timers do count)
    dev.close()


def test_below_the_bound_every_chunk_checks_its_need(nrg):
    recs = np.concatenate([W(5, 0, b"\x07" * 56), G(5)])
    dev = _open(nrg, 1, 8, 1024, timing=True)
    for _ in range(3):
        _round(nrg, dev, recs)
    assert dev.kernel_time("mf_need")[0] == 3 and dev.kernel_time("mf_room")[0] == 3 and dev.kernel_time("mf_grow")[0] == 0
    dev.set_max_capacity(0)  # growth off again: a fixed store
    _round(nrg, dev, recs)
    assert dev.kernel_time("mf_need")[0] == 3
    resp, some = _round(nrg, dev, W(5, 200, b"\x07" * 57))
    assert (int(resp["n"][0]), int(some[0])) == (EFBIG, 0) and dev.mf_geometry() == (1, 256)
    dev.close()


def test_the_bound_and_the_reserve_check_their_arguments(nrg):
    L = nrg._lib
    lib = L.load()
    dev = _open(nrg, 4, 8, sized=False)
    assert lib.nrg_set_max_capacity(dev._h, 1024) == L.NRG_E_INVAL, "sizes are required"
    assert lib.nrg_memfs_reserve(dev._h, 1024) == L.NRG_E_INVAL
    assert lib.nrg_memfs_reserve(dev._h, 256) == L.NRG_E_INVAL
    dev.mf_enable_sizes()
    for bad in (1000, 128, 1 << 27, 1 << 28, 3 << 20, (1 << 64) - 1):  # F * 2^28 > 2^29; 2^27 > 2^26
        assert lib.nrg_set_max_capacity(dev._h, bad) == L.NRG_E_INVAL, bad
    assert dev.mf_max_capacity() == 0
    for good in (256, 1 << 26, 1024, 0, 512):
        assert lib.nrg_set_max_capacity(dev._h, good) == L.NRG_OK, good
        assert dev.mf_max_capacity() == good
    first = dev.log_append(G(5), 1)
    assert lib.nrg_set_max_capacity(dev._h, 1024) == L.NRG_E_NOT_SYNCED
    dev.log_exec(first, first + 1)
    # the reserve: rounded up, never shrinks, nrg_open's limits, with or without a bound
    seed = bytes(range(1, 201))
    dev.mf_init(6, seed)
    dev.mf_truncate(6, 200)
    model = GM.GrowModel(4, 8, 512)
    model.init(6, seed)
    model.truncate(6, 200)
    dev.mf_reserve(100)
    dev.mf_reserve(256)
    assert dev.mf_geometry() == (4, 256)
    dev.mf_reserve(257)
    model.reserve(257)
    _same_state(nrg, dev, model, "reserved 257")
    dev.mf_reserve(2000)  # beyond its bound of 512: a fixed store of 2048 from here on
    model.reserve(2000)
    _same_state(nrg, dev, model, "reserved 2000")
    dev.kernel_timing(True)
    recs = np.concatenate([W(6, 1990, b"\x05" * 58), W(6, 1990, b"\x05" * 59), S(5, 2048), S(5, 2049), R(6, 1980, 128)])
    want = model.replay(recs)
    assert want[1].tolist() == [1, 0, 1, 0, 1]
    resp, some = _round(nrg, dev, recs)
    _same_resp(resp, some, want)
    _same_state(nrg, dev, model, "fixed at 2048")
    assert dev.kernel_time("mf_need")[0] == 0
    for bad in ((1 << 26) + 1, 1 << 28, (1 << 64) - 1):  # F * 2^28 > 2^29
        assert lib.nrg_memfs_reserve(dev._h, bad) == L.NRG_E_INVAL, bad
    assert dev.mf_geometry() == (4, 2048)
    st = nrg.DeviceReplica(L.NRG_DS_STACK, 0, log_bytes=MIN_LOG_BYTES, max_batch=64, stack_capacity=64)
    n = C.c_uint64()
    assert lib.nrg_memfs_reserve(st._h, 256) == L.NRG_E_INVAL and lib.nrg_memfs_max_capacity(st._h, C.byref(n)) == L.NRG_E_INVAL
    st.close()
    dev.close()


def test_truncate_grows_first_and_init_does_not(nrg):
    L = nrg._lib
    dev = _open(nrg, 2, 7, 1024)
    model = GM.GrowModel(2, 7, 1024)
    dev.mf_init(5, b"\x09" * 100)
    model.init(5, b"\x09" * 100)
    assert dev._lib.nrg_memfs_truncate(dev._h, 6, 1025) == L.NRG_E_INVAL
    big = np.full(129, 7, np.uint8)
    assert dev._lib.nrg_memfs_init(dev._h, 5, C.c_void_p(big.ctypes.data), 129) == L.NRG_E_INVAL
    assert dev.mf_geometry() == (2, 128)
    dev.mf_truncate(6, 600)
    model.truncate(6, 600)
    _same_state(nrg, dev, model, "truncated to 600")
    assert dev.mf_read(6, 100, 100) == b"\x01" * 28 + bytes(72) and dev.mf_read(5, 90, 100) == b"\x09" * 10 + b"\x01" * 28
    dev.close()


# ---- pwrite: the host knows the need ---------------------------------------------------------------------------
def test_pwrite_grows_once_from_its_plan(nrg):
    L = nrg._lib
    mx = 1 << 20
    rng = np.random.default_rng(21)
    data = rng.integers(1, 256, mx, dtype=np.uint8)
    dev = _open(nrg, 1, 12, mx, max_batch=8192, timing=True)
    # a request that ends at max + 1 fails whole and grows nothing
    written, some, t = dev.mf_pwrite([[5, 1, mx, 0]], data)
    assert (written.tolist(), some.tolist(), t) == ([EFBIG], [0], 1) and dev.mf_geometry() == (1, 4096)
    assert dev.kernel_time("mf_grow")[0] == 0
    written, some, t = dev.mf_pwrite([[5, 0, mx, 0]], data)
    assert (written.tolist(), some.tolist(), t) == ([mx], [1], mx // 128)
    assert dev.mf_geometry() == (1, mx) and dev.mf_size(5) == mx
    assert dev.kernel_time("mf_grow")[0] == 1 and dev.kernel_time("mf_need")[0] == 0 and dev.kernel_time("mf_room")[0] == 0
    # reads across the old end
    assert dev.mf_read(5, 4000, 300) == data[4000:4300].tobytes()
    reqs = np.zeros(2, nrg.MEMFS_RD_DTYPE)
    reqs["ino"], reqs["offset"], reqs["len"] = [5, 5], [4090, mx - 10], [20000, 100]
    got, offs, sm = dev.mf_pread(reqs)
    got, offs = got.cpu().numpy(), offs.cpu().numpy()
    assert offs.tolist() == [0, 20000, 20010] and sm.cpu().numpy().tolist() == [1, 1]
    assert got[:20000].tobytes() == data[4090:24090].tobytes() and got[20000:].tobytes() == data[mx - 10:].tobytes()
    assert dev.digest() == nrg.digest.memfs([data.tobytes()], [mx])
    # the cut alone decides EFBIG against the bound and grows nothing
    small = _open(nrg, 1, 7, 1024)
    recs = small.mf_pwrite_records([[5, 100, 300, 0], [5, 1000, 25, 0]], data[:400])
    assert small.mf_geometry() == (1, 128) and len(recs) == 4 + 1
    assert recs["offset"].tolist() == [100, 128, 256, 384, 1024] and recs["len"].tolist() == [28, 128, 128, 16, 1]
    model = GM.GrowModel(1, 7, 1024)
    want = model.replay(recs)
    assert want[1].tolist() == [1, 1, 1, 1, 0]
    resp, sm = _round(nrg, small, recs)  # the replay of the records grows
    _same_resp(resp, sm, want)
    _same_state(nrg, small, model)
    small.close()
    dev.close()


def test_replica_api_pwrite_grows(nrg):
    log = nrg.Log(MIN_LOG_BYTES)
    a = nrg.Replica(log, nrg.MemFs, max_batch=64, log2_slots=7, queue_capacity=1)
    t = a.register()
    a.dev.mf_enable_sizes()
    a.dev.set_max_capacity(1024)
    blob = bytes(range(1, 201)) * 3
    assert a.execute_mut(nrg.MfPwrite(5, 100, blob), t) == ("written", 600)
    assert a.dev.mf_geometry() == (1, 1024) and a.dev.mf_size(5) == 700
    assert a.execute_mut(nrg.MfPwrite(5, 425, blob), t) == ("err", nrg._lib.NRG_MEMFS_EFBIG)
    assert a.execute_mut(nrg.MfPwrite(5, 424, blob), t) == ("written", 600)
    assert a.execute_mut(nrg.MfRead(5, 1000, 64), t) == ("data", blob[576:600])
    assert a.execute_mut(nrg.MfSetAttr(5, 1025), t) == ("err", nrg._lib.NRG_MEMFS_EFBIG)
    assert a.dev.mf_dump(5) == b"\x01" * 100 + blob[:324] + blob
    a.dev.close()


def test_replica_cloned_from_a_grown_peer(nrg):
    """Replica(..., clone_from=peer): the clone takes the peer's bound first, so the grown image goes into a
    replica opened at the original B; both then go on growing from the same log."""
    log = nrg.Log(MIN_LOG_BYTES)
    cfg = dict(max_batch=64, log2_slots=7, queue_capacity=2)
    a = nrg.Replica(log, nrg.MemFs, **cfg)
    t = a.register()
    a.dev.mf_enable_sizes()
    a.dev.set_max_capacity(2048)
    assert a.execute_mut(nrg.MfWrite(6, 500, b"\x07" * 100), t) == ("written", 100)
    assert a.dev.mf_geometry() == (2, 1024)
    b = nrg.Replica(log, nrg.MemFs, clone_from=a, **cfg)
    assert b.dev.mf_geometry() == (2, 1024) and b.dev.mf_max_capacity() == 2048 and b.digest() == a.digest()
    assert a.execute_mut(nrg.MfSetAttr(5, 1500), t) == ("attr", 1500)
    assert b.digest() == a.digest() and b.dev.mf_geometry() == a.dev.mf_geometry() == (2, 2048)
    assert b.dev.mf_size(5) == 1500 and b.dev.mf_dump(6) == b"\x01" * 128 + bytes(372) + b"\x07" * 100
    a.dev.close()
    b.dev.close()


# ---- snapshots ------------------------------------------------------------------------------------------------
def test_snapshot_of_a_grown_store(nrg):
    L = nrg._lib
    s = GM.stride()
    model = copy.deepcopy(GM.expected(s)[0])  # (it is replayed further below: the shared one stays as it is)
    src = _open(nrg, s.files, s.log2_b, s.bound, seed=s.seed)
    _round(nrg, src, s.recs)
    img = src.snapshot()
    assert nrg.snapshot.header(img).items == 3 * 1024 // 8 + 3
    # into a fresh context of the original B with the bound set
    dst = _open(nrg, s.files, s.log2_b, s.bound)
    dst.restore(img)
    _same_state(nrg, dst, model, "restored")
    assert dst.digest() == src.digest() and dst.log_state()["ltail"] == len(s.recs)
    more = np.concatenate([W(7, 1500, b"\x0b" * 100), R(5, 0, 128), G(7)])
    want = model.replay(more)
    for d in (src, dst):
        resp, some = _round(nrg, d, more)
        _same_resp(resp, some, want)
        _same_state(nrg, d, model, "after restore")
    # without a bound, or with one below the image's B: refused with nothing touched
    for bound in (0, 512):
        plain = _open(nrg, s.files, s.log2_b, bound)
        plain.mf_init(6, b"\x07" * 50)
        before = plain.digest()
        with pytest.raises(nrg.NrgError) as e:
            plain.restore(img)
        assert e.value.code == L.NRG_E_INVAL
        assert plain.digest() == before and plain.mf_geometry() == (3, 256) and plain.log_state()["ltail"] == 0
        plain.close()
    # a smaller image into the grown store: it never shrinks
    little = _open(nrg, s.files, s.log2_b)
    with pytest.raises(nrg.NrgError) as e:
        src.restore(little.snapshot())
    assert e.value.code == L.NRG_E_INVAL and src.mf_geometry() == (3, 2048)
    _same_state(nrg, src, model, "refused a smaller image")
    for d in (src, dst, little):
        d.close()


# ---- groups over the loopback collectives -----------------------------------------------------------------------
def _group(nrg, files, log2_b, bound):
    L = nrg._lib
    lib = L.load()
    cfg = L.default_config(L.NRG_DS_MEMFS)
    cfg.log_bytes, cfg.max_batch, cfg.log2_slots, cfg.queue_capacity = MIN_LOG_BYTES, 64, log2_b, files
    L.check(lib.nrg_test_loopback_collectives(1))
    g = C.c_void_p()
    try:
        L.check(lib.nrg_group_open((C.c_int * 2)(0, 0), 2, C.byref(cfg), C.byref(g)), "nrg_group_open")
    finally:
        L.check(lib.nrg_test_loopback_collectives(0))
    hs = [lib.nrg_group_replica(g, i) for i in range(2)]
    for h in hs:
        L.check(lib.nrg_memfs_enable_sizes(h))
        if bound:
            L.check(lib.nrg_set_max_capacity(h, bound))
    return g, hs


def _verify(nrg, g):
    L = nrg._lib
    out = np.zeros((2, 3), np.uint64)
    same = C.c_int(-1)
    assert L.load().nrg_group_verify(g, out.ctypes.data_as(C.c_void_p), C.byref(same)) == L.NRG_OK
    return same.value, [tuple(int(v) for v in row) for row in out]


def _geometry(nrg, h):
    f, b = C.c_uint64(), C.c_uint64()
    assert nrg._lib.load().nrg_memfs_geometry(h, C.byref(f), C.byref(b)) == nrg._lib.NRG_OK
    return f.value, b.value


def _replicated_round(nrg, g, segs, wants):
    import torch

    L = nrg._lib
    lib = L.load()
    rd = (L.Round * 2)()
    got, keep = [], []
    for i, recs in enumerate(segs):
        n = len(recs)
        d_ops = _cuda(recs) if n else None
        d_resp = torch.full((max(n, 1) * 136,), 0xEE, dtype=torch.uint8, device="cuda")
        d_some = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
        rd[i].recs, rd[i].n = (d_ops.data_ptr() if n else 0), n
        rd[i].resp, rd[i].some = d_resp.data_ptr(), d_some.data_ptr()
        got.append((d_resp, d_some))
        keep.append(d_ops)
    torch.cuda.synchronize()
    L.check(lib.nrg_group_round_async(g, rd, None), "round")
    L.check(lib.nrg_group_sync(g), "sync")
    torch.cuda.synchronize()
    for i, recs in enumerate(segs):
        n = len(recs)
        _same_resp(got[i][0].cpu().numpy().view(nrg.MEMFS_RESP_DTYPE)[:n], got[i][1].cpu().numpy()[:n], wants[i], f"member {i}")


def test_replicated_group_grows_together_and_resyncs_a_member_left_behind(nrg):
    import torch

    L = nrg._lib
    lib = L.load()
    g, hs = _group(nrg, 3, 8, 2048)
    model = GM.GrowModel(3, 8, 2048)
    segs = [np.concatenate([W(6, 700, b"\x05" * 100), R(6, 672, 128), G(6)]),
            np.concatenate([S(7, 1000), R(7, 900, 128), W(5, 250, b"\x06" * 12), G(5)])]
    _replicated_round(nrg, g, segs, [model.replay(x) for x in segs])  # in rank order: W_0 || W_1
    assert model.B == 1024 and [_geometry(nrg, h) for h in hs] == [(3, 1024)] * 2
    same, rows = _verify(nrg, g)
    assert same == 1 and rows == [nrg.digest.memfs([bytes(d) for d in model.data], model.size)] * 2
    # member 0 alone goes on and grows: member 1 is behind, in state and in capacity
    ahead = np.concatenate([W(5, 1900, b"\x08" * 100), S(6, 10)])
    d_ops = _cuda(ahead)
    torch.cuda.synchronize()
    assert lib.nrg_memfs_round_async(hs[0], d_ops.data_ptr(), len(ahead), 1, None, None) == L.NRG_OK
    assert lib.nrg_sync(hs[0]) == L.NRG_OK
    model.replay(ahead)
    assert [_geometry(nrg, h) for h in hs] == [(3, 2048), (3, 1024)] and _verify(nrg, g)[0] == 0
    assert lib.nrg_group_resync(g, 0) == L.NRG_OK
    same, rows = _verify(nrg, g)
    assert same == 1 and rows == [nrg.digest.memfs([bytes(d) for d in model.data], model.size)] * 2
    assert [_geometry(nrg, h) for h in hs] == [(3, 2048)] * 2
    assert lib.nrg_group_close(g) == L.NRG_OK


def test_file_partitioned_group_refuses_a_bound_and_grows_by_reserve(nrg):
    from test_gpu_memfs_group_pread import _pread
    from test_gpu_memfs_partitioned import _dump, _round as _file_round, _same_resp as _same_file_resp, _untouched

    L = nrg._lib
    lib = L.load()
    g, hs = _group(nrg, 2, 8, 1024)
    try:
        # file 0 (ino 5) is rank 0's, file 1 (ino 6) rank 1's; each rank writes the other's file past the old B
        segs = [np.concatenate([W(6, 300, b"\x05" * 100), R(6, 272, 128), G(6), S(5, 900)]),
                np.concatenate([W(5, 500, b"\x06" * 128), R(5, 450, 128), G(5)])]
        before = _verify(nrg, g)[1]
        bufs = _file_round(nrg, g, segs, want_rc=L.NRG_E_INVAL)  # a bound on a member: every rank the same code
        _untouched(bufs, "a round with a bound set")
        rq = np.zeros(1, nrg.MEMFS_RD_DTYPE)
        rq["ino"], rq["len"] = 5, 16
        _pread(nrg, g, [rq, rq], [16, 16], want_rc=L.NRG_E_INVAL)
        assert _verify(nrg, g)[1] == before and [_geometry(nrg, h) for h in hs] == [(2, 256)] * 2
        # one member still bound: still refused
        assert lib.nrg_set_max_capacity(hs[0], 0) == L.NRG_OK
        _untouched(_file_round(nrg, g, segs, want_rc=L.NRG_E_INVAL), "one member bound")
        assert lib.nrg_set_max_capacity(hs[1], 0) == L.NRG_OK
        for h in hs:
            assert lib.nrg_memfs_reserve(h, 1000) == L.NRG_OK
        assert [_geometry(nrg, h) for h in hs] == [(2, 1024)] * 2
        # the replicated model for the answers (rank order), then each file on its owner
        model = GM.GrowModel(2, 8)
        model.reserve(1000)
        want = [model.replay(x) for x in segs]
        bufs = _file_round(nrg, g, segs)
        for r, (d_resp, d_some) in enumerate(bufs):
            _same_file_resp(nrg, d_resp, d_some, want[r], f"rank {r}")
        assert model.size == [900, 400]
        for f in range(2):
            assert _dump(nrg, hs[f], 5 + f, 1024) == model.dump(5 + f), f"file {f} on its owner"
        # the group-wide pread across the old end, asked by the rank that does not own the file
        rqs = []
        for ino in (6, 5):
            rq = np.zeros(2, nrg.MEMFS_RD_DTYPE)
            rq["ino"], rq["offset"], rq["len"] = ino, [200, 0], [400, 4096]
            rqs.append(rq)
        out = _pread(nrg, g, rqs, [2000, 2000])
        for r, ino in enumerate((6, 5)):
            d_data, d_offs, d_some = out[r]
            full = model.dump(ino)
            expect = full[200:600] + full
            offs = d_offs.cpu().numpy().view(np.uint64)[:3].tolist()
            assert offs == [0, len(full[200:600]), len(expect)] and d_some.cpu().numpy()[:2].tolist() == [1, 1]
            assert d_data.cpu().numpy()[:len(expect)].tobytes() == expect, f"rank {r}"
    finally:
        assert lib.nrg_group_close(g) == L.NRG_OK


def test_python_file_partitioned_group_reserve(nrg):
    """nrgpu.FilePartitionedGroup on a one-rank group: a round with a bound set is refused, and after
    FilePartitionedGroup.reserve a round past the old B answers as the model does."""
    import torch
    from nrgpu.parallel import ReplicaGroup

    L = nrg._lib
    lib = L.load()
    rep = _open(nrg, 2, 8, 1024)
    recs = np.concatenate([W(6, 300, b"\x05" * 100), R(6, 272, 128), G(6), S(5, 900), G(5)])
    model = GM.GrowModel(2, 8)
    L.check(lib.nrg_test_loopback_collectives(1))
    grp = None
    try:
        grp = nrg.FilePartitionedGroup(rep, 0, 1, uid=ReplicaGroup.unique_id(), timeout_ms=20000)
        d_ops = _cuda(recs)
        d_resp = torch.full((len(recs) * 136,), 0xEE, dtype=torch.uint8, device="cuda")
        d_some = torch.full((len(recs),), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(nrg.NrgError) as e:
            grp.round(d_ops, len(recs), d_resp, d_some)
        assert e.value.code == L.NRG_E_INVAL and (d_some.cpu().numpy() == 0xEE).all()
        rep.set_max_capacity(0)
        grp.reserve(1000)
        model.reserve(1000)
        assert rep.mf_geometry() == (2, 1024)
        grp.round(d_ops, len(recs), d_resp, d_some)
        grp.sync()
        torch.cuda.synchronize()
        _same_resp(d_resp.cpu().numpy().view(nrg.MEMFS_RESP_DTYPE), d_some.cpu().numpy(), model.replay(recs))
        _same_state(nrg, rep, model, "after the round")
    finally:
        if grp is not None:
            grp.close()
        rep.close()
        L.check(lib.nrg_test_loopback_collectives(0))
