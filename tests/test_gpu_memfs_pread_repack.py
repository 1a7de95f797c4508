"""The two kernels a group-wide pread adds, each on one plain replica (csrc/partition.hip, csrc/memfs.hip):
nrg_memfs_rd_partition_async against numpy's stable partition, and nrg_memfs_pread_repack_async (the copy
kernel of nrg_memfs_pread_async reading a packed source) against the model, with the source built on the
CPU in partition order. Every output buffer is longer than it need be and filled with a sentinel: nothing
past n requests, and no data byte at or past min(cap, total), may change."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import memfs_group_pread_model as GM
import memfs_model as M
import memfs_part_streams as PS
import memfs_pread_model as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = int(re.search(r"#define NRG_MF_PREAD_TILE (\d+)u", open(os.path.join(ROOT, "include", "nrgpu_testing.h")).read()).group(1))
MIN_LOG_BYTES = 2 * 32 * 256 * 64
SIZES = (0, 1, 255, 256, 257, 513, 1000)
PARTS = (1, 2, 3, 8, 64)


@pytest.fixture(scope="module")
def dev(nrg):
    assert nrg._lib.NRG_MEMFS_PARTITION_TILE in SIZES and nrg._lib.NRG_MF_PREAD_TILE == T
    d = nrg.DeviceReplica(nrg._lib.NRG_DS_MEMFS, 0, log_bytes=MIN_LOG_BYTES, max_batch=64, log2_slots=7, queue_capacity=4)
    yield d
    d.close()


def _dev_bytes(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _sentinel(nbytes):
    import torch

    return torch.full((max(nbytes, 1),), 0xEE, dtype=torch.uint8, device="cuda")


# ---- the request partition -----------------------------------------------------------------------------
ODD = np.array([0, 4, 5, 6, 9, 5 + (1 << 32), (1 << 63) + 12345, (1 << 64) - 1], dtype=np.uint64)


def _requests(stream, n, parts, rng):
    rq = np.zeros(n, P.RD_DTYPE)
    i = np.arange(n, dtype=np.uint64)
    if stream == "one_owner":
        rq["ino"] = np.uint64(5 + 3) + np.uint64(parts) * (i % np.uint64(5))
    elif stream == "round_robin":
        rq["ino"] = np.uint64(5) + i
    else:  # inos 0, 4, 5 and 2^64 - 1 among others
        rq["ino"] = ODD[rng.integers(0, len(ODD), n)]
    rq["offset"] = i  # every request is different from every other
    rq["len"] = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    return rq


@pytest.mark.parametrize("parts", PARTS)
def test_request_partition_against_numpy(nrg, dev, parts):
    import torch
    from nrgpu.parallel import memfs_owner

    L, lib = nrg._lib, dev._lib
    rng = np.random.default_rng(700 + parts)
    PAD = 3
    for stream in ("one_owner", "round_robin", "odd_inos"):
        for n in SIZES:
            what = f"{stream} n={n} parts={parts}"
            rq = _requests(stream, n, parts, rng)
            own = memfs_owner(rq["ino"], parts)
            assert [PS.owner(i, parts) for i in rq["ino"][:50]] == own[:50].tolist()
            order = np.argsort(own, kind="stable")
            d_rq = _dev_bytes(rq) if n else _sentinel(24)
            d_out, d_pos, d_cnt = _sentinel((n + PAD) * 24), _sentinel((n + PAD) * 4), _sentinel((parts + PAD) * 8)
            torch.cuda.synchronize()
            assert lib.nrg_memfs_rd_partition_async(dev._h, d_rq.data_ptr(), n, parts, d_out.data_ptr(), d_pos.data_ptr(),
                                                    d_cnt.data_ptr()) == L.NRG_OK, what
            assert lib.nrg_sync(dev._h) == L.NRG_OK
            out, pos, cnt = d_out.cpu().numpy(), d_pos.cpu().numpy().view(np.uint32), d_cnt.cpu().numpy().view(np.uint64)
            assert out[: n * 24].tobytes() == rq[order].tobytes(), what
            assert (out[n * 24:] == 0xEE).all(), what + ": bytes past n requests"
            inv = np.empty(n, np.int64)
            inv[order] = np.arange(n)
            np.testing.assert_array_equal(pos[:n], inv, err_msg=what)
            assert (pos[n:] == 0xEEEEEEEE).all(), what
            np.testing.assert_array_equal(cnt[:parts], np.bincount(own, minlength=parts), err_msg=what)
            assert (cnt[parts:] == 0xEEEEEEEEEEEEEEEE).all(), what
            if stream == "one_owner" and n:
                assert np.count_nonzero(cnt[:parts]) == 1


def test_request_partition_refusals(nrg, dev):
    L, lib = nrg._lib, dev._lib
    b = _sentinel(4096)
    p = b.data_ptr()
    assert lib.nrg_memfs_rd_partition_async(dev._h, p, 1, 0, p, p, p) == L.NRG_E_INVAL
    assert lib.nrg_memfs_rd_partition_async(dev._h, p, 1, 65, p, p, p) == L.NRG_E_INVAL
    assert lib.nrg_memfs_rd_partition_async(dev._h, p, 1, 2, p, p, None) == L.NRG_E_INVAL
    assert lib.nrg_memfs_rd_partition_async(dev._h, None, 1, 2, p, p, p) == L.NRG_E_INVAL
    assert lib.nrg_memfs_rd_partition_async(dev._h, p + 4, 1, 2, p, p, p) == L.NRG_E_INVAL
    assert lib.nrg_memfs_rd_partition_async(dev._h, p, 1 << 32, 2, p, p, p) == L.NRG_E_CAPACITY
    assert lib.nrg_sync(dev._h) == L.NRG_OK
    assert (b.cpu().numpy() == 0xEE).all()


# ---- the re-pack ---------------------------------------------------------------------------------------
def _model(files, log2_b):
    m = M.MemFsModel(files, log2_b)
    for f in range(files):
        m.init(M.FIRST_INO + f, M._pattern(np.random.default_rng(8100 + f), 1 << log2_b))
    return m


class Packed:
    """A request list answered on the CPU and laid out as the re-pack receives it: `owners` groups."""

    def __init__(self, name, model, rq, own):
        self.name, self.n = name, len(rq)
        order = np.argsort(own, kind="stable")
        self.pos = np.empty(self.n, np.uint32)
        self.pos[order] = np.arange(self.n, dtype=np.uint32)
        self.want = P.pread(model, rq)  # (data, offs, some) in request order
        src, offs, some = P.pread(model, rq[order])
        self.src, self.src_cnt, self.src_some = src, np.diff(offs.astype(np.int64)).astype(np.uint64), some
        self.total = int(self.want[1][-1])
        assert len(src) == self.total


_lists = {}


def packed(name):
    if name in _lists:
        return _lists[name]
    rng = np.random.default_rng(8200)
    if name == "repack_alignment":
        rq = GM.repack_alignment()
        x = Packed(name, _model(2, 12), rq, PS.owners(rq, 2))
    elif name.startswith("n"):  # past one scan tile of 1024 requests, and past two
        n = int(name[1:])
        rq = P.reqs([(5 + int(rng.integers(0, 5)), int(rng.integers(0, 300)), int(rng.integers(0, 40))) for _ in range(n)])
        x = Packed(name, _model(4, 8), rq, rng.integers(0, 3, n))
    else:
        r = {"edges": P.edges, "tile_edges": lambda: P.tile_edges(T), "skew_first": lambda: P.skew(True),
             "skew_last": lambda: P.skew(False)}[name]()
        x = Packed(name, _model(r.files, r.log2_b), r.rq, rng.integers(0, 3, len(r.rq)))  # spread over 3 owners
        assert sorted(x.pos.tolist()) == list(range(x.n)) and (x.pos != np.arange(x.n)).any()
    _lists[name] = x
    return x


def _repack(nrg, dev, x, cap, mis=0, what=""):
    import torch

    L, lib = nrg._lib, dev._lib
    end = min(cap, x.total)
    room = end + 64
    d_src = _sentinel(len(x.src) + 16)  # 16-byte aligned, readable to the next multiple of 16
    if len(x.src):
        d_src[: len(x.src)] = _dev_bytes(x.src)
    d_cnt, d_ssome, d_pos = _dev_bytes(x.src_cnt), _dev_bytes(x.src_some), _dev_bytes(x.pos)
    d_data, d_offs, d_some = _sentinel(room + 16), _sentinel((x.n + 2) * 8), _sentinel(x.n + 2)
    assert d_src.data_ptr() % 16 == 0 and d_data.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    rc = lib.nrg_memfs_pread_repack_async(dev._h, d_src.data_ptr(), d_cnt.data_ptr(), d_ssome.data_ptr(), d_pos.data_ptr(),
                                          x.n, d_data.data_ptr() + mis, cap, d_offs.data_ptr(), d_some.data_ptr())
    assert rc == L.NRG_OK, what
    assert lib.nrg_sync(dev._h) == L.NRG_OK
    data, offs, some = d_data.cpu().numpy(), d_offs.cpu().numpy().view(np.uint64), d_some.cpu().numpy()
    np.testing.assert_array_equal(offs[: x.n + 1], x.want[1], err_msg=what + " offs")
    np.testing.assert_array_equal(some[: x.n], x.want[2], err_msg=what + " some")
    assert offs[x.n + 1] == 0xEEEEEEEEEEEEEEEE and (some[x.n:] == 0xEE).all(), what + ": past n"
    assert data[mis:mis + end].tobytes() == x.want[0][:end].tobytes(), what + " data"
    assert (data[:mis] == 0xEE).all() and (data[mis + end:] == 0xEE).all(), what + ": bytes outside [0, min(cap, total))"


LISTS = ("repack_alignment", "edges", "tile_edges", "skew_first", "skew_last", "n1025", "n2049")


@pytest.mark.parametrize("name", LISTS)
def test_repack_against_the_model(nrg, dev, name):
    x = packed(name)
    _repack(nrg, dev, x, x.total + 100, what=name)
    for mis in (1, 7, 15):
        _repack(nrg, dev, x, x.total, mis=mis, what=f"{name} data + {mis}")


@pytest.mark.parametrize("name", ("repack_alignment", "tile_edges", "n2049"))
def test_repack_caps(nrg, dev, name):
    x = packed(name)
    assert x.total > T + 1
    for cap in (0, 1, x.total - 1, x.total, T - 1, T, T + 1):
        _repack(nrg, dev, x, cap, mis=cap % 16, what=f"{name} cap={cap}")


def test_repack_of_nothing_and_refusals(nrg, dev):
    import torch

    L, lib = nrg._lib, dev._lib
    b = _sentinel(4096)
    p = b.data_ptr()
    assert lib.nrg_memfs_pread_repack_async(dev._h, p, p, p, p, 0, p, 64, p, p) == L.NRG_OK  # n = 0: offs[0] = 0
    assert lib.nrg_sync(dev._h) == L.NRG_OK
    got = b.cpu().numpy()
    assert got[:8].view(np.uint64)[0] == 0 and (got[8:] == 0xEE).all()
    b.fill_(0xEE)
    torch.cuda.synchronize()
    for args in ((p + 8, p, p, p, 1, p, 64, p, p),      # a source that is not 16-byte aligned
                 (p, p + 4, p, p, 1, p, 64, p, p),      # counts not 8-byte aligned
                 (p, p, p, p, 1, p, 64, p + 4, p),      # offs not 8-byte aligned
                 (p, None, p, p, 1, p, 64, p, p), (p, p, None, p, 1, p, 64, p, p), (p, p, p, None, 1, p, 64, p, p),
                 (p, p, p, p, 1, None, 64, p, p), (p, p, p, p, 1, p, 64, None, p), (p, p, p, p, 1, p, 64, p, None)):
        assert lib.nrg_memfs_pread_repack_async(dev._h, *args) == L.NRG_E_INVAL, args
    assert lib.nrg_memfs_pread_repack_async(dev._h, p, p, p, p, 1 << 32, p, 64, p, p) == L.NRG_E_CAPACITY
    assert lib.nrg_sync(dev._h) == L.NRG_OK
    assert (b.cpu().numpy() == 0xEE).all()
    hm = nrg.DeviceReplica(L.NRG_DS_HASHMAP, 0, log2_slots=10, max_batch=64)
    assert lib.nrg_memfs_pread_repack_async(hm._h, p, p, p, p, 0, p, 64, p, p) == L.NRG_E_INVAL
    assert lib.nrg_memfs_rd_partition_async(hm._h, p, 0, 2, p, p, p) == L.NRG_E_INVAL
    hm.close()
