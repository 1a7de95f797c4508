"""The file partition of file-store records and the route-back of their responses
(nrg_memfs_partition_async, nrg_memfs_route_back_async; csrc/partition.hip) against numpy: the stable
partition is np.argsort(owner, kind="stable"). Sizes around a wave, around the kernel's 256-record tile,
around eight tiles, several tiles with a ragged last one, and 20000 records; 1 to 64 owners; streams with
one owner, owners round-robin, runs of one owner longer than a wave and longer than a tile, and inos
below the first file and far past the last. Every output buffer is longer than it need be and filled
with a sentinel: nothing at or past n records may change."""
import ctypes as C

import numpy as np
import pytest

import memfs_model as M

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 3 * 2048 + 17, 20000)
PARTS = (1, 2, 3, 7, 8, 64)
MIN_LOG_BYTES = 2 * 32 * 256 * 64


@pytest.fixture(scope="module")
def dev(nrg):
    assert nrg._lib.NRG_MEMFS_PARTITION_TILE in SIZES  # T - 1, T and T + 1 are in the list
    d = nrg.DeviceReplica(nrg._lib.NRG_DS_MEMFS, 0, log_bytes=MIN_LOG_BYTES, max_batch=64, log2_slots=7, queue_capacity=4)
    yield d
    d.close()


def _inos(stream, n, parts, rng):
    i = np.arange(n, dtype=np.uint64)
    if stream == "one_owner":
        return np.full(n, 5 + 3, np.uint64) + np.uint64(parts) * (i % np.uint64(5))  # several files, one owner
    if stream == "round_robin":
        return np.uint64(5) + i
    if stream == "runs":  # runs of one owner: longer than a wave, longer than a tile, and short ones between
        lens = [70, 300, 1, 65, 257, 5, 129, 64]
        out, k = [], 0
        while sum(len(x) for x in out) < n:
            out.append(np.full(lens[k % len(lens)], 5 + (k * 7) % 97, np.uint64))
            k += 1
        return np.concatenate(out)[:n] if n else np.zeros(0, np.uint64)
    assert stream == "odd_inos"  # below the first ino (owner 0), past the last file, the ends of u64
    pick = np.array([0, 1, 2, 3, 4, 5, 6, 9, 5 + (1 << 20), 5 + (1 << 32), 7 + (1 << 32), (1 << 63), (1 << 63) + 12345,
                     (1 << 64) - 1, (1 << 64) - 2], dtype=np.uint64)
    return pick[rng.integers(0, len(pick), n)]


def _records(nrg, inos, rng):
    n = len(inos)
    recs = rng.integers(0, 256, (n, 152), dtype=np.uint8).view(nrg.MEMFS_OP_DTYPE).reshape(n)
    recs["ino"] = inos
    recs["offset"] = np.arange(n)  # every record is different from every other
    return recs


def _dev_bytes(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _sentinel(torch, nbytes):
    return torch.full((nbytes,), 0xEE, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("parts", PARTS)
def test_partition_and_route_back_against_numpy(nrg, dev, parts):
    import torch
    from nrgpu.parallel import memfs_owner

    L = nrg._lib
    lib = dev._lib
    rng = np.random.default_rng(900 + parts)
    PAD = 3  # records, positions and counts past the end that must keep their sentinel
    for stream in ("one_owner", "round_robin", "runs", "odd_inos"):
        for n in SIZES:
            what = f"{stream} n={n} parts={parts}"
            recs = _records(nrg, _inos(stream, n, parts, rng), rng)
            own = memfs_owner(recs["ino"], parts)
            order = np.argsort(own, kind="stable")
            d_ops = _dev_bytes(torch, recs) if n else _sentinel(torch, 152)
            d_out = _sentinel(torch, (n + PAD) * 152)
            d_pos = _sentinel(torch, (n + PAD) * 4)
            d_cnt = _sentinel(torch, (parts + PAD) * 8)
            torch.cuda.synchronize()
            assert lib.nrg_memfs_partition_async(dev._h, d_ops.data_ptr(), n, parts, d_out.data_ptr(), d_pos.data_ptr(),
                                                 d_cnt.data_ptr()) == L.NRG_OK, what
            # the responses an owner-ordered replay would give, and their way back
            resp = rng.integers(0, 256, (n, 136), dtype=np.uint8)
            some = rng.integers(0, 256, n, dtype=np.uint8)
            d_src = _dev_bytes(torch, resp[order]) if n else _sentinel(torch, 136)
            d_src8 = _dev_bytes(torch, some[order]) if n else _sentinel(torch, 8)
            d_dst = _sentinel(torch, (n + PAD) * 136)
            d_dst8 = _sentinel(torch, n + PAD)
            torch.cuda.synchronize()
            assert lib.nrg_memfs_route_back_async(dev._h, d_src.data_ptr(), d_src8.data_ptr(), d_pos.data_ptr(), n,
                                                  d_dst.data_ptr(), d_dst8.data_ptr()) == L.NRG_OK, what
            assert lib.nrg_sync(dev._h) == L.NRG_OK
            out = d_out.cpu().numpy()
            pos = d_pos.cpu().numpy().view(np.uint32)
            cnt = d_cnt.cpu().numpy().view(np.uint64)
            # groups in owner order, each in issue order
            assert out[: n * 152].tobytes() == recs[order].tobytes(), what
            assert (out[n * 152:] == 0xEE).all(), what + ": bytes past n records"
            # where record i went: a permutation, the inverse of the stable order
            assert sorted(pos[:n].tolist()) == list(range(n)), what
            inv = np.empty(n, np.int64)
            inv[order] = np.arange(n)
            np.testing.assert_array_equal(pos[:n], inv, err_msg=what)
            assert (pos[n:] == 0xEEEEEEEE).all(), what
            np.testing.assert_array_equal(cnt[:parts], np.bincount(own, minlength=parts), err_msg=what)
            assert (cnt[parts:] == 0xEEEEEEEEEEEEEEEE).all(), what
            # the route-back restores issue order
            dst = d_dst.cpu().numpy()
            dst8 = d_dst8.cpu().numpy()
            assert dst[: n * 136].tobytes() == resp.tobytes(), what
            assert (dst[n * 136:] == 0xEE).all() and (dst8[n:] == 0xEE).all(), what
            np.testing.assert_array_equal(dst8[:n], some, err_msg=what)


def test_route_back_of_one_pair_leaves_the_other_alone(nrg, dev):
    import torch

    L, lib = nrg._lib, dev._lib
    n = 300
    rng = np.random.default_rng(5)
    pos = rng.permutation(n).astype(np.uint32)
    resp = rng.integers(0, 256, (n, 136), dtype=np.uint8)
    some = rng.integers(0, 256, n, dtype=np.uint8)
    d_pos, d_src, d_src8 = _dev_bytes(torch, pos), _dev_bytes(torch, resp), _dev_bytes(torch, some)
    d_dst, d_dst8 = _sentinel(torch, n * 136), _sentinel(torch, n)
    torch.cuda.synchronize()
    assert lib.nrg_memfs_route_back_async(dev._h, d_src.data_ptr(), None, d_pos.data_ptr(), n, d_dst.data_ptr(), None) == L.NRG_OK
    assert lib.nrg_sync(dev._h) == L.NRG_OK
    assert d_dst.cpu().numpy().tobytes() == resp[pos].tobytes() and (d_dst8.cpu().numpy() == 0xEE).all()
    d_dst = _sentinel(torch, n * 136)
    torch.cuda.synchronize()
    assert lib.nrg_memfs_route_back_async(dev._h, None, d_src8.data_ptr(), d_pos.data_ptr(), n, None, d_dst8.data_ptr()) == L.NRG_OK
    assert lib.nrg_sync(dev._h) == L.NRG_OK
    np.testing.assert_array_equal(d_dst8.cpu().numpy(), some[pos])
    assert (d_dst.cpu().numpy() == 0xEE).all()


def test_arguments(nrg, dev):
    import torch

    L, lib = nrg._lib, dev._lib
    buf = _sentinel(torch, 4096)
    p = buf.data_ptr()
    torch.cuda.synchronize()
    for parts in (0, L.NRG_MAX_PARTS + 1):
        assert lib.nrg_memfs_partition_async(dev._h, p, 1, parts, p + 1024, p + 2048, p + 3072) == L.NRG_E_INVAL
    assert lib.nrg_memfs_partition_async(dev._h, p, 1, 2, p + 1024, p + 2048, None) == L.NRG_E_INVAL
    assert lib.nrg_memfs_partition_async(dev._h, None, 1, 2, p + 1024, p + 2048, p + 3072) == L.NRG_E_INVAL
    assert lib.nrg_memfs_partition_async(dev._h, p + 4, 1, 2, p + 1024, p + 2048, p + 3072) == L.NRG_E_INVAL  # alignment
    assert lib.nrg_memfs_partition_async(dev._h, p, 1 << 32, 2, p + 1024, p + 2048, p + 3072) == L.NRG_E_CAPACITY
    assert lib.nrg_memfs_route_back_async(dev._h, p, None, None, 1, p + 1024, None) == L.NRG_E_INVAL
    assert lib.nrg_memfs_route_back_async(dev._h, None, None, p, 1, p + 1024, None) == L.NRG_E_INVAL
    assert lib.nrg_memfs_route_back_async(dev._h, p, None, p + 2048, 1 << 32, p + 1024, None) == L.NRG_E_CAPACITY
    hm = nrg.DeviceReplica(L.NRG_DS_HASHMAP, 0, log2_slots=10, log_bytes=MIN_LOG_BYTES, max_batch=64)
    assert lib.nrg_memfs_partition_async(hm._h, p, 1, 2, p + 1024, p + 2048, p + 3072) == L.NRG_E_INVAL  # another kind
    assert lib.nrg_memfs_route_back_async(hm._h, p, None, p + 2048, 1, p + 1024, None) == L.NRG_E_INVAL
    hm.close()
    assert lib.nrg_sync(dev._h) == L.NRG_OK
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0xEE).all()  # none of the refused calls wrote anything
