"""Batched read-only reads of the file store (nrg_memfs_pread_async; run on the GPU box) in three
shapes, each beside the same requests as a loop of nrg_memfs_read calls (one request per call, a host
copy each: the only way before nrg_memfs_pread):
  (a) nrfs    benches/nrfs.rs:88-101 FileRead: 1024 files of 4 KiB, 2^16 whole-file reads (256 MiB out)
  (b) memfs   the Reads of benches/memfs.rs:294-322: 1024 files of 4 KiB, 2^20 reads of 0..127 bytes at
              random offsets (about 63.5 MiB out)
  (c) skew    one 64-MiB file: one whole-file read beside 2^16 one-byte reads

Per shape: WARM warm-up calls, then a window of ROUNDS calls between two stream events (call time =
window / ROUNDS; cap = the exact total, known on the host), then the same window again for the spread;
the per-kernel times are the library's own event pairs (nrg_kernel_timing) in a third window. "GB/s" is
bytes moved (the packed output, read once and written once: 2 x total) divided by the call time. The
baseline loop runs BASE requests of the shape (every BASE-th request; shape (c): the whole-file read
and BASE one-byte reads) and is scaled to the shape's request count.

Measured on an MI355X, MF_PREAD_TILE = 16384, ROUNDS = 10, BASE = 1024 (one run; DESIGN.md "Read-only
reads" has the table and the other tile sizes):
  nrfs   call 0.174 / 0.174 ms, 3084 GB/s moved, mf_pread_copy 0.165 ms; nrg_memfs_read loop 3383 ms
  memfs  call 0.235 / 0.233 ms,  566 GB/s moved, mf_pread_copy 0.210 ms; nrg_memfs_read loop 52827 ms
  skew   call 0.125 / 0.125 ms, 1073 GB/s moved, mf_pread_copy 0.115 ms; nrg_memfs_read loop 3371 ms
Usage: python microbench/memfs_pread.py [ROUNDS] [BASE]
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "node-replication_amd"))
import nrgpu  # noqa: E402
from nrgpu import _lib as L  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
BASE = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
WARM = 3
KERNELS = ("mf_pread_reduce", "mf_pread_aggscan", "mf_pread_scan", "mf_pread_copy")


def shape(name):
    rng = np.random.default_rng(7)
    if name == "nrfs":
        files, log2_b, n = 1024, 12, 1 << 16
        rq = np.zeros(n, nrgpu.MEMFS_RD_DTYPE)
        rq["ino"] = L.NRG_MEMFS_FIRST_INO + rng.integers(0, files, n)
        rq["len"] = 4096
    elif name == "memfs":
        files, log2_b, n = 1024, 12, 1 << 20
        rq = np.zeros(n, nrgpu.MEMFS_RD_DTYPE)
        rq["ino"] = L.NRG_MEMFS_FIRST_INO + rng.integers(0, files, n)
        rq["offset"] = rng.integers(0, 4096 - 256, n)
        rq["len"] = rng.integers(0, 128, n)
    else:
        files, log2_b, n = 1, 26, (1 << 16) + 1
        rq = np.zeros(n, nrgpu.MEMFS_RD_DTYPE)
        rq["ino"] = L.NRG_MEMFS_FIRST_INO
        rq["offset"] = rng.integers(0, 1 << 26, n)
        rq["len"] = 1
        rq[n // 2] = (L.NRG_MEMFS_FIRST_INO, 0, 1 << 26)
    return files, log2_b, rq


def window(dev, d_rq, n, d_data, cap, d_offs, d_some, rounds):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(rounds):
        dev.mf_pread_device(d_rq, n, d_data, cap, d_offs, d_some)
    e1.record()
    e1.synchronize()
    dev.sync()
    return e0.elapsed_time(e1) / rounds


def baseline(dev, rq, name):
    """seconds for the whole shape as a loop of nrg_memfs_read calls, from a subset scaled up"""
    buf = np.zeros(int(rq["len"].max()), np.uint8)
    got = C.c_uint64()
    p = C.c_void_p(buf.ctypes.data)

    def loop(sub):
        t0 = time.perf_counter()
        for r in sub:
            L.check(dev._lib.nrg_memfs_read(dev._h, int(r["ino"]), int(r["offset"]), int(r["len"]), p, C.byref(got)))
        return time.perf_counter() - t0

    if name == "skew":
        small = rq[rq["len"] == 1]
        return loop(rq[rq["len"] > 1]) + loop(small[:BASE]) * len(small) / min(BASE, len(small))
    sub = rq[:: max(len(rq) // BASE, 1)]
    return loop(sub) * len(rq) / len(sub)


def run(name):
    files, log2_b, rq = shape(name)
    n = len(rq)
    dev = nrgpu.DeviceReplica(L.NRG_DS_MEMFS, 0, log2_slots=log2_b, queue_capacity=files, max_batch=1024, max_reads=n)
    dev.use_torch_stream()
    left = (1 << log2_b) - np.minimum(rq["offset"], 1 << log2_b)
    total = int(np.minimum(rq["len"], left).sum())
    d_rq = torch.from_numpy(rq.view(np.uint8).reshape(-1).copy()).cuda()
    d_data = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    d_some = torch.empty(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    args = (dev, d_rq, n, d_data, total, d_offs, d_some)
    window(*args, WARM)
    a = window(*args, ROUNDS)
    b = window(*args, ROUNDS)
    assert int(d_offs[-1].item()) == total and int(d_some.sum().item()) == n
    dev.kernel_timing(True)
    window(*args, ROUNDS)
    kt = {}
    for k in KERNELS:
        launches, ms = dev.kernel_time(k)
        kt[k] = ms / max(launches, 1)
    dev.kernel_timing(False)
    base = baseline(dev, rq, name)
    print(f"memfs_pread {name}: files={files} B={1 << log2_b} requests={n} bytes={total} rounds={ROUNDS}: "
          f"call {a:.3f} ms / {b:.3f} ms ({n / a / 1e3:.1f} Mreads/s, {2 * total / a / 1e6:.1f} GB/s moved); "
          + ", ".join(f"{k} {kt[k]:.3f} ms" for k in KERNELS)
          + f"; nrg_memfs_read loop (scaled from {BASE}): {base * 1e3:.1f} ms = {base * 1e3 / a:.0f} x", flush=True)
    dev.close()


if __name__ == "__main__":
    if nrgpu.device_count() < 1:
        raise SystemExit("memfs_pread: no HIP device visible")
    for s in sys.argv[3:] or ("nrfs", "memfs", "skew"):
        run(s)
