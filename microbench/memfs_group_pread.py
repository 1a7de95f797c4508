"""The group-wide pread of a file-partitioned group at one rank (one GPU; run on the GPU box) beside the
direct call it is made of, the launches it adds, and a plain copy of the same bytes. NO multi-GPU figure
comes out of this: with one rank the owner is the asker, so the "moving" variant pays every step of the
protocol (both host round trips, every launch, the copies that stand in for send / recv) on one device.

Four ways through the same requests, alternating window by window so that drift hits all of them alike
(the method of microbench/memfs_partitioned.py):
  direct    nrg_memfs_pread_async on a plain replica, then a stream synchronise
  identity  nrg_group_memfs_pread on a one-rank group: the same kernels into the caller's buffers, and
            offs[n] read back for the capacity answer (group.hpp pt_ident)
  moving    the same with NRG_KNOB_EXP bit 16: the request partition (three launches), host round trip 1,
            the owner's scan and totals, host round trip 2, the owner's packed copy, the re-pack
  copy      a device-to-device copy of the answer's bytes, then a synchronise
Two shapes of N requests:
  nrfs      benches/nrfs.rs:88-101: F = 16 files of 4096 bytes, every request a whole-file read
  small     the same files, reads of 0 .. 3 bytes at random offsets
A window is ROUNDS calls between a host clock's two readings (every variant ends a call synchronised);
the figure per variant is the median window, with the lowest and highest beside it. Then, in a window of
their own, the library's per-kernel times of the moving variant.
Usage: python microbench/memfs_group_pread.py [N] [ROUNDS] [WINDOWS]
"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "node-replication_amd"))
import nrgpu  # noqa: E402,F401
from nrgpu import _lib as L  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 8
WINDOWS = int(sys.argv[3]) if len(sys.argv) > 3 else 7
WARM = 2
FILES, LOG2_B = 16, 12
KERNELS = (b"rd_count", b"rd_scan", b"rd_scatter", b"mf_pread_reduce", b"mf_pread_aggscan", b"mf_pread_scan",
           b"mf_pread_totals", b"mf_pread_copy", b"mf_repack_reduce", b"mf_repack_aggscan", b"mf_repack_scan", b"mf_repack_copy")
lib = L.load()


def config():
    cfg = L.default_config(L.NRG_DS_MEMFS)
    cfg.log2_slots, cfg.queue_capacity, cfg.max_batch, cfg.max_reads = LOG2_B, FILES, 1024, N
    return cfg


def requests(shape):
    rng = np.random.default_rng(91)
    rq = np.zeros(N, L.MEMFS_RD_DTYPE)
    rq["ino"] = L.NRG_MEMFS_FIRST_INO + rng.integers(0, FILES, N)
    if shape == "nrfs":
        rq["len"] = 1 << LOG2_B
    else:
        rq["offset"] = rng.integers(0, (1 << LOG2_B) - 4, N)
        rq["len"] = rng.integers(0, 4, N)
    return rq


class Direct:
    name = "direct"

    def __init__(self):
        cfg = config()
        self.h = C.c_void_p()
        L.check(lib.nrg_open(0, C.byref(cfg), C.byref(self.h)), "nrg_open")

    def read(self, rq, data, cap, offs, some):
        L.check(lib.nrg_memfs_pread_async(self.h, rq, N, data, cap, offs, some))
        L.check(lib.nrg_sync(self.h))

    def close(self):
        lib.nrg_close(self.h)


class Group:
    def __init__(self, moving):
        self.name = "moving" if moving else "identity"
        cfg = config()
        self.g = C.c_void_p()
        devs = (C.c_int * 1)(0)
        rc = lib.nrg_group_open(devs, 1, C.byref(cfg), C.byref(self.g))
        if rc == L.NRG_E_COMM:  # no RCCL in this process: the loopback collectives
            L.check(lib.nrg_test_loopback_collectives(1))
            rc = lib.nrg_group_open(devs, 1, C.byref(cfg), C.byref(self.g))
            L.check(lib.nrg_test_loopback_collectives(0))
        L.check(rc, "nrg_group_open")
        self.h = lib.nrg_group_replica(self.g, 0)
        if moving:
            L.check(lib.nrg_test_set_knob(self.h, L.KNOBS["EXP"], 0x10000))
        self.rd = (L.Pread * 1)()

    def read(self, rq, data, cap, offs, some):
        r = self.rd[0]
        r.reqs, r.n, r.data, r.cap, r.offs, r.some = rq, N, data, cap, offs, some
        L.check(lib.nrg_group_memfs_pread(self.g, self.rd), "group pread")

    def close(self):
        lib.nrg_group_close(self.g)


class Copy:
    name = "copy"

    def __init__(self, total):
        self.src = torch.empty(max(total, 1), dtype=torch.uint8, device="cuda")
        self.total = total

    def read(self, rq, data, cap, offs, some):
        self.dst[: self.total].copy_(self.src[: self.total])
        torch.cuda.synchronize()

    def close(self):
        pass


def run(shape):
    rq = requests(shape)
    total = int(rq["len"].sum())  # (every request lies inside its file)
    d_rq = torch.from_numpy(rq.view(np.uint8).reshape(-1).copy()).cuda()
    d_data = torch.empty(max(total, 1), dtype=torch.uint8, device="cuda")
    d_offs = torch.empty(N + 1, dtype=torch.int64, device="cuda")
    d_some = torch.empty(N, dtype=torch.uint8, device="cuda")
    variants = [Direct(), Group(False), Group(True), Copy(total)]
    variants[3].dst = d_data
    torch.cuda.synchronize()
    args = (d_rq.data_ptr(), d_data.data_ptr(), total, d_offs.data_ptr(), d_some.data_ptr())
    for v in variants:
        for _ in range(WARM):
            v.read(*args)
        assert int(d_offs[-1].item()) == total
    us = {v.name: [] for v in variants}
    for _ in range(WINDOWS):
        for v in variants:
            t = time.perf_counter()
            for _ in range(ROUNDS):
                v.read(*args)
            us[v.name].append((time.perf_counter() - t) * 1e6 / ROUNDS)
    for name, xs in us.items():
        print(f"{shape}: {N} requests, {total} bytes: {name:9s} median {statistics.median(xs):9.1f} us  "
              f"(windows {min(xs):.1f} .. {max(xs):.1f})", flush=True)
    mv = variants[2]
    L.check(lib.nrg_kernel_timing(mv.h, 1))
    for _ in range(ROUNDS):
        mv.read(*args)
    parts = []
    for k in KERNELS:
        n, ms = C.c_uint64(), C.c_double()
        L.check(lib.nrg_kernel_time(mv.h, k, C.byref(n), C.byref(ms)))
        if n.value:
            parts.append(f"{k.decode()} {ms.value * 1e3 / n.value:.1f} us")
    L.check(lib.nrg_kernel_timing(mv.h, 0))
    print(f"{shape}: moving, per launch: " + ", ".join(parts), flush=True)
    for v in variants:
        v.close()


if __name__ == "__main__":
    if nrgpu.device_count() < 1:
        raise SystemExit("memfs_group_pread: no HIP device visible")
    for shape in ("nrfs", "small"):
        run(shape)
