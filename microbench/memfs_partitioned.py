"""A file-partitioned file-store round at N = 1 (one rank, one GPU; run on the GPU box) beside the direct
call it is made of, the launches it adds, and a plain copy of the same bytes.

Three ways through the same records, alternating window by window so that drift hits all of them alike:
  direct    nrg_memfs_round_async on a plain replica
  identity  nrg_group_file_round on a one-rank group: the replay reads the caller's records and answers
            into the caller's buffers (group.hpp pt_ident)
  moving    the same with NRG_KNOB_EXP bit 16: partition (three launches), the count read back on the
            host, the replay from the partition's output, one route-back launch
Two shapes, N records per round, responses wanted:
  nrfs      benches/nrfs.rs: F = 16 files of 4096 bytes, every op a whole-file FileWrite, so runs of 32
            Write records of 128 bytes, the files in turn
  memfs     benches/memfs.rs: one file of 4096 bytes, 10 % Writes of 128 bytes, the rest Reads of 0 .. 127
A window is ROUNDS rounds between a host clock's two readings, the second after a synchronise; the figure
per variant is the median window, with the lowest and highest beside it. Then, in a window of their own
(the event records sit between the timed kernels), the library's per-kernel times of the moving variant:
the partition's fp_count, fp_scan and fp_scatter and the route-back fp_route beside mf_lines. Last, a plain
device-to-device copy of the same N * 152 bytes: the floor the partition can be held against.
With a fourth argument G > 1, G members take turns on this one GPU over the loopback collectives, N / G
records each: the protocol's cost with every step present, NOT an estimate of G GPUs.
Usage: python microbench/memfs_partitioned.py [N] [ROUNDS] [WINDOWS] [G]
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

N = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 8
WINDOWS = int(sys.argv[3]) if len(sys.argv) > 3 else 7
LOOP_G = int(sys.argv[4]) if len(sys.argv) > 4 else 0
WARM = 2
LOG2_B = 12
lib = L.load()


def config(files):
    cfg = L.default_config(L.NRG_DS_MEMFS)
    cfg.log2_slots, cfg.queue_capacity, cfg.max_batch = LOG2_B, files, N
    cfg.log_bytes = 64 * 4 * max(N, 8192)
    return cfg


def records(shape):
    """(files, two record buffers on the device that take turns)."""
    B = 1 << LOG2_B
    out = []
    for b in range(2):
        rng = np.random.default_rng(77 + b)
        recs = np.zeros(N, L.MEMFS_OP_DTYPE)
        i = np.arange(N)
        if shape == "nrfs":  # op j = FileWrite(file j % 16): 32 records of one ino, a line each
            files = 16
            recs["ino"] = L.NRG_MEMFS_FIRST_INO + (i // 32) % files
            recs["offset"] = (i % 32) * 128
            recs["op"], recs["len"] = L.NRG_MEMFS_WRITE, 128
            recs["data"] = rng.integers(2, 256, (N, 128), dtype=np.uint8)
        else:
            files = 1
            wr = rng.permutation(N) < N // 10
            recs["ino"] = L.NRG_MEMFS_FIRST_INO
            recs["offset"] = rng.integers(0, B - 256, N)
            recs["op"] = np.where(wr, L.NRG_MEMFS_WRITE, L.NRG_MEMFS_READ)
            recs["len"] = np.where(wr, 128, rng.integers(0, 128, N))
            recs["data"][wr] = rng.integers(2, 256, (int(wr.sum()), 128), dtype=np.uint8)
        out.append(torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).cuda())
    return files, out


class Direct:
    name = "direct"

    def __init__(self, files):
        cfg = config(files)
        self.h = C.c_void_p()
        L.check(lib.nrg_open(0, C.byref(cfg), C.byref(self.h)), "nrg_open")

    def round(self, recs, resp, some):
        L.check(lib.nrg_memfs_round_async(self.h, recs, N, 1, resp, some))

    def sync(self):
        L.check(lib.nrg_sync(self.h))

    def close(self):
        lib.nrg_close(self.h)


class Group:
    """G members on device 0; member i's records are the i-th N / G of the round's."""

    def __init__(self, files, moving, G=1):
        self.name = ("moving" if moving else "identity") if G == 1 else f"loop{G}"
        self.G = G
        cfg = config(files)
        self.g = C.c_void_p()
        devs = (C.c_int * G)(*([0] * G))
        rc = L.NRG_E_COMM if G > 1 else lib.nrg_group_open(devs, G, C.byref(cfg), C.byref(self.g))
        if rc == L.NRG_E_COMM:  # several members on one GPU, or no RCCL in this process: the loopback collectives
            L.check(lib.nrg_test_loopback_collectives(1))
            rc = lib.nrg_group_open(devs, G, C.byref(cfg), C.byref(self.g))
            L.check(lib.nrg_test_loopback_collectives(0))
        L.check(rc, "nrg_group_open")
        self.h = lib.nrg_group_replica(self.g, 0)
        if moving:
            L.check(lib.nrg_test_set_knob(self.h, L.KNOBS["EXP"], 0x10000))
        self.rd = (L.Round * G)()

    def round(self, recs, resp, some):
        per = N // self.G
        for i in range(self.G):
            r = self.rd[i]
            r.recs, r.n, r.resp, r.some = recs + i * per * 152, per, resp + i * per * 136, some + i * per
        L.check(lib.nrg_group_file_round(self.g, self.rd), "file round")

    def sync(self):
        L.check(lib.nrg_group_sync(self.g))

    def close(self):
        lib.nrg_group_close(self.g)


def report(what, us):
    for name, xs in us.items():
        print(f"{what} {name:9s} median {statistics.median(xs):9.1f} us  (windows {min(xs):.1f} .. {max(xs):.1f})", flush=True)


def run(shape):
    files, bufs = records(shape)
    resp = torch.empty(N * 136, dtype=torch.uint8, device="cuda")
    some = torch.empty(N, dtype=torch.uint8, device="cuda")
    variants = [Direct(files), Group(files, False), Group(files, True)]
    if LOOP_G > 1:
        variants.append(Group(files, False, LOOP_G))
    torch.cuda.synchronize()

    def one(v, b):
        v.round(bufs[b % 2].data_ptr(), resp.data_ptr(), some.data_ptr())

    for v in variants:
        for b in range(WARM):
            one(v, b)
        v.sync()
    us = {v.name: [] for v in variants}
    for w in range(WINDOWS):
        for v in variants:
            t = time.perf_counter()
            for r in range(ROUNDS):
                one(v, r)
            v.sync()
            us[v.name].append((time.perf_counter() - t) * 1e6 / ROUNDS)
    report(f"{shape}: round of {N} records, F={files}:", us)
    # the moving variant's launches, from the library's own event pairs
    mv = variants[2]
    L.check(lib.nrg_kernel_timing(mv.h, 1))
    for r in range(ROUNDS):
        one(mv, r)
    mv.sync()
    parts = []
    for k in (b"fp_count", b"fp_scan", b"fp_scatter", b"fp_route", b"mf_expand", b"mf_sort", b"mf_lines"):
        n, ms = C.c_uint64(), C.c_double()
        L.check(lib.nrg_kernel_time(mv.h, k, C.byref(n), C.byref(ms)))
        parts.append(f"{k.decode()} {ms.value * 1e3 / max(n.value, 1):.1f} us")
    L.check(lib.nrg_kernel_timing(mv.h, 0))
    print(f"{shape}: moving, per launch: " + ", ".join(parts), flush=True)
    for v in variants:
        v.sync()
        v.close()
    # the floor: the same bytes copied once, device to device
    dst = torch.empty_like(bufs[0])
    cp = []
    for w in range(WINDOWS + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for r in range(ROUNDS):
            dst.copy_(bufs[r % 2])
        torch.cuda.synchronize()
        if w:  # (the first window warms up)
            cp.append((time.perf_counter() - t) * 1e6 / ROUNDS)
    report(f"{shape}: device-to-device copy of {N * 152} bytes:", {"copy": cp})


if __name__ == "__main__":
    for shape in ("nrfs", "memfs"):
        run(shape)
