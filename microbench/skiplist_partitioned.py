"""A partitioned skip-list round at N = 1 (one rank, one GPU; run on the GPU box) beside the direct calls
it is made of, and one group-wide seek.

Three ways through the same ops, alternating window by window so that drift hits all of them alike:
  direct    nrg_skiplist_round_async + nrg_skiplist_get_async on a plain replica
  identity  nrg_group_partitioned_round on a one-rank group: the owner's replay reads the caller's
            records and answers into the caller's buffers (group.hpp pt_ident)
  moving    the same with NRG_KNOB_EXP bit 16: partition copy on the side stream, route-back launch
Shapes are microbench/skiplist_round.py's (generate_sops_concurrent, benches/lockfree.rs:128-154): N ops
per round, 10 % and 100 % Push(random u64, random u64), the rest Get(random u64), on a map prefilled
with 2^22 keys i -> i; random keys are new keys, so every round uses a fresh batch. A window is ROUNDS
rounds between a host clock's two readings, the second after a synchronise; the figure per variant is
the median window, with the lowest and highest beside it (the window-to-window spread). Then one
nrg_group_skiplist_seek of N keys against nrg_skiplist_seek_async, the same way: the identity group
answers straight into the caller's buffers, the moving one takes the general path (padded send copy,
all-gather, candidates back, reduction) with one rank.
No multi-rank figure is taken here: a one-rank group runs no collective in a round.
Usage: python microbench/skiplist_partitioned.py [N] [ROUNDS] [WINDOWS]
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
import nrgpu  # noqa: E402
from nrgpu import _lib as L  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 6
WINDOWS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
PREFILL = 1 << 22
LOG2 = 26
WARM = 2
NB = WARM + ROUNDS * WINDOWS  # a fresh batch for every round of a variant's run
lib = L.load()


def config():
    cfg = L.default_config(L.NRG_DS_SKIPLIST)
    cfg.log2_slots, cfg.max_batch, cfg.max_reads = LOG2, N, N
    cfg.log_bytes = 64 * 4 * max(N, 8192)
    return cfg


def batches(write_ratio):
    W = sum(1 for i in range(100) if i < write_ratio) * (N // 100)
    R = N - W
    puts, gets = [], []
    for b in range(NB):
        rng = np.random.default_rng(4242 + 1000 * write_ratio + b)
        recs = rng.integers(0, 2**64 - 1, (W, 2), dtype=np.uint64)
        puts.append(torch.from_numpy(recs.view(np.int64)).cuda())
        if b < 4 and R:  # the Gets of four batches, used in turn
            gets.append(torch.from_numpy(rng.integers(0, 2**64 - 1, R, dtype=np.uint64).view(np.int64)).cuda())
    return W, R, puts, gets


class Direct:
    name = "direct"

    def __init__(self):
        cfg = config()
        self.h = C.c_void_p()
        L.check(lib.nrg_open(0, C.byref(cfg), C.byref(self.h)), "nrg_open")
        L.check(lib.nrg_skiplist_prefill_range(self.h, PREFILL, 0))

    def round(self, p, W, g, R, gv, gf, resp, some):
        L.check(lib.nrg_skiplist_round_async(self.h, p, W, 1, resp, some))
        if R:
            L.check(lib.nrg_skiplist_get_async(self.h, g, R, gv, gf))

    def sync(self):
        L.check(lib.nrg_sync(self.h))

    def seek(self, k, n, ok, ov, f):
        L.check(lib.nrg_skiplist_seek_async(self.h, k, n, L.NRG_SEEK_GE, ok, ov, f))
        self.sync()

    def close(self):
        lib.nrg_close(self.h)


class Group:
    def __init__(self, moving):
        self.name = "moving" if moving else "identity"
        cfg = config()
        self.g = C.c_void_p()
        rc = lib.nrg_group_open((C.c_int * 1)(0), 1, C.byref(cfg), C.byref(self.g))
        if rc == L.NRG_E_COMM:  # no RCCL in this process: the in-process loopback collectives instead
            print(f"{self.name}: RCCL unavailable, using the loopback collectives", flush=True)
            L.check(lib.nrg_test_loopback_collectives(1))
            rc = lib.nrg_group_open((C.c_int * 1)(0), 1, C.byref(cfg), C.byref(self.g))
            L.check(lib.nrg_test_loopback_collectives(0))
        L.check(rc, "nrg_group_open")
        self.h = lib.nrg_group_replica(self.g, 0)
        if moving:
            L.check(lib.nrg_test_set_knob(self.h, L.KNOBS["EXP"], 0x10000))
        L.check(lib.nrg_skiplist_prefill_partition(self.h, PREFILL, 0, 0, 1))
        self.rd = L.Round()

    def round(self, p, W, g, R, gv, gf, resp, some):
        r = self.rd
        r.recs, r.n, r.resp, r.some = p, W, resp, some
        r.get_keys, r.n_gets, r.get_vals, r.get_found = (g if R else 0), R, gv, gf
        L.check(lib.nrg_group_partitioned_round(self.g, C.byref(r)), "partitioned round")

    def sync(self):
        L.check(lib.nrg_group_sync(self.g))

    def seek(self, k, n, ok, ov, f):
        q = L.Seek(k, n, ok, ov, f)
        L.check(lib.nrg_group_skiplist_seek(self.g, C.byref(q), L.NRG_SEEK_GE), "group seek")

    def close(self):
        lib.nrg_group_close(self.g)


def report(what, us):
    for name, xs in us.items():
        print(f"{what} {name:9s} median {statistics.median(xs):9.1f} us  (windows {min(xs):.1f} .. {max(xs):.1f})", flush=True)


def rounds(write_ratio, variants):
    W, R, puts, gets = batches(write_ratio)
    resp = torch.empty(max(W, 1), dtype=torch.int64, device="cuda")
    some = torch.empty(max(W, 1), dtype=torch.uint8, device="cuda")
    gv = torch.empty(max(R, 1), dtype=torch.int64, device="cuda")
    gf = torch.empty(max(R, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def one(v, b):
        v.round(puts[b].data_ptr(), W, gets[b % 4].data_ptr() if R else 0, R, gv.data_ptr(), gf.data_ptr(),
                resp.data_ptr(), some.data_ptr())

    for v in variants:
        for b in range(WARM):
            one(v, b)
        v.sync()
    us = {v.name: [] for v in variants}
    for w in range(WINDOWS):
        for v in variants:
            t = time.perf_counter()
            for r in range(ROUNDS):
                one(v, WARM + w * ROUNDS + r)
            v.sync()
            us[v.name].append((time.perf_counter() - t) * 1e6 / ROUNDS)
    report(f"round of {W} Push + {R} Get:", us)


def seeks(variants):
    rng = np.random.default_rng(99)
    k = torch.from_numpy(rng.integers(0, 2**64 - 1, N, dtype=np.uint64).view(np.int64)).cuda()
    ok = torch.empty(N, dtype=torch.int64, device="cuda")
    ov = torch.empty(N, dtype=torch.int64, device="cuda")
    f = torch.empty(N, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    us = {v.name: [] for v in variants}
    for w in range(WINDOWS + 1):
        for v in variants:
            t = time.perf_counter()
            for r in range(ROUNDS):
                v.seek(k.data_ptr(), N, ok.data_ptr(), ov.data_ptr(), f.data_ptr())
            if w:  # (the first window warms up)
                us[v.name].append((time.perf_counter() - t) * 1e6 / ROUNDS)
    report(f"seek (GE) of {N} keys, synchronous:", us)


def main():
    for wr in (10, 100):
        variants = [Direct(), Group(False), Group(True)]
        rounds(wr, variants)
        if wr == 100:
            seeks(variants)
        for v in variants:
            v.sync()
            v.close()


if __name__ == "__main__":
    main()
