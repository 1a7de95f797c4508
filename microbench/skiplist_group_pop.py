"""The group-wide pop of a partitioned skip-list group (nrg_group_skiplist_pop) and a Remove-carrying
partitioned round beside a Push-only one (run on the GPU box).

Pop: one PopFront x F per call on rank 0 (the other ranks pass no request), after a Push round that puts
F fresh keys back, so the map keeps its size; a call is synchronous. Variants, taking turns window by
window so that drift hits all of them alike:
  identity  a one-rank group: its own pop step answers straight into the caller's buffers
  moving    the same with NRG_KNOB_EXP bit 16: candidates, all-gather, select, replay of two records
  G = 8     eight members on one GPU over the in-process loopback collectives: an upper bound of the
            work and no estimate of eight GPUs (the members take turns on the device)
A window is CALLS calls between a host clock's two readings; the refill rounds run outside the clock. The
figure per variant is the median window, with the lowest and highest beside it.
Rounds: N records per round from rank 0 of a one-rank group in both forms, all Push, or half of them
Remove(k) of keys pushed the round before (a group that agreed on removal: the owners answer), with
responses asked; ROUNDS rounds per window closed by a synchronise.
Usage: python microbench/skiplist_group_pop.py [N] [CALLS] [WINDOWS]
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

N = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 4
WINDOWS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
PREFILL = 1 << 20
LOG2 = 22
FS = (1, 1024, 65536)
TOMB, FRONT, BACK = 2**64 - 1, 2**64 - 2, 2**64 - 3
lib = L.load()


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


class Group:
    def __init__(self, name, G, moving=False, removal=False, pops=True):
        self.name, self.G = name, G
        cfg = L.default_config(L.NRG_DS_SKIPLIST)
        cfg.log2_slots, cfg.max_batch, cfg.max_reads = LOG2, max(N, max(FS)), 8192
        cfg.log_bytes = 64 * 4 * max(N, 8192)
        self.g = C.c_void_p()
        devs = (C.c_int * G)(*([0] * G))
        rc = L.NRG_E_COMM if G > 1 else lib.nrg_group_open(devs, G, C.byref(cfg), C.byref(self.g))
        if rc == L.NRG_E_COMM:  # several members on one GPU, or no RCCL in this process: the loopback collectives
            L.check(lib.nrg_test_loopback_collectives(1))
            rc = lib.nrg_group_open(devs, G, C.byref(cfg), C.byref(self.g))
            L.check(lib.nrg_test_loopback_collectives(0))
        L.check(rc, "nrg_group_open")
        self.h = [lib.nrg_group_replica(self.g, i) for i in range(G)]
        for p, h in enumerate(self.h):
            if moving:
                L.check(lib.nrg_test_set_knob(h, L.KNOBS["EXP"], 0x10000))
            L.check(lib.nrg_skiplist_prefill_partition(h, PREFILL, 0, p, G))
        if removal:
            L.check(lib.nrg_group_skiplist_enable_removal(self.g, TOMB), "enable_removal")
        if pops:
            L.check(lib.nrg_group_skiplist_enable_pops(self.g, FRONT, BACK), "enable_pops")
        self.rd = (L.Round * G)()
        self.dummy = torch.zeros(8, dtype=torch.int64, device="cuda")
        for i in range(G):
            self.rd[i].get_vals = self.rd[i].get_found = self.dummy.data_ptr()

    def round(self, recs, n, resp=0, some=0):
        r = self.rd[0]
        r.recs, r.n, r.resp, r.some = recs, n, resp, some
        L.check(lib.nrg_group_partitioned_round(self.g, self.rd), "partitioned round")

    def sync(self):
        L.check(lib.nrg_group_sync(self.g))

    def pop(self, q):
        L.check(lib.nrg_group_skiplist_pop(self.g, q), "group pop")

    def close(self):
        lib.nrg_group_close(self.g)


def report(what, us):
    for name, xs in us.items():
        print(f"{what} {name:9s} median {statistics.median(xs):9.1f} us  (windows {min(xs):.1f} .. {max(xs):.1f})", flush=True)


def pops(variants, F):
    """PopFront x F on rank 0; the F smallest keys are pushed back before every call (outside the clock)"""
    refill = cuda(np.stack([np.arange(F, dtype=np.uint64), np.arange(F, dtype=np.uint64)], 1))
    resp = torch.zeros(1, dtype=torch.int64, device="cuda")
    some = torch.zeros(1, dtype=torch.uint8, device="cuda")
    keys = torch.zeros(F, dtype=torch.int64, device="cuda")
    vals = torch.zeros(F, dtype=torch.int64, device="cuda")
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    req = (L.PopReq * 1)(L.PopReq(F, 0, 0))
    torch.cuda.synchronize()
    qs = {}
    for v in variants:
        q = (L.Pops * v.G)()
        q[0].reqs, q[0].n, q[0].resp, q[0].some = req, 1, resp.data_ptr(), some.data_ptr()
        q[0].pop_keys, q[0].pop_vals, q[0].pop_cap, q[0].pop_n = keys.data_ptr(), vals.data_ptr(), F, total.data_ptr()
        qs[v.name] = q
    us = {v.name: [] for v in variants}
    for w in range(WINDOWS + 1):
        for v in variants:
            spent = 0.0
            for c in range(CALLS):
                t = time.perf_counter()
                v.pop(qs[v.name])
                spent += time.perf_counter() - t
                assert int(total.item()) == F and int(keys[F - 1].item()) == F - 1
                v.round(refill.data_ptr(), F)
                v.sync()
            if w:  # (the first window warms up)
                us[v.name].append(spent * 1e6 / CALLS)
    report(f"group pop, PopFront x {F}, synchronous:", us)


def rounds(variants):
    """N records per round: all Push, or Push / Remove(previous round's key) alternating, responses asked"""
    ROUNDS = 6
    nb = 2 + ROUNDS * (WINDOWS + 1)
    rng = np.random.default_rng(7)
    fresh = [rng.integers(1 << 32, 2**63, N, dtype=np.uint64) for _ in range(nb + 1)]
    resp = torch.empty(N, dtype=torch.int64, device="cuda")
    some = torch.empty(N, dtype=torch.uint8, device="cuda")
    for mix in ("push", "push+remove"):
        batches = []
        for b in range(nb):
            k, v = fresh[b + 1].copy(), fresh[b + 1] >> np.uint64(1)
            if mix == "push+remove":
                k[1::2], v[1::2] = fresh[b][::2][:len(k[1::2])], TOMB  # half the records remove the previous round's pushes
            batches.append(cuda(np.stack([k, v], 1)))
        torch.cuda.synchronize()
        us = {v.name: [] for v in variants}
        at = {v.name: 0 for v in variants}
        for w in range(WINDOWS + 1):
            for v in variants:
                t = time.perf_counter()
                for r in range(ROUNDS):
                    v.round(batches[at[v.name]].data_ptr(), N, resp.data_ptr(), some.data_ptr())
                    at[v.name] += 1
                v.sync()
                if w:
                    us[v.name].append((time.perf_counter() - t) * 1e6 / ROUNDS)
        report(f"round of {N} records ({mix}), responses asked:", us)


def main():
    variants = [Group("identity", 1), Group("moving", 1, moving=True), Group("G = 8", 8)]
    for F in FS:
        pops(variants, F)
    for v in variants:
        v.sync()
        v.close()
    variants = [Group("identity", 1, removal=True, pops=False), Group("moving", 1, moving=True, removal=True, pops=False)]
    rounds(variants)
    for v in variants:
        v.sync()
        v.close()


if __name__ == "__main__":
    main()
