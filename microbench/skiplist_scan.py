"""Batched range scans of the skip list (nrg_skiplist_scan_async, nrg_group_skiplist_scan; run on the
GPU box): the "sl_walk" kernel at limit 1, 16, 128 and 1024 beside the "sl_seek" kernel it duplicates
at limit 1, and the group-wide scan of a one-rank group (answering in place, and moving its data with
NRG_KNOB_EXP bit 16) and of a G = 8 group over the loopback collectives on this one GPU.

The map holds KEYS (default 2^22) random u64 keys, three quarters of every replica's share in its
base run and a quarter in its delta run, interleaved: the share is prefilled in four chunks of
max_batch with delta_max at two chunks, so the third chunk compacts and the fourth stays in delta.
Q (default 2^16) queries, half of them present keys and half random u64s, ascending (GE) and
descending (LE).
Kernel times are the library's own event pairs around each launch (nrg_kernel_timing), ITER launches
after a warm-up. A group call is synchronous; its time is a host clock around ROUNDS calls, the
median of WINDOWS windows with the lowest and highest beside it, the variants taking turns window by
window. The G = 8 group's members ask Q / 8 queries each, so that the candidate scratch
(G * nmax * limit entries) stays within the call's bound at limit 1024.
Usage: python microbench/skiplist_scan.py [KEYS] [Q] [ITER] [kernels|groups]
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
from nrgpu.parallel import key_owner  # noqa: E402

KEYS = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 22
Q = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 16
ITER = int(sys.argv[3]) if len(sys.argv) > 3 else 20
ONLY = sys.argv[4] if len(sys.argv) > 4 else ""
LIMITS = (1, 16, 128, 1024)
ROUNDS, WINDOWS = 4, 5
lib = L.load()
rng = np.random.default_rng(2024)
ALL_KEYS = np.unique(rng.integers(0, 2**64 - 1, KEYS, dtype=np.uint64))
rng.shuffle(ALL_KEYS)
QUERIES = np.concatenate([ALL_KEYS[rng.integers(0, len(ALL_KEYS), Q // 2)], rng.integers(0, 2**64 - 1, Q - Q // 2, dtype=np.uint64)])
rng.shuffle(QUERIES)


def log2_ceil(n):
    return max(int(n - 1).bit_length(), 4)


def chunk(share):
    return max((share + 3) // 4, 16)


def config(share):
    cfg = L.default_config(L.NRG_DS_SKIPLIST)
    cfg.log2_slots, cfg.max_batch, cfg.max_reads = log2_ceil(share) + 1, chunk(share), Q
    cfg.log_bytes = 64 * 4 * max(cfg.max_batch, 8192)
    return cfg


def fill(h, keys, max_batch):
    """three quarters into the base run, a quarter into the delta run (max_batch = chunk(share))"""
    L.check(lib.nrg_test_set_knob(h, L.KNOBS["SL_DELTA_MAX"], 2 * max_batch))
    vals = keys + np.uint64(1)
    L.check(lib.nrg_skiplist_prefill(h, keys.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), len(keys)))


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


def kernels():
    mb = chunk(len(ALL_KEYS))
    dev = nrgpu.DeviceReplica(L.NRG_DS_SKIPLIST, 0, log2_slots=log2_ceil(len(ALL_KEYS)) + 1, max_batch=mb, max_reads=Q,
                              log_bytes=64 * 4 * max(mb, 8192))
    fill(dev.handle, ALL_KEYS, mb)
    print(f"one replica: {dev.sl_len()} keys, {Q} queries, {ITER} timed launches per figure", flush=True)
    dq = cuda(QUERIES)
    ok = torch.empty(Q * max(LIMITS), dtype=torch.int64, device="cuda")
    ov = torch.empty_like(ok)
    cnt = torch.empty(Q, dtype=torch.int32, device="cuda")
    found = torch.empty(Q, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for mode, name in ((L.NRG_SEEK_GE, "GE"), (L.NRG_SEEK_LE, "LE")):
        def seek():
            L.check(lib.nrg_skiplist_seek_async(dev.handle, dq.data_ptr(), Q, mode, ok.data_ptr(), ov.data_ptr(), found.data_ptr()))

        def walk(limit):
            L.check(lib.nrg_skiplist_scan_async(dev.handle, dq.data_ptr(), Q, mode, limit, ok.data_ptr(), ov.data_ptr(),
                                                cnt.data_ptr()))

        for what, fn, kname in [("seek", seek, "sl_seek")] + [(f"walk limit {lim}", (lambda lim=lim: walk(lim)), "sl_walk")
                                                               for lim in LIMITS]:
            for _ in range(3):
                fn()
            dev.sync()
            dev.kernel_timing(True, only=kname)
            n0, ms0 = dev.kernel_time(kname)
            for _ in range(ITER):
                fn()
            dev.sync()
            n1, ms1 = dev.kernel_time(kname)
            dev.kernel_timing(False)
            us = 1000.0 * (ms1 - ms0) / max(n1 - n0, 1)
            entries = int(cnt.sum().item()) if kname == "sl_walk" else int(found.sum().item())
            print(f"  {name} {what:16s} {kname}: {us:9.1f} us per launch ({n1 - n0} launches), {entries} entries, "
                  f"{entries * 16 / max(us, 1e-9) / 1e3:.1f} GB/s of entries written", flush=True)
    dev.close()


class Group:
    def __init__(self, name, G, moving=False):
        self.name, self.G = name, G
        own = key_owner(ALL_KEYS, G)
        shares = [np.ascontiguousarray(ALL_KEYS[own == p]) for p in range(G)]
        cfg = config(max(len(s) for s in shares))
        L.check(lib.nrg_test_loopback_collectives(1))
        self.g = C.c_void_p()
        try:
            L.check(lib.nrg_group_open((C.c_int * G)(*([0] * G)), G, C.byref(cfg), C.byref(self.g)), "nrg_group_open")
        finally:
            L.check(lib.nrg_test_loopback_collectives(0))
        for p in range(G):
            h = lib.nrg_group_replica(self.g, p)
            fill(h, shares[p], cfg.max_batch)
            if moving:
                L.check(lib.nrg_test_set_knob(h, L.KNOBS["EXP"], 0x10000))
        n = Q // G
        self.n = n
        self.q = [cuda(QUERIES[p * n:(p + 1) * n]) for p in range(G)]
        self.ok = [torch.empty(n * max(LIMITS), dtype=torch.int64, device="cuda") for _ in range(G)]
        self.ov = [torch.empty_like(t) for t in self.ok]
        self.cnt = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(G)]
        self.sc = (L.Scan * G)()
        for p in range(G):
            s = self.sc[p]
            s.keys, s.n, s.out_keys, s.out_vals, s.counts = (self.q[p].data_ptr(), n, self.ok[p].data_ptr(),
                                                             self.ov[p].data_ptr(), self.cnt[p].data_ptr())

    def scan(self, mode, limit):
        L.check(lib.nrg_group_skiplist_scan(self.g, self.sc, mode, limit), "group scan")

    def close(self):
        lib.nrg_group_close(self.g)


def groups():
    variants = [Group("G=1 identity", 1), Group("G=1 moving", 1, True), Group("G=8 loopback", 8)]
    torch.cuda.synchronize()
    print(f"group-wide scan, synchronous, {Q} queries in all (G = 8: {Q // 8} per member); median of {WINDOWS} windows of "
          f"{ROUNDS} calls", flush=True)
    for mode, name in ((L.NRG_SEEK_GE, "GE"), (L.NRG_SEEK_LE, "LE")):
        for limit in LIMITS:
            us = {v.name: [] for v in variants}
            for w in range(WINDOWS + 1):
                for v in variants:
                    t = time.perf_counter()
                    for _ in range(ROUNDS):
                        v.scan(mode, limit)
                    if w:  # (the first window warms up)
                        us[v.name].append((time.perf_counter() - t) * 1e6 / ROUNDS)
            for v in variants:
                xs = us[v.name]
                print(f"  {name} limit {limit:4d} {v.name:13s} median {statistics.median(xs):10.1f} us  "
                      f"(windows {min(xs):.1f} .. {max(xs):.1f})", flush=True)
    for v in variants:
        v.close()


if __name__ == "__main__":
    if ONLY in ("", "kernels"):
        kernels()
    if ONLY in ("", "groups"):
        groups()
