"""Time of one hashmap round with removal (nrg_hashmap_enable_removal; run on the GPU box).

B1-shaped rounds: W = 100k records and R = 900k Gets through nrg_hashmap_round_async on a table of 2^26
slots prefilled with 10M keys k -> k + 1 (NrHashMap::default). Cases: removal off (stamp rounds, the
headline's schedule), removal off with previous values requested (the partition round an enabled context
always takes), and removal on with 0, 1, 10 and 50 % of the records Remove(k), aimed at prefilled keys;
the other records are Puts of prefilled keys (a Put of a removed key revives its slot). ROUNDS
back-to-back rounds with fresh batches are timed between two stream events (pipeline = 1: a round's Gets
ride in the next round's first launch); a second pass with kernel timing on gives every kernel's mean
time per launch. The off, off + previous values and 0 % cases run three times, alternating, for the
spread. At the end: nrg_hashmap_purge of the table the 50 % case leaves (wall clock, synchronous: a rehash
of 2^26 slots into a fresh table of the same size), with the dead slots it drops.
Usage: python microbench/hm_remove.py [ROUNDS]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "node-replication_amd"))
import nrgpu  # noqa: E402
from nrgpu import _lib as L  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 24
W, R = 100_000, 900_000
LOG2, PREFILL = 26, 10_000_000
TOMB = 2**64 - 1
KERNELS = ("hm_round", "hm_papply")
NB = 2 * ROUNDS + 2


def batches(share, seed):
    out = []
    for b in range(NB):
        rng = np.random.default_rng(seed + b)
        recs = np.zeros(W, nrgpu.PUT_DTYPE)
        recs["key"] = rng.integers(0, PREFILL, W, dtype=np.uint64)
        recs["val"] = rng.integers(0, TOMB, W, dtype=np.uint64)
        recs["val"][rng.random(W) < share / 100.0] = TOMB
        gets = rng.integers(0, PREFILL, R, dtype=np.uint64)
        out.append((torch.from_numpy(recs.view(np.int64).copy()).cuda(), torch.from_numpy(gets.view(np.int64).copy()).cuda()))
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for r in range(ROUNDS):
        fn(r)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / ROUNDS


def case(label, enable, share, prev, seed, purge=False):
    dev = nrgpu.DeviceReplica(L.NRG_DS_HASHMAP, 0, log2_slots=LOG2, max_batch=W, max_reads=R, pipeline=1,
                              log_bytes=64 * 4 * max(W, 8192))
    dev.use_torch_stream()
    dev.hm_prefill_range(PREFILL, 1)
    if enable:
        dev.hm_enable_removal(TOMB)
    bt = batches(share, seed)
    gv = torch.empty(R, dtype=torch.int64, device="cuda")
    gf = torch.empty(R, dtype=torch.uint8, device="cuda")
    pv = torch.empty(W, dtype=torch.int64, device="cuda") if prev else None
    pf = torch.empty(W, dtype=torch.uint8, device="cuda") if prev else None

    def one(r):
        p, g = bt[r % NB]
        dev.hm_round_device(p, W, 1, g, R, gv, gf, pv, pf)

    for r in range(2):
        one(r)
    dev.join()
    torch.cuda.synchronize()
    us = timed(lambda r: one(2 + r))
    dev.kernel_timing(True)
    timed(lambda r: one(2 + ROUNDS + r))
    dev.join()
    dev.sync()
    cells = []
    for name in KERNELS:
        n, ms = dev.kernel_time(name)
        cells.append(f"{1000.0 * ms / n:.1f} x{n}" if n else "-")
    size, occ = dev.hm_size(), dev.hm_occupancy()
    print(f"| {label} | {us:.1f} | " + " | ".join(cells) + f" | {size} | {occ - size} |", flush=True)
    if purge:
        t0 = time.perf_counter()
        dev.hm_purge()
        ms = (time.perf_counter() - t0) * 1e3
        n, kms = dev.kernel_time("hm_rehash")
        print(f"purge of 2^{LOG2} slots, {size} live keys, {occ - size} dead slots dropped: {ms:.2f} ms wall clock, "
              f"hm_rehash {kms:.3f} ms x{n}; occupancy after = {dev.hm_occupancy()}", flush=True)
    dev.close()


print(f"W = {W}, R = {R}, 2^{LOG2} slots, {PREFILL} keys, ROUNDS = {ROUNDS}; us per round; per launch x launches")
print("| case | round | " + " | ".join(KERNELS) + " | keys at the end | dead slots |")
print("|---|---|" + "---|" * (len(KERNELS) + 2))
for rep in range(3):
    case("off", False, 0, False, 100)
    case("off, previous values", False, 0, True, 100)
    case("on, 0 %, no responses", True, 0, False, 100)
    case("on, 0 %", True, 0, True, 100)
for share in (1, 10, 50):
    case(f"on, {share} %", True, share, True, 1000 * share, purge=share == 50)
