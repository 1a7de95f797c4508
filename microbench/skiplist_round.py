"""Steady-state time of one skip-list round (nrg_skiplist_round_async + nrg_skiplist_get_async; run on
the GPU box), with the same Puts through a hashmap replica for scale.

Rounds shaped as generate_sops_concurrent (benches/lockfree.rs:128-154): N ops (default 1M) per round,
idx % 100 < write_ratio of them Push(random u64, random u64) and the rest Get(random u64), at 10 %
and 100 % writes, on a map prefilled with PREFILL keys i -> i (SkipListWrapper::default,
benches/lockfree_partitioned.rs:88-96; 2^22 is the reference's smokebench INITIAL_CAPACITY). Random
u64 keys are new keys, so the map grows by the round's writes. ROUNDS back-to-back rounds are timed
between two stream events, for several delta_max values (NRG_KNOB_SL_DELTA_MAX); a second pass with
kernel timing on gives sl_sort / sl_merge / sl_compact per launch. The compaction policy reads the
run counts (one synchronise) when its bound passes delta_max; that wait is inside the round time.
Usage: python microbench/skiplist_round.py [N] [ROUNDS] [delta_max ...]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "node-replication_amd"))
import nrgpu  # noqa: E402
from nrgpu import _lib as L  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 16
DELTAS = [int(a) for a in sys.argv[3:]] or [1 << 16, 1 << 18, 1 << 20, 1 << 22]
PREFILL = 1 << 22
LOG2 = 26
NB = 2 * ROUNDS + 2  # a fresh batch for every round of a run: random u64 keys are new keys


def batches(write_ratio):
    W = sum(1 for i in range(100) if i < write_ratio) * (N // 100)
    out, gl = [], []
    for b in range(NB):
        rng = np.random.default_rng(777 + 10 * write_ratio + b)
        recs = np.zeros(max(W, 1), nrgpu.PUT_DTYPE)
        recs["key"] = rng.integers(0, 2**64 - 1, max(W, 1), dtype=np.uint64)
        recs["val"] = rng.integers(0, 2**64 - 1, max(W, 1), dtype=np.uint64)
        if b < 4:  # (the Gets of four batches, used in turn)
            gets = torch.from_numpy(rng.integers(0, 2**64 - 1, max(N - W, 1), dtype=np.uint64).view(np.int64)).cuda()
            gl.append(gets)
        out.append((torch.from_numpy(recs.view(np.int64).copy()).cuda(), gl[b % 4]))
    return W, N - W, out


def bufs(R):
    return (torch.empty(N, dtype=torch.int64, device="cuda"), torch.empty(N, dtype=torch.uint8, device="cuda"),
            torch.empty(max(R, 1), dtype=torch.int64, device="cuda"), torch.empty(max(R, 1), dtype=torch.uint8, device="cuda"))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for r in range(ROUNDS):
        fn(r)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / ROUNDS


def skiplist(write_ratio, delta_max):
    W, R, bt = batches(write_ratio)
    dev = nrgpu.DeviceReplica(L.NRG_DS_SKIPLIST, 0, knobs={"SL_DELTA_MAX": delta_max}, log2_slots=LOG2, max_batch=N,
                              max_reads=N, log_bytes=64 * 4 * max(N, 8192))
    dev.use_torch_stream()
    dev.sl_prefill_range(PREFILL, 0)
    resp, some, gv, gf = bufs(R)

    def one(r):
        p, g = bt[r % NB]
        dev.sl_round_device(p, W, 1, resp, some)
        if R:
            dev.sl_get_device(g, R, gv, gf)

    for r in range(2):
        one(r)
    torch.cuda.synchronize()
    us = timed(lambda r: one(2 + r))
    dev.kernel_timing(True, only="sl_sort,sl_merge,sl_compact")
    timed(lambda r: one(2 + ROUNDS + r))
    parts = []
    for name in ("sl_sort", "sl_merge", "sl_compact"):
        n, ms = dev.kernel_time(name)
        parts.append(f"{name} {1000.0 * ms / n:.1f} us x {n}" if n else f"{name} not launched")
    print(f"skiplist writes={write_ratio}% delta_max=2^{delta_max.bit_length() - 1}: {us:.1f} us per round of {W} Push + {R} Get "
          f"over {ROUNDS} rounds, {dev.sl_len()} keys at the end; " + "; ".join(parts), flush=True)
    dev.sync()
    dev.close()


def hashmap(write_ratio):
    W, R, bt = batches(write_ratio)
    dev = nrgpu.DeviceReplica(L.NRG_DS_HASHMAP, 0, log2_slots=LOG2, max_batch=N, max_reads=N, log_bytes=64 * 4 * max(N, 8192))
    dev.use_torch_stream()
    dev.hm_prefill_range(PREFILL, 0)
    _, _, gv, gf = bufs(R)

    def one(r):
        p, g = bt[r % NB]
        dev.hm_round_device(p, W, 1, g if R else None, R, gv if R else None, gf if R else None)

    for r in range(2):
        one(r)
    torch.cuda.synchronize()
    us = timed(lambda r: one(2 + r))
    print(f"hashmap  writes={write_ratio}%: {us:.1f} us per round of {W} Put + {R} Get over {ROUNDS} rounds", flush=True)
    dev.sync()
    dev.close()


for wr in (10, 100):
    hashmap(wr)
    for dm in DELTAS:
        skiplist(wr, dm)
