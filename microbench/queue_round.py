"""Steady-state time of one fused queue round (nrg_queue_round_async; run on the GPU box).

Rounds of N ops (default 1M) of a seeded 50/50 Push/Pop stream on a queue prefilled with 2M
elements (SegQueueWrapper::default pushes 0..n-1, benches/lockfree_comparisons.rs:80-88). Every
batch holds exactly N/2 Pushes in a seeded random order, so the length is back at 2M after each
round and the window can be long. ROUNDS back-to-back rounds are timed between two stream events,
WINDOWS times, with and without response buffers; the byte ledger is what the shipped launch
structure moves by construction.
Usage: python microbench/queue_round.py [N] [ROUNDS] [WINDOWS]
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
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
WINDOWS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
PREFILL = 2_000_000
NB = 4  # distinct batches, used in turn

dev = nrgpu.DeviceReplica(L.NRG_DS_QUEUE, 0, max_batch=N, queue_capacity=1 << 22, log_bytes=64 * 4 * max(N, 8192))
dev.use_torch_stream()
dev.qu_init_range(PREFILL)
batches = []
for b in range(NB):
    rng = np.random.default_rng(12345 + b)
    recs = np.zeros(N, nrgpu.QUEUE_OP_DTYPE)
    recs["val"] = rng.integers(0, 2**64 - 1, N, dtype=np.uint64)
    ops = np.zeros(N, np.uint64)
    ops[: N // 2] = 1
    recs["op"] = rng.permutation(ops)
    batches.append(torch.from_numpy(recs.view(np.int64).copy()).cuda())
resps = [torch.empty(N, dtype=torch.int64, device="cuda") for _ in range(2)]
somes = [torch.empty(N, dtype=torch.uint8, device="cuda") for _ in range(2)]


def window(with_resp):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for r in range(ROUNDS):
        if with_resp:
            dev.qu_round_device(batches[r % NB], N, 1, resps[r & 1], somes[r & 1])
        else:
            dev.qu_round_device(batches[r % NB], N, 1)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / ROUNDS


for _ in range(20):  # warm-up: code objects, both response buffers, every batch
    dev.qu_round_device(batches[_ % NB], N, 1, resps[_ & 1], somes[_ & 1])
torch.cuda.synchronize()
assert dev.qu_len() == PREFILL

pushes = N // 2
ledger = {
    "ops read (aggregate pass)": 16 * N,
    "ops read (tile pass)": 16 * N,
    "log copy": 16 * N,
    "Push writes": 8 * pushes,
    "Pop reads (tile pass)": 8 * (N - pushes),
    "responses (u64 + u8)": 9 * N,
}
total = sum(ledger.values())
no_resp = total - ledger["responses (u64 + u8)"] - ledger["Pop reads (tile pass)"]
for k, v in ledger.items():
    print(f"  {k:28s} {v / 1e6:8.2f} MB")
print(f"  total {total / 1e6:.2f} MB with responses, {no_resp / 1e6:.2f} MB without")
for with_resp, nbytes in ((True, total), (False, no_resp)):
    us = [window(with_resp) for _ in range(WINDOWS)]
    best = min(us)
    print(f"N={N} responses={'yes' if with_resp else 'no'}: " + " ".join(f"{u:.2f}" for u in us) +
          f" us per round over {ROUNDS} rounds; best {best:.2f} us = {nbytes / best / 1e6:.2f} TB/s "
          f"({100.0 * nbytes / best / 1e6 / 8.0:.1f}% of 8 TB/s)")
assert dev.qu_len() == PREFILL
dev.sync()
dev.close()
