"""Time of one skip-list round with removal (nrg_skiplist_enable_removal; run on the GPU box).

A round of N records (default 1M) through nrg_skiplist_round_async on a map prefilled with PREFILL =
2^22 keys i -> i (SkipListWrapper::default). With delta_max = 2^20 and chunks of N the prefill leaves
the keys below BASE_END in the base run and the rest in the delta run. Cases: removal off (every record
a Push of a key below PREFILL: an update), and removal on with 0, 1, 10 and 50 % of the records
Remove(k), the Removes aimed at keys of the base run only, of the delta run only, or of both; the
other records are Pushes as before (a Push of a removed key is a new key again). ROUNDS back-to-back
rounds with fresh batches are timed between two stream events; a second pass with kernel timing on
gives every kernel's mean time per launch and its launches (nrg_kernel_time). "sl_rm_state" is the
state readback of an enabled context, one per chunk: at 0 % it, sl_rm_resp and the two more scans of
sl_scan are all that removal costs. The off and 0 % cases run three times, alternating, for the spread.
Usage: python microbench/skiplist_remove.py [N] [ROUNDS]
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
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 24
PREFILL = 1 << 22
DELTA_MAX = 1 << 20
LOG2 = 23
TOMB = 2**64 - 1
KERNELS = ("sl_stream", "sl_sort", "sl_rm_resp", "sl_resolve", "sl_scan", "sl_scatter", "sl_rm_state", "sl_drop_base",
           "sl_drop_delta", "sl_merge", "sl_compact")
NB = 2 * ROUNDS + 2


def batches(share, lo, hi, seed):
    out = []
    for b in range(NB):
        rng = np.random.default_rng(seed + b)
        recs = np.zeros(N, nrgpu.PUT_DTYPE)
        recs["key"] = rng.integers(0, PREFILL, N, dtype=np.uint64)
        recs["val"] = rng.integers(0, TOMB, N, dtype=np.uint64)
        rm = rng.random(N) < share / 100.0
        recs["key"][rm] = rng.integers(lo, hi, int(rm.sum()), dtype=np.uint64)
        recs["val"][rm] = TOMB
        out.append(torch.from_numpy(recs.view(np.int64).copy()).cuda())
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for r in range(ROUNDS):
        fn(r)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / ROUNDS


def case(label, enable, share, lo, hi, seed):
    dev = nrgpu.DeviceReplica(L.NRG_DS_SKIPLIST, 0, knobs={"SL_DELTA_MAX": DELTA_MAX}, log2_slots=LOG2, max_batch=N,
                              log_bytes=64 * 4 * max(N, 8192))
    dev.use_torch_stream()
    dev.sl_prefill_range(PREFILL, 0)
    if enable:
        dev.sl_enable_removal(TOMB)
    bt = batches(share, lo, hi, seed)
    resp = torch.empty(N, dtype=torch.int64, device="cuda")
    some = torch.empty(N, dtype=torch.uint8, device="cuda")

    def one(r):
        dev.sl_round_device(bt[r % NB], N, 1, resp, some)

    for r in range(2):
        one(r)
    torch.cuda.synchronize()
    us = timed(lambda r: one(2 + r))
    dev.kernel_timing(True)
    timed(lambda r: one(2 + ROUNDS + r))
    cells = []
    for name in KERNELS:
        n, ms = dev.kernel_time(name)
        cells.append(f"{1000.0 * ms / n:.0f} x{n}" if n else "-")
    print(f"| {label} | {us:.0f} | " + " | ".join(cells) + f" | {dev.sl_len()} |", flush=True)
    dev.sync()
    dev.close()


def base_end():
    """where the prefill's last compaction left the base run (chunks of N keys, compaction when nd > delta_max)"""
    nb = nd = 0
    for at in range(0, PREFILL, N):
        nd += min(N, PREFILL - at)
        if nd > DELTA_MAX:
            nb, nd = nb + nd, 0
    return nb


BASE_END = base_end()
print(f"N = {N}, ROUNDS = {ROUNDS}, prefill 2^22: base run [0, {BASE_END}), delta run [{BASE_END}, {PREFILL}); times in us "
      "(per round; per launch x launches over the timed rounds)")
print("| case | round | " + " | ".join(k[3:] for k in KERNELS) + " | keys at the end |")
print("|---|---|" + "---|" * (len(KERNELS) + 1))
for rep in range(3):
    case("off", False, 0, 0, 1, 100)
    case("on, 0 %", True, 0, 0, 1, 100)
for share in (1, 10, 50):
    for tag, lo, hi in (("base", 0, BASE_END), ("delta", BASE_END, PREFILL), ("mixed", 0, PREFILL)):
        if lo < hi:
            case(f"on, {share} % {tag}", True, share, lo, hi, 1000 * share + lo % 97)
