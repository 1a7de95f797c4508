"""Fused rounds of the replicated file store (nrg_memfs_round_async; run on the GPU box) in the shape
of generate_fs_operations (benches/memfs.rs:294-322): N ops per round (default 2^20), 10 % Writes of
128 bytes, Reads of 0..127 bytes, offsets in 0..B-256, shuffled; for one 4 KiB file (memfs.rs's own
shape: 32 lines, so 32 waves of mf_lines) and for 1024 files of 4 KiB (32768 lines).

Per configuration: WARM warm-up rounds, then a window of ROUNDS rounds between two stream events
(round time = window / ROUNDS), responses wanted, two record buffers taking turns; then the same
window again for the spread. The per-kernel times ("mf_expand", "mf_sort", "mf_lines") are the
library's own event pairs (nrg_kernel_timing) in a third window of their own, since the event
records sit between the timed kernels.
A last window per configuration runs the same rounds with no responses wanted (the Reads then
store nothing), to show what the responses cost.
Usage: python microbench/memfs_round.py [N] [ROUNDS]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "node-replication_amd"))
import nrgpu  # noqa: E402
from nrgpu import _lib as L  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
WARM = 3
LOG2_B = 12


def gen_ops(n, files, seed):
    """generate_fs_operations over `files` files: record idx is a Write where idx % 100 < 10."""
    rng = np.random.default_rng(seed)
    B = 1 << LOG2_B
    r = np.zeros(n, nrgpu.MEMFS_OP_DTYPE)
    wr = (np.arange(n) % 100) < 10
    r["ino"] = L.NRG_MEMFS_FIRST_INO + rng.integers(0, files, n)
    r["offset"] = rng.integers(0, B - 256, n)
    r["op"] = np.where(wr, L.NRG_MEMFS_WRITE, L.NRG_MEMFS_READ)
    r["len"] = np.where(wr, 128, rng.integers(0, 128, n))
    r["data"][wr] = 3
    return r[rng.permutation(n)]


def window(dev, bufs, d_resp, d_some, rounds):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(rounds):
        dev.mf_round(bufs[i & 1], N, 1, d_resp, d_some)
    e1.record()
    e1.synchronize()
    dev.sync()
    return e0.elapsed_time(e1) / rounds


def run(files):
    ring = 1 << max(int(2 * N + 8192 - 1).bit_length(), 14)
    dev = nrgpu.DeviceReplica(L.NRG_DS_MEMFS, 0, log2_slots=LOG2_B, queue_capacity=files, max_batch=N,
                              log_bytes=64 * ring)
    dev.use_torch_stream()
    bufs = [torch.from_numpy(gen_ops(N, files, 7 + s).view(np.uint8).reshape(-1)).cuda() for s in range(2)]
    d_resp = torch.empty(N * 136, dtype=torch.uint8, device="cuda")
    d_some = torch.empty(N, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    window(dev, bufs, d_resp, d_some, WARM)
    a = window(dev, bufs, d_resp, d_some, ROUNDS)
    b = window(dev, bufs, d_resp, d_some, ROUNDS)
    dev.kernel_timing(True)
    window(dev, bufs, d_resp, d_some, ROUNDS)
    kt = {}
    for k in ("mf_expand", "mf_sort", "mf_lines"):
        launches, ms = dev.kernel_time(k)
        kt[k] = ms / max(launches, 1)
    dev.kernel_timing(False)
    some = int(d_some.sum().item())
    c = window(dev, bufs, None, None, ROUNDS)
    lines = files * (1 << LOG2_B) // 128
    print(f"memfs_round files={files} B={1 << LOG2_B} lines={lines} ops={N} rounds={ROUNDS}: "
          f"round {a:.3f} ms / {b:.3f} ms ({N / a / 1e3:.1f} Mops/s); "
          f"mf_expand {kt['mf_expand']:.3f} ms, mf_sort {kt['mf_sort']:.3f} ms, mf_lines {kt['mf_lines']:.3f} ms; "
          f"some={some}/{N}; no responses wanted: round {c:.3f} ms", flush=True)
    dev.close()


if __name__ == "__main__":
    if nrgpu.device_count() < 1:
        raise SystemExit("memfs_round: no HIP device visible")
    for files in (1, 1024):
        run(files)
