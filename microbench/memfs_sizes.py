"""What file sizes cost a fused round of the replicated file store (nrg_memfs_enable_sizes; run on the
GPU box). The two shapes of microbench/memfs_round.py (generate_fs_operations, benches/memfs.rs:294-322:
N ops per round, default 2^20, 10 % Writes of 128 bytes, Reads of 0..127 bytes, offsets in 0..B-256,
shuffled; one 4 KiB file, and 1024 files of 4 KiB), three variants each:

  unsized      a context that never enabled sizes: mf_expand, line sort, mf_lines
  sized        sizes enabled, the same stream (no SetAttr): the file sort, the scan and mfs_lines run,
               nothing shrinks
  sized+1%     sizes enabled, 1 % of the records replaced by SetAttr to a size in B/2 .. B

The three contexts live side by side and take turns window by window (a window: ROUNDS rounds between
two stream events), WINDOWS times after a warm-up window each, so that a drift of the machine lands on
all of them; printed are the median and the range of each variant's windows. The per-kernel times are
the library's own event pairs (nrg_kernel_timing) in one more window per variant.
Usage: python microbench/memfs_sizes.py [N] [ROUNDS] [WINDOWS]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "node-replication_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nrgpu  # noqa: E402
from nrgpu import _lib as L  # noqa: E402

from memfs_round import LOG2_B, gen_ops  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
WINDOWS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
KERNELS = ("mf_expand", "mf_sort", "mf_lines", "mfs_keys", "mfs_sort", "mfs_reduce", "mfs_aggscan", "mfs_scan",
           "mfs_expand", "mfs_lines")


def with_setattr(recs, pct, seed):
    """`pct` % of the records become SetAttr to a size in B/2 .. B."""
    rng = np.random.default_rng(seed)
    r = recs.copy()
    pick = rng.random(len(r)) < pct / 100.0
    B = 1 << LOG2_B
    r["op"][pick] = L.NRG_MEMFS_SETATTR
    r["offset"][pick] = rng.integers(B // 2, B + 1, int(pick.sum()))
    r["len"][pick] = 0
    return r


class Variant:
    def __init__(self, name, files, sized, pct):
        ring = 1 << max(int(2 * N + 8192 - 1).bit_length(), 14)
        self.name = name
        self.dev = nrgpu.DeviceReplica(L.NRG_DS_MEMFS, 0, log2_slots=LOG2_B, queue_capacity=files, max_batch=N,
                                       log_bytes=64 * ring)
        if sized:
            self.dev.mf_enable_sizes()
        self.dev.use_torch_stream()
        recs = [gen_ops(N, files, 7 + s) for s in range(2)]
        if pct:
            recs = [with_setattr(r, pct, 70 + s) for s, r in enumerate(recs)]
        self.bufs = [torch.from_numpy(r.view(np.uint8).reshape(-1)).cuda() for r in recs]
        self.ms = []

    def window(self, d_resp, d_some, rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(rounds):
            self.dev.mf_round(self.bufs[i & 1], N, 1, d_resp, d_some)
        e1.record()
        e1.synchronize()
        self.dev.sync()
        return e0.elapsed_time(e1) / rounds


def run(files):
    vs = [Variant("unsized", files, False, 0), Variant("sized", files, True, 0), Variant("sized+1%", files, True, 1)]
    d_resp = torch.empty(N * 136, dtype=torch.uint8, device="cuda")
    d_some = torch.empty(N, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for v in vs:
        v.window(d_resp, d_some, 3)
    for _ in range(WINDOWS):
        for v in vs:  # taking turns
            v.ms.append(v.window(d_resp, d_some, ROUNDS))
    for v in vs:
        v.dev.kernel_timing(True)
        v.window(d_resp, d_some, ROUNDS)
        kt = []
        for k in KERNELS:
            launches, ms = v.dev.kernel_time(k)
            if launches:
                kt.append(f"{k} {ms / launches:.3f}")
        v.dev.kernel_timing(False)
        med = float(np.median(v.ms))
        print(f"memfs_sizes files={files} ops={N} rounds={ROUNDS} windows={WINDOWS} {v.name}: round median {med:.3f} ms "
              f"(range {min(v.ms):.3f} .. {max(v.ms):.3f}, {N / med / 1e3:.1f} Mops/s); per launch, ms: " + ", ".join(kt),
              flush=True)
    base = float(np.median(vs[0].ms))
    for v in vs[1:]:
        print(f"memfs_sizes files={files} {v.name} over unsized: x{float(np.median(v.ms)) / base:.3f}", flush=True)
    for v in vs:
        v.dev.close()


if __name__ == "__main__":
    if nrgpu.device_count() < 1:
        raise SystemExit("memfs_sizes: no HIP device visible")
    for files in (1, 1024):
        run(files)
