"""Logged reads of any length of the file store (nrg_memfs_pread_logged_async; run on the GPU box) in
three shapes, each beside the same bytes through the unlogged nrg_memfs_pread_async and beside what a
caller had before for a logged read: the same T single-line Read records through nrg_memfs_round_async in
rounds of max_batch, with the 136-byte responses copied back and folded on the host:
  (1) nrfs   2^16 whole-file reads over 1024 files of 4 KiB (benches/nrfs.rs's shape, but logged):
             2^16 requests, 2^21 records, 256 MiB
  (2) big    2^12 reads of 64 KiB over 64 files of 64 KiB: 2^12 requests, 2^21 records, 256 MiB
  (3) skew   one 64-MiB read beside 2^16 one-byte reads: 2^16 + 1 requests, 2^19 + 2^16 records

Per shape: WARM warm-up calls, then WINDOWS windows of ROUNDS calls, each window timed on the host from
the first call to the stream's completion (so the host's plan and upload are inside); the call time is
window / ROUNDS, reported as median and range over the windows. The per-kernel times are the library's
own event pairs (nrg_kernel_timing) in one more window, per launch, with the launches per call. The
baseline's copy of the responses to the host and its fold (numpy, vectorised) are timed once each.
Usage: python microbench/memfs_pread_logged.py [ROUNDS] [WINDOWS] [shape ...]
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

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
WINDOWS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
WARM = 2
MAX_BATCH = 1 << 18
KERNELS = ("mf_rfrag", "mf_expand", "mf_sort", "mf_lines", "mf_rgather", "mf_rcount")


def shape(name):
    rng = np.random.default_rng(7)
    F0 = L.NRG_MEMFS_FIRST_INO
    if name == "nrfs":
        files, log2_b, n = 1024, 12, 1 << 16
        rq = np.zeros(n, nrgpu.MEMFS_RD_DTYPE)
        rq["ino"], rq["len"] = F0 + np.arange(n) % files, 4096
    elif name == "big":
        files, log2_b, n = 64, 16, 1 << 12
        rq = np.zeros(n, nrgpu.MEMFS_RD_DTYPE)
        rq["ino"], rq["len"] = F0 + np.arange(n) % files, 1 << 16
    else:
        files, log2_b, n = 2, 26, (1 << 16) + 1
        rq = np.zeros(n, nrgpu.MEMFS_RD_DTYPE)
        rq["ino"][0], rq["len"][0] = F0, 1 << 26
        rq["ino"][1:], rq["len"][1:] = F0 + 1, 1
        rq["offset"][1:] = rng.integers(0, 1 << 26, n - 1)
    return files, log2_b, rq


def windows(fn, sync):
    out = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(ROUNDS):
            fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3 / ROUNDS)
    return float(np.median(out)), min(out), max(out)


def run(name):
    files, log2_b, rq = shape(name)
    n = len(rq)
    cfg = dict(log2_slots=log2_b, queue_capacity=files, max_batch=MAX_BATCH, max_reads=max(n, 1024), log_bytes=64 << 20)
    dev = nrgpu.DeviceReplica(L.NRG_DS_MEMFS, 0, **cfg)
    dev.use_torch_stream()
    # something to read: a write of patterned bytes over the head of every file
    pat = torch.from_numpy(np.random.default_rng(3).integers(2, 256, 4096, dtype=np.uint8)).cuda()
    wr = np.zeros(files, nrgpu.MEMFS_WR_DTYPE)
    wr["ino"], wr["len"] = L.NRG_MEMFS_FIRST_INO + np.arange(files), 4096
    dev.mf_pwrite_device(wr, pat, 4096, 1)
    first, offs, _ = nrgpu.memfs_pread_logged_plan(log2_b, files, rq)
    T, nbytes = int(first[-1]), int(offs[-1])
    d_data = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    d_counts = torch.empty(n, dtype=torch.int64, device="cuda")
    d_some = torch.empty(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def call():
        dev.mf_pread_logged_device(rq, 1, d_data, nbytes, d_counts, d_some)

    for _ in range(WARM):
        call()
    dev.sync()
    med, lo, hi = windows(call, dev.sync)
    dev.kernel_timing(True)
    for _ in range(ROUNDS):
        call()
    dev.sync()
    kt = {}
    for k in KERNELS:
        launches, ms = dev.kernel_time(k)
        kt[k] = (ms / max(launches, 1), launches // ROUNDS)
    dev.kernel_timing(False)

    # the same bytes through the unlogged pread
    d_rq = torch.from_numpy(rq.view(np.uint8).copy()).cuda()
    p_data = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    p_offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    p_some = torch.empty(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def pread():
        dev.mf_pread_device(d_rq, n, p_data, nbytes, p_offs, p_some)

    for _ in range(WARM):
        pread()
    dev.sync()
    pmed, plo, phi = windows(pread, dev.sync)
    assert torch.equal(d_data, p_data) and int(d_counts.sum().item()) == nbytes == int(p_offs[-1].item())

    # what a caller had before: the T single-line Read records through rounds, responses folded on the host
    d_recs = dev.mf_pread_logged_records(rq, device=True)
    d_resp = torch.empty(T * 136, dtype=torch.uint8, device="cuda")
    d_rs = torch.empty(T, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def rounds():
        for a in range(0, T, MAX_BATCH):
            m = min(MAX_BATCH, T - a)
            dev.mf_round(d_recs[a * 152:(a + m) * 152], m, 1, d_resp[a * 136:(a + m) * 136], d_rs[a:a + m])

    for _ in range(WARM):
        rounds()
    dev.sync()
    bmed, blo, bhi = windows(rounds, dev.sync)
    t0 = time.perf_counter()
    resp = d_resp.cpu().numpy().view(nrgpu.MEMFS_RESP_DTYPE)
    t_copy = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    folded = resp["data"][np.arange(128, dtype=np.int64)[None, :] < resp["n"].astype(np.int64)[:, None]]
    t_fold = (time.perf_counter() - t0) * 1e3
    assert folded.tobytes() == d_data.cpu().numpy().tobytes()
    dev.close()
    print(f"memfs_pread_logged {name}: files={files} B={1 << log2_b} requests={n} bytes={nbytes} records={T} "
          f"rounds={ROUNDS} windows={WINDOWS}: call {med:.3f} ms [{lo:.3f}, {hi:.3f}] "
          f"({nbytes / med / 1e6:.2f} GB/s read); "
          + ", ".join(f"{k} {kt[k][0]:.3f} ms x {kt[k][1]}" for k in KERNELS)
          + f"; unlogged pread {pmed:.3f} ms [{plo:.3f}, {phi:.3f}]"
          + f"; before: rounds of single-line Reads {bmed:.3f} ms [{blo:.3f}, {bhi:.3f}], responses to the host "
          f"{t_copy:.1f} ms, host fold {t_fold:.1f} ms", flush=True)


if __name__ == "__main__":
    if nrgpu.device_count() < 1:
        raise SystemExit("memfs_pread_logged: no HIP device visible")
    for s in sys.argv[3:] or ("nrfs", "big", "skew"):
        run(s)
