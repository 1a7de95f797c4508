"""Logged writes of any length of the file store (nrg_memfs_pwrite_async; run on the GPU box) in three
shapes, each beside what a caller had before it: the same bytes as 128-byte Write records built on the
host, shipped, and replayed with nrg_memfs_round_async in rounds of max_batch records:
  (1) nrfs   benches/nrfs.rs:103-115 FileWrite: 1024 files of 4 KiB, one call writes every file whole from
             one shared 4096-byte buffer of 0x0b (nrfs.rs:55,68): 1024 requests, 32768 records; followed by
             one mf_pread of every file (checked)
  (2) file   one file of 64 MiB written whole: 1 request, 2^19 records
  (3) bytes  2^18 one-byte writes at random places of (1)'s store: 2^18 requests, 2^18 records

Per shape: WARM warm-up calls, then WINDOWS windows of ROUNDS calls, each window timed on the host from
the first call to the stream's completion (so the host's plan and upload are inside); the round time is
window / ROUNDS, reported as median and range over the windows. The per-kernel times are the library's
own event pairs (nrg_kernel_timing) in one more window: mf_frag per launch, and the replay kernels per
launch (a call replays its records in chunks of max_batch). The baseline's host encode (numpy, the
records of the whole shape), its copy to the device and its replay are timed separately, the replay the
same way as the round.
Usage: python microbench/memfs_pwrite.py [ROUNDS] [WINDOWS] [shape ...]
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

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
WINDOWS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
WARM = 2
MAX_BATCH = 1 << 18
KERNELS = ("mf_frag", "mf_expand", "mf_sort", "mf_lines")


def shape(name):
    rng = np.random.default_rng(7)
    if name == "nrfs":
        files, log2_b = 1024, 12
        rq = np.zeros(files, nrgpu.MEMFS_WR_DTYPE)
        rq["ino"] = L.NRG_MEMFS_FIRST_INO + np.arange(files)
        rq["len"] = 4096
        data = np.full(4096, 0x0B, np.uint8)
    elif name == "file":
        files, log2_b = 1, 26
        rq = np.zeros(1, nrgpu.MEMFS_WR_DTYPE)
        rq["ino"], rq["len"] = L.NRG_MEMFS_FIRST_INO, 1 << 26
        data = rng.integers(0, 256, 1 << 26, dtype=np.uint8)
    else:
        files, log2_b, n = 1024, 12, 1 << 18
        rq = np.zeros(n, nrgpu.MEMFS_WR_DTYPE)
        rq["ino"] = L.NRG_MEMFS_FIRST_INO + rng.integers(0, files, n)
        rq["offset"] = rng.integers(0, 4096, n)
        rq["len"] = 1
        rq["data_off"] = rng.integers(0, 4096, n)
        data = rng.integers(0, 256, 4096, dtype=np.uint8)
    return files, log2_b, rq, data


def encode(rq, data):
    """The baseline's records: every request cut into 128-byte Writes on the host, vectorised."""
    off, ln = rq["offset"].astype(np.int64), rq["len"].astype(np.int64)
    f = ((off + ln - 1) >> 7) - (off >> 7) + 1
    first = np.concatenate([[0], np.cumsum(f)])
    T = int(first[-1])
    r = np.repeat(np.arange(len(rq)), f)
    k = np.arange(T) - first[r]
    line = (off[r] >> 7) + k
    lo = np.maximum(line << 7, off[r])
    hi = np.minimum((line + 1) << 7, off[r] + ln[r])
    recs = np.zeros(T, nrgpu.MEMFS_OP_DTYPE)
    recs["ino"], recs["offset"], recs["len"] = rq["ino"][r], lo, hi - lo
    src = rq["data_off"].astype(np.int64)[r] + lo - off[r]
    idx = np.minimum(src[:, None] + np.arange(128)[None, :], len(data) - 1)
    recs["data"] = np.where(np.arange(128)[None, :] < (hi - lo)[:, None], data[idx], 0)
    return recs


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
    files, log2_b, rq, data = shape(name)
    n, nbytes = len(rq), int(rq["len"].sum())
    cfg = dict(log2_slots=log2_b, queue_capacity=files, max_batch=MAX_BATCH, max_reads=max(files, 1024), log_bytes=64 << 20)
    dev = nrgpu.DeviceReplica(L.NRG_DS_MEMFS, 0, **cfg)
    dev.use_torch_stream()
    d_data = torch.from_numpy(data).cuda()
    torch.cuda.synchronize()
    T = 0

    def call():
        nonlocal T
        T = dev.mf_pwrite_device(rq, d_data, len(data), 1)

    for _ in range(WARM):
        call()
    dev.sync()
    med, lo, hi = windows(call, dev.sync)
    if name == "nrfs":  # one mf_pread of every file: each reads back the shared buffer
        rd = np.zeros(files, nrgpu.MEMFS_RD_DTYPE)
        rd["ino"], rd["len"] = rq["ino"], 4096
        got, offs, some = dev.mf_pread(rd)
        dev.sync()
        assert bool((got == 0x0B).all()) and int(offs[-1].item()) == files * 4096 and int(some.sum().item()) == files
    dev.kernel_timing(True)
    for _ in range(ROUNDS):
        call()
    dev.sync()
    kt = {}
    for k in KERNELS:
        launches, ms = dev.kernel_time(k)
        kt[k] = (ms / max(launches, 1), launches // ROUNDS)
    dev.kernel_timing(False)
    want = dev.digest()
    dev.close()

    # the baseline: records built on the host, shipped, replayed in rounds of max_batch
    t0 = time.perf_counter()
    recs = encode(rq, data)
    t_enc = (time.perf_counter() - t0) * 1e3
    assert len(recs) == T
    base = nrgpu.DeviceReplica(L.NRG_DS_MEMFS, 0, **cfg)
    base.use_torch_stream()
    flat = recs.view(np.uint8).reshape(-1)
    t0 = time.perf_counter()
    d_recs = torch.from_numpy(flat).cuda()
    torch.cuda.synchronize()
    t_ship = (time.perf_counter() - t0) * 1e3

    def replay():
        for a in range(0, T, MAX_BATCH):
            m = min(MAX_BATCH, T - a)
            base.mf_round(d_recs[a * 152:(a + m) * 152], m, 1)

    for _ in range(WARM):
        replay()
    base.sync()
    bmed, blo, bhi = windows(replay, base.sync)
    assert base.digest() == want
    base.close()
    print(f"memfs_pwrite {name}: files={files} B={1 << log2_b} requests={n} bytes={nbytes} records={T} "
          f"rounds={ROUNDS} windows={WINDOWS}: round {med:.3f} ms [{lo:.3f}, {hi:.3f}] "
          f"({nbytes / med / 1e6:.2f} GB/s written); "
          + ", ".join(f"{k} {kt[k][0]:.3f} ms x {kt[k][1]}" for k in KERNELS)
          + f"; baseline: host encode {t_enc:.1f} ms, copy to device {t_ship:.1f} ms, "
          f"replay {bmed:.3f} ms [{blo:.3f}, {bhi:.3f}]", flush=True)


if __name__ == "__main__":
    if nrgpu.device_count() < 1:
        raise SystemExit("memfs_pwrite: no HIP device visible")
    for s in sys.argv[3:] or ("nrfs", "file", "bytes"):
        run(s)
