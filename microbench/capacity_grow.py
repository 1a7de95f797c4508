"""Time of the three reserve calls, once per size; run on the GPU box.

  stack   nrg_stack_reserve   2^24 -> 2^25 elements, the stack full (64 MiB live)
  queue   nrg_queue_reserve   2^24 -> 2^25 elements, the queue full (128 MiB live; max_batch 2^16, so
                              the ring goes from 2^25 to 2^26 slots), the front in the middle of the ring
  vspace  nrg_vspace_reserve  2^18 -> 2^20 tables after one bench-shaped round of 3000 ops (about
                              10^5 tables allocated), the rest of the new pool zeroed

Each call is timed once on the host (it allocates, launches, synchronises and frees) and its kernel
by nrg_kernel_timing. The yardstick, in the same run: a plain device-to-device hipMemcpy of the live
bytes and a hipMemset of the remainder of a buffer of the new size, between two stream events, the
second of three repeats. The stack's and the queue's kernels leave the remainder alone; the page
table's zeroes it.
Usage: python microbench/capacity_grow.py
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "node-replication_amd"))
import nrgpu  # noqa: E402
from nrgpu import _lib as L  # noqa: E402

D2D = 3  # hipMemcpyDeviceToDevice


def hip_runtime():
    """the HIP runtime the process already holds (torch's), by SONAME"""
    for name in ("libamdhip64.so.7", "libamdhip64.so.6", "libamdhip64.so"):
        try:
            h = C.CDLL(name)
        except OSError:
            continue
        h.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        h.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
        return h
    raise OSError("no libamdhip64")


HIP = hip_runtime()


def yardstick(live, total):
    """(memcpy ms, memcpy + memset ms) for `live` bytes copied into a buffer of `total` bytes"""
    src = torch.empty(live, dtype=torch.uint8, device="cuda").fill_(1)
    dst = torch.empty(total, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    out = None
    for rep in range(3):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        assert HIP.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), live, D2D, None) == 0
        e[1].record()
        if total > live:
            assert HIP.hipMemsetAsync(dst.data_ptr() + live, 0, total - live, None) == 0
        e[2].record()
        torch.cuda.synchronize()
        if rep == 1:
            out = (e[0].elapsed_time(e[1]), e[0].elapsed_time(e[2]))
    del src, dst
    torch.cuda.empty_cache()
    return out


def report(name, what, live, total, host_ms, dev, kernel):
    n, ms = dev.kernel_time(kernel)
    k_ms = ms / n if n else float("nan")
    cp, cpset = yardstick(live, total)
    print(f"{name}: {what}")
    print(f"  reserve call          {host_ms:9.3f} ms (host: allocate, launch, synchronise, free)")
    print(f"  {kernel:10s} kernel     {k_ms:9.3f} ms: {live / 1e6:.1f} MB live = {2 * live / k_ms / 1e9:.2f} TB/s read + written"
          f" (buffer of {total / 1e6:.1f} MB)")
    print(f"  hipMemcpy of the live {cp:9.3f} ms = {2 * live / cp / 1e9:.2f} TB/s; with hipMemset of the other "
          f"{(total - live) / 1e6:.1f} MB {cpset:9.3f} ms")


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


# ---- stack -----------------------------------------------------------------------------------------
N0, N1 = 1 << 24, 1 << 25
st = nrgpu.DeviceReplica(L.NRG_DS_STACK, 0, stack_capacity=N0, max_batch=1 << 16)
vals = np.arange(N0, dtype=np.uint32) * np.uint32(2654435761)
st.st_init(vals)
d0 = st.digest()
st.kernel_timing(True)
ms = timed(lambda: st.st_reserve(N1))
assert st.st_capacity() == N1 and st.st_len() == N0 and st.digest() == d0
report("stack", f"2^24 -> 2^25 elements, {N0} live", N0 * 4, N1 * 4, ms, st, "st_grow")
st.close()

# ---- queue -----------------------------------------------------------------------------------------
MB = 1 << 16
qu = nrgpu.DeviceReplica(L.NRG_DS_QUEUE, 0, queue_capacity=N0, max_batch=MB)
qu.qu_init_range(N0)
# move the front to the middle of the ring (2^25 slots): rounds of max_batch Pops then Pushes
ops = np.zeros(MB, nrgpu.QUEUE_OP_DTYPE)
ops["op"][MB // 2:] = L.NRG_QUEUE_PUSH
ops["val"] = np.arange(MB, dtype=np.uint64)
d_ops = torch.from_numpy(ops.view(np.uint8).copy()).cuda()
torch.cuda.synchronize()
for r in range((1 << 24) // (MB // 2)):
    qu.qu_round_device(d_ops, MB, 1, None, None)
qu.sync()
d0 = qu.digest()
qu.kernel_timing(True)
ms = timed(lambda: qu.qu_reserve(N1))
assert qu.qu_capacity() == N1 and qu.qu_len() == N0 and qu.digest() == d0
report("queue", f"2^24 -> 2^25 elements, {N0} live, ring 2^25 -> 2^26 slots, front at position 2^24", N0 * 8,
       (1 << 26) * 8, ms, qu, "qu_grow")
qu.close()

# ---- page table ------------------------------------------------------------------------------------
NOP = 3000
vs = nrgpu.DeviceReplica(L.NRG_DS_VSPACE, 0, log2_slots=18, max_batch=1 << 16)
rng = np.random.default_rng(2024)
kind = rng.integers(0, 3, NOP)
nw = int((kind != 0).sum())
recs = np.zeros(nw, nrgpu.VSPACE_OP_DTYPE)
for i in range(nw):
    while True:
        vbase = int(rng.integers(0, 1 << 36)) << 12
        length = int(rng.integers(0, 1 << 16)) << 12
        if vbase + length <= 1 << 48:
            break
    recs[i] = (vbase, int(rng.integers(0, 1 << 36)) << 12, length, 0, 3)
recs["op"] = kind[kind != 0] - 1
d_recs = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
torch.cuda.synchronize()
vs.vs_round_device(d_recs, nw, 1, None, None)
vs.sync()
ntab = vs.vs_tables()
d0 = vs.digest()
vs.kernel_timing(True)
ms = timed(lambda: vs.vs_reserve(1 << 20))
assert vs.vs_capacity() == 1 << 20 and vs.vs_tables() == ntab and vs.digest() == d0
report("vspace", f"2^18 -> 2^20 tables, {ntab} allocated", ntab * 4096, (1 << 20) * 4096, ms, vs, "vs_grow")
vs.close()

# ---- growth on, the stack bench's shape --------------------------------------------------------------
# bench.py --workload stack: 50,000 elements, fused rounds of 2^20 ops (50/50), capacity
# 50,000 + 4 * 2^20 + 2^16. The host's bound on the length rises by a round's ops every round, so
# with a growth bound set the exact length is re-read (a stream synchronise) about every fourth
# round; the stack itself stays near 50,000 elements and never reallocates.
N, ROUNDS, POOL = 1 << 20, 200, 8
CAP = 50_000 + 4 * N + (1 << 16)
for bound in (0, 1 << 30):
    rep = nrgpu.DeviceReplica(L.NRG_DS_STACK, 0, max_batch=N, stack_capacity=CAP, log_bytes=64 * 4 * N)
    rep.use_torch_stream()
    rep.st_init(np.arange(50_000, dtype=np.uint32))
    rep.set_max_capacity(bound)
    ops = torch.empty((POOL, N), dtype=torch.int64, device="cuda")
    for p in range(POOL):
        rep.gen_stack_ops_device(ops[p], N, 0x5354434B00000001 + p)
    resp = torch.empty(N, dtype=torch.int32, device="cuda")
    some = torch.empty(N, dtype=torch.uint8, device="cuda")
    for i in range(10):
        rep.st_round_device(ops[i % POOL], N, 1, resp, some)
    rep.sync()
    rep.kernel_timing(True, only="st_room")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for i in range(ROUNDS):
        rep.st_round_device(ops[i % POOL], N, 1, resp, some)
    e1.record()
    torch.cuda.synchronize()
    host_us = (time.perf_counter() - t0) * 1e6 / ROUNDS
    rereads, _ = rep.kernel_time("st_room")
    print(f"stack bench shape, bound {bound}: {e0.elapsed_time(e1) * 1000.0 / ROUNDS:.2f} us per round (stream), "
          f"{host_us:.2f} us per round (host), length re-read {rereads} times in {ROUNDS} rounds, "
          f"capacity {rep.st_capacity()} (opened with {CAP}), length {rep.st_len()}")
    rep.close()
