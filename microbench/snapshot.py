"""Time of a replica snapshot and restore on the two large states; run on the GPU box.

Hashmap at the benchmark's shape: 2^LOG2 slots (default 26) prefilled with KEYS keys (default 10M).
Each call is timed once on the host around the synchronous form (nrg_snapshot_async + nrg_sync,
nrg_restore), and the kernels by nrg_kernel_timing: hm_snapshot (the table scan), hm_restore_init
and hm_restore (the restore's two passes). Beside them, on the same table: hm_digest (reads the
whole table once, as the snapshot does), hm_dump (the export the snapshot replaces: one device
atomic per key), and nrg_hashmap_reserve's hm_grow_init + hm_rehash into the next table size (the
same two passes as a restore). The restore goes into a second replica of the same size.

Page table: the state microbench/vspace_digest.py builds (ROUNDS rounds of NOP ops), snapshot and
restore into a second pool of the same size, host times.
Usage: python microbench/snapshot.py [LOG2] [KEYS] [LOG2_POOL]
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

LOG2 = int(sys.argv[1]) if len(sys.argv) > 1 else 26
KEYS = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
LOG2_POOL = int(sys.argv[3]) if len(sys.argv) > 3 else 20
NOP, ROUNDS = 3000, 3


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def kernel_ms(dev, name):
    n, ms = dev.kernel_time(name)
    return ms / n if n else float("nan")


def snapshot_into(dev, ptr, cap):
    L.check(dev._lib.nrg_snapshot_async(dev.handle, C.c_void_p(ptr), cap), "snapshot")
    dev.sync()


# ---- hashmap ---------------------------------------------------------------------------------
a = nrgpu.DeviceReplica(L.NRG_DS_HASHMAP, 0, log2_slots=LOG2)
b = nrgpu.DeviceReplica(L.NRG_DS_HASHMAP, 0, log2_slots=LOG2)
a.hm_prefill_range(KEYS, 1)
info = a.snapshot_info()
buf = torch.empty(info.bytes, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
slots = 1 << LOG2
moved = slots * 32 + info.items * 16
print(f"hashmap: 2^{LOG2} slots ({slots * 32 / 2**30:.1f} GiB), {info.items} keys, image {info.bytes / 1e6:.1f} MB")
a.kernel_timing(True)
for rep in range(2):
    d, ms = wall(a.digest)
    print(f"  nrg_digest            {ms:8.3f} ms (host), hm_digest kernel so far {kernel_ms(a, 'hm_digest'):.3f} ms/launch")
for rep in range(2):
    _, ms = wall(lambda: snapshot_into(a, buf.data_ptr(), info.bytes))
    print(f"  nrg_snapshot_async+sync {ms:6.3f} ms (host)")
n_snap, ms_snap = a.kernel_time("hm_snapshot")
n_dg, ms_dg = a.kernel_time("hm_digest")  # (the snapshots ran it too)
print(f"  hm_snapshot kernel    {ms_snap / n_snap:8.3f} ms/launch over {n_snap}: {moved / 1e9:.2f} GB by construction "
      f"(slots * 32 + items * 16) = {moved / (ms_snap / n_snap) / 1e9:.2f} TB/s")
print(f"  hm_digest kernel      {ms_dg / n_dg:8.3f} ms/launch over {n_dg}: {slots * 32 / (ms_dg / n_dg) / 1e9:.2f} TB/s over slots * 32")
hinfo = L.SnapshotInfo()
L.check(a._lib.nrg_snapshot_info_read(a.handle, C.c_void_p(buf.data_ptr()), info.bytes, C.byref(hinfo)), "info_read")
assert tuple(int(x) for x in hinfo.digest) == d and hinfo.items == info.items
k = np.zeros(info.items, np.uint64)
v = np.zeros(info.items, np.uint64)
m = C.c_uint64()
_, ms = wall(lambda: L.check(a._lib.nrg_hashmap_dump(a.handle, k.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p),
                                                   info.items, C.byref(m))))
print(f"  nrg_hashmap_dump      {ms:8.1f} ms (host, {info.items * 16 / 1e6:.0f} MB to the host); its device part, "
      f"hm_dump kernel (one atomic per key): {kernel_ms(a, 'hm_dump'):.3f} ms")
b.kernel_timing(True)
for rep in range(2):
    _, ms = wall(lambda: b.restore(buf.data_ptr(), info.bytes))
    print(f"  nrg_restore           {ms:8.3f} ms (host; init + insert + digest check)")
print(f"  hm_restore_init kernel {kernel_ms(b, 'hm_restore_init'):7.3f} ms/launch, hm_restore kernel "
      f"{kernel_ms(b, 'hm_restore'):.3f} ms/launch")
assert b.digest() == d and b.hm_size() == info.items
b.close()
_, ms = wall(lambda: a.hm_reserve((slots // 2) + 1))
print(f"  nrg_hashmap_reserve to 2^{a.hm_log2_slots()} slots {ms:8.3f} ms (host): hm_grow_init "
      f"{kernel_ms(a, 'hm_grow_init'):.3f} ms, hm_rehash {kernel_ms(a, 'hm_rehash'):.3f} ms")
a.close()
del buf

# ---- page table (the state of microbench/vspace_digest.py) -----------------------------------------


def draw(rng):
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
    return recs


va = nrgpu.DeviceReplica(L.NRG_DS_VSPACE, 0, log2_slots=LOG2_POOL, max_batch=1 << 16)
vb = nrgpu.DeviceReplica(L.NRG_DS_VSPACE, 0, log2_slots=LOG2_POOL, max_batch=1 << 16)
va.use_torch_stream()
rng = np.random.default_rng(2024)
for r in range(ROUNDS):
    recs = draw(rng)
    d_recs = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
    va.vs_round_device(d_recs, len(recs), 1, None, None)
    torch.cuda.synchronize()
va.sync()
info = va.snapshot_info()
buf = torch.empty(info.bytes, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
print(f"vspace: pool 2^{LOG2_POOL} tables, {info.items} allocated, image {info.bytes / 1e6:.1f} MB")
d = va.digest()
for rep in range(2):
    _, ms = wall(va.digest)
    print(f"  nrg_digest            {ms:8.3f} ms (host)")
for rep in range(2):
    _, ms = wall(lambda: snapshot_into(va, buf.data_ptr(), info.bytes))
    print(f"  nrg_snapshot_async+sync {ms:6.3f} ms (host; copies {info.bytes / 1e6:.1f} MB and digests)")
for rep in range(2):
    _, ms = wall(lambda: vb.restore(buf.data_ptr(), info.bytes))
    print(f"  nrg_restore           {ms:8.3f} ms (host; copies the image, zeroes the other "
          f"{((1 << LOG2_POOL) - info.items) * 4096 / 2**30:.2f} GiB of the pool, digest check)")
assert vb.digest() == d and vb.vs_tables() == info.items
va.close()
vb.close()
