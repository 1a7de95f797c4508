"""Time of Replica::verify's two forms on a page-table replica: nrg_digest (four launches on the
device, 24 bytes back) and nrg_vspace_dump (every allocated table copied to the host and walked
there); run on the GPU box.

ROUNDS rounds (default 3) of NOP ops (default 3000, the bench's NOP) drawn as generate_operations
draws them (benches/vspace.rs:528-554; the Identify third is not issued), each through one
nrg_vspace_round_async. Then, on that one state: nrg_digest timed once (the first call, which also
allocates and zeroes the tag scratch), once more (tags in place), and nrg_vspace_dump timed once,
all as the host sees them (wall clock around the synchronous call). The dump's leaves go through
nrgpu.digest.vspace and must give the device's triple. The byte ledger is what the digest reads by
construction: every allocated table once, and its tag in each of the three level passes.
Usage: python microbench/vspace_digest.py [NOP] [ROUNDS] [LOG2_POOL]
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
from nrgpu import digest  # noqa: E402

NOP = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
LOG2_POOL = int(sys.argv[3]) if len(sys.argv) > 3 else 20


def draw(rng):
    """the writes of one round"""
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


dev = nrgpu.DeviceReplica(L.NRG_DS_VSPACE, 0, log2_slots=LOG2_POOL, max_batch=1 << 16)
dev.use_torch_stream()
rng = np.random.default_rng(2024)
pages = 0
for k in range(ROUNDS):
    recs = draw(rng)
    pages += int((recs["len"] >> np.uint64(12)).sum())
    d_recs = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
    dev.vs_round_device(d_recs, len(recs), 1, None, None)
    torch.cuda.synchronize()
dev.sync()
tables = dev.vs_tables()
print(f"{ROUNDS} rounds of about {NOP * 2 // 3} writes; pool 2^{LOG2_POOL} tables, {tables} allocated "
      f"({tables * 4096 / 2**30:.2f} GiB), at most {pages} leaves")


def timed_digest():
    t0 = time.perf_counter()
    d = dev.digest()
    return d, (time.perf_counter() - t0) * 1e3


d1, ms1 = timed_digest()
d2, ms2 = timed_digest()
by_construction = tables * 4096 + 3 * tables * 8
print(f"nrg_digest, first call (allocates and zeroes {8 << LOG2_POOL >> 20} MiB of tags): {ms1:9.3f} ms")
print(f"nrg_digest, again:                                          {ms2:9.3f} ms; reads "
      f"{by_construction / 1e6:.1f} MB by construction = {by_construction / ms2 / 1e9:.3f} TB/s")
assert d1 == d2

leaves = np.zeros(max(pages, 1), nrgpu.VSPACE_LEAF_DTYPE)
n = C.c_uint64()
t0 = time.perf_counter()
rc = dev._lib.nrg_vspace_dump(dev.handle, leaves.ctypes.data_as(C.c_void_p), len(leaves), C.byref(n))
ms_dump = (time.perf_counter() - t0) * 1e3
L.check(rc, "nrg_vspace_dump")
print(f"nrg_vspace_dump ({n.value} leaves, {tables * 4096 / 1e6:.1f} MB copied to the host and walked there): "
      f"{ms_dump:9.1f} ms = {ms_dump / ms2:.0f} x the digest")
leaves = leaves[: n.value]
mirror = digest.vspace(leaves["vaddr"], leaves["entry"])
print("device digest", d2, "== mirror of the dump:", mirror == d2)
assert mirror == d2
dev.close()
