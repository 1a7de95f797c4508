"""Time of one fused page-table round (nrg_vspace_round_async) and of Identify batches
(nrg_vspace_resolve_async); run on the GPU box.

Rounds of NOP ops (default 3000, the bench's NOP) drawn as generate_operations draws them
(benches/vspace.rs:528-554): one third Identify(random u64), one third Map, one third MapDevice,
vbase and pbase any 4 KiB multiple below 2^48 and len any 4 KiB multiple below 2^28 (a region
that would cross 2^48 is drawn again). A round's writes go through one nrg_vspace_round_async and
its reads through one nrg_vspace_resolve_async. The table only grows (a 3000-op round allocates
about 130,000 tables, 0.5 GiB), so every timed round is a fresh draw on the state the rounds
before it left: ROUNDS rounds after two warm-up rounds, each between two stream events. A second
pass with kernel timing on gives the time of each of the six launches. The byte ledger is what the
launches move by construction.
Usage: python microbench/vspace_round.py [NOP] [ROUNDS] [LOG2_POOL]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "node-replication_amd"))
import nrgpu  # noqa: E402
from nrgpu import _lib as L  # noqa: E402

NOP = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 8
LOG2_POOL = int(sys.argv[3]) if len(sys.argv) > 3 else 22
WARM = 2
KERNELS = ("vs_prep", "vs_dep", "vs_plan", "vs_alloc", "vs_apply", "vs_seq")
MB2 = 1 << 21


def draw(rng):
    """one round: (write records, Identify addresses)"""
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
    reads = rng.integers(0, 2**64 - 1, NOP - nw, dtype=np.uint64, endpoint=True)
    return recs, reads


def ledger(recs):
    """bytes one round moves by construction (every op independent, nothing mapped before)"""
    pages = int((recs["len"] >> np.uint64(12)).sum())
    last = recs["vbase"] + np.maximum(recs["len"], np.uint64(1)) - np.uint64(1)
    granules = int(((last >> np.uint64(21)) - (recs["vbase"] >> np.uint64(21)) + np.uint64(1)).sum())
    n = len(recs)
    return {
        "leaf entries (8 B each)": 8 * pages,
        "new PD entries (one per granule)": 8 * granules,
        "classify reads (PD entry per granule, plan + apply)": 2 * 8 * granules,
        "records (prep, log copy, plan, apply)": 4 * 32 * n,
        "granule ranges (dep, tiled)": 8 * n * (n // 256 + 1) // 2 + 8 * n,
        "responses (16 B + 1 B)": 17 * n,
    }, pages, granules


dev = nrgpu.DeviceReplica(L.NRG_DS_VSPACE, 0, log2_slots=LOG2_POOL, max_batch=1 << 16, max_reads=1 << 20)
dev.use_torch_stream()
rng = np.random.default_rng(2024)
rounds = [draw(rng) for _ in range(2 * (WARM + ROUNDS))]
d_recs = [torch.from_numpy(r.view(np.uint8).copy()).cuda() for r, _ in rounds]
d_reads = [torch.from_numpy(a.view(np.int64).copy()).cuda() for _, a in rounds]
nmax = max(len(r) for r, _ in rounds)
resp = torch.empty((nmax, 2), dtype=torch.int64, device="cuda")
some = torch.empty(nmax, dtype=torch.uint8, device="cuda")
pa = torch.empty(1 << 20, dtype=torch.int64, device="cuda")
found = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")


def one(k):
    """round k: its writes, then its reads; microseconds of each"""
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    dev.vs_round_device(d_recs[k], len(rounds[k][0]), 1, resp, some)
    e[1].record()
    dev.vs_resolve_device(d_reads[k], len(rounds[k][1]), pa, found)
    e[2].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]) * 1000.0, e[1].elapsed_time(e[2]) * 1000.0


for k in range(WARM):
    one(k)
print(f"NOP={NOP}: rounds of about {NOP * 2 // 3} writes + {NOP // 3} Identify; pool 2^{LOG2_POOL} tables")
for k in range(WARM, WARM + ROUNDS):
    led, pages, granules = ledger(rounds[k][0])
    w_us, r_us = one(k)
    total = sum(led.values())
    ok = int(some[: len(rounds[k][0])].sum())
    print(f"round {k - WARM}: writes {w_us:9.1f} us ({w_us / 6:.1f} us per launch, 6 launches), Identify {r_us:6.1f} us; "
          f"{pages} leaves in {granules} granules, {ok}/{len(rounds[k][0])} ok, {total / 1e6:.1f} MB by construction = "
          f"{total / w_us / 1e6:.3f} TB/s; tables {dev.vs_tables()}")
for k, v in led.items():
    print(f"  {k:52s} {v / 1e6:9.2f} MB (last round)")

# the same again with every launch stamped: time per kernel
dev.kernel_timing(True)
for k in range(WARM + ROUNDS, 2 * (WARM + ROUNDS) - WARM):
    if dev.vs_tables() + 200_000 > (1 << LOG2_POOL):
        break
    one(k)
for name in KERNELS + ("vs_resolve",):
    n, ms = dev.kernel_time(name)
    if n:
        print(f"  {name:10s} {ms * 1000.0 / n:9.1f} us per launch over {n} launches")
dev.kernel_timing(False)

# One sequential step: chains of dependent ops, which all but the first replay one after the
# other in the in-order workgroup. Small: 1024 one-page ops on one granule. Large: 64 ops of
# 32,768 pages, each starting on page 1 of the granule the one before it ends in.
free = 0x7F00_0000_0000  # a PML4 slot the random draws rarely reach; both chains stay below 2^48
small = np.zeros(1024, nrgpu.VSPACE_OP_DTYPE)
# (the second 512 remap the pages of the first 512: they fail at once, still a step each)
small["vbase"] = np.uint64(free) + (np.arange(1024, dtype=np.uint64) % np.uint64(512)) * np.uint64(4096)
small["len"], small["rights"] = 4096, 3
big = np.zeros(64, nrgpu.VSPACE_OP_DTYPE)
big["vbase"] = np.uint64(free + (1 << 32) + 4096) + np.arange(64, dtype=np.uint64) * np.uint64(64 * MB2)
big["len"], big["rights"] = 64 * MB2, 3
for name, chain in (("1-page ops", small), ("32768-page ops", big)):
    if dev.vs_tables() + 10_000 > (1 << LOG2_POOL):
        break
    d_chain = torch.from_numpy(chain.view(np.uint8).copy()).cuda()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    dev.vs_round_device(d_chain, len(chain), 1, resp, some)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1000.0
    print(f"chain of {len(chain)} dependent {name}: round {us:.1f} us, {us / (len(chain) - 1):.2f} us per sequential step "
          f"({int(some[: len(chain)].sum())} ok)")

# Identify throughput: 2^20 addresses, half of them inside mapped regions
recs = np.concatenate([r for r, _ in rounds[: WARM + ROUNDS]])
recs = recs[recs["len"] > 0]
pick = rng.integers(0, len(recs), 1 << 19)
inside = recs["vbase"][pick] + rng.integers(0, 1 << 28, 1 << 19).astype(np.uint64) % recs["len"][pick]
va = np.concatenate([inside, rng.integers(0, 1 << 48, 1 << 19).astype(np.uint64)])
d_va = torch.from_numpy(rng.permutation(va).view(np.int64).copy()).cuda()
for _ in range(3):
    dev.vs_resolve_device(d_va, len(va), pa, found)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(20):
    dev.vs_resolve_device(d_va, len(va), pa, found)
e1.record()
torch.cuda.synchronize()
us = e0.elapsed_time(e1) * 1000.0 / 20
print(f"Identify x {len(va)}: {us:.1f} us per batch = {len(va) / us:.1f} M addresses/s "
      f"({int(found.sum())} found)")
dev.sync()
dev.close()
