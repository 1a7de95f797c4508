"""Cost of one table growth of the NrHashMap replica (nrg_hashmap_reserve; run on the GPU box).

configs[1]'s table (2^26 slots = 2 GiB, prefilled with 10M keys, benches/hashmap.rs:91-100) grows
to 2^27 slots in one rehash. Timed: the whole synchronous call on the host, and inside it the
init pass of the new table ("hm_grow_init") and the rehash pass ("hm_rehash") by the events of
their own dispatches (nrg_kernel_timing). Each repeat runs in a fresh replica.
The byte ledger is what the passes move by construction; the rehash is set against a streaming
read of the old table at the copy rate measured on this GPU (6.3 TB/s).
Usage: python microbench/hm_grow.py [LOG2_SLOTS] [KEYS] [REPEATS]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "node-replication_amd"))
import nrgpu  # noqa: E402
from nrgpu import _lib as L  # noqa: E402

LOG2 = int(sys.argv[1]) if len(sys.argv) > 1 else 26
KEYS = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
REPEATS = int(sys.argv[3]) if len(sys.argv) > 3 else 2
SLOT = 32
COPY_TBS = 6.3

old_b, new_b = SLOT << LOG2, SLOT << (LOG2 + 1)
print(f"old table 2^{LOG2} slots = {old_b / 2**30:.2f} GiB read; new table 2^{LOG2 + 1} slots = "
      f"{new_b / 2**30:.2f} GiB initialised; {KEYS} slots written (claim 8 B + stamps 16 B + value 8 B each, "
      f"{KEYS * 128 / 2**30:.2f} GiB of 128-B lines at most)")
floor_us = old_b / (COPY_TBS * 1e6)
print(f"streaming read of the old table at {COPY_TBS} TB/s: {floor_us:.0f} us")

for rep in range(REPEATS):
    dev = nrgpu.DeviceReplica(L.NRG_DS_HASHMAP, 0, log2_slots=LOG2, max_batch=1 << 16)
    dev.hm_prefill_range(KEYS, 1)
    before = dev.hm_digest()
    dev.kernel_timing(True, "hm_grow_init,hm_rehash")
    dev.sync()
    t0 = time.perf_counter()
    dev.hm_reserve(1 << LOG2)  # one key per two slots of the doubled table
    wall = (time.perf_counter() - t0) * 1e6
    assert dev.hm_log2_slots() == LOG2 + 1
    n_i, ms_i = dev.kernel_time("hm_grow_init")
    n_r, ms_r = dev.kernel_time("hm_rehash")
    assert (n_i, n_r) == (1, 1)
    dev.kernel_timing(False)
    assert dev.hm_digest() == before and dev.hm_size() == KEYS
    print(f"run {rep}: reserve {wall:9.0f} us on the host; init {ms_i * 1e3:8.1f} us "
          f"({new_b / ms_i / 1e9:.2f} TB/s); rehash {ms_r * 1e3:8.1f} us = {ms_r * 1e3 / floor_us:.2f} x the "
          f"streaming read")
    dev.close()
