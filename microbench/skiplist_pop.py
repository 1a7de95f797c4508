"""Times of the skip list's pops (nrg_skiplist_enable_pops; run on the GPU box). Writes
profiles/skiplist_pop.txt (or the file given with --out).

Three parts, every one on a map prefilled with PREFILL = 2^22 keys i -> i (SkipListWrapper::default;
delta_max = 2^20 and chunks of 1M leave keys below 4,000,000 in the base run, the rest in the delta run):

  enable   what enabling costs a round of N = 1M Push records with no pop record: the sl_pop_find launch
           and the readback of its tile counts. Cases "off" and "on" with this tree, and, with
           --parent DIR, "parent": the same round (pops off) on a built checkout of the parent commit, DIR
           its node-replication_amd folder (package and library). The package is chosen when a process
           starts, so every case is a child process of this script, run one after the other, alternating,
           REPS times on the one box. ROUNDS back-to-back rounds between two stream events.
  step     one pop step: a round of one record, PopFront x n or PopBack x n, n = 1, 1024 and 1M, with the
           entries asked for (nrg_skiplist_round_pops_async) and without (nrg_skiplist_round_async). The
           host synchronises inside a pop step, so these are wall-clock times of the call plus a stream
           synchronise, the mean of a few rounds on the shrinking map; the kernels' own times per launch
           beside them (nrg_kernel_time). Front pops of base keys shift the base run; back pops copy nothing.
  segment  a chunk that alternates Push and PopFront x 1 record by record: 2 * K records are 2 * K segments;
           wall-clock per round and per segment.
Usage: python microbench/skiplist_pop.py [--parent DIR] [--out FILE]
"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("NRGPU_PKG") or os.path.join(ROOT, "node-replication_amd"))  # (a child of --parent)

N = 1_000_000
ROUNDS = 24
REPS = 3
PREFILL = 1 << 22
DELTA_MAX = 1 << 20
LOG2 = 23
FRONT, BACK = 2**64 - 2, 2**64 - 3
POP_KERNELS = ("sl_pop_find", "sl_pop_plan", "sl_pop_take", "sl_pop_shift")


def _open(max_batch):
    import nrgpu
    from nrgpu import _lib as L

    dev = nrgpu.DeviceReplica(L.NRG_DS_SKIPLIST, 0, knobs={"SL_DELTA_MAX": DELTA_MAX}, log2_slots=LOG2, max_batch=max_batch,
                              log_bytes=64 * 4 * max(max_batch, 8192))
    dev.use_torch_stream()
    dev.sl_prefill_range(PREFILL, 0)
    return dev


def _cuda(recs):
    import torch

    return torch.from_numpy(recs.view(np.int64).copy()).cuda()


def _recs(keys, vals):
    import nrgpu

    r = np.zeros(len(keys), nrgpu.PUT_DTYPE)
    r["key"], r["val"] = keys, vals
    return r


def enable_case(enable):
    """one child: the mean time of a 1M-record round without pop records, in us"""
    import torch

    dev = _open(N)
    if enable:
        dev.sl_enable_pops()
    nb = ROUNDS + 2
    bt = []
    for b in range(nb):
        rng = np.random.default_rng(100 + b)
        bt.append(_cuda(_recs(rng.integers(0, PREFILL, N, dtype=np.uint64), rng.integers(0, 1 << 62, N, dtype=np.uint64))))
    resp = torch.empty(N, dtype=torch.int64, device="cuda")
    some = torch.empty(N, dtype=torch.uint8, device="cuda")
    for r in range(2):
        dev.sl_round_device(bt[r], N, 1, resp, some)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for r in range(ROUNDS):
        dev.sl_round_device(bt[2 + r], N, 1, resp, some)
    e1.record()
    torch.cuda.synchronize()
    print("ENABLE_US %.1f" % (e0.elapsed_time(e1) * 1000.0 / ROUNDS), flush=True)
    dev.sync()
    dev.close()


def _kernel_cells(dev):
    cells = []
    for name in POP_KERNELS:
        n, ms = dev.kernel_time(name)
        cells.append(f"{1000.0 * ms / n:.0f} x{n}" if n else "-")
    return " | ".join(cells)


def step_part(out):
    import torch

    out("| record | entries | rounds | call + sync, us | " + " | ".join(k[3:] for k in POP_KERNELS) + " | keys at the end |")
    out("|---|---|---|---|" + "---|" * (len(POP_KERNELS) + 1))
    for mark, tag in ((FRONT, "PopFront"), (BACK, "PopBack")):
        for n in (1, 1024, 1_000_000):
            for want in (True, False):
                dev = _open(N)
                dev.sl_enable_pops()
                rounds = 3 if n > 100_000 else 16
                rec = _cuda(_recs([n], [mark]))
                resp = torch.empty(1, dtype=torch.int64, device="cuda")
                some = torch.empty(1, dtype=torch.uint8, device="cuda")
                pk = torch.empty(n, dtype=torch.int64, device="cuda")
                pv = torch.empty(n, dtype=torch.int64, device="cuda")
                pn = torch.empty(1, dtype=torch.int64, device="cuda")

                def one():
                    if want:
                        dev.sl_round_pops_device(rec, 1, 1, resp, some, pk, pv, n, pn)
                    else:
                        dev.sl_round_device(rec, 1, 1, resp, some)

                one()  # warm
                torch.cuda.synchronize()
                dev.kernel_timing(True)
                t0 = time.perf_counter()
                for _ in range(rounds):
                    one()
                    torch.cuda.synchronize()
                us = (time.perf_counter() - t0) * 1e6 / rounds
                out(f"| {tag} x {n} | {'packed' if want else 'counts only'} | {rounds} | {us:.0f} | {_kernel_cells(dev)} | "
                    f"{dev.sl_len()} |")
                dev.sync()
                dev.close()


def segment_part(out):
    import torch

    out("| alternating chunk | segments | rounds | call + sync, us per round | us per segment | keys at the end |")
    out("|---|---|---|---|---|---|")
    for K in (64, 512):
        dev = _open(N)
        dev.sl_enable_pops()
        rounds = 4
        keys = np.empty(2 * K, np.uint64)
        vals = np.empty(2 * K, np.uint64)
        keys[0::2], vals[0::2] = np.arange(K, dtype=np.uint64) + (1 << 40), 7  # new keys at the back
        keys[1::2], vals[1::2] = 1, FRONT
        rec = _cuda(_recs(keys, vals))
        resp = torch.empty(2 * K, dtype=torch.int64, device="cuda")
        some = torch.empty(2 * K, dtype=torch.uint8, device="cuda")
        dev.sl_round_device(rec, 2 * K, 1, resp, some)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(rounds):
            dev.sl_round_device(rec, 2 * K, 1, resp, some)
            torch.cuda.synchronize()
        us = (time.perf_counter() - t0) * 1e6 / rounds
        out(f"| {K} x (Push, PopFront x 1) | {2 * K} | {rounds} | {us:.0f} | {us / (2 * K):.1f} | {dev.sl_len()} |")
        dev.sync()
        dev.close()


def main():
    args = sys.argv[1:]
    if args[:1] == ["--case"]:
        enable_case(args[1] == "on")
        return
    parent = args[args.index("--parent") + 1] if "--parent" in args else None
    path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "skiplist_pop.txt")
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out(f"prefill 2^22: base run [0, 4000000), delta run [4000000, {PREFILL}); times in us")
    out(f"enable: a round of N = {N} Pushes with no pop record, mean of {ROUNDS} rounds, {REPS} alternating runs, one process each")
    cases = ([("parent", "off", parent)] if parent else []) + [("off", "off", None), ("on", "on", None)]
    out("| run | " + " | ".join(c[0] for c in cases) + " |")
    out("|---|" + "---|" * len(cases))
    for rep in range(REPS):
        cells = []
        for label, mode, lib in cases:
            env = dict(os.environ)
            env.pop("NRGPU_LIB", None)
            env.pop("NRGPU_PKG", None)
            if lib:
                env["NRGPU_PKG"] = os.path.abspath(lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", mode], env=env, capture_output=True,
                               text=True, timeout=240)
            got = [ln for ln in p.stdout.splitlines() if ln.startswith("ENABLE_US")]
            if p.returncode != 0 or not got:
                out(f"case {label} failed (exit {p.returncode}): {p.stderr[-400:]}")
                sys.exit(1)  # nothing more is started on the device
            cells.append(got[0].split()[1])
        out(f"| {rep} | " + " | ".join(cells) + " |")
    out("")
    out("step: a round of one pop record (a 4M-key base run, 194304 delta keys)")
    step_part(out)
    out("")
    out("segment: a chunk alternating Push and PopFront x 1 (one segment per record)")
    segment_part(out)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
