"""Capacity growth of the file store, two measurements; run on the GPU box.

(a) Growth: nrg_memfs_reserve of a 256-MiB store (F = 8 files of 32 MiB, every byte live) to 512 MiB. The
    call is timed on the host (it allocates, launches, synchronises and frees) and its kernel, "mf_grow", by
    nrg_kernel_timing; REPS fresh contexts, since a store never shrinks. The yardstick, in the same run and
    alternating with them: per file a device-to-device hipMemcpyAsync of its old bytes to its place at the
    new stride and a hipMemsetAsync of its new tail (16 calls for the 8 files), between two stream events.
    The relayout does the same traffic (256 MiB read, 512 MiB written) in one pass.
(b) The per-round cost of the need check: microbench/memfs_round.py's round (N ops, 10 % Writes of 128
    bytes, responses wanted) on a sized context, with a bound set and B < max, no growth happening,
    against the same round with no bound, the two alternating window by window, REPS windows each, so
    that the difference can be read against the run-to-run spread. The no-bound figure is the one to
    compare across commits with microbench/memfs_sizes.py / memfs_round.py.
Usage: python microbench/memfs_grow.py [N] [ROUNDS] [REPS]
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "node-replication_amd"))
sys.path.insert(0, os.path.join(ROOT, "microbench"))
import nrgpu  # noqa: E402
from nrgpu import _lib as L  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
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


def spread(xs):
    xs = sorted(xs)
    return f"median {xs[len(xs) // 2]:.3f} ms, min {xs[0]:.3f}, max {xs[-1]:.3f} (n = {len(xs)})"


# ---- (a) ---------------------------------------------------------------------------------------------------
def grow_once(files, log2_from, log2_to):
    dev = nrgpu.DeviceReplica(L.NRG_DS_MEMFS, 0, log2_slots=log2_from, queue_capacity=files, max_batch=1 << 10)
    dev.mf_enable_sizes()
    d0 = dev.digest()
    dev.kernel_timing(True, only="mf_grow")
    t0 = time.perf_counter()
    dev.mf_reserve(1 << log2_to)
    host_ms = (time.perf_counter() - t0) * 1e3
    n, ms = dev.kernel_time("mf_grow")
    assert n == 1 and dev.mf_geometry() == (files, 1 << log2_to)
    assert dev.mf_read(L.NRG_MEMFS_FIRST_INO + files - 1, (1 << log2_from) - 4, 8) == b"\x01" * 4
    assert dev.digest() != d0  # (more words, the new ones zero)
    dev.close()
    return ms, host_ms


def yardstick_once(hip, files, log2_from, log2_to):
    B0, B1 = 1 << log2_from, 1 << log2_to
    src = torch.empty(files * B0, dtype=torch.uint8, device="cuda").fill_(1)
    dst = torch.empty(files * B1, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for f in range(files):
        assert hip.hipMemcpyAsync(dst.data_ptr() + f * B1, src.data_ptr() + f * B0, B0, D2D, None) == 0
        assert hip.hipMemsetAsync(dst.data_ptr() + f * B1 + B0, 0, B1 - B0, None) == 0
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    assert int(dst[B0 - 1]) == 1 and int(dst[B0]) == 0 and int(dst[(files - 1) * B1 + B0 - 1]) == 1
    del src, dst
    torch.cuda.empty_cache()
    return ms


def growth():
    hip = hip_runtime()
    files, l0, l1 = 8, 25, 26
    grow_once(files, l0, l1)  # warm-up: code objects, the allocator
    yardstick_once(hip, files, l0, l1)
    k, h, y = [], [], []
    for _ in range(REPS):
        ms, host_ms = grow_once(files, l0, l1)
        k.append(ms)
        h.append(host_ms)
        y.append(yardstick_once(hip, files, l0, l1))
    rd, wr = files << l0, files << l1
    med = sorted(k)[len(k) // 2]
    print(f"memfs_grow (a) F={files} {rd >> 20} MiB -> {wr >> 20} MiB")
    print(f"  mf_grow kernel               {spread(k)}: {(rd + wr) / med / 1e9:.2f} TB/s read + written")
    print(f"  nrg_memfs_reserve (host)     {spread(h)}")
    print(f"  {files} x (hipMemcpyAsync + hipMemsetAsync) {spread(y)}", flush=True)


# ---- (b) ---------------------------------------------------------------------------------------------------
def rounds():
    import memfs_round as MR  # gen_ops: generate_fs_operations' shape (its N is this script's argv[1] too)

    for files in (1, 1024):
        ring = 1 << max(int(2 * N + 8192 - 1).bit_length(), 14)
        devs = {}
        for name, bound in (("no bound", 0), ("bound, B < max", 1 << (MR.LOG2_B + 1))):
            dev = nrgpu.DeviceReplica(L.NRG_DS_MEMFS, 0, log2_slots=MR.LOG2_B, queue_capacity=files, max_batch=N,
                                      log_bytes=64 * ring)
            dev.mf_enable_sizes()
            dev.set_max_capacity(bound)
            dev.use_torch_stream()
            devs[name] = dev
        bufs = [torch.from_numpy(MR.gen_ops(N, files, 7 + s).view(np.uint8).reshape(-1)).cuda() for s in range(2)]
        d_resp = torch.empty(N * 136, dtype=torch.uint8, device="cuda")
        d_some = torch.empty(N, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def window(dev, n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(n):
                dev.mf_round(bufs[i & 1], N, 1, d_resp, d_some)
            e1.record()
            e1.synchronize()
            dev.sync()
            return e0.elapsed_time(e1) / n

        t = {name: [] for name in devs}
        for dev in devs.values():
            window(dev, 3)
        for _ in range(REPS):
            for name, dev in devs.items():  # alternating
                t[name].append(window(dev, ROUNDS))
        bd = devs["bound, B < max"]
        bd.kernel_timing(True, only="mf_need,mf_room")
        window(bd, ROUNDS)
        kn, kms = bd.kernel_time("mf_need")
        rn, rms = bd.kernel_time("mf_room")
        assert kn == ROUNDS and rn == ROUNDS and bd.mf_geometry() == (files, 1 << MR.LOG2_B), "no growth happens"
        print(f"memfs_grow (b) files={files} B={1 << MR.LOG2_B} ops={N} rounds per window={ROUNDS}")
        for name in devs:
            print(f"  round, {name:15s} {spread(t[name])}")
        print(f"  mf_need kernel {kms / kn:.4f} ms, mf_room readback {rms / rn:.4f} ms per round (events, a window of their own)",
              flush=True)
        for dev in devs.values():
            dev.close()


if __name__ == "__main__":
    if nrgpu.device_count() < 1:
        raise SystemExit("memfs_grow: no HIP device visible")
    growth()
    rounds()
