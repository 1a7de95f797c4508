"""ctypes binding of libnrgpu.so (the C ABI declared in include/nrgpu.h).

The HIP library is the product: there is no CPU fallback. If the shared library is missing
this module raises at import time, and every data-plane call goes to the GPU.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("NRGPU_LIB") or os.path.join(PKG_ROOT, "lib", "libnrgpu.so")  # env: A/B builds

# import torch first (when present) so that the process has ONE HIP runtime: torch ships
# its own libamdhip64.so.7 and the loader then reuses it for libnrgpu.so by SONAME.
try:  # pragma: no cover - depends on the image
    import torch  # noqa: F401
except Exception:  # noqa: BLE001
    torch = None

NRG_OK = 0
NRG_E_INVAL = -1
NRG_E_HIP = -2
NRG_E_TABLE_FULL = -3
NRG_E_RING_FULL = -4
NRG_E_NOMEM = -5
NRG_E_NOT_SYNCED = -6
NRG_E_CAPACITY = -7
NRG_E_NODEV = -8
NRG_E_COMM = -9
NRG_E_TIMEOUT = -10
NRG_GROUP_DEFAULT_TIMEOUT_MS = 300000
NRG_GROUP_ID_BYTES = 128
NRG_MAX_PARTS = 64

NRG_DS_HASHMAP = 1
NRG_DS_STACK = 2
NRG_DS_SYNTHETIC = 3
NRG_DS_QUEUE = 4
NRG_DS_VSPACE = 5
NRG_DS_SKIPLIST = 6
NRG_DS_MEMFS = 7

NRG_STACK_POP = 0
NRG_STACK_PUSH = 1
NRG_QUEUE_POP = 0
NRG_QUEUE_PUSH = 1
NRG_SYNTH_WRITE_ONLY = 0
NRG_SYNTH_READ_WRITE = 1
NRG_VSPACE_MAP = 0
NRG_VSPACE_MAP_DEVICE = 1
# nrg_skiplist_seek modes: SkipMap::lower_bound (GE, GT) / upper_bound (LE, LT)
NRG_SEEK_GE = 0
NRG_SEEK_GT = 1
NRG_SEEK_LE = 2
NRG_SEEK_LT = 3
NRG_SCAN_MAX_LIMIT = 1024  # nrg_skiplist_scan: entries per query at most
# file store ops (benches/memfs.rs:24-85 OperationWr), its first inode (:117-119) and error answers
NRG_MEMFS_WRITE = 0
NRG_MEMFS_READ = 1
NRG_MEMFS_GETATTR = 2
NRG_MEMFS_SETATTR = 3  # a sized context only (nrg_memfs_enable_sizes)
NRG_MEMFS_FIRST_INO = 5
NRG_MEMFS_ENOENT = 1
NRG_MEMFS_EFBIG = 2
NRG_MEMFS_EINVAL = 3
NRG_MEMFS_MAX_DATA = 128  # data bytes a record carries at most
NRG_MEMFS_PARTITION_TILE = 256  # records per tile of nrg_memfs_partition_async
NRG_MF_PREAD_TILE = 16384  # output bytes per workgroup of nrg_memfs_pread's copy and of the re-pack

# nrg_vspace_op (32 B), nrg_vspace_resp (16 B) and nrg_vspace_leaf (16 B)
VSPACE_OP_DTYPE = np.dtype([("vbase", "<u8"), ("pbase", "<u8"), ("len", "<u8"), ("op", "<u4"), ("rights", "<u4")])
VSPACE_RESP_DTYPE = np.dtype([("a", "<u8"), ("b", "<u8")])
VSPACE_LEAF_DTYPE = np.dtype([("vaddr", "<u8"), ("entry", "<u8")])
# nrg_memfs_op (152 B) and nrg_memfs_resp (136 B)
MEMFS_OP_DTYPE = np.dtype([("ino", "<u8"), ("offset", "<u8"), ("op", "<u4"), ("len", "<u4"), ("data", "u1", (128,))])
MEMFS_RESP_DTYPE = np.dtype([("n", "<u8"), ("data", "u1", (128,))])
# nrg_memfs_rd (24 B): one request of nrg_memfs_pread
MEMFS_RD_DTYPE = np.dtype([("ino", "<u8"), ("offset", "<u8"), ("len", "<u8")])
# nrg_memfs_wr (32 B): one request of nrg_memfs_pwrite*: data[data_off, data_off + len) to `ino` at `offset`
MEMFS_WR_DTYPE = np.dtype([("ino", "<u8"), ("offset", "<u8"), ("len", "<u8"), ("data_off", "<u8")])


class NrgError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        self.code = code
        msg = _lib.nrg_strerror(code).decode() if _lib is not None else str(code)
        super().__init__(f"{what}: {msg} ({code})" if what else f"{msg} ({code})")


class Config(C.Structure):
    _fields_ = [
        ("ds_kind", C.c_uint32),
        ("log2_slots", C.c_uint32),
        ("log_bytes", C.c_uint64),
        ("max_batch", C.c_uint64),
        ("max_reads", C.c_uint64),
        ("stack_capacity", C.c_uint64),
        ("synth_n", C.c_uint64),
        ("synth_cold_reads", C.c_uint32),
        ("synth_cold_writes", C.c_uint32),
        ("synth_hot_reads", C.c_uint32),
        ("synth_hot_writes", C.c_uint32),
        ("stack_push_resp", C.c_uint32),
        ("replica_id", C.c_uint32),
        ("pipeline", C.c_uint32),
        ("hashmap_max_log2_slots", C.c_uint32),
        ("queue_capacity", C.c_uint64),
    ]


class LogInfo(C.Structure):
    _fields_ = [
        ("size", C.c_uint64),
        ("head", C.c_uint64),
        ("tail", C.c_uint64),
        ("ctail", C.c_uint64),
        ("ltail", C.c_uint64),
        ("replica_id", C.c_uint32),
        ("ds_kind", C.c_uint32),
    ]


class SnapshotInfo(C.Structure):
    """nrg_snapshot_info: a snapshot's header, validated."""

    _fields_ = [
        ("ds_kind", C.c_uint32),
        ("version", C.c_uint32),
        ("items", C.c_uint64),
        ("bytes", C.c_uint64),
        ("log_idx", C.c_uint64),
        ("digest", C.c_uint64 * 3),
    ]


class Round(C.Structure):
    """nrg_round: one group member's part of a round (device pointers on its GPU)."""

    _fields_ = [
        ("recs", C.c_void_p),
        ("n", C.c_uint64),
        ("resp", C.c_void_p),
        ("some", C.c_void_p),
        ("get_keys", C.c_void_p),
        ("n_gets", C.c_uint64),
        ("get_vals", C.c_void_p),
        ("get_found", C.c_void_p),
    ]


class Seek(C.Structure):
    """nrg_seek: one group member's queries of nrg_group_skiplist_seek (device pointers on its GPU)."""

    _fields_ = [
        ("keys", C.c_void_p),
        ("n", C.c_uint64),
        ("out_keys", C.c_void_p),
        ("out_vals", C.c_void_p),
        ("found", C.c_void_p),
    ]


class Scan(C.Structure):
    """nrg_scan: one group member's queries of nrg_group_skiplist_scan (device pointers on its GPU)."""

    _fields_ = [
        ("keys", C.c_void_p),
        ("n", C.c_uint64),
        ("out_keys", C.c_void_p),
        ("out_vals", C.c_void_p),
        ("counts", C.c_void_p),
    ]


class Count(C.Structure):
    """nrg_count: one group member's queries of nrg_group_skiplist_range_count."""

    _fields_ = [
        ("los", C.c_void_p),
        ("his", C.c_void_p),
        ("n", C.c_uint64),
        ("counts", C.c_void_p),
    ]


class PopReq(C.Structure):
    """nrg_pop_req: one request of nrg_group_skiplist_pop: PopFront x n (back = 0) or PopBack x n (back = 1)."""

    _fields_ = [("n", C.c_uint64), ("back", C.c_uint32), ("reserved", C.c_uint32)]


class Pops(C.Structure):
    """nrg_pops: one group member's part of nrg_group_skiplist_pop (reqs a host array, the rest device
    pointers on its GPU)."""

    _fields_ = [
        ("reqs", C.POINTER(PopReq)),
        ("n", C.c_uint64),
        ("resp", C.c_void_p),
        ("some", C.c_void_p),
        ("pop_keys", C.c_void_p),
        ("pop_vals", C.c_void_p),
        ("pop_cap", C.c_uint64),
        ("pop_n", C.c_void_p),
    ]


class Pread(C.Structure):
    """nrg_pread: one group member's requests of nrg_group_memfs_pread (device pointers on its GPU)."""

    _fields_ = [
        ("reqs", C.c_void_p),
        ("n", C.c_uint64),
        ("data", C.c_void_p),
        ("cap", C.c_uint64),
        ("offs", C.c_void_p),
        ("some", C.c_void_p),
    ]


vp = C.c_void_p
u64 = C.c_uint64
u32 = C.c_uint32
u64p = C.POINTER(C.c_uint64)

# every symbol declared in include/nrgpu.h, with its ctypes signature
SIGNATURES = {
    "nrg_config_default": (None, [C.POINTER(Config), u32]),
    "nrg_open": (C.c_int, [C.c_int, C.POINTER(Config), C.POINTER(vp)]),
    "nrg_close": (C.c_int, [vp]),
    "nrg_set_stream": (C.c_int, [vp, vp]),
    "nrg_get_stream": (vp, [vp]),
    "nrg_own_stream": (vp, [vp]),
    "nrg_sync": (C.c_int, [vp]),
    "nrg_join": (C.c_int, [vp]),
    "nrg_set_max_capacity": (C.c_int, [vp, u64]),
    "nrg_digest": (C.c_int, [vp, vp]),
    "nrg_digest_async": (C.c_int, [vp, vp]),
    "nrg_group_verify": (C.c_int, [vp, vp, C.POINTER(C.c_int)]),
    "nrg_snapshot_size": (C.c_int, [vp, C.POINTER(SnapshotInfo)]),
    "nrg_snapshot_async": (C.c_int, [vp, vp, u64]),
    "nrg_snapshot_info_read": (C.c_int, [vp, vp, u64, C.POINTER(SnapshotInfo)]),
    "nrg_restore": (C.c_int, [vp, vp, u64]),
    "nrg_group_resync": (C.c_int, [vp, C.c_int]),
    "nrg_strerror": (C.c_char_p, [C.c_int]),
    "nrg_version": (C.c_char_p, []),
    "nrg_device_count": (C.c_int, []),
    "nrg_log_append": (C.c_int, [vp, vp, u64, u32, u64p]),
    "nrg_log_append_async": (C.c_int, [vp, vp, u64, u32, u64p]),
    "nrg_log_append_segments_async": (C.c_int, [vp, vp, u32, u64, u64p, C.POINTER(u32), u64p]),
    "nrg_log_exec": (C.c_int, [vp, u64, u64, vp, vp]),
    "nrg_log_exec_async": (C.c_int, [vp, u64, u64, vp, vp]),
    "nrg_log_state": (C.c_int, [vp, C.POINTER(LogInfo)]),
    "nrg_log_reset": (C.c_int, [vp]),
    "nrg_hashmap_get": (C.c_int, [vp, vp, u64, vp, vp]),
    "nrg_hashmap_get_async": (C.c_int, [vp, vp, u64, vp, vp]),
    "nrg_hashmap_round_async": (C.c_int, [vp, vp, u64, u32, vp, u64, vp, vp, vp, vp]),
    "nrg_stack_round_async": (C.c_int, [vp, vp, u64, u32, vp, vp]),
    "nrg_synth_round_async": (C.c_int, [vp, vp, u64, u32, vp, vp]),
    "nrg_hashmap_round_segments_async": (C.c_int, [vp, vp, u32, u64, u64p, C.POINTER(u32), u32, vp, u64, vp, vp,
                                                   vp, vp]),
    "nrg_hashmap_prefill": (C.c_int, [vp, vp, vp, u64]),
    "nrg_hashmap_prefill_range": (C.c_int, [vp, u64, u64]),
    "nrg_hashmap_size": (C.c_int, [vp, u64p]),
    "nrg_hashmap_reserve": (C.c_int, [vp, u64]),
    "nrg_hashmap_capacity": (C.c_int, [vp, C.POINTER(u32)]),
    "nrg_hashmap_enable_removal": (C.c_int, [vp, u64]),
    "nrg_hashmap_removal": (C.c_int, [vp, u64p, C.POINTER(C.c_int)]),
    "nrg_hashmap_occupancy": (C.c_int, [vp, u64p]),
    "nrg_hashmap_purge": (C.c_int, [vp]),
    "nrg_hashmap_dump": (C.c_int, [vp, vp, vp, u64, u64p]),
    "nrg_hashmap_digest": (C.c_int, [vp, vp]),
    "nrg_stack_init": (C.c_int, [vp, vp, u64]),
    "nrg_stack_peek": (C.c_int, [vp, C.POINTER(u32), C.POINTER(C.c_uint8)]),
    "nrg_stack_len": (C.c_int, [vp, u64p]),
    "nrg_stack_dump": (C.c_int, [vp, vp, u64, u64p]),
    "nrg_stack_reserve": (C.c_int, [vp, u64]),
    "nrg_stack_capacity": (C.c_int, [vp, u64p]),
    "nrg_queue_init": (C.c_int, [vp, vp, u64]),
    "nrg_queue_init_range": (C.c_int, [vp, u64]),
    "nrg_queue_len": (C.c_int, [vp, u64p]),
    "nrg_queue_dump": (C.c_int, [vp, vp, u64, u64p]),
    "nrg_queue_reserve": (C.c_int, [vp, u64]),
    "nrg_queue_capacity": (C.c_int, [vp, u64p]),
    "nrg_queue_round_async": (C.c_int, [vp, vp, u64, u32, vp, vp]),
    "nrg_vspace_round_async": (C.c_int, [vp, vp, u64, u32, vp, vp]),
    "nrg_vspace_resolve": (C.c_int, [vp, vp, u64, vp, vp]),
    "nrg_vspace_resolve_async": (C.c_int, [vp, vp, u64, vp, vp]),
    "nrg_vspace_tables": (C.c_int, [vp, u64p]),
    "nrg_vspace_dump": (C.c_int, [vp, vp, u64, u64p]),
    "nrg_vspace_reserve": (C.c_int, [vp, u64]),
    "nrg_vspace_capacity": (C.c_int, [vp, u64p]),
    "nrg_skiplist_round_async": (C.c_int, [vp, vp, u64, u32, vp, vp]),
    "nrg_skiplist_get": (C.c_int, [vp, vp, u64, vp, vp]),
    "nrg_skiplist_get_async": (C.c_int, [vp, vp, u64, vp, vp]),
    "nrg_skiplist_seek": (C.c_int, [vp, vp, u64, u32, vp, vp, vp]),
    "nrg_skiplist_seek_async": (C.c_int, [vp, vp, u64, u32, vp, vp, vp]),
    "nrg_skiplist_scan": (C.c_int, [vp, vp, u64, u32, u32, vp, vp, vp]),
    "nrg_skiplist_scan_async": (C.c_int, [vp, vp, u64, u32, u32, vp, vp, vp]),
    "nrg_skiplist_range": (C.c_int, [vp, u64, u64, vp, vp, u64, u64p]),
    "nrg_skiplist_range_count": (C.c_int, [vp, vp, vp, u64, vp]),
    "nrg_skiplist_range_count_async": (C.c_int, [vp, vp, vp, u64, vp]),
    "nrg_skiplist_dump": (C.c_int, [vp, vp, vp, u64, u64p]),
    "nrg_skiplist_len": (C.c_int, [vp, u64p]),
    "nrg_skiplist_prefill": (C.c_int, [vp, vp, vp, u64]),
    "nrg_skiplist_prefill_range": (C.c_int, [vp, u64, u64]),
    "nrg_skiplist_prefill_partition": (C.c_int, [vp, u64, u64, C.c_uint32, C.c_uint32]),
    "nrg_skiplist_reserve": (C.c_int, [vp, u64]),
    "nrg_skiplist_capacity": (C.c_int, [vp, u64p]),
    "nrg_skiplist_enable_removal": (C.c_int, [vp, u64]),
    "nrg_skiplist_removal": (C.c_int, [vp, u64p, C.POINTER(C.c_int)]),
    "nrg_skiplist_enable_pops": (C.c_int, [vp, u64, u64]),
    "nrg_skiplist_pops": (C.c_int, [vp, u64p, u64p, C.POINTER(C.c_int)]),
    "nrg_skiplist_round_pops_async": (C.c_int, [vp, vp, u64, u32, vp, vp, vp, vp, u64, vp]),
    "nrg_skiplist_pop": (C.c_int, [vp, C.c_int, u64, u32, vp, vp, u64p]),
    "nrg_memfs_round_async": (C.c_int, [vp, vp, u64, u32, vp, vp]),
    "nrg_memfs_init": (C.c_int, [vp, u64, vp, u64]),
    "nrg_memfs_read": (C.c_int, [vp, u64, u64, u64, vp, u64p]),
    "nrg_memfs_dump": (C.c_int, [vp, u64, vp, u64, u64p]),
    "nrg_memfs_geometry": (C.c_int, [vp, u64p, u64p]),
    "nrg_memfs_enable_sizes": (C.c_int, [vp]),
    "nrg_memfs_size": (C.c_int, [vp, u64, u64p]),
    "nrg_memfs_truncate": (C.c_int, [vp, u64, u64]),
    "nrg_memfs_reserve": (C.c_int, [vp, u64]),
    "nrg_memfs_max_capacity": (C.c_int, [vp, u64p]),
    "nrg_memfs_pread": (C.c_int, [vp, vp, u64, vp, u64, vp, vp]),
    "nrg_memfs_pread_async": (C.c_int, [vp, vp, u64, vp, u64, vp, vp]),
    "nrg_memfs_pwrite_plan": (C.c_int, [u32, u64, vp, u64, u64, vp, vp, vp]),
    "nrg_memfs_pwrite_async": (C.c_int, [vp, vp, u64, vp, u64, u32, vp, vp, u64p]),
    "nrg_memfs_pwrite": (C.c_int, [vp, vp, u64, vp, u64, u32, vp, vp, u64p]),
    "nrg_memfs_pwrite_records_async": (C.c_int, [vp, vp, u64, vp, u64, vp, u64, u64p]),
    "nrg_memfs_pread_logged_plan": (C.c_int, [u32, u64, vp, u64, vp, vp, vp]),
    "nrg_memfs_pread_logged_async": (C.c_int, [vp, vp, u64, u32, vp, u64, vp, vp, vp, u64p]),
    "nrg_memfs_pread_logged": (C.c_int, [vp, vp, u64, u32, vp, u64, vp, vp, vp, u64p]),
    "nrg_memfs_pread_logged_records_async": (C.c_int, [vp, vp, u64, vp, u64, u64p]),
    "nrg_memfs_pread_logged_gather_async": (C.c_int, [vp, vp, u64, vp, vp, u64, vp, u64, vp, vp]),
    "nrg_synth_read": (C.c_int, [vp, vp, u64, vp]),
    "nrg_synth_read_async": (C.c_int, [vp, vp, u64, vp]),
    "nrg_synth_dump": (C.c_int, [vp, vp, u64, u64p]),
    "nrg_dev_alloc": (C.c_int, [vp, u64, C.POINTER(vp)]),
    "nrg_dev_free": (C.c_int, [vp, vp]),
    "nrg_memcpy_h2d": (C.c_int, [vp, vp, vp, u64]),
    "nrg_memcpy_d2h": (C.c_int, [vp, vp, vp, u64]),
    "nrg_gen_uniform_async": (C.c_int, [vp, vp, u64, u64, u64]),
    "nrg_gen_raw_async": (C.c_int, [vp, vp, u64, u64]),
    "nrg_gen_puts_async": (C.c_int, [vp, vp, vp, vp, u64]),
    "nrg_gen_zipf_async": (C.c_int, [vp, vp, u64, u64, u64, C.c_double, C.c_int]),
    "nrg_gen_stack_ops_async": (C.c_int, [vp, vp, u64, u64]),
    "nrg_kernel_timing": (C.c_int, [vp, C.c_int]),
    "nrg_kernel_timing_only": (C.c_int, [vp, C.c_char_p]),
    "nrg_kernel_time": (C.c_int, [vp, C.c_char_p, u64p, C.POINTER(C.c_double)]),
    "nrg_group_unique_id": (C.c_int, [vp]),
    "nrg_group_join": (C.c_int, [vp, vp, C.c_int, C.c_int, C.POINTER(vp)]),
    "nrg_group_open": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.POINTER(Config), C.POINTER(vp)]),
    "nrg_group_close": (C.c_int, [vp]),
    "nrg_group_info": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "nrg_group_replica": (vp, [vp, C.c_int]),
    "nrg_group_set_input_stream": (C.c_int, [vp, C.c_int, vp]),
    "nrg_group_round_async": (C.c_int, [vp, C.POINTER(Round), u64p]),
    "nrg_group_sync": (C.c_int, [vp]),
    "nrg_group_set_timeout": (C.c_int, [vp, u32]),
    "nrg_group_last_error": (C.c_char_p, [vp]),
    "nrg_combiner_open": (C.c_int, [vp, u32, C.POINTER(vp)]),
    "nrg_combiner_close": (C.c_int, [vp]),
    "nrg_combiner_register": (C.c_int, [vp, C.POINTER(u32)]),
    "nrg_combiner_put": (C.c_int, [vp, u32, vp, vp, u32, vp, vp]),
    "nrg_combiner_execute_mut": (C.c_int, [vp, u32, vp, u32, vp, vp]),
    "nrg_combiner_execute": (C.c_int, [vp, u32, vp, u32, vp, vp]),
    "nrg_combiner_get": (C.c_int, [vp, u32, vp, u32, vp, vp]),
    "nrg_combiner_stats": (C.c_int, [vp, u64p, u64p]),
    "nrg_key_owner": (C.c_uint32, [u64, C.c_uint32]),
    "nrg_hashmap_partition_async": (C.c_int, [vp, vp, u64, vp, u64, C.c_uint32, vp, vp, vp, vp, vp]),
    "nrg_route_back_async": (C.c_int, [vp, vp, vp, vp, u64, vp, vp]),
    "nrg_hashmap_prefill_partition": (C.c_int, [vp, u64, u64, C.c_uint32, C.c_uint32]),
    "nrg_group_partitioned_round": (C.c_int, [vp, C.POINTER(Round)]),
    "nrg_group_partitioned_round_async": (C.c_int, [vp, C.POINTER(Round)]),
    "nrg_group_partitioned_flush": (C.c_int, [vp]),
    "nrg_memfs_owner": (C.c_uint32, [u64, C.c_uint32]),
    "nrg_memfs_partition_async": (C.c_int, [vp, vp, u64, C.c_uint32, vp, vp, vp]),
    "nrg_memfs_route_back_async": (C.c_int, [vp, vp, vp, vp, u64, vp, vp]),
    "nrg_group_file_round": (C.c_int, [vp, C.POINTER(Round)]),
    "nrg_memfs_rd_partition_async": (C.c_int, [vp, vp, u64, C.c_uint32, vp, vp, vp]),
    "nrg_memfs_pread_repack_async": (C.c_int, [vp, vp, vp, vp, vp, u64, vp, u64, vp, vp]),
    "nrg_group_memfs_pread": (C.c_int, [vp, C.POINTER(Pread)]),
    "nrg_group_skiplist_seek": (C.c_int, [vp, C.POINTER(Seek), C.c_uint32]),
    "nrg_group_skiplist_range_count": (C.c_int, [vp, C.POINTER(Count)]),
    "nrg_group_skiplist_scan": (C.c_int, [vp, C.POINTER(Scan), C.c_uint32, C.c_uint32]),
    "nrg_group_skiplist_enable_removal": (C.c_int, [vp, u64]),
    "nrg_group_skiplist_enable_pops": (C.c_int, [vp, u64, u64]),
    "nrg_group_skiplist_pop": (C.c_int, [vp, C.POINTER(Pops)]),
}

# include/nrgpu_testing.h (kernel unit-test hooks)
TEST_SIGNATURES = {
    "nrg_test_combiner_probe": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "nrg_test_combiner_times": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "nrg_test_sort_pairs": (C.c_int, [vp, vp, vp, u64, C.c_int, vp, vp]),
    "nrg_test_maxscan": (C.c_int, [vp, vp, vp, u64, vp]),
    "nrg_test_lds_add_order": (C.c_int, [vp, u32, u32, u32, vp]),
    "nrg_test_ring_read": (C.c_int, [vp, u64, vp]),
    "nrg_test_debug_read": (C.c_int, [vp, vp, u64]),
    "nrg_test_vspace_table": (C.c_int, [vp, u64, vp]),
    "nrg_test_hm_skewed": (C.c_int, [vp, vp]),
    "nrg_test_set_knob": (C.c_int, [vp, C.c_int, u64]),
    "nrg_test_loopback_collectives": (C.c_int, [C.c_int]),
    "nrg_test_group_launches": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
}

# nrg_test_set_knob knobs (include/nrgpu_testing.h): tuning and diagnostics of an open context
KNOBS = {"STAMP_MAX": 1, "SKEW_EVERY": 2, "EPOCH_LIMIT": 3, "K1": 4, "EXP": 6, "SY_SORT": 7,
         "PIPELINE": 8, "COMB_SPIN": 10, "COMB_DEPTH": 11,
         "SMALL_MAX": 12, "PART": 13, "STALL": 14, "COMB_GATHER": 15, "PA_TPB": 16, "COMB_SERVE": 17, "SY_FUSED": 18,
         "SL_DELTA_MAX": 20}

_lib = None


def load(path: str = LIB_PATH):
    """Load libnrgpu.so; raises OSError (loudly) if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(path):
            raise OSError(f"libnrgpu.so not built at {path}: run `make -C node-replication_amd` "
                          "(or __graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(path)
        for name, (res, args) in {**SIGNATURES, **TEST_SIGNATURES}.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def check(code: int, what: str = ""):
    if code != NRG_OK:
        raise NrgError(code, what)
    return code


def default_config(kind: int) -> Config:
    cfg = Config()
    load().nrg_config_default(C.byref(cfg), kind)
    return cfg
