"""nrgpu — MI355X-native node-replication log replay (host side).

The data plane lives in libnrgpu.so (HIP kernels for gfx950 behind the C ABI of
include/nrgpu.h). This package mirrors the reference `nr` crate's API on top of it.
"""
from . import _lib, digest, snapshot
from ._lib import NrgError, load
from .combiner import Combiner
from .replica import (
    MEMFS_OP_DTYPE,
    MEMFS_RD_DTYPE,
    MEMFS_RESP_DTYPE,
    MEMFS_WR_DTYPE,
    PUT_DTYPE,
    QUEUE_OP_DTYPE,
    STACK_OP_DTYPE,
    SYNTH_OP_DTYPE,
    SYNTH_RD_DTYPE,
    VSPACE_LEAF_DTYPE,
    VSPACE_OP_DTYPE,
    VSPACE_RESP_DTYPE,
    AbstractDataStructure,
    DeviceReplica,
    Get,
    Identify,
    Len,
    Log,
    Map,
    MapDevice,
    MemFs,
    MfGetAttr,
    MfPread,
    MfPreadLogged,
    MfPwrite,
    MfRead,
    MfSetAttr,
    MfWrite,
    NrHashMap,
    Peek,
    Pop,
    Push,
    Put,
    Queue,
    ReadOnly,
    ReadWrite,
    Remove,
    Replica,
    ReplicaToken,
    Scan,
    Seek,
    SkipList,
    SlPush,
    SlRemove,
    SlPopFront,
    SlPopBack,
    Stack,
    VSpace,
    WriteOnly,
    memfs_pread_logged_plan,
    memfs_pwrite_plan,
    memfs_rd,
    memfs_wr,
)

__all__ = [
    "_lib", "digest", "snapshot", "NrgError", "load", "Combiner", "PUT_DTYPE", "QUEUE_OP_DTYPE", "STACK_OP_DTYPE", "SYNTH_OP_DTYPE", "SYNTH_RD_DTYPE",
    "AbstractDataStructure", "DeviceReplica", "Get", "Len", "Log", "NrHashMap", "Peek", "Pop", "Push", "Put", "Queue",
    "ReadOnly", "ReadWrite", "Remove", "Replica", "ReplicaToken", "Stack", "WriteOnly",
    "VSPACE_LEAF_DTYPE", "VSPACE_OP_DTYPE", "VSPACE_RESP_DTYPE", "Identify", "Map", "MapDevice", "VSpace",
    "Scan", "Seek", "SkipList", "SlPush", "SlRemove", "SlPopFront", "SlPopBack",
    "MEMFS_OP_DTYPE", "MEMFS_RD_DTYPE", "MEMFS_RESP_DTYPE", "MemFs", "MfGetAttr", "MfPread", "MfRead", "MfSetAttr", "MfWrite",
    "MEMFS_WR_DTYPE", "MfPwrite", "memfs_pwrite_plan", "memfs_wr",
    "MfPreadLogged", "memfs_pread_logged_plan", "memfs_rd",
    "FilePartitionedGroup", "PartitionedGroup", "ReplicaGroup", "memfs_owner", "key_owner",
]


def __getattr__(name):
    # the groups live in nrgpu.parallel, which needs torch.distributed: loaded on first use
    if name in ("parallel", "FilePartitionedGroup", "PartitionedGroup", "ReplicaGroup", "memfs_owner", "key_owner"):
        import importlib

        mod = importlib.import_module(".parallel", __name__)
        return mod if name == "parallel" else getattr(mod, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def device_count() -> int:
    return int(load().nrg_device_count())
