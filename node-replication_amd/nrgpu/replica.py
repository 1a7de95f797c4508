"""Host side of the MI355X NR replica, mirroring the `nr` crate's API over the C ABI.

  DeviceReplica   one nrg_ctx: a replica on one GPU (data structure + HBM log ring)
  Log             nr::Log         (nr/src/log.rs)       — the logical shared log; each GPU
                                   replica holds a physical copy in HBM
  Replica         nr::Replica<D>  (nr/src/replica.rs)   — register / execute_mut / execute /
                                   sync / verify, with flat combining of the registered
                                   threads' pending ops into one log append + one replay
  ReplicaToken    nr::ReplicaToken
  NrHashMap, Stack, AbstractDataStructure, Queue, VSpace, SkipList, MemFs — the Dispatch plug-ins
                                   of the reference (benches/hashmap.rs, benches/stack.rs,
                                   benches/synthetic.rs, benches/lockfree_comparisons.rs,
                                   benches/vspace.rs, benches/lockfree_partitioned.rs, benches/memfs.rs)
"""
from __future__ import annotations

import ctypes as C
import sys
import threading
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import numpy as np

from . import _lib as L
from . import snapshot as _snapshot

PUT_DTYPE = np.dtype([("key", "<u8"), ("val", "<u8")])
# DeviceReplica.sl_enable_pops' default marks (the default tombstone is 2^64 - 1)
SL_FRONT_MARK, SL_BACK_MARK = 2**64 - 2, 2**64 - 3
STACK_OP_DTYPE = np.dtype([("val", "<u4"), ("op", "<u4")])
QUEUE_OP_DTYPE = np.dtype([("val", "<u8"), ("op", "<u8")])
SYNTH_OP_DTYPE = np.dtype([("tid", "<u8"), ("r1", "<u8"), ("r2", "<u8"), ("op", "<u8")])
SYNTH_RD_DTYPE = np.dtype([("tid", "<u8"), ("r1", "<u8"), ("r2", "<u8")])
VSPACE_OP_DTYPE = L.VSPACE_OP_DTYPE
VSPACE_RESP_DTYPE = L.VSPACE_RESP_DTYPE
VSPACE_LEAF_DTYPE = L.VSPACE_LEAF_DTYPE
MEMFS_OP_DTYPE = L.MEMFS_OP_DTYPE
MEMFS_RESP_DTYPE = L.MEMFS_RESP_DTYPE
MEMFS_RD_DTYPE = L.MEMFS_RD_DTYPE
MEMFS_WR_DTYPE = L.MEMFS_WR_DTYPE

# nr/src/log.rs:22,26,36 ; nr/src/context.rs:12 ; nr/src/replica.rs:56
DEFAULT_LOG_BYTES = 32 * 1024 * 1024
MAX_REPLICAS = 192
MAX_PENDING_OPS = 32
MAX_THREADS_PER_REPLICA = 256
GC_FROM_HEAD = MAX_PENDING_OPS * MAX_THREADS_PER_REPLICA


def _ptr(a: np.ndarray):
    return C.c_void_p(a.ctypes.data)


def _dptr(t) -> C.c_void_p:
    """device pointer of a torch tensor / int / None"""
    if t is None:
        return C.c_void_p(0)
    if isinstance(t, int):
        return C.c_void_p(t)
    return C.c_void_p(t.data_ptr())


def memfs_wr(reqs) -> np.ndarray:
    """Requests of nrg_memfs_pwrite* as a contiguous array of MEMFS_WR_DTYPE: from one, or from
    [n, 4] u64 (ino, offset, len, data_off)."""
    host = np.asarray(reqs)
    if host.dtype != L.MEMFS_WR_DTYPE:
        host = np.ascontiguousarray(host, np.uint64).reshape(-1, 4).view(L.MEMFS_WR_DTYPE)
    return np.ascontiguousarray(host.reshape(-1))


def memfs_pwrite_plan(log2_b: int, files: int, reqs, data_bytes: int):
    """The cut of nrg_memfs_pwrite* as host arithmetic (nrg_memfs_pwrite_plan; no device, no context):
    (first, written, some) for F = `files` files of 2^log2_b bytes. first[0..n] is the running sum of the
    requests' record counts, first[n] the records of the call. ValueError for what the library refuses:
    a geometry nrg_open does not accept, or a valid request whose bytes are not inside data."""
    rq = memfs_wr(reqs)
    n = len(rq)
    first = np.zeros(n + 1, np.uint64)
    written = np.zeros(n, np.uint64)
    some = np.zeros(n, np.uint8)
    code = L.load().nrg_memfs_pwrite_plan(log2_b, files, _ptr(rq) if n else None, n, data_bytes, _ptr(first),
                                          _ptr(written) if n else None, _ptr(some) if n else None)
    if code == L.NRG_E_INVAL:
        raise ValueError("nrg_memfs_pwrite_plan: a geometry nrg_open refuses, or a request's bytes lie outside data")
    L.check(code, "memfs_pwrite_plan")
    return first, written, some


def memfs_rd(reqs) -> np.ndarray:
    """Requests of nrg_memfs_pread* as a contiguous array of MEMFS_RD_DTYPE: from one, or from
    [n, 3] u64 (ino, offset, len)."""
    host = np.asarray(reqs)
    if host.dtype != L.MEMFS_RD_DTYPE:
        host = np.ascontiguousarray(host, np.uint64).reshape(-1, 3).view(L.MEMFS_RD_DTYPE)
    return np.ascontiguousarray(host.reshape(-1))


def memfs_pread_logged_plan(log2_adm: int, files: int, reqs):
    """The cut of nrg_memfs_pread_logged* as host arithmetic (nrg_memfs_pread_logged_plan; no device, no
    context): (first, offs, some) for F = `files` files admitted against 2^log2_adm bytes. first[0..n] is
    the running sum of the requests' record counts, offs[0..n] the running sum of the bytes they plan to
    read (request i owns data[offs[i]:offs[i + 1]]). ValueError for a geometry nrg_open does not accept."""
    rq = memfs_rd(reqs)
    n = len(rq)
    first = np.zeros(n + 1, np.uint64)
    offs = np.zeros(n + 1, np.uint64)
    some = np.zeros(n, np.uint8)
    code = L.load().nrg_memfs_pread_logged_plan(log2_adm, files, _ptr(rq) if n else None, n, _ptr(first), _ptr(offs),
                                                _ptr(some) if n else None)
    if code == L.NRG_E_INVAL:
        raise ValueError("nrg_memfs_pread_logged_plan: a geometry nrg_open refuses")
    L.check(code, "memfs_pread_logged_plan")
    return first, offs, some


def _stream_ordered(fn):
    """Stream-ordering contract of every `*_device` helper (and join): the call is ordered AFTER
    all work already queued on torch's current stream (so buffers torch filled or copied there
    are ready), and torch's current stream is ordered AFTER the work the call queued on this
    replica's stream (so torch reads of the outputs see them). When the replica already runs on
    torch's current stream (use_torch_stream) this is free; otherwise two events cross the
    streams. With config.pipeline = 1 a round's deferred outputs are complete only after join(),
    which is ordered the same way. Without this, a replica on its own non-blocking stream
    (nrg_open's default, include/nrgpu.h nrg_set_stream) races torch's null-stream fills."""

    def wrapped(self, *a, **kw):
        cross = self._cross_streams()
        if cross is None:
            return fn(self, *a, **kw)
        cur, mine = cross
        mine.wait_stream(cur)
        try:
            return fn(self, *a, **kw)
        finally:
            cur.wait_stream(mine)

    wrapped.__name__ = fn.__name__
    wrapped.__doc__ = fn.__doc__
    return wrapped


class DeviceReplica:
    """Thin owner of one nrg_ctx (one replica in one GPU's HBM).

    Stream contract: the replica queues its GPU work on its own stream (nrg_own_stream, not
    ordered with the null stream) until use_torch_stream / set_stream says otherwise. Every
    `*_device` method and join() is nevertheless ordered with torch's current stream in both
    directions (`_stream_ordered`), so torch tensors may be filled, passed and read back on
    torch's stream without extra synchronisation. Host-pointer methods are synchronous."""

    def __init__(self, kind: int, device: int = 0, knobs: Optional[dict] = None, **cfg):
        """`cfg`: nrg_config fields; `knobs`: {name: value} of nrg_test_set_knob (tuning and
        diagnostics, include/nrgpu_testing.h), applied right after nrg_open."""
        lib = L.load()
        self.kind = kind
        self.device = device
        c = L.default_config(kind)
        for k, v in cfg.items():
            if not hasattr(c, k):
                raise TypeError(f"unknown config field {k}")
            setattr(c, k, v)
        self.cfg = c
        h = C.c_void_p()
        L.check(lib.nrg_open(device, C.byref(c), C.byref(h)), "nrg_open")
        self._h = h
        self._lib = lib
        for k, v in (knobs or {}).items():
            self.set_knob(k, v)

    def set_knob(self, name: str, value: int):
        """nrg_test_set_knob: a tuning/diagnostic knob by name (L.KNOBS) on this open context."""
        L.check(self._lib.nrg_test_set_knob(self._h, L.KNOBS[name], int(value)), f"knob {name}")

    # -- lifetime ------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            if getattr(self, "_snap", (0, 0))[0]:  # the snapshot buffer (snapshot_device / restore)
                self._lib.nrg_dev_free(self._h, C.c_void_p(self._snap[0]))
                self._snap = (0, 0)
            self._lib.nrg_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    @property
    def handle(self):
        return self._h

    def set_stream(self, stream_ptr: int):
        L.check(self._lib.nrg_set_stream(self._h, C.c_void_p(stream_ptr)), "nrg_set_stream")

    def use_torch_stream(self):
        """Order this replica's work with torch's current stream on its device (the null
        stream when torch is on its default stream)."""
        import torch

        self.set_stream(torch.cuda.current_stream(self.device).cuda_stream)

    def use_own_stream(self):
        self.set_stream(self._lib.nrg_own_stream(self._h) or 0)

    def _cross_streams(self):
        """(torch's current stream, this replica's stream as a torch stream) when the two differ
        and torch drives a GPU; None when no ordering is needed."""
        torch = sys.modules.get("torch")
        if torch is None or not torch.cuda.is_available():
            return None
        cur = torch.cuda.current_stream(self.device)
        mine = self._lib.nrg_get_stream(self._h) or 0
        if cur.cuda_stream == mine:
            return None
        cache = getattr(self, "_ext_stream", None)
        if cache is None or cache[0] != mine:
            s = (torch.cuda.default_stream(self.device) if mine == 0
                 else torch.cuda.ExternalStream(mine, device=torch.device("cuda", self.device)))
            cache = self._ext_stream = (mine, s)
        return cur, cache[1]

    def sync(self):
        L.check(self._lib.nrg_sync(self._h), "nrg_sync")

    @_stream_ordered
    def join(self):
        """Order outstanding side-stream reads (pipeline=1) on this replica's stream.
        Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        L.check(self._lib.nrg_join(self._h), "nrg_join")

    # -- log -----------------------------------------------------------------------
    def log_state(self) -> dict:
        info = L.LogInfo()
        L.check(self._lib.nrg_log_state(self._h, C.byref(info)))
        return {f: getattr(info, f) for f, _ in L.LogInfo._fields_}

    def log_append(self, recs: np.ndarray, origin: int) -> int:
        recs = np.ascontiguousarray(recs)
        first = C.c_uint64()
        L.check(self._lib.nrg_log_append(self._h, _ptr(recs), len(recs), origin, C.byref(first)), "append")
        return first.value

    @_stream_ordered
    def log_append_device(self, d_recs, n: int, origin: int) -> int:
        """Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        first = C.c_uint64()
        L.check(self._lib.nrg_log_append_async(self._h, _dptr(d_recs), n, origin, C.byref(first)), "append")
        return first.value

    @_stream_ordered
    def log_append_segments(self, d_base, seg_stride: int, lens: Sequence[int], origins: Sequence[int]):
        """Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        key = (tuple(lens), tuple(origins))
        if getattr(self, "_seg_key", None) != key:  # marshalled once per distinct round shape
            nseg = len(lens)
            self._seg_key = key
            self._seg_arrays = ((C.c_uint64 * nseg)(*lens), (C.c_uint32 * nseg)(*origins), nseg)
        la, oa, nseg = self._seg_arrays
        fa = (C.c_uint64 * nseg)()
        L.check(self._lib.nrg_log_append_segments_async(self._h, _dptr(d_base), nseg, seg_stride, la, oa, fa),
                "append_segments")
        return list(fa)

    def _resp_dtype(self):
        if self.kind == L.NRG_DS_STACK:
            return np.uint32
        if self.kind == L.NRG_DS_VSPACE:
            return VSPACE_RESP_DTYPE  # (a, b): Ok((a, b)), or Err(at = a) where some = 0
        if self.kind == L.NRG_DS_MEMFS:
            return MEMFS_RESP_DTYPE  # (n, data[128]): Written(n) / Data(data[:n]) / the size, or the error n
        # hashmap previous values, synthetic sums, queue pushed / popped values
        return np.uint64

    def log_exec_rc(self, resp_lo: int = 0, resp_hi: int = 0):
        """nrg_log_exec with its code kept: (code, resp, some). The responses are copied out before the
        error latch is read, so they are valid under NRG_E_INVAL too (a record outside its kind's domain)."""
        n = resp_hi - resp_lo
        resp = np.zeros(max(n, 1), self._resp_dtype())
        some = np.zeros(max(n, 1), np.uint8)
        if n > 0:
            rc = self._lib.nrg_log_exec(self._h, resp_lo, resp_hi, _ptr(resp), _ptr(some))
        else:
            rc = self._lib.nrg_log_exec(self._h, 0, 0, None, None)
        return rc, resp[:n], some[:n]

    def log_exec(self, resp_lo: int = 0, resp_hi: int = 0):
        rc, resp, some = self.log_exec_rc(resp_lo, resp_hi)
        L.check(rc, "exec")
        return resp, some

    @_stream_ordered
    def log_exec_device(self, resp_lo=0, resp_hi=0, d_resp=None, d_some=None):
        """Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        L.check(self._lib.nrg_log_exec_async(self._h, resp_lo, resp_hi, _dptr(d_resp), _dptr(d_some)), "exec")

    @_stream_ordered
    def st_round_device(self, d_ops, n: int, origin: int, d_resp=None, d_some=None):
        """Replica::combine for one stack batch on device buffers: append + exec in one replay
        pass (nrg_stack_round_async); Pop responses for these ops into d_resp / d_some.
        Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        L.check(self._lib.nrg_stack_round_async(self._h, _dptr(d_ops), n, origin, _dptr(d_resp), _dptr(d_some)),
                "stack_round")

    @_stream_ordered
    def sy_round_device(self, d_ops, n: int, origin: int, d_resp=None, d_some=None):
        """Replica::combine for one synthetic batch on device buffers (nrg_synth_round_async).
        Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        L.check(self._lib.nrg_synth_round_async(self._h, _dptr(d_ops), n, origin, _dptr(d_resp), _dptr(d_some)),
                "synth_round")

    @_stream_ordered
    def qu_round_device(self, d_ops, n: int, origin: int, d_resp=None, d_some=None):
        """Replica::combine for one queue batch on device buffers: append + exec, the log copy
        written by the replay (nrg_queue_round_async); responses (u64 pushed or popped value)
        for these ops into d_resp / d_some.
        Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        L.check(self._lib.nrg_queue_round_async(self._h, _dptr(d_ops), n, origin, _dptr(d_resp), _dptr(d_some)),
                "queue_round")

    @_stream_ordered
    def vs_round_device(self, d_ops, n: int, origin: int, d_resp=None, d_some=None):
        """Replica::combine for one page-table batch on device buffers: append + exec, the log
        copy written by the replay (nrg_vspace_round_async); responses (16 B {a, b} each) for
        these ops into d_resp / d_some.
        Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        L.check(self._lib.nrg_vspace_round_async(self._h, _dptr(d_ops), n, origin, _dptr(d_resp), _dptr(d_some)),
                "vspace_round")

    @_stream_ordered
    def sl_round_device(self, d_ops, n: int, origin: int, d_resp=None, d_some=None):
        """Replica::combine for one skip-list batch of Push(k, v) records on device buffers: append +
        exec, the log copy written by the replay (nrg_skiplist_round_async); responses (the key,
        some = 1) for these ops into d_resp / d_some.
        Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        L.check(self._lib.nrg_skiplist_round_async(self._h, _dptr(d_ops), n, origin, _dptr(d_resp), _dptr(d_some)),
                "skiplist_round")

    @_stream_ordered
    def mf_round(self, d_ops, n: int, origin: int, d_resp=None, d_some=None):
        """Replica::combine for one file-store batch of Write / Read / GetAttr records (152 B each) on
        device buffers: append + exec, the log copy written by the replay (nrg_memfs_round_async);
        responses (136 B {n, data[128]} each) for these ops into d_resp / d_some.
        Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        L.check(self._lib.nrg_memfs_round_async(self._h, _dptr(d_ops), n, origin, _dptr(d_resp), _dptr(d_some)),
                "memfs_round")

    def log_reset(self):
        L.check(self._lib.nrg_log_reset(self._h))

    # -- verify --------------------------------------------------------------------
    def digest(self):
        """nrg_digest: (count, sum, xor) of the structure's items, any kind; nrgpu.digest mirrors
        the definition. On a hashmap the same as hm_digest()."""
        out = np.zeros(3, np.uint64)
        L.check(self._lib.nrg_digest(self._h, _ptr(out)), "digest")
        return tuple(int(x) for x in out)

    @_stream_ordered
    def digest_device(self, d_out3):
        """nrg_digest_async: the triple into three u64 on the device, no host round trip.
        Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        L.check(self._lib.nrg_digest_async(self._h, _dptr(d_out3)), "digest")

    # -- snapshot / restore ----------------------------------------------------------
    def _info(self, s: "L.SnapshotInfo"):
        from .snapshot import Info

        return Info(s.ds_kind, s.version, s.items, s.bytes, s.log_idx, tuple(int(x) for x in s.digest))

    def snapshot_info(self):
        """nrg_snapshot_size: what a snapshot taken now would hold (snapshot.Info; digest zero)."""
        s = L.SnapshotInfo()
        L.check(self._lib.nrg_snapshot_size(self._h, C.byref(s)), "snapshot_size")
        return self._info(s)

    def _snap_buf(self, nbytes: int) -> int:
        """a device buffer of this replica's, kept and grown for its snapshots and restores"""
        if getattr(self, "_snap", (0, 0))[1] < nbytes:
            if getattr(self, "_snap", (0, 0))[0]:
                L.check(self._lib.nrg_dev_free(self._h, C.c_void_p(self._snap[0])), "dev_free")
                self._snap = (0, 0)
            p = C.c_void_p()
            L.check(self._lib.nrg_dev_alloc(self._h, nbytes, C.byref(p)), "dev_alloc")
            self._snap = (p.value, nbytes)
        return self._snap[0]

    def snapshot_device(self):
        """nrg_snapshot_async into a device buffer this replica owns: (device pointer, bytes, info),
        complete on return. The buffer is reused by the next snapshot or host restore and freed
        with the replica: restore from it, or copy it, before then."""
        want = self.snapshot_info()
        p = self._snap_buf(want.bytes)
        L.check(self._lib.nrg_snapshot_async(self._h, C.c_void_p(p), want.bytes), "snapshot")
        self.sync()
        s = L.SnapshotInfo()
        L.check(self._lib.nrg_snapshot_info_read(self._h, C.c_void_p(p), want.bytes, C.byref(s)), "snapshot_info_read")
        return p, int(s.bytes), self._info(s)

    def snapshot(self) -> np.ndarray:
        """The replica's state as a snapshot image on the host (u8 array; nrgpu.snapshot.unpack
        reads it, DeviceReplica.restore takes it back, tofile() keeps it)."""
        p, nbytes, _ = self.snapshot_device()
        out = np.zeros(nbytes, np.uint8)
        L.check(self._lib.nrg_memcpy_d2h(self._h, _ptr(out), C.c_void_p(p), nbytes), "d2h")
        return out

    def restore(self, buf, nbytes: Optional[int] = None):
        """nrg_restore: replace this replica's contents and log positions with a snapshot's. `buf`
        is a host image (u8 array or bytes) or, with `nbytes`, a device pointer (int or torch
        tensor) whose contents are complete."""
        if nbytes is None:
            b = _snapshot.as_u8(buf)
            if b.size < 64:
                raise L.NrgError(L.NRG_E_INVAL, "restore")
            p = self._snap_buf(b.size)
            L.check(self._lib.nrg_memcpy_h2d(self._h, C.c_void_p(p), _ptr(b), b.size), "h2d")
            L.check(self._lib.nrg_restore(self._h, C.c_void_p(p), b.size), "restore")
        else:
            L.check(self._lib.nrg_restore(self._h, _dptr(buf), nbytes), "restore")

    # -- hashmap -------------------------------------------------------------------
    def hm_get(self, keys: np.ndarray):
        keys = np.ascontiguousarray(keys, np.uint64)
        n = len(keys)
        vals = np.zeros(max(n, 1), np.uint64)
        found = np.zeros(max(n, 1), np.uint8)
        L.check(self._lib.nrg_hashmap_get(self._h, _ptr(keys), n, _ptr(vals), _ptr(found)), "get")
        return vals[:n], found[:n]

    @_stream_ordered
    def hm_get_device(self, d_keys, n, d_vals, d_found):
        """Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        L.check(self._lib.nrg_hashmap_get_async(self._h, _dptr(d_keys), n, _dptr(d_vals), _dptr(d_found)), "get")

    @_stream_ordered
    def hm_round_device(self, d_puts, W, origin, d_get_keys, R, d_get_vals, d_get_found, d_prev=None,
                        d_prev_found=None):
        """Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        L.check(self._lib.nrg_hashmap_round_async(self._h, _dptr(d_puts), W, origin, _dptr(d_get_keys), R,
                                                  _dptr(d_get_vals), _dptr(d_get_found), _dptr(d_prev),
                                                  _dptr(d_prev_found)), "round")

    @_stream_ordered
    def hm_round_segments_device(self, d_base, seg_stride, lens, origins, resp_seg, d_get_keys, R, d_get_vals,
                                 d_get_found, d_prev=None, d_prev_found=None):
        """Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        key = (tuple(lens), tuple(origins))
        if getattr(self, "_seg_key", None) != key:  # marshalled once per distinct round shape
            nseg = len(lens)
            self._seg_key = key
            self._seg_arrays = ((C.c_uint64 * nseg)(*lens), (C.c_uint32 * nseg)(*origins), nseg)
        la, oa, nseg = self._seg_arrays
        L.check(self._lib.nrg_hashmap_round_segments_async(
            self._h, _dptr(d_base), nseg, seg_stride, la, oa, resp_seg, _dptr(d_get_keys), R, _dptr(d_get_vals),
            _dptr(d_get_found), _dptr(d_prev), _dptr(d_prev_found)), "round_segments")

    def hm_prefill(self, keys: np.ndarray, vals: np.ndarray):
        keys = np.ascontiguousarray(keys, np.uint64)
        vals = np.ascontiguousarray(vals, np.uint64)
        L.check(self._lib.nrg_hashmap_prefill(self._h, _ptr(keys), _ptr(vals), len(keys)), "prefill")

    def hm_prefill_range(self, n: int, off: int = 1):
        L.check(self._lib.nrg_hashmap_prefill_range(self._h, n, off), "prefill_range")

    def hm_prefill_partition(self, n: int, off: int, part: int, parts: int):
        """NrHashMap::default restricted to key partition `part` of `parts` (nrg_key_owner)."""
        L.check(self._lib.nrg_hashmap_prefill_partition(self._h, n, off, part, parts), "prefill_partition")

    @_stream_ordered
    def hm_partition_device(self, d_puts, W, d_keys, R, parts, d_puts_out, d_put_pos, d_keys_out, d_get_pos, d_counts):
        """Stable partition of a round's Puts and Get keys by owner (nrg_hashmap_partition_async).
        Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        L.check(self._lib.nrg_hashmap_partition_async(self._h, _dptr(d_puts), W, _dptr(d_keys), R, parts,
                                                      _dptr(d_puts_out), _dptr(d_put_pos), _dptr(d_keys_out),
                                                      _dptr(d_get_pos), _dptr(d_counts)), "partition")

    @_stream_ordered
    def route_back_device(self, d_src, d_src8, d_pos, n, d_dst, d_dst8):
        """Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        L.check(self._lib.nrg_route_back_async(self._h, _dptr(d_src), _dptr(d_src8), _dptr(d_pos), n, _dptr(d_dst),
                                               _dptr(d_dst8)), "route_back")

    def partitioned_replay(self, puts, keys, want_prev: bool):
        """One owner's share of a key-partitioned round (nrgpu.parallel.PartitionedHashMap): replay
        the received Puts [p, 2] in the given (rank) order, answer the received Gets after them."""
        import torch

        dev = torch.device("cuda", self.device) if torch.cuda.is_available() else torch.device("cpu")
        p = puts.reshape(-1, 2).to(dev).contiguous()
        k = keys.reshape(-1).to(dev).contiguous()
        n, r = p.shape[0], k.shape[0]
        vals = torch.zeros(r, dtype=torch.int64, device=dev)
        found = torch.zeros(r, dtype=torch.uint8, device=dev)
        pv = torch.zeros(n, dtype=torch.int64, device=dev) if want_prev else None
        pf = torch.zeros(n, dtype=torch.uint8, device=dev) if want_prev else None
        self.use_torch_stream()
        self.hm_round_device(p, n, int(self.cfg.replica_id) or 1, k, r, vals, found, pv, pf)
        self.join()
        torch.cuda.synchronize(dev)
        return vals, found, pv, pf

    def hm_size(self) -> int:
        n = C.c_uint64()
        L.check(self._lib.nrg_hashmap_size(self._h, C.byref(n)))
        return n.value

    def hm_reserve(self, n_keys: int):
        """HashMap::reserve: a table large enough for `n_keys` keys in all (one key per two slots);
        never shrinks (nrg_hashmap_reserve). Synchronous."""
        if self.kind != L.NRG_DS_HASHMAP:
            raise TypeError("hm_reserve needs a hashmap replica")
        n_keys = int(n_keys)
        if n_keys < 0 or n_keys >= 2**64:
            raise ValueError("n_keys must be a u64")
        L.check(self._lib.nrg_hashmap_reserve(self._h, n_keys), "reserve")

    def hm_log2_slots(self) -> int:
        """log2 of the table's current number of slots (nrg_hashmap_capacity)."""
        if self.kind != L.NRG_DS_HASHMAP:
            raise TypeError("hm_log2_slots needs a hashmap replica")
        n = C.c_uint32()
        L.check(self._lib.nrg_hashmap_capacity(self._h, C.byref(n)), "capacity")
        return n.value

    def hm_enable_removal(self, tombstone: int = 2**64 - 1):
        """From here on a record whose val == tombstone is Remove(key) (nrg_hashmap_enable_removal).
        Idempotent for one tombstone; there is no way back. Every replica of a log enables it at the
        same log index. Refused while any present value equals the tombstone."""
        L.check(self._lib.nrg_hashmap_enable_removal(self._h, tombstone), "hashmap_enable_removal")

    def hm_removal(self):
        """The tombstone, or None while removal is off (nrg_hashmap_removal)."""
        t, on = C.c_uint64(), C.c_int()
        L.check(self._lib.nrg_hashmap_removal(self._h, C.byref(t), C.byref(on)), "hashmap_removal")
        return t.value if on.value else None

    def hm_remove(self, keys, origin: int = 1):
        """HashMap::remove for a batch, in order: Remove(key) records appended to the log and replayed.
        Returns (prev u64[n], found u8[n]): the value each key had at its log position, found = 0 (and
        prev = 0) where it was absent."""
        tomb = self.hm_removal()
        if tomb is None:
            raise L.NrgError(L.NRG_E_INVAL, "hm_remove: removal is not enabled (hm_enable_removal)")
        recs = np.zeros(len(keys), PUT_DTYPE)
        recs["key"], recs["val"] = np.asarray(keys, np.uint64), tomb
        if len(recs) == 0:
            return np.zeros(0, np.uint64), np.zeros(0, np.uint8)
        first = self.log_append(recs, origin)
        return self.log_exec(first, first + len(recs))

    def hm_occupancy(self) -> int:
        """Slots taken, live and dead (nrg_hashmap_occupancy); hm_size() is the live keys."""
        n = C.c_uint64()
        L.check(self._lib.nrg_hashmap_occupancy(self._h, C.byref(n)), "hashmap_occupancy")
        return n.value

    def hm_purge(self):
        """Drop the dead slots: a rehash into a table of the same size (nrg_hashmap_purge). Synchronous."""
        L.check(self._lib.nrg_hashmap_purge(self._h), "hashmap_purge")

    def hm_dump(self):
        """(keys, vals) sorted by key"""
        n = self.hm_size()
        k = np.zeros(max(n, 1), np.uint64)
        v = np.zeros(max(n, 1), np.uint64)
        m = C.c_uint64()
        L.check(self._lib.nrg_hashmap_dump(self._h, _ptr(k), _ptr(v), n, C.byref(m)), "dump")
        k, v = k[: m.value], v[: m.value]
        o = np.argsort(k, kind="stable")
        return k[o], v[o]

    def hm_digest(self):
        out = np.zeros(3, np.uint64)
        L.check(self._lib.nrg_hashmap_digest(self._h, _ptr(out)), "digest")
        return tuple(int(x) for x in out)

    # -- stack ---------------------------------------------------------------------
    def st_init(self, vals):
        vals = np.ascontiguousarray(np.asarray(vals, np.uint32))
        L.check(self._lib.nrg_stack_init(self._h, _ptr(vals), len(vals)), "stack_init")

    def st_peek(self):
        v = C.c_uint32()
        s = C.c_uint8()
        L.check(self._lib.nrg_stack_peek(self._h, C.byref(v), C.byref(s)), "peek")
        return int(v.value) if s.value else None

    def st_len(self) -> int:
        n = C.c_uint64()
        L.check(self._lib.nrg_stack_len(self._h, C.byref(n)))
        return n.value

    def st_dump(self) -> np.ndarray:
        n = self.st_len()
        out = np.zeros(max(n, 1), np.uint32)
        m = C.c_uint64()
        L.check(self._lib.nrg_stack_dump(self._h, _ptr(out), n, C.byref(m)), "stack_dump")
        return out[: m.value]

    def _reserve(self, fn, kind: int, what: str, n: int):
        if self.kind != kind:
            raise TypeError(f"{what} needs another kind of replica")
        n = int(n)
        if n < 0 or n >= 2**64:
            raise ValueError("the size must be a u64")
        L.check(fn(self._h, n), what)

    def _capacity(self, fn, kind: int, what: str) -> int:
        if self.kind != kind:
            raise TypeError(f"{what} needs another kind of replica")
        n = C.c_uint64()
        L.check(fn(self._h, C.byref(n)), what)
        return n.value

    def set_max_capacity(self, max_items: int):
        """Automatic growth of a stack, queue or skip-list replica up to `max_items` elements; 0 (the state after
        open) is a fixed capacity (nrg_set_max_capacity). Synchronous. A file store (sizes enabled) takes
        the bound in BYTES PER FILE, a power of two: a Write or SetAttr that ends within it is admitted and
        B grows to the power of two that holds it (include/nrgpu.h "File store: capacity growth")."""
        max_items = int(max_items)
        if max_items < 0 or max_items >= 2**64:
            raise ValueError("max_items must be a u64")
        L.check(self._lib.nrg_set_max_capacity(self._h, max_items), "set_max_capacity")

    def st_reserve(self, n_elems: int):
        """Vec::reserve: room for `n_elems` elements in all; never shrinks (nrg_stack_reserve)."""
        self._reserve(self._lib.nrg_stack_reserve, L.NRG_DS_STACK, "st_reserve", n_elems)

    def st_capacity(self) -> int:
        """Vec::capacity: the elements the stack has room for (nrg_stack_capacity)."""
        return self._capacity(self._lib.nrg_stack_capacity, L.NRG_DS_STACK, "st_capacity")

    # -- queue ---------------------------------------------------------------------
    def qu_reserve(self, n_elems: int):
        """Room for `n_elems` elements in all; never shrinks (nrg_queue_reserve)."""
        self._reserve(self._lib.nrg_queue_reserve, L.NRG_DS_QUEUE, "qu_reserve", n_elems)

    def qu_capacity(self) -> int:
        """The elements the queue has room for (nrg_queue_capacity)."""
        return self._capacity(self._lib.nrg_queue_capacity, L.NRG_DS_QUEUE, "qu_capacity")

    def qu_init(self, vals):
        """The queue holds `vals`, front first."""
        vals = np.ascontiguousarray(np.asarray(vals, np.uint64))
        L.check(self._lib.nrg_queue_init(self._h, _ptr(vals), len(vals)), "queue_init")

    def qu_init_range(self, n: int):
        """SegQueueWrapper::default: values 0..n-1 pushed in order."""
        L.check(self._lib.nrg_queue_init_range(self._h, n), "queue_init_range")

    def qu_len(self) -> int:
        n = C.c_uint64()
        L.check(self._lib.nrg_queue_len(self._h, C.byref(n)), "queue_len")
        return n.value

    def qu_dump(self) -> np.ndarray:
        """The elements, front first."""
        n = self.qu_len()
        out = np.zeros(max(n, 1), np.uint64)
        m = C.c_uint64()
        L.check(self._lib.nrg_queue_dump(self._h, _ptr(out), n, C.byref(m)), "queue_dump")
        return out[: m.value]

    # -- vspace --------------------------------------------------------------------
    def vs_reserve(self, n_tables: int):
        """A pool of `n_tables` page tables in all; never shrinks (nrg_vspace_reserve)."""
        self._reserve(self._lib.nrg_vspace_reserve, L.NRG_DS_VSPACE, "vs_reserve", n_tables)

    def vs_capacity(self) -> int:
        """The page tables the pool holds (nrg_vspace_capacity)."""
        return self._capacity(self._lib.nrg_vspace_capacity, L.NRG_DS_VSPACE, "vs_capacity")

    def vs_resolve(self, vaddrs):
        """Identify for a batch of virtual addresses: (paddrs, found); paddr 0 where unmapped."""
        vaddrs = np.ascontiguousarray(np.asarray(vaddrs, np.uint64))
        n = len(vaddrs)
        pa = np.zeros(max(n, 1), np.uint64)
        found = np.zeros(max(n, 1), np.uint8)
        L.check(self._lib.nrg_vspace_resolve(self._h, _ptr(vaddrs), n, _ptr(pa), _ptr(found)), "vspace_resolve")
        return pa[:n], found[:n]

    @_stream_ordered
    def vs_resolve_device(self, d_vaddrs, n: int, d_paddrs, d_found):
        """Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        L.check(self._lib.nrg_vspace_resolve_async(self._h, _dptr(d_vaddrs), n, _dptr(d_paddrs), _dptr(d_found)),
                "vspace_resolve")

    def vs_tables(self) -> int:
        """Tables allocated so far, the PML4 included."""
        n = C.c_uint64()
        L.check(self._lib.nrg_vspace_tables(self._h, C.byref(n)), "vspace_tables")
        return n.value

    def vs_dump(self) -> np.ndarray:
        """Every leaf entry as (vaddr, entry), in ascending vaddr (VSPACE_LEAF_DTYPE)."""
        n = C.c_uint64()
        rc = self._lib.nrg_vspace_dump(self._h, None, 0, C.byref(n))  # the count: nothing fits in 0
        if rc != L.NRG_E_CAPACITY:
            L.check(rc, "vspace_dump")
        out = np.zeros(max(n.value, 1), VSPACE_LEAF_DTYPE)
        m = C.c_uint64()
        L.check(self._lib.nrg_vspace_dump(self._h, _ptr(out), n.value, C.byref(m)), "vspace_dump")
        return out[: m.value]

    # -- skip list -----------------------------------------------------------------
    def sl_get(self, keys):
        """Get for a batch of keys: (vals, found); 0 where the key is absent."""
        keys = np.ascontiguousarray(np.asarray(keys, np.uint64))
        n = len(keys)
        vals = np.zeros(max(n, 1), np.uint64)
        found = np.zeros(max(n, 1), np.uint8)
        L.check(self._lib.nrg_skiplist_get(self._h, _ptr(keys), n, _ptr(vals), _ptr(found)), "skiplist_get")
        return vals[:n], found[:n]

    @_stream_ordered
    def sl_get_device(self, d_keys, n: int, d_vals, d_found):
        """Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        L.check(self._lib.nrg_skiplist_get_async(self._h, _dptr(d_keys), n, _dptr(d_vals), _dptr(d_found)),
                "skiplist_get")

    def sl_seek(self, keys, mode: int):
        """SkipMap::lower_bound / upper_bound for a batch (mode: L.NRG_SEEK_GE / GT / LE / LT):
        (out_keys, out_vals, found)."""
        keys = np.ascontiguousarray(np.asarray(keys, np.uint64))
        n = len(keys)
        ok = np.zeros(max(n, 1), np.uint64)
        ov = np.zeros(max(n, 1), np.uint64)
        found = np.zeros(max(n, 1), np.uint8)
        L.check(self._lib.nrg_skiplist_seek(self._h, _ptr(keys), n, mode, _ptr(ok), _ptr(ov), _ptr(found)),
                "skiplist_seek")
        return ok[:n], ov[:n], found[:n]

    def sl_scan(self, keys, mode: int, limit: int):
        """SkipMap::range from a bound, the first `limit` entries, for a batch (mode: L.NRG_SEEK_GE / GT
        ascending, LE / LT descending): (keys[n, limit], vals[n, limit], counts[n]); row i holds its
        entries in columns 0 .. counts[i] - 1 and zeros behind them."""
        keys = np.ascontiguousarray(np.asarray(keys, np.uint64))
        n = len(keys)
        rows = max(n, 1) * max(int(limit), 1)
        ok = np.zeros(rows, np.uint64)
        ov = np.zeros(rows, np.uint64)
        cnt = np.zeros(max(n, 1), np.uint32)
        L.check(self._lib.nrg_skiplist_scan(self._h, _ptr(keys), n, mode, limit, _ptr(ok), _ptr(ov), _ptr(cnt)),
                "skiplist_scan")
        return ok[: n * limit].reshape(n, limit), ov[: n * limit].reshape(n, limit), cnt[:n]

    @_stream_ordered
    def sl_scan_device(self, d_keys, n: int, mode: int, limit: int, d_out_keys, d_out_vals, d_counts):
        """nrg_skiplist_scan_async: d_out_keys / d_out_vals hold n * limit u64, d_counts n u32 (int32
        tensors); slots at or past a query's count are not written. Stream-ordered as sl_get_device."""
        L.check(self._lib.nrg_skiplist_scan_async(self._h, _dptr(d_keys), n, mode, limit, _dptr(d_out_keys),
                                                  _dptr(d_out_vals), _dptr(d_counts)), "skiplist_scan")

    def sl_range_count(self, los, his) -> np.ndarray:
        """The number of keys in each [lo, hi], both bounds inclusive."""
        los = np.ascontiguousarray(np.asarray(los, np.uint64))
        his = np.ascontiguousarray(np.asarray(his, np.uint64))
        if los.shape != his.shape:
            raise ValueError("los and his differ in length")
        n = len(los)
        out = np.zeros(max(n, 1), np.uint64)
        L.check(self._lib.nrg_skiplist_range_count(self._h, _ptr(los), _ptr(his), n, _ptr(out)), "skiplist_range_count")
        return out[:n]

    def _sl_pairs(self, call, what: str):
        n = C.c_uint64()
        rc = call(None, None, 0, C.byref(n))  # the count: nothing fits in 0
        if rc != L.NRG_E_CAPACITY:
            L.check(rc, what)
        k = np.zeros(max(n.value, 1), np.uint64)
        v = np.zeros(max(n.value, 1), np.uint64)
        m = C.c_uint64()
        L.check(call(_ptr(k), _ptr(v), n.value, C.byref(m)), what)
        return k[: m.value], v[: m.value]

    def sl_range(self, lo: int, hi: int):
        """SkipMap::range(lo..=hi): (keys, vals) in ascending key order."""
        return self._sl_pairs(lambda k, v, cap, n: self._lib.nrg_skiplist_range(self._h, lo, hi, k, v, cap, n),
                              "skiplist_range")

    def sl_dump(self):
        """The whole map, (keys, vals) in ascending key order: Replica::verify's view."""
        return self._sl_pairs(lambda k, v, cap, n: self._lib.nrg_skiplist_dump(self._h, k, v, cap, n),
                              "skiplist_dump")

    def sl_len(self) -> int:
        n = C.c_uint64()
        L.check(self._lib.nrg_skiplist_len(self._h, C.byref(n)), "skiplist_len")
        return n.value

    def sl_prefill(self, keys, vals):
        """Insert the pairs directly (any order, no log traffic); of equal keys the last wins."""
        keys = np.ascontiguousarray(np.asarray(keys, np.uint64))
        vals = np.ascontiguousarray(np.asarray(vals, np.uint64))
        if keys.shape != vals.shape:
            raise ValueError("keys and vals differ in length")
        L.check(self._lib.nrg_skiplist_prefill(self._h, _ptr(keys), _ptr(vals), len(keys)), "skiplist_prefill")

    def sl_prefill_range(self, n: int, off: int = 0):
        """SkipListWrapper::default: keys 0..n-1 -> k + off."""
        L.check(self._lib.nrg_skiplist_prefill_range(self._h, n, off), "skiplist_prefill_range")

    def sl_prefill_partition(self, n: int, off: int, part: int, parts: int):
        """SkipListWrapper::default restricted to partition `part` of `parts`: the keys k < n that
        nrg_key_owner gives to it, values k + off (a member of a partitioned skip-list group)."""
        L.check(self._lib.nrg_skiplist_prefill_partition(self._h, n, off, part, parts), "skiplist_prefill_partition")

    def sl_reserve(self, n_keys: int):
        """Room for `n_keys` keys in all; never shrinks (nrg_skiplist_reserve)."""
        self._reserve(self._lib.nrg_skiplist_reserve, L.NRG_DS_SKIPLIST, "sl_reserve", n_keys)

    def sl_capacity(self) -> int:
        """The keys the map has room for (nrg_skiplist_capacity)."""
        return self._capacity(self._lib.nrg_skiplist_capacity, L.NRG_DS_SKIPLIST, "sl_capacity")

    def sl_enable_removal(self, tombstone: int = 2**64 - 1):
        """From here on a record whose val == tombstone is Remove(key) (nrg_skiplist_enable_removal).
        Idempotent for one tombstone; there is no way back. Every replica of a log enables it at the
        same log index."""
        L.check(self._lib.nrg_skiplist_enable_removal(self._h, tombstone), "skiplist_enable_removal")

    def sl_removal(self):
        """The tombstone, or None while removal is off (nrg_skiplist_removal)."""
        t, on = C.c_uint64(), C.c_int()
        L.check(self._lib.nrg_skiplist_removal(self._h, C.byref(t), C.byref(on)), "skiplist_removal")
        return t.value if on.value else None

    def sl_remove(self, keys, origin: int = 1):
        """SkipMap::remove for a batch, in order: Remove(key) records appended to the log and replayed.
        Returns (prev u64[n], found u8[n]): the value each key had at its log position, found = 0 (and
        prev = 0) where it was absent."""
        tomb = self.sl_removal()
        if tomb is None:
            raise L.NrgError(L.NRG_E_INVAL, "sl_remove: removal is not enabled (sl_enable_removal)")
        recs = np.zeros(len(keys), PUT_DTYPE)
        recs["key"], recs["val"] = np.asarray(keys, np.uint64), tomb
        if len(recs) == 0:
            return np.zeros(0, np.uint64), np.zeros(0, np.uint8)
        first = self.log_append(recs, origin)
        return self.log_exec(first, first + len(recs))

    def sl_enable_pops(self, front_mark: int = SL_FRONT_MARK, back_mark: int = SL_BACK_MARK):
        """From here on a record {n, front_mark} is PopFront x n and {n, back_mark} is PopBack x n
        (nrg_skiplist_enable_pops). Idempotent for one pair of marks; there is no way back. Every replica
        of a log enables it at the same log index."""
        L.check(self._lib.nrg_skiplist_enable_pops(self._h, front_mark, back_mark), "skiplist_enable_pops")

    def sl_pops(self):
        """(front_mark, back_mark), or None while pops are off (nrg_skiplist_pops)."""
        f, b, on = C.c_uint64(), C.c_uint64(), C.c_int()
        L.check(self._lib.nrg_skiplist_pops(self._h, C.byref(f), C.byref(b), C.byref(on)), "skiplist_pops")
        return (f.value, b.value) if on.value else None

    def _sl_pop(self, back: int, n: int, origin: int):
        if self.sl_pops() is None:
            raise L.NrgError(L.NRG_E_INVAL, "sl_pop: pops are not enabled (sl_enable_pops)")
        self.log_exec()  # the length the record will see
        room = min(n, self.sl_len())
        k, v = np.zeros(max(room, 1), np.uint64), np.zeros(max(room, 1), np.uint64)
        m = C.c_uint64()
        L.check(self._lib.nrg_skiplist_pop(self._h, back, n, origin, _ptr(k), _ptr(v), C.byref(m)), "skiplist_pop")
        return k[: m.value], v[: m.value]

    def sl_pop_front(self, n: int = 1, origin: int = 1):
        """SkipMap::pop_front n times as one log record: (keys, vals) of the entries popped, ascending;
        fewer than n where the map is shorter (nrg_skiplist_pop)."""
        return self._sl_pop(0, n, origin)

    def sl_pop_back(self, n: int = 1, origin: int = 1):
        """SkipMap::pop_back n times as one log record: (keys, vals) of the entries popped, descending."""
        return self._sl_pop(1, n, origin)

    @_stream_ordered
    def sl_round_pops_device(self, d_ops, n: int, origin: int, d_resp, d_some, d_pop_keys, d_pop_vals, pop_cap: int,
                             d_pop_n):
        """sl_round_device on a replica with pops enabled, which also packs the entries its pop records
        popped into d_pop_keys / d_pop_vals (the first pop_cap) and their number into d_pop_n
        (nrg_skiplist_round_pops_async)."""
        L.check(self._lib.nrg_skiplist_round_pops_async(self._h, _dptr(d_ops), n, origin, _dptr(d_resp), _dptr(d_some),
                                                        _dptr(d_pop_keys), _dptr(d_pop_vals), pop_cap, _dptr(d_pop_n)),
                "skiplist_round_pops")

    # -- file store ----------------------------------------------------------------
    def mf_geometry(self):
        """(F, B): the number of files and a file's bytes (nrg_memfs_geometry)."""
        f, b = C.c_uint64(), C.c_uint64()
        L.check(self._lib.nrg_memfs_geometry(self._h, C.byref(f), C.byref(b)), "memfs_geometry")
        return f.value, b.value

    def mf_reserve(self, file_bytes: int):
        """Room for `file_bytes` bytes in every file, rounded up to a power of two; never shrinks; a sized
        context only (nrg_memfs_reserve). mf_geometry() reports the new B."""
        self._reserve(self._lib.nrg_memfs_reserve, L.NRG_DS_MEMFS, "mf_reserve", file_bytes)

    def mf_max_capacity(self) -> int:
        """The growth bound in bytes per file, 0 for none (nrg_memfs_max_capacity; no device work)."""
        return self._capacity(self._lib.nrg_memfs_max_capacity, L.NRG_DS_MEMFS, "mf_max_capacity")

    def mf_admit_log2(self) -> int:
        """log2 of what a write's end is admitted against: the growth bound where one is set above B, else
        B. What a caller of memfs_pwrite_plan passes for this replica."""
        _, b = self.mf_geometry()
        return max(b, self.mf_max_capacity()).bit_length() - 1

    def mf_init(self, ino: int, data):
        """Set the first len(data) bytes of file `ino` directly, before any replay (nrg_memfs_init)."""
        b = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8))
        L.check(self._lib.nrg_memfs_init(self._h, ino, _ptr(b) if b.size else None, b.size), "memfs_init")

    def mf_enable_sizes(self):
        """From here on the files have sizes: SetAttr is an op, Writes grow, Reads and GetAttr see the
        size; every size starts as B (nrg_memfs_enable_sizes). Idempotent; there is no way back."""
        L.check(self._lib.nrg_memfs_enable_sizes(self._h), "memfs_enable_sizes")

    def mf_size(self, ino: int) -> int:
        """The size of file `ino` of a sized context, as replayed so far (nrg_memfs_size)."""
        n = C.c_uint64()
        L.check(self._lib.nrg_memfs_size(self._h, ino, C.byref(n)), "memfs_size")
        return n.value

    def mf_truncate(self, ino: int, size: int):
        """What a logged MfSetAttr does, directly and with no log traffic (nrg_memfs_truncate)."""
        L.check(self._lib.nrg_memfs_truncate(self._h, ino, size), "memfs_truncate")

    def mf_read(self, ino: int, offset: int, size: int) -> bytes:
        """pread of a synced replica (nrg_memfs_read): up to `size` bytes of file `ino` from `offset`."""
        out = np.zeros(max(size, 1), np.uint8)
        n = C.c_uint64()
        L.check(self._lib.nrg_memfs_read(self._h, ino, offset, size, _ptr(out), C.byref(n)), "memfs_read")
        return out[: n.value].tobytes()

    @_stream_ordered
    def mf_pread_device(self, d_reqs, n: int, d_data, cap: int, d_offs, d_some):
        """Replica::execute for n read-only reads {ino, offset, len} (24 B each) on device buffers
        (nrg_memfs_pread_async): the clipped lengths scanned into d_offs[0..n], the bytes packed into
        d_data below cap, d_some[i] = 0 for an unknown ino. The caller compares d_offs[n] with cap.
        Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        L.check(self._lib.nrg_memfs_pread_async(self._h, _dptr(d_reqs), n, _dptr(d_data), cap, _dptr(d_offs),
                                                _dptr(d_some)), "memfs_pread")

    def mf_pread(self, reqs, cap: Optional[int] = None):
        """A batch of read-only reads: (data, offs, some), torch tensors on this replica's GPU (uint8
        [cap], int64 [n + 1], uint8 [n]); request i's bytes are data[offs[i]:offs[i + 1]]. `reqs`: a
        numpy array of MEMFS_RD_DTYPE (or [n, 3] u64: ino, offset, len), or a torch tensor on the GPU
        holding those records. cap=None sizes data from the requests on the host (a device tensor is
        copied back for that), so that offs[n] == cap (from B: in a sized context offs[n] <= cap); with
        a cap of the caller's, bytes at or past cap are not written and offs[n] > cap says so."""
        import torch

        dev = torch.device("cuda", self.device)
        host = None
        if hasattr(reqs, "data_ptr"):
            d_reqs = reqs.contiguous()
            n = d_reqs.numel() * d_reqs.element_size() // L.MEMFS_RD_DTYPE.itemsize
        else:
            host = np.asarray(reqs)
            if host.dtype != L.MEMFS_RD_DTYPE:
                host = np.ascontiguousarray(host, np.uint64).reshape(-1, 3).view(L.MEMFS_RD_DTYPE)
            host = np.ascontiguousarray(host.reshape(-1))
            n = len(host)
            d_reqs = torch.from_numpy(host.view(np.uint8).copy()).to(dev)
        if cap is None:
            if host is None:
                host = d_reqs.cpu().numpy().reshape(-1).view(np.uint8).view(L.MEMFS_RD_DTYPE)
            files, b = self.mf_geometry()
            first = np.uint64(L.NRG_MEMFS_FIRST_INO)
            ok = (host["ino"] >= first) & (host["ino"] < first + np.uint64(files)) & (host["offset"] < np.uint64(b))
            left = np.uint64(b) - np.minimum(host["offset"], np.uint64(b))
            cap = int(np.where(ok, np.minimum(host["len"], left), np.uint64(0)).sum(dtype=np.uint64))
        data = torch.empty(cap, dtype=torch.uint8, device=dev)
        offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
        some = torch.empty(n, dtype=torch.uint8, device=dev)
        self.mf_pread_device(d_reqs if n else None, n, data if cap else None, cap, offs, some if n else None)
        return data, offs, some

    @_stream_ordered
    def mf_pwrite_device(self, reqs: np.ndarray, d_data, data_bytes: int, origin: int, d_written=None, d_some=None) -> int:
        """Replica::combine for n logged writes of any length (nrg_memfs_pwrite_async): `reqs`, a host
        array of MEMFS_WR_DTYPE, cut on the device into 128-byte Write records straight into the log
        ring and replayed; the bytes come from the device buffer d_data. The answers go to d_written
        (u64) / d_some (u8), both or neither. Returns the number of records logged.
        Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        t = C.c_uint64()
        L.check(self._lib.nrg_memfs_pwrite_async(self._h, _ptr(reqs) if len(reqs) else None, len(reqs), _dptr(d_data),
                                                 data_bytes, origin, _dptr(d_written), _dptr(d_some), C.byref(t)),
                "memfs_pwrite")
        return t.value

    @_stream_ordered
    def mf_pwrite_records_device(self, reqs: np.ndarray, d_data, data_bytes: int, d_recs, cap: int) -> int:
        """The cut alone (nrg_memfs_pwrite_records_async): the records mf_pwrite_device would log, into
        the device buffer d_recs of cap records; the log and the replica are not touched. Returns the
        number of records; NrgError(NRG_E_CAPACITY) when they exceed cap (nothing is written then).
        Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        t = C.c_uint64()
        L.check(self._lib.nrg_memfs_pwrite_records_async(self._h, _ptr(reqs) if len(reqs) else None, len(reqs),
                                                         _dptr(d_data), data_bytes, _dptr(d_recs), cap, C.byref(t)),
                "memfs_pwrite_records")
        return t.value

    def mf_pwrite(self, reqs, data, origin: int = 1):
        """Logged writes of any length: (written, some, n_records). `reqs`: a numpy array of
        MEMFS_WR_DTYPE (or [n, 4] u64: ino, offset, len, data_off); request i writes data[data_off,
        data_off + len) to file `ino` at `offset`, so requests may share bytes. written[i] = len and
        some[i] = 1, or some[i] = 0 and written[i] = L.NRG_MEMFS_ENOENT / EFBIG (a write that ends past
        the end of the file fails whole). n_records: the 128-byte Write records the call logged (every
        request logs at least one). `data`: bytes or a numpy u8 array (the synchronous
        nrg_memfs_pwrite; written and some are numpy arrays), or a torch u8 tensor on this replica's
        GPU (nrg_memfs_pwrite_async, nothing waited for; written and some are torch tensors, int64 and
        uint8)."""
        rq = memfs_wr(reqs)
        if hasattr(data, "data_ptr"):
            import torch

            dev = torch.device("cuda", self.device)
            d = data.contiguous()
            nb = d.numel() * d.element_size()
            written = torch.empty(len(rq), dtype=torch.int64, device=dev)
            some = torch.empty(len(rq), dtype=torch.uint8, device=dev)
            t = self.mf_pwrite_device(rq, d if nb else None, nb, origin, written if len(rq) else None,
                                      some if len(rq) else None)
            return written, some, t
        b = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, np.uint8)
        written = np.zeros(len(rq), np.uint64)
        some = np.zeros(len(rq), np.uint8)
        t = C.c_uint64()
        L.check(self._lib.nrg_memfs_pwrite(self._h, _ptr(rq) if len(rq) else None, len(rq), _ptr(b) if b.size else None,
                                           b.size, origin, _ptr(written) if len(rq) else None,
                                           _ptr(some) if len(rq) else None, C.byref(t)), "memfs_pwrite")
        return written, some, t.value

    def mf_pwrite_records(self, reqs, data, device: bool = False):
        """The records mf_pwrite(reqs, data) would log, as a numpy array of MEMFS_OP_DTYPE (the cut alone,
        made on the GPU: nrg_memfs_pwrite_records_async; the log and the replica are not touched). With
        device=True the records stay on the GPU: a torch u8 tensor of n_records * 152 bytes, what a
        segment of a group round (nrg_round.recs) takes. `data` as in mf_pwrite."""
        import torch

        rq = memfs_wr(reqs)
        dev = torch.device("cuda", self.device)
        if hasattr(data, "data_ptr"):
            d = data.contiguous()
        else:
            b = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, np.uint8)
            d = torch.from_numpy(b.copy()).to(dev)
        nb = d.numel() * d.element_size()
        files, _ = self.mf_geometry()
        first, _, _ = memfs_pwrite_plan(self.mf_admit_log2(), files, rq, nb)
        T = int(first[-1])
        recs = torch.empty(max(T, 1) * MEMFS_OP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        got = self.mf_pwrite_records_device(rq, d if nb else None, nb, recs, T)
        assert got == T
        recs = recs[: T * MEMFS_OP_DTYPE.itemsize]
        if device:
            return recs
        return recs.cpu().numpy().view(MEMFS_OP_DTYPE).copy()

    @_stream_ordered
    def mf_pread_logged_device(self, reqs: np.ndarray, origin: int, d_data, cap: int, d_counts=None, d_some=None):
        """Replica::combine for n logged reads of any length (nrg_memfs_pread_logged_async): `reqs`, a
        host array of MEMFS_RD_DTYPE, cut on the device into 128-byte Read records straight into the log
        ring, replayed, and the responses gathered into the slots of the device buffer d_data (cap
        bytes). d_counts (u64) / d_some (u8): both or neither. Returns (offs, n_records): the slots'
        offsets (numpy, n + 1) and the records logged. Only data[offs[i]:offs[i] + counts[i]] is written.
        Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        t = C.c_uint64()
        offs = np.zeros(len(reqs) + 1, np.uint64)
        L.check(self._lib.nrg_memfs_pread_logged_async(self._h, _ptr(reqs) if len(reqs) else None, len(reqs), origin,
                                                       _dptr(d_data), cap, _dptr(d_counts), _dptr(d_some), _ptr(offs),
                                                       C.byref(t)), "memfs_pread_logged")
        return offs, t.value

    @_stream_ordered
    def mf_pread_logged_records_device(self, reqs: np.ndarray, d_recs, cap: int) -> int:
        """The cut alone (nrg_memfs_pread_logged_records_async): the records mf_pread_logged_device would
        log, into the device buffer d_recs of cap records; the log and the replica are not touched.
        Returns the number of records; NrgError(NRG_E_CAPACITY) when they exceed cap (nothing is written).
        Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        t = C.c_uint64()
        L.check(self._lib.nrg_memfs_pread_logged_records_async(self._h, _ptr(reqs) if len(reqs) else None, len(reqs),
                                                               _dptr(d_recs), cap, C.byref(t)), "memfs_pread_logged_records")
        return t.value

    @_stream_ordered
    def mf_pread_logged_gather_device(self, reqs: np.ndarray, d_resp, d_resp_some, T: int, d_data, cap: int, d_counts=None,
                                      d_some=None):
        """The way back alone (nrg_memfs_pread_logged_gather_async): the T responses a round wrote for the
        records of mf_pread_logged_records, into the slots of d_data and d_counts / d_some.
        Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        L.check(self._lib.nrg_memfs_pread_logged_gather_async(self._h, _ptr(reqs) if len(reqs) else None, len(reqs),
                                                              _dptr(d_resp), _dptr(d_resp_some), T, _dptr(d_data), cap,
                                                              _dptr(d_counts), _dptr(d_some)), "memfs_pread_logged_gather")

    def mf_pread_logged(self, reqs, origin: int = 1, cap: Optional[int] = None):
        """Logged reads of any length: (data, offs, counts, some), torch tensors on this replica's GPU
        (uint8 [cap], int64 [n + 1], int64 [n], uint8 [n]); request i's bytes are
        data[offs[i]:offs[i] + counts[i]], the file as every earlier record of the log left it. `reqs`: a
        numpy array of MEMFS_RD_DTYPE (or [n, 3] u64: ino, offset, len). cap=None sizes data from the plan
        (offs[n]); data starts as zeros, and bytes outside the answers are not written."""
        import torch

        rq = memfs_rd(reqs)
        n = len(rq)
        dev = torch.device("cuda", self.device)
        if cap is None:
            files, _ = self.mf_geometry()
            cap = int(memfs_pread_logged_plan(self.mf_admit_log2(), files, rq)[1][-1])
        data = torch.zeros(cap, dtype=torch.uint8, device=dev)
        counts = torch.zeros(n, dtype=torch.int64, device=dev)
        some = torch.zeros(n, dtype=torch.uint8, device=dev)
        offs, _ = self.mf_pread_logged_device(rq, origin, data if cap else None, cap, counts if n else None,
                                              some if n else None)
        return data, torch.from_numpy(offs.astype(np.int64)).to(dev), counts, some

    def mf_pread_logged_records(self, reqs, device: bool = False):
        """The records mf_pread_logged(reqs) would log, as a numpy array of MEMFS_OP_DTYPE (the cut alone,
        made on the GPU; the log and the replica are not touched). With device=True the records stay on
        the GPU: a torch u8 tensor of n_records * 152 bytes, what a segment of a group round takes."""
        import torch

        rq = memfs_rd(reqs)
        dev = torch.device("cuda", self.device)
        files, _ = self.mf_geometry()
        T = int(memfs_pread_logged_plan(self.mf_admit_log2(), files, rq)[0][-1])
        recs = torch.empty(max(T, 1) * MEMFS_OP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        got = self.mf_pread_logged_records_device(rq, recs, T)
        assert got == T
        recs = recs[: T * MEMFS_OP_DTYPE.itemsize]
        if device:
            return recs
        return recs.cpu().numpy().view(MEMFS_OP_DTYPE).copy()

    def mf_dump(self, ino: int) -> bytes:
        """The whole file `ino`, in a sized context up to its size: Replica::verify's view (nrg_memfs_dump)."""
        _, b = self.mf_geometry()
        out = np.zeros(b, np.uint8)
        n = C.c_uint64()
        L.check(self._lib.nrg_memfs_dump(self._h, ino, _ptr(out), b, C.byref(n)), "memfs_dump")
        return out[: n.value].tobytes()

    # -- synthetic -----------------------------------------------------------------
    def sy_read(self, ops: np.ndarray) -> np.ndarray:
        ops = np.ascontiguousarray(ops, SYNTH_RD_DTYPE)
        out = np.zeros(max(len(ops), 1), np.uint64)
        L.check(self._lib.nrg_synth_read(self._h, _ptr(ops), len(ops), _ptr(out)), "synth_read")
        return out[: len(ops)]

    def sy_dump(self) -> np.ndarray:
        n = self.cfg.synth_n
        out = np.zeros(n, np.uint64)
        m = C.c_uint64()
        L.check(self._lib.nrg_synth_dump(self._h, _ptr(out), n, C.byref(m)), "synth_dump")
        return out

    # -- generators / timing -------------------------------------------------------
    @_stream_ordered
    def gen_uniform_device(self, d_out, n, seed, span):
        """Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        L.check(self._lib.nrg_gen_uniform_async(self._h, _dptr(d_out), n, seed, span))

    @_stream_ordered
    def gen_raw_device(self, d_out, n, seed):
        """Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        L.check(self._lib.nrg_gen_raw_async(self._h, _dptr(d_out), n, seed))

    @_stream_ordered
    def gen_zipf_device(self, d_out, n, seed, N, theta=0.99, scramble=False):
        """Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        L.check(self._lib.nrg_gen_zipf_async(self._h, _dptr(d_out), n, seed, N, float(theta), int(scramble)), "zipf")

    @_stream_ordered
    def gen_stack_ops_device(self, d_out, n, seed):
        """Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        L.check(self._lib.nrg_gen_stack_ops_async(self._h, _dptr(d_out), n, seed), "stack ops")

    @_stream_ordered
    def gen_puts_device(self, d_out, d_keys, d_vals, n):
        """Ordered after torch's current stream, and torch's stream after it (_stream_ordered)."""
        L.check(self._lib.nrg_gen_puts_async(self._h, _dptr(d_out), _dptr(d_keys), _dptr(d_vals), n))

    def kernel_timing(self, enable: bool = True, only: Optional[str] = None, every: int = 1):
        """HIP-event timing of kernel `only` (all if None), on every `every`-th launch."""
        L.check(self._lib.nrg_kernel_timing_only(self._h, (only or "").encode()))
        L.check(self._lib.nrg_kernel_timing(self._h, max(1, int(every)) if enable else 0))

    def kernel_time(self, name: str):
        n = C.c_uint64()
        ms = C.c_double()
        L.check(self._lib.nrg_kernel_time(self._h, name.encode(), C.byref(n), C.byref(ms)))
        return n.value, ms.value


# =====================================================================================
# Dispatch plug-ins (the reference's data structures) and their operations
# =====================================================================================
@dataclass(frozen=True)
class Put:  # benches/hashmap.rs:52-56
    key: int
    val: int


@dataclass(frozen=True)
class Remove:  # HashMap::remove(key): a record {key, tombstone}, the tombstone the replicas enabled removal with
    key: int
    tombstone: int = 2**64 - 1  # checked against the replica's (NrHashMap.check_ops): a mismatch is an error

    @property
    def val(self) -> int:
        return self.tombstone


@dataclass(frozen=True)
class Get:  # benches/hashmap.rs:59-63
    key: int


@dataclass(frozen=True)
class Push:  # benches/stack.rs:22-28
    val: int


@dataclass(frozen=True)
class Pop:
    pass


@dataclass(frozen=True)
class Peek:  # nr/tests/stack.rs:26-29
    pass


@dataclass(frozen=True)
class Len:  # benches/lockfree.rs:49-52 (QueueRd::Len)
    pass


@dataclass(frozen=True)
class Map:  # benches/vspace.rs:485 OpcodeWr::Map(vbase, len, rights, pbase); rights 1..8 in MapAction order
    vbase: int
    len: int
    rights: int
    pbase: int


@dataclass(frozen=True)
class MapDevice:  # benches/vspace.rs:486 OpcodeWr::MapDevice(vbase, pbase, len)
    vbase: int
    pbase: int
    len: int


@dataclass(frozen=True)
class Identify:  # benches/vspace.rs:491 OpcodeRd::Identify(vaddr)
    vaddr: int


@dataclass(frozen=True)
class SlPush:  # benches/lockfree.rs:86-97 OpWr::Push(key, val) on the skip list
    key: int
    val: int


@dataclass(frozen=True)
class SlRemove:  # SkipMap::remove(key): a record {key, tombstone}; the replicas called sl_enable_removal(tombstone)
    key: int
    tombstone: int = 2**64 - 1

    @property
    def val(self) -> int:
        return self.tombstone


@dataclass(frozen=True)
class SlPopFront:  # SkipMap::pop_front n times: a record {n, front_mark}; the replicas called sl_enable_pops
    n: int = 1
    mark: int = SL_FRONT_MARK  # checked against the replica's (SkipList.check_ops): a mismatch is an error

    @property
    def key(self) -> int:
        return self.n

    @property
    def val(self) -> int:
        return self.mark


@dataclass(frozen=True)
class SlPopBack:  # SkipMap::pop_back n times: a record {n, back_mark}
    n: int = 1
    mark: int = SL_BACK_MARK

    @property
    def key(self) -> int:
        return self.n

    @property
    def val(self) -> int:
        return self.mark


@dataclass(frozen=True)
class Seek:  # SkipMap::lower_bound / upper_bound; mode: L.NRG_SEEK_GE / GT / LE / LT
    key: int
    mode: int


@dataclass(frozen=True)
class Scan:  # SkipMap::range from a bound, .take(limit); mode: GE / GT ascending, LE / LT descending
    key: int
    mode: int
    limit: int


@dataclass(frozen=True)
class MfWrite:  # benches/memfs.rs:66-72 OperationWr::Write{ino, offset, data}; at most 128 bytes
    ino: int
    offset: int
    data: bytes


@dataclass(frozen=True)
class MfRead:  # benches/memfs.rs:73-78 OperationWr::Read{ino, offset, size}: a write operation, logged
    ino: int
    offset: int
    size: int


@dataclass(frozen=True)
class MfGetAttr:  # benches/memfs.rs:27-29 OperationWr::GetAttr{ino}
    ino: int


@dataclass(frozen=True)
class MfSetAttr:  # benches/memfs.rs:30-33 OperationWr::SetAttr{ino, new_attrs}: the size; a sized context only
    ino: int
    size: int


@dataclass(frozen=True)
class MfPwrite:  # benches/nrfs.rs:103-115 OpWr::FileWrite: a logged write of any length (pwrite)
    ino: int
    offset: int
    data: bytes


@dataclass(frozen=True)
class MfPreadLogged:  # benches/memfs.rs:73-78, :267-282 OperationWr::Read with a size of any length: logged
    ino: int
    offset: int
    size: int


@dataclass(frozen=True)
class MfPread:  # benches/nrfs.rs:16-18, :88-101 OpRd::FileRead: a read operation, not logged; any size
    ino: int
    offset: int
    size: int


@dataclass(frozen=True)
class WriteOnly:  # benches/synthetic.rs:33-39
    tid: int
    r1: int
    r2: int


@dataclass(frozen=True)
class ReadWrite:
    tid: int
    r1: int
    r2: int


@dataclass(frozen=True)
class ReadOnly:  # benches/synthetic.rs:28-31
    tid: int
    r1: int
    r2: int


class NrHashMap:
    """NrHashMap: HashMap<u64,u64>; Put -> previous value (nr/examples/hashmap.rs:46-50). Remove -> the
    previous value or None, once every replica of the log has called its DeviceReplica.hm_enable_removal()
    with Remove's tombstone."""

    kind = L.NRG_DS_HASHMAP
    rec_dtype = PUT_DTYPE

    @staticmethod
    def clone_prepare(dev: DeviceReplica, peer: DeviceReplica):
        """Before `dev` is restored from `peer`'s image: an image does not carry the removal setting."""
        tomb = peer.hm_removal()
        if tomb is not None:
            dev.hm_enable_removal(tomb)

    @staticmethod
    def check_ops(dev: DeviceReplica, ops):
        """Before a batch is enqueued: what a record means depends on the replica's tombstone alone, so a
        Remove built for another tombstone (or for a replica without removal) would silently be a Put of
        that value, and a Put of the replica's tombstone silently a Remove. Both are refused here."""
        tomb = dev.hm_removal()  # (touches no device)
        for o in ops:
            if isinstance(o, Remove):
                if tomb is None:
                    raise L.NrgError(L.NRG_E_INVAL, "Remove: removal is not enabled on this replica (hm_enable_removal)")
                if o.tombstone != tomb:
                    raise ValueError(f"Remove(tombstone={o.tombstone:#x}) on a replica whose tombstone is {tomb:#x}")
            elif tomb is not None and o.val == tomb:
                raise ValueError(f"Put of the value {tomb:#x}, which is this replica's tombstone (it would be a Remove)")

    @staticmethod
    def encode(ops: Sequence[Put]) -> np.ndarray:
        r = np.zeros(len(ops), PUT_DTYPE)
        r["key"] = [o.key for o in ops]
        r["val"] = [o.val for o in ops]
        return r

    @staticmethod
    def decode(resp, some) -> list:
        return [int(v) if s else None for v, s in zip(resp, some)]

    @staticmethod
    def read_batch(dev: DeviceReplica, ops: Sequence[Get]) -> list:
        v, f = dev.hm_get(np.array([o.key for o in ops], np.uint64))
        return [int(a) if b else None for a, b in zip(v, f)]

    @staticmethod
    def snapshot(dev: DeviceReplica):
        k, v = dev.hm_dump()
        return dict(zip(k.tolist(), v.tolist()))


class Stack:
    """Stack: Vec<u32>; Push -> None (or Some(v) with push_resp=1), Pop -> Option<u32>."""

    kind = L.NRG_DS_STACK
    rec_dtype = STACK_OP_DTYPE

    @staticmethod
    def encode(ops) -> np.ndarray:
        r = np.zeros(len(ops), STACK_OP_DTYPE)
        r["val"] = [o.val if isinstance(o, Push) else 0 for o in ops]
        r["op"] = [L.NRG_STACK_PUSH if isinstance(o, Push) else L.NRG_STACK_POP for o in ops]
        return r

    @staticmethod
    def decode(resp, some) -> list:
        return [int(v) if s else None for v, s in zip(resp, some)]

    @staticmethod
    def read_batch(dev: DeviceReplica, ops) -> list:
        top = dev.st_peek()
        return [top for _ in ops]

    @staticmethod
    def snapshot(dev: DeviceReplica):
        return dev.st_dump().tolist()


class Queue:
    """SegQueueWrapper (benches/lockfree_comparisons.rs:75-101): a FIFO of u64; Push -> Some(v),
    Pop -> Option<u64>, Len -> the length."""

    kind = L.NRG_DS_QUEUE
    rec_dtype = QUEUE_OP_DTYPE

    @staticmethod
    def encode(ops) -> np.ndarray:
        r = np.zeros(len(ops), QUEUE_OP_DTYPE)
        r["val"] = [o.val if isinstance(o, Push) else 0 for o in ops]
        r["op"] = [L.NRG_QUEUE_PUSH if isinstance(o, Push) else L.NRG_QUEUE_POP for o in ops]
        return r

    @staticmethod
    def decode(resp, some) -> list:
        return [int(v) if s else None for v, s in zip(resp, some)]

    @staticmethod
    def read_batch(dev: DeviceReplica, ops) -> list:
        n = dev.qu_len()
        return [n for _ in ops]

    @staticmethod
    def snapshot(dev: DeviceReplica):
        return dev.qu_dump().tolist()


class VSpace:
    """VSpaceDispatcher (benches/vspace.rs:494-526): an x86-64 four-level page table. Map ->
    ("ok", pbase, len), MapDevice -> ("ok", 0, 0), either -> ("err", at) where the range meets an
    existing mapping; Identify -> the physical address, 0 where nothing is mapped."""

    kind = L.NRG_DS_VSPACE
    rec_dtype = VSPACE_OP_DTYPE

    @staticmethod
    def encode(ops) -> np.ndarray:
        r = np.zeros(len(ops), VSPACE_OP_DTYPE)
        r["vbase"] = [o.vbase for o in ops]
        r["pbase"] = [o.pbase for o in ops]
        r["len"] = [o.len for o in ops]
        r["op"] = [L.NRG_VSPACE_MAP if isinstance(o, Map) else L.NRG_VSPACE_MAP_DEVICE for o in ops]
        r["rights"] = [o.rights if isinstance(o, Map) else 0 for o in ops]
        return r

    @staticmethod
    def decode(resp, some) -> list:
        return [("ok", int(r["a"]), int(r["b"])) if s else ("err", int(r["a"])) for r, s in zip(resp, some)]

    @staticmethod
    def read_batch(dev: DeviceReplica, ops) -> list:
        pa, _ = dev.vs_resolve(np.array([o.vaddr for o in ops], np.uint64))
        return [int(a) for a in pa]

    @staticmethod
    def snapshot(dev: DeviceReplica):
        d = dev.vs_dump()
        return list(zip(d["vaddr"].tolist(), d["entry"].tolist()))


class SkipList:
    """SkipListWrapper (benches/lockfree_partitioned.rs:86-118): an ordered map u64 -> u64. SlPush ->
    the key (Ok(Some(key))); Get -> the value or None; Seek -> (key, value) or None; Scan -> a list of
    (key, value) in the scan's order. SlRemove -> the previous value or None, once every replica of the
    log has called its DeviceReplica.sl_enable_removal(); before, its record is a Push of the tombstone.
    SlPopFront(n) / SlPopBack(n) -> the number of entries popped, or None where the map was empty, once
    every replica of the log has called its DeviceReplica.sl_enable_pops() (the entries themselves:
    DeviceReplica.sl_pop_front / sl_pop_back)."""

    kind = L.NRG_DS_SKIPLIST
    rec_dtype = PUT_DTYPE

    @staticmethod
    def clone_prepare(dev: DeviceReplica, peer: DeviceReplica):
        """Before `dev` is restored from `peer`'s image: an image carries neither the removal nor the
        pops setting."""
        tomb = peer.sl_removal()
        if tomb is not None:
            dev.sl_enable_removal(tomb)
        marks = peer.sl_pops()
        if marks is not None:
            dev.sl_enable_pops(*marks)

    @staticmethod
    def check_ops(dev: DeviceReplica, ops):
        """Before a batch is enqueued: what a record means depends on the replica's marks alone, so a pop
        built for other marks (or for a replica without pops) would silently be a Push, and a Push of a
        mark silently a pop. Both are refused here."""
        marks = dev.sl_pops()  # (touches no device)
        for o in ops:
            if isinstance(o, (SlPopFront, SlPopBack)):
                if marks is None:
                    raise L.NrgError(L.NRG_E_INVAL, "pop: pops are not enabled on this replica (sl_enable_pops)")
                mine = marks[1] if isinstance(o, SlPopBack) else marks[0]
                if o.mark != mine:
                    raise ValueError(f"{type(o).__name__}(mark={o.mark:#x}) on a replica whose mark is {mine:#x}")
            elif marks is not None and isinstance(o, SlPush) and o.val in marks:
                raise ValueError(f"Push of the value {o.val:#x}, which is a pop mark of this replica (it would be a pop)")

    @staticmethod
    def encode(ops) -> np.ndarray:
        r = np.zeros(len(ops), PUT_DTYPE)
        r["key"] = [o.key for o in ops]
        r["val"] = [o.val for o in ops]
        return r

    @staticmethod
    def decode(resp, some) -> list:
        return [int(v) if s else None for v, s in zip(resp, some)]

    @staticmethod
    def read_batch(dev: DeviceReplica, ops) -> list:
        out = [None] * len(ops)
        gets = [i for i, o in enumerate(ops) if isinstance(o, Get)]
        if gets:
            v, f = dev.sl_get(np.array([ops[i].key for i in gets], np.uint64))
            for i, a, b in zip(gets, v, f):
                out[i] = int(a) if b else None
        for mode in sorted({o.mode for o in ops if isinstance(o, Seek)}):
            idx = [i for i, o in enumerate(ops) if isinstance(o, Seek) and o.mode == mode]
            k, v, f = dev.sl_seek(np.array([ops[i].key for i in idx], np.uint64), mode)
            for i, a, b, c in zip(idx, k, v, f):
                out[i] = (int(a), int(b)) if c else None
        for mode, limit in sorted({(o.mode, o.limit) for o in ops if isinstance(o, Scan)}):
            idx = [i for i, o in enumerate(ops) if isinstance(o, Scan) and (o.mode, o.limit) == (mode, limit)]
            k, v, c = dev.sl_scan(np.array([ops[i].key for i in idx], np.uint64), mode, limit)
            for i, kr, vr, m in zip(idx, k, v, c):
                out[i] = list(zip(kr[:m].tolist(), vr[:m].tolist()))
        return out

    @staticmethod
    def snapshot(dev: DeviceReplica):
        k, v = dev.sl_dump()
        return list(zip(k.tolist(), v.tolist()))


class MemFs:
    """NrMemFilesystem (benches/memfs.rs:106-292): files of fixed size (or, with sizes enabled and
    DeviceReplica.set_max_capacity, files that grow up to a bound), every op a log record
    (ReadOperation = (), :194-201). MfWrite -> ("written", len); MfRead -> ("data", bytes), the file
    as every earlier record of the log left it; MfGetAttr -> ("attr", size); MfSetAttr -> ("attr", the
    new size) once the replica's DeviceReplica.mf_enable_sizes() was called, ("err", EINVAL) before;
    any of them -> ("err", code) with code L.NRG_MEMFS_ENOENT / EFBIG / EINVAL. An MfWrite of more
    than 128 bytes is encoded with its length and no data: the replay answers EINVAL.

    MfPwrite (benches/nrfs.rs:103-115 OpWr::FileWrite) is a write of any length -> ("written", len), or
    ("err", ENOENT / EFBIG); one that ends past the end of the file fails whole. It is logged as a
    contiguous run of 128-byte Write records, the cut of nrg_memfs_pwrite* (include/nrgpu.h), which
    needs the replica's geometry: Replica._combine encodes with encode_for(dev, ops) and hands
    decode_ops the per-op record counts. One MfPwrite may expand into more records than
    MAX_PENDING_OPS (the bound counts ops, and the combiner appends a batch in as many appends as the
    log takes); an MfPwrite that alone expands into more records than one append can carry
    (the log's entries less GC_FROM_HEAD) raises ValueError from execute_mut[_batch], before anything
    is enqueued.

    MfPreadLogged (memfs.rs:73-78, :267-282 OperationWr::Read, here with a size of any length) ->
    ("data", bytes), clipped at the end of the file, or ("err", ENOENT): an execute_mut op like MfRead,
    logged as a contiguous run of 128-byte Read records, one per line it touches (the cut of
    nrg_memfs_pread_logged*), and folded from the run's responses. The rules of MfPwrite hold for it."""

    kind = L.NRG_DS_MEMFS
    rec_dtype = MEMFS_OP_DTYPE
    record_errors = True  # a refused record is its op's ("err", EINVAL), not the replica's error (Replica._exec)
    _TAGS = {MfWrite: "written", MfPwrite: "written", MfRead: "data", MfPreadLogged: "data", MfGetAttr: "attr", MfSetAttr: "attr"}

    @staticmethod
    def encode(ops) -> np.ndarray:
        r = np.zeros(len(ops), MEMFS_OP_DTYPE)
        for i, o in enumerate(ops):
            if isinstance(o, MfPwrite):
                raise TypeError("an MfPwrite is cut by the replica's geometry: MemFs.encode_counts(ops, log2_b, files)")
            if isinstance(o, MfPreadLogged):
                raise TypeError("an MfPreadLogged is cut by the replica's geometry: MemFs.encode_counts(ops, log2_b, files)")
            if not isinstance(o, (MfWrite, MfRead, MfGetAttr, MfSetAttr)):
                raise TypeError(f"not a file-store op: {o!r}")
            r["ino"][i] = o.ino
            if isinstance(o, MfWrite):
                r["offset"][i], r["op"][i], r["len"][i] = o.offset, L.NRG_MEMFS_WRITE, len(o.data)
                if len(o.data) <= L.NRG_MEMFS_MAX_DATA:
                    r["data"][i, : len(o.data)] = np.frombuffer(bytes(o.data), np.uint8)
            elif isinstance(o, MfRead):
                r["offset"][i], r["op"][i], r["len"][i] = o.offset, L.NRG_MEMFS_READ, o.size
            elif isinstance(o, MfSetAttr):
                r["offset"][i], r["op"][i] = o.size, L.NRG_MEMFS_SETATTR
            else:
                r["op"][i] = L.NRG_MEMFS_GETATTR
        return r

    @staticmethod
    def _pwrite_reqs(ops):
        """The MfPwrite ops of `ops` as requests of nrg_memfs_pwrite* over their concatenated bytes."""
        pw = [o for o in ops if isinstance(o, MfPwrite)]
        rq = np.zeros(len(pw), L.MEMFS_WR_DTYPE)
        rq["ino"] = [o.ino for o in pw]
        rq["offset"] = [o.offset for o in pw]
        rq["len"] = [len(o.data) for o in pw]
        rq["data_off"][1:] = np.cumsum(rq["len"][:-1], dtype=np.uint64)
        return pw, rq

    @staticmethod
    def _pread_reqs(ops):
        """The MfPreadLogged ops of `ops` as requests of nrg_memfs_pread_logged*."""
        pr = [o for o in ops if isinstance(o, MfPreadLogged)]
        rq = np.zeros(len(pr), L.MEMFS_RD_DTYPE)
        rq["ino"] = [o.ino for o in pr]
        rq["offset"] = [o.offset for o in pr]
        rq["len"] = [o.size for o in pr]
        return pr, rq

    @staticmethod
    def record_counts(ops, log2_b: int, files: int) -> list:
        """The log records each op becomes in a store of `files` files of 2^log2_b bytes: 1, or an
        MfPwrite's or MfPreadLogged's fragments (nrg_memfs_pwrite_plan, nrg_memfs_pread_logged_plan; no
        device is touched)."""
        pw, rq = MemFs._pwrite_reqs(ops)
        first, _, _ = memfs_pwrite_plan(log2_b, files, rq, int(rq["len"].sum(dtype=np.uint64)))
        f = iter(np.diff(first).astype(np.int64).tolist())
        _, rd = MemFs._pread_reqs(ops)
        g = iter(np.diff(memfs_pread_logged_plan(log2_b, files, rd)[0]).astype(np.int64).tolist())
        return [next(f) if isinstance(o, MfPwrite) else next(g) if isinstance(o, MfPreadLogged) else 1 for o in ops]

    @staticmethod
    def encode_counts(ops, log2_b: int, files: int):
        """(records, per-op record counts) of `ops` for a store of `files` files of 2^log2_b bytes: an
        MfPwrite becomes the fragment records of nrg_memfs_pwrite* (the counts and answers from
        nrg_memfs_pwrite_plan, the records built here with numpy; no device is touched), every other
        op the one record of encode()."""
        counts = MemFs.record_counts(ops, log2_b, files)
        pw, rq = MemFs._pwrite_reqs(ops)
        _, written, some = memfs_pwrite_plan(log2_b, files, rq, int(rq["len"].sum(dtype=np.uint64)))
        recs = np.zeros(sum(counts), MEMFS_OP_DTYPE)
        B, pos, q = 1 << log2_b, 0, 0
        _, rd = MemFs._pread_reqs(ops)
        _, roffs, _ = memfs_pread_logged_plan(log2_b, files, rd)
        planned, p = np.diff(roffs).astype(np.int64), 0
        for o, c in zip(ops, counts):
            if isinstance(o, MfPreadLogged):  # one Read per line of what it plans to read; no data bytes
                r = recs[pos:pos + c]
                r["ino"], r["op"], r["offset"] = o.ino, L.NRG_MEMFS_READ, o.offset
                if planned[p]:
                    line = (o.offset >> 7) + np.arange(c, dtype=np.int64)
                    lo = np.maximum(line << 7, o.offset)
                    hi = np.minimum((line + 1) << 7, o.offset + int(planned[p]))
                    r["offset"], r["len"] = lo, hi - lo
                pos += c
                p += 1
                continue
            if not isinstance(o, MfPwrite):
                recs[pos] = MemFs.encode([o])[0]
                pos += 1
                continue
            r = recs[pos:pos + c]
            r["ino"], r["op"] = o.ino, L.NRG_MEMFS_WRITE
            if not some[q]:  # one record that the replay answers with the same error
                if int(written[q]) == L.NRG_MEMFS_EFBIG:
                    r["offset"], r["len"] = B, 1
                else:
                    r["offset"] = o.offset
            elif len(o.data) == 0:
                r["offset"] = o.offset
            else:  # cut at the file's 128-byte lines
                line = (o.offset >> 7) + np.arange(c, dtype=np.int64)
                lo = np.maximum(line << 7, o.offset)
                hi = np.minimum((line + 1) << 7, o.offset + len(o.data))
                r["offset"], r["len"] = lo, hi - lo
                d = np.frombuffer(bytes(o.data), np.uint8)
                for k in range(c):
                    r["data"][k, : hi[k] - lo[k]] = d[lo[k] - o.offset:hi[k] - o.offset]
            pos += c
            q += 1
        return recs, counts

    @staticmethod
    def encode_for(dev: DeviceReplica, ops):
        """encode_counts with the geometry of the replica `dev` (read from its context; no device work):
        admission is decided against its growth bound where one is set (DeviceReplica.mf_admit_log2), and
        the replay of the records grows the store."""
        files, _ = dev.mf_geometry()
        return MemFs.encode_counts(ops, dev.mf_admit_log2(), files)

    @staticmethod
    def records_for(dev: DeviceReplica, ops) -> list:
        """record_counts with the geometry of the replica `dev`."""
        files, _ = dev.mf_geometry()
        return MemFs.record_counts(ops, dev.mf_admit_log2(), files)

    @staticmethod
    def decode_ops(ops, resp, some, counts=None) -> list:
        """The responses of `ops` (a response does not say which op it answers; Replica._combine
        passes the batch). counts: the records each op became (encode_counts; None: one each); an
        MfPwrite's fragments fold into one answer, ("written", the sum), or ("err", code) from its
        failing record; an MfPreadLogged's fold into ("data", each fragment's data[:n] concatenated)."""
        out, pos = [], 0
        for i, o in enumerate(ops):
            c = 1 if counts is None else counts[i]
            r, s = resp[pos:pos + c], some[pos:pos + c]
            pos += c
            bad = np.flatnonzero(np.asarray(s) == 0)
            if len(bad):
                out.append(("err", int(r["n"][bad[0]])))
            elif isinstance(o, MfRead):
                n = int(r["n"][0])
                out.append(("data", r["data"][0][:n].tobytes()))
            elif isinstance(o, MfPreadLogged):  # each fragment's data[:n], concatenated
                out.append(("data", b"".join(r["data"][k][:int(r["n"][k])].tobytes() for k in range(c))))
            else:
                out.append((MemFs._TAGS[type(o)], int(r["n"].sum(dtype=np.uint64))))
        return out

    @staticmethod
    def decode(resp, some) -> list:
        """Without the ops: (n, the 128 data bytes) where some, ("err", code) otherwise."""
        return [(int(r["n"]), r["data"].tobytes()) if s else ("err", int(r["n"])) for r, s in zip(resp, some)]

    @staticmethod
    def read_batch(dev: DeviceReplica, ops) -> list:
        """MfPread -> ("data", bytes), clipped at the end of the file, or ("err", ENOENT): one
        nrg_memfs_pread_async for the batch. memfs.rs itself has no read operations (ReadOperation =
        ()): its MfRead is an execute_mut op and is refused here."""
        for o in ops:
            if isinstance(o, (MfRead, MfPreadLogged)):
                raise TypeError("MfRead is an execute_mut op (memfs.rs: ReadOperation = ()); the read-only read is MfPread")
            if not isinstance(o, MfPread):
                raise TypeError(f"not a file-store read: {o!r}")
        if not ops:
            return []
        reqs = np.zeros(len(ops), L.MEMFS_RD_DTYPE)
        reqs["ino"] = [o.ino for o in ops]
        reqs["offset"] = [o.offset for o in ops]
        reqs["len"] = [o.size for o in ops]
        data, offs, some = dev.mf_pread(reqs)
        data, offs, some = data.cpu().numpy(), offs.cpu().numpy(), some.cpu().numpy()
        return [("data", data[offs[i]:offs[i + 1]].tobytes()) if some[i] else ("err", L.NRG_MEMFS_ENOENT)
                for i in range(len(ops))]

    @staticmethod
    def clone_prepare(dev: DeviceReplica, peer: DeviceReplica):
        """Before `dev` is restored from `peer`'s image (Replica(..., clone_from=peer)): a peer with a
        growth bound may have grown past the B `dev` was opened with, and nrg_restore takes a larger image
        only under a bound, so `dev` gets sizes and the peer's bound first."""
        bound = peer.mf_max_capacity()
        if bound:
            dev.mf_enable_sizes()
            dev.set_max_capacity(bound)

    @staticmethod
    def snapshot(dev: DeviceReplica):
        files, _ = dev.mf_geometry()
        return [dev.mf_dump(L.NRG_MEMFS_FIRST_INO + f) for f in range(files)]


class AbstractDataStructure:
    """benches/synthetic.rs AbstractDataStructure::new(n, 20, 5, 2, 1)."""

    kind = L.NRG_DS_SYNTHETIC
    rec_dtype = SYNTH_OP_DTYPE

    @staticmethod
    def encode(ops) -> np.ndarray:
        r = np.zeros(len(ops), SYNTH_OP_DTYPE)
        r["tid"] = [o.tid for o in ops]
        r["r1"] = [o.r1 for o in ops]
        r["r2"] = [o.r2 for o in ops]
        r["op"] = [L.NRG_SYNTH_READ_WRITE if isinstance(o, ReadWrite) else L.NRG_SYNTH_WRITE_ONLY for o in ops]
        return r

    @staticmethod
    def decode(resp, some) -> list:
        return [int(v) for v in resp]

    @staticmethod
    def read_batch(dev: DeviceReplica, ops) -> list:
        a = np.zeros(len(ops), SYNTH_RD_DTYPE)
        a["tid"] = [o.tid for o in ops]
        a["r1"] = [o.r1 for o in ops]
        a["r2"] = [o.r2 for o in ops]
        return [int(x) for x in dev.sy_read(a)]

    @staticmethod
    def snapshot(dev: DeviceReplica):
        return dev.sy_dump()


# =====================================================================================
# Log / Replica / ReplicaToken — the reference's public API
# =====================================================================================
class ReplicaToken:
    """nr/src/replica.rs:26-48"""

    __slots__ = ("_id",)

    def __init__(self, ident: int):
        self._id = ident

    def id(self) -> int:
        return self._id

    def __eq__(self, o):
        return isinstance(o, ReplicaToken) and o._id == self._id

    def __repr__(self):
        return f"ReplicaToken({self._id})"


class Log:
    """nr::Log — the shared operation log (nr/src/log.rs:88-131).

    Physically, every registered GPU replica holds a copy of the log in its HBM ring; an
    append writes the same records at the same logical indices into every copy (in one
    process the copies are filled directly; across processes/GPUs the write segments are
    all-gathered, see parallel.py). `tail` is the shared logical tail, `ctail` the max tail any
    replica has replayed (nr/src/log.rs:522), used by reads to sync.

    The host keeps the appended batches of the live window [head, tail) (head = the slowest
    replica's ltail, advanced when the log nears full as Log::append's GC does,
    nr/src/log.rs:364-387, :536-580), so that a replica registered after appends can be given the
    entries it has not seen and catch up through exec from its ltail = 0 (nr/src/log.rs:272-292,
    :473-524; nr/src/replica.rs:469-479).
    """

    def __init__(self, nbytes: int = DEFAULT_LOG_BYTES):
        num = nbytes // 64
        if num < 2 * GC_FROM_HEAD:
            num = 2 * GC_FROM_HEAD
        size = 1
        while size < num:
            size <<= 1
        self.bytes = nbytes
        self.size = size
        self.head = 0
        self.tail = 0
        self.ctail = 0
        self._next = 1
        self._replicas: List["Replica"] = []
        self._live: list = []  # (first log index, records, origin) of the batches in [head, tail)
        self.lock = threading.RLock()

    def register(self, replica: "Replica", clone_from: Optional["Replica"] = None) -> Optional[int]:
        """Log::register (nr/src/log.rs:272-292): ids 1.., None at MAX_REPLICAS. A replica
        registered after appends starts at ltail 0 like the reference's; its copy of the log is
        filled with the live entries, which it replays on its next combine or sync. If GC has
        already moved head past entry 0 the reference's exec would panic ("Local tail not within
        the shared log", nr/src/log.rs:486-488): here registration fails with RuntimeError.

        With `clone_from`, a replica registered on this log, the new replica starts from that
        peer's state instead of from entry 0: the peer is synced to the log's tail and
        snapshotted, and the new replica restored from the image (nrg_restore), so its ltail is
        the tail and no live entry is copied. That works after GC too."""
        if clone_from is not None:
            # (the peer's combiner lock before the log's, the order Replica._combine takes them in)
            with clone_from._combiner, self.lock:
                if self._next >= MAX_REPLICAS:
                    return None
                if clone_from not in self._replicas:
                    raise ValueError("clone_from is not registered with this log")
                clone_from._exec()  # to the tail: every copy holds every appended entry
                prepare = getattr(replica.ds, "clone_prepare", None)
                if prepare is not None:  # (MemFs: the peer's growth bound, so that its grown image is taken)
                    prepare(replica.dev, clone_from.dev)
                if clone_from.dev.device == replica.dev.device:
                    p, nbytes, info = clone_from.dev.snapshot_device()
                    if info.log_idx == self.tail:
                        replica.dev.restore(p, nbytes)
                else:  # through the host: the new replica's GPU need not read the peer's memory
                    img = clone_from.dev.snapshot()
                    info = _snapshot.header(img)
                    if info.log_idx == self.tail:
                        replica.dev.restore(img)
                if info.log_idx != self.tail:
                    raise RuntimeError("log copies diverged")
                idx = self._next
                self._next += 1
                self._replicas.append(replica)
                return idx
        with self.lock:
            if self._next >= MAX_REPLICAS:
                return None
            if self.head > 0:
                raise RuntimeError(f"cannot register a replica: the log was garbage-collected up to {self.head}, "
                                   "so entries a new replica must replay from index 0 are gone")
            for first, recs, origin in self._live:  # catch-up copy, same logical indices
                got = replica.dev.log_append(recs, origin)
                if got != first:
                    raise RuntimeError("log copies diverged")
            idx = self._next
            self._next += 1
            self._replicas.append(replica)
            return idx

    def _ltails(self):
        return [r.dev.log_state()["ltail"] for r in self._replicas]

    def get_ctail(self) -> int:
        """Log::get_ctail (nr/src/log.rs:677-679): the largest tail any replica has replayed."""
        with self.lock:
            self.ctail = max([self.ctail] + self._ltails())
            return self.ctail

    def is_replica_synced_for_reads(self, replica: "Replica", ctail: Optional[int] = None) -> bool:
        """Log::is_replica_synced_for_reads (nr/src/log.rs:671-673): ltail >= ctail."""
        c = self.get_ctail() if ctail is None else ctail
        return replica.dev.log_state()["ltail"] >= c

    def advance_head(self) -> int:
        """Log::advance_head (nr/src/log.rs:536-580): head = min over replicas' ltails (each
        device replica's own ring is garbage-collected up to its ltail by libnrgpu.so)."""
        with self.lock:
            lt = self._ltails()
            if lt:
                self.head = max(self.head, min(lt))
            return self.head

    def append(self, recs: np.ndarray, idx: int) -> int:
        """Log::append: the same records at the same logical indices in every copy."""
        with self.lock:
            first = None
            for r in self._replicas:
                f = r.dev.log_append(recs, idx)
                if first is None:
                    first = f
                elif f != first:
                    raise RuntimeError("log copies diverged")
            self.tail = first + len(recs)
            self._live.append((first, np.array(recs, copy=True), idx))
            if self.tail - self.head > self.size - GC_FROM_HEAD:  # nearly full: GC (nr/src/log.rs:364-387)
                self.advance_head()
            while self._live and self._live[0][0] + len(self._live[0][1]) <= self.head:
                self._live.pop(0)
            return first


class Replica:
    """nr::Replica<D> (nr/src/replica.rs:72-595) over a GPU replica backend."""

    def __init__(self, log: Log, ds, device: int = 0, **cfg):
        """`clone_from=peer` (not a config field): start from that registered replica's state
        instead of replaying the log from entry 0 (Log.register); the only way in after GC."""
        clone_from = cfg.pop("clone_from", None)
        self.ds = ds
        self.log = log
        cfg.setdefault("log_bytes", log.bytes)
        self.dev = DeviceReplica(ds.kind, device, **cfg)
        idx = log.register(self, clone_from) if clone_from is not None else log.register(self)
        if idx is None:
            raise RuntimeError("too many replicas registered with the log")
        self.idx = idx
        self._next = 1
        self._combiner = threading.Lock()
        self._ctx: dict = {}
        self._resp: dict = {}
        self._reg = threading.Lock()
        # a thread's pending ops are appended and taken under this lock (the reference's
        # per-thread context rings, nr/src/context.rs:88-194, are lock-free SPSC queues)
        self._ctx_lock = threading.Lock()

    # register (nr/src/replica.rs:279-298): tokens 1..=MAX_THREADS_PER_REPLICA
    def register(self) -> Optional[ReplicaToken]:
        with self._reg:
            if self._next > MAX_THREADS_PER_REPLICA:
                return None
            t = self._next
            self._next += 1
            with self._ctx_lock:
                self._ctx[t] = []
                self._resp[t] = []
            return ReplicaToken(t)

    def _enqueue(self, ops, tid):
        with self._ctx_lock:
            q = self._ctx[tid]
            if len(q) + len(ops) > MAX_PENDING_OPS and len(ops) <= MAX_PENDING_OPS:
                return False
            q.extend(ops)
            return True

    def _exec(self, resp_lo: int = 0, resp_hi: int = 0):
        """DeviceReplica.log_exec for this replica's plug-in. A plug-in whose records can be refused
        one by one (MemFs: `record_errors`) gets the refusal as that op's answer, ("err", EINVAL), and
        every replica that replays the record latches NRG_E_INVAL once: here the latch is read, and
        that code dropped, so that the op's caller gets the answer and no other replica an error for
        an op that was not its own."""
        rc, resp, some = self.dev.log_exec_rc(resp_lo, resp_hi)
        if not (rc == L.NRG_E_INVAL and getattr(self.ds, "record_errors", False)):
            L.check(rc, "exec")
        return resp, some

    def _combine(self):
        """Replica::combine (nr/src/replica.rs:544-595): collect every thread's pending ops,
        append them as one batch, replay the log, route this replica's responses back."""
        with self.log.lock:
            order, batch = [], []
            with self._ctx_lock:
                for t in sorted(self._ctx):
                    q = self._ctx[t]
                    if q:
                        order.append((t, len(q)))
                        batch.extend(q)
                        self._ctx[t] = []
            if batch and getattr(self.ds, "encode_for", None):
                # a plug-in whose ops may become several records each, cut by the replica's geometry
                # (MemFs: MfPwrite): the batch goes into the log in as many appends as the log takes,
                # split between ops, and the per-op record counts go to decode_ops
                recs, counts = self.ds.encode_for(self.dev, batch)
                lim = self.log.size - GC_FROM_HEAD
                parts, i, pos = [], 0, 0
                while i < len(batch):
                    tot = counts[i]  # (execute_mut_batch refused an op of more than lim records)
                    i += 1
                    while i < len(batch) and tot + counts[i] <= lim:
                        tot += counts[i]
                        i += 1
                    first = self.log.append(recs[pos:pos + tot], self.idx)
                    parts.append(self._exec(first, first + tot))
                    pos += tot
                resp = np.concatenate([p[0] for p in parts])
                some = np.concatenate([p[1] for p in parts])
                out = self.ds.decode_ops(batch, resp, some, counts)
            elif batch:
                first = self.log.append(self.ds.encode(batch), self.idx)
                resp, some = self.dev.log_exec(first, first + len(batch))
                # a plug-in whose responses need their ops to be read decodes with the batch
                with_ops = getattr(self.ds, "decode_ops", None)
                out = with_ops(batch, resp, some) if with_ops else self.ds.decode(resp, some)
            if batch:
                s = 0
                for t, n in order:
                    self._resp[t].extend(out[s:s + n])
                    s += n
            else:
                self._exec()
            st = self.dev.log_state()
            self.log.ctail = max(self.log.ctail, st["ltail"])

    def _combine_until(self, done: Callable[[], bool]):
        """Flat combining's wait (nr/src/replica.rs:508-541): until done(), become the combiner
        and combine every thread's pending ops. The reference spins on a failed try-lock; a
        Python thread spinning on the GIL only lets the combiner run every switch interval
        (5 ms), so a thread blocks on the combiner lock instead and re-checks after it: a
        combine that ran meanwhile may have carried its ops."""
        while not done():
            with self._combiner:
                if not done():
                    self._combine()

    def execute_mut(self, op, tok: ReplicaToken):
        """Replica::execute_mut (nr/src/replica.rs:345-356)"""
        return self.execute_mut_batch([op], tok)[0]

    def execute_mut_batch(self, ops: Sequence, tok: ReplicaToken) -> list:
        """Host batcher: enqueue many of this thread's writes, combine once."""
        tid = tok.id()
        ops = list(ops)
        check_ops = getattr(self.ds, "check_ops", None)
        if check_ops is not None:  # (NrHashMap) an op that would not mean on this replica what it says
            check_ops(self.dev, ops)
        records_for = getattr(self.ds, "records_for", None)
        if records_for is not None:  # (MemFs) an op that no single append can carry is refused here
            lim = self.log.size - GC_FROM_HEAD
            for o, c in zip(ops, records_for(self.dev, ops)):
                if c > lim:
                    raise ValueError(f"{type(o).__name__} expands into {c} log records; one append to this log carries "
                                     f"at most {lim} (a larger Log, or several smaller writes)")
        self._combine_until(lambda: self._enqueue(ops, tid))
        want = len(ops)
        self._combine_until(lambda: len(self._resp[tid]) >= want)
        out = self._resp[tid][:want]
        del self._resp[tid][:want]
        return out

    def _sync_to(self, ctail: int):
        self._combine_until(lambda: self.dev.log_state()["ltail"] >= ctail)

    def execute(self, op, tok: ReplicaToken):
        """Replica::execute -> read_only (nr/src/replica.rs:404-410, :483-497)"""
        return self.execute_batch([op], tok)[0]

    def execute_batch(self, ops: Sequence, tok: ReplicaToken) -> list:
        """Sync to ctail, then dispatch with this replica's replay excluded (the reference's
        reader lock against the combiner, nr/src/replica.rs:483-497). The device answers reads
        only with its copy of the log fully replayed (nrg_hashmap_get: NRG_E_NOT_SYNCED
        otherwise), and other replicas' combiners may append to that copy after the sync: those
        entries -- none of them this replica's own, whose combine appends and replays in one go --
        are replayed first, under the log lock so that no further append lands before the read
        (a read then sees a state at least as new as the ctail it synced to, as NR's does)."""
        self._sync_to(self.log.ctail)
        with self._combiner:
            with self.log.lock:
                self._exec()
                return self.ds.read_batch(self.dev, list(ops))

    def sync(self, tok: Optional[ReplicaToken] = None):
        """Replica::sync (nr/src/replica.rs:473-479)"""
        self._sync_to(self.log.ctail)

    def verify(self, v: Callable):
        """Replica::verify (nr/src/replica.rs:443-467): catch up on the log, then run v on
        the replica's data structure (materialised on the host)."""
        with self._combiner:
            with self.log.lock:
                self._exec()
                self.dev.sync()
                v(self.ds.snapshot(self.dev))

    def digest(self):
        """Replica::verify's device-side form: catch up on the log as verify does, then the
        replica's digest triple (DeviceReplica.digest); nothing is materialised on the host."""
        with self._combiner:
            with self.log.lock:
                self._exec()
                return self.dev.digest()
