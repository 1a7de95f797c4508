"""Multi-GPU node replication: one replica per GPU, one process per GPU.

In NR every replica replays every write (nr/src/log.rs:473-524, one exec loop per replica
over the shared log); the reference shares the log through cache-coherent memory across
NUMA nodes. Here each GPU is a NUMA node: per round, every rank contributes the write segment
its clients produced, the segments are all-gathered, and every replica replays the identical
global log W_0 || W_1 || ... || W_{G-1} (concatenation by rank = the deterministic log order
of the round), then answers its own reads against the post-round state. Responses to writes go
only to the origin rank (nr/src/replica.rs:576-578). Reads never leave their GPU.

Two transports, one round semantics:
  ReplicaGroup      the C ABI's group (nrg_group_join / nrg_group_round_async): RCCL over xGMI,
                    called from libnrgpu.so on a library-owned stream per GPU, all-gather of
                    round e+1 overlapping the replay of round e. The MI355X path.
  ReplicatedLog /   the same rounds with the all-gather done by torch.distributed (gloo), for
  ReplicatedHashMap multi-process tests on hosts without GPUs-per-rank (CPU `gloo` tests, the
                    1-GPU box rehearsal); the replay is the same C-ABI call
                    (nrg_hashmap_round_segments_async / append_segments + exec).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch
import torch.distributed as dist

from . import _lib as L
from .replica import SL_BACK_MARK, SL_FRONT_MARK


def _ptr(t) -> int:
    if t is None:
        return 0
    return t if isinstance(t, int) else t.data_ptr()


class ReplicaGroup:
    """This process's replica as one member of a libnrgpu.so replica group (RCCL).

    The group id (ncclUniqueId) is created by rank 0 and broadcast over the default
    torch.distributed process group; every rank then joins with its own replica
    (nrg_group_join, ncclCommInitRank on the replica's GPU), which blocks until every rank has
    joined. A caller that ships the id itself (`uid`, from unique_id()) needs no process group:
    tests run one thread per rank over the loopback collectives that way."""

    @staticmethod
    def unique_id() -> bytes:
        """nrg_group_unique_id (ncclGetUniqueId, or a loopback id while those are selected)."""
        uid = (C.c_uint8 * L.NRG_GROUP_ID_BYTES)()
        L.check(L.load().nrg_group_unique_id(uid), "nrg_group_unique_id")
        return bytes(uid)

    def __init__(self, replica, rank: Optional[int] = None, world: Optional[int] = None,
                 pg: Optional[dist.ProcessGroup] = None, uid: Optional[bytes] = None,
                 timeout_ms: Optional[int] = None):
        lib = L.load()
        self.replica = replica
        self.rank = dist.get_rank(pg) if rank is None else rank
        self.world = dist.get_world_size(pg) if world is None else world
        if uid is not None:
            uid = (C.c_uint8 * L.NRG_GROUP_ID_BYTES).from_buffer_copy(uid)
        else:
            uid = (C.c_uint8 * L.NRG_GROUP_ID_BYTES)()
            if self.rank == 0:
                L.check(lib.nrg_group_unique_id(uid), "nrg_group_unique_id")
            if self.world > 1:
                obj = [bytes(uid)]
                dist.broadcast_object_list(obj, src=0, group=pg)
                uid = (C.c_uint8 * L.NRG_GROUP_ID_BYTES).from_buffer_copy(obj[0])
        h = C.c_void_p()
        L.check(lib.nrg_group_join(replica.handle, uid, self.world, self.rank, C.byref(h)), "nrg_group_join")
        self._h = h
        self._lib = lib
        if timeout_ms is not None:
            self.set_timeout(timeout_ms)
        self._round = L.Round()
        self._lens = None

    def set_timeout(self, ms: int):
        """nrg_group_set_timeout: deadline of every wait on the peer ranks. A round or sync whose
        peers miss it raises NrgError(NRG_E_TIMEOUT) naming this rank and round."""
        L.check(self._lib.nrg_group_set_timeout(self._h, int(ms)), "nrg_group_set_timeout")

    def last_error(self) -> str:
        """nrg_group_last_error: the group's sticky failure, '' if none."""
        return (self._lib.nrg_group_last_error(self._h) or b"").decode()

    def _check(self, rc: int, what: str):
        if rc:
            diag = self.last_error()
            L.check(rc, f"{what} [{diag}]" if diag else what)

    def set_input_stream(self, stream_ptr: int):
        """All-gathers wait only for work on this stream (where the inputs are produced)."""
        L.check(self._lib.nrg_group_set_input_stream(self._h, 0, C.c_void_p(stream_ptr)))

    def round_async(self, recs, n: int, resp=None, some=None, get_keys=None, n_gets: int = 0, get_vals=None,
                    get_found=None, seg_lens: Optional[Sequence[int]] = None):
        """One NR round (device tensors or raw pointers): all-gather + replay + local reads
        (get_keys: a hashmap's or a skip list's Gets, answered against the post-round state).

        seg_lens: every rank's segment length, the same list on every rank (the stream-ordered
        path; a header checks it on every rank). None: the lengths are exchanged first, which
        costs one host round trip but lets every rank's n differ."""
        r = self._round
        r.recs, r.n, r.resp, r.some = _ptr(recs), n, _ptr(resp), _ptr(some)
        r.get_keys, r.n_gets, r.get_vals, r.get_found = _ptr(get_keys), n_gets, _ptr(get_vals), _ptr(get_found)
        lens = None
        if seg_lens is not None:
            if self._lens is None or list(self._lens) != list(seg_lens):
                self._lens = (C.c_uint64 * self.world)(*seg_lens)
            lens = self._lens
        rc = self._lib.nrg_group_round_async(self._h, C.byref(r), lens)
        if rc:
            self._check(rc, "nrg_group_round_async")

    def sync(self):
        self._check(self._lib.nrg_group_sync(self._h), "nrg_group_sync")

    def verify(self):
        """nrg_group_verify (a collective: every rank calls it): (identical, digests), digests an
        ndarray [world, 3] of every rank's (count, sum, xor) in rank order. Replicas that differ
        are a result (identical False), not an error. The members of a partitioned group hold one
        partition each, so they are never identical: add their triples (nrgpu.digest.combine)."""
        import numpy as np

        out = np.zeros((self.world, 3), np.uint64)
        same = C.c_int(0)
        self._check(self._lib.nrg_group_verify(self._h, C.c_void_p(out.ctypes.data), C.byref(same)),
                    "nrg_group_verify")
        return bool(same.value), out

    def resync(self, root: int = 0):
        """nrg_group_resync (a collective: every rank calls it with the same root): rank `root`'s
        replica is snapshotted and every other rank's replica restored from it, log positions
        included; what to do when verify() says the replicas differ. For replicated groups."""
        self._check(self._lib.nrg_group_resync(self._h, int(root)), "nrg_group_resync")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.nrg_group_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class Gathered:
    """One round's all-gathered write log (in flight until wait())."""

    __slots__ = ("buf", "work", "stride", "lens", "words")

    def __init__(self, buf, work, stride, lens, words):
        self.buf, self.work, self.stride, self.lens, self.words = buf, work, stride, lens, words

    def wait(self):
        if self.work is not None:
            self.work.wait()
            self.work = None


class ReplicatedLog:
    """One replica per rank of any NR data structure, driven in rounds of write segments, with
    the all-gather done by torch.distributed (gloo; see ReplicaGroup for RCCL).

    round() = gather_async() + replay(). Records are int64 tensors [W, words] (words = record
    bytes / 8: hashmap 2, stack 1, synthetic 4)."""

    NBUF = 3  # gathered-log buffers in rotation

    def __init__(self, replica, group: Optional[dist.ProcessGroup] = None, device: Optional[torch.device] = None):
        self.replica = replica
        self.group = group
        self.rank = dist.get_rank(group)
        self.world = dist.get_world_size(group)
        self.device = device if device is not None else torch.device("cpu")
        self.origins = [r + 1 for r in range(self.world)]  # replica ids start at 1 (nr/src/log.rs:272-292)
        self._bufs = [None] * self.NBUF
        self._next = 0

    def _buf(self, need: int) -> torch.Tensor:
        i = self._next
        self._next = (i + 1) % self.NBUF
        b = self._bufs[i]
        if b is None or b.numel() < need:
            b = torch.empty(need, dtype=torch.int64)
            self._bufs[i] = b
        return b[:need]

    def exchange_lengths(self, W: int):
        t = torch.tensor([W], dtype=torch.int64)
        out = [torch.zeros_like(t) for _ in range(self.world)]
        dist.all_gather(out, t, group=self.group)
        return [int(x.item()) for x in out]

    def gather_async(self, recs: torch.Tensor, stride: Optional[int] = None, lens=None) -> Gathered:
        """All-gather this rank's write segment (records in issue order). Fixed-size rounds pass
        `stride` (segment capacity) and skip the length exchange."""
        if recs.dim() == 1:
            recs = recs.reshape(-1, 1)
        W, words = recs.shape
        if lens is None:
            lens = [W] * self.world if stride is not None else self.exchange_lengths(W)
        if stride is None:
            stride = max(lens) if lens else 0
        seg = torch.zeros((stride, words), dtype=torch.int64)
        seg[:W] = recs.cpu()
        out = self._buf(self.world * stride * words)
        dist.all_gather_into_tensor(out, seg.reshape(-1), group=self.group)
        return Gathered(out.to(recs.device), None, stride, lens, words)

    def replay(self, g: Gathered, resp: Optional[torch.Tensor] = None, some: Optional[torch.Tensor] = None):
        """Log::append of the gathered segments in rank order (the round's global log order),
        then Log::exec; responses only for this rank's own segment (nr/src/replica.rs:576-578)."""
        g.wait()
        firsts = self.replica.log_append_segments(g.buf, g.stride, g.lens, self.origins)
        lo = firsts[self.rank]
        self.replica.log_exec_device(lo, lo + g.lens[self.rank], resp, some)

    def round(self, recs: torch.Tensor, resp=None, some=None, stride: Optional[int] = None, lens=None):
        g = self.gather_async(recs, stride, lens)
        self.replay(g, resp, some)
        return g.buf


class ReplicatedHashMap(ReplicatedLog):
    """NrHashMap replicas: a round is (write segment, local reads); the fused device round
    appends, replays and answers the reads against the post-round state."""

    def replay(self, g: Gathered, get_keys: torch.Tensor, get_vals: torch.Tensor, get_found: torch.Tensor,
               prev: Optional[torch.Tensor] = None, prev_found: Optional[torch.Tensor] = None):
        """Append the gathered segments in rank order, replay them, answer this rank's reads
        against the post-round state; Put responses (prev) only for this rank's own segment."""
        g.wait()
        self.replica.hm_round_segments_device(g.buf, g.stride, g.lens, self.origins, self.rank, get_keys,
                                              get_keys.shape[0], get_vals, get_found, prev, prev_found)

    def round(self, puts: torch.Tensor, get_keys: torch.Tensor, get_vals: torch.Tensor, get_found: torch.Tensor,
              prev: Optional[torch.Tensor] = None, prev_found: Optional[torch.Tensor] = None,
              stride: Optional[int] = None, lens=None):
        """One NR round: puts [W, 2] int64 (key, value) on this rank's device, in issue order."""
        g = self.gather_async(puts, stride, lens)
        self.replay(g, get_keys, get_vals, get_found, prev, prev_found)
        return g.buf.view(-1, 2)


# ---- cnr-style key-partitioned NrHashMap and skip list ---------------------
# cnr maps every operation to one of several logs with LogMapper::hash (cnr/src/lib.rs:134-167,
# cnr/src/replica.rs:430-445) and each log replays on its own (:673-736). Here partition p's log
# lives on rank p, which holds only the keys it owns: a round routes Puts and Gets to their
# owners, every owner replays what it received in rank order (for each key the NR global-log
# order) and answers its Gets, and the answers come back in the caller's order. Answers equal
# NR's; the replicas hold one partition each (their digests add up to the NR replica's).
# The reference runs its skip list only this way (skiplist-mlnr, benches/lockfree.rs:73-97, :228-317):
# a PartitionedGroup of skip-list replicas takes the same rounds (Push(k, v) records, Get(k) reads)
# and adds the group-wide ordered reads no single partition can answer.

_M1, _M2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def key_owner(keys, parts: int):
    """nrg_key_owner over an array: (low 32 bits of splitmix64(key)) * parts >> 32."""
    import numpy as np

    z = np.ascontiguousarray(keys).view(np.uint64).copy()
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(_M1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(_M2)
        z = z ^ (z >> np.uint64(31))
    return ((z & np.uint64(0xFFFFFFFF)) * np.uint64(parts) >> np.uint64(32)).astype(np.int64)


class PartitionedGroup(ReplicaGroup):
    """This rank's replica (a hashmap or a skip list; every rank the same kind) as partition `rank`
    of a key-partitioned group (libnrgpu.so, RCCL send/recv): nrg_group_partitioned_round. For a
    skip list prev / prev_found receive the Push responses (the key, 1); on a group that agreed on
    removal (enable_removal) they are the Push / Remove responses, written by the keys' owners: Push
    (the key, 1), Remove (the previous value, 1) or (0, 0), in issue order."""

    def enable_removal(self, tombstone: int = 2**64 - 1):
        """nrg_group_skiplist_enable_removal (a collective: every rank calls it with the same
        tombstone): from here on a record whose val == tombstone is Remove(key) in this group's
        partitioned rounds, answered by the key's owner. Nothing is enabled anywhere unless every rank
        agrees; idempotent for one tombstone; there is no way back."""
        rc = self._lib.nrg_group_skiplist_enable_removal(self._h, int(tombstone))
        if rc:
            self._check(rc, "nrg_group_skiplist_enable_removal")

    def enable_pops(self, front_mark: int = SL_FRONT_MARK, back_mark: int = SL_BACK_MARK):
        """nrg_group_skiplist_enable_pops (a collective: every rank calls it with the same marks): from
        here on pop / pop_front / pop_back pop the whole partitioned map, and a partitioned round that
        holds a mark record on any rank is refused on every rank. Idempotent for one pair of marks;
        there is no way back."""
        rc = self._lib.nrg_group_skiplist_enable_pops(self._h, int(front_mark), int(back_mark))
        if rc:
            self._check(rc, "nrg_group_skiplist_enable_pops")

    def pop(self, reqs):
        """nrg_group_skiplist_pop (a collective: every rank calls it, with its own requests and any
        number of them). reqs: a list of (n, back), back = 0 for PopFront x n and 1 for PopBack x n. The
        ranks' requests in rank order are one run of pop records against the whole partitioned map.
        Returns (counts, keys, vals): counts[j] entries popped by request j (a numpy uint64 array), and
        this rank's popped entries packed in request order, each request's in the order popped (numpy
        uint64 arrays). The buffers are sized from the requests, each clipped to world x this replica's
        capacity (no map of a group whose ranks opened alike holds more); synchronous."""
        import numpy as np

        reqs = [(int(n), int(back)) for n, back in reqs]
        n = len(reqs)
        dev = torch.device("cuda", self.replica.device)
        room = self.world * self.replica.sl_capacity()  # no map of this group holds more
        cap = sum(min(c, room) for c, _ in reqs)
        arr = (L.PopReq * max(n, 1))(*[L.PopReq(c, b, 0) for c, b in reqs])
        resp = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
        some = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
        keys = torch.zeros(max(cap, 1), dtype=torch.int64, device=dev)
        vals = torch.zeros_like(keys)
        total = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)  # the buffers exist before the replica's stream writes them
        q = L.Pops(arr, n, _ptr(resp), _ptr(some), _ptr(keys), _ptr(vals), cap, _ptr(total))
        rc = self._lib.nrg_group_skiplist_pop(self._h, C.byref(q))
        if rc:
            self._check(rc, "nrg_group_skiplist_pop")
        m = int(total.item())
        return (resp[:n].cpu().numpy().view(np.uint64), keys[:m].cpu().numpy().view(np.uint64),
                vals[:m].cpu().numpy().view(np.uint64))

    def pop_front(self, n: int = 1):
        """SkipMap::pop_front n times over the whole partitioned map (a collective: pop([(n, 0)]))."""
        return self.pop([(n, 0)])

    def pop_back(self, n: int = 1):
        """SkipMap::pop_back n times over the whole partitioned map (a collective: pop([(n, 1)]))."""
        return self.pop([(n, 1)])

    def round(self, puts, n: int, get_keys, n_gets: int, get_vals, get_found, prev=None, prev_found=None):
        """One round, queued once its counts are exchanged (nrg_group_partitioned_round)."""
        r = self._round
        r.recs, r.n, r.resp, r.some = _ptr(puts), n, _ptr(prev), _ptr(prev_found)
        r.get_keys, r.n_gets, r.get_vals, r.get_found = _ptr(get_keys), n_gets, _ptr(get_vals), _ptr(get_found)
        rc = self._lib.nrg_group_partitioned_round(self._h, C.byref(r))
        if rc:
            self._check(rc, "nrg_group_partitioned_round")

    def round_async(self, puts, n: int, get_keys, n_gets: int, get_vals, get_found, prev=None, prev_found=None):
        """Pipelined: queue this round, move the previous one to its owners and replay it, and send
        the one before back (nrg_group_partitioned_round_async). A round's buffers stay borrowed
        for the next two round_async calls, or until flush / sync."""
        r = self._round
        r.recs, r.n, r.resp, r.some = _ptr(puts), n, _ptr(prev), _ptr(prev_found)
        r.get_keys, r.n_gets, r.get_vals, r.get_found = _ptr(get_keys), n_gets, _ptr(get_vals), _ptr(get_found)
        rc = self._lib.nrg_group_partitioned_round_async(self._h, C.byref(r))
        if rc:
            self._check(rc, "nrg_group_partitioned_round_async (the previous round)")

    def flush(self):
        """Complete the round queued by round_async, if any."""
        rc = self._lib.nrg_group_partitioned_flush(self._h)
        if rc:
            self._check(rc, "nrg_group_partitioned_flush")

    def seek(self, keys, mode: int):
        """nrg_group_skiplist_seek (a collective: every rank calls it with the same mode, its own
        keys and any number of them): SkipMap::lower_bound / upper_bound over the whole partitioned
        map for a 1-D int64 device tensor of keys (u64 bit patterns). Returns (out_keys, out_vals,
        found) device tensors; synchronous (torch's current stream is drained first, so the keys
        may have been produced on it)."""
        keys = keys.contiguous()
        n = keys.numel()
        ok = torch.zeros(max(n, 1), dtype=torch.int64, device=keys.device)
        ov = torch.zeros_like(ok)
        found = torch.zeros(max(n, 1), dtype=torch.uint8, device=keys.device)
        torch.cuda.current_stream(keys.device).synchronize()  # the buffers exist before the library writes them
        q = L.Seek(_ptr(keys) if n else 0, n, _ptr(ok), _ptr(ov), _ptr(found))
        rc = self._lib.nrg_group_skiplist_seek(self._h, C.byref(q), int(mode))
        if rc:
            self._check(rc, "nrg_group_skiplist_seek")
        return ok[:n], ov[:n], found[:n]

    def scan(self, keys, mode: int, limit: int):
        """nrg_group_skiplist_scan (a collective: every rank calls it with the same mode and limit, its
        own keys and any number of them): SkipMap::range from a bound, the first `limit` entries over
        the whole partitioned map (GE / GT ascending, LE / LT descending), for a 1-D int64 device
        tensor of keys (u64 bit patterns). Returns (out_keys [n, limit], out_vals [n, limit],
        counts [n] int32) device tensors, row i valid in columns 0 .. counts[i] - 1; synchronous."""
        keys = keys.contiguous()
        n, limit = keys.numel(), int(limit)
        ok = torch.zeros(max(n, 1) * max(limit, 1), dtype=torch.int64, device=keys.device)
        ov = torch.zeros_like(ok)
        cnt = torch.zeros(max(n, 1), dtype=torch.int32, device=keys.device)
        torch.cuda.current_stream(keys.device).synchronize()  # the buffers exist before the library writes them
        q = L.Scan(_ptr(keys) if n else 0, n, _ptr(ok), _ptr(ov), _ptr(cnt))
        rc = self._lib.nrg_group_skiplist_scan(self._h, C.byref(q), int(mode), limit)
        if rc:
            self._check(rc, "nrg_group_skiplist_scan")
        return ok[: n * limit].view(n, limit), ov[: n * limit].view(n, limit), cnt[:n]

    def items(self, page: int = 1024):
        """The whole partitioned map in ascending key order, as (key, value) pairs of Python ints
        (u64): pages of `page` entries by scan, GE(0) first, then GT(the last key seen). The
        library's partitioned dump. A generator over a collective: every rank iterates it in step,
        with the same page, to its end."""
        dev = torch.device("cuda", self.replica.device)
        key, mode = 0, L.NRG_SEEK_GE
        while True:
            q = torch.tensor([key - (1 << 64) if key >= (1 << 63) else key], dtype=torch.int64, device=dev)
            k, v, c = self.scan(q, mode, page)
            m = int(c[0].item())
            ks = k[0, :m].cpu().numpy().view("uint64").tolist()
            vs = v[0, :m].cpu().numpy().view("uint64").tolist()
            yield from zip(ks, vs)
            if m < page:
                return
            key, mode = ks[-1], L.NRG_SEEK_GT

    def range_count(self, los, his):
        """nrg_group_skiplist_range_count (a collective): the number of keys of the whole
        partitioned map in each [lo, hi], both inclusive (0 where lo > hi), for two 1-D int64 device
        tensors of equal length. Returns a device tensor; synchronous."""
        los, his = los.contiguous(), his.contiguous()
        if los.shape != his.shape:
            raise ValueError("los and his differ in length")
        n = los.numel()
        out = torch.zeros(max(n, 1), dtype=torch.int64, device=los.device)
        torch.cuda.current_stream(los.device).synchronize()  # the buffers exist before the library writes them
        q = L.Count(_ptr(los) if n else 0, _ptr(his) if n else 0, n, _ptr(out))
        rc = self._lib.nrg_group_skiplist_range_count(self._h, C.byref(q))
        if rc:
            self._check(rc, "nrg_group_skiplist_range_count")
        return out[:n]


# ---- file-partitioned file store (nrfs-mlnr) ---------------------------------------------------
# benches/nrfs.rs is a cnr benchmark with one log per file (LogMapper::hash = fd - 1, :25-39; hash % logs,
# cnr/src/replica.rs:430-445): ops on different files never share a log. Here partition p's log lives on
# rank p; every rank holds all F files and a round changes, on rank p, only the files p owns.


def memfs_owner(inos, parts: int):
    """nrg_memfs_owner over an array: (ino - NRG_MEMFS_FIRST_INO) % parts, and 0 for an ino below
    NRG_MEMFS_FIRST_INO (and for parts == 0, as the C function answers)."""
    import numpy as np

    ino = np.ascontiguousarray(inos).astype(np.uint64, copy=False).reshape(-1)
    first = np.uint64(L.NRG_MEMFS_FIRST_INO)
    if parts == 0:
        return np.zeros(ino.shape, np.int64)
    idx = np.where(ino >= first, ino - first, np.uint64(0))  # (below the first ino: 0 % parts = 0)
    return (idx % np.uint64(parts)).astype(np.int64)


class FilePartitionedGroup(ReplicaGroup):
    """This rank's file-store replica as partition `rank` of a file-partitioned group
    (nrg_group_file_round, nrg_group_memfs_pread): every rank opened with the same F and B, sizes enabled
    on all or on none."""

    def owner(self, ino: int) -> int:
        """The rank that owns file `ino` in this group."""
        return int(self._lib.nrg_memfs_owner(int(ino), self.world))

    def reserve(self, file_bytes: int):
        """Room for `file_bytes` bytes in every file on this rank's replica (nrg_memfs_reserve; sized
        contexts). Every rank calls it with the same value between rounds: a file-partitioned round
        needs the same B everywhere, and refuses members with a growth bound (nrg_set_max_capacity),
        since an owner replays its own files' records alone."""
        L.check(self._lib.nrg_memfs_reserve(self.replica._h, int(file_bytes)), "nrg_memfs_reserve")

    def round(self, recs, n: int, resp=None, some=None):
        """One round of this rank's n nrg_memfs_op records (device tensor or raw pointer), queued once
        the counts are exchanged; resp / some (n * 136 bytes, n bytes; both or neither) receive the
        responses in issue order. sync() waits for it; the buffers stay borrowed until then."""
        r = self._round
        r.recs, r.n, r.resp, r.some = _ptr(recs), n, _ptr(resp), _ptr(some)
        r.get_keys, r.n_gets, r.get_vals, r.get_found = 0, 0, 0, 0
        rc = self._lib.nrg_group_file_round(self._h, C.byref(r))
        if rc:
            self._check(rc, "nrg_group_file_round")

    def pread(self, reqs, cap: Optional[int] = None):
        """nrg_group_memfs_pread (a collective: every rank calls it, with its own requests and any number
        of them): POSIX pread of each request against its file's owner. reqs: a device uint8 tensor of
        24-byte nrg_memfs_rd requests, or None for an idle rank. cap defaults to n * B. Returns (data,
        offs, some): data[offs[i]:offs[i + 1]] are request i's bytes (data has cap bytes), offs n + 1
        int64 words, some n bytes. NRG_E_CAPACITY (raised) when a rank's answer exceeds its cap."""
        n = 0 if reqs is None else reqs.numel() // 24
        dev = torch.device("cuda", torch.cuda.current_device()) if reqs is None else reqs.device
        if cap is None:
            B = C.c_uint64()
            L.check(self._lib.nrg_memfs_geometry(self.replica._h, None, C.byref(B)), "nrg_memfs_geometry")
            cap = n * B.value
        data = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        offs = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        some = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)  # the buffers exist before the replica's stream writes them
        rd = L.Pread(_ptr(reqs), n, data.data_ptr() if cap else 0, cap, offs.data_ptr(), some.data_ptr())
        rc = self._lib.nrg_group_memfs_pread(self._h, C.byref(rd))
        if rc:
            self._check(rc, "nrg_group_memfs_pread")
        return data[:cap], offs, some[:n]


class PartitionedHashMap:
    """Key-partitioned rounds with the exchanges done by torch.distributed (all_to_all_single;
    gloo on CPU tests, see PartitionedGroup for RCCL). `replica` must provide
    partitioned_replay(puts [p, 2] int64, keys [k] int64, want_prev) -> (vals, found, prev, prev_found)
    (DeviceReplica does; CPU tests use an oracle-backed double)."""

    def __init__(self, replica, group: Optional[dist.ProcessGroup] = None):
        self.replica = replica
        self.group = group
        self.rank = dist.get_rank(group)
        self.world = dist.get_world_size(group)

    def _split(self, keys: torch.Tensor):
        """Stable partition by owner: (order, counts); order[j] = index of the j-th routed item."""
        import numpy as np

        own = key_owner(keys.cpu().numpy(), self.world)
        order = np.argsort(own, kind="stable")
        counts = np.bincount(own, minlength=self.world)
        return torch.from_numpy(order), [int(c) for c in counts]

    def _a2a(self, send: torch.Tensor, send_counts, recv_counts):
        out = torch.empty((sum(recv_counts),) + tuple(send.shape[1:]), dtype=send.dtype)
        dist.all_to_all_single(out, send.contiguous(), [c for c in recv_counts], [c for c in send_counts],
                               group=self.group)
        return out

    def round(self, puts: torch.Tensor, get_keys: torch.Tensor, get_vals: torch.Tensor, get_found: torch.Tensor,
              prev: Optional[torch.Tensor] = None, prev_found: Optional[torch.Tensor] = None):
        """puts [W, 2] int64 (key, value) and get_keys [R] in issue order, on any device; answers
        land in get_vals / get_found (and prev / prev_found) in that order."""
        dev = get_vals.device
        p_cpu, k_cpu = puts.reshape(-1, 2).cpu(), get_keys.reshape(-1).cpu()
        p_order, p_cnt = self._split(p_cpu[:, 0])
        k_order, k_cnt = self._split(k_cpu)
        want = torch.tensor([1 if prev is not None else 0], dtype=torch.int64)
        sizes = torch.tensor(p_cnt + k_cnt + [int(want.item())], dtype=torch.int64)
        allsz = [torch.zeros_like(sizes) for _ in range(self.world)]
        dist.all_gather(allsz, sizes, group=self.group)  # every rank's counts (and wants-prev flag)
        w = self.world
        p_from = [int(allsz[s][self.rank]) for s in range(w)]
        k_from = [int(allsz[s][w + self.rank]) for s in range(w)]
        any_prev = any(int(allsz[s][2 * w]) for s in range(w))
        rput = self._a2a(p_cpu[p_order], p_cnt, p_from)      # received in rank order = log order
        rkey = self._a2a(k_cpu[k_order], k_cnt, k_from)
        vals, found, pv, pf = self.replica.partitioned_replay(rput, rkey, any_prev)
        a_vals = self._a2a(vals.cpu(), k_from, k_cnt)
        a_found = self._a2a(found.cpu(), k_from, k_cnt)
        back_v = torch.empty_like(a_vals)
        back_f = torch.empty_like(a_found)
        back_v[k_order] = a_vals
        back_f[k_order] = a_found
        get_vals.copy_(back_v.to(dev))
        get_found.copy_(back_f.to(dev))
        if any_prev:
            a_pv = self._a2a(pv.cpu(), p_from, p_cnt)
            a_pf = self._a2a(pf.cpu(), p_from, p_cnt)
            if prev is not None:
                bv, bf = torch.empty_like(a_pv), torch.empty_like(a_pf)
                bv[p_order] = a_pv
                bf[p_order] = a_pf
                prev.copy_(bv.to(prev.device))
                prev_found.copy_(bf.to(prev_found.device))
