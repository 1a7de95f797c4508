/*
 * nrgpu.h — C ABI of the MI355X-native node-replication (NR) log-replay path.
 *
 * One `nrg_ctx` is one NR *replica* living on one GPU: it owns the replicated data
 * structure in HBM (NrHashMap / Stack / AbstractDataStructure / FIFO queue / VSpace / skip list), its copy of the shared
 * operation log (an HBM ring of fixed-width records tagged by logical log index), the
 * per-replica replay epoch (`ltail`), scratch for the replay kernels, and a HIP stream.
 *
 * Each entry point replaces one piece of the reference's Rust API (paths relative to the
 * reference checkout `junghan0611/node-replication`):
 *
 *   nrg_open / nrg_close          Replica::new + Log::new            nr/src/replica.rs:184-232, nr/src/log.rs:179-242
 *   nrg_log_append*               Log::append                        nr/src/log.rs:343-427
 *   nrg_log_exec*                 Log::exec -> Dispatch::dispatch_mut nr/src/log.rs:473-524, nr/src/replica.rs:572-581
 *   nrg_log_state                 head/tail/ctail/ltails            nr/src/log.rs:88-131, :671-679
 *   nrg_log_reset                 Log::reset                         nr/src/log.rs:593-611
 *   nrg_hashmap_get*              Replica::execute -> dispatch       nr/src/replica.rs:404-410,483-497; benches/hashmap.rs:107-111
 *   nrg_hashmap_round_async       Replica::combine (append+exec) + read batch   nr/src/replica.rs:544-595
 *   nrg_hashmap_prefill*          NrHashMap::default                 benches/hashmap.rs:91-100
 *   nrg_hashmap_dump / digest     Replica::verify(closure)           nr/src/replica.rs:443-467
 *   nrg_digest* / nrg_group_verify Replica::verify on the device: one  nr/src/replica.rs:443-467
 *                                 triple per replica, every kind
 *   nrg_snapshot_* / nrg_restore  Replica::new from a state, not  nr/src/replica.rs:184-232, :443-467
 *   / nrg_group_resync            from log index 0; verify's view
 *   nrg_stack_*                   Stack Dispatch                    benches/stack.rs:36-84, nr/tests/stack.rs:31-96
 *   nrg_*_reserve / _capacity,    Vec::reserve / capacity, SegQueue's  benches/stack.rs:36-84,
 *   nrg_set_max_capacity          segments, VSpace's heap tables     benches/lockfree_comparisons.rs:75-101, benches/vspace.rs:388-419
 *   nrg_memfs_reserve, and        the growing vector behind          benches/memfs.rs:106-192 (a write past the end
 *   nrg_set_max_capacity on it    NrMemFilesystem's files            extends the file)
 *   nrg_synth_*                   AbstractDataStructure Dispatch     benches/synthetic.rs:60-195
 *   nrg_queue_*                   FIFO queue Dispatch (SegQueueWrapper) benches/lockfree.rs:43-52, benches/lockfree_comparisons.rs:75-101
 *   nrg_vspace_*                  VSpace Dispatch (x86-64 page table) benches/vspace.rs:177-381, :436-467, :499-526
 *   nrg_skiplist_*                SkipListWrapper Dispatch (SkipMap)  benches/lockfree.rs:73-97, :278-317,
 *                                                                     benches/lockfree_partitioned.rs:86-118
 *   nrg_memfs_*                   NrMemFilesystem Dispatch (Write /   benches/memfs.rs:24-85, :112-121, :194-292
 *                                 Read / GetAttr, all through the log)
 *   nrg_memfs_pread*              Replica::execute -> read_only of    nr/src/replica.rs:404-410, :483-497;
 *                                 OpRd::FileRead, any length          benches/nrfs.rs:16-18, :88-101
 *   nrg_memfs_pwrite*             Replica::combine of OpWr::FileWrite, benches/nrfs.rs:103-115;
 *                                 logged writes of any length         nr/src/replica.rs:544-595
 *   nrg_memfs_pread_logged*       Replica::combine of OperationWr::Read, benches/memfs.rs:73-78, :267-282;
 *                                 logged reads of any length          nr/src/replica.rs:544-595
 *   nrg_group_*                   the shared Log across NUMA nodes   nr/src/log.rs:494-511 (every replica
 *                                 (RCCL all-gather of write segments) replays every entry), :473-524
 *   nrg_key_owner, nrg_hashmap_partition*, nrg_group_partitioned_round
 *                                 cnr's key-partitioned logs         cnr/src/lib.rs:134-167 (LogMapper::hash),
 *                                 (one log per GPU, RCCL send/recv)  cnr/src/replica.rs:430-445, :673-736
 *   nrg_memfs_owner, nrg_memfs_partition_async, nrg_memfs_route_back_async, nrg_group_file_round
 *                                 nrfs-mlnr: one log per file        benches/nrfs.rs:25-39 (hash = fd - 1),
 *                                 (files partitioned over the GPUs)  :132-141; cnr/src/replica.rs:430-445
 *   nrg_memfs_rd_partition_async, nrg_memfs_pread_repack_async, nrg_group_memfs_pread
 *                                 exec_ro(OpRd::FileRead(fd)) routed benches/nrfs.rs:88-101, :146-152;
 *                                 to the owner of the file's log     cnr/src/replica.rs:430-445
 *
 * Conventions
 *   - Every function returns NRG_OK (0) or a negative NRG_E_* code. Nothing throws or aborts.
 *   - A context is NOT thread-safe; callers serialise calls on one context, exactly as the
 *     combiner lock serialises Log::exec on one replica (nr/src/replica.rs:508-540).
 *     Distinct contexts (one per GPU) may be driven from distinct threads.
 *   - `*_async` functions take DEVICE pointers and are ordered on the context's stream
 *     (see nrg_set_stream); buffers are borrowed until the stream reaches that point.
 *     Device-side failures (table full, probe overrun) are latched and reported by the
 *     next nrg_sync / synchronous call.
 *   - Functions without `_async` take HOST pointers and return after the work completed.
 *   - Records in the log are fixed-width structs (below); the log index of a record is its
 *     position in the global total order of writes, exactly as in the reference.
 *   - Responses are produced only for a caller-chosen window [resp_lo, resp_hi) of log
 *     indices: in NR only the replica that appended an op receives its response
 *     (nr/src/replica.rs:576-578), and a replica's own ops form contiguous windows.
 */
#ifndef NRGPU_H
#define NRGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes ---------------------------------------------------------------- */
#define NRG_OK 0
#define NRG_E_INVAL (-1)        /* bad argument / wrong data-structure kind              */
#define NRG_E_HIP (-2)          /* a HIP runtime call failed                             */
#define NRG_E_TABLE_FULL (-3)   /* hash table probe exhausted: a fixed table, or one grown
                                   to config.hashmap_max_log2_slots, is full             */
#define NRG_E_RING_FULL (-4)    /* log ring cannot hold the append even after GC         */
#define NRG_E_NOMEM (-5)        /* device allocation failed                              */
#define NRG_E_NOT_SYNCED (-6)   /* read requested while ltail < tail (sync first)        */
#define NRG_E_CAPACITY (-7)     /* batch exceeds configured max / stack capacity         */
#define NRG_E_NODEV (-8)        /* no HIP device with that ordinal                       */

/* ---- data-structure kinds --------------------------------------------------------- */
#define NRG_DS_HASHMAP 1u   /* NrHashMap: u64 -> u64, Put/Get                       */
#define NRG_DS_STACK 2u     /* Stack: Vec<u32>, Push/Pop, Peek                      */
#define NRG_DS_SYNTHETIC 3u /* AbstractDataStructure(n, 20, 5, 2, 1)                */
#define NRG_DS_QUEUE 4u     /* FIFO queue of u64: Push/Pop, Len   benches/lockfree.rs:43-52 */
#define NRG_DS_VSPACE 5u    /* four-level page table: Map/MapDevice, Identify  benches/vspace.rs:483-526 */
#define NRG_DS_SKIPLIST 6u  /* ordered map u64 -> u64 (SkipMap): Push(k, v) / Get, seek, range
                               benches/lockfree.rs:73-97, benches/lockfree_partitioned.rs:86-118 */
#define NRG_DS_MEMFS 7u     /* file store: Write / Read / GetAttr / SetAttr on files of fixed capacity, reads
                               through the log   benches/memfs.rs:24-85, :194-292 */

/* ---- log record layouts (one WriteOperation each) --------------------------------- */
/* NrHashMap WriteOperation::Put(key, val)               benches/hashmap.rs:52-56;
 * the skip list's OpWr::Push(key, val)                  benches/lockfree.rs:86-97      */
typedef struct {
    uint64_t key;
    uint64_t val;
} nrg_put;

/* Stack WriteOperation: op = NRG_STACK_PUSH (val used) or NRG_STACK_POP  benches/stack.rs:22-28 */
#define NRG_STACK_POP 0u
#define NRG_STACK_PUSH 1u
typedef struct {
    uint32_t val;
    uint32_t op;
} nrg_stack_op;

/* Synthetic WriteOperation: WriteOnly/ReadWrite(tid, rnd1, rnd2)  benches/synthetic.rs:33-39 */
#define NRG_SYNTH_WRITE_ONLY 0u
#define NRG_SYNTH_READ_WRITE 1u
typedef struct {
    uint64_t tid;
    uint64_t r1;
    uint64_t r2;
    uint64_t op;
} nrg_synth_op;

/* Queue WriteOperation (QueueWr): op = NRG_QUEUE_PUSH (val used) or NRG_QUEUE_POP
 * benches/lockfree.rs:43-47; the one read, QueueRd::Len (:49-52), carries no record */
#define NRG_QUEUE_POP 0u
#define NRG_QUEUE_PUSH 1u
typedef struct {
    uint64_t val;
    uint64_t op;
} nrg_queue_op;

/* VSpace WriteOperation (OpcodeWr, benches/vspace.rs:483-487): op = NRG_VSPACE_MAP
 * (Map(vbase, len, rights, pbase)) or NRG_VSPACE_MAP_DEVICE (MapDevice(vbase, pbase, len), which
 * maps ReadWriteUser and ignores `rights`). rights: 1..8 in MapAction order (:54-73: ReadUser,
 * ReadKernel, ReadWriteUser, ReadWriteKernel, ReadExecuteUser, ReadExecuteKernel,
 * ReadWriteExecuteUser, ReadWriteExecuteKernel). Domain: vbase, pbase and len multiples of 4096;
 * vbase, pbase < 2^48; len < 2^30 (so 1 GiB pages never arise); vbase + len <= 2^48; for Map,
 * rights in 1..8. The reference asserts on anything else; here such a record changes nothing,
 * answers some = 0 with a = vbase, and latches NRG_E_INVAL once. The one read,
 * OpcodeRd::Identify(vaddr) (:489-492), carries no record (nrg_vspace_resolve). */
#define NRG_VSPACE_MAP 0u
#define NRG_VSPACE_MAP_DEVICE 1u
typedef struct {
    uint64_t vbase;
    uint64_t pbase;
    uint64_t len;
    uint32_t op;
    uint32_t rights;
} nrg_vspace_op;
/* VSpace write response, Result<(u64, u64), VSpaceError> (:502): Ok -> some = 1 and (a, b) =
 * (pbase, len) for Map, (0, 0) for MapDevice; Err(VSpaceError{at}) -> some = 0, a = at, b = 0 */
typedef struct {
    uint64_t a;
    uint64_t b;
} nrg_vspace_resp;
/* One leaf entry of the page table (nrg_vspace_dump): the first virtual address it maps and the
 * entry itself (paddr | flags; bit 7, PS, set for a 2 MiB page) */
typedef struct {
    uint64_t vaddr;
    uint64_t entry;
} nrg_vspace_leaf;

/* File store WriteOperation (OperationWr, benches/memfs.rs:24-85). In memfs.rs ReadOperation = ()
 * and dispatch is unreachable!() (:194-201): Read is a WRITE operation, logged like Write, and its
 * answer is the file as every earlier record of the log left it. A record carries at most 128 data
 * bytes ([3; 128] in generate_fs_operations, :294-322). The reference shows the op set, the initial
 * file, Written(len) and Data(bytes); everything else is defined here as POSIX pwrite / pread on
 * files of fixed size (the file system behind memfs.rs, btfs, is not part of the reference checkout).
 * A replica holds F files of B bytes, inodes NRG_MEMFS_FIRST_INO .. NRG_MEMFS_FIRST_INO + F - 1.
 *   WRITE    offset + len <= B: bytes [offset, offset + len) take data; some = 1, n = len
 *            (Written(len), :88-98); len = 0 is a valid no-op. Else nothing changes; some = 0,
 *            n = NRG_MEMFS_EFBIG.
 *   READ     some = 1, n = min(len, B - offset), or 0 where offset >= B; data[0, n) are the file's
 *            bytes (Data(bytes)), data[n, 128) zero.
 *   GETATTR  some = 1, n = B (Attr: the size); data zero.
 * A record is checked in this order: len > 128 or an unknown op: some = 0, n = NRG_MEMFS_EINVAL,
 * nothing changes and NRG_E_INVAL is latched once (the page table's rule for a record outside its
 * domain); an ino outside the range: some = 0, n = NRG_MEMFS_ENOENT; then the Write's range. Every
 * error response has data all zero.
 * SIZES (OperationWr::SetAttr{ino, new_attrs}, memfs.rs:26-85, dispatched at :210-213; the file system
 * behind it grows a file when a Write ends past its end). Off unless nrg_memfs_enable_sizes was called:
 * without it everything above holds byte for byte and op 3 is the unknown op it always was. With it a
 * file has a CAPACITY B and a SIZE 0 .. B (B when sizes are enabled), defined as POSIX pwrite / pread /
 * ftruncate, every op evaluated at its own log position:
 *   WRITE    valid exactly when offset + len <= B, as above; with len > 0, size = max(size, offset + len),
 *            and a gap between the old size and offset reads as zero.
 *   READ     n = offset >= size ? 0 : min(len, size - offset).
 *   GETATTR  n = size.
 *   SETATTR  offset carries the new size s; len and data are ignored (but len > 128 is EINVAL, first).
 *            After the EINVAL and ENOENT checks: s > B: some = 0, n = NRG_MEMFS_EFBIG, nothing changes.
 *            Else some = 1, n = s (Attr: the size), data zero; size = s. Bytes [s, old size) are gone;
 *            where s is above the old size the new bytes read as zero.
 * CAPACITY GROWTH (the file system behind memfs.rs keeps a file's bytes in a growing vector). Without it a
 * file holds B bytes for its whole life; capacity growth past B is off unless sizes are enabled and nrg_set_max_capacity gave the context a bound of max bytes per file: then WRITE
 * is valid exactly when offset + len <= max and SETATTR when s <= max, and B grows to hold what is
 * admitted; "File store: capacity growth" below. Without a bound everything above holds as it stands.
 * Out of scope: directories, names, inode creation and removal, rename; the SetAttrRequest fields other
 * than the size; the combiner and key-partitioned group rounds (nrg_group_partitioned_round*) for this
 * kind (NRG_E_INVAL from their entry points). A group of file stores is partitioned by FILE instead, as
 * benches/nrfs.rs runs it: nrg_group_file_round below.
 * A write of more than 128 bytes (benches/nrfs.rs's whole-file FileWrite) is a contiguous run of these
 * records: nrg_memfs_pwrite* below cut it on the device. */
#define NRG_MEMFS_WRITE 0u   /* OperationWr::Write{ino, offset, data[0..len)}  memfs.rs:66-72  */
#define NRG_MEMFS_READ 1u    /* OperationWr::Read{ino, offset, size = len}      memfs.rs:73-78  */
#define NRG_MEMFS_GETATTR 2u /* OperationWr::GetAttr{ino}: n = B, or the size    memfs.rs:27-29  */
#define NRG_MEMFS_SETATTR 3u /* OperationWr::SetAttr{ino, size = offset}; sized contexts only  memfs.rs:30-33 */
#define NRG_MEMFS_FIRST_INO 5u /* the ino of the benchmark's file                memfs.rs:117-119 */
#define NRG_MEMFS_ENOENT 1u
#define NRG_MEMFS_EFBIG 2u
#define NRG_MEMFS_EINVAL 3u
typedef struct {
    uint64_t ino;
    uint64_t offset;
    uint32_t op;
    uint32_t len;
    uint8_t data[128];
} nrg_memfs_op; /* 152 B */
typedef struct {
    uint64_t n;
    uint8_t data[128];
} nrg_memfs_resp; /* 136 B */

/* Synthetic ReadOperation::ReadOnly(tid, rnd1, rnd2)     benches/synthetic.rs:28-31       */
typedef struct {
    uint64_t tid;
    uint64_t r1;
    uint64_t r2;
} nrg_synth_rd;

/* ---- configuration ------------------------------------------------------------------ */
typedef struct {
    uint32_t ds_kind;         /* NRG_DS_*                                                  */
    uint32_t log2_slots;      /* hashmap: table has 2^log2_slots 32-B slots {key, value, two
                                 round stamps} (default 26: 2 GiB of HBM; < 2^30 slots);
                                 vspace (the field is reused): the pool holds 2^log2_slots page
                                 tables of 4 KiB (default 18: 1 GiB; 2 .. 22, else nrg_open
                                 returns NRG_E_INVAL); skip list (reused again): the map holds
                                 up to 2^log2_slots keys at open (default 24: 512 MiB for the two
                                 buffers of keys and values; 4 .. 28, else NRG_E_INVAL); file
                                 store (reused again): log2 of a file's bytes B (default 12, the
                                 4096-byte file of benches/memfs.rs:112-121; 7 .. 26, else
                                 NRG_E_INVAL) */
    uint64_t log_bytes;       /* Log::new(bytes): ring entries = bytes/64 rounded as in the
                                 reference (min 2*GC_FROM_HEAD, power of two). 0 = 32 MiB   */
    uint64_t max_batch;       /* largest number of log records replayed per kernel pass;
                                 larger exec ranges are replayed in order, in chunks
                                 (< 2^30; stack, queue, skip list: <= 2^24; vspace: <= 2^16, its
                                 default) */
    uint64_t max_reads;       /* largest read batch per call                               */
    uint64_t stack_capacity;  /* stack: maximum number of elements (< 2^31) at nrg_open;
                                 nrg_stack_reserve and nrg_set_max_capacity raise it later     */
    uint64_t synth_n;         /* synthetic: number of words (default 200000)               */
    uint32_t synth_cold_reads, synth_cold_writes, synth_hot_reads, synth_hot_writes; /* 20,5,2,1 */
    uint32_t stack_push_resp; /* 0: Push -> None (benches/stack.rs:77-80, nr/examples/stack.rs:70-73)
                                 1: Push -> Some(v) (nr/tests/stack.rs:89-92)               */
    uint32_t replica_id;      /* this replica's id (Log::register, ids start at 1)         */
    uint32_t pipeline;        /* opt-in (default 0). 0: every output of an *_async call is
                                 ordered on the context's stream. 1: the tail of a replay round
                                 rides in the next round's launch -- hashmap: the apply + reads;
                                 stack: the Pops answered from earlier tiles and the commit;
                                 synthetic: the per-op sums and the hot-word fold; queue: accepted,
                                 but nothing is deferred: a queue's outputs are always complete
                                 in stream order; vspace, skip list: the same. Those outputs
                                 (and the buffers they read) are complete only after nrg_join(),
                                 the next round call on this context (an empty one included), or
                                 nrg_sync(); give back-to-back rounds distinct response buffers.
                                 Synchronous calls are unaffected (their outputs are complete on
                                 return). */
    uint32_t hashmap_max_log2_slots; /* hashmap: 0 (default) = a fixed table of 2^log2_slots slots
                                 (NRG_E_TABLE_FULL when it fills). Otherwise the table grows by
                                 itself, as HashMap<u64, u64> does (nr/examples/hashmap.rs starts
                                 from an empty map; benches/hashmap.rs:91-100 only pre-sizes it),
                                 up to 2^hashmap_max_log2_slots slots: before a replay chunk or a
                                 prefill could take it past one key per two slots it is rehashed,
                                 synchronously, into the smallest table that holds the keys.
                                 log2_slots <= hashmap_max_log2_slots <= 30, else nrg_open returns
                                 NRG_E_INVAL. Answers, nrg_hashmap_size / dump / digest do not
                                 depend on the table's size; replicas replaying the same log with
                                 the same config grow at the same record. (The field takes what
                                 was padding in front of queue_capacity: no offset and not the
                                 struct's size changed, and nrg_config_default always zeroed it.) */
    uint64_t queue_capacity;  /* queue: maximum number of elements (default 2^24; 1 .. 2^32,
                                 else nrg_open returns NRG_E_INVAL; the queue's ring holds a
                                 power of two >= queue_capacity + max_batch u64); file store (the
                                 field is reused): the number of files F (default 1; 1 .. 2^16
                                 and F * B <= 2^29, else NRG_E_INVAL; its max_batch <= 2^20) */
} nrg_config;

/* Fill `cfg` with the defaults of the reference benches for `ds_kind`. */
void nrg_config_default(nrg_config* cfg, uint32_t ds_kind);

typedef struct nrg_ctx nrg_ctx;

/* Replica::new(&log): allocate the replica (data structure + ring + scratch) on device
 * `hip_device`; the data structure starts empty (NrHashMap/Stack) or initialised to
 * storage[i] = i (synthetic, benches/synthetic.rs:97-100). */
int nrg_open(int hip_device, const nrg_config* cfg, nrg_ctx** out);
int nrg_close(nrg_ctx* ctx);

/* Use `hip_stream` (a hipStream_t; NULL is the device's null stream, as in HIP) for all
 * further work on this context. A new context works on a non-blocking stream of its own,
 * returned by nrg_own_stream. Work on a caller's stream is ordered with the caller's other
 * work on it; the own stream is NOT ordered with the null stream. */
int nrg_set_stream(nrg_ctx* ctx, void* hip_stream);
void* nrg_get_stream(nrg_ctx* ctx);
void* nrg_own_stream(nrg_ctx* ctx);

/* Replica::sync analogue: wait for all queued work; report latched device errors. */
int nrg_sync(nrg_ctx* ctx);
/* Order outstanding side-stream reads (config.pipeline = 1) on the context's stream without
 * blocking the host; a no-op when nothing is outstanding. */
int nrg_join(nrg_ctx* ctx);

/* Automatic growth of the stack, the queue and the skip list, as Vec<u32> grows under push (benches/stack.rs:36-84)
 * and SegQueue never refuses one (benches/lockfree_comparisons.rs:75-101). max_items = 0, the state
 * after nrg_open, is a fixed capacity (config.stack_capacity / queue_capacity). With a bound, before
 * a replay chunk of n records could take the length past the capacity the structure is reallocated,
 * synchronously, to at least twice the capacity and at least length + n elements, clipped to
 * max_items; only past max_items does a replay latch NRG_E_CAPACITY, as a fixed structure does at its
 * capacity. The length is tracked on the host as an upper bound (exact when last read, plus every
 * record replayed since): a chunk whose bound stays within the capacity costs one comparison, and a
 * balanced Push/Pop stream re-reads its length now and then but never reallocates. Growth happens
 * inside the round call, so it works under a combiner and in a replica group (set the bound on
 * every member's replica); replicas that replay the same log in the same chunks with the same bound
 * grow at the same record, and nothing observable depends on the capacity except where
 * NRG_E_CAPACITY would appear. With a bound, nrg_restore (and nrg_group_resync) accept an image of
 * up to max_items items and grow first. The config is not involved: nrg_config's size and offsets
 * are ABI. The skip list (a SkipMap allocates a node per key) takes the bound in keys: the host keeps
 * len_ub, the exact key count when last read plus every record replayed or prefilled since, and before
 * a chunk could pass the capacity the exact count is read and the runs are reallocated, clipped to the
 * bound (<= 2^28). The file store takes the bound in BYTES PER FILE and grows by what the admitted records
 * need, a pure function of the log prefix: "File store: capacity growth" below. NRG_E_INVAL: a hashmap (it has config.hashmap_max_log2_slots), a synthetic or a vspace
 * context; a nonzero bound below the current capacity or above the kind's nrg_open bound (stack
 * < 2^31, queue <= 2^32). NRG_E_NOMEM from a round call: the larger buffer could not be allocated;
 * nothing of the chunk was launched and the replica is unchanged. Synchronous; like every direct
 * call, not allowed while a combiner is open on the context. */
int nrg_set_max_capacity(nrg_ctx* ctx, uint64_t max_items);

/* Replica::verify (nr/src/replica.rs:443-467) without the state leaving the GPU: a digest of the
 * replica's data structure, the same definition for every kind. out = {count, sum, xor} over the
 * structure's items of h = mix64(k ^ mix64(v)) (mix64: the splitmix64 finaliser; the sum wraps in
 * u64), with (k, v) per kind:
 *   hashmap    (key, value)                                  (= nrg_hashmap_digest)
 *   stack      (index from the bottom, the u32 element zero-extended)
 *   queue      (index from the front, the element): the logical position, not the ring slot
 *   synthetic  (word index, the word); count = synth_n
 *   vspace     (the leaf's first virtual address as nrg_vspace_dump reports it, the leaf entry),
 *              4 KiB and 2 MiB leaves alike; inner entries contribute nothing
 *   skip list  (key, value), the hashmap's definition: a skip list and a hashmap that replayed the
 *              same Puts hold equal triples
 *   file store (file index << 32 | word index, the word) for every aligned 8-byte little-endian
 *              word of every file; count = F * B / 8
 * An empty structure gives {0, 0, 0}; the triple depends on the contents alone, not on the table's
 * size, the ring position or the order in which page tables were allocated. Two replicas that
 * replayed the same log hold equal triples; nrgpu/digest.py computes the triple from a host
 * snapshot or a CPU model. Both calls first launch what the last chunk deferred
 * (config.pipeline = 1) and digest the state replayed so far: they do not need ltail == tail.
 * Like the dumps and every direct call, they are not allowed while a combiner is open on the
 * context. nrg_digest_async takes a device pointer to three u64, is ordered on the context's
 * stream and makes no host round trip; the page table's first digest allocates 8 B per pool table
 * of scratch. */
int nrg_digest(nrg_ctx* ctx, uint64_t out[3]);
int nrg_digest_async(nrg_ctx* ctx, uint64_t* d_out3);

/* ---- snapshot and restore ---------------------------------------------------------------
 * Replica::new (nr/src/replica.rs:184-232) gives a replica that replays the log from index 0, and
 * Replica::verify (:443-467) is the reference's only view of a replica's state. A snapshot is a
 * compact image of that state whose size depends on the contents, not on the table, ring or pool
 * that holds them; nrg_restore builds a replica from one, so a replica can join a log that was
 * garbage-collected, a diverged group member can be brought back (nrg_group_resync), and a
 * structure outlives its context. The image is one buffer, the same on the device, on the host
 * and on disk: a 64-byte header of eight little-endian u64 words, then the payload.
 *   word 0     magic, the ASCII bytes "NRGSNAP1"
 *   word 1     ds_kind in the low 32 bits, the format version (1) in the high 32
 *   word 2     items
 *   word 3     bytes = 64 + payload, rounded up to a multiple of 64 (the padding is zero)
 *   word 4     log_idx: the source's ltail; the state is the replay of [0, log_idx)
 *   words 5-7  the nrg_digest triple {count, sum, xor} of the state
 * Payload by kind:
 *   hashmap    items records of nrg_put layout {key, value}, in any order, the key 2^64 - 1 among them
 *   stack      items u32 elements, bottom first
 *   queue      items u64 elements, front first: the logical order, not the ring's
 *   synthetic  items = synth_n u64 words
 *   vspace     items = the tables allocated (nrg_vspace_tables), 4 KiB each: the pool image, inner
 *              entries as stored (table_index * 4096 | flags). The indices point into the image
 *              itself, so it restores into any pool of at least that many tables.
 *   skip list  items records of nrg_put layout {key, value} in strictly ascending key order;
 *              nrg_restore checks the order on the device (NRG_E_INVAL) before the digest
 *              comparison, and accepts items up to the capacity, or up to the growth bound
 *              (nrg_set_max_capacity), growing first; more is NRG_E_CAPACITY
 *   file store items = F * B / 8 words: the files' bytes in inode order. nrg_restore takes an image
 *              only into a context of the same F and B, NRG_E_INVAL otherwise: another total is
 *              refused with nothing touched; an equal total cut into other files fails the digest
 *              comparison (the items' keys carry the file) and leaves the files as at open
 * Two replicas with equal state need not produce byte-equal images: the hashmap's record order and
 * the page table's table numbering depend on how the state came about. Their digest words are
 * equal. Like the dumps and every direct call, none of these calls is allowed while a combiner is
 * open on the context. */
typedef struct {
    uint32_t ds_kind, version;
    uint64_t items, bytes, log_idx;
    uint64_t digest[3];
} nrg_snapshot_info;

/* What a snapshot taken now would hold (Replica::verify's view, sized): launches what the last
 * chunk deferred, waits for the stream and reads the exact item count from the device (the
 * hashmap's key count as nrg_hashmap_size takes it, the stack's and the queue's length, the page
 * table's tables). Fills kind, version, items, bytes and log_idx; digest is zero. Synchronous. */
int nrg_snapshot_size(nrg_ctx* ctx, nrg_snapshot_info* out);
/* Replica::verify's view as an image in device memory `d_buf` (16-B aligned) of `cap` bytes:
 * launches what the last chunk deferred, writes header and payload and runs the kind's digest
 * straight into header words 5-7. Stream ordered, no host round trip; like the digest it does not
 * need ltail == tail and snapshots what has been replayed. Nothing is stored at or past
 * d_buf + cap: a state that does not fit leaves magic = 0 (when cap >= 64) and latches
 * NRG_E_CAPACITY for the next nrg_sync. */
int nrg_snapshot_async(nrg_ctx* ctx, void* d_buf, uint64_t cap);
/* The header of the image at device pointer `d_buf`, of which the caller holds `bytes` bytes,
 * copied to the host and validated: magic, version, a known kind, `bytes` in the header equal to
 * what `items` items of the kind take and at most the argument. NRG_E_INVAL otherwise. */
int nrg_snapshot_info_read(nrg_ctx* ctx, const void* d_buf, uint64_t bytes, nrg_snapshot_info* out);
/* Replica::new from a state instead of from log index 0: replace the replica's contents with the
 * image's. `d_buf` (16-B aligned) is any device pointer the context's device can read, complete
 * when the call is made. Synchronous. In order:
 *   1  the header is validated as nrg_snapshot_info_read validates it (NRG_E_INVAL);
 *   2  and checked against the context: another kind, or a synthetic image of another synth_n,
 *      NRG_E_INVAL; more stack or queue elements than stack_capacity / queue_capacity, or more
 *      tables than the pool holds, NRG_E_CAPACITY; more keys than a fixed table has slots, or
 *      than a table of 2^hashmap_max_log2_slots slots holds at one key per two slots,
 *      NRG_E_TABLE_FULL. A failure up to here leaves the replica and its log untouched;
 *   3  queued work completes, deferred work included, and the device error latch is cleared;
 *   4  the contents are replaced and the bookkeeping a replay would have left is rebuilt (the
 *      hashmap's key count, stamps and epochs, with growth on a table sized for `items` keys as a
 *      replay would have sized it; the queue's front at ring position 0; the pool beyond the
 *      image zeroed), so that dumps, sizes, reads and the responses of every later round are
 *      those of a replica that replayed the log. The destination's table, ring and pool sizes
 *      may differ from the source's;
 *   5  head = tail = ctail = ltail = log_idx and no origin runs: the next append returns log_idx;
 *   6  the digest of the rebuilt state is compared with the header's. A mismatch (a corrupted
 *      payload; also a fixed table that took items <= slots but whose probe overran) returns
 *      NRG_E_INVAL and leaves unspecified contents: restore again, or close the context. */
int nrg_restore(nrg_ctx* ctx, const void* d_buf, uint64_t bytes);

const char* nrg_strerror(int code);
/* Library build identifier ("nrgpu <version> gfx950"). */
const char* nrg_version(void);
/* Number of visible HIP devices (0 on a host without GPUs; never fails). */
int nrg_device_count(void);

/* ---- Log ------------------------------------------------------------------------------ */
typedef struct {
    uint64_t size;   /* ring entries (power of two)                        */
    uint64_t head;   /* oldest live logical index (GC boundary)            */
    uint64_t tail;   /* next logical index to be appended                  */
    uint64_t ctail;  /* completed tail (max replayed tail)                 */
    uint64_t ltail;  /* this replica's replay epoch (ltails[idx-1])        */
    uint32_t replica_id;
    uint32_t ds_kind;
} nrg_log_info;

/* Log::append(ops, idx): append `n` host records (layout per ds kind) with origin replica
 * `origin`; returns the logical index of the first record. When fewer than GC_FROM_HEAD
 * entries would remain, the replica first replays what it has not replayed (as append's
 * GC path calls exec, nr/src/log.rs:364-387) and advances head to its ltail. */
int nrg_log_append(nrg_ctx* ctx, const void* recs, uint64_t n, uint32_t origin, uint64_t* first_idx);
/* Same, with `d_recs` a device pointer (stream ordered). */
int nrg_log_append_async(nrg_ctx* ctx, const void* d_recs, uint64_t n, uint32_t origin,
                         uint64_t* first_idx);
/* Append `nseg` device segments (e.g. the output of an all-gather of per-GPU write
 * segments): segment s starts at d_base + s*seg_stride records, holds lens[s] records and
 * has origin origins[s]. Segments are appended in order s = 0..nseg-1, which is the global
 * log order of the round. `first_idx[s]` receives each segment's first log index. */
int nrg_log_append_segments_async(nrg_ctx* ctx, const void* d_base, uint32_t nseg,
                                  uint64_t seg_stride, const uint64_t* lens,
                                  const uint32_t* origins, uint64_t* first_idx);

/* Log::exec(idx, dispatch_mut): replay [ltail, tail) into the replica in log order.
 * Responses for log indices in [resp_lo, resp_hi) are written densely:
 *   hashmap  : resp[u64] = previous value, some[u8] = 1 iff the key existed
 *              (HashMap::insert's return, nr/examples/hashmap.rs:46-50)
 *   stack    : resp[u32] = popped (or pushed, if stack_push_resp) value, some[u8]
 *   synthetic: resp[u64] = ReadWrite sum (WriteOnly -> 0), some = 1
 *   queue    : resp[u64] = pushed (Push -> Some(v)) or popped value, some[u8] = 0 for a Pop on
 *              an empty queue (benches/lockfree_comparisons.rs:94-98)
 *   vspace   : resp[nrg_vspace_resp] (16 B), some[u8] = 1 for Ok, 0 for Err (a = at)
 *   skip list: resp[u64] = the key, some[u8] = 1 (Ok(Some(key)), benches/lockfree_partitioned.rs:108-111);
 *              it does not depend on the state: SkipMap::insert replaces the value of a present key
 * `resp`/`some` may be NULL (no responses wanted, as benches/hashmap.rs:114-119 returns
 * Ok(None)); the hashmap then skips the previous-value pipeline entirely. */
int nrg_log_exec(nrg_ctx* ctx, uint64_t resp_lo, uint64_t resp_hi, void* resp, uint8_t* some);
int nrg_log_exec_async(nrg_ctx* ctx, uint64_t resp_lo, uint64_t resp_hi, void* d_resp,
                       uint8_t* d_some);

int nrg_log_state(const nrg_ctx* ctx, nrg_log_info* out);
/* Log::reset: head = tail = ctail = ltail = 0; the data structure is left untouched. */
int nrg_log_reset(nrg_ctx* ctx);

/* ---- NrHashMap ----------------------------------------------------------------------- */
/* Dispatch::dispatch(Get(k)) for a batch, after sync-to-tail (NRG_E_NOT_SYNCED if the
 * replica has unreplayed log entries): vals[i] = value or 0, found[i] = 1 iff present. */
int nrg_hashmap_get(nrg_ctx* ctx, const uint64_t* keys, uint64_t n, uint64_t* vals, uint8_t* found);
int nrg_hashmap_get_async(nrg_ctx* ctx, const uint64_t* d_keys, uint64_t n, uint64_t* d_vals,
                          uint8_t* d_found);

/* Replica::combine for a single-GPU replica, fused: append the W device records `d_puts`
 * with origin `origin`, replay everything up to the new tail, then answer the R reads
 * `d_get_keys` against the post-replay state. Previous-value responses for the appended
 * puts go to d_prev/d_prev_found if non-NULL. */
int nrg_hashmap_round_async(nrg_ctx* ctx, const nrg_put* d_puts, uint64_t W, uint32_t origin,
                            const uint64_t* d_get_keys, uint64_t R, uint64_t* d_get_vals,
                            uint8_t* d_get_found, uint64_t* d_prev, uint8_t* d_prev_found);

/* Multi-GPU round on one replica: the write segments of every replica (e.g. the output of
 * an RCCL all-gather, segment s at d_base + s*seg_stride records, lens[s] records, origin
 * origins[s]) are appended in order s = 0..nseg-1 (the round's global log order), the log is
 * replayed, and the R local reads are answered against the post-round state. Previous-value
 * responses are produced for segment `resp_seg` (this replica's own writes) if d_prev is
 * non-NULL. When every segment but the last is full (lens[s] == seg_stride) the gathered
 * buffer is replayed in place and the log copy is written by the replay itself. */
int nrg_hashmap_round_segments_async(nrg_ctx* ctx, const nrg_put* d_base, uint32_t nseg,
                                     uint64_t seg_stride, const uint64_t* lens,
                                     const uint32_t* origins, uint32_t resp_seg,
                                     const uint64_t* d_get_keys, uint64_t R, uint64_t* d_get_vals,
                                     uint8_t* d_get_found, uint64_t* d_prev, uint8_t* d_prev_found);

/* NrHashMap::default(): insert (keys[i], vals[i]) directly (no log traffic). */
int nrg_hashmap_prefill(nrg_ctx* ctx, const uint64_t* keys, const uint64_t* vals, uint64_t n);
/* Generated on device: keys k = 0..n-1 -> k + val_offset (benches/hashmap.rs:91-100 uses
 * n = INITIAL_CAPACITY, val_offset = 1). */
int nrg_hashmap_prefill_range(nrg_ctx* ctx, uint64_t n, uint64_t val_offset);
int nrg_hashmap_size(nrg_ctx* ctx, uint64_t* n);
/* HashMap::reserve / with_capacity (benches/hashmap.rs:91-100 pre-sizes the map;
 * nr/examples/hashmap.rs lets it grow): make the table large enough for `n_keys` keys in all at
 * one key per two slots, with automatic growth (config.hashmap_max_log2_slots) on or off. It never
 * shrinks: a request the table already satisfies returns NRG_OK and does nothing. Automatic
 * growth stays bounded by the config; a table reserved beyond that bound is a fixed one.
 * NRG_E_INVAL: not a hashmap, or more keys than nrg_open's largest table (2^30 slots) holds.
 * NRG_E_NOMEM: the new table could not be allocated; the old one is intact and the replica
 * usable. Synchronous (one rehash of the whole table); like every direct call, not allowed while
 * a combiner is open on the context. */
int nrg_hashmap_reserve(nrg_ctx* ctx, uint64_t n_keys);
/* The current table size: *log2_slots. */
int nrg_hashmap_capacity(nrg_ctx* ctx, uint32_t* log2_slots);
/* Copy out every (key, value) pair (unordered). `*n` receives the number of pairs; if it
 * exceeds `cap`, nothing is copied and NRG_E_CAPACITY is returned. */
int nrg_hashmap_dump(nrg_ctx* ctx, uint64_t* keys, uint64_t* vals, uint64_t cap, uint64_t* n);
/* Order-independent digest of the contents: count, sum and xor of mix64(k ^ mix64(v)). */
int nrg_hashmap_digest(nrg_ctx* ctx, uint64_t out[3]);
/* Removal of keys (std::collections::HashMap::remove, the container behind NrHashMap,
 * benches/hashmap.rs:77-79: the previous value or None, and the key is absent afterwards; the
 * reference's OpWr has no Remove). A record is {key, val} with both fields spanning all of u64, so the
 * context opts in, as nrg_skiplist_enable_removal does:
 * From here on a record whose val == tombstone is Remove(key); every other record is Put as before.
 * Synchronous, no way back; it flushes the deferred half. NRG_E_NOT_SYNCED while ltail < tail. Calling
 * it again with the same tombstone is NRG_OK; with another one NRG_E_INVAL. NRG_E_INVAL also for a
 * context that is not a hashmap, while a combiner is open on it, and if any present value equals the
 * tombstone (one scan of the table before anything changes: the replica stays as it was). Replicas of
 * one log, and every member of a group, enable it at the same log index with the same tombstone. A
 * context that never calls it behaves as before in every respect ({k, 2^64 - 1} is an ordinary Put
 * there) and launches the same kernels.
 *   Responses go where previous values go, in log order, one op at a time: Put(k, v) and Remove(k) both
 * answer (the previous value, 1) if k was present at that log position, else (0, 0). The answer depends
 * on the records before it, also those of the same chunk: Put(k, v), Remove(k) answers v; Remove(k),
 * Remove(k) answers Some, then None; Remove(k), Put(k, v) answers Some, then None.
 *   A Remove is an ordinary 16-byte record: nrg_log_append* / nrg_log_exec*, nrg_hashmap_round_async,
 * nrg_hashmap_round_segments_async, nrg_group_round_async, nrg_group_resync and the partitioned rounds
 * (nrg_group_partitioned_round*: the owner replays it and its answer travels as a previous value) carry
 * it unchanged. nrg_hashmap_prefill* with a tombstone value returns NRG_E_INVAL. nrg_combiner_open
 * on an enabled context returns NRG_E_INVAL.
 *   A removed key keeps its slot, marked dead, until a rehash (growth, or a purge) drops it; a later
 * Put of the key revives the slot. nrg_hashmap_size, Gets, dump, digest, snapshots and group verify
 * see live keys only, and none of them depends on when a replica grew or purged. Dead slots count
 * against the table: nrg_hashmap_occupancy is what the load limit and NRG_E_TABLE_FULL see. With
 * automatic growth the replay purges or grows by itself; a fixed table (or one at its maximum) needs
 * nrg_hashmap_purge before its dead slots fill it (DESIGN.md "NrHashMap", Removal).
 *   Every write round of an enabled context takes one schedule (the previous-value partition round),
 * whatever NRG_KNOB_PART / _SMALL_MAX / _STAMP_MAX say.
 *   A snapshot holds live pairs only and does not record the setting: a context restored from an
 * image, or resynced, keeps its own. nrg_restore of an image that holds the tombstone as a value into
 * an enabled context returns NRG_E_INVAL, the replica unchanged. */
int nrg_hashmap_enable_removal(nrg_ctx* ctx, uint64_t tombstone);
/* Query, no device touched: *enabled = 1 and *tombstone once removal is on, else 0 and 0 (either
 * pointer may be NULL). */
int nrg_hashmap_removal(nrg_ctx* ctx, uint64_t* tombstone, int* enabled);
/* Slots taken: live keys plus dead slots (nrg_hashmap_size is the live keys). Without removal the two
 * are equal. */
int nrg_hashmap_occupancy(nrg_ctx* ctx, uint64_t* slots_taken);
/* Drop the dead slots: a rehash into a fresh table of the same size, synchronous, under the rules of
 * nrg_hashmap_reserve (NRG_E_NOMEM: the old table is intact). NRG_OK and nothing launched when there
 * are no dead slots or removal is off. */
int nrg_hashmap_purge(nrg_ctx* ctx);

/* ---- Flat combining on the host ---------------------------------------------------------- */
/* Replica's flat combiner for many client threads (nr/src/context.rs:88-194,
 * nr/src/replica.rs:345-356, 404-433, 483-497, 508-595), for the hashmap, the stack, the synthetic
 * structure and the queue (not the page table, the skip list or the file store: nrg_combiner_open
 * on a vspace, skip-list or memfs context returns NRG_E_INVAL):
 * each registered thread posts up to 32 ops (MAX_PENDING_OPS) per call into the open batch and
 * parks; the combiner's own thread seals the batch into ONE GPU round of `ctx` (its writes
 * appended and replayed in batch order, then its reads answered against the post-round state)
 * without waiting for the GPU, so the next batch fills while a round runs (a second round is put
 * in flight only for a batch of 512 ops or more unless NRG_KNOB_COMB_DEPTH fixes the depth).
 * Batches live in mapped pinned host memory that the round's kernels read and write directly.
 * Calls on one token are synchronous and must come from one thread at a time (a second call on
 * a token whose call is still in progress returns NRG_E_INVAL); while a combiner
 * is open, `ctx` is driven only through it, and no thread may be inside a call when it is closed.
 * Needs max_threads * 32 <= max_batch (and <= max_reads for the hashmap). */
typedef struct nrg_combiner nrg_combiner;
int nrg_combiner_open(nrg_ctx* ctx, uint32_t max_threads, nrg_combiner** out);
int nrg_combiner_close(nrg_combiner* comb);
/* Replica::register: a token 0..max_threads-1, or NRG_E_CAPACITY. */
int nrg_combiner_register(nrg_combiner* comb, uint32_t* token);
/* Replica::execute_mut for n <= 32 log records of the replica's kind (nrg_put / nrg_stack_op /
 * nrg_synth_op / nrg_queue_op): resp[i] / some[i] as nrg_log_exec gives them (u64 previous value,
 * u32 popped value, u64 sum, u64 pushed or popped value). */
int nrg_combiner_execute_mut(nrg_combiner* comb, uint32_t token, const void* recs, uint32_t n, void* resp,
                             uint8_t* some);
/* Replica::execute for n <= 32 reads: hashmap Get (u64 keys -> u64 value, found), stack Peek
 * (`reads` unused -> u32 top, some), synthetic ReadOnly (nrg_synth_rd -> u64 sum, some = 1), queue
 * Len (`reads` unused -> u64 length after the round, some = 1). */
int nrg_combiner_execute(nrg_combiner* comb, uint32_t token, const void* reads, uint32_t n, void* resp,
                         uint8_t* some);
/* NrHashMap conveniences: Put(keys[i], vals[i]) -> prev[i]/some[i] = HashMap::insert's previous
 * value; Get(keys[i]) -> vals[i]/found[i]. */
int nrg_combiner_put(nrg_combiner* comb, uint32_t token, const uint64_t* keys, const uint64_t* vals, uint32_t n,
                     uint64_t* prev, uint8_t* some);
int nrg_combiner_get(nrg_combiner* comb, uint32_t token, const uint64_t* keys, uint32_t n, uint64_t* vals,
                     uint8_t* found);
/* GPU rounds combined so far and the ops they carried. */
int nrg_combiner_stats(nrg_combiner* comb, uint64_t* rounds, uint64_t* ops);

/* ---- Stack --------------------------------------------------------------------------- */
/* Stack::default(): storage = vals[0..n) (bottom first). */
int nrg_stack_init(nrg_ctx* ctx, const uint32_t* vals, uint64_t n);
/* Vec::reserve / Vec::capacity (the reference's Stack is a Vec<u32>, benches/stack.rs:36-84): make
 * room for `n_elems` elements in all, with automatic growth (nrg_set_max_capacity) on or off. It
 * never shrinks: a request the stack already satisfies returns NRG_OK and does nothing; a stack
 * reserved beyond its growth bound is a fixed one. NRG_E_INVAL: not a stack, or n_elems >= 2^31
 * (nrg_open's bound). NRG_E_NOMEM: the new buffer could not be allocated; the old one is intact and
 * the replica usable. Synchronous (one copy of the elements); like every direct call, not allowed
 * while a combiner is open on the context. */
int nrg_stack_reserve(nrg_ctx* ctx, uint64_t n_elems);
/* The current capacity in elements: config.stack_capacity, or what growth made of it. */
int nrg_stack_capacity(nrg_ctx* ctx, uint64_t* n_elems);
/* Replica::combine for one stack batch (nr/src/replica.rs:544-595): Log::append of the n ops
 * in d_ops (device) with `origin`, then Log::exec, fused into one replay pass that writes the
 * log copy itself. Pop responses for these ops (d_pop_vals[i], d_some_bits[i]; nullable) as
 * nrg_log_exec_async gives them. Same result as nrg_log_append_async + nrg_log_exec_async. */
int nrg_stack_round_async(nrg_ctx* ctx, const nrg_stack_op* d_ops, uint64_t n, uint32_t origin,
                          uint32_t* d_pop_vals, uint8_t* d_some_bits);
/* Dispatch::dispatch(Peek) after sync: top of stack. */
int nrg_stack_peek(nrg_ctx* ctx, uint32_t* val, uint8_t* some);
int nrg_stack_len(nrg_ctx* ctx, uint64_t* n);
int nrg_stack_dump(nrg_ctx* ctx, uint32_t* vals, uint64_t cap, uint64_t* n);

/* ---- AbstractDataStructure (synthetic) ------------------------------------------------ */
/* Dispatch::dispatch(ReadOnly(tid, r1, r2)) for a batch, after sync. */
/* Replica::combine for one batch of AbstractDataStructure write ops (device buffer): Log::append
 * fused into the replay's first pass, then Log::exec; sums (responses) for these ops as
 * nrg_log_exec_async gives them (nullable). Same result as append + exec. */
int nrg_synth_round_async(nrg_ctx* ctx, const nrg_synth_op* d_ops, uint64_t n, uint32_t origin,
                          uint64_t* d_resp, uint8_t* d_some);
int nrg_synth_read(nrg_ctx* ctx, const nrg_synth_rd* ops, uint64_t n, uint64_t* sums);
int nrg_synth_read_async(nrg_ctx* ctx, const nrg_synth_rd* d_ops, uint64_t n, uint64_t* d_sums);
int nrg_synth_dump(nrg_ctx* ctx, uint64_t* words, uint64_t cap, uint64_t* n);

/* ---- FIFO queue (SegQueueWrapper) ------------------------------------------------------- */
/* The queue holds at most config.queue_capacity elements unless nrg_queue_reserve or automatic
 * growth (nrg_set_max_capacity) raised that; nrg_queue_capacity reads the current value. A replay
 * during which the length exceeds it latches NRG_E_CAPACITY once (reported by the next nrg_sync / synchronous call), as
 * the stack does; afterwards nrg_queue_len and nrg_queue_dump never report or copy more than
 * the capacity. */
/* SegQueueWrapper::default with caller values: the queue holds vals[0..n) (front first). */
int nrg_queue_init(nrg_ctx* ctx, const uint64_t* vals, uint64_t n);
/* SegQueueWrapper::default (benches/lockfree_comparisons.rs:80-88): values 0..n-1 pushed in
 * order, generated on the device. */
int nrg_queue_init_range(nrg_ctx* ctx, uint64_t n);
/* The reference's queue is a SegQueue, which allocates segments as it fills
 * (benches/lockfree_comparisons.rs:75-101); here, as Vec::reserve / Vec::capacity for the stack:
 * make room for `n_elems` elements in all. The ring is reallocated to the power of two at or above
 * n_elems + max_batch and the elements keep their ring positions modulo the new size. It never
 * shrinks: a request already satisfied returns NRG_OK and does nothing. NRG_E_INVAL: not a queue, or
 * n_elems > 2^32 (nrg_open's bound). NRG_E_NOMEM: the new ring could not be allocated; the old one
 * is intact and the replica usable. Synchronous; like every direct call, not allowed while a
 * combiner is open on the context. */
int nrg_queue_reserve(nrg_ctx* ctx, uint64_t n_elems);
/* The current capacity in elements: config.queue_capacity, or what growth made of it. */
int nrg_queue_capacity(nrg_ctx* ctx, uint64_t* n_elems);
/* Dispatch::dispatch(QueueRd::Len) (benches/lockfree_comparisons.rs:99): the length. */
int nrg_queue_len(nrg_ctx* ctx, uint64_t* n);
/* Copy out the elements, front first. `*n` receives their number; if it exceeds `cap`, nothing
 * is copied and NRG_E_CAPACITY is returned (as nrg_stack_dump). */
int nrg_queue_dump(nrg_ctx* ctx, uint64_t* vals, uint64_t cap, uint64_t* n);
/* Replica::combine for one queue batch (nr/src/replica.rs:544-595): Log::append of the n ops in
 * d_ops (device) with `origin`, then Log::exec, with the log copy written by the replay's first
 * pass. Responses for these ops (d_resp[i] u64, d_some[i]; nullable) as nrg_log_exec_async gives
 * them. Same result as nrg_log_append_async + nrg_log_exec_async. */
int nrg_queue_round_async(nrg_ctx* ctx, const nrg_queue_op* d_ops, uint64_t n, uint32_t origin,
                          uint64_t* d_resp, uint8_t* d_some);

/* ---- VSpace: the replicated x86-64 page table (VSpaceDispatcher) ---------------------------- */
/* The replica's tables live in a device pool of 2^config.log2_slots tables of 4 KiB (more after
 * nrg_vspace_reserve), zeroed at open; table 0 is the PML4, and an inner entry holds table_index * 4096 | P|RW|US where the
 * reference stores a heap pointer (nothing observable depends on it). A replay that needs more
 * tables than the pool holds latches NRG_E_CAPACITY once (reported by the next nrg_sync /
 * synchronous call): exactly the ops whose tables do not fit when their turn comes in log order
 * change nothing and answer some = 0 with a = vbase, b = 0; the ops after them go on, and the
 * replica keeps answering from what was written. The result is the same however the log is cut
 * into chunks. Replica groups and the log calls
 * take the kind as they take the others; there is no combiner and no partitioned mode for it. */
/* Replica::combine for one batch (nr/src/replica.rs:544-595) of Map / MapDevice ops
 * (benches/vspace.rs:513-525 dispatch_mut -> :469-481 map_new -> :177-381 map_generic):
 * Log::append of the n ops in d_ops (device) with `origin`, then Log::exec, with the log copy
 * written by the replay's first pass. Responses for these ops (d_resp[i], d_some[i]; nullable) as
 * nrg_log_exec_async gives them. Same result as nrg_log_append_async + nrg_log_exec_async. */
int nrg_vspace_round_async(nrg_ctx* ctx, const nrg_vspace_op* d_ops, uint64_t n, uint32_t origin,
                           nrg_vspace_resp* d_resp, uint8_t* d_some);
/* Dispatch::dispatch(Identify(vaddr)) for a batch (benches/vspace.rs:504-511 -> :436-467
 * resolve_addr), after sync-to-tail (NRG_E_NOT_SYNCED while ltail < tail; n <= max_reads, else
 * NRG_E_CAPACITY): paddrs[i] = the leaf's address plus the offset into its 4 KiB or 2 MiB page,
 * or 0 where nothing is mapped (found[i] = 0). Bits 48..63 of a vaddr are ignored, as the
 * reference's index functions ignore them. */
int nrg_vspace_resolve(nrg_ctx* ctx, const uint64_t* vaddrs, uint64_t n, uint64_t* paddrs, uint8_t* found);
int nrg_vspace_resolve_async(nrg_ctx* ctx, const uint64_t* d_vaddrs, uint64_t n, uint64_t* d_paddrs,
                             uint8_t* d_found);
/* Tables allocated so far, the PML4 included (VSpace::allocs.len() + 1, :384-404). */
int nrg_vspace_tables(nrg_ctx* ctx, uint64_t* n);
/* VSpace takes every page table from the heap (benches/vspace.rs:388-419 new_pt / new_pd / new_pdpt);
 * here the pool is made larger: room for `n_tables` tables in all, the allocated ones copied (inner
 * entries hold table indices, which stay valid) and the rest zeroed. It never shrinks: a request the
 * pool already satisfies returns NRG_OK and does nothing. There is no automatic growth for the page
 * table: the tables a chunk needs are only known on the device. NRG_E_INVAL: not a vspace, or
 * n_tables > 2^22 (nrg_open's bound). NRG_E_NOMEM: the new pool could not be allocated; the old one
 * is intact and the replica usable. Synchronous; nrg_restore accepts an image that fits the pool as
 * reserved. */
int nrg_vspace_reserve(nrg_ctx* ctx, uint64_t n_tables);
/* The tables the pool holds: 2^config.log2_slots, or what nrg_vspace_reserve made of it. */
int nrg_vspace_capacity(nrg_ctx* ctx, uint64_t* n_tables);
/* Replica::verify's view (nr/src/replica.rs:443-467): every leaf entry, one record each, in
 * ascending vaddr, whatever order the tables were allocated in. `*n` receives their number; if it
 * exceeds `cap`, nothing is copied and NRG_E_CAPACITY is returned (as nrg_queue_dump). */
int nrg_vspace_dump(nrg_ctx* ctx, nrg_vspace_leaf* leaves, uint64_t cap, uint64_t* n);

/* ---- Skip list: the replicated ordered map (SkipListWrapper over SkipMap<u64, u64>) -----------
 * benches/lockfree.rs:278-317 runs it as skiplist-partinput / skiplist-mlnr: writes OpWr::Push(k, v)
 * (:86-97), reads SkipListConcurrent::Get(k) (:73-84), a default of i -> i for i < INITIAL_CAPACITY
 * (benches/lockfree_partitioned.rs:88-96). Through Dispatch it is observably the hashmap, but
 * Replica::verify (nr/src/replica.rs:443-467) hands the caller the SkipMap itself, and what a SkipMap
 * has and a HashMap has not is order: front, back, lower_bound, upper_bound, range, iteration in key
 * order. The replica keeps two sorted runs with disjoint key sets; keys span all of u64.
 * The map holds at most 2^config.log2_slots keys unless nrg_skiplist_reserve or automatic growth
 * (nrg_set_max_capacity) raised that. Without a growth bound, a replay that would hold more distinct
 * keys than the capacity latches NRG_E_CAPACITY once (reported by the next nrg_sync / synchronous
 * call); the contents are unspecified from then on, but nrg_skiplist_len is at most the capacity:
 * restore or close. Replica groups and the log calls take the kind as they take the others; a
 * replicated group's round (nrg_group_round_async) answers a skip-list member's get_keys after its
 * replay, as it does a hashmap member's. The reference itself runs the skip list key-partitioned
 * (skiplist-mlnr, a cnr::Replica with several logs, benches/lockfree.rs:228-317, LogMapper::hash
 * :73-97): that is nrg_group_partitioned_round on a group of skip-list replicas, with
 * nrg_skiplist_prefill_partition and the group-wide ordered reads nrg_group_skiplist_seek /
 * nrg_group_skiplist_range_count / nrg_group_skiplist_scan (the cnr section below). Out of scope: there is no combiner
 * (nrg_combiner_open returns NRG_E_INVAL, as for the page table), and neither removal of keys nor
 * pop_front / pop_back in partitioned rounds unless the group agreed on it (nrg_skiplist_enable_removal
 * and nrg_skiplist_enable_pops below serve replicated groups and single replicas; a partitioned group
 * opts in as a whole with nrg_group_skiplist_enable_removal / nrg_group_skiplist_enable_pops and pops
 * with nrg_group_skiplist_pop, the cnr section below). Every call below returns NRG_E_INVAL on a context
 * of another kind. */
/* Replica::combine for one batch of Push(k, v) records (nr/src/replica.rs:544-595): Log::append of the
 * n records in d_ops (device) with `origin`, then Log::exec, with the log copy written by the
 * replay's first pass. Responses (d_resp[i] = the key, d_some[i] = 1; nullable) as nrg_log_exec_async
 * gives them. Same result as nrg_log_append_async + nrg_log_exec_async. */
int nrg_skiplist_round_async(nrg_ctx* ctx, const nrg_put* d_ops, uint64_t n, uint32_t origin, uint64_t* d_resp,
                             uint8_t* d_some);
/* Dispatch::dispatch(Get(k)) for a batch (benches/lockfree.rs:73-84), after sync-to-tail
 * (NRG_E_NOT_SYNCED while ltail < tail; n <= max_reads, else NRG_E_CAPACITY, as nrg_vspace_resolve):
 * vals[i] = value or 0, found[i] = 1 iff present. */
int nrg_skiplist_get(nrg_ctx* ctx, const uint64_t* keys, uint64_t n, uint64_t* vals, uint8_t* found);
int nrg_skiplist_get_async(nrg_ctx* ctx, const uint64_t* d_keys, uint64_t n, uint64_t* d_vals, uint8_t* d_found);
/* SkipMap::lower_bound / upper_bound for a batch, same rules as the Gets: the entry with the smallest
 * key >= k (GE: lower_bound(Included)) or > k (GT: lower_bound(Excluded)), or with the largest key
 * <= k (LE: upper_bound(Included)) or < k (LT: upper_bound(Excluded)). out_keys[i] / out_vals[i] = the
 * entry, found[i] = 1; none: 0, 0 and found[i] = 0. SkipMap::front is GE(0), back is LE(2^64 - 1);
 * GT(2^64 - 1) and LT(0) find nothing, as does every seek on an empty map. Another mode: NRG_E_INVAL. */
#define NRG_SEEK_GE 0u
#define NRG_SEEK_GT 1u
#define NRG_SEEK_LE 2u
#define NRG_SEEK_LT 3u
int nrg_skiplist_seek(nrg_ctx* ctx, const uint64_t* keys, uint64_t n, uint32_t mode, uint64_t* out_keys,
                      uint64_t* out_vals, uint8_t* found);
int nrg_skiplist_seek_async(nrg_ctx* ctx, const uint64_t* d_keys, uint64_t n, uint32_t mode, uint64_t* d_out_keys,
                            uint64_t* d_out_vals, uint8_t* d_found);
/* SkipMap::range from a bound, the first `limit` entries, for a batch: range(k..).take(limit) or
 * range(..=k).rev().take(limit), what a caller does with the SkipMap Replica::verify hands it
 * (nr/src/replica.rs:443-467); YCSB's SCAN. Same rules as the Gets (after sync-to-tail, else
 * NRG_E_NOT_SYNCED; n <= max_reads, else NRG_E_CAPACITY). mode is NRG_SEEK_*:
 *   GE / GT: ascending keys >= k / > k.
 *   LE / LT: DESCENDING keys <= k / < k.
 * Entry j of query i goes to out_keys[i*limit + j] / out_vals[i*limit + j], for j < counts[i];
 * counts[i] (u32) is the number of entries written, 0..limit: min(limit, the entries the map has in
 * the direction). Slots j >= counts[i] are NOT written. With limit = 1 the entry and counts[i] are
 * nrg_skiplist_seek's entry and found[i]. Paging: GT(the last key of a page) continues an ascending
 * walk, LT a descending one. NRG_E_INVAL: mode > NRG_SEEK_LT, limit = 0 or limit >
 * NRG_SCAN_MAX_LIMIT, or a NULL buffer with n > 0; n = 0 returns NRG_OK with nothing written. The
 * host-pointer form stages its answers on the device and returns NRG_E_CAPACITY when n * limit >
 * 2^24; it is synchronous, as the other host forms. One launch per batch ("sl_walk"): a group of
 * lanes per query, DESIGN.md "Skip list replay". */
#define NRG_SCAN_MAX_LIMIT 1024u
int nrg_skiplist_scan(nrg_ctx* ctx, const uint64_t* keys, uint64_t n, uint32_t mode, uint32_t limit,
                      uint64_t* out_keys, uint64_t* out_vals, uint32_t* counts);
int nrg_skiplist_scan_async(nrg_ctx* ctx, const uint64_t* d_keys, uint64_t n, uint32_t mode, uint32_t limit,
                            uint64_t* d_out_keys, uint64_t* d_out_vals, uint32_t* d_counts);
/* SkipMap::range(lo..=hi) into host buffers, ascending, both bounds inclusive (so the key 2^64 - 1 is
 * reachable), after sync-to-tail. `*n` receives the count; if it exceeds `cap`, nothing is copied and
 * NRG_E_CAPACITY is returned, as the dumps do. lo > hi gives *n = 0. */
int nrg_skiplist_range(nrg_ctx* ctx, uint64_t lo, uint64_t hi, uint64_t* keys, uint64_t* vals, uint64_t cap,
                       uint64_t* n);
/* counts[i] = the number of keys in [los[i], his[i]] (0 where lo > hi); the Gets' rules. */
int nrg_skiplist_range_count(nrg_ctx* ctx, const uint64_t* los, const uint64_t* his, uint64_t n, uint64_t* counts);
int nrg_skiplist_range_count_async(nrg_ctx* ctx, const uint64_t* d_los, const uint64_t* d_his, uint64_t n,
                                   uint64_t* d_counts);
/* Replica::verify's view (nr/src/replica.rs:443-467): the whole map in ascending key order. `*n`
 * receives the number of pairs; if it exceeds `cap`, nothing is copied and NRG_E_CAPACITY is returned. */
int nrg_skiplist_dump(nrg_ctx* ctx, uint64_t* keys, uint64_t* vals, uint64_t cap, uint64_t* n);
/* SkipMap::len: the number of keys. */
int nrg_skiplist_len(nrg_ctx* ctx, uint64_t* n);
/* SkipListWrapper::default with caller pairs: insert (keys[i], vals[i]) directly (host arrays, any
 * order, no log traffic); of several records with one key the last wins. */
int nrg_skiplist_prefill(nrg_ctx* ctx, const uint64_t* keys, const uint64_t* vals, uint64_t n);
/* Generated on the device: keys k = 0..n-1 -> k + val_offset. SkipListWrapper::default
 * (benches/lockfree_partitioned.rs:88-96) is n = INITIAL_CAPACITY, val_offset = 0. */
int nrg_skiplist_prefill_range(nrg_ctx* ctx, uint64_t n, uint64_t val_offset);
/* SkipListWrapper::default restricted to one partition: the keys k < n with
 * nrg_key_owner(k, parts) == part, values k + val_offset, generated on the device with no log
 * traffic (a member of a partitioned skip-list group: part = its rank, parts = the group's size).
 * NRG_E_INVAL: parts == 0, parts > NRG_MAX_PARTS or part >= parts. Synchronous; the keys count
 * towards automatic growth as nrg_skiplist_prefill_range's do. */
int nrg_skiplist_prefill_partition(nrg_ctx* ctx, uint64_t n, uint64_t val_offset, uint32_t part, uint32_t parts);
/* A SkipMap allocates a node per key; here, as Vec::reserve / Vec::capacity for the stack
 * (nrg_stack_reserve): make room for `n_keys` keys in all, with automatic growth
 * (nrg_set_max_capacity) on or off. It never shrinks: a request the map already satisfies returns
 * NRG_OK and does nothing; a map reserved beyond its growth bound is a fixed one. NRG_E_INVAL: not a
 * skip list, or n_keys > 2^28 (nrg_open's bound). NRG_E_NOMEM: the new buffers could not be
 * allocated; the old ones are intact and the replica usable. Synchronous (one copy of the base run). */
int nrg_skiplist_reserve(nrg_ctx* ctx, uint64_t n_keys);
/* The current capacity in keys: 2^config.log2_slots, or what growth made of it. */
int nrg_skiplist_capacity(nrg_ctx* ctx, uint64_t* n_keys);
/* Removal of keys (SkipMap::remove; the reference's SkipListWrapper has no such op, the SkipMap that
 * Replica::verify hands out has). A record is {key, val} with both fields spanning all of u64, so the
 * context opts in, as nrg_memfs_enable_sizes does:
 * From here on a record whose val == tombstone is Remove(key) (SkipMap::remove); every other record is
 * Push as before. Synchronous, no way back. NRG_E_NOT_SYNCED while ltail < tail. Calling it again with
 * the same tombstone is NRG_OK; with another one NRG_E_INVAL. Replicas of one log, and every member of a
 * group, enable it at the same log index with the same tombstone. A context that never calls it
 * behaves as before in every respect ({k, 2^64 - 1} is an ordinary Push there) and launches the same
 * kernels.
 *   Responses, in log order, one op at a time: Push(k, v) answers (k, some = 1), unchanged. Remove(k)
 * answers (the previous value, some = 1) if k was present at that log position, else (0, some = 0);
 * k is absent afterwards either way. The answer depends on the records before it, also those of the
 * same chunk: Push(k, v), Remove(k) answers v; Remove(k), Remove(k) answers Some, then None.
 *   A Remove is an ordinary 16-byte record: nrg_log_append* / nrg_log_exec*, nrg_skiplist_round_async,
 * the ring's wrap and GC, nrg_group_round_async and nrg_group_resync carry it unchanged. The
 * nrg_skiplist_prefill* calls run the same pipeline: on an enabled context a prefilled record whose
 * value is the tombstone is a Remove too. Partitioned rounds (nrg_group_partitioned_round*) return
 * NRG_E_INVAL when a member has removal enabled, unless the group agreed on it
 * (nrg_group_skiplist_enable_removal: a partitioned Push response is written by the asker from its own
 * records, which is wrong for a Remove; on such a group the owners answer): the round is dropped like
 * one with any other bad argument, nothing of it is written and no log moves; nrg_combiner_open stays
 * NRG_E_INVAL.
 *   Capacity: a chunk's new keys are admitted against the key count BEFORE the chunk's own removals
 * (a full map replaying Remove(a), Push(new b) in one chunk latches NRG_E_CAPACITY); the room a chunk
 * frees is there for the next chunk. The host's bounds (growth, compaction) stay upper bounds: on an
 * enabled context the host reads the exact counts back once per chunk (DESIGN.md "Skip list replay",
 * Removal), so they are then the counts themselves.
 *   A snapshot does not record the setting: a context restored from an image, or resynced, keeps its
 * own. */
int nrg_skiplist_enable_removal(nrg_ctx* ctx, uint64_t tombstone);
/* Query, no device touched: *enabled = 1 and *tombstone once removal is on, else 0 and 0 (either
 * pointer may be NULL). */
int nrg_skiplist_removal(nrg_ctx* ctx, uint64_t* tombstone, int* enabled);
/* SkipMap::pop_front / pop_back through the log, one or many at a time: what makes the ordered map a
 * priority queue or a work list. (seek + Remove is two records with a host round trip between them, and
 * another replica's record can land in between; a pop is one record, ordered by the log.) The context
 * opts in, under nrg_skiplist_enable_removal's rules: skip-list contexts only; synchronous, no way
 * back; NRG_E_NOT_SYNCED while ltail < tail; replicas of one log, and every member of a group, enable at
 * the same log index with the same marks; again with the same marks is NRG_OK, with others NRG_E_INVAL.
 * The two marks must differ from each other and from the tombstone, whichever of removal and pops is
 * enabled first: NRG_E_INVAL otherwise.
 *   From here on a record {key = n, val = front_mark} is PopFront x n and {key = n, val = back_mark} is
 * PopBack x n: pop_front() (pop_back()) called n times, n = 1 being the reference's call. It removes the
 * n smallest (largest) entries the map has at that log position, or all of them if it has fewer; n = 0
 * does nothing. Its response in the ordinary resp / some arrays is resp = m, the entries popped
 * (0 .. n), and some = (m >= 1): for n = 1 that is pop_front()'s Some / None. Only records are
 * interpreted: values already stored that equal a mark stay ordinary values, nothing is scanned when
 * pops are enabled, and the nrg_skiplist_prefill* calls, which take pairs and not records, insert a
 * mark as the value it is. A context that never enables runs exactly the kernels and launches of
 * before; its {k, mark} records are Pushes.
 *   A pop is an ordinary 16-byte record: nrg_log_append* / nrg_log_exec*, nrg_skiplist_round_async,
 * replicated group rounds and nrg_group_resync carry it and answer the counts; the popped entries
 * themselves are delivered only by the two calls below. Partitioned rounds return NRG_E_INVAL for a
 * member with pops enabled, unless the group agreed on it (nrg_group_skiplist_enable_pops; the front of
 * a key-partitioned map is a group-wide question: nrg_group_skiplist_pop), dropped like
 * a round with any other bad argument; nrg_combiner_open stays NRG_E_INVAL. Snapshot, restore, digest,
 * dump and every read are unchanged (the two runs stay dense), and an image does not record the setting.
 *   Cost: a pop depends on every record before it, so a chunk is cut at its pop records: each maximal
 * run of consecutive pop records is one pop step (one small launch and one 64-byte readback, whatever
 * the counts and the mix of ends), and the ordinary records between two runs replay as a chunk of
 * their own. A batch that alternates Push and Pop record by record therefore replays as one segment per
 * record: correct and slow. Group pops into runs where the order allows it, and prefer one PopFront x n
 * to n PopFront x 1 in different places (DESIGN.md "Skip list replay", Pops). An enabled context also
 * pays one small launch and a readback per chunk to find the pop records. */
int nrg_skiplist_enable_pops(nrg_ctx* ctx, uint64_t front_mark, uint64_t back_mark);
/* Query, no device touched: *enabled = 1 and the marks once pops are on, else 0, 0 and 0 (any pointer
 * may be NULL). */
int nrg_skiplist_pops(nrg_ctx* ctx, uint64_t* front_mark, uint64_t* back_mark, int* enabled);
/* nrg_skiplist_round_async on a context with pops enabled (NRG_E_INVAL otherwise, or with d_pop_n NULL,
 * or with pop_cap > 0 and an array NULL), which also hands out the entries the batch's pop records
 * popped (not those of records the round replays ahead of the batch): packed in record order, each
 * record's entries in the order popped (front: ascending keys, back: descending), so the offsets are the
 * exclusive scan of resp over the batch's pop records, the layout nrg_memfs_pread uses for bytes.
 * *d_pop_n = the total popped; only the first pop_cap entries are stored in d_pop_keys / d_pop_vals and
 * nothing is written past them: a caller whose pop_cap covers the sum of its records' counts loses
 * nothing. All pointers are device pointers; the arrays are written on the context's stream. */
int nrg_skiplist_round_pops_async(nrg_ctx* ctx, const nrg_put* d_ops, uint64_t n, uint32_t origin, uint64_t* d_resp,
                                  uint8_t* d_some, uint64_t* d_pop_keys, uint64_t* d_pop_vals, uint64_t pop_cap,
                                  uint64_t* d_pop_n);
/* One PopFront x n (back = 0) or PopBack x n record, synchronously, into host arrays: what the log
 * holds is replayed first, then the record is appended with `origin` and replayed; *m = the entries
 * popped, keys[0 .. m) / vals[0 .. m) the entries in the order popped. The arrays hold min(n,
 * nrg_skiplist_len) entries or more. NRG_E_INVAL before nrg_skiplist_enable_pops. */
int nrg_skiplist_pop(nrg_ctx* ctx, int back, uint64_t n, uint32_t origin, uint64_t* keys, uint64_t* vals, uint64_t* m);

/* ---- file store (kind NRG_DS_MEMFS; benches/memfs.rs) ---------------------------------------
 * NrMemFilesystem (benches/memfs.rs:106-192) behind Dispatch (:194-292) with ReadOperation = (): every
 * op, Read included, is a log record (nrg_memfs_op above), so the generic log calls carry the whole
 * structure: nrg_log_append* / nrg_log_exec* with records of 152 B and responses of 136 B, and
 * replicated group rounds (nrg_group_round_async). At nrg_open every byte of every file is 0x01
 * (memfs.rs:118). Every call below returns NRG_E_INVAL on a context of another kind, and every
 * other kind's calls return NRG_E_INVAL on this one; the key-partitioned rounds and nrg_combiner_open
 * return NRG_E_INVAL. File-partitioned group rounds: nrg_group_file_round. */
/* Replica::combine for one batch (memfs.rs:194-292 dispatch_mut per record, in order): append + exec
 * in one replay pass that also writes the log copy; responses of these n ops into d_resp / d_some
 * (both NULL: none wanted). d_ops and d_resp 8-byte aligned. n <= config.max_batch. */
int nrg_memfs_round_async(nrg_ctx* ctx, const nrg_memfs_op* d_ops, uint64_t n, uint32_t origin,
                          nrg_memfs_resp* d_resp, uint8_t* d_some);
/* NrMemFilesystem::default's memfs.write(ino, 0, 0, &[1; 4096], 0) (memfs.rs:112-121) with the
 * caller's bytes: set the first `len` bytes of file `ino` directly, no log traffic, before any
 * replay (replicas of one log must be given the same bytes). NRG_E_INVAL: an ino outside the range or
 * len > B. Synchronous. */
int nrg_memfs_init(nrg_ctx* ctx, uint64_t ino, const uint8_t* bytes, uint64_t len);
/* pread in the style of Replica::verify (nr/src/replica.rs:443-467; the benchmark's own Reads are log
 * records, memfs.rs:73-78): *n = min(len, B - offset) bytes of file `ino` from `offset` into buf (any
 * len; 0 where offset >= B). NRG_E_NOT_SYNCED while ltail < tail; NRG_E_INVAL: an ino outside the
 * range. Synchronous. */
int nrg_memfs_read(nrg_ctx* ctx, uint64_t ino, uint64_t offset, uint64_t len, uint8_t* buf, uint64_t* n);
/* Replica::verify's view of one file: *n = B, and its B bytes into buf when cap >= B
 * (NRG_E_CAPACITY otherwise). What has been replayed so far; does not need ltail == tail. */
int nrg_memfs_dump(nrg_ctx* ctx, uint64_t ino, uint8_t* buf, uint64_t cap, uint64_t* n);
/* F and B of the context (either pointer may be NULL). */
int nrg_memfs_geometry(nrg_ctx* ctx, uint64_t* files, uint64_t* file_bytes);
/* Replica::execute -> read_only (nr/src/replica.rs:404-410, :483-497) for a batch of reads: the
 * read-only file op of benches/nrfs.rs:16-18, :88-101 (OpRd::FileRead, a true ReadOperation that
 * copies the whole 4096-byte file), here POSIX pread of any length. Nothing is logged and nothing is
 * latched; the replica is not changed (digest and dumps are the same before and after). The reads
 * see everything already enqueued on the context's stream, as nrg_hashmap_get_async's do.
 *   request i: an ino outside the range gives some[i] = 0 and count_i = 0; otherwise some[i] = 1 and
 *              count_i = offset >= B ? 0 : min(len, B - offset). Any len up to 2^64 - 1 is legal.
 *   offs:      n + 1 words, offs[0] = 0, offs[i + 1] = offs[i] + count_i.
 *   data:      packed in request order: request i's bytes are data[offs[i] .. offs[i + 1]). A byte
 *              whose packed position is at or past cap is not written, and no byte of data at or
 *              past min(cap, offs[n]) is ever written.
 * The async call cannot know the total: the caller compares offs[n] with cap. The synchronous call
 * returns NRG_E_CAPACITY when offs[n] > cap, with offs and some complete and the first cap bytes
 * valid. n == 0 is NRG_OK and writes offs[0] = 0. NRG_E_NOT_SYNCED while ltail < tail;
 * n > config.max_reads: NRG_E_CAPACITY; NRG_E_INVAL: a reqs or offs pointer that is not 8-byte
 * aligned, or with n > 0 a NULL reqs, offs or some, or a NULL data with cap > 0. */
typedef struct {
    uint64_t ino, offset, len;
} nrg_memfs_rd; /* 24 B */
int nrg_memfs_pread_async(nrg_ctx* ctx, const nrg_memfs_rd* d_reqs, uint64_t n, uint8_t* d_data, uint64_t cap,
                          uint64_t* d_offs /* n + 1 */, uint8_t* d_some /* n */);
int nrg_memfs_pread(nrg_ctx* ctx, const nrg_memfs_rd* reqs, uint64_t n, uint8_t* data, uint64_t cap,
                    uint64_t* offs /* n + 1 */, uint8_t* some /* n */);
/* Logged writes of any length: POSIX pwrite, and benches/nrfs.rs:103-115 OpWr::FileWrite(fd), which is
 * memfs.write(fd, &write_buffer[fd - 1], 0) with a 4096-byte buffer. The record stays 152 bytes: a long
 * write is a contiguous run of ordinary WRITE records in the log, atomic against every other op because
 * a log has one appender and group rounds concatenate whole segments, and replayed by every replica
 * like any other records. Request i writes data[data_off, data_off + len) to file `ino` at `offset`;
 * data_off is explicit, so requests may share bytes (nrfs.rs writes one buffer to every file) and a
 * failing request needs none. THE CUT of request i, checked in the replay's order (F files of B bytes):
 *   ino outside the range     some = 0, written = NRG_MEMFS_ENOENT; one record {ino, offset, WRITE, len 0}
 *   !(offset <= B && len <= B - offset)   (no overflow: len may be 2^64 - 1) some = 0, written =
 *                             NRG_MEMFS_EFBIG, nothing changes: a Write that ends past the end fails
 *                             whole; one record {ino, offset B, WRITE, len 1, data zero}, which the replay
 *                             answers with EFBIG
 *   len == 0                  some = 1, written = 0; one record {ino, offset, WRITE, len 0}
 *   else                      some = 1, written = len; cut at the file's 128-byte line boundaries into
 *                             f_i = ((offset + len - 1) >> 7) - (offset >> 7) + 1 records, fragment k
 *                             (line_k = (offset >> 7) + k) covering
 *                             [max(offset, line_k * 128), min(offset + len, (line_k + 1) * 128))
 * Every request logs at least one record (a failed dispatch_mut is a log entry too). first[0..n] is the
 * running sum of the f_i and T = first[n] the records of the call; a record's data bytes past its len
 * are zero. A valid request with len > 0 whose data_off + len exceeds data_bytes (or overflows) is the
 * caller's error: NRG_E_INVAL from the whole call, nothing logged; a failing request's data_off is not
 * looked at. */
typedef struct {
    uint64_t ino, offset, len, data_off;
} nrg_memfs_wr; /* 32 B */
/* The cut as host arithmetic: no device is touched and no context is needed. first: n + 1 words;
 * written and some (n each) may be NULL. NRG_E_INVAL: a geometry nrg_open refuses (log2_b outside
 * 7 .. 26, files outside 1 .. 2^16, files << log2_b above 2^29), a NULL reqs or first with n > 0, or
 * the data_off rule above. */
int nrg_memfs_pwrite_plan(uint32_t log2_b, uint64_t files, const nrg_memfs_wr* reqs, uint64_t n, uint64_t data_bytes,
                          uint64_t* first /* n + 1 */, uint64_t* written /* n */, uint8_t* some /* n */);
/* Replica::combine for these writes. The requests are on the HOST (the log's tail is host state: T must
 * be known before anything is queued, the rule seg_lens follows) and may be reused on return; the data
 * is on the device. In order: the plan, catch-up on the log, then passes of at most log size - 8192
 * records until all T are done: room in the ring (Log::append's GC), the cut written straight into the
 * ring at the tail, the tail advanced, the pass replayed in chunks of max_batch with no responses
 * wanted. A call of any T succeeds on any ring, a request's fragments stay contiguous in the log
 * whatever chunks and passes they straddle, and everything is ordered on the context's stream.
 * d_written / d_some (both or neither): the answers above, n each. *n_records = T (nullable). Works on
 * sized contexts too: the records are ordinary Writes, so a pwrite past a file's size grows it and a
 * gap reads as zero. n == 0: NRG_OK, nothing logged. NRG_E_INVAL: a context of another kind, a NULL
 * reqs, a NULL d_data with data_bytes > 0, exactly one of d_written / d_some, or the plan's.
 * NRG_E_CAPACITY: n > config.max_batch (the uploads of the requests and first[] are sized by it). */
int nrg_memfs_pwrite_async(nrg_ctx* ctx, const nrg_memfs_wr* reqs, uint64_t n, const uint8_t* d_data,
                           uint64_t data_bytes, uint32_t origin, uint64_t* d_written, uint8_t* d_some,
                           uint64_t* n_records);
/* The same with data, written and some on the host. Synchronous. */
int nrg_memfs_pwrite(nrg_ctx* ctx, const nrg_memfs_wr* reqs, uint64_t n, const uint8_t* data, uint64_t data_bytes,
                     uint32_t origin, uint64_t* written, uint8_t* some, uint64_t* n_records);
/* The cut alone, into the caller's device buffer of cap records (8-byte aligned): exactly the records
 * nrg_memfs_pwrite_async would put in the ring; the log and the replica are not touched. The output
 * can be a segment of nrg_group_round_async (nrg_round.recs), which is how a replicated group carries
 * long writes. *n_records = T (nullable). T > cap: NRG_E_CAPACITY with *n_records = T and no byte of
 * d_recs written. Other errors as above. */
int nrg_memfs_pwrite_records_async(nrg_ctx* ctx, const nrg_memfs_wr* reqs, uint64_t n, const uint8_t* d_data,
                                   uint64_t data_bytes, nrg_memfs_op* d_recs, uint64_t cap, uint64_t* n_records);
/* Logged reads of any length: POSIX pread THROUGH THE LOG, the read benches/memfs.rs:73-78, :267-282 has
 * (OperationWr::Read { ino, fh, offset, size: u32 } is a write operation: its answer is the file as every
 * earlier record of the log left it). nrg_memfs_pread* above reads the local replica when it is called and
 * is no record; a single READ record carries at most 128 bytes. Here the record stays 152 bytes and the
 * response 136: a long read is a contiguous run of ordinary NRG_MEMFS_READ records in the log, one per
 * 128-byte line it touches, atomic against every other op for the reason a long write is (one appender;
 * group rounds concatenate whole segments), and replayed by every replica like any other records.
 * Requests are nrg_memfs_rd {ino, offset, len}. Let A = 2^adm, adm the log2 the requests are admitted
 * against: the growth bound where one is set above B, B otherwise (the rule of
 * nrg_memfs_pwrite_records_async: a group round may grow the store before the records are replayed).
 * THE CUT of request i, checked in the replay's order:
 *   ino outside the range       one record {ino, offset, READ, len 0}; some = 0, planned = 0 (the replay
 *                               answers NRG_MEMFS_ENOENT)
 *   len == 0 or offset >= A     one record {ino, offset, READ, len 0}; some = 1, planned = 0
 *   else                        planned = min(len, A - offset) (no overflow: len may be 2^64 - 1, "read to
 *                               the end"); one record per line of [offset, offset + planned), fragment k
 *                               (line_k = (offset >> 7) + k) covering
 *                               [max(offset, line_k * 128), min(offset + planned, (line_k + 1) * 128));
 *                               some = 1
 * Every request logs at least one record, and all 128 data bytes of a cut record are zero. first[0..n] is
 * the running sum of the record counts, T = first[n]; offs[0..n] is the running sum of planned. Both are
 * host arithmetic, known before anything is queued.
 * THE ANSWER of request i: some[i] as above; count[i], the bytes read; the bytes at
 * data[offs[i] .. offs[i] + count[i]). Request i owns the slot [offs[i], offs[i + 1]), and no byte of data
 * outside [offs[i], offs[i] + count[i]) is written, for any i. In an unsized context count[i] ==
 * planned[i] (A == B): data is packed exactly as nrg_memfs_pread would pack the same requests at that log
 * position, with the same offs. In a sized context count[i] = min(planned[i], max(size - offset, 0)) with
 * the file's size at the run's log position (it cannot change inside the run: Reads only). offs[n] > cap
 * is NRG_E_CAPACITY from the call WITH NOTHING LOGGED: the total is host-known. */
/* The cut as host arithmetic: no device, no context. first: n + 1 words; offs (n + 1) and some (n) may be
 * NULL. NRG_E_INVAL: a geometry nrg_open refuses (as nrg_memfs_pwrite_plan), a NULL reqs or first with
 * n > 0. */
int nrg_memfs_pread_logged_plan(uint32_t log2_adm, uint64_t files, const nrg_memfs_rd* reqs, uint64_t n,
                                uint64_t* first /* n + 1 */, uint64_t* offs /* n + 1 */, uint8_t* some /* n */);
/* Replica::combine for these reads. The requests are on the HOST and may be reused on return; data,
 * counts and some are on the device. In order: the plan (offs, host, n + 1 words, nullable, is filled
 * here, also when the call then returns NRG_E_CAPACITY), catch-up on the log, then passes of at most
 * min(log size - 8192, max_batch) records until all T are done: room in the ring, the cut written straight
 * into the ring at the tail, the tail advanced, the pass replayed with its responses into library scratch
 * (made by the first call, sized by max_batch), and the responses gathered into the slots. A request's
 * fragments may straddle passes: counts accumulate in stream order. Everything is ordered on the
 * context's stream. d_counts (8-byte aligned) / d_some: both or neither, n each. *n_records = T
 * (nullable). n == 0: NRG_OK, nothing logged. NRG_E_INVAL: a context of another kind, a NULL reqs, a NULL
 * d_data with cap > 0, exactly one of d_counts / d_some, a misaligned d_counts. NRG_E_CAPACITY:
 * n > config.max_batch, or offs[n] > cap. */
int nrg_memfs_pread_logged_async(nrg_ctx* ctx, const nrg_memfs_rd* reqs, uint64_t n, uint32_t origin, uint8_t* d_data,
                                 uint64_t cap, uint64_t* d_counts, uint8_t* d_some, uint64_t* offs /* n + 1 */,
                                 uint64_t* n_records);
/* The same with data, counts and some on the host, through the staging buffers. Synchronous. */
int nrg_memfs_pread_logged(nrg_ctx* ctx, const nrg_memfs_rd* reqs, uint64_t n, uint32_t origin, uint8_t* data,
                           uint64_t cap, uint64_t* counts, uint8_t* some, uint64_t* offs /* n + 1 */,
                           uint64_t* n_records);
/* The cut alone, into the caller's device buffer of cap records (8-byte aligned): exactly the records
 * nrg_memfs_pread_logged_async would put in the ring; the log and the replica are not touched. The output
 * can be a segment of nrg_group_round_async (nrg_round.recs) or of nrg_group_file_round, which is how a
 * group carries long reads. *n_records = T (nullable). T > cap: NRG_E_CAPACITY with *n_records = T and no
 * byte of d_recs written. */
int nrg_memfs_pread_logged_records_async(nrg_ctx* ctx, const nrg_memfs_rd* reqs, uint64_t n, nrg_memfs_op* d_recs,
                                         uint64_t cap, uint64_t* n_records);
/* The way back alone: the T responses (d_resp, d_resp_some; 8-byte aligned) that a round wrote for such a
 * segment, into the slots of d_data and d_counts / d_some (both or neither). It reads nothing of the
 * replica. NRG_E_INVAL: T != first[n], a NULL d_resp or d_resp_some with n > 0; NRG_E_CAPACITY:
 * offs[n] > cap; the rest as the async call. */
int nrg_memfs_pread_logged_gather_async(nrg_ctx* ctx, const nrg_memfs_rd* reqs, uint64_t n, const nrg_memfs_resp* d_resp,
                                        const uint8_t* d_resp_some, uint64_t T, uint8_t* d_data, uint64_t cap,
                                        uint64_t* d_counts, uint8_t* d_some);
/* Sizes (see nrg_memfs_op above): from here on the context's files have sizes, NRG_MEMFS_SETATTR is an
 * op, Writes grow and Reads / GetAttr see the size. Every size starts as B, so the state described is
 * the one found. Synchronous, idempotent, no way back. NRG_E_NOT_SYNCED while ltail < tail. Replicas of
 * one log must enable sizes at the same log index (nrg_memfs_init's rule). With sizes enabled:
 *   nrg_memfs_init   additionally sets size = max(size, len).
 *   nrg_memfs_read, nrg_memfs_pread*   clip at the size instead of B.
 *   nrg_memfs_dump   *n = size, and that many bytes.
 *   nrg_digest       today's items plus one per file: key file << 32 | 0xFFFFFFFF (no word index reaches
 *                    it), value the size.
 *   snapshots        the payload is followed by the F sizes as u64: items = F * B / 8 + F
 *                    (nrg_snapshot_size and nrg_snapshot_info_read say so). nrg_restore takes an image of
 *                    F * B / 8 items as before (a sized context stays sized, every size B) and one of
 *                    F * B / 8 + F items as a sized image: the context becomes sized; NRG_E_INVAL, the
 *                    files as at open, if a size is above B or a byte at or past a file's size is not
 *                    zero (checked on the device before the digests are compared).
 *   groups           nrg_group_resync carries the sizes in the image; a replicated round replays the
 *                    SetAttr records like any others. Enable sizes on every member (nrg_group_replica)
 *                    at the same log index. */
int nrg_memfs_enable_sizes(nrg_ctx* ctx);
/* *size = the size of file `ino` as replayed so far (does not need ltail == tail). NRG_E_INVAL: sizes not
 * enabled, or an ino outside the range. Synchronous. */
int nrg_memfs_size(nrg_ctx* ctx, uint64_t ino, uint64_t* size);
/* What a logged SetAttr{ino, size} does, directly and with no log traffic, for seeding short or empty
 * files as nrg_memfs_init seeds bytes (replicas of one log must be given the same). NRG_E_INVAL: sizes
 * not enabled, an ino outside the range or size > B; NRG_E_NOT_SYNCED while ltail < tail. Synchronous. */
int nrg_memfs_truncate(nrg_ctx* ctx, uint64_t ino, uint64_t size);
/* File store: capacity growth. A sized context only (the invariant "every stored byte at or past the
 * size is zero" defines the new bytes: they are zero, and holes cost nothing); in an unsized context
 * nrg_set_max_capacity and nrg_memfs_reserve return NRG_E_INVAL.
 *   THE BOUND   nrg_set_max_capacity(ctx, max_bytes): the unit is BYTES PER FILE. max_bytes is a power of
 *               two, at least the current B, at most 2^26, with F * max_bytes <= 2^29 (nrg_open's limits);
 *               else NRG_E_INVAL. 0 turns growth off. NRG_E_NOT_SYNCED while ltail < tail: a record is
 *               admitted by the bound in force at its own log index, so replicas of one log must set the
 *               bound at the same log index (nrg_memfs_enable_sizes' rule).
 *   ADMISSION   with a bound of max: a valid WRITE with len > 0 and offset + len <= max, and a valid
 *               SETATTR with size <= max, are admitted. Everything else EFBIG covers still answers EFBIG and
 *               changes nothing (offset + len overflowing 64 bits included). The EINVAL and ENOENT checks
 *               come first: such a record never causes growth, whatever its offset says.
 *   CAPACITY    B after any log prefix = max(B at open or the last reserve, the power of two at or above
 *               the largest admitted end (offset + len, or a SetAttr's size) so far). It is a PURE
 *               FUNCTION OF THE PREFIX: a maximum, with no doubling rule beyond the rounding. This is
 *               stronger than the other kinds' guarantee: B, and with it nrg_digest (whose items are every
 *               word of every file up to B), does not depend on how the log was cut into chunks. A replica
 *               that runs a fused round and one that follows the ring with nrg_sync in other chunk sizes
 *               end with the same geometry and the same digest. B changes before a chunk is replayed, to
 *               what the whole chunk needs; nothing observable happens mid-chunk, since GETATTR answers
 *               the size, not the capacity. While B < max a replayed chunk costs one more small kernel and
 *               an 8-byte readback; at B == max the store is a fixed one and nothing is launched or read.
 *               NRG_E_NOMEM from a round call: the larger store could not be allocated, nothing of the
 *               chunk was launched and the replica is unchanged.
 *   DIRECT      nrg_memfs_truncate(ino, size) with B < size <= max grows first; nrg_memfs_init with
 *               len > B stays NRG_E_INVAL. nrg_memfs_pwrite[_async] decides EFBIG against max, takes the
 *               need of all its requests from its plan and grows once before its first pass (no readback).
 *               nrg_memfs_pwrite_records_async decides EFBIG against max (against B with no bound) and does
 *               not grow: the replay of its records does. A caller of nrg_memfs_pwrite_plan passes the log2
 *               it wants admission decided against (log2 max under a bound).
 *   READS       nrg_memfs_pread*, nrg_memfs_read, nrg_memfs_dump, nrg_memfs_geometry, nrg_digest and
 *               snapshots see the geometry as it stands at the call.
 *   RESTORE     with a bound, an image of a sized store with the same F and a power-of-two B_img in
 *               (B, max] is accepted: the context is reallocated to B_img first. B_img < B stays
 *               NRG_E_INVAL (the store never shrinks); without a bound the rule is as before.
 *               nrg_group_resync follows.
 *   GROUPS      replicated rounds: every replica replays every record; set the bound on every member.
 *               File-partitioned rounds and group-wide preads (nrg_group_file_round,
 *               nrg_group_memfs_pread): an owner replays only its own files' records, so growth under
 *               replay would let the members' B diverge. A member with a bound set reports NRG_E_INVAL in
 *               its exchange word and every rank returns that code together. Such groups grow with
 *               nrg_memfs_reserve on every member.
 * nrg_memfs_reserve: the explicit, synchronous half. file_bytes is rounded up to a power of two; never
 * shrinks (a request the store satisfies returns NRG_OK and does nothing); NRG_E_INVAL beyond nrg_open's
 * limits or in an unsized context. Works with or without a bound; a store reserved beyond its bound is a
 * fixed one. nrg_memfs_geometry reports the current B. nrg_memfs_max_capacity: *max_bytes = the bound, 0
 * for none (no device is touched). */
int nrg_memfs_reserve(nrg_ctx* ctx, uint64_t file_bytes);
int nrg_memfs_max_capacity(nrg_ctx* ctx, uint64_t* max_bytes);

/* ---- multi-GPU replica groups (RCCL over xGMI) --------------------------------------------
 * The reference shares ONE log between replicas through cache-coherent memory: every replica's
 * Log::exec reads every entry (nr/src/log.rs:494-511, :473-524). Across GPUs the write segments
 * of a round are all-gathered with RCCL (ncclAllGather, one communicator per GPU, over xGMI)
 * and every replica replays the identical global log W_0 || W_1 || ... || W_{n-1} (rank order);
 * reads stay on their GPU; write responses go to the origin replica only
 * (nr/src/replica.rs:576-578). The all-gather runs on a library-owned stream per GPU and the
 * gathered buffers rotate, so the all-gather of round e+1 overlaps the replay of round e.
 * RCCL is loaded at the first group call (librccl.so.1, the process's own copy if one is
 * already loaded); without it these calls return NRG_E_COMM. */
#define NRG_E_COMM (-9)          /* RCCL unavailable or a collective failed               */
#define NRG_E_TIMEOUT (-10)      /* a peer rank did not take part in a collective before the
                                    group's deadline (nrg_group_set_timeout)                 */
#define NRG_GROUP_DEFAULT_TIMEOUT_MS 300000u
#define NRG_GROUP_ID_BYTES 128   /* ncclUniqueId                                           */

typedef struct nrg_group nrg_group;

/* A group member's part of one round (all pointers are device pointers on its GPU). */
typedef struct {
    const void* recs;          /* this replica's write segment (log records, issue order)       */
    uint64_t n;                /* records in it                                                  */
    void* resp;                /* nullable: responses to its own writes (as nrg_log_exec_async)  */
    uint8_t* some;
    const uint64_t* get_keys;  /* hashmap, skip list: reads answered against the post-round state */
    uint64_t n_gets;
    uint64_t* get_vals;
    uint8_t* get_found;
} nrg_round;

/* ncclGetUniqueId: one process creates the id and ships it to the others (any side channel). */
int nrg_group_unique_id(uint8_t id[NRG_GROUP_ID_BYTES]);
/* One process per GPU: `replica` joins group `id` as rank `rank` of `nranks` (ncclCommInitRank
 * on the replica's device). Replica ids should be rank + 1 (Log::register order). */
int nrg_group_join(nrg_ctx* replica, const uint8_t id[NRG_GROUP_ID_BYTES], int nranks, int rank,
                   nrg_group** out);
/* One process driving n GPUs: opens one replica per device (cfg, replica_id = i + 1) and one
 * communicator per device (ncclCommInitAll). The group owns these replicas. */
int nrg_group_open(const int* devices, int n, const nrg_config* cfg, nrg_group** out);
/* Closes the communicators and the group's buffers (and the replicas nrg_group_open opened). */
int nrg_group_close(nrg_group* g);
/* nranks: group size; nlocal: members driven by this process; rank0: rank of local member 0. */
int nrg_group_info(const nrg_group* g, int* nranks, int* nlocal, int* rank0);
nrg_ctx* nrg_group_replica(nrg_group* g, int member);
/* The all-gather of a member's segment waits for work queued on `hip_stream` when the round is
 * issued (default: the replica's own stream, which also orders it after the previous replay;
 * give the stream the inputs are produced on to let all-gathers run ahead of replays). */
int nrg_group_set_input_stream(nrg_group* g, int member, void* hip_stream);
/* One NR round on every local member: all-gather of the members' write segments (RCCL), then on
 * each replica Log::append of the gathered segments in rank order + Log::exec + its reads.
 * Appends of any length interleave, as in the reference (nr/src/log.rs:343-427): ranks may hold
 * different segment lengths, and every rank must learn all of them before the all-gather.
 *   seg_lens == NULL   the ranks exchange {n, local error} first (one 8-B-per-rank all-gather and
 *                      one host round trip); a rank with a bad segment makes the round return
 *                      NRG_E_INVAL on EVERY rank, before any data moves.
 *   seg_lens != NULL   seg_lens[r] = rank r's segment length; every rank must pass the same array.
 *                      The round stays stream ordered: a header {n, fingerprint of seg_lens}
 *                      travels with each segment and is compared on every rank's comm stream. A
 *                      rank whose n differs from seg_lens[rank] still takes part (with zeros) and
 *                      returns NRG_E_INVAL; any disagreement makes the next nrg_group_sync /
 *                      nrg_sync of every rank return NRG_E_INVAL. (Arrays whose longest segment
 *                      differs would give all-gathers of different sizes: RCCL cannot check that.)
 * A single-process group (nrg_group_open) takes its members' n (seg_lens, if given, must agree).
 * Stream ordered; borrows buffers until the replica stream passes this round (config.pipeline =
 * 1: until nrg_join / the next call). */
int nrg_group_round_async(nrg_group* g, const nrg_round* rounds, const uint64_t* seg_lens);
/* Wait for all queued group work and report latched device errors of every local replica. */
int nrg_group_sync(nrg_group* g);
/* Replica::verify (nr/src/replica.rs:443-467) across the group: are the replicas identical? A
 * collective: every rank calls it. It completes queued group work as nrg_group_sync does (a posted
 * partitioned round included, latched device errors reported), runs nrg_digest_async on every
 * local member's replica stream, all-gathers the three words per rank on the comm stream and reads
 * them back under the group's deadline (a missing peer: NRG_E_TIMEOUT). `digests` (nullable)
 * receives nranks * 3 words in rank order; *identical = 1 iff every rank's triple is the same. A
 * difference is a result, not an error: the call returns NRG_OK and the group stays usable. A rank
 * whose own sync reported a latched device error still takes part and then returns that error.
 * The members of a partitioned group hold one partition each, so *identical is 0 by design there:
 * such callers add the triples (count and sum add, xor xors) and compare with the whole map's. */
int nrg_group_verify(nrg_group* g, uint64_t* digests, int* identical);
/* What to do about *identical = 0: every rank's replica becomes rank `root_rank`'s (Replica::new,
 * nr/src/replica.rs:184-232, from the root's state as Replica::verify, :443-467, sees it). A
 * collective: every rank calls it with the same root. It completes queued group work as
 * nrg_group_sync does (a sticky failure returns its code; a latched device error of a replica is
 * cleared, its contents are about to be replaced), the ranks learn the root's image size through one
 * small all-gather read back under the group's deadline (a missing peer: NRG_E_TIMEOUT), every
 * member grows a group-owned buffer, the root snapshots into its own (nrg_snapshot_async) and, inside
 * one ncclGroupStart / ncclGroupEnd on the comm streams, sends it to every other rank; every other
 * member then calls nrg_restore from its buffer, log positions included. A member whose restore
 * fails returns that code (a single-process group: the first such code); the others return NRG_OK.
 * For replicated groups: on a group that runs partitioned rounds every rank would end up with the
 * root's partition. */
int nrg_group_resync(nrg_group* g, int root_rank);
/* Deadline of every wait on the peer ranks (default NRG_GROUP_DEFAULT_TIMEOUT_MS): the host round
 * trips of the length / count exchanges, buffer regrowth and nrg_group_sync. A rank whose peers do
 * not post their part of a collective in time gets NRG_E_TIMEOUT instead of hanging (its
 * communicators are aborted, so the group can still be closed). Failures that leave the ranks'
 * replicas different -- a timeout, a failed collective, ranks that disagreed on seg_lens -- are
 * sticky: every later round or sync of the group returns the same code; close the group.
 * (Like RCCL, a process blocked inside ncclCommInitRank or ncclGroupEnd itself -- before the
 * stream waits -- is not bounded here; bench.py keeps a whole-process watchdog for that.) */
int nrg_group_set_timeout(nrg_group* g, uint32_t ms);
/* The sticky failure's description ("nrg_group rank R of N, round E: ..."), "" if none. */
const char* nrg_group_last_error(const nrg_group* g);

/* ---- cnr-style key-partitioned NrHashMap and skip list --------------------
 * cnr maps each operation to one of several logs with LogMapper::hash() (cnr/src/lib.rs:134-167);
 * the operations of one key share a log, so the logs replay independently
 * (cnr/src/replica.rs:430-445 hash -> log, :673-736 combine(hashidx)). Across GPUs, partition p's
 * log lives on GPU p, which holds only the keys it owns (no full replication): a round's Puts and
 * Gets travel to their owners, each owner replays the Puts it received in rank order -- for every
 * key the same order as the NR global log W_0 || W_1 || ... -- and answers the Gets it received,
 * and answers and previous values travel back in the caller's order. The answers are identical
 * to NR's; the replicas are not (each holds one partition).
 * The reference runs its skip list only this way (skiplist-mlnr{logs}, benches/lockfree.rs:228-317:
 * OpWr::Push(k, v) and SkipListConcurrent::Get(k) both mapped to a log by key, :73-97), so a group
 * of NRG_DS_SKIPLIST replicas takes partitioned rounds too: records are Push(k, v) (nrg_put), the
 * Gets are Get(k). Every member of a group must be of the same kind. */
#define NRG_MAX_PARTS 64
/* Owner partition of a key: (low 32 bits of splitmix64(key)) * parts >> 32. */
uint32_t nrg_key_owner(uint64_t key, uint32_t parts);
/* Stable partition of W Puts and R Get keys by owner (device buffers, the replica's stream):
 * puts_out / keys_out hold them grouped by owner, each group in issue order; put_pos[i] / get_pos[i]
 * = where record i went; counts[p] = Puts of owner p, counts[parts + p] = Gets of owner p (u64).
 * W, R < 2^32. */
int nrg_hashmap_partition_async(nrg_ctx* ctx, const nrg_put* d_puts, uint64_t W, const uint64_t* d_keys, uint64_t R,
                                uint32_t parts, nrg_put* d_puts_out, uint32_t* d_put_pos, uint64_t* d_keys_out,
                                uint32_t* d_get_pos, uint64_t* d_counts);
/* dst[i] = src[pos[i]] (u64 and/or u8 arrays; either pair may be NULL): answers back in order. */
int nrg_route_back_async(nrg_ctx* ctx, const uint64_t* d_src, const uint8_t* d_src8, const uint32_t* d_pos, uint64_t n,
                         uint64_t* d_dst, uint8_t* d_dst8);
/* NrHashMap::default restricted to a partition: keys k < n with nrg_key_owner(k, parts) == part. */
int nrg_hashmap_prefill_partition(nrg_ctx* ctx, uint64_t n, uint64_t off, uint32_t part, uint32_t parts);
/* One partitioned round on every local member (group of hashmap or of skip-list replicas, one
 * partition each, rank = partition; another kind: NRG_E_INVAL): rounds[i].recs / n = the member's
 * Puts (nrg_put), get_keys / n_gets its Gets; get_vals / get_found and (nullable) resp / some = the
 * Gets' answers and the Puts' previous values, in the member's order. A skip list's Push responses
 * are Ok(Some(key)) whatever the state (benches/lockfree_partitioned.rs:108-111): they never travel;
 * resp[i] = recs[i].key and some[i] = 1 are written on the asker's GPU when the round's Get answers
 * arrive, and a dropped round writes none. An owner replays the Puts it received in slices of at
 * most max_batch and then answers the Gets it received in slices of at most max_reads. Ranks whose
 * kinds differ make the round return NRG_E_INVAL on every rank before any payload moves. A round is one fused partition launch (owner regions, no global scan), an
 * all-gather of every rank's per-owner counts, ncclSend / ncclRecv of the Puts and Get keys to
 * their owners (a rank's own part stays on its GPU), the owner's replay, the answers back and one
 * route-back launch. Everything is on the replica's stream. Returns once the round is queued,
 * after one host round trip for the counts (nrg_group_sync waits for the rest). Fails with the
 * same code on every rank when any rank's part is bad, before any payload moves. */
int nrg_group_partitioned_round(nrg_group* g, const nrg_round* rounds);
/* The pipelined form, three calls deep: queues this round's partition and count exchange, moves
 * the previous round's Puts and Gets to their owners and replays it (its counts have landed by
 * then, so the host never waits on the GPU in steady state; its reads ride in the next round's
 * first launch), and sends the round before that back into its caller's order. The caller's
 * buffers of a round stay borrowed for the next two calls, or until nrg_group_partitioned_flush /
 * nrg_group_sync completes every posted round. A round dropped on an agreed error (a rank's bad
 * part) returns that error from the call that moved it (NRG_OK otherwise). A one-rank group
 * partitions on a library-owned side stream, after the work queued on the replica's stream and
 * beside the previous round's replay; the replica's stream waits for it before moving the round. */
int nrg_group_partitioned_round_async(nrg_group* g, const nrg_round* rounds);
/* Complete the round posted by nrg_group_partitioned_round_async, if any (its result). */
int nrg_group_partitioned_flush(nrg_group* g);

/* ---- file-partitioned file store (nrfs-mlnr{logs}) --------------------------------------------
 * benches/nrfs.rs is a cnr benchmark with one log per file: LogMapper::hash() = fd - 1
 * (benches/nrfs.rs:8, :25-39), LogStrategy::Custom(logs) (:132-141), hash % logs
 * (cnr/src/replica.rs:430-445); ops on different files never share a log and each log replays on its
 * own (:673-736). Across GPUs the log of partition p lives on rank p.
 *   OWNER  of file `ino`: (ino - NRG_MEMFS_FIRST_INO) % parts, and 0 for an ino below NRG_MEMFS_FIRST_INO;
 *          inos past the last file map by the same formula. Every member applies the same checks in the
 *          same order, so an ENOENT / EINVAL / EFBIG answer is the same whichever member gives it.
 *   STATE  every member is opened with the group's full geometry (the same F and B); a file-partitioned
 *          round changes, on member p, only files that p owns, and a member's copy of a file it does not
 *          own is never read or written by such a round (cnr: the logs are partitioned, every replica
 *          still holds the structure).
 *   ORDER  an owner replays what it received from rank 0, then rank 1, ..., each rank's part in issue
 *          order: for every file the order of the NR global log W_0 || W_1 || ... restricted to that
 *          file. Every op touches one file and its size only, so every response is bit for bit the
 *          replicated round's and every file on its owner is bit for bit the replicated replica's. A
 *          long write (nrg_memfs_pwrite_records_async) is a contiguous run of Write records of one ino:
 *          one owner, and the stable partition keeps its order.
 *   SIZES  either every member has nrg_memfs_enable_sizes on or none has (else NRG_E_INVAL, below). */
uint32_t nrg_memfs_owner(uint64_t ino, uint32_t parts); /* benches/nrfs.rs:25-39, cnr/src/replica.rs:430-445 */
/* Stable partition of n records by owner (device buffers, the replica's stream; benches/nrfs.rs:25-39,
 * cnr/src/replica.rs:430-445, :673-736): d_out holds them grouped by owner 0 .. parts-1, each group in
 * issue order, compact (no per-owner stride); d_pos[i] = where record i went; d_counts[p] = records of
 * owner p (u64). n < 2^32 (NRG_E_CAPACITY), 1 <= parts <= NRG_MAX_PARTS; d_ops and d_out 8-byte aligned.
 * Three launches: owner counts per tile of NRG_MEMFS_PARTITION_TILE records, a scan of them per owner,
 * the scatter. No byte of d_out at or past n records is written. */
#define NRG_MEMFS_PARTITION_TILE 256
int nrg_memfs_partition_async(nrg_ctx* ctx, const nrg_memfs_op* d_ops, uint64_t n, uint32_t parts,
                              nrg_memfs_op* d_out, uint32_t* d_pos, uint64_t* d_counts);
/* d_dst[i] = d_src[d_pos[i]], d_dst_some[i] = d_src_some[d_pos[i]]: responses back into issue order
 * (either pair may be NULL; benches/nrfs.rs:25-39, cnr/src/replica.rs:430-445, :673-736). */
int nrg_memfs_route_back_async(nrg_ctx* ctx, const nrg_memfs_resp* d_src, const uint8_t* d_src_some,
                               const uint32_t* d_pos, uint64_t n, nrg_memfs_resp* d_dst, uint8_t* d_dst_some);
/* One file-partitioned round on every local member of a group of NRG_DS_MEMFS replicas, rank = partition
 * (benches/nrfs.rs:25-39, cnr/src/replica.rs:430-445, :673-736). rounds[i].recs / n are member i's
 * nrg_memfs_op records: anything nrg_memfs_round_async takes, the runs nrg_memfs_pwrite_records_async
 * makes included. resp / some (nrg_memfs_resp, u8) are nullable: if either is NULL the rank asks for no
 * responses, nothing travels back to it and its buffers are not written. get_keys / n_gets must be
 * NULL / 0. A round is: one partition on the member's stream; an all-gather of every rank's records per
 * owner and flags (its receive capacity, a local error, the kind, F, log2 B, sized, wants responses),
 * read back under the group's deadline (NRG_E_TIMEOUT); the plan; where some rank must grow its receive
 * buffers, a growth-confirm exchange; ncclSend / ncclRecv of the records to their owners (a rank's own
 * part is a device copy); the owner's replay with nrg_memfs_round_async in slices of at most max_batch
 * and origin = rank + 1; responses and some bytes back to the ranks that asked; one route-back launch.
 * Everything runs on the replica's stream. Returns once the round is queued, after one host round trip
 * for the counts; nrg_group_sync waits for the rest, and the caller's buffers stay borrowed until then.
 * Every failure known before the first send / recv is agreed on by all ranks and returned by all of
 * them, the round dropped everywhere (nothing of it written, no replica changed, the group usable):
 *   NRG_E_INVAL     a rank with n > 0 and NULL recs (or recs / resp not 8-byte aligned), n_gets != 0, a
 *                   rank whose replica is not a file store, ranks whose kinds, F, B or sized flags differ
 *   NRG_E_CAPACITY  n >= 2^32
 * An EINVAL record latches NRG_E_INVAL on its owner's replica and nrg_group_sync reports it, as ever.
 * A one-rank group does not partition: it replays the caller's records into the caller's buffers
 * (NRG_KNOB_EXP bit 16, measurement, makes it take the data-moving path). Row p of nrg_group_verify is
 * the digest of a replica that replayed only owner p's records. After such a round the only correct
 * copy of a file is its owner's: read with nrg_group_memfs_pread below, not with nrg_memfs_pread* on a
 * member. Not for this mode: nrg_group_resync (every rank would end up with the root's files), a
 * pipelined form. */
int nrg_group_file_round(nrg_group* g, const nrg_round* rounds);

/* The building blocks of the group-wide pread below, on one replica's stream (device buffers).
 * nrg_memfs_rd_partition_async: the stable partition of n pread requests by the owner of their file
 * (benches/nrfs.rs:25-39 LogMapper::hash, cnr/src/replica.rs:430-445), as nrg_memfs_partition_async
 * partitions records: d_out grouped by owner 0 .. parts-1, each group in request order, compact;
 * d_pos[i] = where request i went; d_counts[p] = requests of owner p. The same three launches over
 * tiles of NRG_MEMFS_PARTITION_TILE requests; no byte of d_out at or past n requests is written.
 * n < 2^32 (NRG_E_CAPACITY), 1 <= parts <= NRG_MAX_PARTS; d_reqs and d_out 8-byte aligned. */
int nrg_memfs_rd_partition_async(nrg_ctx* ctx, const nrg_memfs_rd* d_reqs, uint64_t n, uint32_t parts,
                                 nrg_memfs_rd* d_out, uint32_t* d_pos, uint64_t* d_counts);
/* nrg_memfs_pread_repack_async: answers that lie packed in PARTITION order back into REQUEST order
 * (the asker's half of OpRd::FileRead routed to its log's owner, benches/nrfs.rs:88-101, :146-152,
 * cnr/src/replica.rs:430-445). Partition position p holds d_src_cnt[p] bytes and the byte d_src_some[p];
 * d_src is their concatenation in partition order. Request i (at position p = d_pos[i], a permutation
 * of 0 .. n-1) gets d_some[i] = d_src_some[p], d_offs[i + 1] = d_offs[i] + d_src_cnt[p] (n + 1 words,
 * d_offs[0] = 0), and its bytes at d_data[d_offs[i] ..): the layout nrg_memfs_pread_async writes, by
 * the same copy kernel (tiles of NRG_MF_PREAD_TILE output bytes), and as there no byte of d_data at or
 * past min(cap, d_offs[n]) is ever written. d_src must be 16-byte aligned and READABLE up to the next
 * multiple of 16 past its last byte (the copy reads the aligned 16-byte blocks around a source byte);
 * NRG_E_INVAL otherwise, for d_src_cnt or d_offs not 8-byte aligned, and with n > 0 for a NULL
 * d_src_cnt, d_src_some, d_pos, d_offs or d_some, or cap > 0 and a NULL d_data. n >= 2^32:
 * NRG_E_CAPACITY. n == 0 writes d_offs[0] = 0. A position >= n counts as 0 bytes, some = 0. */
int nrg_memfs_pread_repack_async(nrg_ctx* ctx, const uint8_t* d_src, const uint64_t* d_src_cnt,
                                 const uint8_t* d_src_some, const uint32_t* d_pos, uint64_t n, uint8_t* d_data,
                                 uint64_t cap, uint64_t* d_offs /* n + 1 */, uint8_t* d_some /* n */);
/* Group-wide pread of a file-partitioned group: exec_ro(OpRd::FileRead(fd)) of benches/nrfs.rs:88-101,
 * :146-152, routed to the owner of the file's log as cnr/src/replica.rs:430-445 routes it, here POSIX
 * pread of any length as nrg_memfs_pread. reads[i] is local member i's part (device pointers on its GPU;
 * reqs 8-byte aligned). Member r's some, offs and data are exactly what nrg_memfs_pread would give for
 * r's requests on a replica whose every file is its OWNER's copy (sizes on: clipped at the owner's
 * size); inos below NRG_MEMFS_FIRST_INO and past the last file answer some = 0 and no bytes, whichever
 * owner the formula picks. Nothing is logged and no replica changes: the rows of nrg_group_verify are
 * the same before and after. A collective shaped like nrg_group_skiplist_seek: every rank calls it, the
 * ranks' n may differ, n = 0 on every rank returns NRG_OK after the exchange; it first completes queued
 * group work as nrg_group_sync does (a latched device error is reported at the end) and returns when
 * the answers are in the callers' buffers. config.max_reads does not apply: the scratch is the group's
 * and grows on demand. On the replica's stream, host waits under the group's deadline:
 *   1  the partition of the member's requests by owner (nrg_memfs_rd_partition_async); an all-gather of
 *      every rank's requests per owner and its words (receive capacity, a local error, the kind, F,
 *      log2 B, sized, cap), read back: host round trip 1, the agreement and the plan;
 *   2  ncclSend / ncclRecv of the 24-byte requests to their owners (a rank's own part: a device copy);
 *   3  the owner scans the clipped lengths of all it received (the kernels of nrg_memfs_pread_async):
 *      a count and a some byte per request, and the bytes T[o][s] it owes each asker s;
 *   4  counts and some bytes back to the askers; an all-gather of every owner's row of T, read back:
 *      host round trip 2, the capacity decision and every byte offset;
 *   5  the owner's packed bytes (the copy kernel of nrg_memfs_pread_async), sent to the askers;
 *   6  the re-pack into request order (nrg_memfs_pread_repack_async).
 * A one-rank group runs nrg_memfs_pread_async's kernels straight into the caller's buffers
 * (NRG_KNOB_EXP bit 16, measurement, makes it take steps 1 to 6). Every failure is agreed on by all
 * ranks from the exchanged words before any data byte moves, the first in rank order wins, and the
 * group stays usable:
 *   NRG_E_INVAL       n > 0 with a NULL reqs, offs or some; cap > 0 with a NULL data; reqs or offs not
 *                     8-byte aligned; a member that is no file store; ranks whose F, B or sized flags differ
 *   NRG_E_NOT_SYNCED  a member with ltail < tail
 *   NRG_E_CAPACITY    n >= 2^32; or some rank's total exceeds its cap: then every rank's offs and some
 *                     are complete, data[0, cap) is unspecified and nothing at or past cap is written,
 *                     so a call with cap = 0 and data = NULL on every rank sizes the answer (offs[n]).
 * NRG_E_COMM / NRG_E_TIMEOUT as nrg_group_verify. Out of scope: a pipelined form, nrg_group_resync. */
typedef struct {
    const nrg_memfs_rd* reqs; /* this member's requests */
    uint64_t n;
    uint8_t* data;            /* the packed answer */
    uint64_t cap;
    uint64_t* offs;           /* n + 1 */
    uint8_t* some;            /* n */
} nrg_pread;
int nrg_group_memfs_pread(nrg_group* g, const nrg_pread* reads);

/* Group-wide ordered reads of a partitioned skip-list group. A skip list exists for its order, and
 * under hash partitioning no member alone can answer lower_bound or a range count: every member
 * answers every query against its own partition (the kernels of nrg_skiplist_seek_async /
 * nrg_skiplist_range_count_async) and each asker reduces the candidates of the G partitions. Both
 * calls are collectives, shaped like nrg_group_verify: every rank calls them (seek: with the same
 * mode), with one entry per local member; all pointers are device pointers on the member's GPU.
 * They complete queued group work as nrg_group_sync does (a posted partitioned round included, a
 * latched device error reported at the end), exchange the members' n and argument errors (one
 * 8-byte-per-rank all-gather read back under the group's deadline), all-gather the queries padded
 * to the longest n, answer, return each asker's candidates with ncclSend / ncclRecv (a rank's own:
 * a device copy) and reduce them in one launch; they return when the answers are in the caller's
 * buffers. The members' n may differ; n = 0 on every rank returns NRG_OK after the exchange. A
 * one-rank group's only candidate is the answer: after the exchange its read kernel answers straight
 * into the caller's buffers.
 *   seek         out_keys[i] / out_vals[i] / found[i] as nrg_skiplist_seek's over the whole map: among
 *                the partitions that found a candidate the smallest key (GE, GT) or the largest (LE,
 *                LT); partitions hold disjoint key sets, and 0 and 2^64 - 1 are ordinary keys.
 *   range count  counts[i] = keys of the whole map in [los[i], his[i]] (0 where lo > hi): the sum.
 * NRG_E_INVAL on every rank, before any data moves: the group's replicas are not skip lists, a mode
 * above NRG_SEEK_LT, ranks that passed different modes, or any rank with n > 0 and a NULL buffer
 * (n >= 2^32 counts as that). NRG_E_COMM / NRG_E_TIMEOUT as nrg_group_verify. The scratch belongs to
 * the group and grows on demand. There is no nrg_group_skiplist_len: the count words (word 0 of each
 * rank's triple) of nrg_group_verify add up to it. A partitioned range / dump is the caller's merge
 * of the members' nrg_skiplist_range results, or, page by page and in key order over the whole map,
 * nrg_group_skiplist_scan below. */
typedef struct {
    const uint64_t* keys;
    uint64_t n;
    uint64_t* out_keys;
    uint64_t* out_vals;
    uint8_t* found;
} nrg_seek;
int nrg_group_skiplist_seek(nrg_group* g, const nrg_seek* seeks, uint32_t mode);
typedef struct {
    const uint64_t* los;
    const uint64_t* his;
    uint64_t n;
    uint64_t* counts;
} nrg_count;
int nrg_group_skiplist_range_count(nrg_group* g, const nrg_count* counts);
/* nrg_skiplist_scan over the whole partitioned map (SkipMap::range from a bound, the first `limit`
 * entries; nr/src/replica.rs:443-467): a collective shaped exactly like nrg_group_skiplist_seek, on
 * the same data path. Every rank calls it with the same mode and the same limit, one entry per local
 * member; n may differ, n = 0 on every rank returns NRG_OK after the exchange. Every member answers
 * every rank's queries against its own partition (the kernel of nrg_skiplist_scan_async: up to
 * `limit` candidates per query and partition), the candidate blocks (keys, values, u32 counts) go
 * back to their askers, and one launch per member merges each query's G sorted lists: partitions
 * hold disjoint key sets, so a candidate's place is its place in its own list plus the number of
 * candidates of the other lists that precede it, and the first `limit` places are stored. The
 * answers are nrg_skiplist_scan's over the whole map, slots j >= counts[i] not written. The
 * candidate traffic is G times the answer's size, as the seek's: under hash partitioning every
 * partition may hold the next key. A one-rank group's kernel answers straight into the caller's
 * buffers. Paging with GT(the last key of a page) walks the whole map in key order.
 * NRG_E_INVAL on every rank, before any data moves: not skip lists, mode > NRG_SEEK_LT, limit = 0 or
 * limit > NRG_SCAN_MAX_LIMIT, ranks that passed different modes or limits, or any rank with n > 0 and
 * a NULL buffer. NRG_E_CAPACITY on every rank, before any data moves: G * nmax * limit > 2^27
 * entries, nmax the longest n of the ranks (the candidate scratch of one member: 2 GiB of keys and
 * values at the bound). */
typedef struct {
    const uint64_t* keys;
    uint64_t n;
    uint64_t* out_keys;
    uint64_t* out_vals;
    uint32_t* counts;
} nrg_scan;
int nrg_group_skiplist_scan(nrg_group* g, const nrg_scan* scans, uint32_t mode, uint32_t limit);

/* Removal and pops in a partitioned skip-list group. A member that enabled either on its own context
 * makes a partitioned round return NRG_E_INVAL (above); a GROUP opts in as a whole, through a collective
 * in which every rank passes the same values, so that no round can find two owners reading {k, v}
 * differently. Both calls are collectives shaped like nrg_group_verify: every rank calls them; they
 * first complete queued group work as nrg_group_sync does (a posted partitioned round included; an
 * error of that work counts as the rank's local error below); every rank's values and local status are
 * exchanged (8-byte words, read back under the group's deadline) and every rank derives the same code
 * BEFORE anything is enabled anywhere: the first local error in rank order, else NRG_E_INVAL where the
 * ranks' values differ. Local errors: NRG_E_INVAL for a member that is no skip list, a member already
 * enabled with other values, values other than the group's earlier agreement, marks equal to each other
 * or to the tombstone (the member's or the group's); NRG_E_NOT_SYNCED for a member with ltail < tail. On
 * NRG_OK every local member is enabled (nrg_skiplist_enable_removal / nrg_skiplist_enable_pops; one
 * already enabled with the same values is fine) and the group records the agreement. Again with the same
 * values: NRG_OK; with others: NRG_E_INVAL. There is no way back. A group that never calls them behaves
 * as before in every respect and launches the same kernels, the refusals above included.
 *   Removal: from here on a record whose val == tombstone is Remove(key) in partitioned rounds (both
 * forms, the one-rank identity included). It is routed by its key like a Push, so it reaches the key's
 * owner; the owner replays the slices it received in rank order and, where some rank passed resp / some,
 * answers EVERY received record (Push: (key, 1); Remove: (previous value, 1) or (0, 0), as
 * nrg_skiplist_round_async answers); the responses travel back to the askers as a hashmap group's
 * previous values do and arrive in issue order. They are bit for bit what one replica holding the whole
 * map answers when it replays the round's records in rank order, then issue order; the round's Gets are
 * answered against the post-round state. The asker-side Push response launch is not used on such a
 * group. Costs beyond a plain skip-list round: the response traffic, and what removal costs a replay
 * (nrg_skiplist_enable_removal: a count readback per chunk).
 *   Pops: a record whose val is a mark would be routed by the hash of its count and pop one partition's
 * front, so on a group that agreed on pops a partitioned round that holds a mark record on ANY rank is
 * refused on EVERY rank with NRG_E_INVAL, like a round with any other bad argument: before any payload
 * moves, no response written, no log moved, the group usable. The marks are found on the device in the
 * post step (one small pass over the member's records, launched only on such a group) and folded into
 * the round's exchanged error word. A pops group pays for it: the one-rank identity form, which
 * otherwise never waits for its post step, reads that flag on the host before it replays. Rounds without
 * mark records run as before, so Push rounds and nrg_group_skiplist_pop alternate freely. */
int nrg_group_skiplist_enable_removal(nrg_group* g, uint64_t tombstone);
int nrg_group_skiplist_enable_pops(nrg_group* g, uint64_t front_mark, uint64_t back_mark);
/* The group-wide pop: "the n smallest entries" is a question about the union of G partitions with
 * disjoint key sets, which no member answers alone. A collective shaped like nrg_group_skiplist_seek, on
 * a group that agreed on pops; pops[i] is local member i's part (reqs a HOST array, every other pointer a
 * device pointer on the member's GPU). The ranks' requests, concatenated in rank order (rank 0's in issue
 * order, then rank 1's, ...), are ONE run of consecutive pop records replayed against the whole
 * partitioned map: the grants, front ranks and back ranks of nrg_skiplist_enable_pops' pop step with
 * len = the sum of the members' lengths (counts up to 2^64 - 1, clipped to len). Every rank gets what
 * nrg_skiplist_round_pops_async would give it for its own records of that run on a single replica
 * holding the union: resp[j] = entries popped by request j, some[j] = (resp[j] >= 1), the popped entries
 * packed in request order, each request's in the order popped (front ascending, back descending), and
 * *pop_n = the total this member popped. Only the first pop_cap entries are stored and nothing is
 * written past them. Afterwards the union of the members is the map minus the popped entries and every
 * member still holds only keys it owns. On the replica's stream, host waits under the group's deadline:
 *   1  queued group work completes; every rank's {n, flags, exact length} (one all-gather of three words
 *      per rank, read back), then, unless every n is 0, the requests themselves, padded to the longest n
 *      (a second all-gather, read back). Every rank now derives the whole plan as host arithmetic:
 *      the front and back totals F and Bk, every record's grant, first rank and offset in its asker's
 *      packed output.
 *   2  Member o peeks its min(F, len_o) smallest and min(Bk, len_o) largest entries without popping (a
 *      merge-path prefix and suffix of its two runs, one launch; NRG_SCAN_MAX_LIMIT does not apply); the
 *      candidate blocks (keys and values) are all-gathered, padded to the longest.
 *   3  One launch per member selects: a candidate's rank in the union is its index in its own list plus
 *      the candidates of every other list below (back: above) its key; rank < F (Bk) is popped; where the
 *      rank falls in one of this member's own records the entry is stored at its place under pop_cap.
 *      The same launch writes resp, some and *pop_n, counts the member's own popped candidates c_f and
 *      c_b and writes the records {c_f, front_mark}, {c_b, back_mark} into a device buffer.
 *   4  Every member replays those two device records with nrg_skiplist_round_async (origin rank + 1):
 *      its log moves by two records per call. Fronts and backs cannot meet inside a member because they
 *      do not meet in the union.
 * A one-rank group whose n <= max_batch skips 2 to 4: its own pop step (nrg_skiplist_round_pops_async
 * over the n records) answers straight into the caller's buffers (NRG_KNOB_EXP bit 16, measurement, makes
 * it take every step). The call returns when the answers are in the callers' buffers. Errors are agreed
 * on by every rank from step 1 before any data moves, the first in rank order wins, and the group stays
 * usable:
 *   NRG_E_INVAL       the group has not agreed on pops; members that are no skip lists; n > 0 with a NULL
 *                     reqs; resp without some or the reverse; pop_cap > 0 with a NULL array; a NULL pop_n
 *                     with n > 0; back > 1
 *   NRG_E_NOT_SYNCED  a member with ltail < tail
 *   NRG_E_CAPACITY    n >= 2^32; or G * (the longest n of the ranks) > 2^24 requests (their staging, on
 *                     every rank: 256 MiB); or G * (the longest candidate block, front and back candidates
 *                     together) > 2^27 entries (the scan's scratch bound)
 * NRG_E_COMM / NRG_E_TIMEOUT as nrg_group_verify. n = 0 on every rank returns NRG_OK after the exchange. */
typedef struct {
    uint64_t n;        /* PopFront x n (back = 0) or PopBack x n (back = 1) */
    uint32_t back;
    uint32_t reserved;
} nrg_pop_req;
typedef struct {
    const nrg_pop_req* reqs; /* host, this member's pop requests in issue order */
    uint64_t n;
    uint64_t* resp;          /* device, n: entries popped per request (nullable with some) */
    uint8_t* some;           /* device, n: resp >= 1 */
    uint64_t* pop_keys;      /* device: the popped entries, packed in request order, each */
    uint64_t* pop_vals;      /* request's in the order popped (front ascending, back descending) */
    uint64_t pop_cap;
    uint64_t* pop_n;         /* device: the total this member popped */
} nrg_pops;
int nrg_group_skiplist_pop(nrg_group* g, const nrg_pops* pops);

/* ---- device memory helpers (for callers without their own allocator) ----------------- */
int nrg_dev_alloc(nrg_ctx* ctx, uint64_t bytes, void** d_ptr);
int nrg_dev_free(nrg_ctx* ctx, void* d_ptr);
int nrg_memcpy_h2d(nrg_ctx* ctx, void* d_dst, const void* h_src, uint64_t bytes);
int nrg_memcpy_d2h(nrg_ctx* ctx, void* h_dst, const void* d_src, uint64_t bytes);

/* ---- synthetic workload generators (device side; identical streams to oracle/) -------- */
/* keys[i] = mulhi64(splitmix64_at(seed, i), span): uniform in [0, span). */
int nrg_gen_uniform_async(nrg_ctx* ctx, uint64_t* d_out, uint64_t n, uint64_t seed, uint64_t span);
/* raw splitmix64_at(seed, i) (values for Puts, push values after >> 32). */
int nrg_gen_raw_async(nrg_ctx* ctx, uint64_t* d_out, uint64_t n, uint64_t seed);
/* interleave: puts[i] = {keys[i], vals[i]} */
int nrg_gen_puts_async(nrg_ctx* ctx, nrg_put* d_out, const uint64_t* d_keys, const uint64_t* d_vals,
                       uint64_t n);
/* Zipf(theta) keys over [0, N) (Gray et al. SIGMOD'94 inverse CDF, ranks 1..N; scramble = 0:
 * key = rank-1 so hot keys are adjacent, 1: key = mix64(rank) % N). Statistically identical to
 * oracle/ orc_gen_zipf (device pow may differ from glibc's in the last ulp). theta != 1. */
int nrg_gen_zipf_async(nrg_ctx* ctx, uint64_t* d_out, uint64_t n, uint64_t seed, uint64_t N, double theta,
                       int scramble);
/* Stack ops as benches/stack.rs:87-102 with a seeded stream: r = splitmix64_at(seed, i),
 * op = r & 1 (1 = Push), val = r >> 32 (oracle/ orc_gen_stack_ops). */
int nrg_gen_stack_ops_async(nrg_ctx* ctx, nrg_stack_op* d_out, uint64_t n, uint64_t seed);

/* ---- timing: HIP events recorded around the dominant replay kernel -------------------- */
/* enable = 0: off; 1: every launch; n > 1: every n-th launch (sampling keeps the timed stream
 * unperturbed). The main replay kernel ("hm_round") is timed with start/stop events stamped
 * from its own dispatch (hipExtLaunchKernelGGL); multi-kernel pipelines ("hm_prev",
 * "st_replay", "sy_replay") with event records around them; a table growth's two passes are
 * "hm_grow_init" and "hm_rehash" (a purge's too: nrg_hashmap_purge and the automatic one), the
 * tombstone scan of nrg_hashmap_enable_removal and of a restore into an enabled context is
 * "hm_find_val", a snapshot's table scan "hm_snapshot", a restore's two passes
 * "hm_restore_init" and "hm_restore"; the skip list's chunk sort is "sl_sort" (event records around its
 * launches), its chunk merge "sl_merge" and a compaction of the delta run into the base run
 * "sl_compact" (one launch each: the launches counted are the compactions); its batched reads are
 * "sl_get", "sl_seek", "sl_range_count" and "sl_walk" (nrg_skiplist_scan: "sl_scan" is the chunk
 * replay's prefix scan); with removal enabled a chunk also has "sl_rm_resp" (the Removes' responses),
 * "sl_rm_state" (event records around the state readback) and, only when a run loses keys,
 * "sl_drop_base" / "sl_drop_delta"; the file store's chunk is "mf_expand", "mf_sort" (event records around the
 * slot sort's launches) and "mf_lines". nrg_kernel_time reads (timed
 * launches, their total milliseconds) after synchronising. */
int nrg_kernel_timing(nrg_ctx* ctx, int enable);
/* Restrict timing to one kernel name (NULL or "" = all). */
int nrg_kernel_timing_only(nrg_ctx* ctx, const char* which);
int nrg_kernel_time(nrg_ctx* ctx, const char* which, uint64_t* launches, double* total_ms);

#ifdef __cplusplus
}
#endif
#endif /* NRGPU_H */
