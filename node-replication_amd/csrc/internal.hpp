// internal.hpp — what the host-side files share: the context (nrg_ctx: the log and what every kind
// uses, the growth state (capacity.hpp), plus one state struct per owner, each touched by its owner's
// file alone), each kind's ops table (DsOps), the runtime helpers the structures' entry points use,
// and the few functions one structure's file uses of another's.
#pragma once

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/nrgpu.h"
#include "capacity.hpp"
#include "common.hpp"

namespace nrg {

// Scratch for the stable LSD radix sort of (u32 key, u32 value) pairs (radix_sort.hip).
struct SortScratch {
    u64 cap = 0;           // max elements
    u32* k[2] = {nullptr, nullptr};
    u32* v[2] = {nullptr, nullptr};
    u32* ctlmem = nullptr;  // [hist: 4*256][tickets: 64][desc: 4 * max_tiles * 256]
    u64 max_tiles = 0;
    u64 ctl_words = 0;
};

constexpr u32 SORT_TILE = 2048;  // keys per tile of a radix pass (radix_sort.hip)
int sort_alloc(SortScratch& s, u64 cap);
void sort_free(SortScratch& s);
// Sort n pairs by the low `key_bits` bits of key (stable). vals_in == nullptr means
// values are 0..n-1. Result pointers are returned (inside the scratch).
hipError_t sort_pairs(SortScratch& s, const u32* keys_in, const u32* vals_in, u64 n, int key_bits,
                      hipStream_t st, u32** out_k, u32** out_v);
// The same in two steps, for a caller that builds the digit histograms itself (fused into the
// pass that produces the keys): sort_prepare clears the control words and returns the
// [4][256] histogram array to add into; sort_run runs the digit passes.
hipError_t sort_prepare(SortScratch& s, u64 n, int key_bits, hipStream_t st, u32** hist);
hipError_t sort_run(SortScratch& s, const u32* keys_in, const u32* vals_in, u64 n, int key_bits, hipStream_t st,
                    u32** out_k, u32** out_v);

struct KTimer {
    std::vector<hipEvent_t> ev;  // pairs
    u64 pending = 0;             // recorded pairs not yet harvested
    u64 launches = 0;
    double total_ms = 0.0;
    u64 seen = 0;                // launches of this kernel since timing was enabled
    bool open = false;           // timer_begin recorded a start event not yet closed
};

struct Staging {  // growable device scratch for the host-pointer entry points
    void* p = nullptr;
    uint64_t bytes = 0;
};

// The second half of the last replayed hashmap round, run in the next launch (beside the next
// round's index pass) or by a flush: its reads and, for a stamp round, its apply.
struct HmDeferred {
    bool valid = false;
    u32 epoch = 0;
    bool apply = false;            // stamp round: the elected writers still store their values
    const nrg_put* src = nullptr;  // records: src[i] if set, else ring[(lo + i) & mask]
    u64 lo = 0, n = 0;
    const u64* keys = nullptr;     // the round's reads (R may be 0)
    u64 R = 0;
    u64* vals = nullptr;
    uint8_t* found = nullptr;
};

// A stack chunk whose finish (cross-tile Pops, commit) has not run yet (stack.hip).
struct StDeferred {
    bool valid = false;
    u64 lo = 0, n = 0;
    u32 tiles = 0, par = 0;
    u64 rlo = 0, rhi = 0;
    uint32_t* resp = nullptr;
    uint8_t* some = nullptr;
};

// A synthetic chunk whose bucket pass or per-op sums and hot-word fold have not run yet
// (synthetic.hip); its scratch slots follow from its epoch.
struct SyDeferred {
    bool valid = false;
    u32 epoch = 0;
    u64 lo = 0, n = 0;
    u32 ntiles = 0, want = 0, t0 = 0, t1 = 1;
    u64 rlo = 0, rhi = 0;
    u64* resp = nullptr;
    uint8_t* some = nullptr;
};

// The queue's device state, an allocation of its own (queue.hip): the ring position of the front
// as a monotonic count of elements ever popped, the length, and the same two at the start of the
// chunk being replayed with that chunk's successful Pops.
struct QuState {
    u64 head, len;
    u64 ck_head, ck_len, ck_pops;
};

// The page table's device state (vspace.hip): tables allocated from the pool, the PML4 included.
struct VsState {
    u64 ntables;
};

// The skip list's device state (skiplist.hip): keys in the base and in the delta run, and the delta
// count before the chunk being replayed with that chunk's new keys (what its merge reads). With removal
// enabled (nrg_skiplist_enable_removal) a chunk's scan also leaves the keys the chunk removes from each
// run: nb and nd_in are then already the counts after the drop passes the host launches next. A pop step
// (nrg_skiplist_enable_pops) leaves the counts after it the same way, ahead of the host's shifts.
struct SlState {
    u64 nb, nd;
    u64 nd_in, nnew;
    u64 kb, kd;
};

struct HostRun {  // origin tags of appended log ranges (the Entry::replica field)
    u64 first, count;
    u32 origin;
};

// ---- Host state of each owner, embedded in nrg_ctx. Only the owner's file touches its struct
// ---- (and allocates and frees its buffers); the runtime touches none of them. The growth state
// ---- (nrg_ctx::growth) is the runtime's: a kind's file runs the inline fast path on it before a
// ---- chunk and sets len_ub where it learns the exact count (init, restore, a compaction's re-read).

struct HmHost {  // NrHashMap (hashmap.hip)
    uint32_t slot_shift = 0;  // 64 - log2_slots
    uint64_t slots = 0;
    Slot* d_table = nullptr;
    // Table growth (hm_room / hm_grow): the table may grow to 2^grow_max_log2 slots (0: fixed);
    // keys_ub bounds the key count from above: the exact count when it was last taken plus every
    // Put replayed and every key prefilled since.
    uint32_t grow_max_log2 = 0;
    uint64_t keys_ub = 0;
    uint32_t k1_items = 0;  // Puts per index thread (0: by round size; NRG_KNOB_K1)
    // Reads of the last replayed round: answered in the next launch beside the next round's
    // index pass, or by nrg_join / nrg_sync / any call that reads the table. With
    // pipeline == false they are flushed at the end of every call.
    HmDeferred pend;
    uint64_t small_max = 0;         // rounds of <= small_max Puts take the one-launch small round
    uint64_t* d_created = nullptr;  // [HM_CREATED_SLOTS] keys created by replay rounds
    void* d_bk_ent = nullptr;       // partition rounds: [tiles][tile] 16-B {key, value} entries
    uint32_t* d_bk_idx = nullptr;   // partition rounds with previous values: [tiles][tile] round offset
    uint32_t* d_bk_cnt = nullptr;   // [index tiles][bucket] offset << 16 | count
    // Stamp rounds (<= stamp_max Puts, no previous values): per-Put slot ids by epoch parity.
    uint64_t stamp_max = 0;
    // Partition rounds (part_role + hm_papply_kernel), NRG_KNOB_PART: 1 (default) for previous
    // values, skewed streams and rounds of >= 393216 Puts; 2 for every round; 0 only where a stamp
    // round cannot (previous values, skew).
    uint32_t part_mode = 1;
    uint32_t pa_tpb = 0;       // NRG_KNOB_PA_TPB: partition-round apply workgroup width (0 = by round)
    uint64_t stamp_alloc = 0;  // Puts the put_slot arrays hold (stamp_max <= stamp_alloc)
    uint32_t epoch = 1;        // epoch of the last replay round (1: prefill / before any round)
    uint32_t epoch_limit = 0xFFFFFFF0u;  // renormalise stamps here (NRG_KNOB_EPOCH_LIMIT for tests)
    uint32_t* d_put_slot[2] = {nullptr, nullptr};
    // Key skew (hm_dup_sample_kernel): Puts combined inside their index block, sampled every
    // dup_every rounds into mapped host memory; a skewed stream takes partition rounds.
    uint64_t* d_dup = nullptr;           // [HM_DUP_SLOTS]
    volatile uint64_t* h_dup = nullptr;  // {seq, dups}, mapped pinned host memory
    uint64_t* h_dup_dev = nullptr;       // its device address
    uint64_t dup_seq = 0, dup_puts = 0, dup_puts_sampled = 0;
    uint64_t sample_seq = 0;      // a sample the next hm_round launch takes (0: none pending)
    uint32_t* err_out = nullptr;  // the next hm_round launch copies (and clears) the error latch here
    uint32_t dup_rounds = 0, dup_every = 16;
    bool skewed = false;
    // Removal (nrg_hashmap_enable_removal; off: none of the below exists and no round looks at it)
    bool removal = false;
    uint64_t tombstone = 0;      // a record whose val equals it is Remove(key); a slot whose val equals it is dead
    uint64_t* d_dead = nullptr;  // [HM_CREATED_SLOTS] slots that died minus slots revived (a wrapping sum)
};

struct StHost {  // stack (stack.hip)
    uint32_t* d_stack = nullptr;
    void* d_aux = nullptr;       // per-tile minima, last-Push tables and cross-tile Pops
    StDeferred pend;             // the last chunk's finish, if deferred
    uint32_t par = 0;            // buffer parity of the next chunk
    uint32_t* d_desc = nullptr;  // look-back descriptors of both parities (st_desc_words)
    uint64_t desc_words = 0;
};

struct SyHost {  // synthetic (synthetic.hip)
    uint64_t* d_words = nullptr;
    uint64_t* d_sort_aux = nullptr;  // per-touch max-scan output
    uint32_t key_bits = 0;
    void* d_aux = nullptr;       // bucket replay scratch; nullptr: sort path
    SyDeferred pend;             // the chunk whose sums are deferred, if any
    SyDeferred pend_b;           // one launch per round: the chunk whose bucket pass is deferred
    bool fused = true;           // one launch per round, chunks three deep (NRG_KNOB_SY_FUSED)
    uint32_t round = 0;          // chunks replayed (the chunk epoch: scratch slots, 32-bit seen values)
    uint64_t* d_tmp = nullptr;   // expand / sort scratch (max_batch * touches words)
    uint32_t* d_desc = nullptr;  // look-back descriptors of the max-scan
    uint64_t desc_words = 0;
};

struct QuHost {  // FIFO queue (queue.hip)
    uint64_t* d_queue = nullptr;  // ring of `size` (power of two >= capacity + max_batch) values
    uint64_t size = 0;
    QuState* d_state = nullptr;
    void* d_aux = nullptr;  // per-tile aggregates and scanned starts
};

struct VsHost {  // page table (vspace.hip)
    uint64_t* d_pool = nullptr;  // `cap` tables of 512 entries; table 0 is the PML4
    uint64_t cap = 0;
    VsState* d_state = nullptr;
    void* d_aux = nullptr;  // per-op scratch of one chunk
    uint64_t* d_tag = nullptr;  // the digest's tag per pool table, allocated by the first digest
};

struct SlHost {  // skip list / ordered map (skiplist.hip): two sorted runs with disjoint key sets
    uint64_t* d_bk[2] = {nullptr, nullptr};  // base keys, two buffers (a compaction writes the other one)
    uint64_t* d_bv[2] = {nullptr, nullptr};  // base values
    uint64_t* d_dk[2] = {nullptr, nullptr};  // delta keys (a chunk's merge writes the other one)
    uint64_t* d_dv[2] = {nullptr, nullptr};
    uint32_t bcur = 0, dcur = 0;             // the current buffer of each run
    uint64_t cap = 0;                        // keys the map holds (a base buffer's size)
    uint64_t delta_max = 0;                  // compact when the delta run holds more (NRG_KNOB_SL_DELTA_MAX)
    uint64_t dcap = 0;                       // a delta buffer's size: delta_max + max_batch
    SlState* d_state = nullptr;
    // scratch of one chunk
    uint64_t *d_sk = nullptr, *d_nk = nullptr, *d_nv = nullptr;
    uint32_t *d_sp = nullptr, *d_k32 = nullptr, *d_pv = nullptr, *d_tcnt = nullptr;
    uint8_t* d_miss = nullptr;
    // The compaction policy: nd_ub bounds the delta count from above, as Growth::len_ub bounds the key
    // count: the exact count when it was last read plus every record replayed since.
    uint64_t nd_ub = 0;
    // Removal (nrg_skiplist_enable_removal; off: none of the below exists and no chunk looks at it)
    bool removal = false;
    uint64_t tombstone = 0;       // a record whose val equals it is Remove(key)
    uint32_t* d_kidx = nullptr;   // [max_batch] where a surviving Remove found its key
    uint32_t* d_kcnt = nullptr;   // [2 * tiles] removed base / delta keys per tile, then their offsets
    uint32_t *d_deadb = nullptr, *d_deadd = nullptr;  // [max_batch] the chunk's dead indices of each run, ascending
    // Pops (nrg_skiplist_enable_pops; off: none of the below exists and no chunk looks at it)
    bool pops = false;
    uint64_t front_mark = 0, back_mark = 0;  // a record whose val equals one is PopFront x key / PopBack x key
    uint32_t* d_pfcnt = nullptr;  // [find tiles] the edges of pop runs in each tile of a chunk's positions
    uint32_t* d_pfev = nullptr;   // [find tiles * tile] their positions, compacted per tile
    uint64_t* d_poff = nullptr;   // [max_batch + 1] a pop step's output offsets per record
    uint64_t* d_prank = nullptr;  // [max_batch] a pop step's first rank per record, from the record's end
    uint64_t* d_pplan = nullptr;  // a pop step's plan (skiplist.hip SlPop::plan)
    std::vector<uint32_t> h_pf;   // the host's copy of d_pfcnt, then of the edges read
    // where the popped entries go, for the duration of one nrg_skiplist_round_pops_async (po_n == nullptr:
    // nowhere): the entries of pop records at log positions >= po_from, po_total of them so far
    uint64_t *po_keys = nullptr, *po_vals = nullptr, *po_n = nullptr;
    uint64_t po_cap = 0, po_from = 0, po_total = 0;
};

struct MfHost {  // file store (memfs.hip): F files of B = 2^log2_b bytes, contiguous in inode order
    uint8_t* d_files = nullptr;
    uint64_t files = 0;
    uint32_t log2_b = 0;
    uint32_t nlines = 0;    // F * B / 128: the 128-byte lines of the store; as a slot key, the sentinel
    uint32_t key_bits = 0;  // ceil(log2(nlines + 1)): what the slot sort sorts by
    // Capacity growth (nrg_set_max_capacity, sized contexts only; "Capacity growth" in memfs.hip)
    uint32_t max_log2 = 0;       // log2 of the bound in bytes per file (0: none, a fixed capacity)
    uint64_t* d_need = nullptr;  // the largest admitted end the need kernel has seen (made with the first bound)
    bool planned = false;        // the host planned the records being replayed and has grown: no need check
    // scratch of one chunk
    uint32_t* d_keys = nullptr;  // [2 * max_batch] slot keys
    uint64_t* d_desc = nullptr;  // [max_batch] record descriptors
    // scratch of one nrg_memfs_pread_async: [ceil(max_reads / 1024)] scan-tile aggregates
    uint64_t* d_pagg = nullptr;
    // scratch of one nrg_memfs_pread_repack_async, grown on demand: n + 1 source offsets, then aggregates
    uint64_t* d_rpk = nullptr;
    uint64_t rpk_words = 0;
    // Sizes (nrg_memfs_enable_sizes; nullptr: the context is unsized and none of the below exists)
    uint64_t* d_size = nullptr;  // [F] every file's size; stored bytes at or past it are zero
    uint32_t file_bits = 0;      // ceil(log2 F): what a sized chunk's file sort sorts by
    uint32_t epoch = 0;          // sized chunks replayed: stamps d_fm's entries
    bool unsized_image = false;  // nrg_restore loaded an unsized image: its digest comparison, the next
                                 // digest taken, leaves the size items out
    // scratch of one sized chunk
    uint32_t* d_fkey = nullptr;  // [max_batch] a record's file
    uint32_t* d_el = nullptr;    // [max_batch] a record's function on the size
    void* d_sc = nullptr;        // [max_batch] {size before the record, shrinks of its file before it}
    uint32_t* d_ev = nullptr;    // [max_batch] shrink targets, per file in log order
    void* d_fm = nullptr;        // [F] {first grouped position, shrinks, smallest target, new size}
    uint32_t* d_fep = nullptr;   // [F] the epoch of the chunk that wrote d_fm's entry
    void* d_sagg = nullptr;      // [max_batch / 1024 + 1] scan-tile aggregates
    // Writes of any length (nrg_memfs_pwrite*): made by the first such call, nullptr before
    // (and logged reads of any length, nrg_memfs_pread_logged*: [max_batch] requests of 3 words, then
    // first[max_batch + 1] and offs[max_batch + 1]; 5 * max_batch + 2 words hold either)
    uint64_t* d_rresp = nullptr; // logged reads: one pass's responses, [max_batch] of 136 bytes, then its
                                 // some bytes; made by the first nrg_memfs_pread_logged[_async]
    uint64_t* d_wup = nullptr;   // the upload: [max_batch] requests of 4 words, then first[max_batch + 1]
    uint64_t* h_wup = nullptr;   // its pinned host copy (the caller's requests may be reused on return)
    hipEvent_t ev_wup = nullptr; // the last upload has left h_wup
};

struct CombKnobs {  // read by nrg_combiner_open (combiner.cpp); NRG_KNOB_COMB_*
    int32_t spin = -1;    // -1 = default
    uint32_t depth = 0;   // 0 = default
    int32_t gather = -1;  // us; -1 = default
    int32_t serve = -1;   // -1 = default: on
    uint32_t open = 0;    // combiners open on the context (nrg_hashmap_enable_removal refuses while one is)
};

struct PtHost {  // key partitioning (partition.hip): tile counts / offsets, grown on demand
    void* d_buf = nullptr;
    uint64_t words = 0;
};

struct GenHost {  // workload generators (workload.hip): zeta(zipf_n, zipf_theta)
    uint64_t zipf_n = 0;
    double zipf_theta = 0.0, zipf_zetan = 0.0;
};

// What the runtime knows about a data structure: one table per kind, defined beside the
// structure's launchers and entry points (hashmap.hip, stack.hip, synthetic.hip, queue.hip,
// vspace.hip, skiplist.hip, memfs.hip).
struct DsOps {
    uint32_t rec_bytes;   // one log record
    uint32_t resp_bytes;  // one write response
    // validate c->cfg, allocate and initialise the structure; an NRG_* code (nrg_open closes the
    // context on failure, so nothing is released here)
    int (*open)(nrg_ctx* c);
    // free what open, and growth since, allocated; the context may be half-opened
    void (*close)(nrg_ctx* c);
    // launch the work the last replayed chunk deferred, if any (nullptr: a chunk defers nothing)
    hipError_t (*flush)(nrg_ctx* c);
    // replay the n records at log positions [lo, lo + n) (n <= max_batch): from the ring, or from
    // `src` if given, and then the ring copy is written too; write responses of [resp_lo, resp_hi)
    // into d_resp / d_some (nullptr: none wanted)
    hipError_t (*replay)(nrg_ctx* c, const void* src, u64 lo, u64 n, u64 resp_lo, u64 resp_hi, void* d_resp,
                         uint8_t* d_some);
    // the lowest log position the kind's deferred work still reads from the ring (<= ltail): the
    // log is collected up to here
    u64 (*floor)(const nrg_ctx* c);
    // nrg_test_set_knob for a knob the runtime does not own: NRG_OK, or NRG_E_INVAL for a knob the
    // kind does not have or a value out of range (nullptr: the kind has no knobs)
    int (*set_knob)(nrg_ctx* c, int knob, uint64_t v);
    // u64 words of the timestamp buffer NRG_KNOB_EXP bit 2 needs (nullptr: the kind stamps nothing)
    u64 (*dbg_words)(const nrg_ctx* c);
    // where the kind's nrg_config defaults differ from the common ones (nullptr: nowhere)
    void (*defaults)(nrg_config* cfg);
    // nrg_digest: zero d_out3 and add {count, sum, xor} of mix64(k ^ mix64(v)) over the structure's
    // items into it (common.hpp dg_item), on the context's stream, with nothing read on the host
    hipError_t (*digest)(nrg_ctx* c, u64* d_out3);
    // nrg_snapshot_size: the exact number of snapshot items (keys, elements, words, tables) of what
    // has been replayed, read from the device; synchronous, the stream has been drained
    int (*items)(nrg_ctx* c, u64* n);
    // nrg_snapshot_async: header words 0..4 (common.hpp snap_head) and the payload into d_buf, on
    // the context's stream, nothing stored at or past d_buf + cap; a state that does not fit writes
    // magic = 0 and latches ERR_CAPACITY. Deferred work has been launched.
    hipError_t (*snapshot)(nrg_ctx* c, void* d_buf, u64 cap, u64 log_idx);
    // nrg_restore. check_only: may a payload of `items` items go into this context? An NRG_* code,
    // nothing of the structure touched (the hashmap may read the payload on the stream and wait for it). Else: replace the structure's contents and rebuild its bookkeeping from the
    // payload (the stream has been drained, nothing is deferred). d_payload == nullptr: the empty
    // structure of a fresh context instead (after a restore whose digest did not match).
    int (*restore)(nrg_ctx* c, const void* d_payload, u64 items, bool check_only);
    // Capacity (capacity.hpp; null or zero: the kind has none the runtime drives). The exact item count
    // the policy reads is `items`.
    u64 cap_limit;                        // the largest capacity nrg_open accepts, inclusive
    u64 (*capacity)(const nrg_ctx* c);    // the current capacity, in items
    // reallocate to new_cap items (capacity < new_cap <= cap_limit), synchronously; if the allocation
    // fails nothing of it has been launched and the replica is as it was
    hipError_t (*grow)(nrg_ctx* c, u64 new_cap);
    bool auto_grow;  // grows under replay up to nrg_set_max_capacity's bound (else: nrg_*_reserve only)
    // nrg_set_max_capacity of a kind whose bound is not an item count (the file store: bytes per file),
    // in place of the runtime's own, which reads `items`; the stream has been drained (nullptr: an item
    // count, the runtime's)
    int (*set_bound)(nrg_ctx* c, u64 max);
};
const DsOps *hm_ops(), *st_ops(), *sy_ops(), *qu_ops(), *vs_ops(), *sl_ops(), *mf_ops();
const DsOps* ds_ops(uint32_t kind);  // runtime.cpp; nullptr for an unknown kind

}  // namespace nrg

// What every kind uses stays here; the rest is its owner's struct.
struct nrg_ctx {
    int device = 0;
    nrg_config cfg{};
    const nrg::DsOps* ops = nullptr;  // of cfg.ds_kind
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;

    // ---- Log (per-replica HBM ring) ----
    uint64_t log_size = 0;  // entries (power of two), as Log::new computes it
    uint64_t head = 0, tail = 0, ctail = 0, ltail = 0;
    uint32_t rec_bytes = 0;
    void* d_ring = nullptr;
    std::vector<nrg::HostRun> origins;

    nrg::DevCtl* d_ctl = nullptr;

    nrg::Growth growth;  // of the context's kind (stack, queue, skip list; the file store keeps its bound here)

    uint64_t rounds = 0;  // replay rounds launched (statistics)
    // set only through nrg_test_set_knob (include/nrgpu_testing.h)
    uint32_t exp = 0;       // NRG_KNOB_EXP: 2 phase timestamps, 0x10000 group.hpp pt_ident
    bool pipeline = false;  // a chunk's deferred work waits for the next launch, nrg_join or a sync
    uint32_t stall = 0;     // NRG_KNOB_STALL (tests): 1 odd waves sleep at LDS reuse points, 2 (synthetic,
                            // diagnostic: wrong results) without the bucket pass's tile-map barrier

    nrg::HmHost hm;
    nrg::StHost st;
    nrg::SyHost sy;
    nrg::QuHost qu;
    nrg::VsHost vs;
    nrg::SlHost sl;
    nrg::MfHost mf;
    nrg::CombKnobs comb;
    nrg::PtHost pt;
    nrg::GenHost gen;

    nrg::SortScratch sort;  // allocated by the synthetic's open, or on demand (nrg_test_sort_pairs)
    nrg::Staging stg[4];
    uint64_t* d_dbg = nullptr;  // diagnostic phase timestamps (NRG_KNOB_EXP), [tiles][16]
    uint64_t dbg_words = 0;     // u64 words d_dbg holds

    // ---- timing ----
    bool timing = false;
    uint32_t timing_every = 1;  // event-stamp every n-th launch (nrg_kernel_timing(ctx, n))
    std::string timing_only;  // if non-empty, only this kernel is timed
    std::map<std::string, nrg::KTimer> timers;
};

namespace nrg {
// timing helpers (runtime.cpp)
void timer_begin(nrg_ctx* c, const char* name, hipStream_t s = nullptr);
void timer_end(nrg_ctx* c, const char* name, hipStream_t s = nullptr);
// Event pair for one launch of kernel `name` when it is being timed (false otherwise). The
// pair is passed to hipExtLaunchKernelGGL, which stamps it from the kernel's own dispatch:
// no marker packets between kernels, so timing does not perturb the timed stream.
bool timer_events(nrg_ctx* c, const char* name, hipEvent_t* start, hipEvent_t* stop);

#define NRG_LAUNCH(CTX, NAME, KERNEL, GRID, BLOCK, SHMEM, STREAM, ...)                                  \
    do {                                                                                                \
        hipEvent_t nrg_e0_, nrg_e1_;                                                                    \
        if (timer_events((CTX), (NAME), &nrg_e0_, &nrg_e1_))                                            \
            hipExtLaunchKernelGGL((KERNEL), dim3(GRID), dim3(BLOCK), (SHMEM), (STREAM), nrg_e0_, nrg_e1_, 0, \
                                  __VA_ARGS__);                                                         \
        else                                                                                            \
            KERNEL<<<(GRID), (BLOCK), (SHMEM), (STREAM)>>>(__VA_ARGS__);                                \
    } while (0)
// make the context's device current for this thread (runtime.cpp; cached per thread)
int ctx_use_device(nrg_ctx* c);

// ---- what the structures' entry points use of the runtime (runtime.cpp) ----
// NRG_E_INVAL unless c is a context of `kind`; then its device is made current
int need(nrg_ctx* c, uint32_t kind);
hipError_t flush_deferred(nrg_ctx* c);  // launch what the last chunk deferred
hipError_t sync_all(nrg_ctx* c);        // flush_deferred and wait for the stream
int check_err(nrg_ctx* c);              // read and clear the device's error latch: an NRG_* code
// device scratch of the host-pointer entry points: grow slot st to `bytes`
int staging(Staging& st, uint64_t bytes);
// replay [ltail, min(tail, end)) in chunks of at most max_batch records
int exec_range(nrg_ctx* c, uint64_t resp_lo, uint64_t resp_hi, void* d_resp, uint8_t* d_some, uint64_t end = ~0ull);
int reserve(nrg_ctx* c, uint64_t n);  // room for n records (Log::append's GC path)
uint64_t append_max(const nrg_ctx* c);  // the longest append reserve accepts: log_size - GC_FROM_HEAD
void note_origin(nrg_ctx* c, uint64_t first, uint64_t n, uint32_t origin);
void commit_round(nrg_ctx* c, uint64_t lo, uint64_t n);  // [lo, lo + n) appended and replayed
// Replica::combine for one batch of a kind whose rounds carry no reads: one replay pass that also
// writes the log copy
int round_common(nrg_ctx* c, uint32_t kind, const void* d_ops, uint64_t n, uint32_t origin, void* d_resp,
                 uint8_t* d_some);
inline u64 floor_ltail(const nrg_ctx* c) { return c->ltail; }  // DsOps::floor of a kind that defers no ring reads
// The slow half of the growth policy, for a chunk of n records that growth_fits (capacity.hpp) did
// not pass: the exact count (DsOps::items: what the chunk deferred, a copy and a stream synchronise,
// timed as `timer` so that nrg_kernel_time counts the re-reads), the grow if exact + n does not fit,
// then len_ub = exact + n. On an error the growth state is untouched.
hipError_t room(nrg_ctx* c, u64 n, const char* timer);
// nrg_*_reserve and nrg_*_capacity of `kind`
int reserve_common(nrg_ctx* c, uint32_t kind, uint64_t n);
int capacity_common(nrg_ctx* c, uint32_t kind, uint64_t* out);
// The head of a growing kind's DsOps::restore. True: *r answers the call (check_only's answer, or a
// grow that failed). False: the structure holds *items items (0 without a payload): load them.
bool restore_room(nrg_ctx* c, const void* d_payload, u64* items, bool check_only, int* r);

inline int hip_fail(hipError_t e) {
    if (e == hipSuccess) return NRG_OK;
    if (e == hipErrorOutOfMemory) return NRG_E_NOMEM;
    return NRG_E_HIP;
}
#define HIPCHK(x)                                  \
    do {                                           \
        hipError_t _e = (x);                       \
        if (_e != hipSuccess) return hip_fail(_e); \
    } while (0)

inline uint64_t pow2_at_least(uint64_t x) {
    uint64_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

// ---- what one file uses of another ----
// hashmap.hip
hipError_t hm_replay_chunk(nrg_ctx* c, const void* src_recs, u64 lo, u64 n, bool write_ring,
                           const u64* d_get_keys, u64 R, u64* d_get_vals, uint8_t* d_get_found,
                           u64 resp_lo, u64 resp_hi, u64* d_prev, uint8_t* d_prev_found);
hipError_t hm_prefill_range(nrg_ctx* c, u64 n, u64 off, u32 part = 0, u32 parts = 1);
// Table growth. hm_room: every path calls it before it replays n Puts (or prefills n keys): it adds
// them to keys_ub and, when the load limit could be passed, counts the keys and grows the table
// (synchronously). With `due` given it launches nothing: when a count or a grow would be needed it
// sets *due, accounts nothing and returns (the combiner's round server must stop first).
hipError_t hm_room(nrg_ctx* c, u64 n, bool* due = nullptr);
// the flat combiner's round server (hashmap.hip hm_serve_kernel), in mapped host memory
// The host's words and the device's sit on separate 128-B lines: the GPU's L2 keeps host memory
// lines it has written, and a poll of a word on a line the server itself dirtied read that stale
// line (its buffer_inv keeps dirty lines), so the server never saw the next round.
constexpr uint32_t SERVE_SLOTS = 8;
struct ServeCtl {
    alignas(128) uint64_t door[SERVE_SLOTS];  // (host) slot k % NB: (k + 1) << 32 | Puts << 16 | Gets
    uint32_t stop;                            // (host) exit once every rung round is served
    alignas(128) uint64_t served;             // rounds served (device)
    uint64_t exited;                          // session of the last server that exited (device)
    uint64_t trace[4];                        // (diagnostic) -, round, doorbell seen, polls
};
// Gets per served round (4 per thread of the 1024: the resident loop's registers; the combiner
// launches rounds with more)
constexpr uint32_t SERVE_R = 4096;
struct SmallJobBlob {  // one small round's job (hashmap.hip SmallJob)
    alignas(16) unsigned char b[192];
};
bool hm_small_fill(nrg_ctx* c, const nrg_put* recs, u64 lo, u64 W, const u64* keys, u64 R, u64* vals, uint8_t* found,
                   u64* prev, uint8_t* prevf, u32* e_out, SmallJobBlob* blob);
// a round as nrg_hashmap_round_async would run it as a small round, its log bookkeeping
// done and nothing launched (the server runs it); *lo = its first log position. NRG_E_INVAL: not a
// small round of a caught-up replica. blob (optional): the round's whole job.
int hm_small_job(nrg_ctx* c, const nrg_put* recs, u64 W, u32 origin, const u64* keys, u64 R, u64* vals,
                 uint8_t* found, u64* prev, uint8_t* prevf, u32* e_out, SmallJobBlob* blob, u64* lo);
hipError_t hm_serve_launch(nrg_ctx* c, ServeCtl* sc, const SmallJobBlob* hdr, u32 nslots, u64 first, u64 first_lo,
                           u64 session, u64 idle_ticks);
// the replica group's partitioned rounds (partition.hip): one fused launch for the Puts and Get
// keys into owner regions of capacity cap_p / cap_k; counts[0, parts) Puts and [parts, 2 parts)
// Gets per owner, then the nxw host words xw; desc: pt_desc_words() look-back descriptors
constexpr u32 PT_XW_MAX = 8;
hipError_t pt_fused(hipStream_t s, const u64* puts, u64 W, u64 cap_p, u64* pout, u32* ppos, const u64* keys, u64 R,
                    u64 cap_k, u64* kout, u32* gpos, u64* desc, u32 parts, u32 epoch, u64* counts, const u64* xw,
                    u32 nxw);
u64 pt_desc_words(u64 W, u64 R, u32 parts);
hipError_t pt_route2(hipStream_t s, const u64* src_a, const uint8_t* src8_a, const u32* pos_a, u64 n_a, u64* dst_a,
                     uint8_t* dst8_a, const u64* src_b, const uint8_t* src8_b, const u32* pos_b, u64 n_b, u64* dst_b,
                     uint8_t* dst8_b);
void pt_close(nrg_ctx* c);  // partition.hip: free the partition scratch (the hashmap's and the file store's close)
// the file partition of file-store records (partition.hip; nrg_memfs_partition_async, group_files.cpp):
// out = the n records grouped by file_owner, compact, each group in issue order; pos[i] = where record i
// went; total[p] = records of owner p. On the context's stream; n < 2^32.
hipError_t fp_partition(nrg_ctx* c, const nrg_memfs_op* in, u64 n, u32 parts, nrg_memfs_op* out, u32* pos, u64* total);
// dst[i] = src[pos[i]], dst8[i] = src8[pos[i]] (either pair may be null)
hipError_t fp_route(nrg_ctx* c, const nrg_memfs_resp* src, const uint8_t* src8, const u32* pos, u64 n,
                    nrg_memfs_resp* dst, uint8_t* dst8);
// ... and of pread requests (nrg_memfs_rd_partition_async, group_file_reads.cpp): the same, 24-byte records
hipError_t rd_partition(nrg_ctx* c, const nrg_memfs_rd* in, u64 n, u32 parts, nrg_memfs_rd* out, u32* pos, u64* total);
// memfs.hip: the pread kernels over n < 2^32 requests in the caller's device buffers, on the context's
// stream (the replica group's group-wide pread; no max_reads bound: d_agg is the caller's scratch of
// mf_pread_agg_words(n) words).
u64 mf_pread_agg_words(u64 n);
u64 mf_pread_bound(const nrg_ctx* c, u64 n, u64 cap);  // the most bytes n requests can answer, or cap if that is less
// the scan: d_offs[0 .. n], d_some and, if given, every request's clipped length d_cnt
hipError_t mf_pread_scan_launch(nrg_ctx* c, const nrg_memfs_rd* d_reqs, u64 n, u64* d_offs, uint8_t* d_some, u64* d_cnt,
                                u64* d_agg);
// the copy of the scanned requests' bytes into d_data[0, min(cap, d_offs[n])); bound: what the host
// knows that minimum cannot exceed (the grid)
hipError_t mf_pread_copy_launch(nrg_ctx* c, const nrg_memfs_rd* d_reqs, u64 n, const u64* d_offs, uint8_t* d_data, u64 cap,
                                u64 bound);
// an owner's bytes per asker: d_out[s], s < G, from the offsets at the asker boundaries of its recvd requests
// (d_allcnt: every rank's exchange words, cw per rank, requests per owner first)
hipError_t mf_pread_totals_launch(nrg_ctx* c, const u64* d_offs, u64 recvd, const u64* d_allcnt, u32 G, u32 cw, u32 rank,
                                  u64* d_out);
// nrg_memfs_pread_repack_async's two halves: d_offs, d_some and d_src_offs[0 .. n] (scratch); then the bytes
hipError_t mf_repack_scan_launch(nrg_ctx* c, const u64* d_src_cnt, const uint8_t* d_src_some, const u32* d_pos, u64 n,
                                 u64* d_offs, uint8_t* d_some, u64* d_src_offs, u64* d_agg);
hipError_t mf_repack_copy_launch(nrg_ctx* c, const uint8_t* d_src, const u64* d_src_offs, const u32* d_pos, u64 n,
                                 const u64* d_offs, uint8_t* d_data, u64 cap, u64 bound);
// hashmap.hip: the log's segment copy (nrg_log_append_segments_async)
hipError_t copy_segments(nrg_ctx* c, const void* d_base, u32 nseg, u64 seg_stride, const u64* lens,
                         u64 dst_lo);
// skiplist.hip: the seek, range-count and scan kernels over n < 2^32 queries in the caller's device
// buffers, on the context's stream (the replica group's group-wide reads; no max_reads bound)
hipError_t sl_seek_launch(nrg_ctx* c, const u64* d_keys, u64 n, u32 mode, u64* d_okeys, u64* d_ovals, uint8_t* d_found);
hipError_t sl_count_launch(nrg_ctx* c, const u64* d_los, const u64* d_his, u64 n, u64* d_counts);
hipError_t sl_walk_launch(nrg_ctx* c, const u64* d_keys, u64 n, u32 mode, u32 limit, u64* d_okeys, u64* d_ovals,
                          u32* d_counts);
// ... and a member's candidates of a group-wide pop (group_pops.cpp): its nf smallest entries ascending,
// its nk largest descending, nothing popped
hipError_t sl_peek_launch(nrg_ctx* c, u64 nf, u64 nk, u64* d_fk, u64* d_fv, u64* d_kk, u64* d_kv);
bool hm_removal(const nrg_ctx* c);  // hashmap.hip: nrg_hashmap_enable_removal was called (nrg_combiner_open refuses)
bool sl_removal(const nrg_ctx* c);  // nrg_skiplist_enable_removal was called (group_partitioned.cpp refuses such a member,
                                    // unless its group agreed on removal)
bool sl_pops(const nrg_ctx* c);     // nrg_skiplist_enable_pops was called (likewise: the front is group-wide, group_pops.cpp)
// queue.hip
hipError_t qu_len_answers(nrg_ctx* c, u32 n, u64* d_out, uint8_t* d_some);  // n Len reads (the combiner)
}  // namespace nrg
