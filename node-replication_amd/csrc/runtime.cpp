// runtime.cpp — the log and the context: replica lifetime and streams, the per-replica HBM log
// ring with the reference's head/tail/ctail/ltail bookkeeping (the nrg_log_* calls), dispatch of
// the replay pipelines through each structure's ops table, timing and the device-memory helpers.
// Everything about one data structure, its entry points included, is in its own file
// (hashmap.hip, stack.hip, synthetic.hip, queue.hip, vspace.hip, skiplist.hip, memfs.hip); nothing here names a kind
// except ds_ops and one open-time check.
//
// Log bookkeeping follows nr/src/log.rs: Log::new sizing (:179-242), append with GC when
// fewer than GC_FROM_HEAD entries would remain (:343-427, :536-580), exec of
// [ltail, tail) (:473-524) followed by ctail = max(ctail, tail) and ltail = tail (:522-523).
// Each GPU context holds its own copy of the shared log (the all-gather of write segments
// makes every copy identical), so head = min over replicas = this ltail.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>

#include "internal.hpp"
#include "../../include/nrgpu_testing.h"

using namespace nrg;

namespace {

constexpr uint64_t GC_FROM_HEAD = 32 * 256;  // MAX_PENDING_OPS * MAX_THREADS_PER_REPLICA
constexpr uint64_t ENTRY_BYTES = 64;         // size_of::<Entry<T>>() in the reference
constexpr uint64_t DEFAULT_LOG_BYTES = 32ull << 20;

thread_local int g_dev_set = -1;

int use_device(nrg_ctx* c) {
    if (g_dev_set != c->device) {
        HIPCHK(hipSetDevice(c->device));
        g_dev_set = c->device;
    }
    return NRG_OK;
}

// Log GC boundary: the slowest replica's tail (this replica's ltail), held back to the first
// record the kind's deferred work still reads from the ring.
uint64_t gc_head(const nrg_ctx* c) { return std::min<uint64_t>(c->ltail, c->ops->floor(c)); }

}  // namespace

// ---- shared with the structures' entry points (internal.hpp) ---------------------------------
namespace nrg {
int ctx_use_device(nrg_ctx* c) { return use_device(c); }

int need(nrg_ctx* c, uint32_t kind) {
    if (!c) return NRG_E_INVAL;
    if (c->cfg.ds_kind != kind) return NRG_E_INVAL;
    return use_device(c);
}

// what the last replayed chunk deferred (a round's reads, a chunk's finish or sums), launched now
// if there is any
hipError_t flush_deferred(nrg_ctx* c) { return c->ops->flush ? c->ops->flush(c) : hipSuccess; }

// wait for everything queued on this replica, including what the last chunk deferred
hipError_t sync_all(nrg_ctx* c) {
    hipError_t e = flush_deferred(c);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(c->stream);
}

int check_err(nrg_ctx* c) {
    uint32_t err = 0;
    HIPCHK(hipMemcpyAsync(&err, &c->d_ctl->err, sizeof(err), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_all(c));
    if (err) {
        uint32_t z = 0;
        HIPCHK(hipMemcpyAsync(&c->d_ctl->err, &z, sizeof(z), hipMemcpyHostToDevice, c->stream));
        HIPCHK(sync_all(c));
        if (err & ERR_TABLE_FULL) return NRG_E_TABLE_FULL;
        if (err & ERR_CAPACITY) return NRG_E_CAPACITY;
        if (err & ERR_GROUP) return NRG_E_INVAL;
        if (err & ERR_INVAL) return NRG_E_INVAL;
        return NRG_E_HIP;
    }
    return NRG_OK;
}

// replay [ltail, tail) in order, in chunks of at most max_batch records; with `end` given, only
// up to there (a caller that replays the last chunk itself)
int exec_range(nrg_ctx* c, uint64_t resp_lo, uint64_t resp_hi, void* d_resp, uint8_t* d_some, uint64_t end) {
    if (end > c->tail) end = c->tail;
    while (c->ltail < end) {
        uint64_t n = end - c->ltail;
        if (n > c->cfg.max_batch) n = c->cfg.max_batch;
        const uint64_t lo = c->ltail;
        HIPCHK(c->ops->replay(c, nullptr, lo, n, resp_lo, resp_hi, d_resp, d_some));
        c->ltail = lo + n;
    }
    if (c->ctail < c->ltail) c->ctail = c->ltail;
    return NRG_OK;
}

// a round appended and replayed in one go (Log::append + Log::exec of [lo, lo + n))
void commit_round(nrg_ctx* c, uint64_t lo, uint64_t n) {
    c->tail = lo + n;
    c->ltail = c->tail;
    if (c->ctail < c->tail) c->ctail = c->tail;
}

// Make room for n records (Log::append's GC path): advance head to the slowest replica's
// tail (this replica's ltail), replaying first if nothing can be freed.
int reserve(nrg_ctx* c, uint64_t n) {
    if (n > c->log_size - GC_FROM_HEAD) return NRG_E_RING_FULL;
    if (c->tail + n > c->head + c->log_size - GC_FROM_HEAD) {
        c->head = gc_head(c);
        if (c->tail + n > c->head + c->log_size - GC_FROM_HEAD) {
            int r = exec_range(c, 0, 0, nullptr, nullptr);
            if (r != NRG_OK) return r;
            HIPCHK(flush_deferred(c));
            c->head = gc_head(c);
        }
    }
    return NRG_OK;
}

uint64_t append_max(const nrg_ctx* c) { return c->log_size - GC_FROM_HEAD; }

void note_origin(nrg_ctx* c, uint64_t first, uint64_t n, uint32_t origin) {
    if (!c->origins.empty()) {
        HostRun& b = c->origins.back();
        if (b.origin == origin && b.first + b.count == first) {
            b.count += n;
            return;
        }
    }
    c->origins.push_back(HostRun{first, n, origin});
    // keep only runs that are still inside the live window
    size_t drop = 0;
    while (drop < c->origins.size() && c->origins[drop].first + c->origins[drop].count <= c->head) drop++;
    if (drop) c->origins.erase(c->origins.begin(), c->origins.begin() + drop);
}

static int copy_into_ring(nrg_ctx* c, const void* src, uint64_t n, hipMemcpyKind kind) {
    const uint64_t phys = c->tail & (c->log_size - 1);
    const uint64_t first = n < c->log_size - phys ? n : c->log_size - phys;
    char* ring = (char*)c->d_ring;
    const char* s = (const char*)src;
    HIPCHK(hipMemcpyAsync(ring + phys * c->rec_bytes, s, first * c->rec_bytes, kind, c->stream));
    if (first < n)
        HIPCHK(hipMemcpyAsync(ring, s + first * c->rec_bytes, (n - first) * c->rec_bytes, kind, c->stream));
    return NRG_OK;
}

int staging(Staging& st, uint64_t bytes) {
    if (st.bytes >= bytes) return NRG_OK;
    if (st.p) (void)hipFree(st.p);
    st.p = nullptr;
    st.bytes = 0;
    uint64_t b = bytes < 4096 ? 4096 : bytes;
    HIPCHK(hipMalloc(&st.p, b));
    st.bytes = b;
    return NRG_OK;
}

// Replica::combine for one batch of a stack, synthetic, queue, page-table, skip-list or file-store replica: one replay pass that
// also writes the log copy (Log::append + Log::exec of this batch)
int round_common(nrg_ctx* c, uint32_t kind, const void* d_ops, uint64_t n, uint32_t origin, void* d_resp,
                 uint8_t* d_some) {
    int r = need(c, kind);
    if (r) return r;
    if (n > c->cfg.max_batch) return NRG_E_CAPACITY;
    if (n && !d_ops) return NRG_E_INVAL;
    if (!d_resp || !d_some) d_resp = nullptr, d_some = nullptr;
    // catch up on anything appended by others first (Replica::combine execs the whole log)
    if ((r = exec_range(c, 0, 0, nullptr, nullptr))) return r;
    if ((r = reserve(c, n))) return r;
    const uint64_t lo = c->tail;
    HIPCHK(c->ops->replay(c, d_ops, lo, n, lo, lo + n, d_resp, d_some));
    if (n) note_origin(c, lo, n, origin);
    commit_round(c, lo, n);
    return NRG_OK;
}

// ---- capacity and growth (capacity.hpp), driven through the kind's DsOps ------------------------
hipError_t room(nrg_ctx* c, u64 n, const char* timer) {
    const DsOps* o = c->ops;
    u64 exact = 0;
    timer_begin(c, timer);
    const int r = o->items(c, &exact);
    timer_end(c, timer);
    if (r != NRG_OK) return r == NRG_E_NOMEM ? hipErrorOutOfMemory : hipErrorUnknown;
    const u64 cap = o->capacity(c), to = growth_target(c->growth, cap, exact + n);
    hipError_t e;
    if (to != cap && (e = o->grow(c, to)) != hipSuccess) return e;
    c->growth.len_ub = exact + n;
    return hipSuccess;
}

// nrg_set_max_capacity of a kind that grows under replay: the bound, and the count bound restarts
// from the exact count. The stream has been drained.
static int set_max(nrg_ctx* c, u64 max_items) {
    if (!growth_bound_ok(max_items, c->ops->capacity(c), c->ops->cap_limit)) return NRG_E_INVAL;
    u64 exact = 0;
    int r = c->ops->items(c, &exact);
    if (r) return r;
    c->growth = Growth{max_items, exact};
    return NRG_OK;
}

int reserve_common(nrg_ctx* c, uint32_t kind, uint64_t n) {
    int r = need(c, kind);
    if (r) return r;
    if (n > c->ops->cap_limit) return NRG_E_INVAL;  // nrg_open's bound
    if (n <= c->ops->capacity(c)) return NRG_OK;    // never shrinks
    HIPCHK(c->ops->grow(c, n));
    return NRG_OK;
}

int capacity_common(nrg_ctx* c, uint32_t kind, uint64_t* out) {  // no device is touched
    if (!c || !out || c->cfg.ds_kind != kind) return NRG_E_INVAL;
    *out = c->ops->capacity(c);
    return NRG_OK;
}

bool restore_room(nrg_ctx* c, const void* d_payload, u64* items, bool check_only, int* r) {
    const u64 cap = c->ops->capacity(c);
    *r = NRG_OK;
    if (check_only) {
        if (!growth_admits(c->growth, cap, *items)) *r = NRG_E_CAPACITY;
        return true;
    }
    if (!d_payload) *items = 0;
    if (*items > cap) *r = hip_fail(c->ops->grow(c, growth_target(c->growth, cap, *items)));
    return *r != NRG_OK;
}

const DsOps* ds_ops(uint32_t kind) {
    switch (kind) {
        case NRG_DS_HASHMAP: return hm_ops();
        case NRG_DS_STACK: return st_ops();
        case NRG_DS_SYNTHETIC: return sy_ops();
        case NRG_DS_QUEUE: return qu_ops();
        case NRG_DS_VSPACE: return vs_ops();
        case NRG_DS_SKIPLIST: return sl_ops();
        case NRG_DS_MEMFS: return mf_ops();
        default: return nullptr;
    }
}

// c->timing_only: empty (time every kernel) or a comma-separated list of kernel names
static bool timer_match(const nrg_ctx* c, const char* name) {
    if (c->timing_only.empty()) return true;
    const std::string& w = c->timing_only;
    const size_t n = std::strlen(name);
    for (size_t p = 0; (p = w.find(name, p)) != std::string::npos; p++)
        if ((p == 0 || w[p - 1] == ',') && (p + n == w.size() || w[p + n] == ',')) return true;
    return false;
}
// HIP events around a kernel, recorded on the stream that kernel is launched on. When
// c->timing_only is set, only the kernels it names are bracketed (keeps event packets off
// the others).
void timer_begin(nrg_ctx* c, const char* name, hipStream_t s) {
    if (!c->timing || !timer_match(c, name)) return;
    KTimer& t = c->timers[name];
    t.open = false;
    if (++t.seen % c->timing_every != 0) return;  // sampled, as timer_events
    const size_t idx = t.pending * 2;
    while (t.ev.size() < idx + 2) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        t.ev.push_back(e);
    }
    (void)hipEventRecord(t.ev[idx], s ? s : c->stream);
    t.open = true;
}
bool timer_events(nrg_ctx* c, const char* name, hipEvent_t* start, hipEvent_t* stop) {
    if (!c->timing || !timer_match(c, name)) return false;
    KTimer& t = c->timers[name];
    // sampled: launches every-1, 2*every-1, ... (skips a stream's first launch when every > 1)
    if (++t.seen % c->timing_every != 0) return false;
    const size_t idx = t.pending * 2;
    while (t.ev.size() < idx + 2) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return false;
        t.ev.push_back(e);
    }
    *start = t.ev[idx];
    *stop = t.ev[idx + 1];
    t.pending++;
    return true;
}
void timer_end(nrg_ctx* c, const char* name, hipStream_t s) {
    if (!c->timing || !timer_match(c, name)) return;
    KTimer& t = c->timers[name];
    if (!t.open) return;
    (void)hipEventRecord(t.ev[t.pending * 2 + 1], s ? s : c->stream);
    t.pending++;
    t.open = false;
}
}  // namespace nrg

extern "C" {

void nrg_config_default(nrg_config* cfg, uint32_t ds_kind) {
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->ds_kind = ds_kind;
    cfg->log2_slots = 26;
    cfg->log_bytes = DEFAULT_LOG_BYTES;
    cfg->max_batch = 1u << 20;
    cfg->max_reads = 1u << 20;
    cfg->stack_capacity = 1u << 24;
    cfg->synth_n = 200000;
    cfg->synth_cold_reads = 20;
    cfg->synth_cold_writes = 5;
    cfg->synth_hot_reads = 2;
    cfg->synth_hot_writes = 1;
    cfg->stack_push_resp = 0;
    cfg->replica_id = 1;
    cfg->pipeline = 0;  // opt-in: see nrg_config.pipeline
    cfg->queue_capacity = 1u << 24;
    const DsOps* ops = ds_ops(ds_kind);
    if (ops && ops->defaults) ops->defaults(cfg);
}

const char* nrg_strerror(int code) {
    switch (code) {
        case NRG_OK: return "ok";
        case NRG_E_INVAL: return "invalid argument";
        case NRG_E_HIP: return "HIP runtime error";
        case NRG_E_TABLE_FULL: return "hash table full";
        case NRG_E_RING_FULL: return "log ring full";
        case NRG_E_NOMEM: return "device out of memory";
        case NRG_E_NOT_SYNCED: return "replica not synced to the log tail";
        case NRG_E_CAPACITY: return "capacity exceeded";
        case NRG_E_NODEV: return "no such HIP device";
        case NRG_E_COMM: return "RCCL unavailable or a collective failed";
        case NRG_E_TIMEOUT: return "a peer rank missed the replica group's deadline for a collective";
        default: return "unknown error";
    }
}

const char* nrg_version(void) { return "nrgpu 0.2 gfx950"; }

int nrg_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int nrg_close(nrg_ctx* c);

// nrg_open's allocations: the stream, the log ring and DevCtl, then the structure's own
static int open_buffers(nrg_ctx* c) {
    HIPCHK(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    // Log::new(bytes): entries = bytes / 64, at least 2*GC_FROM_HEAD, power of two.
    uint64_t num = (c->cfg.log_bytes ? c->cfg.log_bytes : DEFAULT_LOG_BYTES) / ENTRY_BYTES;
    if (num < 2 * GC_FROM_HEAD) num = 2 * GC_FROM_HEAD;
    c->log_size = pow2_at_least(num);
    HIPCHK(hipMalloc(&c->d_ring, c->log_size * c->rec_bytes));
    HIPCHK(hipMalloc(&c->d_ctl, sizeof(DevCtl)));
    HIPCHK(hipMemsetAsync(c->d_ctl, 0, sizeof(DevCtl), c->stream));
    int r = c->ops->open(c);
    if (r != NRG_OK) return r;
    HIPCHK(hipStreamSynchronize(c->stream));
    return NRG_OK;
}

int nrg_open(int dev, const nrg_config* cfg_in, nrg_ctx** out) {
    if (!cfg_in || !out) return NRG_E_INVAL;
    *out = nullptr;
    const DsOps* ops = ds_ops(cfg_in->ds_kind);
    if (!ops) return NRG_E_INVAL;
    // table growth (0: a fixed table): up to a size nrg_open accepts for log2_slots, never below it
    if (cfg_in->ds_kind == NRG_DS_HASHMAP && cfg_in->hashmap_max_log2_slots &&
        (cfg_in->hashmap_max_log2_slots < cfg_in->log2_slots || cfg_in->hashmap_max_log2_slots > 30))
        return NRG_E_INVAL;
    int ndev = nrg_device_count();
    if (dev < 0 || dev >= ndev) return NRG_E_NODEV;
    nrg_ctx* c = new (std::nothrow) nrg_ctx();
    if (!c) return NRG_E_NOMEM;
    c->device = dev;
    c->cfg = *cfg_in;
    c->ops = ops;
    nrg_config& cf = c->cfg;
    nrg_config def;  // a zero max_batch or max_reads means the kind's default
    nrg_config_default(&def, cf.ds_kind);
    if (!cf.max_batch) cf.max_batch = def.max_batch;
    if (!cf.max_reads) cf.max_reads = def.max_reads;
    if (!cf.replica_id) cf.replica_id = 1;
    if (cf.max_batch >= (1ull << 30)) { delete c; return NRG_E_INVAL; }
    c->rec_bytes = ops->rec_bytes;
    g_dev_set = -1;
    int rc = use_device(c);
    if (rc != NRG_OK) { delete c; return rc; }
    rc = open_buffers(c);
    if (rc != NRG_OK) {
        nrg_close(c);
        return rc;
    }
    *out = c;
    return NRG_OK;
}

int nrg_close(nrg_ctx* c) {
    if (!c) return NRG_E_INVAL;
    (void)hipSetDevice(c->device);
    g_dev_set = c->device;
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    if (c->stream && c->stream != c->own_stream) (void)hipStreamSynchronize(c->stream);
    // what every kind shares; each structure frees its own buffers
    void* ptrs[] = {c->d_ring, c->d_ctl, c->d_dbg};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    sort_free(c->sort);
    c->ops->close(c);
    Staging* s = c->stg;
    for (int i = 0; i < 4; i++)
        if (s[i].p) (void)hipFree(s[i].p);
    for (auto& kv : c->timers)
        for (hipEvent_t e : kv.second.ev) (void)hipEventDestroy(e);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return NRG_OK;
}

int nrg_set_stream(nrg_ctx* c, void* s) {
    if (!c) return NRG_E_INVAL;
    int r = use_device(c);
    if (r) return r;
    // deferred work belongs to the old stream: launch it there first
    hipError_t e = flush_deferred(c);
    if (e != hipSuccess) return hip_fail(e);
    hipStream_t ns = (hipStream_t)s;  // NULL: the device's null stream, as in HIP
    if (ns != c->stream) {
        // everything already queued on the old stream (the replica's table, ring and scratch)
        // comes before anything the new stream runs from now on
        hipEvent_t ev;
        HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        e = hipEventRecord(ev, c->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(ns, ev, 0);
        (void)hipEventDestroy(ev);
        if (e != hipSuccess) return hip_fail(e);
    }
    c->stream = ns;
    return NRG_OK;
}

void* nrg_get_stream(nrg_ctx* c) { return c ? (void*)c->stream : nullptr; }

void* nrg_own_stream(nrg_ctx* c) { return c ? (void*)c->own_stream : nullptr; }

int nrg_sync(nrg_ctx* c) {
    if (!c) return NRG_E_INVAL;
    int r = use_device(c);
    if (r) return r;
    HIPCHK(sync_all(c));
    return check_err(c);
}

// The bound of a kind that grows under replay as its reference structure does (Vec, SegQueue), in
// the kind's items (DsOps::auto_grow), or in the kind's own unit through DsOps::set_bound.
int nrg_set_max_capacity(nrg_ctx* c, uint64_t max_items) {
    if (!c || !c->ops->auto_grow) return NRG_E_INVAL;
    int r = use_device(c);
    if (r) return r;
    HIPCHK(sync_all(c));
    return c->ops->set_bound ? c->ops->set_bound(c, max_items) : set_max(c, max_items);
}

int nrg_join(nrg_ctx* c) {
    if (!c) return NRG_E_INVAL;
    int r = use_device(c);
    if (r) return r;
    HIPCHK(flush_deferred(c));
    return NRG_OK;
}

// Replica::verify (nr/src/replica.rs:443-467) without the state leaving the device: the kind's
// digest of what has been replayed so far, after what the last chunk deferred.
int nrg_digest_async(nrg_ctx* c, uint64_t* d_out3) {
    if (!c || !d_out3) return NRG_E_INVAL;
    int r = use_device(c);
    if (r) return r;
    HIPCHK(flush_deferred(c));
    HIPCHK(c->ops->digest(c, d_out3));
    return NRG_OK;
}

int nrg_digest(nrg_ctx* c, uint64_t out[3]) {
    if (!c || !out) return NRG_E_INVAL;
    int r = use_device(c);
    if (r) return r;
    if ((r = staging(c->stg[3], 64))) return r;
    if ((r = nrg_digest_async(c, (uint64_t*)c->stg[3].p))) return r;
    HIPCHK(hipMemcpyAsync(out, c->stg[3].p, 24, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_all(c));
    return check_err(c);
}

// ---- Log -------------------------------------------------------------------------------
static int append_common(nrg_ctx* c, const void* recs, uint64_t n, uint32_t origin, uint64_t* first_idx,
                         hipMemcpyKind kind) {
    if (!c || (!recs && n)) return NRG_E_INVAL;
    int r = use_device(c);
    if (r) return r;
    if (n == 0) {
        if (first_idx) *first_idx = c->tail;
        return NRG_OK;
    }
    if ((r = reserve(c, n)) != NRG_OK) return r;
    if ((r = copy_into_ring(c, recs, n, kind)) != NRG_OK) return r;
    if (first_idx) *first_idx = c->tail;
    note_origin(c, c->tail, n, origin);
    c->tail += n;
    return NRG_OK;
}

int nrg_log_append(nrg_ctx* c, const void* recs, uint64_t n, uint32_t origin, uint64_t* first_idx) {
    int r = append_common(c, recs, n, origin, first_idx, hipMemcpyHostToDevice);
    if (r) return r;
    HIPCHK(sync_all(c));
    return NRG_OK;
}

int nrg_log_append_async(nrg_ctx* c, const void* d_recs, uint64_t n, uint32_t origin, uint64_t* first_idx) {
    return append_common(c, d_recs, n, origin, first_idx, hipMemcpyDeviceToDevice);
}

int nrg_log_append_segments_async(nrg_ctx* c, const void* d_base, uint32_t nseg, uint64_t seg_stride,
                                  const uint64_t* lens, const uint32_t* origins, uint64_t* first_idx) {
    if (!c || !lens || nseg == 0 || nseg > 64) return NRG_E_INVAL;
    int r = use_device(c);
    if (r) return r;
    uint64_t total = 0;
    for (uint32_t s = 0; s < nseg; s++) {
        if (lens[s] > seg_stride) return NRG_E_INVAL;
        total += lens[s];
    }
    if ((r = reserve(c, total)) != NRG_OK) return r;
    hipError_t e = copy_segments(c, d_base, nseg, seg_stride, lens, c->tail);
    if (e != hipSuccess) return hip_fail(e);
    for (uint32_t s = 0; s < nseg; s++) {
        if (first_idx) first_idx[s] = c->tail;
        if (lens[s]) note_origin(c, c->tail, lens[s], origins ? origins[s] : s + 1);
        c->tail += lens[s];
    }
    return NRG_OK;
}

int nrg_log_exec_async(nrg_ctx* c, uint64_t resp_lo, uint64_t resp_hi, void* d_resp, uint8_t* d_some) {
    if (!c || resp_hi < resp_lo) return NRG_E_INVAL;
    int r = use_device(c);
    if (r) return r;
    if (!d_resp || !d_some) {
        d_resp = nullptr;
        d_some = nullptr;
    }
    return exec_range(c, resp_lo, resp_hi, d_resp, d_some);
}

int nrg_log_exec(nrg_ctx* c, uint64_t resp_lo, uint64_t resp_hi, void* resp, uint8_t* some) {
    if (!c || resp_hi < resp_lo) return NRG_E_INVAL;
    int r = use_device(c);
    if (r) return r;
    const uint64_t w = (resp && some) ? resp_hi - resp_lo : 0;
    void* dr = nullptr;
    uint8_t* ds = nullptr;
    Staging* s = c->stg;
    const uint64_t eb = c->ops->resp_bytes;
    if (w) {
        if ((r = staging(s[0], w * eb)) || (r = staging(s[1], w))) return r;
        dr = s[0].p;
        ds = (uint8_t*)s[1].p;
        HIPCHK(hipMemsetAsync(dr, 0, w * eb, c->stream));
        HIPCHK(hipMemsetAsync(ds, 0, w, c->stream));
    }
    if ((r = exec_range(c, resp_lo, resp_hi, dr, ds))) return r;
    HIPCHK(flush_deferred(c));  // deferred work writes responses too: complete them before the copy
    if (w) {
        HIPCHK(hipMemcpyAsync(resp, dr, w * eb, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(some, ds, w, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(sync_all(c));
    return check_err(c);
}

int nrg_log_state(const nrg_ctx* c, nrg_log_info* o) {
    if (!c || !o) return NRG_E_INVAL;
    o->size = c->log_size;
    o->head = c->head;
    o->tail = c->tail;
    o->ctail = c->ctail;
    o->ltail = c->ltail;
    o->replica_id = c->cfg.replica_id;
    o->ds_kind = c->cfg.ds_kind;
    return NRG_OK;
}

int nrg_log_reset(nrg_ctx* c) {
    if (!c) return NRG_E_INVAL;
    int r = use_device(c);
    if (r) return r;
    // deferred work (reads, a chunk's finish or sums) belongs to the log positions being reset: run it now
    HIPCHK(flush_deferred(c));
    c->head = c->tail = c->ctail = c->ltail = 0;
    c->origins.clear();
    return NRG_OK;
}

// ---- device memory helpers -----------------------------------------------------------------
int nrg_dev_alloc(nrg_ctx* c, uint64_t bytes, void** p) {
    if (!c || !p) return NRG_E_INVAL;
    int r = use_device(c);
    if (r) return r;
    HIPCHK(hipMalloc(p, bytes ? bytes : 1));
    return NRG_OK;
}
int nrg_dev_free(nrg_ctx* c, void* p) {
    if (!c) return NRG_E_INVAL;
    int r = use_device(c);
    if (r) return r;
    HIPCHK(sync_all(c));
    HIPCHK(hipFree(p));
    return NRG_OK;
}
int nrg_memcpy_h2d(nrg_ctx* c, void* d, const void* h, uint64_t bytes) {
    if (!c) return NRG_E_INVAL;
    int r = use_device(c);
    if (r) return r;
    HIPCHK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(sync_all(c));
    return NRG_OK;
}
int nrg_memcpy_d2h(nrg_ctx* c, void* h, const void* d, uint64_t bytes) {
    if (!c) return NRG_E_INVAL;
    int r = use_device(c);
    if (r) return r;
    HIPCHK(flush_deferred(c));
    HIPCHK(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_all(c));
    return NRG_OK;
}

// ---- kernel timing -------------------------------------------------------------------------------
int nrg_kernel_timing(nrg_ctx* c, int enable) {
    if (!c || enable < 0) return NRG_E_INVAL;
    c->timing = enable != 0;
    c->timing_every = enable > 1 ? (uint32_t)enable : 1;
    for (auto& kv : c->timers) kv.second.seen = 0;
    return NRG_OK;
}

int nrg_kernel_timing_only(nrg_ctx* c, const char* which) {
    if (!c) return NRG_E_INVAL;
    c->timing_only = which ? which : "";
    return NRG_OK;
}

int nrg_kernel_time(nrg_ctx* c, const char* which, uint64_t* launches, double* total_ms) {
    if (!c || !which) return NRG_E_INVAL;
    int r = use_device(c);
    if (r) return r;
    HIPCHK(sync_all(c));
    auto it = c->timers.find(which);
    if (it == c->timers.end()) {
        *launches = 0;
        *total_ms = 0;
        return NRG_OK;
    }
    KTimer& t = it->second;
    for (uint64_t p = 0; p < t.pending; p++) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, t.ev[2 * p], t.ev[2 * p + 1]));
        t.total_ms += ms;
    }
    t.launches += t.pending;
    t.pending = 0;
    *launches = t.launches;
    *total_ms = t.total_ms;
    return NRG_OK;
}

}  // extern "C"

// ---- test hooks (include/nrgpu_testing.h) -----------------------------------------------------
extern "C" int nrg_test_ring_read(nrg_ctx* c, uint64_t phys, void* out) {
    if (!c || !out || phys >= c->log_size) return NRG_E_INVAL;
    int r = use_device(c);
    if (r) return r;
    HIPCHK(sync_all(c));
    HIPCHK(hipMemcpy(out, (const char*)c->d_ring + phys * c->rec_bytes, c->rec_bytes, hipMemcpyDeviceToHost));
    return NRG_OK;
}

extern "C" int nrg_test_debug_read(nrg_ctx* c, uint64_t* out, uint64_t words) {
    if (!c || !out) return NRG_E_INVAL;
    if (!c->d_dbg || words > c->dbg_words) return NRG_E_INVAL;
    int r = use_device(c);
    if (r) return r;
    // diagnostic timestamps of the launches so far: no flush of deferred work (it would stamp over them)
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out, c->d_dbg, words * 8, hipMemcpyDeviceToHost));
    return NRG_OK;
}

// Tuning and diagnostic knobs (include/nrgpu_testing.h): the only way to change them.
extern "C" int nrg_test_set_knob(nrg_ctx* c, int knob, uint64_t v) {
    if (!c) return NRG_E_INVAL;
    int r = use_device(c);
    if (r) return r;
    HIPCHK(sync_all(c));  // deferred work of the old setting completes first
    switch (knob) {
        case NRG_KNOB_EXP: {
            if (v & ~0x10002ull) return NRG_E_INVAL;  // 2: phase timestamps, 0x10000: group.hpp pt_ident
            c->exp = (uint32_t)v;
            // the kind's timestamp buffer
            const uint64_t words = (c->exp & 2) && c->ops->dbg_words ? c->ops->dbg_words(c) : 0;
            if (words > c->dbg_words) {
                if (c->d_dbg) HIPCHK(hipFree(c->d_dbg));
                c->d_dbg = nullptr;
                c->dbg_words = 0;
                HIPCHK(hipMalloc(&c->d_dbg, words * sizeof(uint64_t)));
                HIPCHK(hipMemsetAsync(c->d_dbg, 0, words * sizeof(uint64_t), c->stream));
                c->dbg_words = words;
            }
            return NRG_OK;
        }
        case NRG_KNOB_STALL:
            if (v > 3) return NRG_E_INVAL;
            c->stall = (uint32_t)v;
            return NRG_OK;
        case NRG_KNOB_PIPELINE:
            if (v > 1) return NRG_E_INVAL;
            c->pipeline = v != 0;
            return NRG_OK;
        case NRG_KNOB_COMB_SPIN:
            if (v > 4096) return NRG_E_INVAL;
            c->comb.spin = (int32_t)v;
            return NRG_OK;
        case NRG_KNOB_COMB_GATHER:
            if (v > 1000) return NRG_E_INVAL;
            c->comb.gather = (int32_t)v;
            return NRG_OK;
        case NRG_KNOB_COMB_SERVE:
            if (v > (1u << 20)) return NRG_E_INVAL;
            c->comb.serve = (int32_t)v;
            return NRG_OK;
        case NRG_KNOB_COMB_DEPTH:
            if (v < 1 || v > 4) return NRG_E_INVAL;
            c->comb.depth = (uint32_t)v;
            return NRG_OK;
        default:  // the kind's own knobs
            return c->ops->set_knob ? c->ops->set_knob(c, knob, v) : NRG_E_INVAL;
    }
}
