// snapshot.cpp — replica snapshot and restore, the same for every kind (include/nrgpu.h,
// nrg_snapshot_* / nrg_restore): the image's header, its validation, and the order of a restore's
// steps. What a kind's items are, how its payload is written and how its bookkeeping is rebuilt
// from one is in the kind's file, behind DsOps::items / snapshot / restore.
//
// Reference: Replica::new (nr/src/replica.rs:184-232) builds a replica that replays the log from
// index 0, and Replica::verify (:443-467) is the only view of a replica's state. Here a replica is
// also built from another replica's state at log index log_idx, and goes on from there.
#include <hip/hip_runtime.h>

#include <cstring>

#include "internal.hpp"

using namespace nrg;

namespace {

// bytes of one payload item of a kind (0: not a kind)
uint64_t item_bytes(uint32_t kind) {
    switch (kind) {
        case NRG_DS_HASHMAP: return sizeof(nrg_put);
        case NRG_DS_STACK: return sizeof(uint32_t);
        case NRG_DS_SYNTHETIC: return sizeof(uint64_t);
        case NRG_DS_QUEUE: return sizeof(uint64_t);
        case NRG_DS_VSPACE: return 4096;
        case NRG_DS_SKIPLIST: return sizeof(nrg_put);
        case NRG_DS_MEMFS: return sizeof(uint64_t);  // an aligned 8-byte word of a file
        default: return 0;
    }
}

// the header's eight words against the format and the bytes the caller holds
int parse_header(const uint64_t h[8], uint64_t bytes, nrg_snapshot_info* out) {
    if (h[0] != SNAP_MAGIC) return NRG_E_INVAL;
    const uint32_t kind = (uint32_t)h[1], version = (uint32_t)(h[1] >> 32);
    const uint64_t ib = item_bytes(kind);
    if (version != SNAP_VERSION || !ib) return NRG_E_INVAL;
    const uint64_t items = h[2];
    if (items > (1ull << 40)) return NRG_E_INVAL;  // (more than any structure holds; keeps items * ib from wrapping)
    if (h[3] != snap_bytes(items * ib) || h[3] > bytes) return NRG_E_INVAL;
    out->ds_kind = kind;
    out->version = version;
    out->items = items;
    out->bytes = h[3];
    out->log_idx = h[4];
    std::memcpy(out->digest, h + 5, sizeof out->digest);
    return NRG_OK;
}

int read_header(nrg_ctx* c, const void* d_buf, uint64_t bytes, nrg_snapshot_info* out) {
    if (bytes < SNAP_HDR) return NRG_E_INVAL;
    uint64_t h[8];
    HIPCHK(hipMemcpyAsync(h, d_buf, SNAP_HDR, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return parse_header(h, bytes, out);
}

}  // namespace

extern "C" {

int nrg_snapshot_size(nrg_ctx* c, nrg_snapshot_info* out) {
    if (!c || !out) return NRG_E_INVAL;
    int r = ctx_use_device(c);
    if (r) return r;
    HIPCHK(sync_all(c));
    uint64_t items = 0;
    if ((r = c->ops->items(c, &items))) return r;
    std::memset(out, 0, sizeof *out);
    out->ds_kind = c->cfg.ds_kind;
    out->version = SNAP_VERSION;
    out->items = items;
    out->bytes = snap_bytes(items * item_bytes(c->cfg.ds_kind));
    out->log_idx = c->ltail;
    return NRG_OK;
}

int nrg_snapshot_async(nrg_ctx* c, void* d_buf, uint64_t cap) {
    if (!c || !d_buf || ((uintptr_t)d_buf & 15)) return NRG_E_INVAL;  // (the payload is stored 16 B at a time)
    int r = ctx_use_device(c);
    if (r) return r;
    HIPCHK(flush_deferred(c));
    HIPCHK(c->ops->snapshot(c, d_buf, cap, c->ltail));
    // the triple straight into header words 5..7 (inside cap whenever the header is)
    if (cap >= SNAP_HDR) HIPCHK(c->ops->digest(c, (uint64_t*)d_buf + 5));
    return NRG_OK;
}

int nrg_snapshot_info_read(nrg_ctx* c, const void* d_buf, uint64_t bytes, nrg_snapshot_info* out) {
    if (!c || !d_buf || !out) return NRG_E_INVAL;
    int r = ctx_use_device(c);
    if (r) return r;
    return read_header(c, d_buf, bytes, out);
}

int nrg_restore(nrg_ctx* c, const void* d_buf, uint64_t bytes) {
    if (!c || !d_buf || ((uintptr_t)d_buf & 15)) return NRG_E_INVAL;
    int r = ctx_use_device(c);
    if (r) return r;
    // 1, 2: the header against the format, then against this context; nothing of the replica's state is
    // touched yet (a hashmap with removal enabled scans the payload for its tombstone here: one launch,
    // a stream synchronise, and DevCtl::counter, which is scratch of the dump and the snapshot)
    nrg_snapshot_info info;
    if ((r = read_header(c, d_buf, bytes, &info))) return r;
    if (info.ds_kind != c->cfg.ds_kind) return NRG_E_INVAL;
    const void* payload = (const char*)d_buf + SNAP_HDR;
    if ((r = c->ops->restore(c, payload, info.items, true))) return r;
    // 3: queued and deferred work completes against the old contents; the error latch starts clear
    HIPCHK(sync_all(c));
    (void)check_err(c);
    // 4, 5: the contents, then the log: the replica has replayed [0, log_idx) and holds no entry
    if ((r = c->ops->restore(c, payload, info.items, false))) return r;
    c->head = c->tail = c->ctail = c->ltail = info.log_idx;
    c->origins.clear();
    // 6: the rebuilt state's digest against the header's
    uint64_t got[3] = {0, 0, 0};
    if ((r = staging(c->stg[3], 64))) return r;
    HIPCHK(c->ops->digest(c, (uint64_t*)c->stg[3].p));
    HIPCHK(hipMemcpyAsync(got, c->stg[3].p, sizeof got, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_all(c));
    r = check_err(c);  // (a probe that overran the table: ERR_TABLE_FULL)
    if (r == NRG_OK && std::memcmp(got, info.digest, sizeof got) == 0) return NRG_OK;
    if (r != NRG_OK && r != NRG_E_TABLE_FULL && r != NRG_E_CAPACITY && r != NRG_E_INVAL) return r;
    // The payload is not the state its header describes. What it put into the structure may not be
    // a valid state (a page table whose inner entries point past the pool): leave the empty one.
    if (c->ops->restore(c, nullptr, 0, false) == NRG_OK) (void)sync_all(c);
    (void)check_err(c);
    return NRG_E_INVAL;
}

}  // extern "C"
