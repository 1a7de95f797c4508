// group.cpp — multi-GPU replica groups: the write segments of a round are all-gathered with RCCL
// over xGMI and every replica replays the identical global log (include/nrgpu.h, nrg_group_*).
// Here: the backend, join / open / close, the replicated round, sync, verify and resync; the
// key-partitioned rounds are group_partitioned.cpp's, the group-wide reads group_reads.cpp's
// (group.hpp: what the three share).
//
// Reference: the shared Log of nr/src/log.rs, read by every replica's exec loop
// (nr/src/log.rs:494-511, :473-524) through cache-coherent memory. Here each GPU keeps its own
// copy of the log; one ncclAllGather per round moves the new entries to every copy, in rank
// order, which is the round's deterministic global log order.
//
// Per member and round e (b = e % NBUF):
//   comm stream : wait(input ready) -> wait(freed[b]) -> [pad copy] -> ncclAllGather -> gathered[b]
//   replica     : wait(gathered[b]) -> Log::append + Log::exec + reads (replay kernels) -> freed[b]
// The comm stream never waits for a replay except through freed[b] (NBUF rounds back), so the
// all-gather of round e+1 runs while round e replays.
//
// RCCL is resolved with dlopen at the first group call: the process's own librccl.so.1 when one
// is already loaded (torch ships one), else the system's. libnrgpu.so itself does not link it.
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <mutex>
#include <new>
#include <thread>

#include "group.hpp"
#include "../../include/nrgpu_testing.h"

using namespace nrg::grp;

namespace {

std::mutex g_rccl_mu;
bool g_rccl_tried = false;
Rccl g_rccl;
bool g_rccl_ok = false;

const Rccl* rccl() {
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    if (!g_rccl_tried) {
        g_rccl_tried = true;
        void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (h) {
            Rccl r;
            r.get_unique_id = (decltype(r.get_unique_id))dlsym(h, "ncclGetUniqueId");
            r.init_rank = (decltype(r.init_rank))dlsym(h, "ncclCommInitRank");
            r.init_all = (decltype(r.init_all))dlsym(h, "ncclCommInitAll");
            r.all_gather = (decltype(r.all_gather))dlsym(h, "ncclAllGather");
            r.group_start = (decltype(r.group_start))dlsym(h, "ncclGroupStart");
            r.group_end = (decltype(r.group_end))dlsym(h, "ncclGroupEnd");
            r.destroy = (decltype(r.destroy))dlsym(h, "ncclCommDestroy");
            r.send = (decltype(r.send))dlsym(h, "ncclSend");
            r.recv = (decltype(r.recv))dlsym(h, "ncclRecv");
            r.abort = (decltype(r.abort))dlsym(h, "ncclCommAbort");
            g_rccl_ok = r.get_unique_id && r.init_rank && r.init_all && r.all_gather && r.group_start &&
                        r.group_end && r.destroy;
            if (g_rccl_ok) g_rccl = r;
        }
    }
    return g_rccl_ok ? &g_rccl : nullptr;
}

// nrg_test_loopback_collectives: groups created from now on use loopback.cpp instead of RCCL
std::atomic<int> g_loopback{0};

// the collectives a new group binds to (kept by the group for its lifetime)
const Rccl* backend() { return g_loopback.load() ? nrg::loopback_collectives() : rccl(); }

constexpr uint64_t WX_MAX = 3;  // words per rank of a words exchange (gather_words); wx takes 4, so that gwx
                                // is 16-byte aligned as the two-word exchanges always had it

int member_init(Member& m, int nranks) {
    int r = nrg::ctx_use_device(m.ctx);
    if (r) return r;
    GCHK(hipStreamCreateWithFlags(&m.cstream, hipStreamNonBlocking));
    GCHK(hipStreamCreateWithFlags(&m.pstream, hipStreamNonBlocking));
    GCHK(hipEventCreateWithFlags(&m.in_ev, hipEventDisableTiming));
    GCHK(hipEventCreateWithFlags(&m.ord_ev, hipEventDisableTiming));
    for (int b = 0; b < NBUF; b++) {
        GCHK(hipEventCreateWithFlags(&m.gathered[b], hipEventDisableTiming));
        GCHK(hipEventCreateWithFlags(&m.freed[b], hipEventDisableTiming));
    }
    const uint64_t G = (uint64_t)nranks;
    GCHK(hipMalloc(&m.xmem, (NBUF * (2 + 2 * G) + 4 + WX_MAX * G) * 8));
    uint64_t* x = (uint64_t*)m.xmem;
    for (int b = 0; b < NBUF; b++, x += 2 + 2 * G) {
        m.hdr[b] = x;
        m.ghdr[b] = x + 2;
    }
    m.wx = x;
    m.gwx = x + 4;
    GCHK(hipHostMalloc(&m.h_gwx, WX_MAX * G * 8, hipHostMallocDefault));
    RCHK(m.pt.init(m, nranks));
    RCHK(m.fp.init(m, nranks));
    return m.pr.init(m, nranks);
}

void member_free(Member& m, const Rccl* R) {
    if (!m.ctx) return;
    (void)nrg::ctx_use_device(m.ctx);
    if (m.cstream) (void)hipStreamSynchronize(m.cstream);
    if (m.comm && R) R->destroy(m.comm);
    for (int b = 0; b < NBUF; b++) {
        free_buf(m.gbuf[b]);
        if (m.gathered[b]) (void)hipEventDestroy(m.gathered[b]);
        if (m.freed[b]) (void)hipEventDestroy(m.freed[b]);
    }
    free_buf(m.sbuf);
    free_buf(m.snap);
    if (m.xmem) (void)hipFree(m.xmem);
    if (m.h_gwx) (void)hipHostFree(m.h_gwx);
    m.pt.free();
    m.sk.free();
    m.fp.free();
    m.pr.free();
    m.po.free();
    if (m.ord_ev) (void)hipEventDestroy(m.ord_ev);
    if (m.pstream) (void)hipStreamSynchronize(m.pstream);
    if (m.pstream) (void)hipStreamDestroy(m.pstream);
    if (m.in_ev) (void)hipEventDestroy(m.in_ev);
    if (m.cstream) (void)hipStreamDestroy(m.cstream);
    m = Member{};
}

// Round header check (on the comm stream, after the all-gather): every rank's {n, fingerprint}
// must match this rank's view of the round. A mismatch latches ERR_GROUP in the replica, which
// nrg_sync / nrg_group_sync report as NRG_E_INVAL.
struct LensArg {
    uint64_t v[64];
};
__global__ void grp_check_kernel(const uint64_t* ghdr, uint32_t G, LensArg lens, uint64_t fp, uint32_t* err) {
    const uint32_t r = threadIdx.x;
    if (r < G && (ghdr[2 * r] != lens.v[r] || ghdr[2 * r + 1] != fp)) atomicOr(err, nrg::ERR_GROUP);
}

// dst[0] = a, dst[1] = b in stream order (kernel arguments are captured at launch)
__global__ void grp_put2_kernel(uint64_t* dst, uint64_t a, uint64_t b) {
    if (threadIdx.x < 2) dst[threadIdx.x] = threadIdx.x ? b : a;
}

// Wait until `query` succeeds, at most the group's deadline from now. A stream that does not drain
// is one whose collective a peer never joined (or a hung device): the group fails with NRG_E_TIMEOUT.
template <typename Q>
int wait_until(nrg_group* g, Q query, const char* phase) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    const auto dl = t0 + std::chrono::milliseconds(g->timeout_ms);
    for (uint32_t naps = 0;;) {
        const hipError_t e = query();
        if (e == hipSuccess) return NRG_OK;
        if (e != hipErrorNotReady) return hip_rc(e);
        const auto now = clk::now();
        if (now >= dl) {
            char what[192];
            std::snprintf(what, sizeof what, "%s did not complete within %u ms (a peer rank never joined the collective?)",
                          phase, g->timeout_ms);
            return group_fail(g, NRG_E_TIMEOUT, what);
        }
        // a host round trip is short: spin for the first 200 us, then back off: 2000 naps of 20 us,
        // then of 500 us. The naps are counted, not the queries: 200 us of polling is far more than
        // 2000 queries, and a round's counts that sit behind a replay of a few hundred us (a
        // file-partitioned round) must not cost a 500 us nap.
        if (now - t0 > std::chrono::microseconds(200))
            std::this_thread::sleep_for(std::chrono::microseconds(naps++ < 2000 ? 20 : 500));
    }
}

// The gathered and the send buffers grow by a rule of their own, not grow_buf's: the exact size, and
// a wait for the comm stream alone, under the deadline (it may hold a collective a peer never
// joined, and that wait must be able to time out).
int grow_exact(nrg_group* g, Member& m, DBuf& d, uint64_t bytes, const char* phase) {
    if (d.bytes >= bytes) return NRG_OK;
    RCHK(wait_stream(g, m.cstream, phase));
    if (d.p) GCHK(hipFree(d.p));
    d.p = nullptr;
    d.bytes = 0;
    GCHK(hipMalloc(&d.p, bytes));
    d.bytes = bytes;
    return NRG_OK;
}

}  // namespace

// (RCCL's abort ends a collective a peer never posted, so the streams drain and close() cannot hang)
int nrg::grp::group_fail(nrg_group* g, int code, const char* what) {
    if (g->broken == NRG_OK) {
        g->broken = code;
        std::snprintf(g->diag, sizeof g->diag, "nrg_group rank %d of %d, round %llu: %s", g->rank0, g->nranks,
                      (unsigned long long)g->round, what);
        std::fprintf(stderr, "%s\n", g->diag);
        if (code == NRG_E_TIMEOUT && g->R && g->R->abort)
            for (Member& m : g->m)
                if (m.comm) {
                    (void)g->R->abort(m.comm);
                    m.comm = nullptr;
                }
    }
    return g->broken;
}

// (the loopback blocks there until its peers post; RCCL enqueues and returns, and a missing peer
// shows up in the stream waits)
int nrg::grp::group_end(nrg_group* g, const char* phase) {
    if (g->R->set_timeout_ms) g->R->set_timeout_ms(g->timeout_ms);
    const ncclResult_t r = g->R->group_end();
    if (r == ncclSuccess) return NRG_OK;
    char what[192];
    if (r == ncclSystemError && g->R->set_timeout_ms) {
        std::snprintf(what, sizeof what, "%s: a peer rank did not post its part within %u ms", phase, g->timeout_ms);
        return group_fail(g, NRG_E_TIMEOUT, what);
    }
    std::snprintf(what, sizeof what, "%s: collective failed (ncclResult %d)", phase, (int)r);
    return group_fail(g, NRG_E_COMM, what);
}

int nrg::grp::wait_stream(nrg_group* g, hipStream_t s, const char* phase) {
    return wait_until(g, [s] { return hipStreamQuery(s); }, phase);
}
int nrg::grp::wait_event(nrg_group* g, hipEvent_t ev, const char* phase) {
    return wait_until(g, [ev] { return hipEventQuery(ev); }, phase);
}

int nrg::grp::gather_words(nrg_group* g, int w, const char* phase) {
    RCHK(collective(g, phase, [&](Member& m, int) {
        return g->R->all_gather(m.wx, m.gwx, (size_t)w, ncclUint64, m.comm, m.cstream);
    }));
    for (Member& m : g->m) {
        RCHK(nrg::ctx_use_device(m.ctx));
        GCHK(hipMemcpyAsync(m.h_gwx, m.gwx, (uint64_t)w * g->nranks * 8, hipMemcpyDeviceToHost, m.cstream));
        RCHK(wait_stream(g, m.cstream, phase));
    }
    return NRG_OK;
}

int nrg::grp::exchange_pairs(nrg_group* g, const std::vector<uint64_t>& a, const std::vector<uint64_t>& b,
                             const char* phase) {
    const int nl = (int)g->m.size();
    for (int i = 0; i < nl; i++) {
        Member& m = g->m[i];
        RCHK(nrg::ctx_use_device(m.ctx));
        grp_put2_kernel<<<1, 64, 0, m.cstream>>>(m.wx, a[i], b[i]);
        GCHK(hipGetLastError());
    }
    return gather_words(g, 2, phase);
}

// (nrg_skiplist_get_async takes no more in one call; a skewed partitioned round can hand one owner
// G times a member's Gets)
int nrg::grp::sl_gets(nrg_ctx* c, const uint64_t* keys, uint64_t n, uint64_t* vals, uint8_t* found) {
    const uint64_t step = std::max<uint64_t>(1, c->cfg.max_reads);
    for (uint64_t at = 0; at < n; at += step)
        RCHK(nrg_skiplist_get_async(c, keys + at, std::min(step, n - at), vals + at, found + at));
    return NRG_OK;
}

// Every rank's segment length of a round whose caller gave none (seg_lens == NULL, one member per
// process): each rank all-gathers {n, local error} and the host reads them back (one host round
// trip). A rank whose own part is bad makes every rank return NRG_E_INVAL, so no rank is left
// inside a collective its peers never post.
static int exchange_lengths(nrg_group* g, const nrg_round* rounds, const std::vector<int>& bad,
                            std::vector<uint64_t>& lens) {
    const int nl = (int)g->m.size(), G = g->nranks;
    std::vector<uint64_t> a(nl), b(nl);
    for (int i = 0; i < nl; i++) a[i] = rounds[i].n, b[i] = bad[i] ? 1 : 0;
    RCHK(exchange_pairs(g, a, b, "length exchange"));
    const uint64_t* H = g->m[0].h_gwx;  // identical on every rank
    bool any_bad = false;
    for (int r = 0; r < G; r++) {
        lens[r] = H[2 * r];
        any_bad |= H[2 * r + 1] != 0;
    }
    return any_bad ? NRG_E_INVAL : NRG_OK;
}

// A round's gathered log, replayed by one member (on its replica's stream): the hashmap's round
// over the G segments (or its reads alone when no rank wrote), any other kind's append then exec;
// a skip list's reads (SkipListConcurrent::Get, benches/lockfree.rs:73-84) then run against the
// post-round state, as the hashmap's round answers its own.
static int replay_gathered(Member& m, const nrg_round& x, uint32_t kind, const void* gathered, uint32_t G, uint64_t stride,
                           const std::vector<uint64_t>& lens, const std::vector<uint32_t>& origins) {
    nrg_ctx* c = m.ctx;
    if (kind == NRG_DS_HASHMAP) {
        if (stride)
            return nrg_hashmap_round_segments_async(c, (const nrg_put*)gathered, G, stride, lens.data(), origins.data(),
                                                    (uint32_t)m.rank, x.get_keys, x.n_gets, x.get_vals, x.get_found,
                                                    (uint64_t*)x.resp, x.some);
        return nrg_hashmap_round_async(c, nullptr, 0, origins[m.rank], x.get_keys, x.n_gets, x.get_vals, x.get_found,
                                       nullptr, nullptr);
    }
    if (stride) {
        std::vector<uint64_t> firsts(G);
        RCHK(nrg_log_append_segments_async(c, gathered, G, stride, lens.data(), origins.data(), firsts.data()));
        RCHK(nrg_log_exec_async(c, firsts[m.rank], firsts[m.rank] + lens[m.rank], x.resp, x.some));
    }
    return kind == NRG_DS_SKIPLIST ? sl_gets(c, x.get_keys, x.n_gets, x.get_vals, x.get_found) : NRG_OK;
}

extern "C" {

int nrg_test_loopback_collectives(int on) {
    g_loopback.store(on ? 1 : 0);
    return NRG_OK;
}

int nrg_group_unique_id(uint8_t id[NRG_GROUP_ID_BYTES]) {
    if (!id) return NRG_E_INVAL;
    const Rccl* R = backend();
    if (!R) return NRG_E_COMM;
    ncclUniqueId u;
    if (R->get_unique_id(&u) != ncclSuccess) return NRG_E_COMM;
    static_assert(sizeof(u) == NRG_GROUP_ID_BYTES, "ncclUniqueId size");
    std::memcpy(id, &u, NRG_GROUP_ID_BYTES);
    return NRG_OK;
}

int nrg_group_join(nrg_ctx* replica, const uint8_t id[NRG_GROUP_ID_BYTES], int nranks, int rank, nrg_group** out) {
    if (!replica || !id || !out || nranks < 1 || rank < 0 || rank >= nranks || nranks > 64) return NRG_E_INVAL;
    *out = nullptr;
    const Rccl* R = backend();
    if (!R) return NRG_E_COMM;
    nrg_group* g = new (std::nothrow) nrg_group();
    if (!g) return NRG_E_NOMEM;
    g->R = R;
    g->nranks = nranks;
    g->rank0 = rank;
    g->m.resize(1);
    Member& m = g->m[0];
    m.ctx = replica;
    m.rank = rank;
    int r = member_init(m, nranks);
    ncclUniqueId u;
    std::memcpy(&u, id, NRG_GROUP_ID_BYTES);
    if (r == NRG_OK && R->init_rank(&m.comm, nranks, u, rank) != ncclSuccess) r = NRG_E_COMM;
    if (r != NRG_OK) {
        member_free(m, R);
        delete g;
        return r;
    }
    *out = g;
    return NRG_OK;
}

int nrg_group_open(const int* devices, int n, const nrg_config* cfg, nrg_group** out) {
    if (!devices || n < 1 || n > 64 || !cfg || !out) return NRG_E_INVAL;
    *out = nullptr;
    const Rccl* R = backend();
    if (!R) return NRG_E_COMM;
    nrg_group* g = new (std::nothrow) nrg_group();
    if (!g) return NRG_E_NOMEM;
    g->R = R;
    g->nranks = n;
    g->rank0 = 0;
    g->owns = true;
    g->m.resize(n);
    int r = NRG_OK;
    for (int i = 0; i < n && r == NRG_OK; i++) {
        nrg_config c = *cfg;
        c.replica_id = (uint32_t)i + 1;  // Log::register hands out ids from 1 (nr/src/log.rs:272-292)
        r = nrg_open(devices[i], &c, &g->m[i].ctx);
        g->m[i].rank = i;
        if (r == NRG_OK) r = member_init(g->m[i], n);
    }
    if (r == NRG_OK) {
        std::vector<ncclComm_t> comms(n);
        if (R->init_all(comms.data(), n, devices) != ncclSuccess) r = NRG_E_COMM;
        else
            for (int i = 0; i < n; i++) g->m[i].comm = comms[i];
    }
    if (r != NRG_OK) {
        nrg_group_close(g);
        return r;
    }
    *out = g;
    return NRG_OK;
}

int nrg_group_close(nrg_group* g) {
    if (!g) return NRG_E_INVAL;
    const Rccl* R = g->R;
    for (Member& m : g->m) {
        nrg_ctx* c = m.ctx;
        member_free(m, R);
        if (g->owns && c) nrg_close(c);
    }
    delete g;
    return NRG_OK;
}

int nrg_group_info(const nrg_group* g, int* nranks, int* nlocal, int* rank0) {
    if (!g) return NRG_E_INVAL;
    if (nranks) *nranks = g->nranks;
    if (nlocal) *nlocal = (int)g->m.size();
    if (rank0) *rank0 = g->rank0;
    return NRG_OK;
}

nrg_ctx* nrg_group_replica(nrg_group* g, int member) {
    if (!g || member < 0 || member >= (int)g->m.size()) return nullptr;
    return g->m[member].ctx;
}

int nrg_group_set_input_stream(nrg_group* g, int member, void* s) {
    if (!g || member < 0 || member >= (int)g->m.size()) return NRG_E_INVAL;
    g->m[member].in_stream = (hipStream_t)s;
    g->m[member].in_set = true;
    return NRG_OK;
}

int nrg_group_round_async(nrg_group* g, const nrg_round* rounds, const uint64_t* seg_lens) {
    if (!g || !rounds) return NRG_E_INVAL;
    if (g->broken) return g->broken;
    const Rccl* R = g->R;
    if (!R) return NRG_E_COMM;
    const int nl = (int)g->m.size(), G = g->nranks;
    const uint32_t kind = g->m[0].ctx->cfg.ds_kind;
    const uint64_t rb = g->m[0].ctx->rec_bytes;
    // every rank's segment length, in rank order
    std::vector<uint64_t> lens(G);
    std::vector<int> bad(nl, 0);
    for (int i = 0; i < nl; i++)
        bad[i] = g->m[i].ctx->cfg.ds_kind != kind || (rounds[i].n && !rounds[i].recs) ||
                 (kind == NRG_DS_SKIPLIST && rounds[i].n_gets &&
                  (!rounds[i].get_keys || !rounds[i].get_vals || !rounds[i].get_found));
    // Three ways to know them:
    //   whole   this process drives every rank: the members' n (or seg_lens, checked against them)
    //   given   seg_lens from the caller, who promises every rank passes the same array: a header
    //           {n, fingerprint of seg_lens} travels with each segment and a kernel on the comm
    //           stream compares it with this rank's view (mismatch -> NRG_E_INVAL at the next sync)
    //   exchanged  seg_lens == NULL: exchange_lengths (one host round trip)
    const bool whole = nl == G;
    const bool given = !whole && seg_lens;
    if (whole) {
        for (int i = 0; i < nl; i++) {
            const uint64_t n = rounds[i].n;
            if (bad[i] || (seg_lens && seg_lens[g->m[i].rank] != n)) return NRG_E_INVAL;
            lens[g->m[i].rank] = n;
        }
    } else if (given) {
        for (int r = 0; r < G; r++) lens[r] = seg_lens[r];
        for (int i = 0; i < nl; i++) bad[i] |= rounds[i].n != lens[g->m[i].rank];
    } else {
        RCHK(exchange_lengths(g, rounds, bad, lens));
    }
    const uint64_t stride = lens_stride(lens);
    const uint64_t fp = lens_fp(lens);
    LensArg la{};
    for (int r = 0; r < G; r++) la.v[r] = lens[r];
    std::vector<uint32_t> origins(G);
    for (int r = 0; r < G; r++) origins[r] = (uint32_t)r + 1;
    const int b = (int)(g->round % NBUF);
    const uint64_t seg_bytes = stride * rb;
    std::vector<const void*> send(nl);
    if (stride || given) {
        for (int i = 0; i < nl; i++) {
            Member& m = g->m[i];
            const nrg_round& x = rounds[i];
            RCHK(nrg::ctx_use_device(m.ctx));
            // the all-gather reads the caller's segment: ordered after its producer
            GCHK(hipEventRecord(m.in_ev, m.in_set ? m.in_stream : m.ctx->stream));
            GCHK(hipStreamWaitEvent(m.cstream, m.in_ev, 0));
            // and it overwrites gathered buffer b: ordered after the replay that read it
            if (m.used[b]) GCHK(hipStreamWaitEvent(m.cstream, m.freed[b], 0));
            if (given) grp_put2_kernel<<<1, 64, 0, m.cstream>>>(m.hdr[b], bad[i] ? ~0ull : x.n, fp);
            GCHK(hipGetLastError());
            if (!stride) continue;
            RCHK(grow_exact(g, m, m.gbuf[b], (uint64_t)G * seg_bytes, "gathered-buffer growth"));
            if (x.n == stride && !bad[i]) {
                send[i] = x.recs;
            } else {  // pad a short segment to the common stride (a bad one sends zeros)
                RCHK(grow_exact(g, m, m.sbuf, seg_bytes, "send-buffer growth"));
                const uint64_t keep = bad[i] ? 0 : x.n;
                if (keep) GCHK(hipMemcpyAsync(m.sbuf.p, x.recs, keep * rb, hipMemcpyDeviceToDevice, m.cstream));
                GCHK(hipMemsetAsync((char*)m.sbuf.p + keep * rb, 0, seg_bytes - keep * rb, m.cstream));
                send[i] = m.sbuf.p;
            }
        }
        RCHK(collective(g, "segment all-gather", [&](Member& m, int i) {
            ncclResult_t res = ncclSuccess;
            if (given) res = R->all_gather(m.hdr[b], m.ghdr[b], 2, ncclUint64, m.comm, m.cstream);
            if (stride && res == ncclSuccess)
                res = R->all_gather(send[i], m.gbuf[b].p, seg_bytes / 8, ncclUint64, m.comm, m.cstream);
            return res;
        }));
        if (given)
            for (int i = 0; i < nl; i++) {
                Member& m = g->m[i];
                RCHK(nrg::ctx_use_device(m.ctx));
                grp_check_kernel<<<1, 64, 0, m.cstream>>>(m.ghdr[b], (uint32_t)G, la, fp, &m.ctx->d_ctl->err);
                GCHK(hipGetLastError());
            }
    }
    int rc = NRG_OK;
    for (int i = 0; i < nl; i++) {
        Member& m = g->m[i];
        nrg_ctx* c = m.ctx;
        RCHK(nrg::ctx_use_device(c));
        if (bad[i]) {  // took part in the collectives, replays nothing
            // Its peers replay the round (with this rank's segment as zeros) and latch ERR_GROUP;
            // the replicas now differ, so the group is over for every rank (sticky error).
            rc = group_fail(g, NRG_E_INVAL, "this rank's segment disagreed with seg_lens (or its buffers were missing): replicas diverged");
            continue;
        }
        if (stride) {
            GCHK(hipEventRecord(m.gathered[b], m.cstream));
            GCHK(hipStreamWaitEvent(c->stream, m.gathered[b], 0));
        }
        RCHK(replay_gathered(m, rounds[i], kind, m.gbuf[b].p, (uint32_t)G, stride, lens, origins));
        if (stride) {
            GCHK(hipEventRecord(m.freed[b], c->stream));
            m.used[b] = true;
        }
    }
    g->round++;
    return rc;
}

int nrg_group_sync(nrg_group* g) {
    if (!g) return NRG_E_INVAL;
    if (g->broken) return g->broken;
    int rc = pt_flush_posted(g);  // posted partitioned rounds complete first
    if (g->broken) return g->broken;
    for (Member& m : g->m) {
        int r = nrg::ctx_use_device(m.ctx);
        if (r) return r;
        RCHK(wait_stream(g, m.cstream, "group sync (collectives)"));
        RCHK(wait_stream(g, m.pstream, "group sync (partitions)"));
        RCHK(wait_stream(g, m.ctx->stream, "group sync (replay)"));
        // disagreeing round headers (ERR_GROUP, latched by grp_check_kernel) end the group: the
        // ranks have replayed different logs, so every later call reports it too
        uint32_t err = 0;
        GCHK(hipMemcpyAsync(&err, &m.ctx->d_ctl->err, sizeof err, hipMemcpyDeviceToHost, m.ctx->stream));
        GCHK(hipStreamSynchronize(m.ctx->stream));  // drained above: returns at once
        r = nrg_sync(m.ctx);
        if (err & nrg::ERR_GROUP)
            r = group_fail(g, NRG_E_INVAL, "ranks disagreed on a round's segment lengths: replicas diverged");
        if (r && rc == NRG_OK) rc = r;
    }
    return rc;
}

// Replica::verify (nr/src/replica.rs:443-467) across the group: every rank's digest triple, all-
// gathered. Members of a partitioned group hold one partition each, so their triples differ by
// design (*identical = 0): such callers add them (count and sum add, xor xors).
int nrg_group_verify(nrg_group* g, uint64_t* digests, int* identical) {
    if (!g || !identical) return NRG_E_INVAL;
    if (g->broken) return g->broken;
    if (!g->R) return NRG_E_COMM;
    const int G = g->nranks;
    // queued group work first; a latched device error of this rank (not sticky) is reported at the
    // end: the rank still posts its part, so that its peers are not left inside the collective
    const int rc = nrg_group_sync(g);
    if (g->broken) return g->broken;
    for (Member& m : g->m) {  // the words are the digest triple, already on the device
        RCHK(nrg::ctx_use_device(m.ctx));
        RCHK(nrg_digest_async(m.ctx, m.wx));
        RCHK(order(m, m.ctx->stream, m.cstream));
    }
    RCHK(gather_words(g, 3, "verify"));
    const uint64_t* H = g->m[0].h_gwx;  // identical on every rank
    int same = 1;
    for (int r = 1; r < G; r++)
        if (std::memcmp(H, H + 3 * r, 24) != 0) same = 0;
    if (digests) std::memcpy(digests, H, 3 * (uint64_t)G * 8);
    *identical = same;
    return rc;
}

// Replica::new from the root's state (include/nrgpu.h): the root's snapshot to every other rank,
// which restores from it. After the sync below no round is in flight.
int nrg_group_resync(nrg_group* g, int root) {
    if (!g || root < 0 || root >= g->nranks) return NRG_E_INVAL;
    if (g->broken) return g->broken;
    const Rccl* R = g->R;
    if (!R || !R->send || !R->recv) return NRG_E_COMM;
    const int nl = (int)g->m.size(), G = g->nranks;
    // queued group work first; a replica's latched device error is cleared by this (nrg_sync
    // reports it once): the contents it speaks of are about to be replaced
    (void)nrg_group_sync(g);
    if (g->broken) return g->broken;
    // the root's image size to every rank
    std::vector<uint64_t> size(nl, 0), zero(nl, 0);
    for (int i = 0; i < nl; i++) {
        Member& m = g->m[i];
        if (m.rank != root) continue;
        RCHK(nrg::ctx_use_device(m.ctx));
        nrg_snapshot_info info{};
        RCHK(nrg_snapshot_size(m.ctx, &info));
        size[i] = info.bytes;
    }
    RCHK(exchange_pairs(g, size, zero, "resync size exchange"));
    const uint64_t bytes = g->m[0].h_gwx[2 * root];  // identical on every rank
    if (bytes < 64 || (bytes & 63)) return group_fail(g, NRG_E_COMM, "resync: the root sent no snapshot size");
    for (Member& m : g->m) {
        RCHK(nrg::ctx_use_device(m.ctx));
        RCHK(grow_buf(m, m.snap, bytes));
        if (m.rank != root) continue;
        RCHK(nrg_snapshot_async(m.ctx, m.snap.p, bytes));
        RCHK(order(m, m.ctx->stream, m.cstream));
    }
    if (G > 1)
        RCHK(collective(g, "resync send/recv", [&](Member& m, int) {
            if (m.rank != root) return R->recv(m.snap.p, bytes / 8, ncclUint64, root, m.comm, m.cstream);
            ncclResult_t res = ncclSuccess;
            for (int o = 0; o < G && res == ncclSuccess; o++)
                if (o != root) res = R->send(m.snap.p, bytes / 8, ncclUint64, o, m.comm, m.cstream);
            return res;
        }));
    int rc = NRG_OK;
    for (Member& m : g->m) {
        RCHK(nrg::ctx_use_device(m.ctx));
        RCHK(wait_stream(g, m.cstream, "resync send/recv"));
        if (m.rank == root) continue;
        const int r = nrg_restore(m.ctx, m.snap.p, bytes);
        if (r && rc == NRG_OK) rc = r;
    }
    return rc;
}

int nrg_group_set_timeout(nrg_group* g, uint32_t ms) {
    if (!g || ms == 0) return NRG_E_INVAL;
    g->timeout_ms = ms;
    return NRG_OK;
}

const char* nrg_group_last_error(const nrg_group* g) { return g ? g->diag : ""; }

}  // extern "C"
