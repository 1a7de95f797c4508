// group_file_reads.cpp — the group-wide pread of a file-partitioned group of file-store replicas
// (include/nrgpu.h, nrg_group_memfs_pread; DESIGN.md §7 "Group-wide pread").
//
// benches/nrfs.rs reads with exec_ro(OpRd::FileRead(fd)) (:88-101, :146-152) on a cnr replica with one
// log per file (LogMapper::hash() = fd - 1, :25-39): the read goes to the replica state of its file's
// log (cnr/src/replica.rs:430-445). Here the log of partition p lives on rank p, and after a
// file-partitioned round (group_files.cpp) the only correct copy of a file is its owner's, so a read
// travels to the owner and its bytes travel back. One call, everything on the replica's stream:
//   1  the partition of the member's requests by owner (partition.hip rd_partition), whose counts are
//      the first G of the member's exchange words; the RW_* words follow them; the all-gather of every
//      rank's words, copied to pinned host memory and waited for under the group's deadline (host
//      round trip 1); the agreement and the plan (group_plan.hpp pr_agree, fp_plan_for), where some
//      owner receives more than its buffers hold after a growth-confirm exchange
//   2  ncclSend / ncclRecv of the 24-byte requests to their owners (a rank's own part: a device copy);
//      the owner holds them grouped by asker in rank order
//   3  the owner scans the clipped lengths of all it received (memfs.hip mf_pread_scan_launch, the
//      group's aggregate scratch): offsets, a count and a some byte per request, and one tiny launch
//      for the bytes T[o][s] it owes each asker, from the offsets at the asker boundaries
//   4  counts and some bytes back to the askers; the all-gather of every owner's row of T with its
//      TW_* words, read back (host round trip 2): the capacity decision and every byte offset
//      (pr_bytes_agree, pr_byte_plan_for); where a data buffer must grow, growth-confirm again
//   5  the owner's packed bytes (mf_pread_copy_launch, the host-known total as cap), sent to the
//      askers: an asker's receive buffer is then its answer packed in partition order
//   6  the re-pack into request order (mf_repack_scan_launch, mf_repack_copy_launch)
// A capacity failure (some rank's answer exceeds its cap) stops after step 4 and still runs step 6's
// scan, so that every rank's offs and some are complete. A one-rank group (pt_ident) runs the pread
// kernels straight into the caller's buffers and reads offs[n] back for the capacity answer.
#include <algorithm>

#include "group.hpp"

using namespace nrg::grp;

int PrMember::init(Member& m, int nranks) {
    GCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    // the fixed-size buffers of the two exchanges (so that a call cannot fail on them)
    const uint64_t G = (uint64_t)nranks, CW = rw_cw(nranks), TW = tw_cw(nranks);
    RCHK(grow_buf(m, b[RB_CNT], CW * 8));
    RCHK(grow_buf(m, b[RB_ALLCNT], G * CW * 8));
    RCHK(grow_buf(m, b[RB_TOT], TW * 8));
    RCHK(grow_buf(m, b[RB_ALLTOT], G * TW * 8));
    RCHK(grow_buf(m, b[RB_ROFFS], 8));  // (an owner that receives nothing still scans: offs[0] = 0)
    GCHK(hipHostMalloc(&h_cnt, G * CW * 8, hipHostMallocDefault));
    GCHK(hipHostMalloc(&h_tot, G * TW * 8, hipHostMallocDefault));
    return NRG_OK;
}

void PrMember::free() {
    for (DBuf& d : b) free_buf(d);
    if (h_cnt) (void)hipHostFree(h_cnt);
    if (h_tot) (void)hipHostFree(h_tot);
    if (ev) (void)hipEventDestroy(ev);
    h_cnt = h_tot = nullptr;
    ev = nullptr;
}

namespace {

int grow(Member& m, PrBuf k, uint64_t bytes) { return grow_buf(m, m.pr.b[k], bytes); }

// requests its owner-side buffers hold now
uint64_t recv_cap(const Member& m) {
    const DBuf* b = m.pr.b;
    const uint64_t offs = b[RB_ROFFS].bytes / 8;  // (one word more than requests)
    return std::min({b[RB_RREQ].bytes / PR_REQ_BYTES, offs ? offs - 1 : 0, b[RB_RCNT].bytes / 8, b[RB_RSOME].bytes,
                     b[RB_RAGG].bytes / 8 * 1024});
}

// ... grown to hold n
int recv_grow(Member& m, uint64_t n) {
    RCHK(grow(m, RB_RREQ, n * PR_REQ_BYTES));
    RCHK(grow(m, RB_ROFFS, (n + 1) * 8));
    RCHK(grow(m, RB_RCNT, n * 8));
    RCHK(grow(m, RB_RSOME, n));
    return grow(m, RB_RAGG, nrg::mf_pread_agg_words(n) * 8);
}

// what this member's own part of the call is worth before anything is exchanged
int local_check(const Member& m, const nrg_pread& x) {
    const nrg_ctx* c = m.ctx;
    if (c->cfg.ds_kind != NRG_DS_MEMFS) return NRG_E_INVAL;
    if (c->growth.max_items) return NRG_E_INVAL;  // a bound on a member: group_files.cpp local_check
    if ((x.n && (!x.reqs || !x.offs || !x.some)) || (x.cap && !x.data)) return NRG_E_INVAL;
    if (((uintptr_t)x.reqs | (uintptr_t)x.offs) & 7) return NRG_E_INVAL;
    if (c->ltail < c->tail) return NRG_E_NOT_SYNCED;
    if (x.n >= (1ull << 32)) return NRG_E_CAPACITY;  // positions are u32
    return NRG_OK;
}

// every local member's words from `dev` (its own when the group has one rank: the all-gather is the
// identity) to its pinned `host`, waited for under the group's deadline
int read_back(nrg_group* g, PrBuf own, PrBuf all, uint64_t* PrMember::*host, uint64_t cw, const char* phase) {
    const int G = g->nranks;
    if (G > 1)
        RCHK(collective(g, phase, [&](Member& m, int) {
            return g->R->all_gather(m.pr.b[own].p, m.pr.b[all].p, cw, ncclUint64, m.comm, m.ctx->stream);
        }));
    for (Member& m : g->m) {
        RCHK(nrg::ctx_use_device(m.ctx));
        GCHK(hipMemcpyAsync(m.pr.*host, m.pr.b[G > 1 ? all : own].p, (uint64_t)G * cw * 8, hipMemcpyDeviceToHost,
                            m.ctx->stream));
        GCHK(hipEventRecord(m.pr.ev, m.ctx->stream));
    }
    for (Member& m : g->m) {
        RCHK(nrg::ctx_use_device(m.ctx));
        RCHK(wait_event(g, m.pr.ev, phase));
    }
    return NRG_OK;
}

// Every rank grew (or failed to grow) its buffers: all learn the first failure in rank order before
// any send / recv that needs them (as group_files.cpp fp_plan_and_grow confirms a round's growth).
int confirm(nrg_group* g, const std::vector<int>& grow_err, const char* phase) {
    const int nl = (int)g->m.size();
    std::vector<uint64_t> a(nl), b(nl, 0);
    for (int i = 0; i < nl; i++) a[i] = (uint64_t)(-grow_err[i]);
    RCHK(exchange_pairs(g, a, b, phase));
    const uint64_t* H = g->m[0].h_gwx;
    for (int s = 0; s < g->nranks; s++)
        if (H[2 * s]) return -(int)H[2 * s];
    return NRG_OK;
}

// Step 1 up to the host's copy of every rank's words: H (identical on every rank).
int pr_exchange(nrg_group* g, const nrg_pread* reads, std::vector<uint64_t>& n_own, const uint64_t** H) {
    const int G = g->nranks, nl = (int)g->m.size();
    for (int i = 0; i < nl; i++) {
        Member& m = g->m[i];
        nrg_ctx* c = m.ctx;
        const nrg_pread& x = reads[i];
        RCHK(nrg::ctx_use_device(c));
        if (m.in_set && m.in_stream != c->stream) RCHK(order(m, m.in_stream, c->stream));
        int err = local_check(m, x);
        // the asker's buffers follow its own n
        const PrBuf mine[] = {RB_OUT, RB_POS, RB_ACNT, RB_ASOME, RB_SOFFS, RB_AAGG};
        const uint64_t bytes[] = {x.n * PR_REQ_BYTES, x.n * 4, x.n * 8, x.n, (x.n + 1) * 8, nrg::mf_pread_agg_words(x.n) * 8};
        for (int k = 0; k < 6 && err == NRG_OK; k++) err = grow(m, mine[k], bytes[k]);
        const uint64_t n = err ? 0 : x.n;  // a bad part takes part in the exchange with no requests
        n_own[i] = n;
        uint64_t* cnt = (uint64_t*)m.pr.b[RB_CNT].p;
        const hipError_t he = nrg::rd_partition(c, x.reqs, n, (uint32_t)G, (nrg_memfs_rd*)m.pr.b[RB_OUT].p,
                                                (uint32_t*)m.pr.b[RB_POS].p, cnt);
        if (he != hipSuccess) return hip_rc(he);
        uint64_t w[RW_N] = {};
        w[RW_CAP] = recv_cap(m);
        w[RW_ERR] = (uint64_t)(-err);
        w[RW_KIND] = c->cfg.ds_kind;
        w[RW_FILES] = c->mf.files;
        w[RW_LOG2B] = c->mf.log2_b;
        w[RW_SIZED] = c->mf.d_size ? 1 : 0;
        w[RW_DCAP] = x.cap;
        RCHK(put_words(c->stream, cnt + G, w, (uint32_t)RW_N));
    }
    RCHK(read_back(g, RB_CNT, RB_ALLCNT, &PrMember::h_cnt, rw_cw(G), "group pread: count exchange"));
    *H = g->m[0].pr.h_cnt;
    return NRG_OK;
}

// The plan of every local member; where some owner has to grow its buffers (every rank knows), all
// grow and confirm before any send / recv.
int pr_plan_and_grow(nrg_group* g, const uint64_t* H, const std::vector<uint64_t>& n_own, bool any_grow) {
    const int G = g->nranks, nl = (int)g->m.size();
    std::vector<int> grow_err(nl, NRG_OK);
    for (int i = 0; i < nl; i++) {
        Member& m = g->m[i];
        fp_plan_for(H, G, m.rank, m.pr.plan);
        if (m.pr.plan.sent != n_own[i]) grow_err[i] = NRG_E_HIP;  // the partition kernels disagree with the caller's n
        if (any_grow && grow_err[i] == NRG_OK) {
            RCHK(nrg::ctx_use_device(m.ctx));
            grow_err[i] = recv_grow(m, m.pr.plan.recvd);
        }
    }
    if (any_grow) return confirm(g, grow_err, "group pread: growth confirm (requests)");
    for (int e : grow_err)
        if (e) return e;  // cannot happen: the counts come from the same requests
    return NRG_OK;
}

// One send / recv step along a plan, `unit` bytes per plan entry (a rank's own part: a device copy).
// fwd: a rank sends its to / to_off groups from `sbuf` and receives its from / from_off groups into
// `rbuf` (requests to their owners; bytes to their askers, whose plan is written from the owner's
// side). Otherwise the reverse: what it holds by from / from_off goes back and lands by to / to_off
// (the counts and some bytes of the requests it sent).
template <typename Plan>
int pr_swap(nrg_group* g, Plan PrMember::*plan, PrBuf sbuf, PrBuf rbuf, uint64_t unit, bool fwd, const char* phase) {
    const Rccl* R = g->R;
    const int G = g->nranks;
    auto side = [&](const Plan& P, bool send, int o, uint64_t* off) {  // bytes of this rank's send / recv with o
        const bool by_to = send == fwd;
        *off = (by_to ? P.to_off[o] : P.from_off[o]) * unit;
        return (by_to ? P.to[o] : P.from[o]) * unit;
    };
    if (G > 1)
        RCHK(collective(g, phase, [&](Member& m, int) {
            const Plan& P = m.pr.*plan;
            hipStream_t s = m.ctx->stream;
            ncclResult_t res = ncclSuccess;
            for (int o = 0; o < G && res == ncclSuccess; o++) {
                if (o == m.rank) continue;
                uint64_t off = 0;
                if (const uint64_t nb = side(P, true, o, &off)) res = R->send(at(m.pr.b[sbuf].p, off), nb, ncclUint8, o, m.comm, s);
                const uint64_t nb = side(P, false, o, &off);
                if (res == ncclSuccess && nb) res = R->recv(at(m.pr.b[rbuf].p, off), nb, ncclUint8, o, m.comm, s);
            }
            return res;
        }));
    for (Member& m : g->m) {
        const Plan& P = m.pr.*plan;
        uint64_t soff = 0, roff = 0;
        const uint64_t nb = side(P, true, m.rank, &soff);
        (void)side(P, false, m.rank, &roff);
        if (!nb) continue;
        RCHK(nrg::ctx_use_device(m.ctx));
        GCHK(hipMemcpyAsync(at(m.pr.b[rbuf].p, roff), at(m.pr.b[sbuf].p, soff), nb, hipMemcpyDeviceToDevice, m.ctx->stream));
    }
    return NRG_OK;
}

// Step 3: an owner's scan of what it received, and its words of the second exchange
int pr_owner_scan(nrg_group* g) {
    const int G = g->nranks;
    for (Member& m : g->m) {
        nrg_ctx* c = m.ctx;
        RCHK(nrg::ctx_use_device(c));
        const DBuf* b = m.pr.b;
        const uint64_t recvd = m.pr.plan.recvd;
        hipError_t he = nrg::mf_pread_scan_launch(c, (const nrg_memfs_rd*)b[RB_RREQ].p, recvd, (uint64_t*)b[RB_ROFFS].p,
                                                  (uint8_t*)b[RB_RSOME].p, (uint64_t*)b[RB_RCNT].p, (uint64_t*)b[RB_RAGG].p);
        if (he == hipSuccess)
            he = nrg::mf_pread_totals_launch(c, (const uint64_t*)b[RB_ROFFS].p, recvd,
                                             (const uint64_t*)b[G > 1 ? RB_ALLCNT : RB_CNT].p, (uint32_t)G,
                                             (uint32_t)rw_cw(G), (uint32_t)m.rank, (uint64_t*)b[RB_TOT].p);
        if (he != hipSuccess) return hip_rc(he);
        uint64_t w[TW_N] = {};
        w[TW_SCAP] = b[RB_SDATA].bytes;
        w[TW_RCAP] = b[RB_RDATA].bytes;
        RCHK(put_words(c->stream, (uint64_t*)b[RB_TOT].p + G, w, (uint32_t)TW_N));
    }
    return NRG_OK;
}

// The byte plan of every local member; where a data buffer has to grow, all grow and confirm.
int pr_bytes_plan_and_grow(nrg_group* g, const uint64_t* T, bool any_grow) {
    const int G = g->nranks, nl = (int)g->m.size();
    std::vector<int> grow_err(nl, NRG_OK);
    for (int i = 0; i < nl; i++) {
        Member& m = g->m[i];
        pr_byte_plan_for(T, G, m.rank, m.pr.bytes);
        if (!any_grow) continue;
        RCHK(nrg::ctx_use_device(m.ctx));
        grow_err[i] = grow(m, RB_SDATA, m.pr.bytes.sent);
        if (grow_err[i] == NRG_OK) grow_err[i] = grow(m, RB_RDATA, pr_recv_room(m.pr.bytes.recvd));
    }
    return any_grow ? confirm(g, grow_err, "group pread: growth confirm (bytes)") : NRG_OK;
}

// Step 6's scan for every local member: offs and some of its own requests from the counts that came back
int pr_repack_scan(nrg_group* g, const nrg_pread* reads, const std::vector<uint64_t>& n_own) {
    for (size_t i = 0; i < g->m.size(); i++) {
        Member& m = g->m[i];
        const DBuf* b = m.pr.b;
        RCHK(nrg::ctx_use_device(m.ctx));
        const hipError_t he = nrg::mf_repack_scan_launch(m.ctx, (const uint64_t*)b[RB_ACNT].p, (const uint8_t*)b[RB_ASOME].p,
                                                         (const uint32_t*)b[RB_POS].p, n_own[i], reads[i].offs, reads[i].some,
                                                         (uint64_t*)b[RB_SOFFS].p, (uint64_t*)b[RB_AAGG].p);
        if (he != hipSuccess) return hip_rc(he);
    }
    return NRG_OK;
}

int wait_all(nrg_group* g) {
    for (Member& m : g->m) {
        RCHK(nrg::ctx_use_device(m.ctx));
        RCHK(wait_stream(g, m.ctx->stream, "group pread"));
    }
    return NRG_OK;
}

// A one-rank group without the measurement knob: the member's checks are the agreement, the pread
// kernels answer straight into the caller's buffers, and offs[n] comes back for the capacity answer.
int pr_ident(nrg_group* g, const nrg_pread& x, int rc) {
    Member& m = g->m[0];
    nrg_ctx* c = m.ctx;
    RCHK(nrg::ctx_use_device(c));
    RCHK(local_check(m, x));
    if (m.in_set && m.in_stream != c->stream) RCHK(order(m, m.in_stream, c->stream));
    RCHK(grow(m, RB_AAGG, nrg::mf_pread_agg_words(x.n) * 8));
    hipError_t he = nrg::mf_pread_scan_launch(c, x.reqs, x.n, x.offs, x.some, nullptr, (uint64_t*)m.pr.b[RB_AAGG].p);
    if (he == hipSuccess)
        he = nrg::mf_pread_copy_launch(c, x.reqs, x.n, x.offs, x.data, x.cap, nrg::mf_pread_bound(c, x.n, x.cap));
    if (he != hipSuccess) return hip_rc(he);
    m.pr.h_tot[0] = 0;
    if (x.n) GCHK(hipMemcpyAsync(m.pr.h_tot, x.offs + x.n, 8, hipMemcpyDeviceToHost, c->stream));
    RCHK(wait_stream(g, c->stream, "group pread"));
    if (m.pr.h_tot[0] > x.cap) return NRG_E_CAPACITY;
    return rc;
}

}  // namespace

extern "C" {

int nrg_group_memfs_pread(nrg_group* g, const nrg_pread* reads) {
    RCHK(pt_check(g));
    if (!reads) return NRG_E_INVAL;
    // queued group work first; a latched device error of this rank is reported at the end, after it
    // has taken its part in the collectives (as the group-wide skip-list reads)
    const int rc = nrg_group_sync(g);
    if (g->broken) return g->broken;
    if (pt_ident(g, g->m[0])) return pr_ident(g, reads[0], rc);
    const int G = g->nranks, nl = (int)g->m.size();
    std::vector<uint64_t> n_own(nl, 0);
    const uint64_t *H = nullptr, *T = nullptr;
    RCHK(pr_exchange(g, reads, n_own, &H));
    const PrAgree A = pr_agree(H, G);
    if (A.rc) return A.rc;  // on every rank, before any request moves
    if (A.asked) {
        RCHK(pr_plan_and_grow(g, H, n_own, A.any_grow));
        RCHK(pr_swap(g, &PrMember::plan, RB_OUT, RB_RREQ, PR_REQ_BYTES, true, "group pread: requests to their owners"));
        RCHK(pr_owner_scan(g));
        RCHK(pr_swap(g, &PrMember::plan, RB_RCNT, RB_ACNT, 8, false, "group pread: counts back"));
        RCHK(pr_swap(g, &PrMember::plan, RB_RSOME, RB_ASOME, 1, false, "group pread: some bytes back"));
        RCHK(read_back(g, RB_TOT, RB_ALLTOT, &PrMember::h_tot, tw_cw(G), "group pread: byte exchange"));
        T = g->m[0].pr.h_tot;
    }
    // (nothing asked: every offs[0] = 0 below, nothing else to do)
    const PrBytes B = A.asked ? pr_bytes_agree(H, T, G) : PrBytes{};
    if (A.asked && B.rc == NRG_OK) {
        RCHK(pr_bytes_plan_and_grow(g, T, B.any_grow));
        for (Member& m : g->m) {  // step 5: the owner's packed bytes
            const DBuf* b = m.pr.b;
            const uint64_t sent = m.pr.bytes.sent;
            RCHK(nrg::ctx_use_device(m.ctx));
            const hipError_t he = nrg::mf_pread_copy_launch(m.ctx, (const nrg_memfs_rd*)b[RB_RREQ].p, m.pr.plan.recvd,
                                                            (const uint64_t*)b[RB_ROFFS].p, (uint8_t*)b[RB_SDATA].p, sent, sent);
            if (he != hipSuccess) return hip_rc(he);
        }
        RCHK(pr_swap(g, &PrMember::bytes, RB_SDATA, RB_RDATA, 1, true, "group pread: bytes to the askers"));
    }
    RCHK(pr_repack_scan(g, reads, n_own));  // (a rank without requests: offs[0] = 0, if it gave offs)
    if (A.asked && B.rc == NRG_OK)
        for (int i = 0; i < nl; i++) {
            Member& m = g->m[i];
            const DBuf* b = m.pr.b;
            const uint64_t total = m.pr.bytes.recvd;  // <= cap: the agreement
            RCHK(nrg::ctx_use_device(m.ctx));
            const hipError_t he = nrg::mf_repack_copy_launch(m.ctx, (const uint8_t*)b[RB_RDATA].p, (const uint64_t*)b[RB_SOFFS].p,
                                                             (const uint32_t*)b[RB_POS].p, n_own[i], reads[i].offs, reads[i].data,
                                                             reads[i].cap, total);
            if (he != hipSuccess) return hip_rc(he);
        }
    RCHK(wait_all(g));
    return B.rc ? B.rc : rc;
}

}  // extern "C"
