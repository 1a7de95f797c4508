// group_files.cpp — file-partitioned rounds of a group of file-store replicas, as benches/nrfs.rs runs
// them (include/nrgpu.h, nrg_group_file_round; DESIGN.md §7 "File-partitioned rounds (nrfs-mlnr)").
//
// nrfs.rs is a cnr benchmark with one log per file: LogMapper::hash() = fd - 1 (benches/nrfs.rs:25-39),
// LogStrategy::Custom(logs) (:132-141), hash % logs (cnr/src/replica.rs:430-445), and each log is
// combined and replayed on its own (:673-736). Here the log of partition p lives on rank p: a round's
// records travel to the owners of their files (common.hpp file_owner), every owner replays what it
// received in rank order, each rank's part in issue order (for every file the order of the NR global
// log W_0 || W_1 || ... restricted to it), and the responses travel back. Every member holds all F files;
// a round changes only the files the member owns.
//
// One round, everything on the replica's stream:
//   1  the partition of the member's records by owner (partition.hip fp_partition), whose counts are the
//      first G of the member's exchange words; the FW_* words follow them (fp_words_kernel)
//   2  the all-gather of every rank's words, copied to pinned host memory and waited for under the
//      group's deadline (the round's one host round trip)
//   3  the agreement and the plan (group_plan.hpp fp_agree, fp_plan_for): every rank reaches the same
//      code from the same words, so a bad round is dropped everywhere before any payload moves
//   4  where some rank receives more than its buffers hold: all grow and confirm (as pt_plan_and_grow)
//   5  ncclSend / ncclRecv of the records to their owners (a rank's own part: a device copy)
//   6  the owner's replay, nrg_memfs_round_async in slices of replay_chunk records, origin = rank + 1
//   7  responses and some bytes back to the ranks that asked, into the partition output's order
//   8  one route-back launch into the caller's order (partition.hip fp_route)
// A one-rank group owns every file: it replays the caller's records into the caller's buffers and
// nothing moves (pt_ident; NRG_KNOB_EXP bit 16 makes it partition, replay from the partition's output
// and route back, for measurement).
#include <algorithm>

#include "group.hpp"

using namespace nrg::grp;

int FpMember::init(Member& m, int nranks) {
    GCHK(hipEventCreateWithFlags(&cnt_ev, hipEventDisableTiming));
    // the fixed-size buffers of the count and status exchanges (so that a round cannot fail on them)
    const uint64_t G = (uint64_t)nranks, CW = fw_cw(nranks);
    RCHK(grow_buf(m, b[FB_CNT], CW * 8));
    RCHK(grow_buf(m, b[FB_ALLCNT], G * CW * 8));
    GCHK(hipHostMalloc(&h_cnt, G * CW * 8, hipHostMallocDefault));
    RCHK(grow_buf(m, b[FB_ST], 8));
    return grow_buf(m, b[FB_ALLST], G * 8);
}

void FpMember::free() {
    for (DBuf& d : b) free_buf(d);
    if (h_cnt) (void)hipHostFree(h_cnt);
    if (cnt_ev) (void)hipEventDestroy(cnt_ev);
    h_cnt = nullptr;
    cnt_ev = nullptr;
}

namespace {

// dst[k] = w.v[k] in stream order (kernel arguments are captured at launch)
struct FpWords {
    uint64_t v[FW_N];
};
__global__ void fp_words_kernel(uint64_t* dst, FpWords w, uint32_t n) {
    if (threadIdx.x == 0) {  // (constant indices: a lane-indexed argument array goes to scratch)
#pragma unroll
        for (uint32_t k = 0; k < FW_N; k++)
            if (k < n) dst[k] = w.v[k];
    }
}

int grow(Member& m, FpBuf k, uint64_t bytes) { return grow_buf(m, m.fp.b[k], bytes); }

// records its receive buffers hold now (one rank replays from its partition output: no FB_RREC)
uint64_t recv_cap(const Member& m, int G) {
    const DBuf* b = m.fp.b;
    const uint64_t a = std::min(b[FB_RRESP].bytes / FP_RESP_BYTES, b[FB_RSOME].bytes);
    return G == 1 ? a : std::min(a, b[FB_RREC].bytes / FP_REC_BYTES);
}

// what this member's own part of the round is worth before anything is exchanged
int local_check(const Member& m, const nrg_round& x) {
    if (m.ctx->cfg.ds_kind != NRG_DS_MEMFS || (x.n && !x.recs) || x.n_gets || x.get_keys) return NRG_E_INVAL;
    // An owner replays its own files' records alone, so growth under replay would let the members' B
    // diverge: a member with a bound (nrg_set_max_capacity) is refused, and every rank learns it from the
    // exchange. Such a group grows with nrg_memfs_reserve on every member.
    if (m.ctx->growth.max_items) return NRG_E_INVAL;
    if (((uintptr_t)x.recs | (uintptr_t)x.resp) & 7) return NRG_E_INVAL;  // (records and responses move as u64 words)
    if (x.n >= (1ull << 32)) return NRG_E_CAPACITY;                        // positions are u32
    return NRG_OK;
}

// Steps 1 and 2: partition, words, exchange; H = every rank's words (identical on every rank).
int fp_exchange(nrg_group* g, const nrg_round* rounds, std::vector<uint64_t>& n_own, const uint64_t** H) {
    const int G = g->nranks, nl = (int)g->m.size();
    const uint64_t CW = fw_cw(G);
    for (int i = 0; i < nl; i++) {
        Member& m = g->m[i];
        nrg_ctx* c = m.ctx;
        const nrg_round& x = rounds[i];
        RCHK(nrg::ctx_use_device(c));
        if (m.in_set && m.in_stream != c->stream) RCHK(order(m, m.in_stream, c->stream));
        int err = local_check(m, x);
        const bool wants = x.resp && x.some;
        if (err == NRG_OK) err = grow(m, FB_OUT, fp_rec_at(x.n));
        if (err == NRG_OK) err = grow(m, FB_POS, x.n * 4);
        if (err == NRG_OK && wants && G > 1) {  // (one rank's answers stay in FB_RRESP / FB_RSOME)
            err = grow(m, FB_ARESP, fp_resp_at(x.n));
            if (err == NRG_OK) err = grow(m, FB_ASOME, fp_some_at(x.n));
        }
        const uint64_t n = err ? 0 : x.n;  // a bad part takes part in the exchange with no records
        n_own[i] = n;
        uint64_t* cnt = (uint64_t*)m.fp.b[FB_CNT].p;
        const hipError_t he = nrg::fp_partition(c, (const nrg_memfs_op*)x.recs, n, (uint32_t)G,
                                                (nrg_memfs_op*)m.fp.b[FB_OUT].p, (uint32_t*)m.fp.b[FB_POS].p, cnt);
        if (he != hipSuccess) return hip_rc(he);
        FpWords w{};
        w.v[FW_CAP] = recv_cap(m, G);
        w.v[FW_ERR] = (uint64_t)(-err);
        w.v[FW_KIND] = c->cfg.ds_kind;
        w.v[FW_FILES] = c->mf.files;
        w.v[FW_LOG2B] = c->mf.log2_b;
        w.v[FW_SIZED] = c->mf.d_size ? 1 : 0;
        w.v[FW_RESP] = wants ? 1 : 0;
        fp_words_kernel<<<1, 64, 0, c->stream>>>(cnt + G, w, (uint32_t)FW_N);
        GCHK(hipGetLastError());
    }
    if (G > 1)
        RCHK(collective(g, "file-partitioned count exchange", [&](Member& m, int) {
            return g->R->all_gather(m.fp.b[FB_CNT].p, m.fp.b[FB_ALLCNT].p, CW, ncclUint64, m.comm, m.ctx->stream);
        }));
    for (Member& m : g->m) {
        RCHK(nrg::ctx_use_device(m.ctx));
        // (one rank's all-gather is the identity)
        GCHK(hipMemcpyAsync(m.fp.h_cnt, m.fp.b[G > 1 ? FB_ALLCNT : FB_CNT].p, (uint64_t)G * CW * 8, hipMemcpyDeviceToHost,
                            m.ctx->stream));
        GCHK(hipEventRecord(m.fp.cnt_ev, m.ctx->stream));
    }
    for (Member& m : g->m) {
        RCHK(nrg::ctx_use_device(m.ctx));
        RCHK(wait_event(g, m.fp.cnt_ev, "file-partitioned count exchange"));
    }
    *H = g->m[0].fp.h_cnt;
    return NRG_OK;
}

// Steps 3 and 4: every local member's plan; where some rank has to grow its receive buffers
// (any_grow: every rank knows), all grow and confirm before any send / recv.
int fp_plan_and_grow(nrg_group* g, const uint64_t* H, const std::vector<uint64_t>& n_own, bool any_grow) {
    const int G = g->nranks, nl = (int)g->m.size();
    std::vector<int> grow_err(nl, NRG_OK);
    for (int i = 0; i < nl; i++) {
        Member& m = g->m[i];
        FpPlan& P = m.fp.plan;
        fp_plan_for(H, G, m.rank, P);
        if (P.sent != n_own[i]) grow_err[i] = NRG_E_HIP;  // the partition kernels disagree with the caller's n
        if (any_grow && grow_err[i] == NRG_OK) {
            RCHK(nrg::ctx_use_device(m.ctx));
            const FpBuf recv[] = {FB_RREC, FB_RRESP, FB_RSOME};
            const uint64_t bytes[] = {G > 1 ? fp_rec_at(P.recvd) : 0, fp_resp_at(P.recvd), fp_some_at(P.recvd)};
            for (int k = 0; k < 3 && grow_err[i] == NRG_OK; k++) grow_err[i] = grow(m, recv[k], bytes[k]);
        }
    }
    if (!any_grow) {
        for (int i = 0; i < nl; i++)
            if (grow_err[i]) return grow_err[i];  // cannot happen: the counts come from the same records
        return NRG_OK;
    }
    for (int i = 0; i < nl; i++) {
        Member& m = g->m[i];
        RCHK(nrg::ctx_use_device(m.ctx));
        FpWords w{};
        w.v[0] = (uint64_t)(-grow_err[i]);
        fp_words_kernel<<<1, 64, 0, m.ctx->stream>>>((uint64_t*)m.fp.b[FB_ST].p, w, 1u);
        GCHK(hipGetLastError());
    }
    RCHK(collective(g, "file-partitioned status exchange", [&](Member& m, int) {
        return g->R->all_gather(m.fp.b[FB_ST].p, m.fp.b[FB_ALLST].p, 1, ncclUint64, m.comm, m.ctx->stream);
    }));
    std::vector<uint64_t> st(G);
    for (int i = 0; i < nl; i++) {
        Member& m = g->m[i];
        RCHK(nrg::ctx_use_device(m.ctx));
        GCHK(hipMemcpyAsync(st.data(), m.fp.b[FB_ALLST].p, (uint64_t)G * 8, hipMemcpyDeviceToHost, m.ctx->stream));
        RCHK(wait_stream(g, m.ctx->stream, "file-partitioned status exchange"));
    }
    for (int s = 0; s < G; s++)
        if (st[s]) return -(int)st[s];
    return NRG_OK;
}

// Step 5 (G > 1): the records to their owners
int fp_move(nrg_group* g) {
    const Rccl* R = g->R;
    const int G = g->nranks;
    RCHK(collective(g, "file-partitioned send/recv of records", [&](Member& m, int) {
        const FpPlan& P = m.fp.plan;
        void *out = m.fp.b[FB_OUT].p, *rrec = m.fp.b[FB_RREC].p;
        hipStream_t s = m.ctx->stream;
        ncclResult_t res = ncclSuccess;
        for (int o = 0; o < G && res == ncclSuccess; o++) {
            if (o == m.rank) continue;
            if (P.to[o]) res = R->send(at(out, fp_rec_at(P.to_off[o])), fp_rec_at(P.to[o]) / 8, ncclUint64, o, m.comm, s);
            if (res == ncclSuccess && P.from[o])
                res = R->recv(at(rrec, fp_rec_at(P.from_off[o])), fp_rec_at(P.from[o]) / 8, ncclUint64, o, m.comm, s);
        }
        return res;
    }));
    for (Member& m : g->m) {
        const FpPlan& P = m.fp.plan;
        const int r = m.rank;
        RCHK(nrg::ctx_use_device(m.ctx));
        if (P.to[r])
            GCHK(hipMemcpyAsync(at(m.fp.b[FB_RREC].p, fp_rec_at(P.from_off[r])), at(m.fp.b[FB_OUT].p, fp_rec_at(P.to_off[r])),
                                fp_rec_at(P.to[r]), hipMemcpyDeviceToDevice, m.ctx->stream));
    }
    return NRG_OK;
}

// Step 6: an owner replays what it received, in slices its max_batch and its ring take. A slice
// boundary may fall inside a long write's run: the run stays contiguous in the owner's log.
int fp_replay(Member& m, const nrg_memfs_op* recs, uint64_t n, nrg_memfs_resp* resp, uint8_t* some) {
    nrg_ctx* c = m.ctx;
    const uint64_t chunk = replay_chunk(c->log_size, c->cfg.max_batch);
    for (uint64_t off = 0; off < n; off += chunk)
        RCHK(nrg_memfs_round_async(c, recs + off, std::min(chunk, n - off), (uint32_t)m.rank + 1, resp ? resp + off : nullptr,
                                   some ? some + off : nullptr));
    return NRG_OK;
}

// Step 7 (G > 1): responses and some bytes back to the ranks that asked (own part: device copies)
int fp_answers(nrg_group* g, uint64_t wants) {
    const Rccl* R = g->R;
    const int G = g->nranks;
    RCHK(collective(g, "file-partitioned responses back", [&](Member& m, int) {
        const FpPlan& P = m.fp.plan;
        const DBuf* b = m.fp.b;
        const bool mine = wants >> m.rank & 1;
        hipStream_t s = m.ctx->stream;
        ncclResult_t res = ncclSuccess;
        for (int o = 0; o < G && res == ncclSuccess; o++) {
            if (o == m.rank) continue;
            if ((wants >> o & 1) && P.from[o]) {
                res = R->send(at(b[FB_RRESP].p, fp_resp_at(P.from_off[o])), fp_resp_at(P.from[o]) / 8, ncclUint64, o, m.comm, s);
                if (res == ncclSuccess)
                    res = R->send(at(b[FB_RSOME].p, fp_some_at(P.from_off[o])), P.from[o], ncclUint8, o, m.comm, s);
            }
            if (res == ncclSuccess && mine && P.to[o]) {
                res = R->recv(at(b[FB_ARESP].p, fp_resp_at(P.to_off[o])), fp_resp_at(P.to[o]) / 8, ncclUint64, o, m.comm, s);
                if (res == ncclSuccess)
                    res = R->recv(at(b[FB_ASOME].p, fp_some_at(P.to_off[o])), P.to[o], ncclUint8, o, m.comm, s);
            }
        }
        return res;
    }));
    for (Member& m : g->m) {
        const FpPlan& P = m.fp.plan;
        const DBuf* b = m.fp.b;
        const int r = m.rank;
        if (!(wants >> r & 1) || !P.to[r]) continue;
        RCHK(nrg::ctx_use_device(m.ctx));
        GCHK(hipMemcpyAsync(at(b[FB_ARESP].p, fp_resp_at(P.to_off[r])), at(b[FB_RRESP].p, fp_resp_at(P.from_off[r])),
                            fp_resp_at(P.to[r]), hipMemcpyDeviceToDevice, m.ctx->stream));
        GCHK(hipMemcpyAsync(at(b[FB_ASOME].p, fp_some_at(P.to_off[r])), at(b[FB_RSOME].p, fp_some_at(P.from_off[r])),
                            fp_some_at(P.to[r]), hipMemcpyDeviceToDevice, m.ctx->stream));
    }
    return NRG_OK;
}

// A one-rank group without the measurement knob: the member's checks are the agreement, its records
// replay where they lie and the responses land where the caller wants them.
int fp_round_ident(nrg_group* g, const nrg_round& x) {
    Member& m = g->m[0];
    RCHK(nrg::ctx_use_device(m.ctx));
    RCHK(local_check(m, x));
    if (m.in_set && m.in_stream != m.ctx->stream) RCHK(order(m, m.in_stream, m.ctx->stream));
    const bool wants = x.resp && x.some;
    RCHK(fp_replay(m, (const nrg_memfs_op*)x.recs, x.n, wants ? (nrg_memfs_resp*)x.resp : nullptr, wants ? x.some : nullptr));
    g->round++;
    return NRG_OK;
}

}  // namespace

int nrg::grp::put_words(hipStream_t s, uint64_t* dst, const uint64_t* v, uint32_t n) {
    if (n > FW_N) return NRG_E_INVAL;
    FpWords w{};
    for (uint32_t k = 0; k < n; k++) w.v[k] = v[k];
    fp_words_kernel<<<1, 64, 0, s>>>(dst, w, n);
    GCHK(hipGetLastError());
    return NRG_OK;
}

extern "C" {

int nrg_group_file_round(nrg_group* g, const nrg_round* rounds) {
    int r = pt_check(g);
    if (r) return r;
    if (!rounds) return NRG_E_INVAL;
    if ((r = pt_flush_posted(g))) return r;  // (a posted key-partitioned round: this kind's is dropped there)
    const int G = g->nranks, nl = (int)g->m.size();
    if (pt_ident(g, g->m[0])) return fp_round_ident(g, rounds[0]);
    std::vector<uint64_t> n_own(nl, 0);
    const uint64_t* H = nullptr;
    RCHK(fp_exchange(g, rounds, n_own, &H));
    const FpAgree A = fp_agree(H, G);
    if (A.rc) return A.rc;  // on every rank, before any payload moves
    RCHK(fp_plan_and_grow(g, H, n_own, A.any_grow));
    if (G > 1) RCHK(fp_move(g));
    for (Member& m : g->m) {
        RCHK(nrg::ctx_use_device(m.ctx));
        const DBuf* b = m.fp.b;
        // (responses are written for everything received once any rank asks: an owner's slices do not
        // follow the ranks' boundaries)
        RCHK(fp_replay(m, (const nrg_memfs_op*)b[G == 1 ? FB_OUT : FB_RREC].p, m.fp.plan.recvd,
                       A.wants ? (nrg_memfs_resp*)b[FB_RRESP].p : nullptr, A.wants ? (uint8_t*)b[FB_RSOME].p : nullptr));
    }
    if (G > 1 && A.wants) RCHK(fp_answers(g, A.wants));
    for (int i = 0; i < nl; i++) {
        Member& m = g->m[i];
        const nrg_round& x = rounds[i];
        if (!(A.wants >> m.rank & 1)) continue;  // asked for nothing: its buffers are not written
        RCHK(nrg::ctx_use_device(m.ctx));
        const DBuf* b = m.fp.b;
        const hipError_t he = nrg::fp_route(m.ctx, (const nrg_memfs_resp*)b[G == 1 ? FB_RRESP : FB_ARESP].p,
                                            (const uint8_t*)b[G == 1 ? FB_RSOME : FB_ASOME].p, (const uint32_t*)b[FB_POS].p,
                                            n_own[i], (nrg_memfs_resp*)x.resp, x.some);
        if (he != hipSuccess) return hip_rc(he);
    }
    g->round++;
    return NRG_OK;
}

}  // extern "C"
