// group_partitioned.cpp — cnr-style key-partitioned rounds of a replica group (SURVEY.md §8 f4;
// cnr/src/replica.rs:430-445, :673-736; include/nrgpu.h, nrg_group_partitioned_*).
//
// Partitioned rounds, pipelined over three calls (nrg_group_partitioned_round_async):
//   call e     post(e):    the fused partition of round e's Puts and Gets into owner regions
//                          (partition.hip pt_fused, which also writes the member's exchange words)
//                          and the all-gather of every rank's counts, copied to pinned host memory
//                          behind an event;
//   call e+1   stage A(e): its counts (landed long ago: no host wait in steady state), the plan,
//                          Puts and Get keys to their owners (RCCL send/recv; a rank's own part is a
//                          device copy, or none with one rank), the owner's replay with the reads
//                          deferred: they ride in round e+1's index launch (the replicated
//                          pipeline's overlap);
//   call e+2   stage B(e): (round e's reads were launched in stage A(e+1)) answers and previous
//                          values back to the ranks that asked, one route-back launch into the
//                          caller's order.
// Everything runs on the replica's stream. Every failure before a round's first send/recv is
// agreed on by all ranks (the same exchanged words, group_plan.hpp plan_agree): the round is
// dropped everywhere and the call that ran its stage A returns the error.
// A group of skip-list replicas (the reference's skiplist-mlnr, benches/lockfree.rs:228-317) takes
// the same rounds: the records are Push(k, v), the owner's replay is nrg_skiplist_round_async per
// slice and nrg_skiplist_get_async for the Gets, nothing is deferred, and the Push responses
// Ok(Some(key)) are written on the asker's side in stage B (they never travel: XW_PREV = 0). A group
// that agreed on removal (group_pops.cpp) also carries Remove(k): there the owners' replay answers
// every received record and the responses come back as a hashmap's previous values do; one that
// agreed on pops looks for mark records in the post step and refuses a round that holds one.
// A one-rank group owns every key, so its partition is the identity and so is the route-back
// (pt_ident): the owner's replay reads the caller's records and Get keys and answers straight into
// the caller's buffers -- no data moves, as a cnr replica with one log appends and replays in place
// (cnr/src/replica.rs:673-736). NRG_KNOB_EXP bit 16 (measurement) makes a one-rank group move
// its data like a multi-rank one: partition copy on the side stream, route-back launch.
#include <algorithm>

#include "../../include/nrgpu_testing.h"
#include "group.hpp"

using namespace nrg::grp;

int PtMember::init(Member& m, int nranks) {
    for (int q = 0; q < PT_DEPTH; q++) GCHK(hipEventCreateWithFlags(&cnt_ev[q], hipEventDisableTiming));
    GCHK(hipEventCreateWithFlags(&pin_ev, hipEventDisableTiming));
    // the fixed-size buffers of a round's count and status exchanges
    const uint64_t G = (uint64_t)nranks, CW = xw_cw(nranks);
    for (int q = 0; q < PT_DEPTH; q++) {
        RCHK(grow_buf(m, pp[q][PP_CNT], CW * 8));
        RCHK(grow_buf(m, pp[q][PP_ALLCNT], G * CW * 8));
        // mapped: a one-rank group's partition writes its counts here directly (no exchange)
        GCHK(hipHostMalloc(&h_cnt[q], G * CW * 8, hipHostMallocMapped));
    }
    RCHK(grow_buf(m, pt[PB_ST], 8));
    return grow_buf(m, pt[PB_ALLST], G * 8);
}

void PtMember::free() {
    for (DBuf& d : pt) free_buf(d);
    for (int q = 0; q < PT_DEPTH; q++) {
        for (DBuf& d : pp[q]) free_buf(d);
        if (h_cnt[q]) (void)hipHostFree(h_cnt[q]);
        if (cnt_ev[q]) (void)hipEventDestroy(cnt_ev[q]);
    }
    for (int q = 0; q < 2; q++)
        for (DBuf& d : rv[q]) free_buf(d);
    if (pin_ev) (void)hipEventDestroy(pin_ev);
}

namespace {

// A partitioned skip-list round's Push responses, Ok(Some(key)) (benches/lockfree_partitioned.rs:
// 108-111): they do not depend on the state, so the asker writes them from its own records.
__global__ __launch_bounds__(GRP_TPB) void grp_push_resp_kernel(const nrg_put* __restrict__ recs, uint64_t n,
                                                                uint64_t* __restrict__ resp, uint8_t* __restrict__ some) {
    for (uint64_t i = blockIdx.x * (uint64_t)GRP_TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * GRP_TPB) {
        resp[i] = recs[i].key;
        some[i] = 1;
    }
}

// A group that agreed on pops (nrg_group_skiplist_enable_pops): a record whose val is a mark would be
// routed by the hash of its count and pop one partition's front, so a round that holds one is refused.
// One pass over the member's records; a mark makes *err_word -NRG_E_INVAL (the member's XW_ERR, zero
// before: the lanes that find one all store the same word).
__global__ __launch_bounds__(GRP_TPB) void grp_find_marks_kernel(const nrg_put* __restrict__ recs, uint64_t n, uint64_t fm,
                                                                 uint64_t bm, uint64_t* err_word) {
    bool hit = false;
    for (uint64_t i = blockIdx.x * (uint64_t)GRP_TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * GRP_TPB) {
        const uint64_t v = recs[i].val;
        hit |= v == fm || v == bm;
    }
    if (hit) *err_word = (uint64_t)(-NRG_E_INVAL);
}

int grow(Member& m, PtBuf k, uint64_t bytes) { return grow_buf(m, m.pt.pt[k], bytes); }

int pt_post(nrg_group* g, const nrg_round* rounds, uint64_t e) {
    const int G = g->nranks, nl = (int)g->m.size();
    const int sl = (int)(e % PT_DEPTH), par = (int)(e & 1);
    const uint64_t CW = xw_cw(G);
    for (int i = 0; i < nl; i++) {
        Member& m = g->m[i];
        PtMember& t = m.pt;
        const nrg_round& x = rounds[i];
        nrg_ctx* c = m.ctx;
        int err = NRG_OK;
        const uint32_t kind = c->cfg.ds_kind;
        // (a skip list with removal: a Remove's response is not the asker's to write, see grp_push_resp_kernel,
        // unless the group agreed on it and the owners answer; with pops: the front of a key-partitioned
        // map is no member's own, and a group that agreed on them refuses the mark records below)
        if ((kind != NRG_DS_HASHMAP && kind != NRG_DS_SKIPLIST) || (nrg::sl_removal(c) && !g->sl_rm) ||
            (nrg::sl_pops(c) && !g->sl_pops) ||
            (x.n && !x.recs) ||
            (x.n_gets && (!x.get_keys || !x.get_vals || !x.get_found)))
            err = NRG_E_INVAL;
        else if (x.n >= (1ull << 32) || x.n_gets >= (1ull << 32) || (uint64_t)G * x.n >= (1ull << 32) ||
                 (uint64_t)G * x.n_gets >= (1ull << 32))
            err = NRG_E_CAPACITY;  // positions are u32 owner-region offsets
        RCHK(nrg::ctx_use_device(c));
        if (m.in_set && m.in_stream != c->stream) RCHK(order(m, m.in_stream, c->stream));
        const uint64_t n = err ? 0 : x.n, k = err ? 0 : x.n_gets;
        if (err == NRG_OK) {
            DBuf* pp = t.pp[sl];
            const uint64_t bytes[] = {G * n * 16, n * 4, G * k * 8, k * 4};
            const PtPar which[] = {PP_POUT, PP_PPOS, PP_KOUT, PP_GPOS};
            for (int q = 0; q < 4 && err == NRG_OK; q++) err = grow_buf(m, pp[which[q]], bytes[q]);
            if (err == NRG_OK) err = grow(m, PB_DESC, nrg::pt_desc_words(n, k, (uint32_t)G) * 8);
            // owner-region answer buffers (a single rank's answers need none: they stay in RVAL)
            if (err == NRG_OK && G > 1) {
                const PtBuf ans[] = {PB_AVAL, PB_AFOUND, PB_APREV, PB_APREVF};
                const uint64_t ab[] = {G * k * 8, G * k, G * n * 8, G * n};
                for (int q = 0; q < 4 && err == NRG_OK; q++) err = grow(m, ans[q], ab[q]);
            }
        }
        uint64_t* w = t.xwords;
        // (a skip list's Push responses are its own keys: they never travel, see pt_stage_b; on a group
        // that agreed on removal they are the owners' and travel as the hashmap's previous values do)
        w[XW_PREV] = ((kind == NRG_DS_HASHMAP || g->sl_rm) && x.resp && x.some) ? 1 : 0;
        w[XW_KIND] = kind;
        // receive capacities of the round's parity (one rank replays straight from its partition
        // output: no RPUT / RKEY)
        const DBuf* rv = t.rv[par];
        const uint64_t rp_own = std::min(rv[PR_RPREV].bytes / 8, rv[PR_RPREVF].bytes);
        const uint64_t rk_own = std::min(rv[PR_RVAL].bytes / 8, rv[PR_RFOUND].bytes);
        w[XW_RP_CAP] = G == 1 ? rp_own : std::min(rv[PR_RPUT].bytes / 16, rp_own);
        w[XW_RK_CAP] = G == 1 ? rk_own : std::min(rv[PR_RKEY].bytes / 8, rk_own);
        w[XW_ERR] = (uint64_t)(-err);
        for (int q = 0; q < (int)XW_N; q++) t.xw1[sl][q] = w[q];
        // A one-rank group partitions on a side stream, after everything queued on the replica's
        // stream so far (the inputs, the slot's previous round), beside the previous round's
        // replay queued next (with RCCL the partition stays in line: the count exchange must keep
        // its place among the communicator's operations)
        if (pt_ident(g, m)) {  // nothing to partition (the counts are n, n_gets; the words are xw1)
            t.xw1[sl][XW_RP_CAP] = t.xw1[sl][XW_RK_CAP] = ~0ull;  // nothing received: no buffer to grow
            t.pr[sl] = x;
            t.cap_p[sl] = err ? 0 : n;
            t.cap_k[sl] = err ? 0 : k;
            if (g->sl_pops) {  // the mark pass writes the slot's mapped error word: stage A waits for it
                uint64_t* ew = &t.h_cnt[sl][2 * G + XW_ERR];
                *ew = 0;  // (the slot's previous round is through stage A: nothing on the device writes it now)
                if (n) {
                    grp_find_marks_kernel<<<grp_grid(n), GRP_TPB, 0, c->stream>>>((const nrg_put*)x.recs, n, g->sl_front,
                                                                                 g->sl_back, ew);
                    GCHK(hipGetLastError());
                    g->launches[nrg_group::L_MARKS]++;
                }
                GCHK(hipEventRecord(t.cnt_ev[sl], c->stream));
            }
            continue;
        }
        hipStream_t ps = c->stream;
        if (G == 1) {
            ps = m.pstream;
            GCHK(hipEventRecord(t.pin_ev, c->stream));
            GCHK(hipStreamWaitEvent(ps, t.pin_ev, 0));
        }
        if (++t.epoch >= (1u << 22)) {  // the descriptor tag wraps: clear the stale ones once
            t.epoch = 1;
            if (t.pt[PB_DESC].p) GCHK(hipMemsetAsync(t.pt[PB_DESC].p, 0, t.pt[PB_DESC].bytes, ps));
        }
        const bool ok = err == NRG_OK;
        const hipError_t he = nrg::pt_fused(ps, (const uint64_t*)x.recs, ok ? n : 0, n,
                                            (uint64_t*)t.pp[sl][PP_POUT].p, (uint32_t*)t.pp[sl][PP_PPOS].p,
                                            x.get_keys, ok ? k : 0, k, (uint64_t*)t.pp[sl][PP_KOUT].p,
                                            (uint32_t*)t.pp[sl][PP_GPOS].p, (uint64_t*)t.pt[PB_DESC].p, (uint32_t)G,
                                            t.epoch, G == 1 ? t.h_cnt[sl] : (uint64_t*)t.pp[sl][PP_CNT].p, w,
                                            XW_N);
        if (he != hipSuccess) return hip_rc(he);
        g->launches[nrg_group::L_FUSED]++;
        if (g->sl_pops && ok && n) {  // after the partition wrote the words: a mark record makes XW_ERR -NRG_E_INVAL
            uint64_t* cnt = G == 1 ? t.h_cnt[sl] : (uint64_t*)t.pp[sl][PP_CNT].p;
            grp_find_marks_kernel<<<grp_grid(n), GRP_TPB, 0, ps>>>((const nrg_put*)x.recs, n, g->sl_front, g->sl_back,
                                                                  cnt + 2 * G + XW_ERR);
            GCHK(hipGetLastError());
            g->launches[nrg_group::L_MARKS]++;
        }
        t.pr[sl] = x;
        t.cap_p[sl] = n;
        t.cap_k[sl] = k;
    }
    if (G > 1)  // (one rank's all-gather is the identity: its partition wrote h_cnt itself)
        RCHK(collective(g, "partitioned count exchange", [&](Member& m, int) {
            return g->R->all_gather(m.pt.pp[sl][PP_CNT].p, m.pt.pp[sl][PP_ALLCNT].p, CW, ncclUint64, m.comm,
                                    m.ctx->stream);
        }));
    for (int i = 0; i < nl; i++) {
        Member& m = g->m[i];
        RCHK(nrg::ctx_use_device(m.ctx));
        if (pt_ident(g, m)) continue;
        if (G > 1)
            GCHK(hipMemcpyAsync(m.pt.h_cnt[sl], m.pt.pp[sl][PP_ALLCNT].p, (uint64_t)G * CW * 8, hipMemcpyDeviceToHost,
                                m.ctx->stream));
        GCHK(hipEventRecord(m.pt.cnt_ev[sl], G == 1 ? m.pstream : m.ctx->stream));
    }
    return NRG_OK;
}

// Stage A, step 1: the round's exchanged words H, identical on every rank. A one-rank group owns
// every key: its counts are its own n and n_gets and its words are its own (written into H1), so
// the host does not wait for the partition (the replay waits for it on the device).
int pt_counts(nrg_group* g, int sl, uint64_t* H1, const uint64_t** H) {
    const int G = g->nranks;
    for (Member& m : g->m) {
        RCHK(nrg::ctx_use_device(m.ctx));
        if (G == 1) {
            if (!pt_ident(g, m)) GCHK(hipStreamWaitEvent(m.ctx->stream, m.pt.cnt_ev[sl], 0));  // (side stream)
            H1[0] = m.pt.cap_p[sl];
            H1[1] = m.pt.cap_k[sl];
            for (int q = 0; q < (int)XW_N; q++) H1[2 + q] = m.pt.xw1[sl][q];
            // a group that agreed on pops pays a host wait here: the mark pass of the post step has the
            // last word on the round's error (a mark record: the round is dropped before any replay)
            if (g->sl_pops) {
                RCHK(wait_event(g, m.pt.cnt_ev[sl], "partitioned round: mark records"));
                if (!H1[2 + XW_ERR]) H1[2 + XW_ERR] = m.pt.h_cnt[sl][2 + XW_ERR];
            }
        } else {
            RCHK(wait_event(g, m.pt.cnt_ev[sl], "partitioned count exchange"));
        }
    }
    *H = G == 1 ? H1 : g->m[0].pt.h_cnt[sl];
    return NRG_OK;
}

// Stage A, steps 3 and 4: every local member's plan; where some rank has to grow its receive
// buffers (any_grow: every rank knows), all grow and confirm before any send/recv.
int pt_plan_and_grow(nrg_group* g, int sl, int par, const uint64_t* H, bool any_grow) {
    const int G = g->nranks, nl = (int)g->m.size();
    std::vector<int> grow_err(nl, NRG_OK);
    for (int i = 0; i < nl; i++) {
        Member& m = g->m[i];
        PtPlan& P = m.pt.plan[sl];
        plan_for(H, G, m.rank, P);
        if (P.sp != m.pt.cap_p[sl] || P.sk != m.pt.cap_k[sl]) grow_err[i] = NRG_E_HIP;  // partition kernel disagrees
        if (any_grow && grow_err[i] == NRG_OK) {
            RCHK(nrg::ctx_use_device(m.ctx));
            const PtRecv recv[] = {PR_RPUT, PR_RPREV, PR_RPREVF, PR_RKEY, PR_RVAL, PR_RFOUND};
            const uint64_t bytes[] = {G > 1 ? P.rp * 16 : 0, P.rp * 8, P.rp, G > 1 ? P.rk * 8 : 0, P.rk * 8, P.rk};
            for (int k = 0; k < 6 && grow_err[i] == NRG_OK; k++) grow_err[i] = grow_buf(m, m.pt.rv[par][recv[k]], bytes[k]);
        }
    }
    if (!any_grow) {
        for (int i = 0; i < nl; i++)
            if (grow_err[i]) return grow_err[i];  // cannot happen: the counts come from the same kernel
        return NRG_OK;
    }
    for (int i = 0; i < nl; i++) {
        Member& m = g->m[i];
        RCHK(nrg::ctx_use_device(m.ctx));
        m.pt.xwords[0] = (uint64_t)(-grow_err[i]);
        GCHK(hipMemcpyAsync(m.pt.pt[PB_ST].p, m.pt.xwords, 8, hipMemcpyHostToDevice, m.ctx->stream));
    }
    RCHK(collective(g, "partitioned status exchange", [&](Member& m, int) {
        return g->R->all_gather(m.pt.pt[PB_ST].p, m.pt.pt[PB_ALLST].p, 1, ncclUint64, m.comm, m.ctx->stream);
    }));
    std::vector<uint64_t> st(G);
    for (int i = 0; i < nl; i++) {
        Member& m = g->m[i];
        RCHK(nrg::ctx_use_device(m.ctx));
        GCHK(hipMemcpyAsync(st.data(), m.pt.pt[PB_ALLST].p, (uint64_t)G * 8, hipMemcpyDeviceToHost, m.ctx->stream));
        RCHK(wait_stream(g, m.ctx->stream, "partitioned status exchange"));
    }
    for (int s = 0; s < G; s++)
        if (st[s]) return -(int)st[s];
    return NRG_OK;
}

// Stage A, step 5 (G > 1): Puts and Get keys to their owners (own part: a device copy)
int pt_move(nrg_group* g, int sl, int par) {
    const Rccl* R = g->R;
    const int G = g->nranks;
    RCHK(collective(g, "partitioned send/recv of Puts and Gets", [&](Member& m, int) {
        const PtPlan& P = m.pt.plan[sl];
        const uint64_t cp = m.pt.cap_p[sl], ck = m.pt.cap_k[sl];
        void *pout = m.pt.pp[sl][PP_POUT].p, *kout = m.pt.pp[sl][PP_KOUT].p;
        const DBuf* rv = m.pt.rv[par];
        hipStream_t s = m.ctx->stream;
        ncclResult_t res = ncclSuccess;
        for (int o = 0; o < G && res == ncclSuccess; o++) {
            if (o == m.rank) continue;
            if (P.pto[o]) res = R->send(at(pout, o * cp * 16), P.pto[o] * 2, ncclUint64, o, m.comm, s);
            if (res == ncclSuccess && P.pfrom[o])
                res = R->recv(at(rv[PR_RPUT].p, P.pfrom_off[o] * 16), P.pfrom[o] * 2, ncclUint64, o, m.comm, s);
            if (res == ncclSuccess && P.gto[o]) res = R->send(at(kout, o * ck * 8), P.gto[o], ncclUint64, o, m.comm, s);
            if (res == ncclSuccess && P.gfrom[o])
                res = R->recv(at(rv[PR_RKEY].p, P.gfrom_off[o] * 8), P.gfrom[o], ncclUint64, o, m.comm, s);
        }
        return res;
    }));
    for (Member& m : g->m) {
        const PtPlan& P = m.pt.plan[sl];
        const DBuf* rv = m.pt.rv[par];
        const int r = m.rank;
        RCHK(nrg::ctx_use_device(m.ctx));
        if (P.pto[r])
            GCHK(hipMemcpyAsync(at(rv[PR_RPUT].p, P.pfrom_off[r] * 16), at(m.pt.pp[sl][PP_POUT].p, r * m.pt.cap_p[sl] * 16),
                                P.pto[r] * 16, hipMemcpyDeviceToDevice, m.ctx->stream));
        if (P.gto[r])
            GCHK(hipMemcpyAsync(at(rv[PR_RKEY].p, P.gfrom_off[r] * 8), at(m.pt.pp[sl][PP_KOUT].p, r * m.pt.cap_k[sl] * 8),
                                P.gto[r] * 8, hipMemcpyDeviceToDevice, m.ctx->stream));
    }
    return NRG_OK;
}

// Where an owner's replay reads its Puts and Get keys and writes the Gets' answers: the caller's
// own buffers (identity), the partition output (one rank), or what it received.
struct OwnerIo {
    const nrg_put* rput;
    const uint64_t* rkey;
    uint64_t* rval;
    uint8_t* rfound;
};
OwnerIo owner_io(const nrg_group* g, const Member& m, int sl, int par) {
    const nrg_round& x = m.pt.pr[sl];
    const DBuf* rv = m.pt.rv[par];
    if (pt_ident(g, m)) return {(const nrg_put*)x.recs, x.get_keys, x.get_vals, x.get_found};
    const void* rput = g->nranks == 1 ? m.pt.pp[sl][PP_POUT].p : rv[PR_RPUT].p;
    const void* rkey = g->nranks == 1 ? m.pt.pp[sl][PP_KOUT].p : rv[PR_RKEY].p;
    return {(const nrg_put*)rput, (const uint64_t*)rkey, (uint64_t*)rv[PR_RVAL].p, (uint8_t*)rv[PR_RFOUND].p};
}

// Stage A, step 6: an owner replays the Puts it received (rank order) and answers the Gets it
// received; the reads (and a stamp round's apply) are deferred into the next round's first launch.
// A skewed round can hand one owner more Puts than its max_batch (or ring) takes in one replay:
// consecutive rounds of at most that many, the Gets answered after the last.
int owner_replay_hashmap(const nrg_group* g, Member& m, int sl, int par, bool any_prev) {
    const PtPlan& P = m.pt.plan[sl];
    nrg_ctx* c = m.ctx;
    const uint64_t chunk = replay_chunk(c->log_size, c->cfg.max_batch);
    const OwnerIo io = owner_io(g, m, sl, par);
    const bool ident = pt_ident(g, m);
    const nrg_round& x = m.pt.pr[sl];
    // (identity: the caller's own answer buffers, and previous values only if it asked)
    uint64_t* rprev = ident ? (x.resp && x.some ? (uint64_t*)x.resp : nullptr)
                            : any_prev ? (uint64_t*)m.pt.rv[par][PR_RPREV].p : nullptr;
    uint8_t* rprevf = ident ? (x.resp && x.some ? x.some : nullptr)
                            : any_prev ? (uint8_t*)m.pt.rv[par][PR_RPREVF].p : nullptr;
    uint64_t off = 0;
    do {
        const uint64_t n = std::min(chunk, P.rp - off);
        const bool last = off + n == P.rp;
        if (n || (last && P.rk))
            RCHK(nrg_hashmap_round_async(c, io.rput + off, n, (uint32_t)m.rank + 1, last ? io.rkey : nullptr,
                                         last ? P.rk : 0, last ? io.rval : nullptr, last ? io.rfound : nullptr,
                                         rprev ? rprev + off : nullptr, rprevf ? rprevf + off : nullptr));
        off += n;
    } while (off < P.rp);
    // a round with nothing for this owner launches nothing, and the previous round's reads
    // would wait for a later launch while its answers go back in this call's stage B: now
    if (P.rp == 0 && P.rk == 0) RCHK(nrg_join(c));
    return NRG_OK;
}

// Push(k, v) slices in rank order, then the Gets against the post-round state. The skip list
// defers nothing; its chunk replay synchronises this stream now and then (the counts behind the
// compaction policy and growth), which every send and recv it waits for allows: they were all
// enqueued before any member's replay.
// Identity form: the responses Ok(Some(key)) come from the replay itself.
// A group that agreed on removal: where some rank asked for responses, the replay answers every
// received record (Push: the key; Remove: the previous value or None) into the receive-side
// previous-value buffers, chunk by chunk at the chunk's offset, and stage B takes them back to the
// askers as it takes a hashmap's previous values.
int owner_replay_skiplist(const nrg_group* g, Member& m, int sl, int par, bool any_prev) {
    const PtPlan& P = m.pt.plan[sl];
    nrg_ctx* c = m.ctx;
    const uint64_t chunk = replay_chunk(c->log_size, c->cfg.max_batch);
    const OwnerIo io = owner_io(g, m, sl, par);
    const nrg_round& x = m.pt.pr[sl];
    const bool owners = g->sl_rm && any_prev && !pt_ident(g, m);
    uint64_t* presp = owners ? (uint64_t*)m.pt.rv[par][PR_RPREV].p
                             : pt_ident(g, m) && x.resp && x.some ? (uint64_t*)x.resp : nullptr;
    uint8_t* psome = owners ? (uint8_t*)m.pt.rv[par][PR_RPREVF].p : presp ? x.some : nullptr;
    for (uint64_t off = 0; off < P.rp; off += chunk) {
        const uint64_t n = std::min(chunk, P.rp - off);
        RCHK(nrg_skiplist_round_async(c, io.rput + off, n, (uint32_t)m.rank + 1, presp ? presp + off : nullptr,
                                      psome ? psome + off : nullptr));
    }
    return sl_gets(c, io.rkey, P.rk, io.rval, io.rfound);
}

// Stage A of round e: wait for its counts, agree, plan, grow and confirm, move, replay.
int pt_stage_a(nrg_group* g, uint64_t e) {
    const int sl = (int)(e % PT_DEPTH), par = (int)(e & 1);
    g->pt.drop[sl] = true;  // until the round's payload has moved
    uint64_t H1[2 + XW_N];
    const uint64_t* H = nullptr;
    RCHK(pt_counts(g, sl, H1, &H));
    const PlanAgree A = plan_agree(H, g->nranks);
    if (A.rc) return A.rc;
    RCHK(pt_plan_and_grow(g, sl, par, H, A.any_grow));
    g->pt.drop[sl] = false;
    if (g->nranks > 1) RCHK(pt_move(g, sl, par));
    for (Member& m : g->m) {
        RCHK(nrg::ctx_use_device(m.ctx));
        RCHK(A.kind == NRG_DS_SKIPLIST ? owner_replay_skiplist(g, m, sl, par, A.any_prev)
                                       : owner_replay_hashmap(g, m, sl, par, A.any_prev));
    }
    return NRG_OK;
}

// Stage B of round e: its reads and previous values are queued (launched with the next round's
// replay, or by the flush's join).
int pt_stage_b(nrg_group* g, uint64_t e) {
    const Rccl* R = g->R;
    const int G = g->nranks;
    const int sl = (int)(e % PT_DEPTH), par = (int)(e & 1);
    if (g->pt.drop[sl]) return NRG_OK;  // dropped in stage A (its error was returned there)
    // (the kind every rank agreed on in stage A: a skip list's Push responses never travel, unless
    // the group agreed on removal: then the owners answered and the responses come back)
    const bool skiplist = g->m[0].ctx->cfg.ds_kind == NRG_DS_SKIPLIST;
    const bool travel = !skiplist || g->sl_rm;
    const uint64_t* H = g->m[0].pt.h_cnt[sl];
    if (G > 1)  // answers back to the ranks that asked, into their owner regions
        RCHK(collective(g, "partitioned answers back", [&](Member& m, int) {
            const PtPlan& P = m.pt.plan[sl];
            const bool mine = travel && m.pt.pr[sl].resp && m.pt.pr[sl].some;
            const uint64_t cp = m.pt.cap_p[sl], ck = m.pt.cap_k[sl];
            const DBuf *rv = m.pt.rv[par], *pt = m.pt.pt;
            hipStream_t s = m.ctx->stream;
            ncclResult_t res = ncclSuccess;
            for (int o = 0; o < G && res == ncclSuccess; o++) {
                if (o == m.rank) continue;
                const bool theirs = xw_word(H, G, o, XW_PREV) != 0;
                if (P.gfrom[o]) {
                    res = R->send(at(rv[PR_RVAL].p, P.gfrom_off[o] * 8), P.gfrom[o], ncclUint64, o, m.comm, s);
                    if (res == ncclSuccess)
                        res = R->send(at(rv[PR_RFOUND].p, P.gfrom_off[o]), P.gfrom[o], ncclUint8, o, m.comm, s);
                }
                if (res == ncclSuccess && P.gto[o]) {
                    res = R->recv(at(pt[PB_AVAL].p, o * ck * 8), P.gto[o], ncclUint64, o, m.comm, s);
                    if (res == ncclSuccess) res = R->recv(at(pt[PB_AFOUND].p, o * ck), P.gto[o], ncclUint8, o, m.comm, s);
                }
                if (res == ncclSuccess && theirs && P.pfrom[o]) {
                    res = R->send(at(rv[PR_RPREV].p, P.pfrom_off[o] * 8), P.pfrom[o], ncclUint64, o, m.comm, s);
                    if (res == ncclSuccess)
                        res = R->send(at(rv[PR_RPREVF].p, P.pfrom_off[o]), P.pfrom[o], ncclUint8, o, m.comm, s);
                }
                if (res == ncclSuccess && mine && P.pto[o]) {
                    res = R->recv(at(pt[PB_APREV].p, o * cp * 8), P.pto[o], ncclUint64, o, m.comm, s);
                    if (res == ncclSuccess) res = R->recv(at(pt[PB_APREVF].p, o * cp), P.pto[o], ncclUint8, o, m.comm, s);
                }
            }
            return res;
        }));
    // back into the caller's order (one launch for the Gets' answers and the previous values)
    for (Member& m : g->m) {
        const PtMember& t = m.pt;
        const PtPlan& P = t.plan[sl];
        const nrg_round& x = t.pr[sl];
        nrg_ctx* c = m.ctx;
        const int r = m.rank;
        if (pt_ident(g, m)) continue;  // the replay answered into the caller's buffers
        RCHK(nrg::ctx_use_device(c));
        const bool mine = travel && x.resp && x.some;
        const uint64_t cp = t.cap_p[sl], ck = t.cap_k[sl];
        const DBuf* rv = t.rv[par];
        void *aval = t.pt[PB_AVAL].p, *afound = t.pt[PB_AFOUND].p, *aprev = t.pt[PB_APREV].p, *aprevf = t.pt[PB_APREVF].p;
        if (G == 1) {
            aval = rv[PR_RVAL].p, afound = rv[PR_RFOUND].p, aprev = rv[PR_RPREV].p, aprevf = rv[PR_RPREVF].p;
        } else {
            hipStream_t s = c->stream;
            if (P.gto[r]) {
                GCHK(hipMemcpyAsync(at(aval, r * ck * 8), at(rv[PR_RVAL].p, P.gfrom_off[r] * 8), P.gto[r] * 8,
                                    hipMemcpyDeviceToDevice, s));
                GCHK(hipMemcpyAsync(at(afound, r * ck), at(rv[PR_RFOUND].p, P.gfrom_off[r]), P.gto[r],
                                    hipMemcpyDeviceToDevice, s));
            }
            if (mine && P.pto[r]) {
                GCHK(hipMemcpyAsync(at(aprev, r * cp * 8), at(rv[PR_RPREV].p, P.pfrom_off[r] * 8), P.pto[r] * 8,
                                    hipMemcpyDeviceToDevice, s));
                GCHK(hipMemcpyAsync(at(aprevf, r * cp), at(rv[PR_RPREVF].p, P.pfrom_off[r]), P.pto[r],
                                    hipMemcpyDeviceToDevice, s));
            }
        }
        const hipError_t he = nrg::pt_route2(
            c->stream, (const uint64_t*)aval, (const uint8_t*)afound, (const uint32_t*)t.pp[sl][PP_GPOS].p, x.n_gets,
            x.get_vals, x.get_found, (const uint64_t*)aprev, (const uint8_t*)aprevf,
            (const uint32_t*)t.pp[sl][PP_PPOS].p, mine ? x.n : 0, mine ? (uint64_t*)x.resp : nullptr, mine ? x.some : nullptr);
        if (he != hipSuccess) return hip_rc(he);
        g->launches[nrg_group::L_ROUTE]++;
        if (skiplist && !travel && x.n && x.resp && x.some) {  // Ok(Some(key)) from the asker's own records
            grp_push_resp_kernel<<<grp_grid(x.n), GRP_TPB, 0, c->stream>>>((const nrg_put*)x.recs, x.n,
                                                                          (uint64_t*)x.resp, x.some);
            GCHK(hipGetLastError());
            g->launches[nrg_group::L_PUSH_RESP]++;
        }
    }
    g->round++;
    return NRG_OK;
}

// every local member's deferred reads, now
int pt_join(nrg_group* g) {
    for (Member& m : g->m) {
        RCHK(nrg::ctx_use_device(m.ctx));
        RCHK(nrg_join(m.ctx));
    }
    return NRG_OK;
}

// every posted round through stage B (its result: the first error)
int pt_flush(nrg_group* g) {
    PtGroup& t = g->pt;
    int rc = NRG_OK;
    while (t.a < t.posted) {
        const int r = pt_stage_a(g, t.a++);
        if (g->broken) return g->broken;
        if (r && rc == NRG_OK) rc = r;
    }
    if (t.b < t.a) RCHK(pt_join(g));  // the last round's deferred reads
    while (t.b < t.a) {
        const int r = pt_stage_b(g, t.b++);
        if (g->broken) return g->broken;
        if (r && rc == NRG_OK) rc = r;
    }
    if (g->nranks == 1)  // a one-rank group's partitions ran on its side stream: ordered again
        for (Member& m : g->m) {
            RCHK(nrg::ctx_use_device(m.ctx));
            RCHK(order(m, m.pstream, m.ctx->stream));
        }
    return rc;
}

}  // namespace

int nrg::grp::pt_flush_posted(nrg_group* g) { return g->pt.b < g->pt.posted ? pt_flush(g) : NRG_OK; }

int nrg::grp::pt_check(nrg_group* g) {
    if (!g) return NRG_E_INVAL;
    if (g->broken) return g->broken;
    const Rccl* R = g->R;
    if (!R || !R->send || !R->recv) return NRG_E_COMM;
    if (g->nranks > NRG_MAX_PARTS) return NRG_E_INVAL;
    return NRG_OK;
}

extern "C" {

int nrg_test_group_launches(const nrg_group* g, uint64_t out[4]) {
    if (!g || !out) return NRG_E_INVAL;
    for (int k = 0; k < nrg_group::L_N; k++) out[k] = g->launches[k];
    return NRG_OK;
}

int nrg_group_partitioned_round_async(nrg_group* g, const nrg_round* rounds) {
    int r = pt_check(g);
    if (r) return r;
    if (!rounds) return NRG_E_INVAL;
    PtGroup& t = g->pt;
    if ((r = pt_post(g, rounds, t.posted))) return r;
    t.posted++;
    int rc = NRG_OK;
    if (t.posted - t.a >= 2) {  // the previous round: its counts have landed by now
        rc = pt_stage_a(g, t.a++);
        if (g->broken) return g->broken;
    }
    if (t.a - t.b >= 2) {  // the round before: its reads rode in the launch just queued
        if (rc != NRG_OK) RCHK(pt_join(g));  // (that round was dropped, so nothing launched them: now)
        const int r2 = pt_stage_b(g, t.b++);
        if (g->broken) return g->broken;
        if (r2 && rc == NRG_OK) rc = r2;
    }
    return rc;
}

int nrg_group_partitioned_flush(nrg_group* g) {
    const int r = pt_check(g);
    return r ? r : pt_flush(g);
}

int nrg_group_partitioned_round(nrg_group* g, const nrg_round* rounds) {
    int r = pt_check(g);
    if (r) return r;
    if (!rounds) return NRG_E_INVAL;
    if ((r = pt_flush(g))) return r;
    if ((r = pt_post(g, rounds, g->pt.posted))) return r;
    g->pt.posted++;
    return pt_flush(g);
}

}  // extern "C"
