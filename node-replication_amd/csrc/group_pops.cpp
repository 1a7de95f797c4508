// group_pops.cpp — what a partitioned skip-list group opts into as a whole, and its group-wide pop
// (include/nrgpu.h: nrg_group_skiplist_enable_removal / _enable_pops, nrg_group_skiplist_pop).
//
// The opt-ins are collectives: every rank's values and local status are exchanged and every rank
// derives the same code (group_plan.hpp optin_agree) before any member is enabled, so a round never
// finds two owners reading {k, v} differently. What the group agreed on lives in nrg_group;
// group_partitioned.cpp reads it (a removal group's responses come from the owners; a pops group's
// rounds refuse mark records).
//
// The group-wide pop (SkipMap::pop_front / pop_back over the union of G partitions with disjoint key
// sets), on the replica's stream, every collective queued for all local members before any host wait:
//   1  {n, flags, exact length} of every rank, then the requests padded to the longest n: the plan
//      (group_pop_plan.hpp gp_plan), the same host arithmetic on every rank
//   2  every member's candidates (skiplist.hip sl_peek: its min(F, len) smallest and min(Bk, len)
//      largest entries, nothing popped), all-gathered padded to the longest block
//   3  grp_pop_select_kernel, one launch per member: a candidate's rank in the union, the entries of
//      this member's own records to their places, resp / some / *pop_n, and the two records
//      {c_f, front_mark}, {c_b, back_mark} of what this member's partition loses
//   4  nrg_skiplist_round_async of those two device records
// A one-rank group answers with its own pop step (nrg_skiplist_round_pops_async).
#include <algorithm>
#include <cstring>
#include <new>

#include "group.hpp"
#include "group_pop_plan.hpp"

using namespace nrg::grp;

void PoMember::free() {
    for (DBuf& d : b) free_buf(d);
}

namespace {

// A member's part of the plan on the device (PO_PLAN), u64 words:
//   cf[G], cb[G]                  every member's candidate counts
//   grant[n]                      its records' grants in issue order (resp)
//   ffirst[kf], foff[kf]          its front records: first front rank and offset in its packed output
//   bfirst[kb], boff[kb]          its back records
struct PopSel {
    const uint64_t *ck, *cv;  // every member's candidates: [G][stride], front block then back block
    const uint64_t* plan;
    uint64_t stride, cfmax;
    uint32_t G, me;
    uint64_t F, Bk;
    uint64_t n, kf, kb;       // its records, its front records, its back records
    uint64_t fa, fn, ba, bn;  // its front entries are the front ranks [fa, fa + fn), its back entries [ba, ba + bn)
    uint64_t *resp, *pk, *pv, *pop_n;
    uint8_t* some;
    uint64_t cap, total;
    uint64_t* rec;            // {c_f, front_mark, c_b, back_mark}: zero counts before the launch
};

// a candidate's rank at its end of the union (group_pop_plan.hpp gp_cand_rank, which tests/group_pop_plan.cpp
// checks on the host against sorting the union)
__device__ __forceinline__ uint64_t cand_rank(const PopSel& s, bool back, uint32_t o, uint64_t x, uint64_t key) {
    return gp_cand_rank(s.ck, s.stride, s.cfmax, s.plan + (back ? s.G : 0), s.G, back, o, x, key);
}

// Step 3. A work item per candidate slot of the gathered blocks, then one per own record (resp and
// some). A popped candidate whose rank falls among this member's own entries goes to its record's
// place under cap. The member's own lists also give what its partition loses: ranks ascend along a
// list, so the popped candidates are a prefix and the last popped one writes the count.
__global__ __launch_bounds__(GRP_TPB) void grp_pop_select_kernel(PopSel s) {
    const uint64_t slots = (uint64_t)s.G * s.stride;
    const uint64_t *cf = s.plan, *cb = s.plan + s.G, *grant = s.plan + 2 * (uint64_t)s.G;
    const uint64_t *ffirst = grant + s.n, *foff = ffirst + s.kf, *bfirst = foff + s.kf, *boff = bfirst + s.kb;
    for (uint64_t w = blockIdx.x * (uint64_t)GRP_TPB + threadIdx.x; w < slots + s.n; w += (uint64_t)gridDim.x * GRP_TPB) {
        if (w >= slots) {
            const uint64_t j = w - slots;
            if (s.resp) {
                s.resp[j] = grant[j];
                s.some[j] = grant[j] ? 1 : 0;
            }
            continue;
        }
        const uint32_t o = (uint32_t)(w / s.stride);
        uint64_t x = w % s.stride;
        const bool back = x >= s.cfmax;
        if (back) x -= s.cfmax;
        const uint64_t have = back ? cb[o] : cf[o], end = back ? s.Bk : s.F;
        if (x >= have) continue;  // padding
        const uint64_t at = (uint64_t)o * s.stride + (back ? s.cfmax : 0) + x;
        const uint64_t r = cand_rank(s, back, o, x, s.ck[at]);
        if (r >= end) continue;  // stays
        const uint64_t a0 = back ? s.ba : s.fa, an = back ? s.bn : s.fn;
        if (r >= a0 && r - a0 < an) {  // one of this member's own entries
            const uint64_t pos = gp_place(back ? bfirst : ffirst, back ? boff : foff, back ? s.kb : s.kf, r);
            if (pos < s.cap) {
                s.pk[pos] = s.ck[at];
                s.pv[pos] = s.cv[at];
            }
        }
        if (o == s.me) {  // the last popped candidate of its own list: what its partition loses at this end
            const bool last = x + 1 == have || cand_rank(s, back, o, x + 1, s.ck[at + 1]) >= end;
            if (last) s.rec[back ? 2 : 0] = x + 1;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && s.pop_n) *s.pop_n = s.total;
}

// ---- the opt-ins --------------------------------------------------------------------------------------

// a member's state of both settings (no device touched); false: no skip list
struct SlSet {
    uint64_t tomb = 0, front = 0, back = 0;
    int rm = 0, pops = 0;
};
bool settings(nrg_ctx* c, SlSet& s) {
    return nrg_skiplist_removal(c, &s.tomb, &s.rm) == NRG_OK && nrg_skiplist_pops(c, &s.front, &s.back, &s.pops) == NRG_OK;
}

int removal_status(const nrg_group* g, nrg_ctx* c, uint64_t tomb) {
    SlSet s;
    if (!settings(c, s)) return NRG_E_INVAL;
    if (g->sl_rm && tomb != g->sl_tomb) return NRG_E_INVAL;
    if (g->sl_pops && (tomb == g->sl_front || tomb == g->sl_back)) return NRG_E_INVAL;
    if (s.pops && (tomb == s.front || tomb == s.back)) return NRG_E_INVAL;
    if (s.rm) return tomb == s.tomb ? NRG_OK : NRG_E_INVAL;
    return c->ltail != c->tail ? NRG_E_NOT_SYNCED : NRG_OK;
}

int pops_status(const nrg_group* g, nrg_ctx* c, uint64_t fm, uint64_t bm) {
    SlSet s;
    if (!settings(c, s)) return NRG_E_INVAL;
    if (fm == bm) return NRG_E_INVAL;
    if (g->sl_pops && (fm != g->sl_front || bm != g->sl_back)) return NRG_E_INVAL;
    if (g->sl_rm && (fm == g->sl_tomb || bm == g->sl_tomb)) return NRG_E_INVAL;
    if (s.rm && (fm == s.tomb || bm == s.tomb)) return NRG_E_INVAL;
    if (s.pops) return fm == s.front && bm == s.back ? NRG_OK : NRG_E_INVAL;
    return c->ltail != c->tail ? NRG_E_NOT_SYNCED : NRG_OK;
}

// The head of both opt-ins: queued group work completes (its error is this rank's local error), then
// status(member) of every local member. st[i]: the word member i exchanges.
template <typename Status>
int optin_begin(nrg_group* g, std::vector<uint64_t>& st, Status status) {
    if (!g) return NRG_E_INVAL;
    if (g->broken) return g->broken;
    if (!g->R) return NRG_E_COMM;
    const int queued = nrg_group_sync(g);
    if (g->broken) return g->broken;
    st.resize(g->m.size());
    for (size_t i = 0; i < g->m.size(); i++) st[i] = (uint64_t)(-(queued ? queued : status(g->m[i].ctx)));
    return NRG_OK;
}

// The tail: every local member enabled. Its peers enable too, so a member that cannot (out of
// memory) ends the group.
template <typename Enable>
int optin_enable(nrg_group* g, Enable enable) {
    for (Member& m : g->m) {
        RCHK(nrg::ctx_use_device(m.ctx));
        const int r = enable(m.ctx);
        if (r) return group_fail(g, r, "group opt-in: a member could not be enabled after every rank agreed");
    }
    return NRG_OK;
}

// ---- the group-wide pop ---------------------------------------------------------------------------------

// a member's local check: the flags word it exchanges
int pop_args(const nrg_group* g, const nrg_ctx* c, const nrg_pops& x) {
    if (!g->sl_pops || c->cfg.ds_kind != NRG_DS_SKIPLIST || (x.n && !x.reqs) || (!x.resp != !x.some) ||
        (x.pop_cap && (!x.pop_keys || !x.pop_vals)) || (x.n && !x.pop_n))
        return NRG_E_INVAL;
    if (x.n >= (1ull << 32)) return NRG_E_CAPACITY;
    for (uint64_t j = 0; j < x.n; j++)
        if (x.reqs[j].back > 1) return NRG_E_INVAL;
    return c->ltail != c->tail ? NRG_E_NOT_SYNCED : NRG_OK;
}

// its peers are already inside the collectives that follow: the group cannot go on
int po_grow(nrg_group* g, Member& m, PoBuf k, uint64_t bytes) {
    const int r = grow_buf(m, m.po.b[k], bytes);
    return r ? group_fail(g, r, "group-wide pop: scratch allocation failed") : NRG_OK;
}

// Step 1, second half: every rank's requests (host to device, all-gather padded to nmax, back to the host).
// G * nmax <= GP_MAX_REQS, agreed before this (gp_reqs_fit). The requests are staged through pageable
// host vectors; the plain stream synchronise after a member's upload waits for that copy alone, this
// thread's own work and no peer's, so it stands outside the group's deadline. The wait that depends on
// the peers (the all-gather) is under it.
int pop_requests(nrg_group* g, const nrg_pops* pops, const std::vector<uint64_t>& ns, uint64_t nmax,
                 std::vector<nrg_pop_req>& all) {
    const int nl = (int)g->m.size(), G = g->nranks;
    static_assert(sizeof(nrg_pop_req) == 16, "a pop request is two words");
    std::vector<nrg_pop_req> pad(nmax);
    for (int i = 0; i < nl; i++) {
        Member& m = g->m[i];
        RCHK(nrg::ctx_use_device(m.ctx));
        RCHK(po_grow(g, m, PO_SEND, nmax * 16));
        RCHK(po_grow(g, m, PO_ALLREQ, (uint64_t)G * nmax * 16));
        std::fill(pad.begin(), pad.end(), nrg_pop_req{0, 0, 0});
        for (uint64_t j = 0; j < pops[i].n; j++) pad[j] = nrg_pop_req{pops[i].reqs[j].n, pops[i].reqs[j].back, 0};
        GCHK(hipMemcpyAsync(m.po.b[PO_SEND].p, pad.data(), nmax * 16, hipMemcpyHostToDevice, m.cstream));
        GCHK(hipStreamSynchronize(m.cstream));  // (pad is filled again)
    }
    RCHK(collective(g, "group-wide pop: requests", [&](Member& m, int) {
        return g->R->all_gather(m.po.b[PO_SEND].p, m.po.b[PO_ALLREQ].p, 2 * nmax, ncclUint64, m.comm, m.cstream);
    }));
    std::vector<nrg_pop_req> got((uint64_t)G * nmax);
    for (Member& m : g->m) {  // (identical on every member: the last copy stays)
        RCHK(nrg::ctx_use_device(m.ctx));
        GCHK(hipMemcpyAsync(got.data(), m.po.b[PO_ALLREQ].p, (uint64_t)G * nmax * 16, hipMemcpyDeviceToHost, m.cstream));
        RCHK(wait_stream(g, m.cstream, "group-wide pop: requests"));
    }
    all.clear();
    for (int r = 0; r < G; r++) all.insert(all.end(), got.begin() + (uint64_t)r * nmax, got.begin() + (uint64_t)r * nmax + ns[r]);
    return NRG_OK;
}

// A one-rank group: its own pop step over the n records {count, mark}, straight into the caller's buffers
// (the stream synchronise waits for the member's own upload, no peer: outside the group's deadline)
int pop_own(nrg_group* g, Member& m, const nrg_pops& x) {
    nrg_ctx* c = m.ctx;
    RCHK(nrg::ctx_use_device(c));
    RCHK(po_grow(g, m, PO_SEND, x.n * 16));
    std::vector<nrg_put> recs(x.n);
    for (uint64_t j = 0; j < x.n; j++) recs[j] = nrg_put{x.reqs[j].n, x.reqs[j].back ? g->sl_back : g->sl_front};
    if (m.in_set && m.in_stream != c->stream) RCHK(order(m, m.in_stream, c->stream));
    GCHK(hipMemcpyAsync(m.po.b[PO_SEND].p, recs.data(), x.n * 16, hipMemcpyHostToDevice, c->stream));
    GCHK(hipStreamSynchronize(c->stream));  // (recs leaves the stack)
    return nrg_skiplist_round_pops_async(c, (const nrg_put*)m.po.b[PO_SEND].p, x.n, (uint32_t)m.rank + 1, x.resp, x.some,
                                         x.pop_keys, x.pop_vals, x.pop_cap, x.pop_n);
}

// Steps 2 to 4 for every local member
// (words: what the members' streams copy from, alive until they have drained)
int pop_union(nrg_group* g, const nrg_pops* pops, const GpPlan& P, const std::vector<nrg_pop_req>& all,
              std::vector<std::vector<uint64_t>>& words) {
    const int nl = (int)g->m.size(), G = g->nranks;
    const uint64_t stride = P.stride();
    words.assign(nl, {});
    for (int i = 0; i < nl; i++) {  // the scratch, and the member's candidates
        Member& m = g->m[i];
        nrg_ctx* c = m.ctx;
        RCHK(nrg::ctx_use_device(c));
        const uint64_t n = pops[i].n;
        RCHK(po_grow(g, m, PO_CK, stride * 8));
        RCHK(po_grow(g, m, PO_CV, stride * 8));
        RCHK(po_grow(g, m, PO_ALLK, (uint64_t)G * stride * 8));
        RCHK(po_grow(g, m, PO_ALLV, (uint64_t)G * stride * 8));
        RCHK(po_grow(g, m, PO_PLAN, (2 * (uint64_t)G + 3 * n) * 8));
        RCHK(po_grow(g, m, PO_REC, 32));
        if (m.in_set && m.in_stream != c->stream) RCHK(order(m, m.in_stream, c->stream));
        uint64_t *ck = (uint64_t*)m.po.b[PO_CK].p, *cv = (uint64_t*)m.po.b[PO_CV].p;
        const hipError_t he = nrg::sl_peek_launch(c, P.cf[m.rank], P.cb[m.rank], ck, cv, ck + P.cfmax, cv + P.cfmax);
        if (he != hipSuccess) return group_fail(g, hip_rc(he), "group-wide pop: the candidate launch failed");
    }
    if (stride)
        RCHK(collective(g, "group-wide pop: candidates", [&](Member& m, int) {
            ncclResult_t res = g->R->all_gather(m.po.b[PO_CK].p, m.po.b[PO_ALLK].p, stride, ncclUint64, m.comm, m.ctx->stream);
            if (res == ncclSuccess)
                res = g->R->all_gather(m.po.b[PO_CV].p, m.po.b[PO_ALLV].p, stride, ncclUint64, m.comm, m.ctx->stream);
            return res;
        }));
    for (int i = 0; i < nl; i++) {  // select, then replay what this partition loses
        Member& m = g->m[i];
        nrg_ctx* c = m.ctx;
        const nrg_pops& x = pops[i];
        const int r = m.rank;
        RCHK(nrg::ctx_use_device(c));
        // its part of the plan
        std::vector<uint64_t>& w = words[i];
        std::vector<uint64_t> ffirst, foff, bfirst, boff;
        uint64_t fn = 0, bn = 0;
        w.insert(w.end(), P.cf.begin(), P.cf.end());
        w.insert(w.end(), P.cb.begin(), P.cb.end());
        for (uint64_t q = P.rec0[r]; q < P.rec0[r + 1]; q++) {
            w.push_back(P.grant[q]);
            (all[q].back ? bfirst : ffirst).push_back(P.first[q]);
            (all[q].back ? boff : foff).push_back(P.off[q]);
            (all[q].back ? bn : fn) += P.grant[q];
        }
        w.insert(w.end(), ffirst.begin(), ffirst.end());
        w.insert(w.end(), foff.begin(), foff.end());
        w.insert(w.end(), bfirst.begin(), bfirst.end());
        w.insert(w.end(), boff.begin(), boff.end());
        const uint64_t plan_words = w.size();
        for (uint64_t v : {(uint64_t)0, g->sl_front, (uint64_t)0, g->sl_back}) w.push_back(v);  // the two records, counts zero
        GCHK(hipMemcpyAsync(m.po.b[PO_PLAN].p, w.data(), plan_words * 8, hipMemcpyHostToDevice, c->stream));
        GCHK(hipMemcpyAsync(m.po.b[PO_REC].p, w.data() + plan_words, 32, hipMemcpyHostToDevice, c->stream));
        PopSel s{};
        s.ck = (const uint64_t*)m.po.b[PO_ALLK].p, s.cv = (const uint64_t*)m.po.b[PO_ALLV].p;
        s.plan = (const uint64_t*)m.po.b[PO_PLAN].p;
        s.stride = stride, s.cfmax = P.cfmax, s.G = (uint32_t)G, s.me = (uint32_t)r, s.F = P.F, s.Bk = P.Bk;
        s.n = x.n, s.kf = ffirst.size(), s.kb = bfirst.size();
        s.fa = ffirst.empty() ? 0 : ffirst[0], s.fn = fn, s.ba = bfirst.empty() ? 0 : bfirst[0], s.bn = bn;
        s.resp = x.resp && x.some ? x.resp : nullptr, s.some = x.some;
        s.pk = x.pop_keys, s.pv = x.pop_vals, s.cap = x.pop_cap, s.pop_n = x.pop_n, s.total = P.total[r];
        s.rec = (uint64_t*)m.po.b[PO_REC].p;
        grp_pop_select_kernel<<<grp_grid((uint64_t)G * stride + x.n), GRP_TPB, 0, c->stream>>>(s);
        GCHK(hipGetLastError());
        const int rr = nrg_skiplist_round_async(c, (const nrg_put*)m.po.b[PO_REC].p, 2, (uint32_t)r + 1, nullptr, nullptr);
        if (rr) return group_fail(g, rr, "group-wide pop: a member could not replay its pops");
    }
    return NRG_OK;
}

// after step 1's words: the requests, the plan, steps 2 to 4 (or a one-rank group's own pop step), the final waits
int pop_run(nrg_group* g, const nrg_pops* pops, const std::vector<uint64_t>& ns, const std::vector<uint64_t>& lens,
            uint64_t nmax);

}  // namespace

extern "C" {

int nrg_group_skiplist_enable_removal(nrg_group* g, uint64_t tombstone) {
    std::vector<uint64_t> st;
    RCHK(optin_begin(g, st, [&](nrg_ctx* c) { return removal_status(g, c, tombstone); }));
    RCHK(exchange_pairs(g, std::vector<uint64_t>(st.size(), tombstone), st, "removal agreement"));
    RCHK(optin_agree(g->m[0].h_gwx, g->nranks));
    RCHK(optin_enable(g, [&](nrg_ctx* c) { return nrg_skiplist_enable_removal(c, tombstone); }));
    g->sl_rm = true;
    g->sl_tomb = tombstone;
    return NRG_OK;
}

int nrg_group_skiplist_enable_pops(nrg_group* g, uint64_t front_mark, uint64_t back_mark) {
    std::vector<uint64_t> st;
    RCHK(optin_begin(g, st, [&](nrg_ctx* c) { return pops_status(g, c, front_mark, back_mark); }));
    // two exchanges: {front mark, status}, {back mark, 0}; every rank reaches the same code after each
    RCHK(exchange_pairs(g, std::vector<uint64_t>(st.size(), front_mark), st, "pops agreement"));
    RCHK(optin_agree(g->m[0].h_gwx, g->nranks));
    RCHK(exchange_pairs(g, std::vector<uint64_t>(st.size(), back_mark), std::vector<uint64_t>(st.size(), 0), "pops agreement"));
    RCHK(optin_agree(g->m[0].h_gwx, g->nranks));
    RCHK(optin_enable(g, [&](nrg_ctx* c) { return nrg_skiplist_enable_pops(c, front_mark, back_mark); }));
    g->sl_pops = true;
    g->sl_front = front_mark;
    g->sl_back = back_mark;
    return NRG_OK;
}

int nrg_group_skiplist_pop(nrg_group* g, const nrg_pops* pops) {
    RCHK(pt_check(g));
    if (!pops) return NRG_E_INVAL;
    const int nl = (int)g->m.size(), G = g->nranks;
    // queued group work first; a latched device error of this rank is reported at the end, after it
    // has taken its part in the collectives (as nrg_group_verify)
    const int rc = nrg_group_sync(g);
    if (g->broken) return g->broken;
    // step 1: {n, flags, exact length}
    for (int i = 0; i < nl; i++) {
        Member& m = g->m[i];
        nrg_ctx* c = m.ctx;
        RCHK(nrg::ctx_use_device(c));
        int err = pop_args(g, c, pops[i]);
        uint64_t len = 0;  // from the device counts: the host's figures are upper bounds without removal
        if (err == NRG_OK) err = nrg_skiplist_len(c, &len);
        const uint64_t v[3] = {err ? 0 : pops[i].n, (uint64_t)(-err), len};
        RCHK(put_words(m.cstream, m.wx, v, 3));
    }
    RCHK(gather_words(g, 3, "group-wide pop: exchange"));
    const std::vector<uint64_t> H(g->m[0].h_gwx, g->m[0].h_gwx + 3 * (uint64_t)G);
    RCHK(gp_flags_agree(H.data(), G));
    std::vector<uint64_t> ns(G), lens(G);
    uint64_t nmax = 0;
    for (int r = 0; r < G; r++) {
        ns[r] = H[3 * r], lens[r] = H[3 * r + 2];
        nmax = std::max(nmax, ns[r]);
    }
    if (nmax == 0) return rc;
    // the staging of the requests: decided from the exchanged n, the same on every rank, before anything
    // is allocated (so one rank's huge n is an ordinary refusal everywhere and the group stays usable)
    if (!gp_reqs_fit(G, nmax)) return NRG_E_CAPACITY;
    try {
        const int r = pop_run(g, pops, ns, lens, nmax);
        if (r) return r;
    } catch (const std::bad_alloc&) {  // (its peers are inside the collectives: the group cannot go on)
        return group_fail(g, NRG_E_NOMEM, "group-wide pop: host allocation failed");
    }
    return rc;
}

}  // extern "C"

namespace {

int pop_run(nrg_group* g, const nrg_pops* pops, const std::vector<uint64_t>& ns, const std::vector<uint64_t>& lens,
            uint64_t nmax) {
    const int G = g->nranks;
    std::vector<std::vector<uint64_t>> words;
    // One rank owns every key: its own pop step answers (NRG_KNOB_EXP bit 16 keeps the general path
    // selectable for it, and a run longer than max_batch takes it too: a pop step is one round)
    if (pt_ident(g, g->m[0]) && pops[0].n <= g->m[0].ctx->cfg.max_batch) {
        RCHK(pop_own(g, g->m[0], pops[0]));
    } else {
        std::vector<nrg_pop_req> all;
        if (G == 1) {
            all.assign(pops[0].reqs, pops[0].reqs + pops[0].n);
        } else {
            RCHK(pop_requests(g, pops, ns, nmax, all));
        }
        GpPlan P;
        gp_plan(ns, all.data(), lens, P);
        if (!gp_fits(G, P)) return NRG_E_CAPACITY;  // (the same words on every rank: before any candidate moves)
        RCHK(pop_union(g, pops, P, all, words));
    }
    for (Member& m : g->m) {  // wait for every local member's stream under the group's deadline
        RCHK(nrg::ctx_use_device(m.ctx));
        RCHK(wait_stream(g, m.ctx->stream, "group-wide pop"));
    }
    return NRG_OK;
}

}  // namespace
