// group_reads.cpp — group-wide ordered reads of a partitioned skip-list group (include/nrgpu.h,
// nrg_group_skiplist_seek / _range_count / _scan).
//
// Under hash partitioning no member alone can answer lower_bound or a range count: every member
// answers every query against its own partition and the asker reduces the G candidates.
//   1. {n, flags} of every rank (exchange_pairs): the flags carry a rank's bad arguments, its kind,
//      the seek mode and a scan's limit (group_plan.hpp sk_flags), so that every rank returns the
//      same code before any data moves (a scan also bounds G * nmax * limit, which every rank
//      derives from the same lengths);
//   2. the queries, padded to the longest n, all-gathered (a range count's los and his travel as one
//      block: the los of every slot, then the his);
//   3. the skip-list read kernels over all G * nmax of them (skiplist.hip);
//   4. each asker's candidates back with send / recv in one group (a rank's own: a device copy; a
//      scan's block is lens * limit keys, as many values and lens counts);
//   5. one reduction launch into the caller's buffers.
// Everything after step 1 runs on the replica's stream, which the call then waits for. A one-rank
// group (pt_ident) stops after step 1 and runs step 3 straight into the caller's buffers.
#include <algorithm>

#include "group.hpp"

using namespace nrg::grp;

void SkMember::free() {
    for (DBuf& d : b) free_buf(d);
}

namespace {

// nrg_group_skiplist_seek's reduction: query i has one candidate per partition, ck / cv / cf[o * n + i]
// (found = 0: that partition has none). Partitions hold disjoint key sets, so among the found ones
// the smallest key (GE, GT) or the largest (LE, LT) is the answer of the whole map; no key value
// stands for "none".
__global__ __launch_bounds__(GRP_TPB) void grp_seek_reduce_kernel(const uint64_t* __restrict__ ck,
                                                                  const uint64_t* __restrict__ cv,
                                                                  const uint8_t* __restrict__ cf, uint32_t G, uint64_t n,
                                                                  uint32_t mode, uint64_t* __restrict__ okeys,
                                                                  uint64_t* __restrict__ ovals, uint8_t* __restrict__ found) {
    const bool up = mode == NRG_SEEK_GE || mode == NRG_SEEK_GT;
    for (uint64_t i = blockIdx.x * (uint64_t)GRP_TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * GRP_TPB) {
        uint64_t bk = 0, bv = 0;
        bool any = false;
        for (uint32_t o = 0; o < G; o++) {
            const uint64_t at = (uint64_t)o * n + i;
            if (!cf[at]) continue;
            const uint64_t k = ck[at];
            if (!any || (up ? k < bk : k > bk)) bk = k, bv = cv[at];
            any = true;
        }
        okeys[i] = bk;
        ovals[i] = bv;
        found[i] = any ? 1 : 0;
    }
}

// nrg_group_skiplist_range_count's: the sum of the partitions' counts (at most 2^64 keys exist, and
// 2^64 only for [0, 2^64 - 1] on a full key space, which no capacity allows: the sum cannot wrap)
__global__ __launch_bounds__(GRP_TPB) void grp_count_reduce_kernel(const uint64_t* __restrict__ cc, uint32_t G,
                                                                   uint64_t n, uint64_t* __restrict__ counts) {
    for (uint64_t i = blockIdx.x * (uint64_t)GRP_TPB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * GRP_TPB) {
        uint64_t c = 0;
        for (uint32_t o = 0; o < G; o++) c += cc[(uint64_t)o * n + i];
        counts[i] = c;
    }
}

// nrg_group_skiplist_scan's reduction: query i has one sorted candidate list per partition,
// ck / cv[(o * n + i) * limit + t] for t < cc[o * n + i], ascending (GE, GT) or descending (LE, LT).
// Partitions hold disjoint key sets, so keys never tie and a candidate's place in the merge of the G
// lists is t plus, for every other list, the number of its candidates that precede the key (smaller
// when ascending, greater when descending): a binary search per list. The places below `limit` are
// stored; the places are a permutation, so no slot is written twice and none at or past the count.
// A group of 2^lw lanes per query strides over the G * limit candidate slots.
__global__ __launch_bounds__(GRP_TPB) void grp_scan_reduce_kernel(const uint64_t* __restrict__ ck,
                                                                  const uint64_t* __restrict__ cv,
                                                                  const uint32_t* __restrict__ cc, uint32_t G, uint64_t n,
                                                                  uint32_t mode, uint32_t limit, uint32_t lw,
                                                                  uint64_t* __restrict__ okeys,
                                                                  uint64_t* __restrict__ ovals, uint32_t* __restrict__ counts) {
    const uint64_t gt = blockIdx.x * (uint64_t)GRP_TPB + threadIdx.x;
    const uint64_t i = gt >> lw;
    if (i >= n) return;
    const uint32_t W = 1u << lw, lane = (uint32_t)gt & (W - 1);
    const bool up = mode == NRG_SEEK_GE || mode == NRG_SEEK_GT;
    for (uint32_t s = lane; s < G * limit; s += W) {
        const uint32_t o = s / limit, t = s - o * limit;
        if (t >= cc[(uint64_t)o * n + i]) continue;
        const uint64_t at = ((uint64_t)o * n + i) * limit + t;
        const uint64_t k = ck[at];
        uint32_t place = t;
        for (uint32_t p = 0; p < G && place < limit; p++) {
            if (p == o) continue;
            const uint64_t* l = ck + ((uint64_t)p * n + i) * limit;
            uint32_t lo = 0, hi = cc[(uint64_t)p * n + i];
            while (lo < hi) {  // the candidates of list p that precede k
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (up ? l[mid] < k : l[mid] > k) lo = mid + 1; else hi = mid;
            }
            place += lo;
        }
        if (place < limit) {
            okeys[i * limit + place] = k;
            ovals[i * limit + place] = cv[at];
        }
    }
    if (lane == 0) {
        uint64_t c = 0;
        for (uint32_t o = 0; o < G; o++) c += cc[(uint64_t)o * n + i];
        counts[i] = c < limit ? (uint32_t)c : limit;
    }
}

struct SkQuery {
    const uint64_t *a, *b;  // keys, or los and his
    uint64_t n;
    bool bad;
};

// What kind of read a call is: the words, candidates and flag bytes it moves per query.
struct SkShape {
    bool count, scan;
    uint32_t mode, limit;
    uint64_t words() const { return count ? 2 : 1; }  // u64 words per query
    // per query and partition: per() candidate keys and values, and one flag of fb() bytes (a seek's
    // found byte, a scan's u32 count)
    uint64_t per() const { return scan ? limit : 1; }
    uint64_t fb() const { return scan ? 4 : 1; }
};

// Step 1: every rank's n and flags; the code every rank returns, the lengths and the longest.
int sk_agree(nrg_group* g, const std::vector<SkQuery>& q, const SkShape& sh, uint64_t* nmax_out, std::vector<uint64_t>& lens) {
    const int nl = (int)g->m.size(), G = g->nranks;
    std::vector<uint64_t> a(nl), b(nl);
    for (int i = 0; i < nl; i++) {
        const nrg_ctx* c = g->m[i].ctx;
        const bool bad = q[i].bad || c->cfg.ds_kind != NRG_DS_SKIPLIST || c->ltail != c->tail ||
                         (!sh.count && sh.mode > NRG_SEEK_LT) || q[i].n >= (1ull << 32) ||
                         (sh.scan && (sh.limit == 0 || sh.limit > NRG_SCAN_MAX_LIMIT));
        a[i] = q[i].n;
        b[i] = sk_flags(bad, sh.count, sh.mode, sh.scan, sh.limit, c->cfg.ds_kind);
    }
    RCHK(exchange_pairs(g, a, b, "length exchange"));
    const uint64_t* H = g->m[0].h_gwx;
    RCHK(sk_flags_agree(H, G));
    uint64_t nmax = 0;
    for (int r = 0; r < G; r++) {
        lens[r] = H[2 * r];
        nmax = std::max(nmax, lens[r]);
    }
    *nmax_out = nmax;
    // a scan's candidate scratch: the bound follows from the exchanged lengths, the same on every rank
    if (sh.scan && !sk_scan_fits(G, nmax, sh.limit)) return NRG_E_CAPACITY;
    return NRG_OK;
}

// Step 2's buffers and the padded send copy of every local member's queries
int sk_stage(nrg_group* g, const std::vector<SkQuery>& q, const SkShape& sh, uint64_t nmax) {
    const int nl = (int)g->m.size();
    const uint64_t G = (uint64_t)g->nranks, words = sh.words(), per = sh.per(), fb = sh.fb();
    for (int i = 0; i < nl; i++) {
        Member& m = g->m[i];
        DBuf* sk = m.sk.b;
        nrg_ctx* c = m.ctx;
        RCHK(nrg::ctx_use_device(c));
        const uint64_t cand = G * nmax * per * 8, back = G * q[i].n * per * 8;  // (a count moves keys only)
        const uint64_t v = sh.count ? 0 : 1;
        const uint64_t need[SK_N] = {words * nmax * 8, G * words * nmax * 8,           // SEND, QALL
                                     cand,             v * cand, v * G * nmax * fb,    // CK, CV, CF
                                     back,             v * back, v * G * q[i].n * fb};  // BK, BV, BF
        int r = NRG_OK;
        for (int k = 0; k < SK_N && r == NRG_OK; k++) r = grow_buf(m, sk[k], need[k]);
        // (its peers are already inside the collectives below: the group cannot go on)
        if (r) return group_fail(g, r, "group-wide skip-list read: scratch allocation failed");
        hipStream_t s = c->stream;
        if (m.in_set && m.in_stream != s) RCHK(order(m, m.in_stream, s));
        // the padded send copy (padding queries are zeros: answered, never returned)
        char* send = (char*)sk[SK_SEND].p;
        GCHK(hipMemsetAsync(send, 0, words * nmax * 8, s));
        if (q[i].n) {
            GCHK(hipMemcpyAsync(send, q[i].a, q[i].n * 8, hipMemcpyDeviceToDevice, s));
            if (sh.count) GCHK(hipMemcpyAsync(send + nmax * 8, q[i].b, q[i].n * 8, hipMemcpyDeviceToDevice, s));
        }
    }
    return NRG_OK;
}

// Step 3: every member answers every rank's block against its own partition
int sk_answer(nrg_group* g, const SkShape& sh, uint64_t nmax, const std::vector<uint64_t>& lens) {
    const uint64_t words = sh.words(), per = sh.per(), fb = sh.fb();
    for (Member& m : g->m) {
        nrg_ctx* c = m.ctx;
        RCHK(nrg::ctx_use_device(c));
        const uint64_t* qall = (const uint64_t*)m.sk.b[SK_QALL].p;
        for (int s = 0; s < g->nranks; s++) {
            if (!lens[s]) continue;
            const uint64_t* blk = qall + (uint64_t)s * words * nmax;
            uint64_t* ck = (uint64_t*)m.sk.b[SK_CK].p + (uint64_t)s * nmax * per;
            uint64_t* cv = (uint64_t*)m.sk.b[SK_CV].p + (uint64_t)s * nmax * per;
            void* cf = at(m.sk.b[SK_CF].p, (uint64_t)s * nmax * fb);
            const hipError_t he = sh.count  ? nrg::sl_count_launch(c, blk, blk + nmax, lens[s], ck)
                                  : sh.scan ? nrg::sl_walk_launch(c, blk, lens[s], sh.mode, sh.limit, ck, cv, (uint32_t*)cf)
                                            : nrg::sl_seek_launch(c, blk, lens[s], sh.mode, ck, cv, (uint8_t*)cf);
            if (he != hipSuccess) return hip_rc(he);
        }
    }
    return NRG_OK;
}

// Step 4: the candidates back to their askers: rank r's block for asker s lands at s's slot r
int sk_back(nrg_group* g, const std::vector<SkQuery>& q, const SkShape& sh, uint64_t nmax, const std::vector<uint64_t>& lens) {
    const Rccl* R = g->R;
    const int nl = (int)g->m.size(), G = g->nranks;
    const bool count = sh.count;
    const uint64_t per = sh.per(), fb = sh.fb();
    const ncclDataType_t ft = sh.scan ? ncclUint32 : ncclUint8;
    if (G > 1)
        RCHK(collective(g, "group-wide skip-list read: candidates back", [&](Member& m, int i) {
            const uint64_t n = q[i].n;
            DBuf* sk = m.sk.b;
            hipStream_t s = m.ctx->stream;
            ncclResult_t res = ncclSuccess;
            for (int o = 0; o < G && res == ncclSuccess; o++) {
                if (o == m.rank) continue;
                if (lens[o]) {
                    res = R->send(at(sk[SK_CK].p, o * nmax * per * 8), lens[o] * per, ncclUint64, o, m.comm, s);
                    if (res == ncclSuccess && !count)
                        res = R->send(at(sk[SK_CV].p, o * nmax * per * 8), lens[o] * per, ncclUint64, o, m.comm, s);
                    if (res == ncclSuccess && !count) res = R->send(at(sk[SK_CF].p, o * nmax * fb), lens[o], ft, o, m.comm, s);
                }
                if (res == ncclSuccess && n) {
                    res = R->recv(at(sk[SK_BK].p, o * n * per * 8), n * per, ncclUint64, o, m.comm, s);
                    if (res == ncclSuccess && !count)
                        res = R->recv(at(sk[SK_BV].p, o * n * per * 8), n * per, ncclUint64, o, m.comm, s);
                    if (res == ncclSuccess && !count) res = R->recv(at(sk[SK_BF].p, o * n * fb), n, ft, o, m.comm, s);
                }
            }
            return res;
        }));
    for (int i = 0; i < nl; i++) {  // a rank's own candidates: a device copy
        Member& m = g->m[i];
        DBuf* sk = m.sk.b;
        const uint64_t n = q[i].n, r = (uint64_t)m.rank;
        if (!n) continue;
        RCHK(nrg::ctx_use_device(m.ctx));
        hipStream_t s = m.ctx->stream;
        const uint64_t kb = n * per * 8;  // the block's keys (and values) in bytes
        GCHK(hipMemcpyAsync(at(sk[SK_BK].p, r * kb), at(sk[SK_CK].p, r * nmax * per * 8), kb, hipMemcpyDeviceToDevice, s));
        if (count) continue;
        GCHK(hipMemcpyAsync(at(sk[SK_BV].p, r * kb), at(sk[SK_CV].p, r * nmax * per * 8), kb, hipMemcpyDeviceToDevice, s));
        GCHK(hipMemcpyAsync(at(sk[SK_BF].p, r * n * fb), at(sk[SK_CF].p, r * nmax * fb), n * fb, hipMemcpyDeviceToDevice, s));
    }
    return NRG_OK;
}

// Steps 1 to 4. *nmax_out == 0: nothing to answer; *ident: the caller runs the read kernel itself.
int sk_collect(nrg_group* g, const std::vector<SkQuery>& q, const SkShape& sh, uint64_t* nmax_out,
               std::vector<uint64_t>& lens, bool* ident) {
    RCHK(sk_agree(g, q, sh, nmax_out, lens));
    const uint64_t nmax = *nmax_out;
    if (nmax == 0) return NRG_OK;
    // One rank owns every key: its only candidate is the answer, so the read kernel answers straight
    // into the caller's buffers and nothing moves (as a one-rank group's rounds; NRG_KNOB_EXP bit 16
    // keeps the general path selectable for it).
    *ident = pt_ident(g, g->m[0]);
    if (*ident) {
        Member& m = g->m[0];
        if (m.in_set && m.in_stream != m.ctx->stream) RCHK(order(m, m.in_stream, m.ctx->stream));
        return NRG_OK;
    }
    RCHK(sk_stage(g, q, sh, nmax));
    RCHK(collective(g, "group-wide skip-list read: queries", [&](Member& m, int) {
        return g->R->all_gather(m.sk.b[SK_SEND].p, m.sk.b[SK_QALL].p, sh.words() * nmax, ncclUint64, m.comm, m.ctx->stream);
    }));
    RCHK(sk_answer(g, sh, nmax, lens));
    return sk_back(g, q, sh, nmax, lens);
}

// The three calls' common course. query(x): a member's SkQuery; own(ctx, x): the read kernel
// straight into the caller's buffers (one rank); reduce(member, x): step 5's launch.
template <typename Arg, typename Query, typename Own, typename Reduce>
int sk_read(nrg_group* g, const Arg* args, const SkShape& sh, Query query, Own own, Reduce reduce) {
    RCHK(pt_check(g));
    if (!args) return NRG_E_INVAL;
    const int nl = (int)g->m.size();
    // queued group work first; a latched device error of this rank is reported at the end, after it
    // has taken its part in the collectives (as nrg_group_verify)
    const int rc = nrg_group_sync(g);
    if (g->broken) return g->broken;
    std::vector<SkQuery> q(nl);
    for (int i = 0; i < nl; i++) q[i] = query(args[i]);
    std::vector<uint64_t> lens(g->nranks);
    uint64_t nmax = 0;
    bool ident = false;
    RCHK(sk_collect(g, q, sh, &nmax, lens, &ident));
    if (nmax == 0) return rc;
    if (ident) {
        const hipError_t he = own(g->m[0].ctx, args[0]);
        if (he != hipSuccess) return hip_rc(he);
    } else {
        for (int i = 0; i < nl; i++) {
            if (!args[i].n) continue;
            RCHK(nrg::ctx_use_device(g->m[i].ctx));
            reduce(g->m[i], args[i]);
            GCHK(hipGetLastError());
        }
    }
    for (Member& m : g->m) {  // wait for every local member's stream under the group's deadline
        RCHK(nrg::ctx_use_device(m.ctx));
        RCHK(wait_stream(g, m.ctx->stream, "group-wide skip-list read"));
    }
    return rc;
}

}  // namespace

extern "C" {

int nrg_group_skiplist_seek(nrg_group* g, const nrg_seek* seeks, uint32_t mode) {
    return sk_read(
        g, seeks, SkShape{false, false, mode, 0},
        [](const nrg_seek& x) { return SkQuery{x.keys, nullptr, x.n, x.n && (!x.keys || !x.out_keys || !x.out_vals || !x.found)}; },
        [&](nrg_ctx* c, const nrg_seek& x) { return nrg::sl_seek_launch(c, x.keys, x.n, mode, x.out_keys, x.out_vals, x.found); },
        [&](Member& m, const nrg_seek& x) {
            grp_seek_reduce_kernel<<<grp_grid(x.n), GRP_TPB, 0, m.ctx->stream>>>(
                (const uint64_t*)m.sk.b[SK_BK].p, (const uint64_t*)m.sk.b[SK_BV].p, (const uint8_t*)m.sk.b[SK_BF].p,
                (uint32_t)g->nranks, x.n, mode, x.out_keys, x.out_vals, x.found);
        });
}

int nrg_group_skiplist_range_count(nrg_group* g, const nrg_count* counts) {
    return sk_read(
        g, counts, SkShape{true, false, 0, 0},
        [](const nrg_count& x) { return SkQuery{x.los, x.his, x.n, x.n && (!x.los || !x.his || !x.counts)}; },
        [](nrg_ctx* c, const nrg_count& x) { return nrg::sl_count_launch(c, x.los, x.his, x.n, x.counts); },
        [&](Member& m, const nrg_count& x) {
            grp_count_reduce_kernel<<<grp_grid(x.n), GRP_TPB, 0, m.ctx->stream>>>((const uint64_t*)m.sk.b[SK_BK].p,
                                                                                  (uint32_t)g->nranks, x.n, x.counts);
        });
}

int nrg_group_skiplist_scan(nrg_group* g, const nrg_scan* scans, uint32_t mode, uint32_t limit) {
    return sk_read(
        g, scans, SkShape{false, true, mode, limit},
        [](const nrg_scan& x) { return SkQuery{x.keys, nullptr, x.n, x.n && (!x.keys || !x.out_keys || !x.out_vals || !x.counts)}; },
        [&](nrg_ctx* c, const nrg_scan& x) { return nrg::sl_walk_launch(c, x.keys, x.n, mode, limit, x.out_keys, x.out_vals, x.counts); },
        [&](Member& m, const nrg_scan& x) {
            // the lane group of a query, up to a wave
            const uint32_t lw = scan_lane_log2(g->nranks, limit);
            const uint64_t per_wg = (uint64_t)GRP_TPB >> lw;
            grp_scan_reduce_kernel<<<(unsigned)((x.n + per_wg - 1) / per_wg), GRP_TPB, 0, m.ctx->stream>>>(
                (const uint64_t*)m.sk.b[SK_BK].p, (const uint64_t*)m.sk.b[SK_BV].p, (const uint32_t*)m.sk.b[SK_BF].p,
                (uint32_t)g->nranks, x.n, mode, limit, lw, x.out_keys, x.out_vals, x.counts);
        });
}

}  // extern "C"
