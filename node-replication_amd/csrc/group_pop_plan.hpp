// group_pop_plan.hpp — the plan of a group-wide pop (nrg_group_skiplist_pop, include/nrgpu.h;
// group_pops.cpp), as pure host arithmetic: no HIP header and no RCCL header, so
// tests/group_pop_plan.cpp checks it without a GPU.
//
// The ranks' requests, concatenated in rank order, are one run of consecutive pop records replayed
// against the union of the G partitions: skiplist_pop_plan.hpp's grants with len = the sum of the
// members' lengths. Every rank runs gp_plan on the same exchanged words and so reaches the same
// grants, ranks and offsets before any candidate moves:
//   grant[i]  entries record i of the run pops (its response)
//   first[i]  the grants to the earlier records of its own end: a front record pops the ascending ranks
//             [first, first + grant) of the union, a back record the same ranks counted from the top
//   off[i]    where its entries begin in its asker's packed output: the grants to the asker's earlier
//             records, whatever their end
//   F, Bk     the front and back totals; F + Bk <= len, so fronts and backs never meet
//   cf[o]     the front candidates member o contributes: its min(F, len_o) smallest entries. Whatever
//             the other partitions hold, no entry of o beyond those can be among the F smallest of the
//             union; cb[o] likewise from the top.
// A rank's records are contiguous in the run, so its front records are consecutive among all front
// records: their entries are the front ranks [first of its first front record, + its front grants).
#pragma once

#include <stdint.h>

#include <vector>

#include "../../include/nrgpu.h"
#include "skiplist_pop_plan.hpp"

namespace nrg {
namespace grp {

constexpr uint64_t GP_MAX_SLOTS = 1ull << 27;  // G * (cfmax + cbmax): a member's gathered candidates (include/nrgpu.h)

struct GpPlan {
    uint64_t len = 0, F = 0, Bk = 0;
    std::vector<uint64_t> rec0;                // [G + 1] rank r's records are [rec0[r], rec0[r + 1]) of the run
    std::vector<uint64_t> grant, first, off;   // per record of the run
    std::vector<uint64_t> total;               // [G] what rank r popped in all (its *pop_n)
    std::vector<uint64_t> cf, cb;              // [G] member o's front and back candidates
    uint64_t cfmax = 0, cbmax = 0;             // the longest of each
    // a member's candidate block: cfmax front slots, then cbmax back slots
    uint64_t stride() const { return cfmax + cbmax; }
};

// ns[r]: rank r's number of requests; reqs: all of them in rank order; lens[o]: member o's length
// (each at most 2^28, nrg_open's bound, and G <= NRG_MAX_PARTS: their sum does not wrap).
inline void gp_plan(const std::vector<uint64_t>& ns, const nrg_pop_req* reqs, const std::vector<uint64_t>& lens, GpPlan& P) {
    const size_t G = ns.size();
    P = GpPlan{};
    for (uint64_t l : lens) P.len += l;
    P.rec0.assign(G + 1, 0);
    for (size_t r = 0; r < G; r++) P.rec0[r + 1] = P.rec0[r] + ns[r];
    const uint64_t R = P.rec0[G], len = P.len;
    P.grant.assign(R, 0), P.first.assign(R, 0), P.off.assign(R, 0), P.total.assign(G, 0);
    uint64_t S = 0;  // the clipped counts before the record, saturating (a saturated sum stays >= len)
    for (size_t r = 0; r < G; r++) {
        uint64_t mine = 0;
        for (uint64_t i = P.rec0[r]; i < P.rec0[r + 1]; i++) {
            const uint64_t n = slp::clip(reqs[i].n, len), m = slp::grant(n, len, S);
            uint64_t& end = reqs[i].back ? P.Bk : P.F;
            P.grant[i] = m, P.first[i] = end, P.off[i] = mine;
            end += m, mine += m;
            S = slp::add(S, n);
        }
        P.total[r] = mine;
    }
    P.cf.assign(G, 0), P.cb.assign(G, 0);
    for (size_t o = 0; o < G; o++) {
        P.cf[o] = slp::clip(P.F, lens[o]), P.cb[o] = slp::clip(P.Bk, lens[o]);
        P.cfmax = P.cf[o] > P.cfmax ? P.cf[o] : P.cfmax;
        P.cbmax = P.cb[o] > P.cbmax ? P.cb[o] : P.cbmax;
    }
}

// the gathered candidates fit a member's scratch (stride <= 2^29 and G <= 64: the product cannot wrap)
inline bool gp_fits(int G, const GpPlan& P) { return (uint64_t)G * P.stride() <= GP_MAX_SLOTS; }

// The requests of every rank, padded to the longest n, are staged on the host and gathered on the device:
// G * nmax of them at most (256 MiB of requests), decided from the exchanged n before anything is allocated.
constexpr uint64_t GP_MAX_REQS = 1ull << 24;
inline bool gp_reqs_fit(int G, uint64_t nmax) { return nmax <= GP_MAX_REQS / (uint64_t)G; }

// ---- the select step's arithmetic (group_pops.cpp grp_pop_select_kernel runs it on the device) ----------
// Every member's candidates lie gathered as [G][stride] keys: member q's cf[q] front candidates ascending
// at q * stride, its cb[q] back candidates descending at q * stride + cfmax.

// the first index of the ascending a[0, n) whose key is not below k
NRG_SLP_HD inline uint64_t gp_lower_asc(const uint64_t* a, uint64_t n, uint64_t k) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the number of keys above k in the descending a[0, n)
NRG_SLP_HD inline uint64_t gp_above_desc(const uint64_t* a, uint64_t n, uint64_t k) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] > k) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the last index of the ascending a[0, n), n >= 1, whose value is at most x (a[0] <= x)
NRG_SLP_HD inline uint64_t gp_last_le(const uint64_t* a, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// The rank of candidate x (key `key`) of list o at its end of the union: its index in its own list plus,
// for every other list, the candidates below (back: above) its key. cnt: cf (back: cb). Partitions hold
// disjoint key sets and a list holds min(total, len_o) candidates, so a rank below the end's total is
// exact, and a candidate whose true rank is at or above the total is never ranked below it.
NRG_SLP_HD inline uint64_t gp_cand_rank(const uint64_t* ck, uint64_t stride, uint64_t cfmax, const uint64_t* cnt, uint32_t G,
                                        bool back, uint32_t o, uint64_t x, uint64_t key) {
    uint64_t r = x;
    for (uint32_t q = 0; q < G; q++) {
        if (q == o) continue;
        const uint64_t* a = ck + (uint64_t)q * stride + (back ? cfmax : 0);
        r += back ? gp_above_desc(a, cnt[q], key) : gp_lower_asc(a, cnt[q], key);
    }
    return r;
}

// Where the entry of rank r goes in its asker's packed output: first[] and off[] are the first ranks and
// offsets of the asker's k records of that end, in issue order (first[0] <= r < first[0] + their grants).
NRG_SLP_HD inline uint64_t gp_place(const uint64_t* first, const uint64_t* off, uint64_t k, uint64_t r) {
    const uint64_t i = gp_last_le(first, k, r);
    return off[i] + (r - first[i]);
}

// A rank's flags word of the {n, flags, length} exchange: -NRG_E_* of its local check (bad arguments,
// its kind, ltail < tail, a group that has not agreed on pops), or 0.
inline int gp_flags_agree(const uint64_t* H, int G) {
    for (int r = 0; r < G; r++)
        if (H[3 * r + 1]) return -(int)H[3 * r + 1];
    return NRG_OK;
}

}  // namespace grp
}  // namespace nrg
