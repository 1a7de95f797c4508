// group_pop_plan.cpp — the host plan of a group-wide pop (node-replication_amd/csrc/group_pop_plan.hpp)
// against the sequential loop it restates: the ranks' requests, concatenated in rank order, replayed one
// record at a time with pop_front() / pop_back() on a deque that holds the union of the partitions (its
// entries are their own ascending ranks). Checked per record: the grant, the first rank and the offset
// in the asker's packed output; per call: F, Bk, every rank's total, the candidate block lengths and the
// 2^27 capacity decision; then the select step's rank and place arithmetic (what the device runs per
// candidate) against sorting the union. Random and edge inputs: counts of 0, 1 and 2^64 - 1, sums that would wrap,
// len = 0, runs whose fronts and backs exhaust the map exactly and by one, G from 1 to NRG_MAX_PARTS.
// A stand-alone host program (tests/test_group_pop_plan.py builds it under AddressSanitizer and
// UndefinedBehaviorSanitizer).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <vector>

#include "../node-replication_amd/csrc/group_pop_plan.hpp"

using namespace nrg;
using namespace nrg::grp;
using u64 = uint64_t;

static long g_records = 0, g_runs = 0;

#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            std::exit(1);                                            \
        }                                                            \
    } while (0)

static u64 g_seed = 0x9E3779B97F4A7C15ull;
static u64 rnd() {  // splitmix64
    u64 z = (g_seed += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// reqs[r]: rank r's requests; lens[o]: member o's length. The deque replay needs a map it can hold.
static void check_run(const std::vector<std::vector<nrg_pop_req>>& reqs, const std::vector<u64>& lens) {
    const size_t G = reqs.size();
    std::vector<u64> ns(G);
    std::vector<nrg_pop_req> all;
    for (size_t r = 0; r < G; r++) {
        ns[r] = reqs[r].size();
        all.insert(all.end(), reqs[r].begin(), reqs[r].end());
    }
    GpPlan P;
    gp_plan(ns, all.data(), lens, P);
    u64 len = 0;
    for (u64 l : lens) len += l;
    CHECK(P.len == len && P.rec0.size() == G + 1 && P.rec0[G] == all.size() && P.grant.size() == all.size());
    const bool model = len <= 4096;
    std::deque<u64> q;
    if (model)
        for (u64 i = 0; i < len; i++) q.push_back(i);
    u64 F = 0, B = 0;
    for (size_t r = 0; r < G; r++) {
        CHECK(P.rec0[r + 1] - P.rec0[r] == ns[r]);
        u64 mine = 0;
        for (u64 i = P.rec0[r]; i < P.rec0[r + 1]; i++) {
            const bool back = all[i].back != 0;
            CHECK(P.first[i] == (back ? B : F) && P.off[i] == mine);
            CHECK(P.grant[i] <= all[i].n && F + B + P.grant[i] <= len);
            if (model) {  // the sequential loop: n times, while the map has an entry
                u64 got = 0;
                for (u64 k = 0; k < all[i].n && !q.empty(); k++, got++) {
                    const u64 e = back ? q.back() : q.front();
                    if (back) q.pop_back(); else q.pop_front();
                    CHECK(got < P.grant[i] && slp::rank_of(back, len, P.first[i], got) == e);
                }
                CHECK(got == P.grant[i]);
            } else {  // what is left, or the count
                CHECK(P.grant[i] == (all[i].n < len - (F + B) ? all[i].n : len - (F + B)));
            }
            (back ? B : F) += P.grant[i];
            mine += P.grant[i];
            g_records++;
        }
        CHECK(P.total[r] == mine);
    }
    CHECK(P.F == F && P.Bk == B && F + B <= len);
    if (model) CHECK(q.size() == len - (F + B));
    u64 cfmax = 0, cbmax = 0;
    for (size_t o = 0; o < G; o++) {
        CHECK(P.cf[o] == (F < lens[o] ? F : lens[o]) && P.cb[o] == (B < lens[o] ? B : lens[o]));
        cfmax = P.cf[o] > cfmax ? P.cf[o] : cfmax;
        cbmax = P.cb[o] > cbmax ? P.cb[o] : cbmax;
    }
    CHECK(P.cfmax == cfmax && P.cbmax == cbmax && P.stride() == cfmax + cbmax);
    CHECK(gp_fits((int)G, P) == ((u64)G * (cfmax + cbmax) <= (1ull << 27)));
    g_runs++;
}

static std::vector<u64> spread(u64 len, size_t G, bool skew) {  // len entries over G members
    std::vector<u64> lens(G, 0);
    if (skew) {
        lens[rnd() % G] = len;
        return lens;
    }
    for (size_t o = 0; o < G; o++) lens[o] = len / G + (o < len % G ? 1 : 0);
    return lens;
}

int main() {
    const u64 big[] = {~0ull, 1ull << 63, ~0ull - 1, (1ull << 63) + 1, 1ull << 32};
    // random runs: every G, ragged request counts (empty ranks among them), counts around what is left
    for (int G = 1; G <= NRG_MAX_PARTS; G++)
        for (int rep = 0; rep < 12; rep++) {
            const u64 len = rep == 0 ? 0 : rnd() % (rep < 6 ? 40 : 3000);
            std::vector<std::vector<nrg_pop_req>> reqs(G);
            for (int r = 0; r < G; r++) {
                const u64 n = rnd() % 4 == 0 ? 0 : rnd() % 6;
                for (u64 j = 0; j < n; j++) {
                    const u64 pick = rnd() % 10;
                    const u64 c = pick == 0 ? 0 : pick == 1 ? 1 : pick == 2 ? big[rnd() % 5] : rnd() % (2 * len / (u64)G + 3);
                    reqs[r].push_back(nrg_pop_req{c, (uint32_t)(rnd() & 1), 0});
                }
            }
            check_run(reqs, spread(len, G, rep & 1));
        }
    // fronts and backs that exhaust the map exactly, and by one (the last record is short), then None
    for (int G : {1, 2, 3, 8, NRG_MAX_PARTS})
        for (u64 len : {1ull, 7ull, 350ull, 4096ull})
            for (u64 extra : {0ull, 1ull}) {
                std::vector<std::vector<nrg_pop_req>> reqs(G);
                const u64 f = len / 3, b = len - f + extra;
                reqs[0].push_back(nrg_pop_req{f, 0, 0});
                reqs[G - 1].push_back(nrg_pop_req{b, 1, 0});
                reqs[G / 2].push_back(nrg_pop_req{1, 0, 0});   // (G = 1: after both; else between them)
                reqs[G - 1].push_back(nrg_pop_req{1, 1, 0});
                check_run(reqs, spread(len, G, false));
                check_run(reqs, spread(len, G, true));
            }
    // counts of 2^64 - 1 and sums that would wrap, on maps the deque cannot hold too
    for (int G : {1, 3, NRG_MAX_PARTS})
        for (u64 len : {0ull, 1ull, 5ull, 350ull, 1ull << 28, 64ull << 28})
            for (u64 a : big)
                for (u64 b : big)
                    for (unsigned ends = 0; ends < 16; ends++) {
                        std::vector<std::vector<nrg_pop_req>> reqs(G);
                        const u64 c[4] = {3, a, b, 1};
                        for (int i = 0; i < 4; i++) reqs[(i * G) / 4].push_back(nrg_pop_req{c[i], (ends >> i) & 1u, 0});
                        check_run(reqs, spread(len, G, false));
                    }
    // the capacity decision at the bound and one past it: G * (cfmax + cbmax) <= 2^27
    {
        const int G = 8;
        const u64 per = (1ull << 27) / G;  // slots per member at the bound
        for (u64 over : {0ull, 1ull}) {
            std::vector<std::vector<nrg_pop_req>> reqs(G);
            reqs[0].push_back(nrg_pop_req{per / 2, 0, 0});
            reqs[1].push_back(nrg_pop_req{per / 2 + over, 1, 0});
            std::vector<u64> lens(G, 1ull << 25);  // every member holds more than either total
            std::vector<u64> ns(G);
            std::vector<nrg_pop_req> all;
            for (int r = 0; r < G; r++) {
                ns[r] = reqs[r].size();
                all.insert(all.end(), reqs[r].begin(), reqs[r].end());
            }
            GpPlan P;
            gp_plan(ns, all.data(), lens, P);
            CHECK(P.cfmax == per / 2 && P.cbmax == per / 2 + over && gp_fits(G, P) == (over == 0));
            check_run(reqs, lens);
        }
        // one rank: the block may take the whole bound
        GpPlan P;
        const nrg_pop_req one[2] = {{1ull << 26, 0, 0}, {(1ull << 26) + 1, 1, 0}};
        gp_plan({1}, one, {1ull << 28}, P);
        CHECK(P.stride() == (1ull << 26) && gp_fits(1, P));
        gp_plan({2}, one, {1ull << 28}, P);
        CHECK(P.stride() == (1ull << 27) + 1 && !gp_fits(1, P));
    }
    // the request staging bound: G * nmax <= 2^24, at the bound and one past it
    CHECK(gp_reqs_fit(1, 1ull << 24) && !gp_reqs_fit(1, (1ull << 24) + 1) && gp_reqs_fit(8, 1ull << 21) &&
          !gp_reqs_fit(8, (1ull << 21) + 1) && gp_reqs_fit(NRG_MAX_PARTS, 1ull << 18) && !gp_reqs_fit(3, 1ull << 32));
    // the select step (gp_cand_rank, gp_place: what grp_pop_select_kernel runs per candidate) on random
    // partitions of random key sets: the candidates ranked below an end's total are exactly that end of the
    // sorted union, each at its rank; a member's popped candidates are a prefix of its list; and every popped
    // entry lands in its asker's packed output where the one-record-at-a-time replay puts it
    for (int rep = 0; rep < 400; rep++) {
        const int G = 1 + (int)(rnd() % (rep < 300 ? 9 : NRG_MAX_PARTS));
        const u64 len = rnd() % 300;
        std::vector<u64> un;  // the union, ascending and distinct (0 and 2^64 - 1 among the keys now and then)
        u64 k = rnd() % 3 == 0 ? 0 : rnd() % 1000;
        for (u64 i = 0; i < len; i++, k += 1 + rnd() % 1000) un.push_back(i + 1 == len && rnd() % 3 == 0 ? ~0ull : k);
        std::vector<std::vector<u64>> part(G);
        const bool skew = rnd() % 4 == 0;
        for (u64 key : un) part[skew ? (rnd() % 8 ? 0 : rnd() % G) : rnd() % G].push_back(key);
        std::vector<std::vector<nrg_pop_req>> reqs(G);
        for (int r = 0; r < G; r++)
            for (u64 j = rnd() % 4; j > 0; j--) reqs[r].push_back(nrg_pop_req{rnd() % 5 == 0 ? ~0ull : rnd() % (len / 2 + 2), (uint32_t)(rnd() & 1), 0});
        std::vector<u64> ns(G), lens(G);
        std::vector<nrg_pop_req> all;
        for (int r = 0; r < G; r++) {
            ns[r] = reqs[r].size(), lens[r] = part[r].size();
            all.insert(all.end(), reqs[r].begin(), reqs[r].end());
        }
        GpPlan P;
        gp_plan(ns, all.data(), lens, P);
        const u64 stride = P.stride();
        std::vector<u64> ck((size_t)G * stride + 1, 0xDEADull);  // the gathered blocks, padding never read as a key
        for (int o = 0; o < G; o++) {
            for (u64 x = 0; x < P.cf[o]; x++) ck[o * stride + x] = part[o][x];
            for (u64 x = 0; x < P.cb[o]; x++) ck[o * stride + P.cfmax + x] = part[o][part[o].size() - 1 - x];
        }
        // the expected packed outputs: the replay, one record at a time, on a deque of the union
        std::deque<u64> q(un.begin(), un.end());
        std::vector<std::vector<u64>> want(G);
        for (int r = 0; r < G; r++)
            for (const nrg_pop_req& x : reqs[r])
                for (u64 c = 0; c < x.n && !q.empty(); c++) {
                    want[r].push_back(x.back ? q.back() : q.front());
                    if (x.back) q.pop_back(); else q.pop_front();
                }
        std::vector<std::vector<u64>> got(G);
        for (int r = 0; r < G; r++) got[r].assign(P.total[r], 0xBADull);
        for (int end = 0; end < 2; end++) {
            const bool back = end == 1;
            const u64 total = back ? P.Bk : P.F;
            const std::vector<u64>& cnt = back ? P.cb : P.cf;
            std::vector<char> seen(total, 0);
            for (int o = 0; o < G; o++) {
                u64 popped = 0;
                for (u64 x = 0; x < cnt[o]; x++) {
                    const u64 key = ck[o * stride + (back ? P.cfmax : 0) + x];
                    const u64 r = gp_cand_rank(ck.data(), stride, P.cfmax, cnt.data(), (uint32_t)G, back, (uint32_t)o, x, key);
                    if (r >= total) continue;
                    CHECK(popped == x && !seen[r] && key == (back ? un[len - 1 - r] : un[r]));  // a prefix; the rank is exact
                    seen[r] = 1, popped++;
                    for (int a = 0; a < G; a++) {  // the asker whose records hold rank r at this end
                        std::vector<u64> first, off;
                        u64 mine = 0;
                        for (u64 i = P.rec0[a]; i < P.rec0[a + 1]; i++)
                            if ((all[i].back != 0) == back) first.push_back(P.first[i]), off.push_back(P.off[i]), mine += P.grant[i];
                        if (first.empty() || r < first[0] || r - first[0] >= mine) continue;
                        const u64 pos = gp_place(first.data(), off.data(), first.size(), r);
                        CHECK(pos < got[a].size() && got[a][pos] == 0xBADull);
                        got[a][pos] = key;
                    }
                }
            }
            for (u64 r = 0; r < total; r++) CHECK(seen[r]);
        }
        for (int r = 0; r < G; r++) CHECK(got[r] == want[r]);
        g_runs++;
    }
    // the flags word: the first error in rank order
    {
        const u64 H[9] = {4, 0, 10, 0, (u64)(-NRG_E_NOT_SYNCED), 0, 0, (u64)(-NRG_E_INVAL), 0};
        CHECK(gp_flags_agree(H, 3) == NRG_E_NOT_SYNCED && gp_flags_agree(H, 1) == NRG_OK);
    }
    std::printf("group_pop_plan: ok (%ld runs, %ld records)\n", g_runs, g_records);
    return 0;
}
