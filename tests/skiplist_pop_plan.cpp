// skiplist_pop_plan.cpp — the grants of a pop step (node-replication_amd/csrc/skiplist_pop_plan.hpp)
// against the sequential loop they restate: pop_front() / pop_back() called n_i times, record by record,
// on a deque of len entries. Exhaustive over small len and count vectors with every mix of ends, then
// the counts no small case reaches: 2^63, 2^64 - 1, and sums that wrap. A stand-alone host program
// (tests/test_skiplist_pop_plan.py builds it under AddressSanitizer and UndefinedBehaviorSanitizer).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <vector>

#include "../node-replication_amd/csrc/skiplist_pop_plan.hpp"

using namespace nrg;
using u64 = uint64_t;

static long g_cases = 0;

#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            std::exit(1);                                            \
        }                                                            \
    } while (0)

// One run against a map whose entries are their own ascending ranks 0 .. len - 1. `sat`: the sum of
// the counts as given, saturating (what a caller that does not clip would keep); else of the clipped
// counts (what sl_pop_plan keeps).
static void check_run(u64 len, const std::vector<u64>& n, const std::vector<bool>& back, bool sat) {
    std::deque<u64> q;
    const u64 model_len = len < 4096 ? len : 4096;  // (the loop below is run only on maps it can hold)
    for (u64 i = 0; i < model_len; i++) q.push_back(i);
    u64 S = 0, F = 0, B = 0;
    for (size_t i = 0; i < n.size(); i++) {
        const u64 m = slp::grant(sat ? n[i] : slp::clip(n[i], len), len, S);
        CHECK(m <= n[i] && slp::taken(len, S) + m <= len && slp::taken(len, S) == F + B);
        if (model_len == len) {
            // the sequential loop: n[i] times, while the map has an entry (a count of 2^63 stops there)
            u64 got = 0;
            for (u64 r = 0; r < n[i] && !q.empty(); r++, got++) {
                const u64 e = back[i] ? q.back() : q.front();
                if (back[i]) q.pop_back(); else q.pop_front();
                CHECK(got < m && slp::rank_of(back[i], len, back[i] ? B : F, got) == e);
            }
            CHECK(got == m);
        }
        (back[i] ? B : F) += m;
        S = sat ? slp::add(S, n[i]) : S + slp::clip(n[i], len);
        g_cases++;
    }
    CHECK(F + B == slp::taken(len, S) && F + B <= len);
    if (model_len == len) CHECK(q.size() == len - (F + B));
}

int main() {
    // exhaustive: len 0..6, up to 4 records, counts 0..len + 1, every mix of ends, both ways of summing
    for (u64 len = 0; len <= 6; len++)
        for (size_t recs = 1; recs <= 4; recs++) {
            const u64 base = len + 2;
            u64 combos = 1;
            for (size_t i = 0; i < recs; i++) combos *= base;
            for (u64 c = 0; c < combos; c++)
                for (unsigned ends = 0; ends < (1u << recs); ends++) {
                    std::vector<u64> n(recs);
                    std::vector<bool> back(recs);
                    u64 x = c;
                    for (size_t i = 0; i < recs; i++) {
                        n[i] = x % base;
                        x /= base;
                        back[i] = (ends >> i) & 1;
                    }
                    check_run(len, n, back, false);
                    check_run(len, n, back, true);
                }
        }
    // the large counts: alone, after a small one, twice (the plain sum wraps to a small number), and
    // on a map as large as nrg_open allows
    const u64 big[] = {1ull << 63, ~0ull, (1ull << 63) + 1, ~0ull - 1, 1ull << 32};
    for (u64 len : {0ull, 1ull, 5ull, 350ull, 1ull << 28})
        for (u64 a : big)
            for (u64 b : big)
                for (unsigned ends = 0; ends < 16; ends++) {
                    const std::vector<u64> n = {3, a, b, 1};
                    const std::vector<bool> back = {bool(ends & 1), bool(ends & 2), bool(ends & 4), bool(ends & 8)};
                    check_run(len, n, back, false);
                    check_run(len, n, back, true);
                }
    CHECK(slp::add(1ull << 63, 1ull << 63) == ~0ull && slp::add(~0ull, 1) == ~0ull && slp::add(2, 3) == 5);
    CHECK(slp::clip(1ull << 63, 350) == 350 && slp::clip(7, 350) == 7 && slp::clip(5, 0) == 0);
    CHECK(slp::grant(1ull << 63, 350, 0) == 350 && slp::grant(1ull << 63, 350, 349) == 1 && slp::grant(9, 350, ~0ull) == 0);
    CHECK(slp::rank_of(false, 10, 2, 3) == 5 && slp::rank_of(true, 10, 2, 3) == 4 && slp::rank_of(true, 1, 0, 0) == 0);
    std::printf("skiplist_pop_plan: ok (%ld records)\n", g_cases);
    return 0;
}
