// group_plan.cpp — what a replica group decides from its exchanged words
// (node-replication_amd/csrc/group_plan.hpp) without a GPU: a stand-alone program, built with the
// host compiler and -fsanitize=address,undefined and run by tests/test_group_plan.py. Exit status
// 0: every check held; else the failed checks are on stderr.
#include <stdint.h>
#include <stdio.h>

#include <utility>
#include <vector>

#include "../node-replication_amd/csrc/group_plan.hpp"

using namespace nrg::grp;

static int failures = 0;

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            if (failures < 50) fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
            failures++;                                                 \
        }                                                               \
    } while (0)

static uint64_t rng_state = 0x5EEDull;
static uint64_t rnd() {  // splitmix64, fixed seed
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// An exchanged matrix, written through its own indexing (not the header's accessors).
struct Mat {
    int G;
    uint64_t cw;
    std::vector<uint64_t> H;
    explicit Mat(int g) : G(g), cw(2 * (uint64_t)g + 5), H((size_t)g * (2 * (size_t)g + 5), 0) {
        for (int s = 0; s < G; s++) word(s, 4) = NRG_DS_HASHMAP, word(s, 1) = word(s, 2) = ~0ull;
    }
    uint64_t& puts(int s, int o) { return H[(size_t)s * cw + o]; }
    uint64_t& gets(int s, int o) { return H[(size_t)s * cw + G + o]; }
    uint64_t& word(int s, int k) { return H[(size_t)s * cw + 2 * G + k]; }
    uint64_t recv_puts(int r) { uint64_t t = 0; for (int s = 0; s < G; s++) t += puts(s, r); return t; }
    uint64_t recv_gets(int r) { uint64_t t = 0; for (int s = 0; s < G; s++) t += gets(s, r); return t; }
};

// conservation, offsets and totals of every rank's plan
static void check_plans(Mat& M) {
    const int G = M.G;
    CHECK(xw_cw(G) == M.cw);
    std::vector<PtPlan> P(G);
    for (int r = 0; r < G; r++) plan_for(M.H.data(), G, r, P[r]);
    for (int r = 0; r < G; r++) {
        uint64_t row_p = 0, row_k = 0, sum_p = 0, sum_k = 0, off_p = 0, off_k = 0;
        CHECK((int)P[r].pto.size() == G && (int)P[r].gfrom_off.size() == G);
        for (int o = 0; o < G; o++) {
            CHECK(P[r].pto[o] == P[o].pfrom[r]);
            CHECK(P[r].gto[o] == P[o].gfrom[r]);
            CHECK(P[r].pto[o] == M.puts(r, o) && P[r].gto[o] == M.gets(r, o));
            CHECK(xw_puts(M.H.data(), G, r, o) == M.puts(r, o) && xw_gets(M.H.data(), G, r, o) == M.gets(r, o));
            CHECK(P[r].pfrom_off[o] == off_p && P[r].gfrom_off[o] == off_k);  // exclusive prefix sums, rank order
            off_p += P[r].pfrom[o], off_k += P[r].gfrom[o];
            row_p += M.puts(r, o), row_k += M.gets(r, o);
            sum_p += P[r].pto[o], sum_k += P[r].gto[o];
        }
        CHECK(P[r].rp == off_p && P[r].rk == off_k);
        CHECK(P[r].rp == M.recv_puts(r) && P[r].rk == M.recv_gets(r));
        CHECK(sum_p == row_p && sum_k == row_k);    // what stage A compares with cap_p / cap_k
        CHECK(P[r].sp == row_p && P[r].sk == row_k);
    }
}

// plan_agree against the same conclusions drawn here
static void check_agree(Mat& M) {
    const int G = M.G;
    int rc = NRG_OK;
    for (int s = G - 1; s >= 0; s--)
        if (M.word(s, 3)) rc = -(int)M.word(s, 3);  // ends on the first in rank order
    if (rc == NRG_OK)
        for (int s = 1; s < G; s++)
            if (M.word(s, 4) != M.word(0, 4)) rc = NRG_E_INVAL;
    bool prev = false, grow = false;
    for (int s = 0; s < G; s++) {
        prev |= M.word(s, 0) != 0;
        grow |= M.recv_puts(s) > M.word(s, 1) || M.recv_gets(s) > M.word(s, 2);
    }
    const PlanAgree A = plan_agree(M.H.data(), G);
    std::vector<uint64_t> copy(M.H);  // another rank's copy of the same words
    const PlanAgree B = plan_agree(copy.data(), G);
    CHECK(A.rc == rc && B.rc == rc);
    if (rc != NRG_OK) return;
    CHECK(A.kind == M.word(0, 4) && B.kind == A.kind);
    CHECK(A.any_prev == prev && B.any_prev == prev);
    CHECK(A.any_grow == grow && B.any_grow == grow);
}

static void check_matrix(Mat& M) {
    check_plans(M);
    check_agree(M);
}

static void plans(int G) {
    {  // all zeros
        Mat M(G);
        check_matrix(M);
        CHECK(!plan_agree(M.H.data(), G).any_grow && !plan_agree(M.H.data(), G).any_prev);
    }
    for (int owner : {0, G - 1}) {  // everything to one owner
        Mat M(G);
        for (int s = 0; s < G; s++) M.puts(s, owner) = 1000 + s, M.gets(s, owner) = 1ull << 31;
        check_matrix(M);
        PtPlan P;
        plan_for(M.H.data(), G, owner, P);
        CHECK(P.rk == (uint64_t)G << 31);
    }
    {  // one rank silent
        Mat M(G);
        const int quiet = G / 2;
        for (int s = 0; s < G; s++)
            for (int o = 0; o < G; o++)
                if (s != quiet) M.puts(s, o) = 1 + (uint64_t)s * G + o, M.gets(s, o) = 7 * (uint64_t)o + s;
        check_matrix(M);
        PtPlan P;
        plan_for(M.H.data(), G, quiet, P);
        CHECK(P.sp == 0 && P.sk == 0);
        CHECK(G == 1 || P.rp != 0);
    }
    for (int t = 0; t < 300; t++) {  // fixed-seed matrices, entries up to 2^31, capacities around the totals
        Mat M(G);
        for (int s = 0; s < G; s++)
            for (int o = 0; o < G; o++) {
                const uint64_t a = rnd(), b = rnd();
                M.puts(s, o) = (a & 3) == 0 ? 0 : (a >> 8) % ((1ull << 31) + 1);
                M.gets(s, o) = (b & 3) == 0 ? 0 : (b >> 8) % ((1ull << 31) + 1);
            }
        for (int s = 0; s < G; s++) {
            M.word(s, 0) = rnd() & 1;
            M.word(s, 1) = M.recv_puts(s) + (t % 3 == 0 && s == (int)(rnd() % G) ? -1 : (int)(rnd() % 3));
            M.word(s, 2) = M.recv_gets(s) + (t % 5 == 0 && s == (int)(rnd() % G) ? -1 : (int)(rnd() % 3));
        }
        if (t % 7 == 3) M.word((int)(rnd() % G), 3) = 7, M.word((int)(rnd() % G), 3) = 1;  // errors -7 and -1
        if (t % 11 == 5 && G > 1) M.word(1 + (int)(rnd() % (G - 1)), 4) = NRG_DS_SKIPLIST;
        check_matrix(M);
    }
    // any_grow: exactly when some rank's received total exceeds its advertised capacity
    for (int s = 0; s < G; s++) {
        Mat M(G);
        for (int a = 0; a < G; a++)
            for (int o = 0; o < G; o++) M.puts(a, o) = 3, M.gets(a, o) = 2;
        for (int a = 0; a < G; a++) M.word(a, 1) = 3 * (uint64_t)G, M.word(a, 2) = 2 * (uint64_t)G;
        CHECK(!plan_agree(M.H.data(), G).any_grow);
        M.word(s, 1)--;
        CHECK(plan_agree(M.H.data(), G).any_grow);
        M.word(s, 1)++, M.word(s, 2)--;
        CHECK(plan_agree(M.H.data(), G).any_grow);
        M.word(s, 1) = M.word(s, 2) = ~0ull;  // the one-rank identity form: nothing to grow
        CHECK(!plan_agree(M.H.data(), G).any_grow);
    }
    // the first error in rank order, before mixed kinds
    for (int i = 0; i < G; i++)
        for (int j = i + 1; j < G; j++) {
            Mat M(G);
            M.word(i, 3) = (uint64_t)(-NRG_E_CAPACITY), M.word(j, 3) = (uint64_t)(-NRG_E_INVAL);
            M.word(j, 4) = NRG_DS_SKIPLIST;
            CHECK(plan_agree(M.H.data(), G).rc == NRG_E_CAPACITY);
            std::swap(M.word(i, 3), M.word(j, 3));
            CHECK(plan_agree(M.H.data(), G).rc == NRG_E_INVAL);
            M.word(i, 3) = M.word(j, 3) = 0;
            CHECK(plan_agree(M.H.data(), G).rc == NRG_E_INVAL);  // mixed kinds
            M.word(j, 4) = NRG_DS_HASHMAP;
            CHECK(plan_agree(M.H.data(), G).rc == NRG_OK);
        }
}

static void chunks() {
    const unsigned long long GC = GC_FROM_HEAD;
    for (uint64_t log_size : {1ull, GC, 2 * GC, 2 * GC + 1, 3 * GC, 1ull << 20, 1ull << 32, ~0ull})
        for (uint64_t max_batch : {0ull, 1ull, 100ull, GC, GC + 1, 1ull << 23, ~0ull}) {
            const uint64_t c = replay_chunk(log_size, max_batch);
            CHECK(c >= 1 && (c <= max_batch || (max_batch == 0 && c == 1)));
            if (log_size > 2 * GC) CHECK(c <= log_size - GC);
            if (max_batch == 0) CHECK(c == 1);
        }
}

static void reads(int G) {
    // the fields of the flags word do not overlap
    for (uint32_t mode = 0; mode <= 3; mode++)
        for (uint32_t limit = 1; limit <= 1024; limit++)
            for (uint32_t kind = 1; kind <= 7; kind++) {
                const uint64_t f = sk_flags(false, false, mode, true, limit, kind);
                CHECK((f & 1) == 0 && ((f >> 8) & 0xFF) == mode && ((f >> 16) & 0x7FF) == limit && (f >> 40) == kind);
                CHECK((f & ~((0xFFull << 8) | (0x7FFull << 16) | (0xFFFFFFull << 40))) == 0);
                CHECK(sk_flags(true, false, mode, true, limit, kind) == (f | 1));
                CHECK(sk_flags(false, false, mode, false, limit, kind) == (f & ~(0x7FFull << 16)));  // a seek: no limit
                CHECK(sk_flags(false, true, mode, false, limit, kind) == ((uint64_t)kind << 40));    // a count: no mode
            }
    // one differing rank, one bad bit, at every position
    const uint64_t f = sk_flags(false, false, NRG_SEEK_GT, true, 16, NRG_DS_SKIPLIST);
    std::vector<uint64_t> H(2 * (size_t)G);
    for (int r = 0; r < G; r++) H[2 * r] = 100 + r, H[2 * r + 1] = f;
    CHECK(sk_flags_agree(H.data(), G) == NRG_OK);
    for (int r = 0; r < G; r++) {
        H[2 * r + 1] = sk_flags(false, false, NRG_SEEK_GT, true, 17, NRG_DS_SKIPLIST);
        CHECK(G == 1 || sk_flags_agree(H.data(), G) == NRG_E_INVAL);
        H[2 * r + 1] = f | 1;
        CHECK(sk_flags_agree(H.data(), G) == NRG_E_INVAL);
        H[2 * r + 1] = f;
    }
    for (int r = 0; r < G; r++) H[2 * r + 1] = f | 1;  // the same on every rank, and bad
    CHECK(sk_flags_agree(H.data(), G) == NRG_E_INVAL);
    // the least lane width that covers G * limit slots, up to a wave
    for (uint32_t limit = 1; limit <= 1024; limit++) {
        uint32_t want = 6;
        for (uint32_t lw = 0; lw <= 6; lw++)
            if ((1ull << lw) >= (uint64_t)G * limit) {
                want = lw;
                break;
            }
        CHECK(scan_lane_log2(G, limit) == want);
    }
    // nmax near 2^32 does not wrap the bound
    CHECK(!sk_scan_fits(G, (1ull << 32) - 1, 1024) && !sk_scan_fits(G, (1ull << 32) - 1, 1));
}

static void scan_bound() {
    CHECK(SK_SCAN_MAX_SLOTS == 1ull << 27);
    CHECK(sk_scan_fits(8, 1ull << 14, 1024) && !sk_scan_fits(8, (1ull << 14) + 1, 1024));
    CHECK(sk_scan_fits(1, 1ull << 27, 1) && !sk_scan_fits(1, (1ull << 27) + 1, 1));
    CHECK(sk_scan_fits(64, 1ull << 11, 1024) && !sk_scan_fits(64, (1ull << 11) + 1, 1024));
    CHECK(sk_scan_fits(2, 1ull << 25, 2) && !sk_scan_fits(2, 1ull << 25, 3) && !sk_scan_fits(3, 1ull << 25, 2));
    // (a product taken in 32 bits would wrap to 0 here)
    CHECK(!sk_scan_fits(64, 1ull << 31, 2) && !sk_scan_fits(64, (1ull << 32) - 1, 1024));
}

static void lengths() {
    CHECK(lens_fp({1, 2, 3}) != lens_fp({2, 1, 3}) && lens_fp({1, 2, 3}) != lens_fp({1, 3, 2}));
    CHECK(lens_fp({1, 2}) != lens_fp({1, 2, 0}) && lens_fp({}) != lens_fp({0}));
    CHECK(lens_fp({5, 0, 9}) == lens_fp({5, 0, 9}));
    CHECK(lens_stride({}) == 0 && lens_stride({0, 0}) == 0 && lens_stride({3, 9, 4}) == 9 && lens_stride({~0ull, 1}) == ~0ull);
}

int main() {
    for (int G : {1, 2, 3, 8, 64}) {
        plans(G);
        reads(G);
    }
    chunks();
    scan_bound();
    lengths();
    if (failures) {
        fprintf(stderr, "group_plan: %d check(s) failed\n", failures);
        return 1;
    }
    printf("group_plan: ok\n");
    return 0;
}
