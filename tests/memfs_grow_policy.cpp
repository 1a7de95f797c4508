// memfs_grow_policy.cpp — the arithmetic of the file store's capacity growth (csrc/memfs_plan.hpp:
// mf_rec_need, mf_grow_log2, plan_need) without a GPU. A stand-alone program, built and run by
// tests/test_memfs_grow_cpu.py under AddressSanitizer and UndefinedBehaviorSanitizer.
//   1  mf_rec_need against a restatement in 128-bit arithmetic (so that nothing here can wrap), on the
//      edge records of include/nrgpu.h "File store: capacity growth" and on seeded random ones
//   2  mf_grow_log2 against a loop over the powers of two
//   3  the chunking property: the capacity after a log is the same whether the need is folded record by
//      record, chunk by chunk for random cuts, or over the whole log at once
//   4  plan_need against the records the plan's cut produces
// With --dump it also prints every record of 1 with the header's answer, one per line, for the Python
// model (tests/memfs_grow_model.py need()) to be compared with.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../node-replication_amd/csrc/memfs_plan.hpp"

using namespace nrg::mfp;
typedef unsigned __int128 u128;

struct Rec {
    uint64_t ino, off;
    uint32_t op, len;
};

static int fails = 0;
#define CHECK(c, ...)                         \
    do {                                      \
        if (!(c)) {                           \
            if (fails++ < 20) {               \
                std::printf("FAIL %s: ", #c); \
                std::printf(__VA_ARGS__);     \
                std::printf("\n");            \
            }                                 \
        }                                     \
    } while (0)

// the definition, in the order the replay checks a record
static uint64_t ref_need(const Rec& r, uint64_t files, uint64_t max_bytes) {
    if (r.op > 3 || r.len > 128) return 0;                                // EINVAL
    if (r.ino < 5 || (u128)r.ino >= (u128)5 + files) return 0;            // ENOENT
    if (r.op == 0) {                                                      // Write
        const u128 end = (u128)r.off + r.len;
        return r.len > 0 && end <= max_bytes ? (uint64_t)end : 0;
    }
    if (r.op == 3) return r.off <= max_bytes ? r.off : 0;                 // SetAttr
    return 0;
}

static uint32_t ref_log2(uint32_t log2_b, uint64_t need, uint32_t max_log2) {
    for (uint32_t l = log2_b; l < max_log2; l++)
        if (((u128)1 << l) >= need) return l;
    return max_log2 > log2_b ? max_log2 : log2_b;
}

static std::vector<Rec> edge_records(uint64_t files, uint64_t mx) {
    const uint64_t U = ~0ull;
    std::vector<Rec> v;
    for (uint32_t op = 0; op <= 4; op++)
        for (uint32_t len : {0u, 1u, 127u, 128u, 129u})
            for (uint64_t ino : {(uint64_t)4, (uint64_t)5, 5 + files - 1, 5 + files, U, (uint64_t)0}) {
                const uint64_t offs[] = {0,      1,      mx - 129, mx - 128, mx - 127, mx - 1,  mx,     mx + 1,
                                         2 * mx, 1ull << 40, U - 129,  U - 128,  U - 127,  U - 1,   U,      mx - len,
                                         mx - len + 1};
                for (uint64_t off : offs) v.push_back(Rec{ino, off, op, len});
            }
    return v;
}

int main(int argc, char** argv) {
    const bool dump = argc > 1 && !std::strcmp(argv[1], "--dump");
    std::mt19937_64 rng(20240607);
    // 1
    const uint64_t geos[][2] = {{1, 4096}, {3, 1024}, {5, 1ull << 20}, {1, 128}, {65536, 8192}, {8, 1ull << 26}};
    uint64_t checked = 0;
    for (auto& g : geos) {
        const uint64_t files = g[0], mx = g[1];
        std::vector<Rec> recs = edge_records(files, mx);
        for (int i = 0; i < 4000; i++) {
            Rec r;
            r.ino = rng() % 8 ? 5 + rng() % files : rng();
            const uint64_t k = rng() % 4;
            r.off = k == 0 ? rng() : (k == 1 ? rng() % (2 * mx) : (k == 2 ? mx - rng() % 200 : ~0ull - rng() % 200));
            r.op = rng() % 16 ? (uint32_t)(rng() % 4) : (uint32_t)rng();
            r.len = rng() % 16 ? (uint32_t)(rng() % 129) : (uint32_t)rng();
            recs.push_back(r);
        }
        for (const Rec& r : recs) {
            const uint64_t got = mf_rec_need(r.ino, r.off, r.op, r.len, files, mx);
            CHECK(got == ref_need(r, files, mx), "ino %llu off %llu op %u len %u files %llu max %llu: %llu",
                  (unsigned long long)r.ino, (unsigned long long)r.off, r.op, r.len, (unsigned long long)files,
                  (unsigned long long)mx, (unsigned long long)got);
            CHECK(got <= mx, "a need past the bound");
            checked++;
            if (dump && files <= 5)
                std::printf("need %llu %llu %u %u %llu %llu %llu\n", (unsigned long long)r.ino, (unsigned long long)r.off,
                            r.op, r.len, (unsigned long long)files, (unsigned long long)mx, (unsigned long long)got);
        }
    }
    // the edges by name: end == max, end == max + 1, SetAttr at max and max + 1, 2^64 - 1, a bad ino, len 129
    CHECK(mf_rec_need(5, 4096 - 128, 0, 128, 1, 4096) == 4096, "end == max");
    CHECK(mf_rec_need(5, 4096 - 127, 0, 128, 1, 4096) == 0, "end == max + 1");
    CHECK(mf_rec_need(5, 4096, 3, 0, 1, 4096) == 4096, "SetAttr at max");
    CHECK(mf_rec_need(5, 4097, 3, 0, 1, 4096) == 0, "SetAttr at max + 1");
    CHECK(mf_rec_need(5, ~0ull, 0, 1, 1, 4096) == 0 && mf_rec_need(5, ~0ull - 3, 0, 128, 1, 4096) == 0, "offsets near 2^64");
    CHECK(mf_rec_need(6, 100, 0, 8, 1, 4096) == 0 && mf_rec_need(4, 1ull << 60, 3, 0, 1, 4096) == 0, "ENOENT");
    CHECK(mf_rec_need(5, 100, 0, 129, 1, 4096) == 0 && mf_rec_need(5, 1ull << 60, 0, 129, 1, 4096) == 0, "len 129");
    CHECK(mf_rec_need(5, 100, 0, 0, 1, 4096) == 0 && mf_rec_need(5, 4096, 0, 0, 1, 4096) == 0, "len 0 needs nothing");
    // 2
    for (uint32_t lb = LOG2_MIN; lb <= LOG2_MAX; lb++)
        for (uint32_t ml = 0; ml <= LOG2_MAX; ml++) {
            std::vector<uint64_t> needs = {0, 1, 127, 128, 129, ~0ull};
            for (uint32_t l = LOG2_MIN; l <= LOG2_MAX; l++)
                for (int d = -1; d <= 1; d++) needs.push_back((1ull << l) + d);
            for (uint64_t n : needs) {
                const uint32_t got = mf_grow_log2(lb, n, ml);
                CHECK(got == ref_log2(lb, n, ml), "log2_b %u need %llu max %u: %u", lb, (unsigned long long)n, ml, got);
                CHECK(got >= lb && (got <= ml || got == lb), "never shrinks, never past the bound");
            }
        }
    // 3
    for (int trial = 0; trial < 300; trial++) {
        const uint32_t lb = LOG2_MIN + rng() % 6, ml = lb + rng() % 10;
        const uint64_t files = 1 + rng() % 5, mx = 1ull << ml;
        const size_t n = 1 + rng() % 200;
        std::vector<Rec> log(n);
        for (Rec& r : log) {
            r.ino = rng() % 10 ? 5 + rng() % files : 5 + files;
            r.off = rng() % 4 ? rng() % (mx >> (rng() % ml + 0)) : mx - rng() % 300 + rng() % 150;
            r.op = rng() % 20 ? (uint32_t)(rng() % 4) : 9;
            r.len = rng() % 20 ? (uint32_t)(rng() % 129) : 129;
        }
        uint32_t by_rec = lb;  // record by record: the model's way
        for (const Rec& r : log) by_rec = mf_grow_log2(by_rec, mf_rec_need(r.ino, r.off, r.op, r.len, files, mx), ml);
        uint64_t all = 0;  // the whole log as one chunk
        for (const Rec& r : log) {
            const uint64_t x = mf_rec_need(r.ino, r.off, r.op, r.len, files, mx);
            all = x > all ? x : all;
        }
        CHECK(mf_grow_log2(lb, all, ml) == by_rec, "one chunk");
        for (int cut = 0; cut < 8; cut++) {  // random cuts; the need word is a running maximum, as the device's
            uint32_t by_chunk = lb;
            uint64_t word = 0;
            for (size_t i = 0; i < n;) {
                const size_t m = 1 + rng() % (cut % 2 ? 3 : n);
                for (size_t k = i; k < n && k < i + m; k++) {
                    const uint64_t x = mf_rec_need(log[k].ino, log[k].off, log[k].op, log[k].len, files, mx);
                    if (x > (1ull << by_chunk) && x > word) word = x;  // (a workgroup skips a need B already holds)
                }
                by_chunk = mf_grow_log2(by_chunk, word, ml);
                i += m;
            }
            CHECK(by_chunk == by_rec, "chunks of cut %d: %u != %u", cut, by_chunk, by_rec);
        }
    }
    // 4
    for (int trial = 0; trial < 200; trial++) {
        const uint32_t adm = LOG2_MIN + rng() % 14;
        const uint64_t files = 1 + rng() % 4, mx = 1ull << adm;
        std::vector<nrg_memfs_wr> rq(1 + rng() % 20);
        uint64_t want = 0;
        for (nrg_memfs_wr& r : rq) {
            r.ino = rng() % 8 ? 5 + rng() % files : 5 + files;
            r.offset = rng() % 6 ? rng() % (mx + 64) : ~0ull - rng() % 64;
            r.len = rng() % 6 ? rng() % (mx / 2 + 2) : (rng() % 2 ? 0 : ~0ull);
            r.data_off = 0;
            const bool ok = r.ino >= 5 && r.ino - 5 < files && (u128)r.offset + r.len <= mx && r.len;
            if (ok && r.offset + r.len > want) want = r.offset + r.len;
        }
        CHECK(plan_need(adm, files, rq.data(), rq.size()) == want, "plan_need");
    }
    if (fails) {
        std::printf("memfs_grow_policy: %d FAILED\n", fails);
        return 1;
    }
    std::printf("memfs_grow_policy: ok (%llu records)\n", (unsigned long long)checked);
    return 0;
}
