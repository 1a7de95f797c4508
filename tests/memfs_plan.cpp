// memfs_plan.cpp — the cut of the file store's writes of any length into 128-byte log records
// (node-replication_amd/csrc/memfs_plan.hpp, include/nrgpu.h nrg_memfs_pwrite*) without a GPU: a
// stand-alone program, built with the host compiler and -fsanitize=address,undefined and run by
// tests/test_memfs_plan.py. The cut is checked against a restatement that walks a request byte by
// byte, and the fragments, applied in order as the replay applies Write records, against one memcpy per
// valid request. Exit status 0: every check held; else the failed checks are on stderr.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../node-replication_amd/csrc/memfs_plan.hpp"

using namespace nrg::mfp;

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

struct Rec {  // a log record as the replay sees it
    uint64_t ino, offset;
    uint32_t len;
    uint8_t data[128];
};

// The restatement: request r's records, byte by byte. A valid request's byte p goes to the record of
// its line p / 128; a record starts where the line changes.
static std::vector<Rec> expect(uint32_t log2_b, uint64_t files, const nrg_memfs_wr& r, const std::vector<uint8_t>& data,
                               uint64_t* written, uint8_t* some) {
    const uint64_t B = 1ull << log2_b;
    std::vector<Rec> out;
    Rec z;
    memset(&z, 0, sizeof z);
    z.ino = r.ino;
    if (r.ino < 5 || r.ino >= 5 + files) {
        z.offset = r.offset;
        out.push_back(z);
        *written = NRG_MEMFS_ENOENT, *some = 0;
        return out;
    }
    // offset + len > B without the sum: the request's last byte, if it has one, is at or past B
    const bool past = r.offset > B || (r.len > 0 && (r.len - 1 >= B || r.offset + (r.len - 1) >= B));
    if (past) {
        z.offset = B, z.len = 1;
        out.push_back(z);
        *written = NRG_MEMFS_EFBIG, *some = 0;
        return out;
    }
    *written = r.len, *some = 1;
    if (r.len == 0) {
        z.offset = r.offset;
        out.push_back(z);
        return out;
    }
    for (uint64_t q = 0; q < r.len; q++) {
        const uint64_t p = r.offset + q;
        if (out.empty() || p / 128 != out.back().offset / 128) {
            z.offset = p;
            out.push_back(z);
        }
        Rec& b = out.back();
        b.data[b.len++] = data[r.data_off + q];
    }
    return out;
}

// what the replay does with a Write record (include/nrgpu.h): valid exactly when it ends inside the file
static void apply(std::vector<uint8_t>& store, uint32_t log2_b, uint64_t files, const Rec& w) {
    const uint64_t B = 1ull << log2_b;
    if (w.ino < 5 || w.ino >= 5 + files) return;
    if (!(w.offset <= B && w.len <= B - w.offset)) return;
    for (uint32_t q = 0; q < w.len; q++) store[(w.ino - 5) * B + w.offset + q] = w.data[q];
}

// One call: the plan and every fragment against the restatement, and the store the fragments leave
// against one memcpy per valid request.
static void check_call(uint32_t log2_b, uint64_t files, const std::vector<nrg_memfs_wr>& reqs,
                       const std::vector<uint8_t>& data) {
    const uint64_t n = reqs.size(), B = 1ull << log2_b;
    std::vector<uint64_t> first(n + 1, ~0ull), written(n, ~0ull);
    std::vector<uint8_t> some(n, 7);
    CHECK(plan(log2_b, files, reqs.data(), n, data.size(), first.data(), written.data(), some.data()) == NRG_OK);
    std::vector<uint64_t> first2(n + 1, ~0ull);  // written and some may be NULL
    CHECK(plan(log2_b, files, reqs.data(), n, data.size(), first2.data(), nullptr, nullptr) == NRG_OK);
    CHECK(first2 == first);
    std::vector<uint8_t> got(files * B, 1), want(files * B, 1);
    uint64_t run = 0;
    for (uint64_t i = 0; i < n; i++) {
        const nrg_memfs_wr& r = reqs[i];
        uint64_t w = 0;
        uint8_t s = 0;
        const std::vector<Rec> e = expect(log2_b, files, r, data, &w, &s);
        CHECK(first[i] == run);
        CHECK(written[i] == w && some[i] == s);
        const Cut c = cut_of(log2_b, files, r.ino, r.offset, r.len);
        CHECK(c.frags == e.size() && c.frags >= 1);
        CHECK(c.written == w && c.some == s);
        for (uint64_t k = 0; k < c.frags && k < e.size(); k++) {
            uint64_t off = ~0ull, src = ~0ull;
            uint32_t len = ~0u;
            frag_of(log2_b, c.kind, r.offset, r.len, k, &off, &len, &src);
            CHECK(off == e[k].offset && len == e[k].len && len <= 128);
            Rec f;
            memset(&f, 0, sizeof f);
            f.ino = r.ino, f.offset = off, f.len = len;
            if (c.kind == CUT_BYTES) {
                CHECK(len >= 1 && off / 128 == (off + len - 1) / 128);  // one line, so one slot of the line sort
                CHECK(r.data_off + src + len <= data.size());
                for (uint32_t q = 0; q < len; q++) f.data[q] = data[r.data_off + src + q];
            } else {
                CHECK(src == 0);
            }
            CHECK(memcmp(f.data, e[k].data, 128) == 0);
            apply(got, log2_b, files, f);
        }
        if (s && r.len) memcpy(&want[(r.ino - 5) * B + r.offset], &data[r.data_off], r.len);
        run += e.size();
    }
    CHECK(first[n] == run);
    CHECK(got == want);
}

static nrg_memfs_wr rq(uint64_t ino, uint64_t offset, uint64_t len, uint64_t data_off) {
    nrg_memfs_wr r;
    r.ino = ino, r.offset = offset, r.len = len, r.data_off = data_off;
    return r;
}

static std::vector<uint8_t> bytes(size_t n) {
    std::vector<uint8_t> d(n);
    for (size_t i = 0; i < n; i++) d[i] = (uint8_t)(rnd() | 2);  // never the store's 1, never 0
    return d;
}

// the edge list of the feature's tests, for F files of B bytes
static std::vector<nrg_memfs_wr> edges(uint32_t log2_b, uint64_t files, uint64_t data_bytes) {
    const uint64_t B = 1ull << log2_b;
    std::vector<nrg_memfs_wr> v;
    v.push_back(rq(5, 0, 0, 0));
    v.push_back(rq(5, 0, 1, 0));
    v.push_back(rq(5, 0, 128, 3));
    v.push_back(rq(6, 0, B, 0));  // a whole file
    if (B >= 512) {
        v.push_back(rq(5, 1, 128, 7));
        v.push_back(rq(5, 127, 2, 9));
        v.push_back(rq(7, 100, 300, 11));  // 28 / 128 / 128 / 16
    }
    v.push_back(rq(5, B - 77, 77, 1));  // ends exactly at B
    v.push_back(rq(5, B, 0, 0));        // valid
    v.push_back(rq(5, B - 1, 2, 0));    // offset + len = B + 1
    v.push_back(rq(5, B + 1, 0, 0));
    v.push_back(rq(5, 1ull << 63, 1ull << 63, 0));  // no overflow
    v.push_back(rq(5, 0, ~0ull, 0));
    v.push_back(rq(5, ~0ull, ~0ull, ~0ull));  // a failing request's data_off is not looked at
    v.push_back(rq(4, 0, 10, ~0ull));
    v.push_back(rq(5 + files, 3, 10, 0));
    v.push_back(rq(0, ~0ull, ~0ull, 0));
    for (uint64_t a = 0; a < 16; a++) v.push_back(rq(5 + a % files, (a * 37) % (B - 40), 33 + a % 7, 16 + a));
    v.push_back(rq(5, 5, 40, data_bytes - 40));  // ends on the last byte of data
    v.push_back(rq(6, 10, 50, 64));              // two requests share one data_off
    v.push_back(rq(7, 20, 50, 64));
    v.push_back(rq(6, 30, 60, 200));  // overlaps the one before the last: the later wins
    return v;
}

static void check_errors() {
    std::vector<uint64_t> first(4, 0);
    const nrg_memfs_wr ok = rq(5, 0, 10, 0);
    // geometry outside what nrg_open accepts
    CHECK(plan(6, 1, &ok, 1, 10, first.data(), nullptr, nullptr) == NRG_E_INVAL);
    CHECK(plan(27, 1, &ok, 1, 10, first.data(), nullptr, nullptr) == NRG_E_INVAL);
    CHECK(plan(12, 0, &ok, 1, 10, first.data(), nullptr, nullptr) == NRG_E_INVAL);
    CHECK(plan(12, (1ull << 16) + 1, &ok, 1, 10, first.data(), nullptr, nullptr) == NRG_E_INVAL);
    CHECK(plan(26, 16, &ok, 1, 10, first.data(), nullptr, nullptr) == NRG_E_INVAL);  // 2^30 bytes
    CHECK(plan(26, 8, &ok, 1, 10, first.data(), nullptr, nullptr) == NRG_OK);
    CHECK(plan(7, 1ull << 16, &ok, 1, 10, first.data(), nullptr, nullptr) == NRG_OK);
    // pointers
    CHECK(plan(12, 1, nullptr, 1, 10, first.data(), nullptr, nullptr) == NRG_E_INVAL);
    CHECK(plan(12, 1, &ok, 1, 10, nullptr, nullptr, nullptr) == NRG_E_INVAL);
    CHECK(plan(12, 1, nullptr, 0, 0, nullptr, nullptr, nullptr) == NRG_OK);
    first[0] = 9;
    CHECK(plan(12, 1, nullptr, 0, 0, first.data(), nullptr, nullptr) == NRG_OK && first[0] == 0);
    // a valid request's bytes must lie inside data
    CHECK(plan(12, 1, &ok, 1, 9, first.data(), nullptr, nullptr) == NRG_E_INVAL);
    const nrg_memfs_wr off1 = rq(5, 0, 10, 1);
    CHECK(plan(12, 1, &off1, 1, 10, first.data(), nullptr, nullptr) == NRG_E_INVAL);
    CHECK(plan(12, 1, &off1, 1, 11, first.data(), nullptr, nullptr) == NRG_OK);
    const nrg_memfs_wr wrap = rq(5, 0, 10, ~0ull - 3);  // data_off + len overflows
    CHECK(plan(12, 1, &wrap, 1, 1000, first.data(), nullptr, nullptr) == NRG_E_INVAL);
    const nrg_memfs_wr empty = rq(5, 7, 0, 1000);  // no bytes: data_off is not looked at
    CHECK(plan(12, 1, &empty, 1, 0, first.data(), nullptr, nullptr) == NRG_OK && first[1] == 1);
}

int main() {
    check_errors();
    for (uint32_t log2_b : {12u, 7u}) {
        const std::vector<uint8_t> data = bytes(4096 + 13);
        const std::vector<nrg_memfs_wr> e = edges(log2_b, 3, data.size());
        check_call(log2_b, 3, e, data);
        for (const nrg_memfs_wr& r : e) check_call(log2_b, 3, std::vector<nrg_memfs_wr>(1, r), data);
    }
    // about a thousand seeded random requests over several geometries, in calls of 1 .. 40
    uint64_t total = 0;
    while (total < 1000) {
        const uint32_t log2_b = 7 + (uint32_t)(rnd() % 7);
        const uint64_t files = 1 + rnd() % 4, B = 1ull << log2_b;
        const std::vector<uint8_t> data = bytes(1 + rnd() % (2 * B));
        std::vector<nrg_memfs_wr> v;
        const uint64_t n = 1 + rnd() % 40;
        for (uint64_t i = 0; i < n; i++) {
            uint64_t ino = 5 + rnd() % files, off = rnd() % (B + 1), len;
            switch (rnd() % 8) {
            case 0: len = 0; break;
            case 1: len = B - off; break;                    // ends exactly at B
            case 2: len = B - off + 1 + rnd() % 3; break;    // EFBIG
            case 3: ino = rnd() % 12; len = rnd() % 200; break;  // sometimes ENOENT
            case 4: off = (off & ~127ull) % B; len = 128 * (rnd() % ((B - off) / 128 + 1)); break;  // whole lines
            default: len = rnd() % (B - off + 1); break;
            }
            const bool bytes_wanted = ino >= 5 && ino < 5 + files && off <= B && len <= B - off && len > 0;
            if (bytes_wanted && len > data.size()) len = data.size();
            const uint64_t doff = bytes_wanted ? rnd() % (data.size() - len + 1) : rnd();
            v.push_back(rq(ino, off, len, doff));
        }
        check_call(log2_b, files, v, data);
        total += n;
    }
    if (failures) {
        fprintf(stderr, "memfs_plan: %d checks failed\n", failures);
        return 1;
    }
    printf("memfs_plan: ok (%llu random requests)\n", (unsigned long long)total);
    return 0;
}
