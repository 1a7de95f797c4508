// memfs_read_plan.cpp — the cut of the file store's logged reads of any length into 128-byte Read records
// (node-replication_amd/csrc/memfs_plan.hpp, include/nrgpu.h nrg_memfs_pread_logged*) without a GPU: a
// stand-alone program, built with the host compiler and -fsanitize=address,undefined and run by
// tests/test_memfs_read_plan.py. first, offs, some and every fragment's (offset, len) are checked against a
// restatement that walks a request byte by byte, and the way back (rfrag_at, rfrag_pos) against the
// positions that walk met. Exit status 0: every check held; else the failed checks are on stderr.
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

struct Rec {  // a Read record's header
    uint64_t offset;
    uint32_t len;
};

// The restatement: request r's records, byte by byte. Byte q of what it plans to read lies in the record
// of its line (offset + q) / 128; a record starts where the line changes. where[q] = (record, index).
static std::vector<Rec> expect(uint32_t log2_adm, uint64_t files, const nrg_memfs_rd& r, uint64_t* planned, uint8_t* some,
                               std::vector<Rec>* where) {
    const uint64_t A = 1ull << log2_adm;
    std::vector<Rec> out;
    where->clear();
    *planned = 0;
    if (r.ino < 5 || r.ino >= 5 + files) {
        out.push_back(Rec{r.offset, 0});
        *some = 0;
        return out;
    }
    *some = 1;
    if (r.len == 0 || r.offset >= A) {
        out.push_back(Rec{r.offset, 0});
        return out;
    }
    // bytes offset, offset + 1, ... while there are len of them and they lie below A
    for (uint64_t q = 0; q < r.len && r.offset + q < A; q++) {
        const uint64_t p = r.offset + q;
        if (out.empty() || p / 128 != out.back().offset / 128) out.push_back(Rec{p, 0});
        where->push_back(Rec{out.size() - 1, out.back().len});
        out.back().len++;
        ++*planned;
    }
    return out;
}

static void check_call(uint32_t log2_adm, uint64_t files, const std::vector<nrg_memfs_rd>& reqs) {
    const uint64_t n = reqs.size();
    std::vector<uint64_t> first(n + 1, ~0ull), offs(n + 1, ~0ull);
    std::vector<uint8_t> some(n, 7);
    CHECK(read_plan(log2_adm, files, reqs.data(), n, first.data(), offs.data(), some.data()) == NRG_OK);
    std::vector<uint64_t> first2(n + 1, ~0ull);  // offs and some may be NULL
    CHECK(read_plan(log2_adm, files, reqs.data(), n, first2.data(), nullptr, nullptr) == NRG_OK);
    CHECK(first2 == first);
    uint64_t run = 0, bytes = 0;
    std::vector<Rec> where;
    for (uint64_t i = 0; i < n; i++) {
        const nrg_memfs_rd& r = reqs[i];
        uint64_t p = 0;
        uint8_t s = 0;
        const std::vector<Rec> e = expect(log2_adm, files, r, &p, &s, &where);
        CHECK(first[i] == run && offs[i] == bytes && some[i] == s);
        const RCut c = rcut_of(log2_adm, files, r.ino, r.offset, r.len);
        CHECK(c.frags == e.size() && c.frags >= 1 && c.planned == p && c.some == s && c.bytes == (p > 0));
        uint64_t pos = 0;
        for (uint64_t k = 0; k < c.frags && k < e.size(); k++) {
            uint64_t off = ~0ull;
            uint32_t len = ~0u;
            rfrag_of(c, r.offset, k, &off, &len);
            CHECK(off == e[k].offset && len == e[k].len && len <= 128);
            if (c.bytes) {
                CHECK(len >= 1 && off / 128 == (off + len - 1) / 128);  // one line
                CHECK(rfrag_pos(r.offset, c.planned, c.frags, k) == pos);
            }
            pos += len;
        }
        if (c.bytes) CHECK(rfrag_pos(r.offset, c.planned, c.frags, c.frags) == p && pos == p);
        for (uint64_t q = 0; q < where.size(); q++) {  // the way back: a slot byte's fragment and index
            uint32_t idx = ~0u;
            const uint64_t k = rfrag_at(r.offset, q, &idx);
            CHECK(k == where[q].offset && idx == where[q].len);
        }
        run += e.size();
        bytes += p;
    }
    CHECK(first[n] == run && offs[n] == bytes);
}

static nrg_memfs_rd rq(uint64_t ino, uint64_t offset, uint64_t len) {
    nrg_memfs_rd r;
    r.ino = ino, r.offset = offset, r.len = len;
    return r;
}

// the edge list of the feature's tests, for F files admitted against A bytes
static std::vector<nrg_memfs_rd> edges(uint32_t log2_adm, uint64_t files) {
    const uint64_t A = 1ull << log2_adm;
    std::vector<nrg_memfs_rd> v;
    v.push_back(rq(5, 0, 0));
    v.push_back(rq(5, 0, 1));
    v.push_back(rq(5, A - 1, 1));
    for (uint64_t off : {0ull, 1ull, 127ull, 128ull})
        for (uint64_t len : {127ull, 128ull, 129ull}) v.push_back(rq(6, off % A, len));
    v.push_back(rq(7, 100 % A, 128));  // across two lines
    v.push_back(rq(7, 60 % A, 300));   // across three
    v.push_back(rq(5, 0, A));          // the whole file
    v.push_back(rq(6, 0, ~0ull));      // read to the end
    v.push_back(rq(4, 0, 10));
    v.push_back(rq(7, 67 % A, ~0ull));
    v.push_back(rq(5, A, 5));
    v.push_back(rq(5, A + 1, 5));
    v.push_back(rq(5, 1ull << 63, ~0ull));
    v.push_back(rq(5, ~0ull, ~0ull));
    v.push_back(rq(5, ~0ull - 3, 10));  // offset + len overflows
    v.push_back(rq(5, A - 1, ~0ull));
    v.push_back(rq(5 + files, 3, 10));
    v.push_back(rq(0, ~0ull, ~0ull));
    v.push_back(rq(6, 40 % A, 200));
    v.push_back(rq(6, 40 % A, 200));  // the same range twice
    return v;
}

static void check_errors() {
    std::vector<uint64_t> first(4, 0), offs(4, 0);
    const nrg_memfs_rd ok = rq(5, 0, 10);
    // geometry outside what nrg_open accepts
    CHECK(read_plan(6, 1, &ok, 1, first.data(), offs.data(), nullptr) == NRG_E_INVAL);
    CHECK(read_plan(27, 1, &ok, 1, first.data(), offs.data(), nullptr) == NRG_E_INVAL);
    CHECK(read_plan(12, 0, &ok, 1, first.data(), offs.data(), nullptr) == NRG_E_INVAL);
    CHECK(read_plan(12, (1ull << 16) + 1, &ok, 1, first.data(), offs.data(), nullptr) == NRG_E_INVAL);
    CHECK(read_plan(26, 16, &ok, 1, first.data(), offs.data(), nullptr) == NRG_E_INVAL);  // 2^30 bytes
    CHECK(read_plan(26, 8, &ok, 1, first.data(), offs.data(), nullptr) == NRG_OK);
    CHECK(read_plan(7, 1ull << 16, &ok, 1, first.data(), offs.data(), nullptr) == NRG_OK);
    // pointers
    CHECK(read_plan(12, 1, nullptr, 1, first.data(), offs.data(), nullptr) == NRG_E_INVAL);
    CHECK(read_plan(12, 1, &ok, 1, nullptr, offs.data(), nullptr) == NRG_E_INVAL);
    CHECK(read_plan(12, 1, nullptr, 0, nullptr, nullptr, nullptr) == NRG_OK);
    first[0] = offs[0] = 9;
    CHECK(read_plan(12, 1, nullptr, 0, first.data(), offs.data(), nullptr) == NRG_OK && first[0] == 0 && offs[0] == 0);
    CHECK(read_plan(12, 1, &ok, 1, first.data(), offs.data(), nullptr) == NRG_OK && first[1] == 1 && offs[1] == 10);
}

int main() {
    check_errors();
    for (uint32_t log2_adm : {12u, 7u, 26u}) {
        const std::vector<nrg_memfs_rd> e = edges(log2_adm, 3);
        if (log2_adm != 26) check_call(log2_adm, 3, e);  // (a byte walk of 2^26 is for single requests below)
        for (const nrg_memfs_rd& r : e)
            if (log2_adm != 26 || r.len <= 300) check_call(log2_adm, 3, std::vector<nrg_memfs_rd>(1, r));
    }
    // about a thousand seeded random requests over several geometries, in calls of 1 .. 40
    uint64_t total = 0;
    while (total < 1000) {
        const uint32_t log2_adm = 7 + (uint32_t)(rnd() % 7);
        const uint64_t files = 1 + rnd() % 4, A = 1ull << log2_adm;
        std::vector<nrg_memfs_rd> v;
        const uint64_t n = 1 + rnd() % 40;
        for (uint64_t i = 0; i < n; i++) {
            uint64_t ino = 5 + rnd() % files, off = rnd() % (A + 1), len;
            switch (rnd() % 8) {
            case 0: len = 0; break;
            case 1: len = A - off; break;                    // ends exactly at A
            case 2: len = A - off + 1 + rnd() % 3; break;    // clipped
            case 3: ino = rnd() % 12; len = rnd() % 200; break;  // sometimes ENOENT
            case 4: off = (off & ~127ull) % A; len = 128 * (rnd() % ((A - off) / 128 + 1)); break;  // whole lines
            case 5: len = ~0ull - rnd() % 3; break;          // read to the end
            case 6: off = ~0ull - rnd() % 300; len = rnd(); break;  // offset near 2^64
            default: len = rnd() % (A - off + 1); break;
            }
            v.push_back(rq(ino, off, len));
        }
        check_call(log2_adm, files, v);
        total += n;
    }
    if (failures) {
        fprintf(stderr, "memfs_read_plan: %d checks failed\n", failures);
        return 1;
    }
    printf("memfs_read_plan: ok (%llu random requests)\n", (unsigned long long)total);
    return 0;
}
