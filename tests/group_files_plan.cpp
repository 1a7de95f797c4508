// group_files_plan.cpp — what a file-partitioned round decides from its exchanged words
// (node-replication_amd/csrc/group_plan.hpp: fp_agree, fp_plan_for and the byte offsets) without a GPU:
// a stand-alone program, built with the host compiler and -fsanitize=address,undefined and run by
// tests/test_group_files_plan.py. Exit status 0: every check held; else the failed checks are on stderr.
#include <stdint.h>
#include <stdio.h>

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

static uint64_t rng_state = 0xF11E5ull;
static uint64_t rnd() {  // splitmix64, fixed seed
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// the words as include/nrgpu.h lists them, by number (not the header's enum)
enum { CAP = 0, ERR = 1, KIND = 2, FILES = 3, LOG2B = 4, SIZED = 5, RESP = 6, WORDS = 7 };

// An exchanged matrix, written through its own indexing (not the header's accessors): a good round of
// file stores of 16 files of 4096 bytes, unsized, nobody short of room, nobody asking.
struct Mat {
    int G;
    uint64_t cw;
    std::vector<uint64_t> H;
    explicit Mat(int g) : G(g), cw((uint64_t)g + WORDS), H((size_t)g * ((size_t)g + WORDS), 0) {
        for (int s = 0; s < G; s++) word(s, KIND) = NRG_DS_MEMFS, word(s, FILES) = 16, word(s, LOG2B) = 12, word(s, CAP) = ~0ull;
    }
    uint64_t& recs(int s, int o) { return H[(size_t)s * cw + o]; }
    uint64_t& word(int s, int k) { return H[(size_t)s * cw + G + k]; }
    uint64_t recv(int r) { uint64_t t = 0; for (int s = 0; s < G; s++) t += recs(s, r); return t; }
    void fill(uint64_t max) {
        for (int s = 0; s < G; s++) {
            const bool idle = rnd() % 5 == 0;  // ragged: some ranks bring nothing
            for (int o = 0; o < G; o++) recs(s, o) = idle || rnd() % 4 == 0 ? 0 : rnd() % (max + 1);
        }
    }
};

static int rc_of(Mat& M) { return fp_agree(M.H.data(), M.G).rc; }

// every error row, and the first one in rank order wins
static void check_errors(int G) {
    const int codes[] = {NRG_E_INVAL, NRG_E_CAPACITY, NRG_E_NOMEM, NRG_E_HIP};
    Mat ok(G);
    ok.fill(7);
    CHECK(rc_of(ok) == NRG_OK);
    for (int s = 0; s < G; s++)
        for (int code : codes) {
            Mat M = ok;
            M.word(s, ERR) = (uint64_t)(-code);
            CHECK(rc_of(M) == code);
            if (s + 1 < G) {
                M.word(s + 1, ERR) = (uint64_t)(-(code == NRG_E_INVAL ? NRG_E_CAPACITY : NRG_E_INVAL));
                CHECK(rc_of(M) == code);  // rank s is first
                M.word(s, ERR) = 0;
                CHECK(rc_of(M) == (code == NRG_E_INVAL ? NRG_E_CAPACITY : NRG_E_INVAL));
            }
            // an error row beats a kind or geometry mismatch elsewhere: the same answer on every rank
            Mat N = ok;
            N.word(s, ERR) = (uint64_t)(-code);
            N.word((s + 1) % G, KIND) = NRG_DS_HASHMAP;
            CHECK(rc_of(N) == code);
        }
}

// kinds, F, B and the sized flag: every rank a file store, and all the same
static void check_mixed(int G) {
    Mat ok(G);
    ok.fill(3);
    for (int s = 0; s < G; s++) {
        for (uint64_t kind : {(uint64_t)NRG_DS_HASHMAP, (uint64_t)NRG_DS_SKIPLIST, (uint64_t)0}) {
            Mat M = ok;
            M.word(s, KIND) = kind;
            CHECK(rc_of(M) == NRG_E_INVAL);  // (also with one rank: no file store, no file round)
        }
        const int which[] = {FILES, LOG2B, SIZED};
        for (int k : which) {
            Mat M = ok;
            M.word(s, k) += 1;
            CHECK(rc_of(M) == (G == 1 ? NRG_OK : NRG_E_INVAL));
        }
    }
    Mat all(G);  // a whole group of another kind, or all sized: the first is refused, the second is fine
    for (int s = 0; s < G; s++) all.word(s, KIND) = NRG_DS_HASHMAP;
    CHECK(rc_of(all) == NRG_E_INVAL);
    Mat sized(G);
    for (int s = 0; s < G; s++) sized.word(s, SIZED) = 1;
    CHECK(rc_of(sized) == NRG_OK);
}

// any-grow: exactly when some rank receives more than it holds; wants: exactly the ranks that asked
static void check_grow_and_wants(int G) {
    for (int t = 0; t < 20; t++) {
        Mat M(G);
        M.fill(9);
        uint64_t want = 0;
        for (int s = 0; s < G; s++) {
            M.word(s, CAP) = M.recv(s);  // exactly enough
            if (rnd() & 1) M.word(s, RESP) = 1, want |= 1ull << s;
        }
        FpAgree A = fp_agree(M.H.data(), G);
        CHECK(A.rc == NRG_OK && !A.any_grow && A.wants == want);
        for (int s = 0; s < G; s++) {
            if (M.recv(s) == 0) continue;
            Mat N = M;
            N.word(s, CAP) = M.recv(s) - 1;  // one short
            A = fp_agree(N.H.data(), G);
            CHECK(A.rc == NRG_OK && A.any_grow && A.wants == want);
        }
        Mat Z(G);  // nothing anywhere, no room anywhere: nothing to grow
        for (int s = 0; s < G; s++) Z.word(s, CAP) = 0;
        A = fp_agree(Z.H.data(), G);
        CHECK(A.rc == NRG_OK && !A.any_grow && A.wants == 0);
    }
}

// The offsets against a restatement that walks the records one by one: sender s lays its records out by
// owner 0, 1, ... (the compact partition output); receiver r lays what it gets out by sender 0, 1, ...
static void check_offsets(int G) {
    for (int t = 0; t < (G > 8 ? 3 : 20); t++) {
        Mat M(G);
        M.fill(G > 8 ? 3 : 11);
        CHECK(fw_cw(G) == M.cw);
        std::vector<FpPlan> P(G);
        for (int r = 0; r < G; r++) fp_plan_for(M.H.data(), G, r, P[r]);
        for (int s = 0; s < G; s++) {  // the sender's side
            uint64_t at_rec = 0, at_resp = 0, at_some = 0, pos = 0;
            CHECK((int)P[s].to.size() == G && (int)P[s].to_off.size() == G && (int)P[s].from.size() == G &&
                  (int)P[s].from_off.size() == G);
            for (int o = 0; o < G; o++) {
                CHECK(fw_recs(M.H.data(), G, s, o) == M.recs(s, o) && P[s].to[o] == M.recs(s, o) && P[o].from[s] == M.recs(s, o));
                CHECK(P[s].to_off[o] == pos);
                CHECK(fp_rec_at(P[s].to_off[o]) == at_rec && fp_resp_at(P[s].to_off[o]) == at_resp &&
                      fp_some_at(P[s].to_off[o]) == at_some);
                for (uint64_t j = 0; j < M.recs(s, o); j++) pos++, at_rec += 152, at_resp += 136, at_some += 1;
            }
            CHECK(P[s].sent == pos);
        }
        for (int r = 0; r < G; r++) {  // the receiver's side: rank order is the log order
            uint64_t at_rec = 0, at_resp = 0, at_some = 0, pos = 0;
            for (int s = 0; s < G; s++) {
                CHECK(P[r].from_off[s] == pos);
                CHECK(fp_rec_at(P[r].from_off[s]) == at_rec && fp_resp_at(P[r].from_off[s]) == at_resp &&
                      fp_some_at(P[r].from_off[s]) == at_some);
                for (uint64_t j = 0; j < M.recs(s, r); j++) pos++, at_rec += 152, at_resp += 136, at_some += 1;
            }
            CHECK(P[r].recvd == pos && pos == M.recv(r));
        }
        for (int s = 0; s < G; s++)
            for (int k = 0; k < WORDS; k++) CHECK(fw_word(M.H.data(), G, s, (uint64_t)k) == M.word(s, k));
    }
    // counts near 2^32 records: the byte offsets do not wrap
    Mat B(G);
    for (int s = 0; s < G; s++) B.recs(s, 0) = (1ull << 32) - 1;
    FpPlan P;
    fp_plan_for(B.H.data(), G, 0, P);
    CHECK(P.recvd == (uint64_t)G * ((1ull << 32) - 1));
    CHECK(fp_rec_at(P.recvd) == P.recvd * 152 && fp_rec_at(P.recvd) / 152 == P.recvd);
}

int main() {
    static_assert((int)FW_CAP == CAP && (int)FW_ERR == ERR && (int)FW_KIND == KIND && (int)FW_FILES == FILES &&
                      (int)FW_LOG2B == LOG2B && (int)FW_SIZED == SIZED && (int)FW_RESP == RESP && (int)FW_N == WORDS,
                  "the exchange words");
    static_assert(FP_REC_BYTES == 152 && FP_RESP_BYTES == 136, "record sizes");
    const int sizes[] = {1, 2, 3, 8, 64};
    for (int G : sizes) {
        check_errors(G);
        check_mixed(G);
        check_grow_and_wants(G);
        check_offsets(G);
    }
    if (failures) {
        fprintf(stderr, "group_files_plan: %d checks failed\n", failures);
        return 1;
    }
    printf("group_files_plan: ok\n");
    return 0;
}
