// group_pread_plan.cpp — what the group-wide pread of a file-partitioned group decides from its two
// exchanges (node-replication_amd/csrc/group_plan.hpp: pr_agree, fp_plan_for on its rows, pr_bytes_agree,
// pr_byte_plan_for, pr_recv_room) without a GPU: a stand-alone program, built with the host compiler and
// -fsanitize=address,undefined and run by tests/test_group_pread_plan.py. Exit status 0: every check
// held; else the failed checks are on stderr.
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

static uint64_t rng_state = 0x9EADull;
static uint64_t rnd() {  // splitmix64, fixed seed
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// the words as include/nrgpu.h lists them, by number (not the header's enums)
enum { CAP = 0, ERR = 1, KIND = 2, FILES = 3, LOG2B = 4, SIZED = 5, DCAP = 6, WORDS = 7 };
enum { SCAP = 0, RCAP = 1, TWORDS = 2 };

// The first exchange, written through its own indexing: file stores of 16 files of 4096 bytes, unsized,
// nobody short of room, every data buffer as large as can be.
struct Mat {
    int G;
    uint64_t cw;
    std::vector<uint64_t> H;
    explicit Mat(int g) : G(g), cw((uint64_t)g + WORDS), H((size_t)g * ((size_t)g + WORDS), 0) {
        for (int s = 0; s < G; s++)
            word(s, KIND) = NRG_DS_MEMFS, word(s, FILES) = 16, word(s, LOG2B) = 12, word(s, CAP) = ~0ull, word(s, DCAP) = ~0ull;
    }
    uint64_t& reqs(int s, int o) { return H[(size_t)s * cw + o]; }
    uint64_t& word(int s, int k) { return H[(size_t)s * cw + G + k]; }
    void fill(uint64_t max, int idle_rank, int dry_owner) {  // an idle rank asks nothing; a dry owner gets nothing
        for (int s = 0; s < G; s++)
            for (int o = 0; o < G; o++) reqs(s, o) = s == idle_rank || o == dry_owner || rnd() % 4 == 0 ? 0 : rnd() % (max + 1);
    }
};

// The second exchange: T[o][s] bytes, every buffer as large as can be.
struct Tot {
    int G;
    uint64_t cw;
    std::vector<uint64_t> T;
    explicit Tot(int g) : G(g), cw((uint64_t)g + TWORDS), T((size_t)g * ((size_t)g + TWORDS), 0) {
        for (int o = 0; o < G; o++) word(o, SCAP) = ~0ull, word(o, RCAP) = ~0ull;
    }
    uint64_t& bytes(int o, int s) { return T[(size_t)o * cw + s]; }
    uint64_t& word(int o, int k) { return T[(size_t)o * cw + G + k]; }
    uint64_t answer(int s) { uint64_t t = 0; for (int o = 0; o < G; o++) t += bytes(o, s); return t; }
    uint64_t packed(int o) { uint64_t t = 0; for (int s = 0; s < G; s++) t += bytes(o, s); return t; }
};

static int rc_of(Mat& M) { return pr_agree(M.H.data(), M.G).rc; }

// every error row, and the first one in rank order wins
static void check_errors(int G) {
    const int codes[] = {NRG_E_INVAL, NRG_E_NOT_SYNCED, NRG_E_CAPACITY, NRG_E_NOMEM};
    Mat ok(G);
    ok.fill(9, -1, -1);
    CHECK(rc_of(ok) == NRG_OK);
    for (int s = 0; s < G; s++)
        for (int code : codes) {
            const int other = code == NRG_E_INVAL ? NRG_E_NOT_SYNCED : NRG_E_INVAL;
            Mat M = ok;
            M.word(s, ERR) = (uint64_t)(-code);
            CHECK(rc_of(M) == code);
            if (s + 1 < G) {
                M.word(s + 1, ERR) = (uint64_t)(-other);
                CHECK(rc_of(M) == code);  // rank s is first
                M.word(s, ERR) = 0;
                CHECK(rc_of(M) == other);
            }
            Mat N = ok;  // an error row beats a geometry mismatch elsewhere: the same answer on every rank
            N.word(s, ERR) = (uint64_t)(-code);
            N.word((s + 1) % G, FILES) = 17;
            CHECK(rc_of(N) == code);
        }
    // a member that is no file store (even when every member is the same other kind); differing F, B, sized
    for (int s = 0; s < G; s++) {
        Mat M = ok;
        M.word(s, KIND) = NRG_DS_SKIPLIST;
        CHECK(rc_of(M) == NRG_E_INVAL);
        for (int k : {FILES, LOG2B, SIZED}) {
            Mat N = ok;
            N.word(s, k) += 1;
            CHECK(rc_of(N) == (G == 1 ? NRG_OK : NRG_E_INVAL));  // (one rank agrees with itself)
        }
    }
    Mat all(G);
    for (int s = 0; s < G; s++) all.word(s, KIND) = NRG_DS_HASHMAP;
    CHECK(rc_of(all) == NRG_E_INVAL);
    Mat sized(G);
    for (int s = 0; s < G; s++) sized.word(s, SIZED) = 1;
    CHECK(rc_of(sized) == NRG_OK);
}

// the requests' plan against a walk of the requests one by one, any-grow and the asked count
static void check_request_plan(int G, int idle_rank, int dry_owner) {
    Mat M(G);
    M.fill(5, idle_rank, dry_owner);
    // every request of every rank, in rank order then owner order (the partition's output)
    std::vector<std::vector<int>> held(G);  // held[o]: the askers of what owner o holds, in arrival order
    uint64_t asked = 0;
    for (int s = 0; s < G; s++)
        for (int o = 0; o < G; o++)
            for (uint64_t k = 0; k < M.reqs(s, o); k++) held[o].push_back(s), asked++;
    const PrAgree A = pr_agree(M.H.data(), G);
    CHECK(A.rc == NRG_OK && !A.any_grow && A.asked == asked);
    for (int r = 0; r < G; r++) {
        FpPlan P;
        fp_plan_for(M.H.data(), G, r, P);
        CHECK(P.recvd == held[r].size());
        uint64_t sent = 0;
        for (int o = 0; o < G; o++) {
            CHECK(P.to_off[o] == sent && P.to[o] == M.reqs(r, o));
            sent += M.reqs(r, o);
            // what r holds of asker o is one run at from_off[o]
            for (uint64_t k = 0; k < P.from[o]; k++) CHECK(held[r][P.from_off[o] + k] == o);
        }
        CHECK(P.sent == sent);
        if (r == idle_rank) CHECK(P.sent == 0);
        if (r == dry_owner) CHECK(P.recvd == 0);
        // any-grow at exactly one request past the capacity
        Mat N = M;
        N.word(r, CAP) = held[r].size();
        CHECK(!pr_agree(N.H.data(), G).any_grow);
        if (!held[r].empty()) {
            N.word(r, CAP) = held[r].size() - 1;
            CHECK(pr_agree(N.H.data(), G).any_grow);
        }
    }
    Mat Z(G);  // nobody asks
    CHECK(pr_agree(Z.H.data(), G).asked == 0 && pr_agree(Z.H.data(), G).rc == NRG_OK);
}

// the bytes' plan against a walk of the bytes one by one; the capacity decision at total = cap and
// cap + 1; any-grow of the send and of the padded receive buffer
static void check_byte_plan(int G, int idle_rank, int dry_owner) {
    Mat M(G);
    Tot T(G);
    for (int o = 0; o < G; o++)
        for (int s = 0; s < G; s++) T.bytes(o, s) = s == idle_rank || o == dry_owner || rnd() % 3 == 0 ? 0 : rnd() % 40;
    CHECK(pr_bytes_agree(M.H.data(), T.T.data(), G).rc == NRG_OK && !pr_bytes_agree(M.H.data(), T.T.data(), G).any_grow);
    // every byte: sendbuf[o] holds (asker) per byte in asker order; recvbuf[s] holds (owner) per byte
    for (int r = 0; r < G; r++) {
        PrBytePlan P;
        pr_byte_plan_for(T.T.data(), G, r, P);
        std::vector<int> sendbuf, recvbuf;
        for (int s = 0; s < G; s++)
            for (uint64_t k = 0; k < T.bytes(r, s); k++) sendbuf.push_back(s);
        for (int o = 0; o < G; o++)
            for (uint64_t k = 0; k < T.bytes(o, r); k++) recvbuf.push_back(o);
        CHECK(P.sent == sendbuf.size() && P.recvd == recvbuf.size());
        CHECK(P.sent == T.packed(r) && P.recvd == T.answer(r) && pr_answer_bytes(T.T.data(), G, r) == T.answer(r));
        for (int o = 0; o < G; o++) {
            CHECK(P.to[o] == T.bytes(r, o) && P.from[o] == T.bytes(o, r));
            for (uint64_t k = 0; k < P.to[o]; k++) CHECK(sendbuf[P.to_off[o] + k] == o);
            for (uint64_t k = 0; k < P.from[o]; k++) CHECK(recvbuf[P.from_off[o] + k] == o);
        }
        if (r == idle_rank) CHECK(P.recvd == 0);
        if (r == dry_owner) CHECK(P.sent == 0);
        // capacity: a total equal to the rank's cap passes, one byte more fails on every rank
        Mat N = M;
        N.word(r, DCAP) = T.answer(r);
        CHECK(pr_bytes_agree(N.H.data(), T.T.data(), G).rc == NRG_OK);
        if (T.answer(r)) {
            N.word(r, DCAP) = T.answer(r) - 1;
            CHECK(pr_bytes_agree(N.H.data(), T.T.data(), G).rc == NRG_E_CAPACITY);
        }
        Mat S = M;  // the sizing call: cap = 0 everywhere fails exactly when somebody's answer has bytes
        bool any = false;
        for (int s = 0; s < G; s++) S.word(s, DCAP) = 0, any |= T.answer(s) != 0;
        CHECK(pr_bytes_agree(S.H.data(), T.T.data(), G).rc == (any ? NRG_E_CAPACITY : NRG_OK));
        // any-grow: the send buffer at its exact size, the receive buffer at its padded size
        Tot U = T;
        U.word(r, SCAP) = T.packed(r);
        U.word(r, RCAP) = (T.answer(r) + 15) / 16 * 16;
        CHECK(!pr_bytes_agree(M.H.data(), U.T.data(), G).any_grow);
        if (T.packed(r)) {
            U.word(r, SCAP) = T.packed(r) - 1;
            CHECK(pr_bytes_agree(M.H.data(), U.T.data(), G).any_grow);
            U.word(r, SCAP) = T.packed(r);
        }
        if (T.answer(r)) {
            U.word(r, RCAP) = (T.answer(r) + 15) / 16 * 16 - 1;
            CHECK(pr_bytes_agree(M.H.data(), U.T.data(), G).any_grow);
        }
    }
}

int main() {
    CHECK(pr_recv_room(0) == 0 && pr_recv_room(1) == 16 && pr_recv_room(16) == 16 && pr_recv_room(17) == 32);
    CHECK(rw_cw(3) == 10 && tw_cw(3) == 5 && PR_REQ_BYTES == 24);
    for (int G : {1, 2, 3, 8, 64}) {
        check_errors(G);
        for (int rep = 0; rep < 4; rep++) {
            const int idle = rep & 1 ? (int)(rnd() % G) : -1, dry = rep & 2 ? (int)(rnd() % G) : -1;
            check_request_plan(G, idle, dry);
            check_byte_plan(G, idle, dry);
        }
    }
    if (failures) {
        fprintf(stderr, "group_pread_plan: %d checks failed\n", failures);
        return 1;
    }
    printf("group_pread_plan: ok\n");
    return 0;
}
