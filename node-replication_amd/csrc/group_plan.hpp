// group_plan.hpp — what a replica group decides from the words its ranks exchanged, as pure host
// arithmetic: no HIP header and no RCCL header, so tests/group_plan.cpp checks it without a GPU.
// Every rank runs these on the same exchanged words and so reaches the same code, the same plan and
// the same byte offsets before any payload moves; group.cpp, group_partitioned.cpp, group_reads.cpp,
// group_files.cpp and group_file_reads.cpp do the waiting, the collectives and the launches around
// them (tests/group_files_plan.cpp checks the file-partitioned part, tests/group_pread_plan.cpp the
// group-wide pread's).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/nrgpu.h"

namespace nrg {
namespace grp {

// ---- replicated rounds (group.cpp) ----------------------------------------------------------------

// the splitmix64 finaliser (common.hpp mix64, which needs the HIP header for its qualifiers)
inline uint64_t plan_mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// fingerprint of a round's segment lengths (every rank must pass the same ones)
inline uint64_t lens_fp(const std::vector<uint64_t>& lens) {
    uint64_t h = 0x9E3779B97F4A7C15ull ^ lens.size();
    for (uint64_t l : lens) h = plan_mix64(h ^ l) + 0x632BE59BD9B4E019ull;
    return h;
}

// the common stride of a round's segments: the longest
inline uint64_t lens_stride(const std::vector<uint64_t>& lens) {
    uint64_t stride = 0;
    for (uint64_t l : lens) stride = l > stride ? l : stride;
    return stride;
}

// ---- partitioned rounds (group_partitioned.cpp) ---------------------------------------------------

// Exchange words per rank (u64) of a partitioned round: [0, G) Puts per owner, [G, 2G) Gets per
// owner, then
enum : uint64_t {
    XW_PREV = 0,    // 1 when this rank wants its Puts' previous values
    XW_RP_CAP = 1,  // received Puts its buffers hold now
    XW_RK_CAP = 2,  // received Get keys its buffers hold now
    XW_ERR = 3,     // -NRG_E_* of a local failure before the exchange, else 0
    XW_KIND = 4,    // the member's data structure (NRG_DS_*): every rank's must be the same
    XW_N = 5,
};

// The exchanged matrix H holds G rows of xw_cw(G) words, in rank order.
inline uint64_t xw_cw(int G) { return 2 * (uint64_t)G + XW_N; }
inline uint64_t xw_puts(const uint64_t* H, int G, int s, int o) { return H[(size_t)s * xw_cw(G) + o]; }      // s -> owner o
inline uint64_t xw_gets(const uint64_t* H, int G, int s, int o) { return H[(size_t)s * xw_cw(G) + G + o]; }
inline uint64_t xw_word(const uint64_t* H, int G, int s, uint64_t k) { return H[(size_t)s * xw_cw(G) + 2 * G + k]; }

// What every rank concludes from H before any payload moves.
struct PlanAgree {
    int rc = NRG_OK;     // the code every rank returns: the first XW_ERR in rank order, or mixed kinds
    uint64_t kind = 0;   // the group's kind (rc == NRG_OK)
    bool any_prev = false;  // some rank wants previous values
    bool any_grow = false;  // some rank receives more than its buffers hold: all confirm the growth
};

inline PlanAgree plan_agree(const uint64_t* H, int G) {
    PlanAgree A;
    for (int s = 0; s < G; s++)
        if (xw_word(H, G, s, XW_ERR)) {
            A.rc = -(int)xw_word(H, G, s, XW_ERR);  // the same answer on every rank
            return A;
        }
    for (int s = 1; s < G; s++)
        if (xw_word(H, G, s, XW_KIND) != xw_word(H, G, 0, XW_KIND)) {
            A.rc = NRG_E_INVAL;  // hashmap and skip-list ranks in one group
            return A;
        }
    A.kind = xw_word(H, G, 0, XW_KIND);
    for (int s = 0; s < G; s++) {
        A.any_prev |= xw_word(H, G, s, XW_PREV) != 0;
        uint64_t rp = 0, rk = 0;  // what rank s receives
        for (int o = 0; o < G; o++) {
            rp += xw_puts(H, G, o, s);
            rk += xw_gets(H, G, o, s);
        }
        A.any_grow |= rp > xw_word(H, G, s, XW_RP_CAP) || rk > xw_word(H, G, s, XW_RK_CAP);
    }
    return A;
}

// A round's send/recv plan of one rank (stage A), kept for its answers (stage B): the rank sends its
// owner-o region to o and receives rank s's group for it at offset sum_{s' < s} (rank order = the
// global log order).
struct PtPlan {
    std::vector<uint64_t> pto, gto, pfrom, gfrom, pfrom_off, gfrom_off;
    uint64_t rp = 0, rk = 0;  // received Puts and Get keys in all
    uint64_t sp = 0, sk = 0;  // sent in all: the rank's own n and n_gets, if its partition agrees
};

inline void plan_for(const uint64_t* H, int G, int r, PtPlan& P) {
    P.pto.assign(G, 0), P.gto.assign(G, 0), P.pfrom.assign(G, 0), P.gfrom.assign(G, 0);
    P.pfrom_off.assign(G, 0), P.gfrom_off.assign(G, 0);
    uint64_t a = 0, b = 0, cq = 0, d = 0;
    for (int o = 0; o < G; o++) {
        P.pto[o] = xw_puts(H, G, r, o);
        P.gto[o] = xw_gets(H, G, r, o);
        P.pfrom[o] = xw_puts(H, G, o, r);
        P.gfrom[o] = xw_gets(H, G, o, r);
        a += P.pto[o], b += P.gto[o];
        P.pfrom_off[o] = cq, cq += P.pfrom[o];
        P.gfrom_off[o] = d, d += P.gfrom[o];
    }
    P.sp = a;
    P.sk = b;
    P.rp = cq;
    P.rk = d;
}

// What a group opts into as a whole (nrg_group_skiplist_enable_removal): H holds {value, -NRG_E_* of
// the rank's local check, or 0} of every rank. The first local error in rank order wins; ranks that
// passed different values are NRG_E_INVAL. Nothing is enabled anywhere unless this is NRG_OK.
inline int optin_agree(const uint64_t* H, int G) {
    for (int r = 0; r < G; r++)
        if (H[2 * r + 1]) return -(int)H[2 * r + 1];
    for (int r = 1; r < G; r++)
        if (H[2 * r] != H[0]) return NRG_E_INVAL;
    return NRG_OK;
}

constexpr uint64_t GC_FROM_HEAD = 32 * 256;  // nr/src/log.rs:36 (the ring keeps this much free)

// The most Puts an owner replays in one call: its max_batch, within what the log's ring takes.
inline uint64_t replay_chunk(uint64_t log_size, uint64_t max_batch) {
    const uint64_t ring_room = log_size > 2 * GC_FROM_HEAD ? log_size - GC_FROM_HEAD : GC_FROM_HEAD;
    return std::max<uint64_t>(1, std::min<uint64_t>(max_batch, ring_room));
}

// ---- file-partitioned rounds of a file-store group (group_files.cpp) ------------------------------

// Exchange words per rank (u64) of a file-partitioned round: [0, G) records per owner, then
enum : uint64_t {
    FW_CAP = 0,    // received records its buffers hold now
    FW_ERR = 1,    // -NRG_E_* of a local failure before the exchange, else 0
    FW_KIND = 2,   // the member's data structure (NRG_DS_*): every rank's must be NRG_DS_MEMFS
    FW_FILES = 3,  // its F
    FW_LOG2B = 4,  // its log2 B
    FW_SIZED = 5,  // 1 when nrg_memfs_enable_sizes is on
    FW_RESP = 6,   // 1 when this rank wants its responses
    FW_N = 7,
};

// The exchanged matrix H holds G rows of fw_cw(G) words, in rank order.
inline uint64_t fw_cw(int G) { return (uint64_t)G + FW_N; }
inline uint64_t fw_recs(const uint64_t* H, int G, int s, int o) { return H[(size_t)s * fw_cw(G) + o]; }  // s -> owner o
inline uint64_t fw_word(const uint64_t* H, int G, int s, uint64_t k) { return H[(size_t)s * fw_cw(G) + G + k]; }

// What every rank concludes from H before any payload moves.
struct FpAgree {
    int rc = NRG_OK;        // the code every rank returns: the first FW_ERR in rank order, a rank that is no
                            // file store, or ranks whose geometry or sized flags differ
    bool any_grow = false;  // some rank receives more than its buffers hold: all confirm the growth
    uint64_t wants = 0;     // bit s: rank s wants its responses (G <= NRG_MAX_PARTS = 64)
};

inline FpAgree fp_agree(const uint64_t* H, int G) {
    FpAgree A;
    for (int s = 0; s < G; s++)
        if (fw_word(H, G, s, FW_ERR)) {
            A.rc = -(int)fw_word(H, G, s, FW_ERR);  // the same answer on every rank
            return A;
        }
    for (int s = 0; s < G; s++) {
        bool same = fw_word(H, G, s, FW_KIND) == NRG_DS_MEMFS;
        for (uint64_t k : {FW_FILES, FW_LOG2B, FW_SIZED}) same = same && fw_word(H, G, s, k) == fw_word(H, G, 0, k);
        if (!same) {
            A.rc = NRG_E_INVAL;
            return A;
        }
    }
    for (int s = 0; s < G; s++) {
        if (fw_word(H, G, s, FW_RESP)) A.wants |= 1ull << s;
        uint64_t r = 0;  // what rank s receives
        for (int o = 0; o < G; o++) r += fw_recs(H, G, o, s);
        A.any_grow |= r > fw_word(H, G, s, FW_CAP);
    }
    return A;
}

// A round's send / recv plan of one rank, every count and offset in records. The rank's partition
// output is compact: owner o's group starts at to_off[o] = sum of to[o'], o' < o, and so do the
// answers that come back for it. What it receives from rank s lies at from_off[s] = sum of
// from[s'], s' < s: rank order, which is the global log order.
struct FpPlan {
    std::vector<uint64_t> to, to_off, from, from_off;
    uint64_t sent = 0, recvd = 0;  // in all: sent is the rank's own n, if its partition agrees
};

inline void fp_plan_for(const uint64_t* H, int G, int r, FpPlan& P) {
    P.to.assign(G, 0), P.to_off.assign(G, 0), P.from.assign(G, 0), P.from_off.assign(G, 0);
    uint64_t a = 0, b = 0;
    for (int o = 0; o < G; o++) {
        P.to[o] = fw_recs(H, G, r, o);
        P.from[o] = fw_recs(H, G, o, r);
        P.to_off[o] = a, a += P.to[o];
        P.from_off[o] = b, b += P.from[o];
    }
    P.sent = a;
    P.recvd = b;
}

// byte offsets of a record, a response and a some byte at a position of the plan
constexpr uint64_t FP_REC_BYTES = sizeof(nrg_memfs_op), FP_RESP_BYTES = sizeof(nrg_memfs_resp);
static_assert(FP_REC_BYTES == 152 && FP_RESP_BYTES == 136, "file store record layout");
inline uint64_t fp_rec_at(uint64_t records) { return records * FP_REC_BYTES; }
inline uint64_t fp_resp_at(uint64_t records) { return records * FP_RESP_BYTES; }
inline uint64_t fp_some_at(uint64_t records) { return records; }

// ---- group-wide pread of a file-partitioned group (group_file_reads.cpp) --------------------------

// Exchange words per rank (u64) of the read's first exchange: [0, G) requests per owner, then
enum : uint64_t {
    RW_CAP = 0,    // received requests its buffers hold now
    RW_ERR = 1,    // -NRG_E_* of a local failure before the exchange, else 0
    RW_KIND = 2,   // the member's data structure (NRG_DS_*): every rank's must be NRG_DS_MEMFS
    RW_FILES = 3,  // its F
    RW_LOG2B = 4,  // its log2 B
    RW_SIZED = 5,  // 1 when nrg_memfs_enable_sizes is on
    RW_DCAP = 6,   // the bytes its caller's data buffer holds (nrg_pread::cap)
    RW_N = 7,
};
// A row has the file round's layout (fw_cw words, the per-owner counts first), so fp_plan_for plans
// the requests' way to their owners and the counts' way back: FpPlan in requests.
static_assert((uint64_t)RW_N == (uint64_t)FW_N, "a read's exchange row is laid out as a file round's");
inline uint64_t rw_cw(int G) { return fw_cw(G); }
inline uint64_t rw_reqs(const uint64_t* H, int G, int s, int o) { return fw_recs(H, G, s, o); }  // s -> owner o
inline uint64_t rw_word(const uint64_t* H, int G, int s, uint64_t k) { return fw_word(H, G, s, k); }

// What every rank concludes from H before any request moves.
struct PrAgree {
    int rc = NRG_OK;        // the first RW_ERR in rank order, or ranks whose geometry or sized flags differ
    bool any_grow = false;  // some owner receives more requests than its buffers hold: all confirm the growth
    uint64_t asked = 0;     // requests of all ranks (0: nothing to answer)
};

inline PrAgree pr_agree(const uint64_t* H, int G) {
    PrAgree A;
    for (int s = 0; s < G; s++)
        if (rw_word(H, G, s, RW_ERR)) {
            A.rc = -(int)rw_word(H, G, s, RW_ERR);  // the same answer on every rank
            return A;
        }
    for (int s = 0; s < G; s++) {
        bool same = rw_word(H, G, s, RW_KIND) == NRG_DS_MEMFS;
        for (uint64_t k : {RW_FILES, RW_LOG2B, RW_SIZED}) same = same && rw_word(H, G, s, k) == rw_word(H, G, 0, k);
        if (!same) {
            A.rc = NRG_E_INVAL;
            return A;
        }
    }
    for (int s = 0; s < G; s++) {
        uint64_t r = 0;  // what owner s receives
        for (int o = 0; o < G; o++) r += rw_reqs(H, G, o, s);
        A.any_grow |= r > rw_word(H, G, s, RW_CAP);
        A.asked += r;
    }
    return A;
}

// Words per rank (u64) of the second exchange: [0, G) T[o][s], the bytes owner o answers asker s with, then
enum : uint64_t {
    TW_SCAP = 0,  // the bytes its packed send buffer holds now
    TW_RCAP = 1,  // the bytes its receive buffer holds now
    TW_N = 2,
};
inline uint64_t tw_cw(int G) { return (uint64_t)G + TW_N; }
inline uint64_t tw_bytes(const uint64_t* T, int G, int o, int s) { return T[(size_t)o * tw_cw(G) + s]; }  // owner o -> s
inline uint64_t tw_word(const uint64_t* T, int G, int o, uint64_t k) { return T[(size_t)o * tw_cw(G) + G + k]; }

// The re-pack's wide path reads the aligned 16-byte blocks around a source byte: a receive buffer of
// `bytes` answer bytes is readable up to the next multiple of 16.
inline uint64_t pr_recv_room(uint64_t bytes) { return (bytes + 15) / 16 * 16; }

// An asker's answer in bytes: column s of T. (A count is at most B <= 2^26 and a rank asks fewer than
// 2^32 requests: no sum wraps.)
inline uint64_t pr_answer_bytes(const uint64_t* T, int G, int s) {
    uint64_t t = 0;
    for (int o = 0; o < G; o++) t += tw_bytes(T, G, o, s);
    return t;
}

// What every rank concludes from both exchanges before any data byte moves.
struct PrBytes {
    int rc = NRG_OK;        // NRG_E_CAPACITY: some rank's answer exceeds its RW_DCAP
    bool any_grow = false;  // some rank's send or receive buffer has to grow: all confirm the growth
};

inline PrBytes pr_bytes_agree(const uint64_t* H, const uint64_t* T, int G) {
    PrBytes B;
    for (int s = 0; s < G; s++) {
        const uint64_t answer = pr_answer_bytes(T, G, s);
        if (answer > rw_word(H, G, s, RW_DCAP)) B.rc = NRG_E_CAPACITY;
        uint64_t packed = 0;  // what s sends as an owner: row s
        for (int a = 0; a < G; a++) packed += tw_bytes(T, G, s, a);
        B.any_grow |= packed > tw_word(T, G, s, TW_SCAP) || pr_recv_room(answer) > tw_word(T, G, s, TW_RCAP);
    }
    return B;
}

// The data's send / recv plan of one rank, in bytes. As an owner its packed answers lie grouped by
// asker in rank order: asker s's at to_off[s], a prefix of row T[r][.]. As an asker it receives owner
// o's bytes at from_off[o], a prefix of column T[.][r]: its answer packed in partition order.
struct PrBytePlan {
    std::vector<uint64_t> to, to_off, from, from_off;
    uint64_t sent = 0, recvd = 0;
};

inline void pr_byte_plan_for(const uint64_t* T, int G, int r, PrBytePlan& P) {
    P.to.assign(G, 0), P.to_off.assign(G, 0), P.from.assign(G, 0), P.from_off.assign(G, 0);
    uint64_t a = 0, b = 0;
    for (int o = 0; o < G; o++) {
        P.to[o] = tw_bytes(T, G, r, o);
        P.from[o] = tw_bytes(T, G, o, r);
        P.to_off[o] = a, a += P.to[o];
        P.from_off[o] = b, b += P.from[o];
    }
    P.sent = a;
    P.recvd = b;
}

constexpr uint64_t PR_REQ_BYTES = sizeof(nrg_memfs_rd);
static_assert(PR_REQ_BYTES == 24, "file store request layout");

// ---- group-wide skip-list reads (group_reads.cpp) -------------------------------------------------

constexpr uint64_t SK_SCAN_MAX_SLOTS = 1ull << 27;  // G * nmax * limit of a scan (include/nrgpu.h)

// A rank's flags word of the {n, flags} exchange: its bad arguments, the seek mode, a scan's limit
// (1 .. 1024) in bits 16..26 (a seek and a range count leave them zero) and its kind.
inline uint64_t sk_flags(bool bad, bool count, uint32_t mode, bool scan, uint32_t limit, uint32_t kind) {
    return (bad ? 1 : 0) | ((uint64_t)(count ? 0 : mode) << 8) | ((uint64_t)(scan ? limit & 0x7FFu : 0) << 16) |
           ((uint64_t)kind << 40);
}

// H: {n, flags} of every rank. No rank's arguments are bad and every rank's flags are the same.
inline int sk_flags_agree(const uint64_t* H, int G) {
    for (int r = 0; r < G; r++)
        if ((H[2 * r + 1] & 1) || H[2 * r + 1] != H[1]) return NRG_E_INVAL;
    return NRG_OK;
}

// a scan's candidate scratch (nmax < 2^32, G <= 64 and limit <= 1024: the product cannot wrap)
inline bool sk_scan_fits(int G, uint64_t nmax, uint32_t limit) { return (uint64_t)G * nmax * limit <= SK_SCAN_MAX_SLOTS; }

// the lane group of a scan's query: the power of two at or above its G * limit candidate slots, up to a wave
inline uint32_t scan_lane_log2(int G, uint32_t limit) {
    uint32_t lw = 0;
    while (lw < 6 && (1ull << lw) < (uint64_t)G * limit) lw++;
    return lw;
}

}  // namespace grp
}  // namespace nrg
