// group.hpp — what the replica group's six files share (private to the library):
//   group.cpp              the backend, join / open / close, the replicated round, sync, verify, resync
//   group_partitioned.cpp  key-partitioned rounds (PtMember, PtGroup)
//   group_reads.cpp        group-wide ordered reads of a partitioned skip-list group (SkMember)
//   group_files.cpp        file-partitioned rounds of a file-store group (FpMember)
//   group_file_reads.cpp   the group-wide pread of such a group (PrMember)
//   group_pops.cpp         what a partitioned skip-list group opts into as a whole, and its group-wide pop (PoMember)
// A member's state of a protocol is a struct of that protocol's file, embedded in Member: only the
// owner's file touches its struct (the rule internal.hpp states for HmHost ... MfHost), and
// member_init / member_free call its init / free. The decisions taken from exchanged words are
// group_plan.hpp's, pure host arithmetic.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdio>
#include <vector>

#include "collectives.hpp"
#include "group_plan.hpp"
#include "internal.hpp"

namespace nrg {
namespace grp {

using Rccl = nrg::Collectives;

constexpr int NBUF = 3;  // gathered-log buffers in rotation per member

// A device buffer grown on demand; a reallocation first drains the streams that may use it.
struct DBuf {
    void* p = nullptr;
    uint64_t bytes = 0;
};
inline void free_buf(DBuf& d) {
    if (d.p) (void)hipFree(d.p);
    d = DBuf{};
}

struct Member;

// Partitioned rounds (nrg_group_partitioned_round*): the state of one member.
// A round lives over three calls in the pipelined form (post, stage A, stage B: see pt_post), so its
// partition output and count exchange (PtPar) rotate over PT_DEPTH slots and what the owner
// received and answered (PtRecv) over two.
enum PtBuf { PB_AVAL, PB_AFOUND, PB_APREV, PB_APREVF, PB_ST, PB_ALLST, PB_DESC, PB_N };
enum PtPar { PP_POUT, PP_PPOS, PP_KOUT, PP_GPOS, PP_CNT, PP_ALLCNT, PP_N };
enum PtRecv { PR_RPUT, PR_RKEY, PR_RVAL, PR_RFOUND, PR_RPREV, PR_RPREVF, PR_N };
constexpr int PT_DEPTH = 3;

struct PtMember {
    DBuf pt[PB_N];
    DBuf pp[PT_DEPTH][PP_N];           // by round slot (round % PT_DEPTH)
    DBuf rv[2][PR_N];                  // by round parity
    uint64_t* h_cnt[PT_DEPTH] = {};    // pinned: [nranks][2 * nranks + XW_N] counts, capacities, flags
    hipEvent_t cnt_ev[PT_DEPTH] = {};  // the counts of that slot are in h_cnt
    nrg_round pr[PT_DEPTH] = {};       // the caller's part of the round of that slot
    uint64_t cap_p[PT_DEPTH] = {}, cap_k[PT_DEPTH] = {};  // its owner-region capacities (n, n_gets)
    PtPlan plan[PT_DEPTH];
    uint32_t epoch = 0;            // look-back descriptor tag of the last fused partition
    hipEvent_t pin_ev = nullptr;   // the replica stream's work up to a post (inputs, older rounds)
    uint64_t xwords[8] = {};       // this rank's host words of the exchange
    uint64_t xw1[PT_DEPTH][8] = {};  // a one-rank group: the words of the round of that slot (its
                                     // "exchange" needs no wait: its counts are its own n, n_gets)
    int init(Member& m, int nranks);  // (group_partitioned.cpp)
    void free();
};

// the group's part of them: rounds posted (partition + count exchange), through stage A (payload to
// the owners, replay with its reads deferred), through stage B (answers back, route-back)
struct PtGroup {
    uint64_t posted = 0, a = 0, b = 0;
    bool drop[PT_DEPTH] = {};  // the round failed in stage A (an agreed error): no stage B
};

// Group-wide ordered reads of a partitioned skip-list group (nrg_group_skiplist_seek / _range_count /
// _scan): the padded send copy of this member's queries, every rank's queries, this partition's
// candidates for all of them (keys or counts, values, found; a scan: `limit` keys and values per
// query and a u32 count) and the candidates that came back for its own.
enum SkBuf { SK_SEND, SK_QALL, SK_CK, SK_CV, SK_CF, SK_BK, SK_BV, SK_BF, SK_N };

struct SkMember {
    DBuf b[SK_N];
    void free();  // (group_reads.cpp; nothing to set up at join: the buffers grow with the first read)
};

// The group-wide pop of a partitioned skip-list group (nrg_group_skiplist_pop): the padded send copy of
// this member's requests and every rank's, its candidates (keys, values: cfmax front slots, then cbmax
// back slots), every member's, its part of the plan, and the two records it replays.
enum PoBuf { PO_SEND, PO_ALLREQ, PO_CK, PO_CV, PO_ALLK, PO_ALLV, PO_PLAN, PO_REC, PO_N };

struct PoMember {
    DBuf b[PO_N];
    void free();  // (group_pops.cpp; nothing to set up at join: the buffers grow with the first pop)
};

// File-partitioned rounds of a file-store group (nrg_group_file_round): the state of one member. A
// round is complete, as far as the host goes, when the call returns, so nothing rotates: the stream
// orders a round's use of these buffers after the previous round's.
enum FpBuf {
    FB_OUT,     // its records grouped by owner (the partition's output)
    FB_POS,     // where each of its records went
    FB_CNT,     // its exchange words: records per owner (written by the partition), then FW_*
    FB_ALLCNT,  // every rank's
    FB_RREC,    // the records it received as an owner, in rank order
    FB_RRESP,   // the responses to them
    FB_RSOME,
    FB_ARESP,   // the responses to its own records, in the partition output's order
    FB_ASOME,
    FB_ST,      // the growth-confirm exchange
    FB_ALLST,
    FB_N
};

struct FpMember {
    DBuf b[FB_N];
    uint64_t* h_cnt = nullptr;  // pinned: [nranks][nranks + FW_N], every rank's exchange words
    hipEvent_t cnt_ev = nullptr;  // they are in h_cnt
    FpPlan plan;
    int init(Member& m, int nranks);  // (group_files.cpp)
    void free();
};

// The group-wide pread of a file-partitioned group (nrg_group_memfs_pread): the state of one member. The
// call returns when the answers are in the callers' buffers, so nothing rotates.
enum PrBuf {
    RB_OUT,     // its requests grouped by owner (the partition's output)
    RB_POS,     // where each of its requests went
    RB_CNT,     // its words of the first exchange: requests per owner (written by the partition), then RW_*
    RB_ALLCNT,  // every rank's
    RB_RREQ,    // the requests it received as an owner, in rank order
    RB_ROFFS,   // the scan of their clipped lengths (one more word than requests)
    RB_RCNT,    // their clipped lengths
    RB_RSOME,
    RB_RAGG,    // the scan's tile aggregates
    RB_TOT,     // its words of the second exchange: the bytes it owes each asker, then TW_*
    RB_ALLTOT,  // every rank's
    RB_SDATA,   // its packed answers as an owner, grouped by asker
    RB_ACNT,    // the clipped lengths of its own requests, in the partition output's order
    RB_ASOME,
    RB_RDATA,   // its own answer packed in that order (16-byte aligned, readable to the next multiple of 16)
    RB_SOFFS,   // the re-pack's scratch: where each position's bytes begin in RB_RDATA
    RB_AAGG,    // ... and its scans' tile aggregates
    RB_N
};

struct PrMember {
    DBuf b[RB_N];
    uint64_t* h_cnt = nullptr;  // pinned: [nranks][nranks + RW_N], every rank's words of the first exchange
    uint64_t* h_tot = nullptr;  // pinned: [nranks][nranks + TW_N], of the second
    hipEvent_t ev = nullptr;    // they are there
    FpPlan plan;                // in requests
    PrBytePlan bytes;
    int init(Member& m, int nranks);  // (group_file_reads.cpp)
    void free();
};

struct Member {
    nrg_ctx* ctx = nullptr;
    int rank = 0;
    ncclComm_t comm = nullptr;
    hipStream_t cstream = nullptr;  // library-owned: pad copies + all-gathers
    hipStream_t pstream = nullptr;  // library-owned: a one-rank group's partitions, beside the replay
    hipStream_t in_stream = nullptr;
    bool in_set = false;
    hipEvent_t in_ev = nullptr;
    hipEvent_t ord_ev = nullptr;  // order()
    DBuf gbuf[NBUF];              // the gathered log of a round
    hipEvent_t gathered[NBUF] = {};
    hipEvent_t freed[NBUF] = {};
    bool used[NBUF] = {};
    DBuf sbuf;  // padded send copy when a segment is shorter than the stride
    // Round headers and the words exchange (allocated at join, so a round cannot fail on them):
    //   hdr[b]  {n, fingerprint of seg_lens} sent with round b's segment; ghdr[b] every rank's
    //   wx      this rank's words of a words exchange (gather_words); gwx every rank's
    uint64_t* hdr[NBUF] = {};
    uint64_t* ghdr[NBUF] = {};
    uint64_t* wx = nullptr;
    uint64_t* gwx = nullptr;
    uint64_t* h_gwx = nullptr;  // pinned host copy of gwx
    DBuf snap;                  // nrg_group_resync: the root's snapshot, sent or received
    void* xmem = nullptr;
    PtMember pt;
    SkMember sk;
    FpMember fp;
    PrMember pr;
    PoMember po;
};

}  // namespace grp
}  // namespace nrg

struct nrg_group {
    const nrg::grp::Rccl* R = nullptr;  // RCCL, or the test loopback (fixed at creation)
    int nranks = 0;
    int rank0 = 0;
    bool owns = false;  // replicas opened by nrg_group_open
    std::vector<nrg::grp::Member> m;
    uint64_t round = 0;
    uint32_t timeout_ms = NRG_GROUP_DEFAULT_TIMEOUT_MS;  // deadline of every wait on the peers
    int broken = NRG_OK;  // sticky: a timed-out collective or disagreeing ranks end the group
    nrg::grp::PtGroup pt;
    // what every rank agreed on (nrg_group_skiplist_enable_removal): each member removes with this
    // tombstone, and a partitioned round's Push / Remove responses come from the keys' owners
    bool sl_rm = false;
    uint64_t sl_tomb = 0;
    // ... and nrg_group_skiplist_enable_pops: a round that holds a mark record is refused everywhere,
    // and nrg_group_skiplist_pop pops the union
    bool sl_pops = false;
    uint64_t sl_front = 0, sl_back = 0;
    // the partitioned rounds' own launches (nrg_test_group_launches)
    enum { L_FUSED, L_ROUTE, L_PUSH_RESP, L_MARKS, L_N };
    uint64_t launches[L_N] = {};
    char diag[256] = {};  // what broke it (nrg_group_last_error)
};

namespace nrg {
namespace grp {

inline int hip_rc(hipError_t e) { return e == hipSuccess ? NRG_OK : (e == hipErrorOutOfMemory ? NRG_E_NOMEM : NRG_E_HIP); }

#define GCHK(x)                          \
    do {                                 \
        hipError_t _e = (x);             \
        if (_e != hipSuccess) return nrg::grp::hip_rc(_e); \
    } while (0)

#define RCHK(x)                                   \
    do {                                          \
        int _r = (x);                             \
        if (_r != NRG_OK) return _r;              \
    } while (0)

inline int grow_buf(Member& m, DBuf& d, uint64_t bytes) {
    if (d.bytes >= bytes) return NRG_OK;
    GCHK(hipStreamSynchronize(m.cstream));
    GCHK(hipStreamSynchronize(m.ctx->stream));
    if (m.pstream) GCHK(hipStreamSynchronize(m.pstream));  // a one-rank group's partitions
    if (d.p) GCHK(hipFree(d.p));
    d.p = nullptr;
    d.bytes = 0;
    uint64_t b = bytes < 4096 ? 4096 : bytes + bytes / 4;  // headroom: rounds vary in size
    GCHK(hipMalloc(&d.p, b));
    d.bytes = b;
    return NRG_OK;
}

// `to` waits for the work queued on `from` so far
inline int order(Member& m, hipStream_t from, hipStream_t to) {
    GCHK(hipEventRecord(m.ord_ev, from));
    GCHK(hipStreamWaitEvent(to, m.ord_ev, 0));
    return NRG_OK;
}

inline void* at(void* base, uint64_t off) { return (void*)((char*)base + off); }

constexpr int GRP_TPB = 256;
inline unsigned grp_grid(uint64_t n) {
    const uint64_t b = (n + GRP_TPB - 1) / GRP_TPB;
    return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

// ---- group.cpp ----
// The group cannot go on: remember why, give up on the communicators and return `code`.
int group_fail(nrg_group* g, int code, const char* what);
// ncclGroupEnd under the group's deadline (collective() is its one caller).
int group_end(nrg_group* g, const char* phase);
// Wait until the stream drains (the event completes), at most the group's deadline from now.
int wait_stream(nrg_group* g, hipStream_t s, const char* phase);
int wait_event(nrg_group* g, hipEvent_t ev, const char* phase);
// Words from every rank to the host: the first w (<= 3) words of every rank's Member::wx,
// all-gathered on the comm streams and read back under the group's deadline. Member::h_gwx of every
// local member then holds them in rank order, w per rank (identical on every rank).
int gather_words(nrg_group* g, int w, const char* phase);
// ... of two words per rank that the host knows: wx = {a[i], b[i]} in stream order first
int exchange_pairs(nrg_group* g, const std::vector<uint64_t>& a, const std::vector<uint64_t>& b, const char* phase);
// n Gets of a skip-list replica in slices of at most max_reads
int sl_gets(nrg_ctx* c, const uint64_t* keys, uint64_t n, uint64_t* vals, uint8_t* found);

// ---- group_partitioned.cpp ----
// every posted partitioned round through stage B (nrg_group_sync flushes them first)
int pt_flush_posted(nrg_group* g);
// the checks of every call that needs send / recv
int pt_check(nrg_group* g);
// A one-rank group owns every key, so its partition is the identity and so is the route-back
// (NRG_KNOB_EXP bit 16, measurement, makes it move its data like a multi-rank one).
inline bool pt_ident(const nrg_group* g, const Member& m) { return g->nranks == 1 && !(m.ctx->exp & 0x10000); }

// ---- group_files.cpp ----
// dst[k] = v[k], k < n <= FW_N, in stream order (the words are captured at the launch)
int put_words(hipStream_t s, uint64_t* dst, const uint64_t* v, uint32_t n);

// One collective step: post(member, i) enqueues member i's calls between ncclGroupStart and
// ncclGroupEnd and returns the first refusal. The order is what keeps a peer from hanging: a
// group_start that fails returns NRG_E_COMM with nothing posted (the group is not broken); members
// post while none is refused; group_end ALWAYS follows, under the group's deadline, refused post
// or not, because the peers of what was posted are already waiting for it; only then does a
// refusal end the group.
template <typename Post>  // ncclResult_t post(Member&, int i)
int collective(nrg_group* g, const char* phase, Post post) {
    if (g->R->group_start() != ncclSuccess) return NRG_E_COMM;
    ncclResult_t res = ncclSuccess;
    const int nl = (int)g->m.size();
    for (int i = 0; i < nl && res == ncclSuccess; i++) res = post(g->m[i], i);
    RCHK(group_end(g, phase));
    if (res == ncclSuccess) return NRG_OK;
    char what[192];
    std::snprintf(what, sizeof what, "%s: refused", phase);
    return group_fail(g, NRG_E_COMM, what);
}

}  // namespace grp
}  // namespace nrg
