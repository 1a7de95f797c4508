// memfs_plan.hpp — the cut of the file store's writes of any length (nrg_memfs_pwrite*, include/nrgpu.h)
// into 128-byte log records, as pure arithmetic: no HIP header, so tests/memfs_plan.cpp checks it
// without a GPU. The host plans a call with plan() before anything is queued (T, the records of the
// call, moves the log's tail, which is host state); memfs.hip's mf_frag kernel builds fragment t of the
// call with the same cut_of() and frag_of(), compiled for the device. Log content is observable
// (nrg_test_ring_read), so the cut is specified in nrgpu.h and both sides follow it from here.
// The read-shaped cut of the logged reads of any length (nrg_memfs_pread_logged*: rcut_of, rfrag_of,
// rfrag_pos, rfrag_at, read_plan) follows the writes', shared with mf_rfrag / mf_rgather / mf_rcount the
// same way and checked by tests/memfs_read_plan.cpp.
// The arithmetic of capacity growth (what a record needs, the capacity that holds it) is at the end,
// shared the same way and checked by tests/memfs_grow_policy.cpp.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/nrgpu.h"

#if defined(__HIPCC__)
#define NRG_MFP_HD __host__ __device__
#else
#define NRG_MFP_HD
#endif

namespace nrg {
namespace mfp {

constexpr uint32_t LINE_LOG2 = 7;  // a record carries at most one 128-byte line
constexpr uint64_t LINE = 1ull << LINE_LOG2;
// what nrg_open accepts of a file store (memfs.hip mf_open)
constexpr uint32_t LOG2_MIN = 7, LOG2_MAX = 26;
constexpr uint64_t MAX_FILES = 1ull << 16, MAX_BYTES = 1ull << 29;

inline bool geometry_ok(uint32_t log2_b, uint64_t files) {
    return log2_b >= LOG2_MIN && log2_b <= LOG2_MAX && files >= 1 && files <= MAX_FILES &&
           (files << log2_b) <= MAX_BYTES;
}

// What request r comes to: its records, its answer, and whether its records carry bytes of `data`.
struct Cut {
    uint64_t frags;    // f_i >= 1
    uint64_t written;  // len, or the error
    uint8_t some;
    uint8_t kind;      // CUT_*
};
enum : uint8_t { CUT_ENOENT = 0, CUT_EFBIG = 1, CUT_EMPTY = 2, CUT_BYTES = 3 };

// checked in the order the replay checks a record: the ino, then the Write's range (no overflow: len
// may be 2^64 - 1)
NRG_MFP_HD inline Cut cut_of(uint32_t log2_b, uint64_t files, uint64_t ino, uint64_t offset, uint64_t len) {
    const uint64_t B = 1ull << log2_b;
    if (ino < NRG_MEMFS_FIRST_INO || ino - NRG_MEMFS_FIRST_INO >= files) return Cut{1, NRG_MEMFS_ENOENT, 0, CUT_ENOENT};
    if (!(offset <= B && len <= B - offset)) return Cut{1, NRG_MEMFS_EFBIG, 0, CUT_EFBIG};
    if (len == 0) return Cut{1, 0, 1, CUT_EMPTY};
    return Cut{((offset + len - 1) >> LINE_LOG2) - (offset >> LINE_LOG2) + 1, len, 1, CUT_BYTES};
}

// Record k (< frags) of a request of kind `kind`: the record's offset and len, and where its len data
// bytes start in the request's bytes (*src, from data_off; only a CUT_BYTES record has any).
NRG_MFP_HD inline void frag_of(uint32_t log2_b, uint8_t kind, uint64_t offset, uint64_t len, uint64_t k, uint64_t* rec_off,
                               uint32_t* rec_len, uint64_t* src) {
    *src = 0;
    if (kind == CUT_EFBIG) {  // a Write the replay answers with EFBIG whatever the request's numbers were
        *rec_off = 1ull << log2_b, *rec_len = 1;
    } else if (kind != CUT_BYTES) {
        *rec_off = offset, *rec_len = 0;
    } else {
        const uint64_t line = (offset >> LINE_LOG2) + k;
        const uint64_t ls = line << LINE_LOG2;
        const uint64_t lo = ls > offset ? ls : offset;
        const uint64_t end = offset + len, le = (line + 1) << LINE_LOG2;
        const uint64_t hi = le < end ? le : end;
        *rec_off = lo, *rec_len = (uint32_t)(hi - lo), *src = lo - offset;
    }
}

// nrg_memfs_pwrite_plan. first: n + 1 words; written, some: n each or NULL.
inline int plan(uint32_t log2_b, uint64_t files, const nrg_memfs_wr* reqs, uint64_t n, uint64_t data_bytes,
                uint64_t* first, uint64_t* written, uint8_t* some) {
    if (!geometry_ok(log2_b, files)) return NRG_E_INVAL;
    if (n && (!reqs || !first)) return NRG_E_INVAL;
    uint64_t run = 0;
    for (uint64_t i = 0; i < n; i++) {
        const nrg_memfs_wr& r = reqs[i];
        const Cut c = cut_of(log2_b, files, r.ino, r.offset, r.len);
        if (c.kind == CUT_BYTES && (r.data_off > data_bytes || r.len > data_bytes - r.data_off)) return NRG_E_INVAL;
        first[i] = run;
        run += c.frags;
        if (written) written[i] = c.written;
        if (some) some[i] = c.some;
    }
    if (first) first[n] = run;
    return NRG_OK;
}

// ---- logged reads of any length (nrg_memfs_pread_logged*, include/nrgpu.h) ---------------------------
// The read-shaped cut: a request {ino, offset, len} becomes one Read record per 128-byte line of what it
// plans to read, planned = min(len, A - offset) with A = 2^log2_adm, and owns planned bytes of the
// caller's buffer (its slot). memfs.hip's mf_rfrag and mf_rgather kernels use these same functions.
struct RCut {
    uint64_t frags;    // f_i >= 1
    uint64_t planned;  // bytes of the slot
    uint8_t some;
    uint8_t bytes;     // planned > 0: the records ask for bytes
};

// checked in the order the replay checks a record: the ino, then the range (no overflow: len may be
// 2^64 - 1, "read to the end", and offset anything)
NRG_MFP_HD inline RCut rcut_of(uint32_t log2_adm, uint64_t files, uint64_t ino, uint64_t offset, uint64_t len) {
    const uint64_t A = 1ull << log2_adm;
    if (ino < NRG_MEMFS_FIRST_INO || ino - NRG_MEMFS_FIRST_INO >= files) return RCut{1, 0, 0, 0};
    if (len == 0 || offset >= A) return RCut{1, 0, 1, 0};
    const uint64_t planned = len < A - offset ? len : A - offset;
    return RCut{((offset + planned - 1) >> LINE_LOG2) - (offset >> LINE_LOG2) + 1, planned, 1, 1};
}

// Where fragment k of a request with bytes starts inside the request's slot; k == frags gives planned.
NRG_MFP_HD inline uint64_t rfrag_pos(uint64_t offset, uint64_t planned, uint64_t frags, uint64_t k) {
    if (k == 0) return 0;
    if (k >= frags) return planned;
    return (((offset >> LINE_LOG2) + k) << LINE_LOG2) - offset;
}

// Record k (< frags) of a request: the record's offset and len.
NRG_MFP_HD inline void rfrag_of(const RCut& c, uint64_t offset, uint64_t k, uint64_t* rec_off, uint32_t* rec_len) {
    if (!c.bytes) {
        *rec_off = offset, *rec_len = 0;
    } else {
        const uint64_t lo = rfrag_pos(offset, c.planned, c.frags, k), hi = rfrag_pos(offset, c.planned, c.frags, k + 1);
        *rec_off = offset + lo, *rec_len = (uint32_t)(hi - lo);
    }
}

// The fragment of the slot's byte q (< planned) and the byte's index inside that fragment's response.
NRG_MFP_HD inline uint64_t rfrag_at(uint64_t offset, uint64_t q, uint32_t* idx) {
    const uint64_t k = ((offset + q) >> LINE_LOG2) - (offset >> LINE_LOG2);
    *idx = k ? (uint32_t)((offset + q) & (LINE - 1)) : (uint32_t)q;
    return k;
}

// nrg_memfs_pread_logged_plan. first: n + 1 words; offs: n + 1 words or NULL; some: n or NULL.
inline int read_plan(uint32_t log2_adm, uint64_t files, const nrg_memfs_rd* reqs, uint64_t n, uint64_t* first,
                     uint64_t* offs, uint8_t* some) {
    if (!geometry_ok(log2_adm, files)) return NRG_E_INVAL;
    if (n && (!reqs || !first)) return NRG_E_INVAL;
    uint64_t run = 0, bytes = 0;
    for (uint64_t i = 0; i < n; i++) {
        const RCut c = rcut_of(log2_adm, files, reqs[i].ino, reqs[i].offset, reqs[i].len);
        first[i] = run;
        run += c.frags;
        if (offs) offs[i] = bytes;
        bytes += c.planned;
        if (some) some[i] = c.some;
    }
    if (first) first[n] = run;
    if (offs) offs[n] = bytes;
    return NRG_OK;
}

// ---- capacity growth (nrg_set_max_capacity / nrg_memfs_reserve on a file store, include/nrgpu.h) ----
// The capacity after a log prefix is max(the capacity at open or the last reserve, the power of two at
// or above the largest admitted end so far): a maximum, so folding it record by record, chunk by chunk
// or over the whole prefix gives the same number. memfs.hip's mf_need kernel, its host paths and
// tests/memfs_grow_policy.cpp share the two functions below.

// The end (bytes of its file) a record asks the store to hold under a bound of max_bytes per file, or 0:
// a valid Write of len > 0 with offset + len <= max_bytes, a valid SetAttr of size <= max_bytes. Checked
// in the replay's order, so an EINVAL or ENOENT record asks for nothing whatever its offset says, and
// neither does a record the replay answers with EFBIG (offset + len may not overflow).
NRG_MFP_HD inline uint64_t mf_rec_need(uint64_t ino, uint64_t offset, uint32_t op, uint32_t len, uint64_t files,
                                       uint64_t max_bytes) {
    if (op > NRG_MEMFS_SETATTR || len > LINE) return 0;
    if (ino < NRG_MEMFS_FIRST_INO || ino - NRG_MEMFS_FIRST_INO >= files) return 0;
    if (op == NRG_MEMFS_WRITE) return len && offset <= max_bytes && len <= max_bytes - offset ? offset + len : 0;
    if (op == NRG_MEMFS_SETATTR) return offset <= max_bytes ? offset : 0;
    return 0;
}

// log2 of the capacity that holds `need` bytes per file: log2_b itself where they fit, else the power of
// two at or above need, never past max_log2 (an admitted need is within it; a store reserved beyond its
// bound stays as it is).
NRG_MFP_HD inline uint32_t mf_grow_log2(uint32_t log2_b, uint64_t need, uint32_t max_log2) {
    uint32_t l = log2_b;
    while (l < max_log2 && (1ull << l) < need) l++;
    return l;
}

// The need of a planned call: the largest end of the requests that plan(log2_adm, ...) admits with bytes.
inline uint64_t plan_need(uint32_t log2_adm, uint64_t files, const nrg_memfs_wr* reqs, uint64_t n) {
    uint64_t need = 0;
    for (uint64_t i = 0; i < n; i++) {
        const nrg_memfs_wr& r = reqs[i];
        if (cut_of(log2_adm, files, r.ino, r.offset, r.len).kind == CUT_BYTES && r.offset + r.len > need)
            need = r.offset + r.len;
    }
    return need;
}

}  // namespace mfp
}  // namespace nrg
