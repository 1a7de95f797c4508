// memfs_plan.hpp — the cut of the file store's writes of any length (nrg_memfs_pwrite*, include/nrgpu.h)
// into 128-byte log records, as pure arithmetic: no HIP header, so tests/memfs_plan.cpp checks it
// without a GPU. The host plans a call with plan() before anything is queued (T, the records of the
// call, moves the log's tail, which is host state); memfs.hip's mf_frag kernel builds fragment t of the
// call with the same cut_of() and frag_of(), compiled for the device. Log content is observable
// (nrg_test_ring_read), so the cut is specified in nrgpu.h and both sides follow it from here.
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

}  // namespace mfp
}  // namespace nrg
