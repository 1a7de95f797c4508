// skiplist_pop_plan.hpp — the grants of one pop step of the skip list (nrg_skiplist_enable_pops,
// include/nrgpu.h; skiplist.hip sl_pop_plan), as pure arithmetic: no HIP header, so
// tests/skiplist_pop_plan.cpp checks it without a GPU.
//
// A pop step replays a run of consecutive pop records against a map of `len` entries. Record i asks
// for n_i entries from its end (front: the smallest, back: the largest); replayed one by one it gets
// m_i = min(n_i, what is left). The entries left shrink by every grant, whatever the end, so with
// S_i = n_0 + ... + n_{i-1} the grants before record i sum to min(len, S_i) and
//   m_i = min(n_i, len - min(len, S_i)).
// n_i may be anything up to 2^64 - 1, so S is summed over the counts clipped to len (clip): the
// minimum with len is the same, and a run of r records sums to at most r * len. Where even that could
// wrap, add() saturates; saturated sums stay >= len and the grants stay right.
// A front record's entries are the ascending ranks [F_i, F_i + m_i) of the map before the step, F_i
// the grants to earlier front records of the run; a back record's are the descending ranks
// [B_i, B_i + m_i) from the top, that is the ascending ranks len - 1 - B_i downwards. Fronts and backs
// never meet: all grants together are at most len.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define NRG_SLP_HD __host__ __device__
#else
#define NRG_SLP_HD
#endif

namespace nrg {
namespace slp {

// a record's count as far as a map of len entries can tell
NRG_SLP_HD inline uint64_t clip(uint64_t n, uint64_t len) { return n < len ? n : len; }

// a + b, or 2^64 - 1 where that wraps
NRG_SLP_HD inline uint64_t add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }

// the entries granted to the records before one whose earlier (clipped) counts sum to S
NRG_SLP_HD inline uint64_t taken(uint64_t len, uint64_t S) { return S < len ? S : len; }

// m_i: what a record asking for n gets
NRG_SLP_HD inline uint64_t grant(uint64_t n, uint64_t len, uint64_t S) {
    const uint64_t left = len - taken(len, S);
    return n < left ? n : left;
}

// The ascending rank, in the map before the step, of entry r (0 <= r < m_i) of a record whose end has
// granted `before` entries to earlier records of the run (F_i or B_i).
NRG_SLP_HD inline uint64_t rank_of(bool back, uint64_t len, uint64_t before, uint64_t r) {
    return back ? len - 1 - (before + r) : before + r;
}

}  // namespace slp
}  // namespace nrg
