// capacity.hpp — the capacity and growth policy of the kinds that grow under replay (stack, queue,
// skip list; the page table has the explicit half only), as pure host arithmetic: no HIP header, so
// tests/capacity_policy.cpp checks it without a GPU. The runtime drives it (runtime.cpp: room,
// set_max, reserve_common, restore_room) through what a kind's DsOps says about its capacity.
// The hashmap keeps its own (hm_room / hm_grow): its unit is log2 slots against a load limit and the
// combiner needs the `due` variant, so folding it in would add parameters, not remove code.
//
// The item count lives on the device, so the host keeps an upper bound of it, len_ub: the exact
// count when it was last read plus every record replayed (or prefilled) since. A chunk of n records
// with len_ub + n <= capacity costs that comparison. Only when the bound passes the capacity is the
// exact count read (a stream synchronise), and only if exact + n still passes it does the structure
// grow. A balanced Push/Pop stream re-reads its length now and then and never reallocates. At the
// bound the structure is a fixed one: nothing is read, and a chunk that overflows latches
// ERR_CAPACITY as it always did. Every decision depends on the log prefix, the chunking and the bound
// alone, so replicas that replay the same log in the same chunks grow at the same record.
#pragma once

#include <stdint.h>

namespace nrg {

struct Growth {
    uint64_t max_items = 0;  // the capacity automatic growth stops at (0: a fixed capacity)
    uint64_t len_ub = 0;     // upper bound of the item count
};

// The fast path, inline before every chunk of n records: true when the chunk fits (and is accounted,
// where anything is), false when the exact count has to be read first (runtime.cpp room).
inline bool growth_fits(Growth& g, uint64_t cap, uint64_t n) {
    if (!g.max_items || cap >= g.max_items) return true;
    if (g.len_ub + n > cap) return false;
    g.len_ub += n;
    return true;
}

// The capacity that holds `need` items (the exact count + n, or a snapshot's items): cap itself where
// they fit, else at least double and at least `need`, clipped to the bound.
inline uint64_t growth_target(const Growth& g, uint64_t cap, uint64_t need) {
    if (need <= cap) return cap;
    const uint64_t want = 2 * cap < need ? need : 2 * cap;
    return want > g.max_items ? g.max_items : want;
}

// nrg_restore: with a bound the image may be as large as the bound (the structure grows first)
inline bool growth_admits(const Growth& g, uint64_t cap, uint64_t items) {
    return items <= (cap > g.max_items ? cap : g.max_items);
}

// nrg_set_max_capacity: 0 (off), or from the current capacity to the largest nrg_open accepts
inline bool growth_bound_ok(uint64_t max_items, uint64_t cap, uint64_t cap_limit) {
    return !max_items || (max_items >= cap && max_items <= cap_limit);
}

}  // namespace nrg
