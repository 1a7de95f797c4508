// skiplist.hip — replicated ordered map (SkipMap<u64, u64>) replay on gfx950
// (benches/lockfree.rs:73-97 SkipListConcurrent::Get / OpWr::Push, :278-317 main;
// benches/lockfree_partitioned.rs:86-118 SkipListWrapper, its default :88-96).
//
// What the reference's skip list has and a hash map has not is order: front, back, lower_bound,
// upper_bound, range, iteration in key order (Replica::verify hands the caller the SkipMap itself,
// nr/src/replica.rs:443-467). A pointer-chasing list would serialise a replay; here the map is two
// sorted runs with DISJOINT key sets, each a pair of arrays (keys, values):
//   base   up to `capacity` keys
//   delta  up to delta_max + max_batch keys
// Disjointness keeps everything else simple: len = nb + nd, a range count is two rank differences
// per run, a seek is the better of two candidates, and the dump, the snapshot and the digest never
// de-duplicate. Both runs are double-buffered: a merge reads one buffer and writes the other.
//
// Replay of a chunk of n records (Push(k, v) = SkipMap::insert, which replaces the value of a
// present key; the response Ok(Some(k)) does not depend on the state), in stream order, no
// workgroup waiting on another except inside the radix sort's look-back:
//   sl_stream    the log copy of a fused round, the responses (key, 1), the keys' low words
//   sort         stable sort of (key, position) by the full 64-bit key: n <= SL_SORT_WG in the LDS of
//                one workgroup (bitonic on the pair, which is unique, so the order is the stable
//                one); else two runs of the 32-bit pair sort (radix_sort.hip, tiles of
//                SL_SORT_TILE), low word then high word. Timed as "sl_sort".
//   sl_resolve   last-writer election (the last record of every run of equal keys survives) and a
//                binary search of each survivor in base and in delta: a hit stores the value in
//                place (survivors are distinct: no two lanes write one element), a miss is flagged
//                and counted per tile of SL_RES_TILE
//   sl_scan      one workgroup: the tiles' offsets, the number of new keys, the capacity check
//   sl_scatter   the misses, still sorted, into the chunk's list of new keys
//   sl_merge     merge path of delta and the new keys into the other delta buffer, partitions of
//                SL_MERGE_PART outputs per workgroup, staged in LDS, and SL_MERGE_ITEMS per lane;
//                diagonals are found by a binary search over index bounds (no padding key:
//                2^64 - 1 is an ordinary key)
//   sl_compact   only when nd > delta_max after the merge: the same merge of base and delta into
//                the other base buffer; delta becomes empty
// The host does not know nd exactly: it keeps an upper bound (nd when last read plus every record
// replayed since) and reads the counts, one synchronise, only when the bound passes delta_max.
//
// Removal (nrg_skiplist_enable_removal; DESIGN.md "Skip list replay", Removal). On an enabled context a
// record whose val is the tombstone is Remove(key) (SkipMap::remove). The runs stay dense: a removed key
// is dropped physically, so no reader, digest, snapshot or merge ever sees a dead entry. A chunk there:
//   sl_stream, sort   unchanged (a Remove's response (key, 1) is overwritten below)
//   sl_rm_resp        a Remove's response: from the record before it in sorted order if that has the
//                     same key (a Push: its value; a Remove: None), else a lookup of the state before
//                     the chunk. It only reads the runs and is a launch of its own ahead of sl_resolve,
//                     whose surviving Pushes store values in place from other lanes and workgroups.
//   sl_resolve<true>  a surviving Remove that hits a run records the index (kidx) and flags the run;
//                     a miss does nothing (it is no new key). Three counts per tile.
//   sl_scan<true>     the misses as before, checked against the counts BEFORE the chunk's removals;
//                     the kill counts kb, kd; the state then already holds the counts after the drops
//   sl_scatter<true>  the misses, and the dead indices of each run, ascending (survivors are sorted by
//                     key and so are the runs)
//   (the host reads the state back: it cannot know otherwise whether a buffer flips)
//   sl_drop_base      only when kb > 0: the base run without its dead indices into the other buffer
//   sl_drop_delta     only when kd > 0: the same for the delta run, before the merge of the new keys
//   sl_merge, sl_compact   as before, on exact counts
//
// Pops (nrg_skiplist_enable_pops; DESIGN.md "Skip list replay", Pops). On an enabled context a record
// {n, front_mark} is PopFront x n and {n, back_mark} PopBack x n (SkipMap::pop_front / pop_back n times),
// answered (m, m >= 1), m the entries popped. The smallest m entries are a prefix of each run and the
// largest a suffix, split by one merge-path co-rank, so a run of pop records is one step whatever its
// counts. A pop depends on everything before it, so a chunk there is cut at its pop records:
//   sl_pop_find       once per chunk, ahead of sl_stream: the edges of the maximal runs of pop records,
//                     compacted per tile of SL_FIND_PART positions; the host reads the tiles' counts and,
//                     where one is not zero, the edges. None: the chunk as it is, through the pipeline above.
//   (else the chunk is replayed as alternating segments: an ordinary stretch is a chunk of its own through
//   the pipeline above, with or without removal; a run of pop records is one pop step)
//   sl_pop_plan       one workgroup: the grants of skiplist_pop_plan.hpp, the responses, per record its
//                     output offset and first rank, the totals and their co-ranks, the counts after the step
//   (the host reads the plan back: it cannot know otherwise whether a buffer flips)
//   sl_pop_take       only for nrg_skiplist_round_pops_async: the popped entries, packed in record order,
//                     the work spread over output positions
//   sl_pop_shift      only for a run that lost a prefix: the rest of it to the start of its other buffer.
//                     Back pops alone lower the counts.
//   sl_peek           for the group-wide pop of a partitioned group (group_pops.cpp): a member's smallest and
//                     largest entries by the same merge-path split, nothing popped
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "internal.hpp"
#include "skiplist_pop_plan.hpp"
#include "../../include/nrgpu_testing.h"

namespace nrg {

constexpr int SL_TPB = 256;
constexpr u32 SL_SORT_WG = 1024;     // chunks up to here sort in one workgroup's LDS
constexpr u32 SL_SORT_TILE = 2048;   // keys per tile of the radix sort's passes (radix_sort.hip)
constexpr u32 SL_RES_TILE = 256;     // records per resolve / scatter workgroup
constexpr u32 SL_MERGE_ITEMS = 8;    // outputs per lane of a merge
constexpr u32 SL_MERGE_PART = 2048;  // outputs per merge workgroup: SL_TPB * SL_MERGE_ITEMS
constexpr int SL_SCAN_TPB = 1024;
constexpr u32 SL_MAX_GRID = 4096;    // merge workgroups launched at most; the rest by stride
constexpr u32 SL_DROP_ITEMS = 8;     // inputs per lane of a drop pass
constexpr u32 SL_DROP_PART = 2048;   // inputs per drop workgroup and turn: SL_TPB * SL_DROP_ITEMS
constexpr u32 SL_FIND_ITEMS = 8;     // positions per lane of the pop-run search
constexpr u32 SL_FIND_PART = 2048;   // positions per sl_pop_find workgroup: SL_TPB * SL_FIND_ITEMS
constexpr u32 SL_TAKE_PART = 2048;   // outputs per sl_pop_take workgroup and turn
constexpr u32 SL_LOG2_MIN = 4, SL_LOG2_MAX = 28, SL_LOG2_DEFAULT = 24;
// delta_max unless NRG_KNOB_SL_DELTA_MAX sets it (microbench/skiplist_round.py, DESIGN.md "Skip list replay")
constexpr u64 SL_DELTA_DEFAULT = 1ull << 22;
static_assert(SL_MERGE_PART == SL_TPB * SL_MERGE_ITEMS, "a merge workgroup's lanes cover its partition");
static_assert(SL_SORT_TILE == SORT_TILE, "the radix sort's tile, mirrored for the tests' chunk sizes");
static_assert(SL_RES_TILE == SL_TPB, "resolve and scatter take one record per lane");
static_assert(SL_DROP_PART == SL_TPB * SL_DROP_ITEMS, "a drop workgroup's lanes cover its partition");
static_assert(SL_FIND_PART == SL_TPB * SL_FIND_ITEMS, "a find workgroup's lanes cover its partition");

struct SlJob {
    const nrg_put* src;  // the batch of a fused round or a prefill, or nullptr: read from the ring
    nrg_put* ring;       // the log ring; written when src is a fused round's batch (wring)
    u64 ring_mask;
    u32 wring;
    u64 lo, n;           // the chunk: log indices [lo, lo + n)
    u64 rlo, rhi;        // response window
    u64* resp;
    uint8_t* some;
    SlState* st;
    DevCtl* ctl;
    u64 *bk, *bv, *dk, *dv;  // the current base and delta buffers
    u64 cap, dcap;           // keys the base and the delta buffers hold
    u64* sk;                 // [n] sorted keys
    u32* sp;                 // [n] their chunk positions
    u32* k32;                // [n] low / high words (radix sort input)
    u32* pv;                 // [n] permutation after the low-word sort
    uint8_t* miss;           // [n] survivor found in neither run (removal: | SL_KILL_BASE / SL_KILL_DELTA)
    u32* tcnt;               // [tiles] misses per tile, then their exclusive offsets
    u64 *nk, *nv;            // the chunk's new keys, sorted
    // removal only (nullptr / 0 otherwise)
    u64 tomb;                // val of a Remove record
    u32* kidx;               // [n] the run index a surviving Remove hit
    u32* kcnt;               // [2 * tiles] base kills per tile, then delta kills; then their offsets
    u32 *deadb, *deadd;      // the chunk's dead indices of base and of delta, ascending
};
constexpr uint8_t SL_MISS = 1, SL_KILL_BASE = 2, SL_KILL_DELTA = 4;  // SlJob::miss flags

__device__ __forceinline__ nrg_put sl_load(const SlJob& j, u64 i) {
    return j.src ? j.src[i] : j.ring[(j.lo + i) & j.ring_mask];
}

// first index with a[idx] >= k (lower) or > k (upper), in [0, n]
template <typename T>  // (u64 keys of a run; u32 run indices of a chunk's dead list)
__device__ __forceinline__ u64 sl_lower(const T* __restrict__ a, u64 n, u64 k) {
    u64 lo = 0, hi = n;
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (a[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ u64 sl_upper(const u64* __restrict__ a, u64 n, u64 k) {
    u64 lo = 0, hi = n;
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(SL_TPB) void sl_stream_kernel(SlJob j) {
    const u64 i = (u64)blockIdx.x * SL_TPB + threadIdx.x;
    if (i >= j.n) return;
    const nrg_put r = sl_load(j, i);
    if (j.wring) j.ring[(j.lo + i) & j.ring_mask] = r;  // Log::append of a fused round
    const u64 g = j.lo + i;
    if (j.resp && g >= j.rlo && g < j.rhi) {  // Ok(Some(key)) (benches/lockfree_partitioned.rs:108-111)
        j.resp[g - j.rlo] = r.key;
        j.some[g - j.rlo] = 1;
    }
    j.k32[i] = (u32)r.key;
}

// (key, position) pairs of a chunk of n <= SL_SORT_WG records, sorted in LDS: a bitonic network over
// P = the power of two at or above n; the slots past n hold (2^64 - 1, 2^32 - 1), which no record
// equals (positions are < n), so they sort last without any key being reserved.
__global__ __launch_bounds__(SL_TPB) void sl_sort_wg_kernel(SlJob j, u32 P) {
    __shared__ u64 s_k[SL_SORT_WG];
    __shared__ u32 s_p[SL_SORT_WG];
    const u32 t = threadIdx.x, n = (u32)j.n;
    for (u32 i = t; i < P; i += SL_TPB) {
        s_k[i] = i < n ? sl_load(j, i).key : ~0ull;
        s_p[i] = i < n ? i : 0xFFFFFFFFu;
    }
    __syncthreads();
    for (u32 k = 2; k <= P; k <<= 1)
        for (u32 s = k >> 1; s > 0; s >>= 1) {
            for (u32 q = t; q < P / 2; q += SL_TPB) {
                const u32 a = ((q & ~(s - 1)) << 1) | (q & (s - 1)), b = a | s;
                const bool up = (a & k) == 0;
                const u64 ka = s_k[a], kb = s_k[b];
                const u32 pa = s_p[a], pb = s_p[b];
                const bool gt = ka > kb || (ka == kb && pa > pb);
                if (gt == up) {
                    s_k[a] = kb, s_k[b] = ka;
                    s_p[a] = pb, s_p[b] = pa;
                }
            }
            __syncthreads();
        }
    for (u32 i = t; i < n; i += SL_TPB) {
        j.sk[i] = s_k[i];
        j.sp[i] = s_p[i];
    }
}

// after the low-word sort: the permutation, and the high word of each record in that order
__global__ __launch_bounds__(SL_TPB) void sl_gather_hi_kernel(SlJob j, const u32* __restrict__ perm) {
    const u64 i = (u64)blockIdx.x * SL_TPB + threadIdx.x;
    if (i >= j.n) return;
    const u32 p = perm[i];
    j.pv[i] = p;
    j.k32[i] = (u32)(sl_load(j, p).key >> 32);
}

// after the high-word sort: the sorted keys and their positions
__global__ __launch_bounds__(SL_TPB) void sl_gather_kernel(SlJob j, const u32* __restrict__ perm) {
    const u64 i = (u64)blockIdx.x * SL_TPB + threadIdx.x;
    if (i >= j.n) return;
    const u32 p = perm[i];
    j.sp[i] = p;
    j.sk[i] = sl_load(j, p).key;
}

// Removal: the response of every Remove in the response window, one lane per sorted position. The
// record before it in sorted order, if it has the same key, is the latest record of that key ahead of
// it in the log (equal keys lie in ascending log position) and decides alone: a Push leaves its value,
// a Remove leaves nothing. The first record of a key asks the state before the chunk. Reads the runs
// only: sl_resolve, which writes them, is a later launch.
__global__ __launch_bounds__(SL_TPB) void sl_rm_resp_kernel(SlJob j) {
    const u64 i = (u64)blockIdx.x * SL_TPB + threadIdx.x;
    if (i >= j.n) return;
    const u32 p = j.sp[i];
    const u64 g = j.lo + p;
    if (g < j.rlo || g >= j.rhi) return;
    const nrg_put r = sl_load(j, p);
    if (r.val != j.tomb) return;
    u64 v = 0;
    uint8_t f = 0;
    if (i > 0 && j.sk[i - 1] == r.key) {
        const u64 pv = sl_load(j, j.sp[i - 1]).val;
        if (pv != j.tomb) v = pv, f = 1;
    } else {
        const u64 nb = j.st->nb, nd = j.st->nd;
        const u64 ib = sl_lower(j.bk, nb, r.key);
        if (ib < nb && j.bk[ib] == r.key) {
            v = j.bv[ib], f = 1;
        } else {
            const u64 id = sl_lower(j.dk, nd, r.key);
            if (id < nd && j.dk[id] == r.key) v = j.dv[id], f = 1;
        }
    }
    j.resp[g - j.rlo] = v;  // Some(previous value) or None (SkipMap::remove)
    j.some[g - j.rlo] = f;
}

// RM: the context has removal enabled. A surviving Remove that hits a run stores nothing: it notes the
// index and flags the run; one that misses is no new key.
template <bool RM>
__global__ __launch_bounds__(SL_TPB) void sl_resolve_kernel(SlJob j) {
    constexpr int NC = RM ? 3 : 1;  // what a tile counts: misses, base kills, delta kills
    __shared__ u32 s_cnt[NC][SL_TPB / 64];
    const u64 i = (u64)blockIdx.x * SL_RES_TILE + threadIdx.x;
    uint8_t f = 0;
    if (i < j.n) {
        const u64 k = j.sk[i];
        // equal keys lie in ascending log position: the last one is the chunk's last writer
        if (i + 1 == j.n || j.sk[i + 1] != k) {
            const u64 v = sl_load(j, j.sp[i]).val;
            const bool rm = RM && v == j.tomb;
            const u64 nb = j.st->nb, nd = j.st->nd;
            const u64 ib = sl_lower(j.bk, nb, k);
            if (ib < nb && j.bk[ib] == k) {
                if (rm) j.kidx[i] = (u32)ib, f = SL_KILL_BASE; else j.bv[ib] = v;
            } else {
                const u64 id = sl_lower(j.dk, nd, k);
                if (id < nd && j.dk[id] == k) {
                    if (rm) j.kidx[i] = (u32)id, f = SL_KILL_DELTA; else j.dv[id] = v;
                } else if (!rm) {
                    f = SL_MISS;
                }
            }
        }
        j.miss[i] = f;
    }
#pragma unroll
    for (int q = 0; q < NC; q++) {
        const u64 b = __ballot((f >> q) & 1);
        if ((threadIdx.x & 63) == 0) s_cnt[q][threadIdx.x >> 6] = (u32)__popcll(b);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < NC; q++) {
            u32 c = 0;
            for (int w = 0; w < SL_TPB / 64; w++) c += s_cnt[q][w];
            if (q == 0) j.tcnt[blockIdx.x] = c; else j.kcnt[(q - 1) * gridDim.x + blockIdx.x] = c;
        }
    }
}

// cnt[0, tiles) becomes its exclusive prefix sums, by the workgroup; the total
__device__ __forceinline__ u32 sl_scan_tiles(u32* cnt, u32 tiles, u32* s_scan) {
    const u32 t = threadIdx.x;
    const u32 per = (tiles + SL_SCAN_TPB - 1) / SL_SCAN_TPB;
    const u32 i0 = t * per < tiles ? t * per : tiles, i1 = i0 + per < tiles ? i0 + per : tiles;
    u32 mine = 0;
    for (u32 i = i0; i < i1; i++) mine += cnt[i];
    s_scan[t] = mine;
    __syncthreads();
    for (u32 s = 1; s < SL_SCAN_TPB; s <<= 1) {
        const u32 o = t >= s ? s_scan[t - s] : 0;
        __syncthreads();
        s_scan[t] += o;
        __syncthreads();
    }
    u32 run = s_scan[t] - mine;
    for (u32 i = i0; i < i1; i++) {
        const u32 c = cnt[i];
        cnt[i] = run;
        run += c;
    }
    const u32 total = s_scan[SL_SCAN_TPB - 1];
    __syncthreads();  // s_scan may be filled again
    return total;
}

// One workgroup: tcnt becomes the tiles' exclusive offsets; the number of new keys is clipped to the
// room left (nb + nd + nnew <= cap, and the delta buffer), ERR_CAPACITY latched when anything was
// clipped: the chunk's largest new keys are then left out and len stays within the capacity.
// RM: the two kill counts likewise. The room is what the runs leave BEFORE the chunk's own removals
// (the keys a chunk frees are room for the next chunk); nb and nd_in then drop by the kills, which is
// what the drop passes (launched by the host from kb, kd) make true before the merge reads nd_in.
template <bool RM>
__global__ __launch_bounds__(SL_SCAN_TPB) void sl_scan_kernel(SlJob j, u32 tiles) {
    __shared__ u32 s_scan[SL_SCAN_TPB];
    const u32 t = threadIdx.x;
    const u32 total = sl_scan_tiles(j.tcnt, tiles, s_scan);
    u32 kb = 0, kd = 0;
    if (RM) {
        kb = sl_scan_tiles(j.kcnt, tiles, s_scan);
        kd = sl_scan_tiles(j.kcnt + tiles, tiles, s_scan);
    }
    if (t == 0) {
        const u64 nb = j.st->nb, nd = j.st->nd;
        u64 nnew = total;
        u64 room = nb + nd < j.cap ? j.cap - (nb + nd) : 0;
        const u64 droom = nd < j.dcap ? j.dcap - nd : 0;  // (never the smaller one under the host's policy)
        if (droom < room) room = droom;
        if (nnew > room) {
            nnew = room;
            atomicOr(&j.ctl->err, ERR_CAPACITY);
        }
        if (RM) {
            j.st->nb = nb - kb;
            j.st->kb = kb;
            j.st->kd = kd;
        }
        j.st->nd_in = nd - kd;
        j.st->nnew = nnew;
        j.st->nd = nd - kd + nnew;
    }
}

template <bool RM>
__global__ __launch_bounds__(SL_TPB) void sl_scatter_kernel(SlJob j) {
    constexpr int NC = RM ? 3 : 1;
    __shared__ u32 s_cnt[NC][SL_TPB / 64];
    const u64 i = (u64)blockIdx.x * SL_RES_TILE + threadIdx.x;
    const uint8_t f = i < j.n ? j.miss[i] : 0;
    const u32 lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    u64 b[NC];
#pragma unroll
    for (int q = 0; q < NC; q++) {
        b[q] = __ballot((f >> q) & 1);
        if (lane == 0) s_cnt[q][w] = (u32)__popcll(b[q]);
    }
    __syncthreads();
    if (!f) return;
    const int c = f == SL_MISS ? 0 : (f == SL_KILL_BASE ? 1 : 2);  // (a survivor carries one flag)
    u32 pos = c == 0 ? j.tcnt[blockIdx.x] : j.kcnt[(c - 1) * gridDim.x + blockIdx.x];
#pragma unroll
    for (int q = 0; q < NC; q++)
        if (q == c) {
            pos += (u32)__popcll(b[q] & ((1ull << lane) - 1));
            for (u32 x = 0; x < w; x++) pos += s_cnt[q][x];
        }
    if (c == 0) {
        if (pos < j.st->nnew) {
            j.nk[pos] = j.sk[i];
            j.nv[pos] = sl_load(j, j.sp[i]).val;
        }
    } else {
        (c == 1 ? j.deadb : j.deadd)[pos] = j.kidx[i];
    }
}

// Removal's drop pass: the run in[0, n) without the nk indices dead[] lists (ascending, distinct, < n)
// into out[0, n - nk), a stream compaction. A workgroup takes a contiguous range [x0, x1) of
// SL_DROP_PART inputs per turn: its slice of the list is dead[d0, d1) by two binary searches, its
// outputs start at x0 - d0 (every dead index below x0 is one output less). The slice marks a byte
// per input in LDS; then, SL_TPB consecutive inputs at a time, the lanes flag, rank themselves by
// ballot and the waves' counts, and store. No workgroup waits on another, no atomics; n and nk are the
// host's (it has read the state back), so nothing here reads the state.
__global__ __launch_bounds__(SL_TPB) void sl_drop_kernel(const u64* __restrict__ ik, const u64* __restrict__ iv, u64 n,
                                                         const u32* __restrict__ dead, u32 nk, u64* __restrict__ ok,
                                                         u64* __restrict__ ov) {
    __shared__ uint8_t s_dead[SL_DROP_PART];
    __shared__ u32 s_cnt[SL_TPB / 64];
    const u32 t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (u64 part = blockIdx.x; part * SL_DROP_PART < n; part += gridDim.x) {
        const u64 x0 = part * SL_DROP_PART, x1 = x0 + SL_DROP_PART < n ? x0 + SL_DROP_PART : n;
        const u32 d0 = (u32)sl_lower(dead, nk, x0), d1 = (u32)sl_lower(dead, nk, x1);
        __syncthreads();  // the previous partition is done with the marks
        for (u32 q = t; q < SL_DROP_PART; q += SL_TPB) s_dead[q] = 0;
        __syncthreads();
        for (u32 q = d0 + t; q < d1; q += SL_TPB) {
            const u64 off = (u64)dead[q] - x0;
            if (off < SL_DROP_PART) s_dead[off] = 1;  // (always: dead[d0, d1) lies in [x0, x1))
        }
        __syncthreads();
        u64 out = x0 - d0;
        for (u32 it = 0; it < SL_DROP_ITEMS; it++) {
            const u32 o = it * SL_TPB + t;
            const u64 x = x0 + o;
            const bool keep = x < x1 && !s_dead[o];
            const u64 b = __ballot(keep);
            if (lane == 0) s_cnt[w] = (u32)__popcll(b);
            __syncthreads();
            u32 pos = (u32)__popcll(b & ((1ull << lane) - 1)), tot = 0;
            for (u32 q = 0; q < SL_TPB / 64; q++) {
                const u32 c = s_cnt[q];
                if (q < w) pos += c;
                tot += c;
            }
            if (keep) {
                ok[out + pos] = ik[x];
                ov[out + pos] = iv[x];
            }
            out += tot;
            __syncthreads();  // the counts are written again
        }
    }
}

// ---- merge path ----------------------------------------------------------------------------------
struct SlMerge {
    const u64 *ak, *av, *bk, *bv;  // two sorted runs
    u64 na, nb;                    // their lengths, unless from_state
    const SlState* st;             // from_state 1: na = st->nd_in, nb = st->nnew (a chunk's merge)
    u32 from_state;
    u64 *ok, *ov;                  // output arrays, or
    nrg_put* orec;                 // output records
};

// The split of diagonal d of the merge of a[0, na) and b[0, nb): how many of the first d outputs come
// from a, a first where keys are equal (they never are: the runs merged here hold disjoint key sets).
// The search runs over the index range max(0, d - nb) <= i <= min(d, na): every element it reads exists.
__device__ __forceinline__ u64 sl_split(const u64* a, u64 na, const u64* b, u64 nb, u64 d) {
    u64 lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= b[d - 1 - mid]) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The merge, a partition of SL_MERGE_PART outputs per workgroup and turn. The partition's two diagonals
// are searched in global memory (every lane the same search: the loads broadcast); its stretch of a
// and of b goes into LDS with coalesced loads; every lane finds the diagonal of its SL_MERGE_ITEMS
// outputs in LDS and merges them into registers; the outputs go back through LDS so that the stores
// are coalesced too. Workgroups of SL_TPB lanes.
template <bool AOS>
__device__ __forceinline__ void sl_merge_all(const SlMerge& m, u64 na, u64 nb) {
    __shared__ u64 s_k[SL_MERGE_PART], s_v[SL_MERGE_PART];
    const u32 t = threadIdx.x;
    const u64 total = na + nb;
    for (u64 part = blockIdx.x; part * SL_MERGE_PART < total; part += gridDim.x) {
        const u64 D0 = part * SL_MERGE_PART, D1 = D0 + SL_MERGE_PART < total ? D0 + SL_MERGE_PART : total;
        const u64 a0 = sl_split(m.ak, na, m.bk, nb, D0), a1 = sl_split(m.ak, na, m.bk, nb, D1);
        const u64 b0 = D0 - a0;
        const u32 cnt = (u32)(D1 - D0), la = (u32)(a1 - a0), lb = cnt - la;
        __syncthreads();  // the previous partition's stores are done with the tile
        for (u32 i = t; i < cnt; i += SL_TPB) {
            s_k[i] = i < la ? m.ak[a0 + i] : m.bk[b0 + (i - la)];
            s_v[i] = i < la ? m.av[a0 + i] : m.bv[b0 + (i - la)];
        }
        __syncthreads();
        u64 k[SL_MERGE_ITEMS], v[SL_MERGE_ITEMS];
        const u32 d0 = t * SL_MERGE_ITEMS;
        const u32 c = d0 >= cnt ? 0 : (cnt - d0 < SL_MERGE_ITEMS ? cnt - d0 : SL_MERGE_ITEMS);
        if (c) {
            u32 i = (u32)sl_split(s_k, la, s_k + la, lb, d0), jx = d0 - i;
#pragma unroll
            for (u32 q = 0; q < SL_MERGE_ITEMS; q++)
                if (q < c) {
                    const u64 ka = i < la ? s_k[i] : 0, kb = jx < lb ? s_k[la + jx] : 0;
                    const bool ta = jx >= lb || (i < la && ka <= kb);
                    k[q] = ta ? ka : kb;
                    v[q] = ta ? s_v[i] : s_v[la + jx];
                    if (ta) i++; else jx++;
                }
        }
        __syncthreads();  // every lane has read its inputs from the tile
#pragma unroll
        for (u32 q = 0; q < SL_MERGE_ITEMS; q++)
            if (q < c) {
                s_k[d0 + q] = k[q];
                s_v[d0 + q] = v[q];
            }
        __syncthreads();
        for (u32 i = t; i < cnt; i += SL_TPB) {
            if (AOS) {
                m.orec[D0 + i] = nrg_put{s_k[i], s_v[i]};
            } else {
                m.ok[D0 + i] = s_k[i];
                m.ov[D0 + i] = s_v[i];
            }
        }
    }
}

__global__ __launch_bounds__(SL_TPB) void sl_merge_kernel(SlMerge m) {
    const u64 na = m.from_state ? m.st->nd_in : m.na, nb = m.from_state ? m.st->nnew : m.nb;
    sl_merge_all<false>(m, na, nb);
}

__global__ void sl_set_state_kernel(SlState* st, u64 nb, u64 nd) { *st = SlState{nb, nd, nd, 0}; }

// ---- pops (nrg_skiplist_enable_pops) ---------------------------------------------------------------
struct SlPop {
    u64 fm, bm;        // val of a PopFront / PopBack record
    u64* off;          // [n + 1] entries granted to the records before record i of the run (the output offsets)
    u64* rank;         // [n] entries granted to the earlier records of record i's own end (F_i or B_i)
    u64* plan;         // [SL_PLAN_WORDS] {f, b, fb, fd, bb, bd, nb, nd}: totals, co-ranks, the counts before the step
    u64* pop_n;        // delivery (nrg_skiplist_round_pops_async): *pop_n = pop_base + f + b; or nullptr
    u64 pop_base;
};
constexpr u32 SL_PLAN_WORDS = 8;

// The edges of a chunk's pop runs: the positions x in [0, n] where "record x - 1 is a pop record"
// and "record x is one" differ (neither holds outside the chunk). In ascending order they alternate
// between the start of a maximal run and its end, so the host pairs them up. A workgroup takes
// SL_FIND_PART positions, SL_TPB consecutive ones at a time, and compacts its edges into its own
// stretch of ev[] by ballot ranks (as sl_drop); cnt[] gets the tile's number. No workgroup needs
// another's count, nothing is scanned: the host reads cnt[], and ev[] only where it is not all zero.
__global__ __launch_bounds__(SL_TPB) void sl_pop_find_kernel(SlJob j, u64 fm, u64 bm, u32* __restrict__ cnt,
                                                             u32* __restrict__ ev) {
    __shared__ u32 s_cnt[SL_TPB / 64];
    const u32 t = threadIdx.x, lane = t & 63, w = t >> 6;
    const u64 x0 = (u64)blockIdx.x * SL_FIND_PART;
    u32 out = 0;
    for (u32 it = 0; it < SL_FIND_ITEMS; it++) {
        const u64 x = x0 + it * SL_TPB + t;
        bool edge = false;
        if (x <= j.n) {
            const u64 va = x > 0 ? sl_load(j, x - 1).val : 0, vb = x < j.n ? sl_load(j, x).val : 0;
            const bool a = x > 0 && (va == fm || va == bm), b = x < j.n && (vb == fm || vb == bm);
            edge = a != b;
        }
        const u64 bal = __ballot(edge);
        if (lane == 0) s_cnt[w] = (u32)__popcll(bal);
        __syncthreads();
        u32 pos = (u32)__popcll(bal & ((1ull << lane) - 1)), tot = 0;
        for (u32 q = 0; q < SL_TPB / 64; q++) {
            const u32 c = s_cnt[q];
            if (q < w) pos += c;
            tot += c;
        }
        if (edge) ev[x0 + out + pos] = (u32)x;
        out += tot;
        __syncthreads();  // the counts are written again
    }
    if (t == 0) cnt[blockIdx.x] = out;
}

// the workgroup's exclusive prefix sums of one value per lane; *total gets their sum
__device__ __forceinline__ u64 sl_scan_lanes(u64 mine, u64* s_scan, u64* total) {
    const u32 t = threadIdx.x;
    s_scan[t] = mine;
    __syncthreads();
    for (u32 s = 1; s < SL_SCAN_TPB; s <<= 1) {
        const u64 o = t >= s ? s_scan[t - s] : 0;
        __syncthreads();
        s_scan[t] += o;
        __syncthreads();
    }
    const u64 ex = s_scan[t] - mine;
    *total = s_scan[SL_SCAN_TPB - 1];
    __syncthreads();  // s_scan may be filled again
    return ex;
}

// One pop step: the chunk j is a run of consecutive pop records (key = the count n_i, val = the end's
// mark), replayed against the len = nb + nd entries of the state. One workgroup, a contiguous stretch
// of the run per lane, three walks over it with the grants of skiplist_pop_plan.hpp:
//   the sum of the clipped counts, scanned: S_i, so off[i] = min(len, S_i) and the grant m_i
//   the grants to front records, scanned: F_i (and B_i = off[i] - F_i)
//   off[], rank[], the responses (m_i, m_i >= 1) inside the window, the log copy of a fused round
// Lane 0 then splits the totals f and b between the runs (sl_split: index bounds, no padding key: the
// f smallest entries are base[0, fb) and delta[0, fd), the b largest base[nb - bb, nb) and
// delta[nd - bd, nd)), leaves the plan for sl_pop_take and the host, and stores the counts after the
// step. The runs themselves are untouched here: the host launches the shifts from the plan.
__global__ __launch_bounds__(SL_SCAN_TPB) void sl_pop_plan_kernel(SlJob j, SlPop p) {
    __shared__ u64 s_scan[SL_SCAN_TPB];
    const u32 t = threadIdx.x;
    const u64 nb = j.st->nb, nd = j.st->nd, len = nb + nd;
    const u64 per = (j.n + SL_SCAN_TPB - 1) / SL_SCAN_TPB;
    const u64 i0 = t * per < j.n ? t * per : j.n, i1 = i0 + per < j.n ? i0 + per : j.n;
    u64 mine = 0;
    for (u64 i = i0; i < i1; i++) mine += slp::clip(sl_load(j, i).key, len);  // (< 2^24 * 2^28: no wrap)
    u64 stot, f;
    const u64 S = sl_scan_lanes(mine, s_scan, &stot);
    u64 s = S, fmine = 0;
    for (u64 i = i0; i < i1; i++) {
        const nrg_put r = sl_load(j, i);
        const u64 n = slp::clip(r.key, len);
        if (r.val == p.fm) fmine += slp::grant(n, len, s);
        s += n;
    }
    u64 F = sl_scan_lanes(fmine, s_scan, &f);
    s = S;
    for (u64 i = i0; i < i1; i++) {
        const nrg_put r = sl_load(j, i);
        const u64 n = slp::clip(r.key, len), m = slp::grant(n, len, s), o = slp::taken(len, s);
        const bool front = r.val == p.fm;
        p.off[i] = o;
        p.rank[i] = front ? F : o - F;
        if (front) F += m;
        s += n;
        const u64 g = j.lo + i;
        if (j.wring) j.ring[g & j.ring_mask] = r;  // Log::append of a fused round
        if (j.resp && g >= j.rlo && g < j.rhi) {
            j.resp[g - j.rlo] = m;  // entries popped: pop_front() n times, Some while the map had one
            j.some[g - j.rlo] = m ? 1 : 0;
        }
    }
    if (t == 0) {
        const u64 all = slp::taken(len, stot), b = all - f;
        p.off[j.n] = all;
        const u64 fb = sl_split(j.bk, nb, j.dk, nd, f), fd = f - fb;
        const u64 bb = nb - sl_split(j.bk, nb, j.dk, nd, len - b), bd = b - bb;
        p.plan[0] = f, p.plan[1] = b, p.plan[2] = fb, p.plan[3] = fd, p.plan[4] = bb, p.plan[5] = bd;
        p.plan[6] = nb, p.plan[7] = nd;
        *j.st = SlState{nb - fb - bb, nd - fd - bd, nd - fd - bd, 0, 0, 0};
        if (p.pop_n) *p.pop_n = p.pop_base + all;
    }
}

// The popped entries of a step, packed: output x in [0, cnt) is entry x - off[i] of the record i with
// off[i] <= x < off[i + 1], the entry of ascending rank slp::rank_of in the merge of the two runs as they
// were before the step (the plan's nb, nd; the shifts come later on the stream). The work is spread over
// output positions, SL_TAKE_PART per workgroup and turn, whatever the records' counts: a tile's records
// are found once by two searches of off[] (every lane the same: the loads broadcast), a lane's record
// inside that stretch, its entry by the merge-path split of its rank. Consecutive lanes store
// consecutive slots. cnt is the host's: the step's total, clipped to the room the caller's arrays have.
__global__ __launch_bounds__(SL_TPB) void sl_pop_take_kernel(SlJob j, SlPop p, u64* __restrict__ okeys,
                                                             u64* __restrict__ ovals, u64 cnt) {
    const u64 nb = p.plan[6], nd = p.plan[7], len = nb + nd;
    for (u64 part = blockIdx.x; part * SL_TAKE_PART < cnt; part += gridDim.x) {
        const u64 x0 = part * SL_TAKE_PART, x1 = x0 + SL_TAKE_PART < cnt ? x0 + SL_TAKE_PART : cnt;
        const u64 r0 = sl_upper(p.off, j.n, x0) - 1, r1 = sl_upper(p.off, j.n, x1 - 1) - 1;  // (off[0] = 0 <= x)
        for (u64 x = x0 + threadIdx.x; x < x1; x += SL_TPB) {
            const u64 i = r0 + sl_upper(p.off + r0, r1 - r0 + 1, x) - 1;
            const bool back = sl_load(j, i).val == p.bm;
            const u64 q = slp::rank_of(back, len, p.rank[i], x - p.off[i]);
            const u64 ia = sl_split(j.bk, nb, j.dk, nd, q), id = q - ia;  // (ia < nb or id < nd: q < len)
            const bool ta = id >= nd || (ia < nb && j.bk[ia] < j.dk[id]);
            okeys[x] = ta ? j.bk[ia] : j.dk[id];
            ovals[x] = ta ? j.bv[ia] : j.dv[id];
        }
    }
}

// The nf smallest entries of the map in ascending order and its nk largest in descending order, nothing
// popped: a member's candidates of a group-wide pop (group_pops.cpp). A lane per output, its entry by
// the merge-path split of its rank as in sl_pop_take; consecutive lanes store consecutive slots. The
// host's nf and nk are at most the state's length (it read the counts back); a rank the state does not
// have is skipped all the same.
__global__ __launch_bounds__(SL_TPB) void sl_peek_kernel(const u64* __restrict__ bk, const u64* __restrict__ bv,
                                                         const u64* __restrict__ dk, const u64* __restrict__ dv,
                                                         const SlState* __restrict__ st, u64 nf, u64 nk,
                                                         u64* __restrict__ fk, u64* __restrict__ fv,
                                                         u64* __restrict__ kk, u64* __restrict__ kv) {
    const u64 nb = st->nb, nd = st->nd, len = nb + nd;
    for (u64 x = (u64)blockIdx.x * SL_TPB + threadIdx.x; x < nf + nk; x += (u64)gridDim.x * SL_TPB) {
        const bool back = x >= nf;
        const u64 r = back ? x - nf : x;
        if (r >= len) continue;
        const u64 q = slp::rank_of(back, len, 0, r);
        const u64 ia = sl_split(bk, nb, dk, nd, q), id = q - ia;  // (ia < nb or id < nd: q < len)
        const bool ta = id >= nd || (ia < nb && bk[ia] < dk[id]);
        (back ? kk : fk)[r] = ta ? bk[ia] : dk[id];
        (back ? kv : fv)[r] = ta ? bv[ia] : dv[id];
    }
}

// what a front pop leaves of a run, in[from, from + n), to the start of the run's other buffer
__global__ __launch_bounds__(SL_TPB) void sl_pop_shift_kernel(const u64* __restrict__ ik, const u64* __restrict__ iv,
                                                              u64 from, u64 n, u64* __restrict__ ok, u64* __restrict__ ov) {
    for (u64 i = (u64)blockIdx.x * SL_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * SL_TPB) {
        ok[i] = ik[from + i];
        ov[i] = iv[from + i];
    }
}

// ---- reads: one lane per query, a binary search per run --------------------------------------------
__global__ __launch_bounds__(SL_TPB) void sl_get_kernel(const u64* bk, const u64* bv, const u64* dk, const u64* dv,
                                                        const SlState* st, const u64* keys, u64 n, u64* vals,
                                                        uint8_t* found) {
    const u64 i = (u64)blockIdx.x * SL_TPB + threadIdx.x;
    if (i >= n) return;
    const u64 k = keys[i], nb = st->nb, nd = st->nd;
    u64 v = 0;
    uint8_t f = 0;
    const u64 ib = sl_lower(bk, nb, k);
    if (ib < nb && bk[ib] == k) {
        v = bv[ib], f = 1;
    } else {
        const u64 id = sl_lower(dk, nd, k);
        if (id < nd && dk[id] == k) v = dv[id], f = 1;
    }
    vals[i] = v;
    found[i] = f;
}

// the run's candidate for a seek: its index, or n where the run has none
__device__ __forceinline__ u64 sl_seek_idx(const u64* a, u64 n, u64 k, u32 mode) {
    if (mode == NRG_SEEK_GE) return sl_lower(a, n, k);
    if (mode == NRG_SEEK_GT) return sl_upper(a, n, k);
    const u64 i = mode == NRG_SEEK_LE ? sl_upper(a, n, k) : sl_lower(a, n, k);
    return i ? i - 1 : n;
}

__global__ __launch_bounds__(SL_TPB) void sl_seek_kernel(const u64* bk, const u64* bv, const u64* dk, const u64* dv,
                                                         const SlState* st, const u64* keys, u64 n, u32 mode,
                                                         u64* okeys, u64* ovals, uint8_t* found) {
    const u64 i = (u64)blockIdx.x * SL_TPB + threadIdx.x;
    if (i >= n) return;
    const u64 k = keys[i], nb = st->nb, nd = st->nd;
    const u64 ib = sl_seek_idx(bk, nb, k, mode), id = sl_seek_idx(dk, nd, k, mode);
    const bool hb = ib < nb, hd = id < nd;
    u64 ok = 0, ov = 0;
    if (hb || hd) {
        const u64 kb = hb ? bk[ib] : 0, kd = hd ? dk[id] : 0;
        const bool up = mode == NRG_SEEK_GE || mode == NRG_SEEK_GT;  // the smaller candidate, else the larger
        const bool take_b = hb && (!hd || (up ? kb < kd : kb > kd));
        ok = take_b ? kb : kd;
        ov = take_b ? bv[ib] : dv[id];
    }
    okeys[i] = ok;
    ovals[i] = ov;
    found[i] = (hb || hd) ? 1 : 0;
}

// SkipMap::range from a bound, the first `limit` entries (nrg_skiplist_scan): a group of W = 2^lw
// lanes per query, SL_TPB / W queries per workgroup. The answer is the head of the merge of two
// windows of at most `limit` keys, one per run, found by the seek's searches (every lane of the group
// runs them with the same addresses: the loads broadcast). Both directions are one ascending merge:
//   GE / GT  windows base[ib, ib + la), delta[id, id + lb); output t is merge position t
//   LE / LT  windows base[eb - la, eb), delta[ed - lb, ed) ending at the seek; output t is merge
//            position la + lb - 1 - t (the first `limit` in descending order are the last `limit` of
//            the merge, and those lie in the last `limit` keys of each run's stretch)
// Lane j takes outputs j, j + W, ...: its merge-path split (sl_split: index bounds, no padding key)
// says how many keys before its position come from base, and the smaller of the two keys there is
// its entry. Consecutive lanes store consecutive slots. No lane waits for another.
__global__ __launch_bounds__(SL_TPB) void sl_walk_kernel(const u64* bk, const u64* bv, const u64* dk, const u64* dv,
                                                         const SlState* st, const u64* keys, u64 n, u32 mode, u32 limit,
                                                         u32 lw, u64* okeys, u64* ovals, u32* counts) {
    const u64 gt = (u64)blockIdx.x * SL_TPB + threadIdx.x;
    const u64 q = gt >> lw;
    if (q >= n) return;
    const u32 W = 1u << lw, lane = (u32)gt & (W - 1);
    const u64 k = keys[q], nb = st->nb, nd = st->nd;
    const bool up = mode == NRG_SEEK_GE || mode == NRG_SEEK_GT;
    const u64 ib = sl_seek_idx(bk, nb, k, mode), id = sl_seek_idx(dk, nd, k, mode);
    // the keys of each run in the direction: from the seek index on, or up to and including it
    const u64 rb = up ? nb - ib : (ib < nb ? ib + 1 : 0), rd = up ? nd - id : (id < nd ? id + 1 : 0);
    const u32 la = rb < limit ? (u32)rb : limit, lb = rd < limit ? (u32)rd : limit;
    const u32 total = la + lb < limit ? la + lb : limit;
    const u64 a0 = up ? ib : rb - la, b0 = up ? id : rd - lb;
    const u64 *ak = bk + a0, *ck = dk + b0;
    u64* ok = okeys + q * limit;
    u64* ov = ovals + q * limit;
    for (u32 t = lane; t < total; t += W) {
        const u32 p = up ? t : la + lb - 1 - t;
        const u32 i = (u32)sl_split(ak, la, ck, lb, p), jx = p - i;  // (i < la or jx < lb: p < la + lb)
        const u64 ka = i < la ? ak[i] : 0, kc = jx < lb ? ck[jx] : 0;
        const bool ta = jx >= lb || (i < la && ka < kc);
        ok[t] = ta ? ka : kc;
        ov[t] = ta ? bv[a0 + i] : dv[b0 + jx];
    }
    if (lane == 0) counts[q] = total;
}

__global__ __launch_bounds__(SL_TPB) void sl_range_count_kernel(const u64* bk, const u64* dk, const SlState* st,
                                                                const u64* los, const u64* his, u64 n, u64* counts) {
    const u64 i = (u64)blockIdx.x * SL_TPB + threadIdx.x;
    if (i >= n) return;
    const u64 lo = los[i], hi = his[i], nb = st->nb, nd = st->nd;
    u64 c = 0;
    if (lo <= hi) c = (sl_upper(bk, nb, hi) - sl_lower(bk, nb, lo)) + (sl_upper(dk, nd, hi) - sl_lower(dk, nd, lo));
    counts[i] = c;
}

// the ranks of [lo, hi] in both runs: out = {b0, b1, d0, d1} (an empty window where lo > hi)
__global__ void sl_rank_kernel(const u64* bk, const u64* dk, const SlState* st, u64 lo, u64 hi, u64* out) {
    const u64 nb = st->nb, nd = st->nd;
    const bool any = lo <= hi;
    out[0] = any ? sl_lower(bk, nb, lo) : 0;
    out[1] = any ? sl_upper(bk, nb, hi) : 0;
    out[2] = any ? sl_lower(dk, nd, lo) : 0;
    out[3] = any ? sl_upper(dk, nd, hi) : 0;
}

// SkipListWrapper::default's records (keys k0 .. k0 + n - 1 -> k + off) for the replay pipeline
__global__ __launch_bounds__(SL_TPB) void sl_gen_kernel(nrg_put* out, u64 k0, u64 n, u64 off) {
    const u64 i = (u64)blockIdx.x * SL_TPB + threadIdx.x;
    if (i < n) out[i] = nrg_put{k0 + i, k0 + i + off};
}

// ---- host side -------------------------------------------------------------------------------------
static hipError_t sl_read_state(nrg_ctx* c, SlState* s) {
    hipError_t e = hipMemcpyAsync(s, c->sl.d_state, sizeof(*s), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && s->nb + s->nd > c->sl.cap) e = hipErrorUnknown;  // (the scan never lets it)
    return e;
}

static unsigned sl_merge_grid(u64 total) {
    const u64 g = (total + SL_MERGE_PART - 1) / SL_MERGE_PART;
    return g < 1 ? 1u : (g > SL_MAX_GRID ? SL_MAX_GRID : (unsigned)g);
}

static void sl_free_pair(u64* p[2]) {
    for (int i = 0; i < 2; i++) {
        if (p[i]) (void)hipFree(p[i]);
        p[i] = nullptr;
    }
}

// two buffers of `n` keys and two of `n` values; all or nothing
static hipError_t sl_alloc_runs(u64* k[2], u64* v[2], u64 n) {
    k[0] = k[1] = v[0] = v[1] = nullptr;
    for (int i = 0; i < 2; i++)
        if (hipMalloc(&k[i], n * 8) != hipSuccess || hipMalloc(&v[i], n * 8) != hipSuccess) {
            (void)hipGetLastError();  // (the failure is reported by the return value alone)
            sl_free_pair(k);
            sl_free_pair(v);
            return hipErrorOutOfMemory;
        }
    return hipSuccess;
}

__global__ __launch_bounds__(DG_TPB) void sl_grow_kernel(const u64* fk, const u64* fv, u64* tk, u64* tv,
                                                         const SlState* st, u64 from_cap) {
    const u64 n = st->nb < from_cap ? st->nb : from_cap;
    for (u64 i = blockIdx.x * (u64)DG_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * DG_TPB) {
        tk[i] = fk[i];
        tv[i] = fv[i];
    }
}

// Growth of the base run, as st_grow: the copy, then the stream is synchronised, the old buffers are
// freed and the new ones installed. If the allocation fails nothing has been launched.
static hipError_t sl_grow(nrg_ctx* c, u64 new_cap) {
    SlHost& s = c->sl;
    if (new_cap <= s.cap || new_cap > (1ull << SL_LOG2_MAX)) return hipErrorInvalidValue;
    u64 *nk[2], *nv[2];
    hipError_t e = sl_alloc_runs(nk, nv, new_cap);
    if (e != hipSuccess) return e;
    NRG_LAUNCH(c, "sl_grow", sl_grow_kernel, copy_grid(s.cap), DG_TPB, 0, c->stream, (const u64*)s.d_bk[s.bcur],
               (const u64*)s.d_bv[s.bcur], nk[s.bcur], nv[s.bcur], (const SlState*)s.d_state, s.cap);
    e = hipGetLastError();
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        sl_free_pair(nk);
        sl_free_pair(nv);
        return e;
    }
    sl_free_pair(s.d_bk);
    sl_free_pair(s.d_bv);
    for (int i = 0; i < 2; i++) s.d_bk[i] = nk[i], s.d_bv[i] = nv[i];
    s.cap = new_cap;
    return hipSuccess;
}

static hipError_t sl_compact(nrg_ctx* c, u64 nb, u64 nd) {
    SlHost& s = c->sl;
    SlMerge m{};
    m.ak = s.d_bk[s.bcur], m.av = s.d_bv[s.bcur], m.na = nb;
    m.bk = s.d_dk[s.dcur], m.bv = s.d_dv[s.dcur], m.nb = nd;
    m.ok = s.d_bk[s.bcur ^ 1], m.ov = s.d_bv[s.bcur ^ 1];
    NRG_LAUNCH(c, "sl_compact", sl_merge_kernel, sl_merge_grid(nb + nd), SL_TPB, 0, c->stream, m);
    sl_set_state_kernel<<<1, 1, 0, c->stream>>>(s.d_state, nb + nd, 0);
    s.bcur ^= 1;
    s.nd_ub = 0;
    return hipGetLastError();
}

static unsigned sl_drop_grid(u64 n) {
    const u64 g = (n + SL_DROP_PART - 1) / SL_DROP_PART;
    return g < 1 ? 1u : (g > SL_MAX_GRID ? SL_MAX_GRID : (unsigned)g);
}

// The rest of a chunk on a context with removal, after the sort. The records live on the device, so
// whether a run loses keys (and its buffer flips) is known only from the state: one readback per chunk,
// 48 bytes and a synchronise. After it the host knows nb and nd exactly and its bounds are the counts.
static hipError_t sl_chunk_rm(nrg_ctx* c, SlJob& j, u32 tiles) {
    SlHost& s = c->sl;
    hipError_t e;
    const unsigned g256 = (unsigned)((j.n + SL_TPB - 1) / SL_TPB);
    if (j.resp) NRG_LAUNCH(c, "sl_rm_resp", sl_rm_resp_kernel, g256, SL_TPB, 0, c->stream, j);
    NRG_LAUNCH(c, "sl_resolve", sl_resolve_kernel<true>, tiles, SL_TPB, 0, c->stream, j);
    NRG_LAUNCH(c, "sl_scan", sl_scan_kernel<true>, 1, SL_SCAN_TPB, 0, c->stream, j, tiles);
    NRG_LAUNCH(c, "sl_scatter", sl_scatter_kernel<true>, tiles, SL_TPB, 0, c->stream, j);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    SlState st{};
    timer_begin(c, "sl_rm_state");
    e = sl_read_state(c, &st);
    timer_end(c, "sl_rm_state");
    if (e != hipSuccess) return e;
    if (st.kb > j.n || st.kd > j.n || st.nb + st.kb > s.cap || st.nd_in + st.kd > s.dcap) return hipErrorUnknown;  // (never)
    if (st.kb) {
        NRG_LAUNCH(c, "sl_drop_base", sl_drop_kernel, sl_drop_grid(st.nb + st.kb), SL_TPB, 0, c->stream,
                   (const u64*)s.d_bk[s.bcur], (const u64*)s.d_bv[s.bcur], st.nb + st.kb, (const u32*)s.d_deadb,
                   (u32)st.kb, s.d_bk[s.bcur ^ 1], s.d_bv[s.bcur ^ 1]);
        s.bcur ^= 1;
    }
    if (st.kd) {
        NRG_LAUNCH(c, "sl_drop_delta", sl_drop_kernel, sl_drop_grid(st.nd_in + st.kd), SL_TPB, 0, c->stream,
                   (const u64*)s.d_dk[s.dcur], (const u64*)s.d_dv[s.dcur], st.nd_in + st.kd, (const u32*)s.d_deadd,
                   (u32)st.kd, s.d_dk[s.dcur ^ 1], s.d_dv[s.dcur ^ 1]);
        s.dcur ^= 1;
    }
    SlMerge m{};
    m.ak = s.d_dk[s.dcur], m.av = s.d_dv[s.dcur], m.bk = j.nk, m.bv = j.nv;
    m.st = s.d_state;
    m.from_state = 1;
    m.ok = s.d_dk[s.dcur ^ 1], m.ov = s.d_dv[s.dcur ^ 1];
    NRG_LAUNCH(c, "sl_merge", sl_merge_kernel, sl_merge_grid(st.nd), SL_TPB, 0, c->stream, m);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    s.dcur ^= 1;
    s.nd_ub = st.nd;
    if (c->growth.max_items) c->growth.len_ub = st.nb + st.nd;
    if (st.nd > s.delta_max) return sl_compact(c, st.nb, st.nd);
    return hipSuccess;
}

// One chunk of n <= max_batch records through the pipeline. `wring`: src is a fused round's batch and
// the log copy is written; a prefill passes its records as src with no log position behind them.
static hipError_t sl_chunk(nrg_ctx* c, const nrg_put* src, bool wring, u64 lo, u64 n, u64 resp_lo, u64 resp_hi,
                           void* d_resp, uint8_t* d_some) {
    if (n == 0) return hipSuccess;
    SlHost& s = c->sl;
    hipError_t e;
    // the runs grow first if they have to (one comparison if not)
    if (!growth_fits(c->growth, s.cap, n) && (e = room(c, n, "sl_room")) != hipSuccess) return e;
    SlJob j{};
    j.src = src;
    j.ring = (nrg_put*)c->d_ring;
    j.ring_mask = c->log_size - 1;
    j.wring = wring ? 1 : 0;
    j.lo = lo;
    j.n = n;
    const bool want = d_resp != nullptr && d_some != nullptr && resp_lo < resp_hi && resp_lo < lo + n && resp_hi > lo;
    j.rlo = want ? resp_lo : 0;
    j.rhi = want ? resp_hi : 0;
    j.resp = want ? (u64*)d_resp : nullptr;
    j.some = want ? d_some : nullptr;
    j.st = s.d_state;
    j.ctl = c->d_ctl;
    j.bk = s.d_bk[s.bcur], j.bv = s.d_bv[s.bcur];
    j.dk = s.d_dk[s.dcur], j.dv = s.d_dv[s.dcur];
    j.cap = s.cap;
    j.dcap = s.dcap;
    j.sk = s.d_sk, j.sp = s.d_sp, j.k32 = s.d_k32, j.pv = s.d_pv, j.miss = s.d_miss, j.tcnt = s.d_tcnt;
    j.nk = s.d_nk, j.nv = s.d_nv;
    const bool rm = s.removal;
    if (rm) j.tomb = s.tombstone, j.kidx = s.d_kidx, j.kcnt = s.d_kcnt, j.deadb = s.d_deadb, j.deadd = s.d_deadd;
    const unsigned g256 = (unsigned)((n + SL_TPB - 1) / SL_TPB);
    NRG_LAUNCH(c, "sl_stream", sl_stream_kernel, g256, SL_TPB, 0, c->stream, j);
    timer_begin(c, "sl_sort");
    if (n <= SL_SORT_WG) {
        u32 P = 2;
        while (P < n) P <<= 1;
        sl_sort_wg_kernel<<<1, SL_TPB, 0, c->stream>>>(j, P);
    } else {
        u32 *ok = nullptr, *ov = nullptr;
        if ((e = sort_pairs(c->sort, j.k32, nullptr, n, 32, c->stream, &ok, &ov)) != hipSuccess) return e;
        sl_gather_hi_kernel<<<g256, SL_TPB, 0, c->stream>>>(j, ov);
        if ((e = sort_pairs(c->sort, j.k32, j.pv, n, 32, c->stream, &ok, &ov)) != hipSuccess) return e;
        sl_gather_kernel<<<g256, SL_TPB, 0, c->stream>>>(j, ov);
    }
    timer_end(c, "sl_sort");
    const u32 tiles = (u32)((n + SL_RES_TILE - 1) / SL_RES_TILE);
    if (rm) return sl_chunk_rm(c, j, tiles);
    NRG_LAUNCH(c, "sl_resolve", sl_resolve_kernel<false>, tiles, SL_TPB, 0, c->stream, j);
    NRG_LAUNCH(c, "sl_scan", sl_scan_kernel<false>, 1, SL_SCAN_TPB, 0, c->stream, j, tiles);
    NRG_LAUNCH(c, "sl_scatter", sl_scatter_kernel<false>, tiles, SL_TPB, 0, c->stream, j);
    SlMerge m{};
    m.ak = j.dk, m.av = j.dv, m.bk = j.nk, m.bv = j.nv;
    m.st = s.d_state;
    m.from_state = 1;
    m.ok = s.d_dk[s.dcur ^ 1], m.ov = s.d_dv[s.dcur ^ 1];
    NRG_LAUNCH(c, "sl_merge", sl_merge_kernel, sl_merge_grid(s.nd_ub + n), SL_TPB, 0, c->stream, m);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    s.dcur ^= 1;
    s.nd_ub += n;
    // compaction policy: compact when nd > delta_max after a chunk's merge
    if (s.nd_ub > s.delta_max) {
        SlState st{};
        if ((e = sl_read_state(c, &st)) != hipSuccess) return e;
        s.nd_ub = st.nd;
        if (c->growth.max_items) c->growth.len_ub = st.nb + st.nd;
        if (st.nd > s.delta_max) return sl_compact(c, st.nb, st.nd);
    }
    return hipSuccess;
}

// ---- pops: a chunk cut at its pop runs ---------------------------------------------------------------
// what the pop kernels read of a job: the records, the window, the state and the current runs
static SlJob sl_pop_job(nrg_ctx* c, const nrg_put* src, bool wring, u64 lo, u64 n, u64 resp_lo, u64 resp_hi, void* d_resp,
                        uint8_t* d_some) {
    SlHost& s = c->sl;
    SlJob j{};
    j.src = src;
    j.ring = (nrg_put*)c->d_ring;
    j.ring_mask = c->log_size - 1;
    j.wring = wring ? 1 : 0;
    j.lo = lo;
    j.n = n;
    const bool want = d_resp != nullptr && d_some != nullptr && resp_lo < resp_hi && resp_lo < lo + n && resp_hi > lo;
    j.rlo = want ? resp_lo : 0;
    j.rhi = want ? resp_hi : 0;
    j.resp = want ? (u64*)d_resp : nullptr;
    j.some = want ? d_some : nullptr;
    j.st = s.d_state;
    j.ctl = c->d_ctl;
    j.bk = s.d_bk[s.bcur], j.bv = s.d_bv[s.bcur];
    j.dk = s.d_dk[s.dcur], j.dv = s.d_dv[s.dcur];
    j.cap = s.cap;
    j.dcap = s.dcap;
    return j;
}

// The chunk's pop runs into s.h_pf as ascending edges (start, end, start, end, ...), *ne their number.
// The records live on the device: one launch, and a readback of the tiles' counts (4 bytes per
// SL_FIND_PART records); the edges themselves are read only where a count is not zero.
static hipError_t sl_pop_find(nrg_ctx* c, const nrg_put* src, u64 lo, u64 n, size_t* ne) {
    SlHost& s = c->sl;
    hipError_t e;
    const SlJob j = sl_pop_job(c, src, false, lo, n, 0, 0, nullptr, nullptr);
    const u32 tiles = (u32)((n + 1 + SL_FIND_PART - 1) / SL_FIND_PART);
    NRG_LAUNCH(c, "sl_pop_find", sl_pop_find_kernel, tiles, SL_TPB, 0, c->stream, j, s.front_mark, s.back_mark, s.d_pfcnt,
               s.d_pfev);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    std::vector<u32>& h = s.h_pf;
    h.resize(tiles);
    if ((e = hipMemcpyAsync(h.data(), s.d_pfcnt, tiles * 4, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return e;
    u64 total = 0;
    u32 t0 = tiles, t1 = 0;
    for (u32 t = 0; t < tiles; t++) {
        if (h[t] > SL_FIND_PART) return hipErrorUnknown;  // (never)
        if (h[t]) t0 = t < t0 ? t : t0, t1 = t + 1;
        total += h[t];
    }
    *ne = (size_t)total;
    if (total == 0) return hipSuccess;
    if (total & 1) return hipErrorUnknown;  // (never: the flag is 0 at both ends)
    // the tiles [t0, t1) in one copy behind the counts, then compacted to the front
    h.resize(tiles + (size_t)(t1 - t0) * SL_FIND_PART);
    if ((e = hipMemcpyAsync(h.data() + tiles, s.d_pfev + (size_t)t0 * SL_FIND_PART, (size_t)(t1 - t0) * SL_FIND_PART * 4,
                            hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
        return e;
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return e;
    std::vector<u32> edges;
    edges.reserve(total);
    for (u32 t = t0; t < t1; t++) {
        const u32* ev = h.data() + tiles + (size_t)(t - t0) * SL_FIND_PART;
        edges.insert(edges.end(), ev, ev + h[t]);
    }
    for (size_t i = 0; i < edges.size(); i++)
        if (edges[i] > n || (i && edges[i] <= edges[i - 1])) return hipErrorUnknown;  // (never)
    h.swap(edges);
    return hipSuccess;
}

static unsigned sl_part_grid(u64 n, u64 part) {
    const u64 g = (n + part - 1) / part;
    return g < 1 ? 1u : (g > SL_MAX_GRID ? SL_MAX_GRID : (unsigned)g);
}

// One pop step: the n records at [lo, lo + n) are a run of pop records. The plan, its readback (64 bytes
// and a synchronise: whether a buffer flips is known only from it), the entries if a caller asked for
// them, and a shift per run that lost a prefix. Back pops alone copy nothing. After it the host knows nb
// and nd exactly and its bounds are the counts.
static hipError_t sl_pop_step(nrg_ctx* c, const nrg_put* src, bool wring, u64 lo, u64 n, u64 resp_lo, u64 resp_hi,
                              void* d_resp, uint8_t* d_some) {
    SlHost& s = c->sl;
    hipError_t e;
    const SlJob j = sl_pop_job(c, src, wring, lo, n, resp_lo, resp_hi, d_resp, d_some);
    SlPop p{s.front_mark, s.back_mark, s.d_poff, s.d_prank, s.d_pplan, nullptr, 0};
    const bool deliver = s.po_n != nullptr && lo >= s.po_from;
    if (deliver) p.pop_n = s.po_n, p.pop_base = s.po_total;
    NRG_LAUNCH(c, "sl_pop_plan", sl_pop_plan_kernel, 1, SL_SCAN_TPB, 0, c->stream, j, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    u64 pl[SL_PLAN_WORDS];
    if ((e = hipMemcpyAsync(pl, s.d_pplan, sizeof pl, hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return e;
    const u64 f = pl[0], b = pl[1], fb = pl[2], fd = pl[3], bb = pl[4], bd = pl[5], nb = pl[6], nd = pl[7];
    if (nb > s.cap || nd > s.dcap || fb + bb > nb || fd + bd > nd || fb + fd != f || bb + bd != b) return hipErrorUnknown;  // (never)
    if (deliver) {
        const u64 room = s.po_total < s.po_cap ? s.po_cap - s.po_total : 0, cnt = f + b < room ? f + b : room;
        if (cnt)
            NRG_LAUNCH(c, "sl_pop_take", sl_pop_take_kernel, sl_part_grid(cnt, SL_TAKE_PART), SL_TPB, 0, c->stream, j, p,
                       s.po_keys + s.po_total, s.po_vals + s.po_total, cnt);
        s.po_total += f + b;
    }
    if (fb) {
        NRG_LAUNCH(c, "sl_pop_shift", sl_pop_shift_kernel, sl_part_grid(nb - fb - bb, SL_MERGE_PART), SL_TPB, 0, c->stream,
                   (const u64*)s.d_bk[s.bcur], (const u64*)s.d_bv[s.bcur], fb, nb - fb - bb, s.d_bk[s.bcur ^ 1],
                   s.d_bv[s.bcur ^ 1]);
        s.bcur ^= 1;
    }
    if (fd) {
        NRG_LAUNCH(c, "sl_pop_shift", sl_pop_shift_kernel, sl_part_grid(nd - fd - bd, SL_MERGE_PART), SL_TPB, 0, c->stream,
                   (const u64*)s.d_dk[s.dcur], (const u64*)s.d_dv[s.dcur], fd, nd - fd - bd, s.d_dk[s.dcur ^ 1],
                   s.d_dv[s.dcur ^ 1]);
        s.dcur ^= 1;
    }
    s.nd_ub = nd - fd - bd;
    if (c->growth.max_items) c->growth.len_ub = nb + nd - f - b;
    return hipGetLastError();
}

// DsOps::replay. A context without pops: the chunk as it is. With pops the chunk is cut at its pop runs,
// which depend on everything before them: the ordinary stretches between them go through the pipeline
// as chunks of their own (their window, their ring copy), each run is one pop step. A chunk that
// alternates Push and Pop record by record is one segment per record: correct and slow.
static hipError_t sl_replay_chunk(nrg_ctx* c, const void* src, u64 lo, u64 n, u64 resp_lo, u64 resp_hi, void* d_resp,
                                  uint8_t* d_some) {
    const nrg_put* recs = (const nrg_put*)src;
    const bool wring = src != nullptr;
    if (!c->sl.pops || n == 0) return sl_chunk(c, recs, wring, lo, n, resp_lo, resp_hi, d_resp, d_some);
    hipError_t e;
    size_t ne = 0;
    if ((e = sl_pop_find(c, recs, lo, n, &ne)) != hipSuccess) return e;
    if (ne == 0) return sl_chunk(c, recs, wring, lo, n, resp_lo, resp_hi, d_resp, d_some);
    const std::vector<u32> edges(c->sl.h_pf.begin(), c->sl.h_pf.begin() + ne);
    u64 at = 0;
    for (size_t k = 0; k < ne; k += 2) {
        const u64 a = edges[k], b = edges[k + 1];
        if (a > at && (e = sl_chunk(c, recs ? recs + at : nullptr, wring, lo + at, a - at, resp_lo, resp_hi, d_resp,
                                    d_some)) != hipSuccess)
            return e;
        if ((e = sl_pop_step(c, recs ? recs + a : nullptr, wring, lo + a, b - a, resp_lo, resp_hi, d_resp, d_some)) != hipSuccess)
            return e;
        at = b;
    }
    if (at < n) return sl_chunk(c, recs ? recs + at : nullptr, wring, lo + at, n - at, resp_lo, resp_hi, d_resp, d_some);
    return hipSuccess;
}

static void sl_free_delta(SlHost& s) {
    sl_free_pair(s.d_dk);
    sl_free_pair(s.d_dv);
}

static int sl_open(nrg_ctx* c) {
    const nrg_config& cf = c->cfg;
    SlHost& s = c->sl;
    const u64 mb = cf.max_batch;
    // log2_slots: the map holds up to 2^log2_slots keys; max_batch <= 2^24: one workgroup scans a
    // chunk's tile counts
    if (cf.log2_slots < SL_LOG2_MIN || cf.log2_slots > SL_LOG2_MAX || mb > (1ull << 24)) return NRG_E_INVAL;
    s.cap = 1ull << cf.log2_slots;
    s.delta_max = std::min<u64>(s.cap, SL_DELTA_DEFAULT);
    s.dcap = s.delta_max + mb;
    HIPCHK(sl_alloc_runs(s.d_bk, s.d_bv, s.cap));
    HIPCHK(sl_alloc_runs(s.d_dk, s.d_dv, s.dcap));
    HIPCHK(hipMalloc(&s.d_state, sizeof(SlState)));
    HIPCHK(hipMemsetAsync(s.d_state, 0, sizeof(SlState), c->stream));
    HIPCHK(hipMalloc(&s.d_sk, mb * 8));
    HIPCHK(hipMalloc(&s.d_nk, mb * 8));
    HIPCHK(hipMalloc(&s.d_nv, mb * 8));
    HIPCHK(hipMalloc(&s.d_sp, mb * 4));
    HIPCHK(hipMalloc(&s.d_k32, mb * 4));
    HIPCHK(hipMalloc(&s.d_pv, mb * 4));
    HIPCHK(hipMalloc(&s.d_miss, mb));
    HIPCHK(hipMalloc(&s.d_tcnt, ((mb + SL_RES_TILE - 1) / SL_RES_TILE) * 4));
    if (mb > SL_SORT_WG && sort_alloc(c->sort, mb) != NRG_OK) return NRG_E_NOMEM;
    c->pipeline = false;  // config.pipeline is accepted: nothing is deferred
    return NRG_OK;
}

static void sl_close(nrg_ctx* c) {
    SlHost& s = c->sl;
    sl_free_pair(s.d_bk);
    sl_free_pair(s.d_bv);
    sl_free_delta(s);
    void* ptrs[] = {s.d_state, s.d_sk,   s.d_nk,   s.d_nv,   s.d_sp,    s.d_k32,  s.d_pv,
                    s.d_miss,  s.d_tcnt, s.d_kidx, s.d_kcnt, s.d_deadb, s.d_deadd,
                    s.d_pfcnt, s.d_pfev, s.d_poff, s.d_prank, s.d_pplan};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
}

// NRG_KNOB_SL_DELTA_MAX on an empty context: the delta buffers are sized by it
static int sl_set_knob(nrg_ctx* c, int knob, uint64_t v) {
    SlHost& s = c->sl;
    if (knob != NRG_KNOB_SL_DELTA_MAX || v < 1 || v > s.cap) return NRG_E_INVAL;
    SlState st{};
    HIPCHK(sl_read_state(c, &st));
    if (st.nb + st.nd) return NRG_E_INVAL;
    u64 *nk[2], *nv[2];
    HIPCHK(sl_alloc_runs(nk, nv, v + c->cfg.max_batch));
    sl_free_delta(s);
    for (int i = 0; i < 2; i++) s.d_dk[i] = nk[i], s.d_dv[i] = nv[i];
    s.delta_max = v;
    s.dcap = v + c->cfg.max_batch;
    s.nd_ub = 0;
    return NRG_OK;
}

static void sl_defaults(nrg_config* cfg) { cfg->log2_slots = SL_LOG2_DEFAULT; }

// nrg_digest: items are (key, value), the hashmap's definition; a grid-stride over both runs
__global__ __launch_bounds__(DG_TPB) void sl_digest_kernel(const u64* bk, const u64* bv, const u64* dk, const u64* dv,
                                                           const SlState* st, u64* out3) {
    const u64 nb = st->nb, n = nb + st->nd;
    u64 c = 0, sm = 0, x = 0;
    for (u64 i = blockIdx.x * (u64)DG_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * DG_TPB) {
        const u64 h = i < nb ? dg_item(bk[i], bv[i]) : dg_item(dk[i - nb], dv[i - nb]);
        c++;
        sm += h;
        x ^= h;
    }
    dg_commit(c, sm, x, out3);
}

static hipError_t sl_digest(nrg_ctx* c, u64* d_out3) {
    SlHost& s = c->sl;
    hipError_t e = hipMemsetAsync(d_out3, 0, 3 * sizeof(u64), c->stream);
    if (e != hipSuccess) return e;
    NRG_LAUNCH(c, "sl_digest", sl_digest_kernel, dg_grid(s.cap), DG_TPB, 0, c->stream, (const u64*)s.d_bk[s.bcur],
               (const u64*)s.d_bv[s.bcur], (const u64*)s.d_dk[s.dcur], (const u64*)s.d_dv[s.dcur],
               (const SlState*)s.d_state, d_out3);
    return hipGetLastError();
}

static int sl_items(nrg_ctx* c, u64* n) {
    SlState st{};
    HIPCHK(sl_read_state(c, &st));
    *n = st.nb + st.nd;
    return NRG_OK;
}

// The snapshot payload: the merge of the two runs as nrg_put records in ascending key order. The
// image must fit whole or nothing of the payload is stored.
__global__ __launch_bounds__(SL_TPB) void sl_snapshot_kernel(SlMerge m, u64* buf, u64 cap, u64 log_idx, DevCtl* ctl) {
    const u64 na = m.st->nb, nb = m.st->nd;
    if (blockIdx.x == 0 && threadIdx.x == 0) snap_head(buf, cap, NRG_DS_SKIPLIST, na + nb, (na + nb) * 16, log_idx, ctl);
    if (snap_bytes((na + nb) * 16) > cap) return;
    m.orec = (nrg_put*)(buf + SNAP_HDR / 8);
    sl_merge_all<true>(m, na, nb);
}

static hipError_t sl_snapshot(nrg_ctx* c, void* d_buf, u64 cap, u64 log_idx) {
    SlHost& s = c->sl;
    SlMerge m{};
    m.ak = s.d_bk[s.bcur], m.av = s.d_bv[s.bcur], m.bk = s.d_dk[s.dcur], m.bv = s.d_dv[s.dcur];
    m.st = s.d_state;
    NRG_LAUNCH(c, "sl_snapshot", sl_snapshot_kernel, sl_merge_grid(s.cap), SL_TPB, 0, c->stream, m, (u64*)d_buf, cap,
               log_idx, c->d_ctl);
    return hipGetLastError();
}

// The payload into base, delta empty; records out of strictly ascending key order latch ERR_INVAL
// (the digest does not see the order).
__global__ __launch_bounds__(DG_TPB) void sl_restore_kernel(u64* bk, u64* bv, const nrg_put* __restrict__ rec, u64 n,
                                                            SlState* st, DevCtl* ctl) {
    bool bad = false;
    for (u64 i = blockIdx.x * (u64)DG_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * DG_TPB) {
        const nrg_put r = rec[i];
        if (i + 1 < n && rec[i + 1].key <= r.key) bad = true;
        bk[i] = r.key;
        bv[i] = r.val;
    }
    if (bad) atomicOr(&ctl->err, ERR_INVAL);
    if (blockIdx.x == 0 && threadIdx.x == 0) *st = SlState{n, 0, 0, 0};
}

static int sl_restore(nrg_ctx* c, const void* d_payload, u64 items, bool check_only) {
    SlHost& s = c->sl;
    int r;
    if (restore_room(c, d_payload, &items, check_only, &r)) return r;
    NRG_LAUNCH(c, "sl_restore", sl_restore_kernel, dg_grid(items), DG_TPB, 0, c->stream, s.d_bk[s.bcur], s.d_bv[s.bcur],
               (const nrg_put*)d_payload, items, s.d_state, c->d_ctl);
    c->growth.len_ub = items;
    s.nd_ub = 0;
    return hip_fail(hipGetLastError());
}

static u64 sl_capacity(const nrg_ctx* c) { return c->sl.cap; }

bool sl_removal(const nrg_ctx* c) { return c->cfg.ds_kind == NRG_DS_SKIPLIST && c->sl.removal; }

// nrg_skiplist_enable_removal on a drained stream: the scratch of a chunk's removals (sl_close frees
// it, also after a failure half way: the flag is set last)
static int sl_enable_removal(nrg_ctx* c, u64 tombstone) {
    SlHost& s = c->sl;
    const u64 mb = c->cfg.max_batch ? c->cfg.max_batch : 1;
    const u64 tiles = (mb + SL_RES_TILE - 1) / SL_RES_TILE;
    if (!s.d_kidx) HIPCHK(hipMalloc(&s.d_kidx, mb * 4));
    if (!s.d_deadb) HIPCHK(hipMalloc(&s.d_deadb, mb * 4));
    if (!s.d_deadd) HIPCHK(hipMalloc(&s.d_deadd, mb * 4));
    if (!s.d_kcnt) HIPCHK(hipMalloc(&s.d_kcnt, 2 * tiles * 4));
    s.tombstone = tombstone;
    s.removal = true;
    return NRG_OK;
}

bool sl_pops(const nrg_ctx* c) { return c->cfg.ds_kind == NRG_DS_SKIPLIST && c->sl.pops; }

// nrg_skiplist_enable_pops on a drained stream: the scratch of the pop-run search and of a pop step
// (sl_close frees it, also after a failure half way: the flag is set last)
static int sl_enable_pops(nrg_ctx* c, u64 front_mark, u64 back_mark) {
    SlHost& s = c->sl;
    const u64 mb = c->cfg.max_batch ? c->cfg.max_batch : 1;
    const u64 tiles = (mb + 1 + SL_FIND_PART - 1) / SL_FIND_PART;
    if (!s.d_pfcnt) HIPCHK(hipMalloc(&s.d_pfcnt, tiles * 4));
    if (!s.d_pfev) HIPCHK(hipMalloc(&s.d_pfev, tiles * SL_FIND_PART * 4));
    if (!s.d_poff) HIPCHK(hipMalloc(&s.d_poff, (mb + 1) * 8));
    if (!s.d_prank) HIPCHK(hipMalloc(&s.d_prank, mb * 8));
    if (!s.d_pplan) HIPCHK(hipMalloc(&s.d_pplan, SL_PLAN_WORDS * 8));
    try {
        s.h_pf.reserve(tiles);
    } catch (const std::bad_alloc&) {
        return NRG_E_NOMEM;
    }
    s.front_mark = front_mark;
    s.back_mark = back_mark;
    s.pops = true;
    return NRG_OK;
}

const DsOps* sl_ops() {
    static const DsOps ops = {sizeof(nrg_put), sizeof(uint64_t), sl_open, sl_close, nullptr, sl_replay_chunk,
                              floor_ltail, sl_set_knob, nullptr, sl_defaults, sl_digest,
                              sl_items, sl_snapshot, sl_restore, 1ull << SL_LOG2_MAX, sl_capacity, sl_grow, true};
    return &ops;
}

// The keys of [lo, hi] in ascending order into host arrays: the ranks of the window in both runs (one
// launch and a 32-byte copy), then the merge of the two sub-runs into staging.
static int sl_extract(nrg_ctx* c, u64 lo, u64 hi, uint64_t* keys, uint64_t* vals, uint64_t cap, uint64_t* n) {
    SlHost& s = c->sl;
    Staging* g = c->stg;
    int r;
    if ((r = staging(g[3], 64))) return r;
    u64 rk[4] = {0, 0, 0, 0};
    sl_rank_kernel<<<1, 1, 0, c->stream>>>(s.d_bk[s.bcur], s.d_dk[s.dcur], s.d_state, lo, hi, (u64*)g[3].p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rk, g[3].p, sizeof rk, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_all(c));
    const u64 na = rk[1] - rk[0], nb = rk[3] - rk[2];
    *n = na + nb;
    if (*n > cap) return NRG_E_CAPACITY;
    if (*n == 0) return NRG_OK;
    if (!keys || !vals) return NRG_E_INVAL;
    if ((r = staging(g[0], *n * 8)) || (r = staging(g[1], *n * 8))) return r;
    SlMerge m{};
    m.ak = s.d_bk[s.bcur] + rk[0], m.av = s.d_bv[s.bcur] + rk[0], m.na = na;
    m.bk = s.d_dk[s.dcur] + rk[2], m.bv = s.d_dv[s.dcur] + rk[2], m.nb = nb;
    m.ok = (u64*)g[0].p, m.ov = (u64*)g[1].p;
    NRG_LAUNCH(c, "sl_range", sl_merge_kernel, sl_merge_grid(*n), SL_TPB, 0, c->stream, m);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(keys, g[0].p, *n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(vals, g[1].p, *n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_all(c));
    return NRG_OK;
}

// The read kernels for the replica group's group-wide reads (group_reads.cpp): the queries and the answers
// live in the group's scratch, so max_reads (the bound of the entry points' staging) does not apply.
hipError_t sl_seek_launch(nrg_ctx* c, const u64* d_keys, u64 n, u32 mode, u64* d_okeys, u64* d_ovals, uint8_t* d_found) {
    if (n == 0) return hipSuccess;
    if (c->cfg.ds_kind != NRG_DS_SKIPLIST || mode > NRG_SEEK_LT || n >= (1ull << 32)) return hipErrorInvalidValue;
    SlHost& s = c->sl;
    NRG_LAUNCH(c, "sl_seek", sl_seek_kernel, (unsigned)((n + SL_TPB - 1) / SL_TPB), SL_TPB, 0, c->stream,
               (const u64*)s.d_bk[s.bcur], (const u64*)s.d_bv[s.bcur], (const u64*)s.d_dk[s.dcur],
               (const u64*)s.d_dv[s.dcur], (const SlState*)s.d_state, d_keys, n, mode, d_okeys, d_ovals, d_found);
    return hipGetLastError();
}

hipError_t sl_count_launch(nrg_ctx* c, const u64* d_los, const u64* d_his, u64 n, u64* d_counts) {
    if (n == 0) return hipSuccess;
    if (c->cfg.ds_kind != NRG_DS_SKIPLIST || n >= (1ull << 32)) return hipErrorInvalidValue;
    SlHost& s = c->sl;
    NRG_LAUNCH(c, "sl_range_count", sl_range_count_kernel, (unsigned)((n + SL_TPB - 1) / SL_TPB), SL_TPB, 0, c->stream,
               (const u64*)s.d_bk[s.bcur], (const u64*)s.d_dk[s.dcur], (const SlState*)s.d_state, d_los, d_his, n,
               d_counts);
    return hipGetLastError();
}

// The lane group of a scan: the power of two at or above `limit`, up to a wave. A group covers
// `limit` outputs in ceil(limit / width) steps; a narrower group for a small limit leaves no lane
// without an output, and SL_TPB / width queries share a workgroup.
static u32 sl_walk_log2_width(u32 limit) {
    u32 lw = 0;
    while (lw < 6 && (1u << lw) < limit) lw++;
    return lw;
}

hipError_t sl_walk_launch(nrg_ctx* c, const u64* d_keys, u64 n, u32 mode, u32 limit, u64* d_okeys, u64* d_ovals,
                          u32* d_counts) {
    if (n == 0) return hipSuccess;
    if (c->cfg.ds_kind != NRG_DS_SKIPLIST || mode > NRG_SEEK_LT || limit == 0 || limit > NRG_SCAN_MAX_LIMIT ||
        n >= (1ull << 32))
        return hipErrorInvalidValue;
    SlHost& s = c->sl;
    const u32 lw = sl_walk_log2_width(limit);
    const u64 per_wg = (u64)SL_TPB >> lw;  // queries per workgroup
    NRG_LAUNCH(c, "sl_walk", sl_walk_kernel, (unsigned)((n + per_wg - 1) / per_wg), SL_TPB, 0, c->stream,
               (const u64*)s.d_bk[s.bcur], (const u64*)s.d_bv[s.bcur], (const u64*)s.d_dk[s.dcur],
               (const u64*)s.d_dv[s.dcur], (const SlState*)s.d_state, d_keys, n, mode, limit, lw, d_okeys, d_ovals,
               d_counts);
    return hipGetLastError();
}

// A member's candidates of a group-wide pop: its nf smallest entries into fk / fv (ascending) and its nk
// largest into kk / kv (descending), in the group's scratch; nothing is popped and nothing is bounded
// by NRG_SCAN_MAX_LIMIT or max_reads.
hipError_t sl_peek_launch(nrg_ctx* c, u64 nf, u64 nk, u64* d_fk, u64* d_fv, u64* d_kk, u64* d_kv) {
    if (nf + nk == 0) return hipSuccess;
    if (c->cfg.ds_kind != NRG_DS_SKIPLIST || nf > c->sl.cap || nk > c->sl.cap) return hipErrorInvalidValue;
    SlHost& s = c->sl;
    const u64 blocks = (nf + nk + SL_TPB - 1) / SL_TPB;
    NRG_LAUNCH(c, "sl_peek", sl_peek_kernel, (unsigned)(blocks < 4096 ? blocks : 4096), SL_TPB, 0, c->stream,
               (const u64*)s.d_bk[s.bcur], (const u64*)s.d_bv[s.bcur], (const u64*)s.d_dk[s.dcur],
               (const u64*)s.d_dv[s.dcur], (const SlState*)s.d_state, nf, nk, d_fk, d_fv, d_kk, d_kv);
    return hipGetLastError();
}

// SkipListWrapper::default restricted to a partition: of the keys k0 .. k0 + n - 1, the records of
// those `part` owns (nrg_key_owner), compacted into `out` in no particular order (the keys are
// distinct and the chunk sorts them); *cnt, zero before the launch, receives their number. One
// atomic per wave: the lanes that own their key take consecutive places from the wave's base.
__global__ __launch_bounds__(SL_TPB) void sl_gen_part_kernel(nrg_put* out, u64 k0, u64 n, u64 off, u32 part, u32 parts,
                                                             u32* cnt) {
    const u64 i = (u64)blockIdx.x * SL_TPB + threadIdx.x;
    const bool mine = i < n && key_owner(k0 + i, parts) == part;
    const u64 b = __ballot(mine);
    if (b == 0) return;
    const u32 lane = threadIdx.x & 63;
    u32 base = 0;
    if (lane == (u32)__ffsll((unsigned long long)b) - 1) base = atomicAdd(cnt, (u32)__popcll(b));
    base = __shfl(base, __ffsll((unsigned long long)b) - 1);
    if (mine) out[base + (u32)__popcll(b & ((1ull << lane) - 1))] = nrg_put{k0 + i, k0 + i + off};
}

}  // namespace nrg

// ---- the skip list's entry points (include/nrgpu.h) ------------------------------------------------
using namespace nrg;

extern "C" {

int nrg_skiplist_round_async(nrg_ctx* c, const nrg_put* d_ops, uint64_t n, uint32_t origin, uint64_t* d_resp,
                             uint8_t* d_some) {
    return round_common(c, NRG_DS_SKIPLIST, d_ops, n, origin, d_resp, d_some);
}

// the checks every read shares (nrg_vspace_resolve's)
static int sl_read_check(nrg_ctx* c, uint64_t n) {
    int r = need(c, NRG_DS_SKIPLIST);
    if (r) return r;
    if (c->ltail != c->tail) return NRG_E_NOT_SYNCED;
    if (n > c->cfg.max_reads) return NRG_E_CAPACITY;
    return NRG_OK;
}

int nrg_skiplist_get_async(nrg_ctx* c, const uint64_t* d_keys, uint64_t n, uint64_t* d_vals, uint8_t* d_found) {
    int r = sl_read_check(c, n);
    if (r) return r;
    if (n == 0) return NRG_OK;
    if (!d_keys || !d_vals || !d_found) return NRG_E_INVAL;
    SlHost& s = c->sl;
    NRG_LAUNCH(c, "sl_get", sl_get_kernel, (unsigned)((n + SL_TPB - 1) / SL_TPB), SL_TPB, 0, c->stream,
               (const u64*)s.d_bk[s.bcur], (const u64*)s.d_bv[s.bcur], (const u64*)s.d_dk[s.dcur],
               (const u64*)s.d_dv[s.dcur], (const SlState*)s.d_state, d_keys, n, d_vals, d_found);
    return hip_fail(hipGetLastError());
}

int nrg_skiplist_get(nrg_ctx* c, const uint64_t* keys, uint64_t n, uint64_t* vals, uint8_t* found) {
    int r = sl_read_check(c, n);
    if (r) return r;
    if (n == 0) return NRG_OK;
    if (!keys || !vals || !found) return NRG_E_INVAL;
    Staging* g = c->stg;
    if ((r = staging(g[0], n * 8)) || (r = staging(g[1], n * 8)) || (r = staging(g[2], n))) return r;
    HIPCHK(hipMemcpyAsync(g[0].p, keys, n * 8, hipMemcpyHostToDevice, c->stream));
    if ((r = nrg_skiplist_get_async(c, (u64*)g[0].p, n, (u64*)g[1].p, (uint8_t*)g[2].p))) return r;
    HIPCHK(hipMemcpyAsync(vals, g[1].p, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(found, g[2].p, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_all(c));
    return check_err(c);
}

int nrg_skiplist_seek_async(nrg_ctx* c, const uint64_t* d_keys, uint64_t n, uint32_t mode, uint64_t* d_out_keys,
                            uint64_t* d_out_vals, uint8_t* d_found) {
    int r = sl_read_check(c, n);
    if (r) return r;
    if (mode > NRG_SEEK_LT) return NRG_E_INVAL;
    if (n == 0) return NRG_OK;
    if (!d_keys || !d_out_keys || !d_out_vals || !d_found) return NRG_E_INVAL;
    SlHost& s = c->sl;
    NRG_LAUNCH(c, "sl_seek", sl_seek_kernel, (unsigned)((n + SL_TPB - 1) / SL_TPB), SL_TPB, 0, c->stream,
               (const u64*)s.d_bk[s.bcur], (const u64*)s.d_bv[s.bcur], (const u64*)s.d_dk[s.dcur],
               (const u64*)s.d_dv[s.dcur], (const SlState*)s.d_state, d_keys, n, mode, d_out_keys, d_out_vals,
               d_found);
    return hip_fail(hipGetLastError());
}

int nrg_skiplist_seek(nrg_ctx* c, const uint64_t* keys, uint64_t n, uint32_t mode, uint64_t* out_keys,
                      uint64_t* out_vals, uint8_t* found) {
    int r = sl_read_check(c, n);
    if (r) return r;
    if (mode > NRG_SEEK_LT) return NRG_E_INVAL;
    if (n == 0) return NRG_OK;
    if (!keys || !out_keys || !out_vals || !found) return NRG_E_INVAL;
    Staging* g = c->stg;
    // keys, then out_keys behind them in one slot; values; found
    if ((r = staging(g[0], 2 * n * 8)) || (r = staging(g[1], n * 8)) || (r = staging(g[2], n))) return r;
    u64* dk = (u64*)g[0].p;
    HIPCHK(hipMemcpyAsync(dk, keys, n * 8, hipMemcpyHostToDevice, c->stream));
    if ((r = nrg_skiplist_seek_async(c, dk, n, mode, dk + n, (u64*)g[1].p, (uint8_t*)g[2].p))) return r;
    HIPCHK(hipMemcpyAsync(out_keys, dk + n, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out_vals, g[1].p, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(found, g[2].p, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_all(c));
    return check_err(c);
}

int nrg_skiplist_scan_async(nrg_ctx* c, const uint64_t* d_keys, uint64_t n, uint32_t mode, uint32_t limit,
                            uint64_t* d_out_keys, uint64_t* d_out_vals, uint32_t* d_counts) {
    int r = sl_read_check(c, n);
    if (r) return r;
    if (mode > NRG_SEEK_LT || limit == 0 || limit > NRG_SCAN_MAX_LIMIT) return NRG_E_INVAL;
    if (n == 0) return NRG_OK;
    if (!d_keys || !d_out_keys || !d_out_vals || !d_counts) return NRG_E_INVAL;
    return hip_fail(sl_walk_launch(c, d_keys, n, mode, limit, d_out_keys, d_out_vals, d_counts));
}

int nrg_skiplist_scan(nrg_ctx* c, const uint64_t* keys, uint64_t n, uint32_t mode, uint32_t limit, uint64_t* out_keys,
                      uint64_t* out_vals, uint32_t* counts) {
    int r = sl_read_check(c, n);
    if (r) return r;
    if (mode > NRG_SEEK_LT || limit == 0 || limit > NRG_SCAN_MAX_LIMIT) return NRG_E_INVAL;
    if (n == 0) return NRG_OK;
    if (!keys || !out_keys || !out_vals || !counts) return NRG_E_INVAL;
    const uint64_t slots = n * limit;  // (n <= max_reads < 2^54: no wrap)
    if (slots > (1ull << 24)) return NRG_E_CAPACITY;  // the staging's size
    // the device writes only the slots below each count, and so does this call: the entries come
    // back through host copies of the staging and only the written ones reach the caller's arrays
    std::vector<uint64_t> hk, hv;
    try {
        hk.resize(slots);
        hv.resize(slots);
    } catch (const std::bad_alloc&) {
        return NRG_E_NOMEM;
    }
    Staging* g = c->stg;
    // keys, then out_keys behind them in one slot; values; counts
    if ((r = staging(g[0], (n + slots) * 8)) || (r = staging(g[1], slots * 8)) || (r = staging(g[2], n * 4))) return r;
    u64* dk = (u64*)g[0].p;
    HIPCHK(hipMemcpyAsync(dk, keys, n * 8, hipMemcpyHostToDevice, c->stream));
    if ((r = nrg_skiplist_scan_async(c, dk, n, mode, limit, dk + n, (u64*)g[1].p, (u32*)g[2].p))) return r;
    HIPCHK(hipMemcpyAsync(hk.data(), dk + n, slots * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(hv.data(), g[1].p, slots * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(counts, g[2].p, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_all(c));
    if ((r = check_err(c))) return r;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t cnt = counts[i] < limit ? counts[i] : limit;
        std::memcpy(out_keys + i * limit, hk.data() + i * limit, cnt * 8);
        std::memcpy(out_vals + i * limit, hv.data() + i * limit, cnt * 8);
    }
    return NRG_OK;
}

int nrg_skiplist_range_count_async(nrg_ctx* c, const uint64_t* d_los, const uint64_t* d_his, uint64_t n,
                                   uint64_t* d_counts) {
    int r = sl_read_check(c, n);
    if (r) return r;
    if (n == 0) return NRG_OK;
    if (!d_los || !d_his || !d_counts) return NRG_E_INVAL;
    SlHost& s = c->sl;
    NRG_LAUNCH(c, "sl_range_count", sl_range_count_kernel, (unsigned)((n + SL_TPB - 1) / SL_TPB), SL_TPB, 0, c->stream,
               (const u64*)s.d_bk[s.bcur], (const u64*)s.d_dk[s.dcur], (const SlState*)s.d_state, d_los, d_his, n,
               d_counts);
    return hip_fail(hipGetLastError());
}

int nrg_skiplist_range_count(nrg_ctx* c, const uint64_t* los, const uint64_t* his, uint64_t n, uint64_t* counts) {
    int r = sl_read_check(c, n);
    if (r) return r;
    if (n == 0) return NRG_OK;
    if (!los || !his || !counts) return NRG_E_INVAL;
    Staging* g = c->stg;
    if ((r = staging(g[0], n * 8)) || (r = staging(g[1], n * 8)) || (r = staging(g[2], n * 8))) return r;
    HIPCHK(hipMemcpyAsync(g[0].p, los, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(g[1].p, his, n * 8, hipMemcpyHostToDevice, c->stream));
    if ((r = nrg_skiplist_range_count_async(c, (u64*)g[0].p, (u64*)g[1].p, n, (u64*)g[2].p))) return r;
    HIPCHK(hipMemcpyAsync(counts, g[2].p, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_all(c));
    return check_err(c);
}

int nrg_skiplist_range(nrg_ctx* c, uint64_t lo, uint64_t hi, uint64_t* keys, uint64_t* vals, uint64_t cap,
                       uint64_t* n) {
    int r = need(c, NRG_DS_SKIPLIST);
    if (r) return r;
    if (!n) return NRG_E_INVAL;
    if (c->ltail != c->tail) return NRG_E_NOT_SYNCED;
    return sl_extract(c, lo, hi, keys, vals, cap, n);
}

int nrg_skiplist_dump(nrg_ctx* c, uint64_t* keys, uint64_t* vals, uint64_t cap, uint64_t* n) {
    int r = need(c, NRG_DS_SKIPLIST);
    if (r) return r;
    if (!n) return NRG_E_INVAL;
    return sl_extract(c, 0, ~0ull, keys, vals, cap, n);
}

int nrg_skiplist_len(nrg_ctx* c, uint64_t* n) {
    int r = need(c, NRG_DS_SKIPLIST);
    if (r) return r;
    if (!n) return NRG_E_INVAL;
    SlState st{};
    HIPCHK(sl_read_state(c, &st));
    *n = st.nb + st.nd;
    return check_err(c);
}

int nrg_skiplist_prefill(nrg_ctx* c, const uint64_t* keys, const uint64_t* vals, uint64_t n) {
    int r = need(c, NRG_DS_SKIPLIST);
    if (r) return r;
    if (n && (!keys || !vals)) return NRG_E_INVAL;
    const uint64_t mb = c->cfg.max_batch;
    std::vector<nrg_put> recs;
    try {
        recs.resize(n < mb ? n : mb);
    } catch (const std::bad_alloc&) {
        return NRG_E_NOMEM;
    }
    // the replay pipeline without a log position: later records win, as in a replay
    for (uint64_t at = 0; at < n; at += mb) {
        const uint64_t m = n - at < mb ? n - at : mb;
        for (uint64_t i = 0; i < m; i++) recs[i] = nrg_put{keys[at + i], vals[at + i]};
        if ((r = staging(c->stg[0], m * sizeof(nrg_put)))) return r;
        HIPCHK(hipMemcpyAsync(c->stg[0].p, recs.data(), m * sizeof(nrg_put), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));  // (recs is filled again)
        HIPCHK(sl_chunk(c, (const nrg_put*)c->stg[0].p, false, 0, m, 0, 0, nullptr, nullptr));
    }
    HIPCHK(sync_all(c));
    return check_err(c);
}

int nrg_skiplist_prefill_range(nrg_ctx* c, uint64_t n, uint64_t val_offset) {
    int r = need(c, NRG_DS_SKIPLIST);
    if (r) return r;
    const uint64_t mb = c->cfg.max_batch;
    for (uint64_t at = 0; at < n; at += mb) {
        const uint64_t m = n - at < mb ? n - at : mb;
        if ((r = staging(c->stg[0], m * sizeof(nrg_put)))) return r;
        sl_gen_kernel<<<(unsigned)((m + SL_TPB - 1) / SL_TPB), SL_TPB, 0, c->stream>>>((nrg_put*)c->stg[0].p, at, m,
                                                                                      val_offset);
        HIPCHK(hipGetLastError());
        HIPCHK(sl_chunk(c, (const nrg_put*)c->stg[0].p, false, 0, m, 0, 0, nullptr, nullptr));
    }
    HIPCHK(sync_all(c));
    return check_err(c);
}

int nrg_skiplist_prefill_partition(nrg_ctx* c, uint64_t n, uint64_t val_offset, uint32_t part, uint32_t parts) {
    int r = need(c, NRG_DS_SKIPLIST);
    if (r) return r;
    if (parts == 0 || parts > NRG_MAX_PARTS || part >= parts) return NRG_E_INVAL;
    const uint64_t mb = c->cfg.max_batch;
    if ((r = staging(c->stg[3], 64))) return r;
    u32* d_cnt = (u32*)c->stg[3].p;
    // a slice of max_batch keys at a time: its owned records compacted on the device, their number
    // read back (the call is synchronous anyway), and that many handed to the chunk path, which
    // accounts them for growth as any prefill's
    for (uint64_t at = 0; at < n; at += mb) {
        const uint64_t m = n - at < mb ? n - at : mb;
        if ((r = staging(c->stg[0], m * sizeof(nrg_put)))) return r;
        HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(u32), c->stream));
        sl_gen_part_kernel<<<(unsigned)((m + SL_TPB - 1) / SL_TPB), SL_TPB, 0, c->stream>>>((nrg_put*)c->stg[0].p, at, m,
                                                                                           val_offset, part, parts, d_cnt);
        HIPCHK(hipGetLastError());
        u32 owned = 0;
        HIPCHK(hipMemcpyAsync(&owned, d_cnt, sizeof owned, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (owned > m) return NRG_E_HIP;  // (cannot happen: a slice owns at most its keys)
        HIPCHK(sl_chunk(c, (const nrg_put*)c->stg[0].p, false, 0, owned, 0, 0, nullptr, nullptr));
    }
    HIPCHK(sync_all(c));
    return check_err(c);
}

int nrg_skiplist_enable_removal(nrg_ctx* c, uint64_t tombstone) {
    int r = need(c, NRG_DS_SKIPLIST);
    if (r) return r;
    if (c->sl.removal) return tombstone == c->sl.tombstone ? NRG_OK : NRG_E_INVAL;
    if (c->sl.pops && (tombstone == c->sl.front_mark || tombstone == c->sl.back_mark)) return NRG_E_INVAL;
    if (c->ltail != c->tail) return NRG_E_NOT_SYNCED;
    HIPCHK(sync_all(c));
    return sl_enable_removal(c, tombstone);
}

int nrg_skiplist_removal(nrg_ctx* c, uint64_t* tombstone, int* enabled) {  // no device is touched
    if (!c || c->cfg.ds_kind != NRG_DS_SKIPLIST) return NRG_E_INVAL;
    if (tombstone) *tombstone = c->sl.removal ? c->sl.tombstone : 0;
    if (enabled) *enabled = c->sl.removal ? 1 : 0;
    return NRG_OK;
}

int nrg_skiplist_enable_pops(nrg_ctx* c, uint64_t front_mark, uint64_t back_mark) {
    int r = need(c, NRG_DS_SKIPLIST);
    if (r) return r;
    SlHost& s = c->sl;
    if (s.pops) return front_mark == s.front_mark && back_mark == s.back_mark ? NRG_OK : NRG_E_INVAL;
    if (front_mark == back_mark || (s.removal && (front_mark == s.tombstone || back_mark == s.tombstone))) return NRG_E_INVAL;
    if (c->ltail != c->tail) return NRG_E_NOT_SYNCED;
    HIPCHK(sync_all(c));
    return sl_enable_pops(c, front_mark, back_mark);
}

int nrg_skiplist_pops(nrg_ctx* c, uint64_t* front_mark, uint64_t* back_mark, int* enabled) {  // no device is touched
    if (!c || c->cfg.ds_kind != NRG_DS_SKIPLIST) return NRG_E_INVAL;
    if (front_mark) *front_mark = c->sl.pops ? c->sl.front_mark : 0;
    if (back_mark) *back_mark = c->sl.pops ? c->sl.back_mark : 0;
    if (enabled) *enabled = c->sl.pops ? 1 : 0;
    return NRG_OK;
}

int nrg_skiplist_round_pops_async(nrg_ctx* c, const nrg_put* d_ops, uint64_t n, uint32_t origin, uint64_t* d_resp,
                                  uint8_t* d_some, uint64_t* d_pop_keys, uint64_t* d_pop_vals, uint64_t pop_cap,
                                  uint64_t* d_pop_n) {
    int r = need(c, NRG_DS_SKIPLIST);
    if (r) return r;
    SlHost& s = c->sl;
    if (!s.pops || !d_pop_n || (pop_cap && (!d_pop_keys || !d_pop_vals))) return NRG_E_INVAL;
    if (n > c->cfg.max_batch) return NRG_E_CAPACITY;  // (before anything is queued)
    HIPCHK(hipMemsetAsync(d_pop_n, 0, sizeof(uint64_t), c->stream));
    // the batch goes to the log's tail: what the round replays ahead of it (others' records) delivers nothing
    s.po_keys = d_pop_keys, s.po_vals = d_pop_vals, s.po_n = d_pop_n;
    s.po_cap = pop_cap, s.po_from = c->tail, s.po_total = 0;
    r = round_common(c, NRG_DS_SKIPLIST, d_ops, n, origin, d_resp, d_some);
    s.po_keys = s.po_vals = s.po_n = nullptr;
    return r;
}

int nrg_skiplist_pop(nrg_ctx* c, int back, uint64_t n, uint32_t origin, uint64_t* keys, uint64_t* vals, uint64_t* m) {
    int r = need(c, NRG_DS_SKIPLIST);
    if (r) return r;
    SlHost& s = c->sl;
    if (!s.pops || !m) return NRG_E_INVAL;
    // what the log holds is replayed first: the record can pop no more than the map then has
    if ((r = exec_range(c, 0, 0, nullptr, nullptr))) return r;
    SlState st{};
    HIPCHK(sl_read_state(c, &st));
    const uint64_t cap = n < st.nb + st.nd ? n : st.nb + st.nd;
    if (cap && (!keys || !vals)) return NRG_E_INVAL;
    Staging* g = c->stg;
    if ((r = staging(g[0], 64)) || (r = staging(g[1], cap * 8)) || (r = staging(g[2], cap * 8))) return r;
    // the record, its response and some byte, and the entries' number in one slot
    char* d = (char*)g[0].p;
    const nrg_put rec{n, back ? s.back_mark : s.front_mark};
    HIPCHK(hipMemcpyAsync(d, &rec, sizeof rec, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));  // (rec leaves the stack)
    if ((r = nrg_skiplist_round_pops_async(c, (const nrg_put*)d, 1, origin, (u64*)(d + 16), (uint8_t*)(d + 24), (u64*)g[1].p,
                                           (u64*)g[2].p, cap, (u64*)(d + 32))))
        return r;
    uint64_t got = 0;
    HIPCHK(hipMemcpyAsync(&got, d + 32, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_all(c));
    if (got > cap) return NRG_E_HIP;  // (never: a record pops at most min(n, len))
    if (got) {
        HIPCHK(hipMemcpyAsync(keys, g[1].p, got * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(vals, g[2].p, got * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(sync_all(c));
    }
    *m = got;
    return check_err(c);
}

int nrg_skiplist_reserve(nrg_ctx* c, uint64_t n_keys) { return reserve_common(c, NRG_DS_SKIPLIST, n_keys); }

int nrg_skiplist_capacity(nrg_ctx* c, uint64_t* n) { return capacity_common(c, NRG_DS_SKIPLIST, n); }

}  // extern "C"
