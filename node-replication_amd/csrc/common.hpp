// common.hpp — shared device/host definitions for the nrgpu HIP kernels (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nrg {

typedef uint64_t u64;
typedef unsigned int u32;
typedef unsigned short u16;

// Empty-slot marker of the open-addressing tables. Keys span all of u64 (key 0 is used by
// benches/hashmap.rs:95-96,150), so the one key equal to the marker lives in a side slot
// (DevCtl::sp), giving the full HashMap<u64,u64> key domain (SURVEY.md §7 "Sentinels").
constexpr u64 EMPTY_KEY = ~0ull;

// Device error bits latched in DevCtl::err and reported by nrg_sync.
constexpr u32 ERR_TABLE_FULL = 1u;
constexpr u32 ERR_CAPACITY = 4u;
constexpr u32 ERR_INVAL = 16u;  // a log record outside its structure's domain (vspace.hip)
constexpr u32 ERR_GROUP = 8u;  // a replica group's ranks disagreed on a round's segment lengths (group.cpp)

// Counters of keys created by replay rounds (claiming blocks add to slot blk % HM_CREATED_SLOTS).
constexpr u64 HM_CREATED_SLOTS = 8192;
// Counters of Puts combined inside their index block (key skew statistic, hm_dup_sample_kernel).
constexpr u64 HM_DUP_SLOTS = 64;
// Slot buckets of a partition round (hashmap.hip part_role / hm_papply_kernel): at most this many.
constexpr u32 HM_BK_MAX = 1024;
// Largest hashmap replay chunk: keeps the partition apply's per-tile LDS prefix (one u32 + one
// u16 per tile of 2048 Puts) and 16-bit tile offsets within bounds.
constexpr u64 HM_MAX_BATCH = 1ull << 23;
// Table growth (nrg_config.hashmap_max_log2_slots, nrg_hashmap_reserve): a table of S slots that
// growth manages holds at most S / HM_GROW_SLOTS_PER_KEY keys, a load of 0.5. A Get reads its key's
// home group (a 128-B line of 4 slots, probe_slot below) and goes on to the next group only when
// that one is full and does not hold the key; every further group is another random line, and
// random lines are what the read role's time is made of. With uniform homes (a sequential model of
// 2^20 slots): at a = 0.5 16 % of the groups are full, a hit reads 1.05 groups and a miss 1.23; at
// a = 0.75 49 % are full, a hit reads 1.27 and a miss 2.69.
constexpr u64 HM_GROW_SLOTS_PER_KEY = 2;

// splitmix64 finaliser — identical constants to oracle/nr_oracle.c (orc_mix64) so that
// device-generated workloads are reproducible by the CPU oracle.
__host__ __device__ __forceinline__ u64 mix64(u64 z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ u64 sm64_at(u64 seed, u64 i) {
    return mix64(seed + (i + 1) * 0x9E3779B97F4A7C15ull);
}
__device__ __forceinline__ u64 mulhi64(u64 a, u64 b) { return __umul64hi(a, b); }

// Owner of a key among `parts` key partitions (partition.hip): the low 32 bits of the mixed key
// scaled to [0, parts), independent of the home-slot bits below.
constexpr u32 PT_MAX_PARTS = 64;
__host__ __device__ __forceinline__ u32 key_owner(u64 key, u32 parts) {
    return (u32)(((mix64(key) & 0xFFFFFFFFull) * parts) >> 32);
}

// Owner of a file among `parts` file partitions (nrg_memfs_owner; benches/nrfs.rs:25-39 LogMapper::hash
// = fd - 1, cnr/src/replica.rs:435 hash % logs): the file index modulo parts; an ino below the first
// file belongs to owner 0. (Almost every index fits 32 bits: the 64-bit remainder is the rare arm.)
constexpr u64 MF_FIRST_INO = 5;  // NRG_MEMFS_FIRST_INO
__host__ __device__ __forceinline__ u32 file_owner(u64 ino, u32 parts) {
    if (ino < MF_FIRST_INO) return 0u;
    const u64 f = ino - MF_FIRST_INO;
    return (f >> 32) == 0 ? (u32)f % parts : (u32)(f % parts);
}

// Home slot of a key: top bits of the mixed key.
__device__ __forceinline__ u64 table_home(u64 key, u32 shift) { return mix64(key) >> shift; }

// The probe sequence of a key with home slot `home`, p = 0, 1, 2, ...: round the home's group of four
// slots (one 128-B line) from the home slot on, then round the next group from the same offset, and so
// on, wrapping at the table's end. It is a function of the key alone, every walk of a chain goes
// through it, and no key is ever deleted (a full group stays full): a key that is removed
// (nrg_hashmap_enable_removal) keeps its slot, which is marked dead and still holds the key, until a
// rehash builds a new table without it. So a present key lies in the first
// group of its sequence that had an empty slot when the key was inserted: a reader that sees a group
// with an empty slot and no match has its answer, absent, without looking at a later group.
__host__ __device__ constexpr u64 probe_slot(u64 home, u64 p, u64 tmask) {
    return ((((home >> 2) + (p >> 2)) << 2) | ((home + p) & 3)) & tmask;
}
// The same sequence one step at a time, for walks that keep the slot and not the home: slot p + 1 of
// the sequence whose slot p is s (the next slot of s's group, or of the following group after every
// fourth step).
__host__ __device__ constexpr u64 probe_next(u64 s, u64 p, u64 tmask) {
    return probe_slot(s, ((p + 1) & 3) ? 1 : 5, tmask);
}
namespace probe_check {
// p = 0 .. slots-1 visits every slot exactly once from every home, p = 0 .. 3 stays in the home's group,
// and probe_next walks the same sequence
constexpr bool covers(u64 slots) {
    for (u64 home = 0; home < slots; home++) {
        u64 seen = 0;
        for (u64 p = 0; p < slots; p++) {
            const u64 s = probe_slot(home, p, slots - 1);
            if (s >= slots || ((seen >> s) & 1)) return false;
            if (p < 4 && (s >> 2) != (home >> 2)) return false;
            if (probe_next(s, p, slots - 1) != probe_slot(home, p + 1, slots - 1)) return false;
            seen |= 1ull << s;
        }
    }
    return true;
}
static_assert(probe_slot(6, 0, 15) == 6 && probe_slot(6, 1, 15) == 7 && probe_slot(6, 2, 15) == 4 &&
                  probe_slot(6, 3, 15) == 5 && probe_slot(6, 4, 15) == 10 && probe_slot(14, 5, 15) == 3,
              "round the home group from the home slot, then the next group from the same offset, wrapping");
static_assert(covers(16), "a 16-slot table: every slot once from every home, the first four in the home group");
static_assert(covers(64), "a 64-slot table: every slot once from every home, the first four in the home group");
}  // namespace probe_check

// 32-byte table slot, four per 128-B line (2^26 slots = 2 GiB). A random read costs one 128-B
// line at the memory side whatever its width (profiles/r01_rdreq_size.txt), so the replay's
// per-key bookkeeping rides in the key's line: a Get reads {key, val} and the stamp of its
// round's parity, two 16-B loads of one line.
//   st[p]  stamp of the last round of parity p that wrote or created the key:
//          epoch << 32 | (i+1) for the round's last writer (raised with atomicMax), or
//          epoch << 32 | 0 as the mark a round leaves in the OTHER parity when it creates the key.
//          0 = never stamped: a slot whose claim is still in flight reads as absent.
// Epoch 1 means "present since before any replay round" (prefill, bucket-round claims); replay
// rounds take epochs 2, 3, ... and are renormalised before the 32-bit epoch wraps.
// A Get of round ep reads st[ep & 1]:  0 or epoch > ep -> absent (created by a later round);
// epoch == ep -> the round's last writer (its record); epoch < ep -> present, value in `val`.
struct __attribute__((aligned(32))) Slot {
    u64 key;  // EMPTY_KEY when free
    u64 val;
    u64 st[2];
};
__host__ __device__ __forceinline__ u64 stamp_make(u32 epoch, u64 i1) { return ((u64)epoch << 32) | i1; }
__host__ __device__ __forceinline__ u32 stamp_epoch(u64 st) { return (u32)(st >> 32); }
constexpr u64 STAMP_PRESENT = 1ull << 32;  // epoch 1, no writer: present since before the replay rounds

// One replica-wide control block in HBM.
struct __attribute__((aligned(64))) DevCtl {
    u32 err;          // latched ERR_* bits
    u32 sp_claim;     // hashmap: the key EMPTY_KEY has been inserted (its slot is `sp`)
    u64 nkeys;        // hashmap: keys inserted directly (prefill)
    long long depth;  // stack: current length
    u64 counter;      // scratch counter (dump compaction)
    u64 nkeys_total;  // hashmap: nkeys + keys created by replay rounds (hm_count)
    long long depth0;      // stack: length after the last chunk of buffer parity 0 (stack.hip)
    long long depth_next;  // stack: ... of parity 1; a chunk starts from the other parity's slot
    u64 pad;
    Slot sp;          // hashmap: side slot of the key EMPTY_KEY (val, stamps; key unused)
    u64 occ_total;    // hashmap with removal: slots taken, live and dead (hm_count; nkeys_total is the live ones)
};

__device__ __forceinline__ u64 ld_relaxed(const u64* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ u32 ld_relaxed32(const u32* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Test-only stall (NRG_KNOB_STALL): odd waves sleep ~30 us at a point where the workgroup's
// waves next reuse LDS another wave may still read, so a missing barrier shows up as a wrong
// result instead of a rare timing accident.
__device__ __forceinline__ void test_stall(u32 on, int wave) {
    if (on && (wave & 1))
        for (int i = 0; i < 32; i++) __builtin_amdgcn_s_sleep(127);
}

// The state digest (nrg_digest, Replica::verify nr/src/replica.rs:443-467): {count, sum, xor} of
// dg_item(k, v) over a structure's items; (k, v) per kind is in include/nrgpu.h. Every kind's
// digest kernel runs workgroups of DG_TPB lanes and ends in dg_commit.
constexpr int DG_TPB = 256;
constexpr u32 DG_MAX_GRID = 1024;
__host__ __device__ __forceinline__ u64 dg_item(u64 k, u64 v) { return mix64(k ^ mix64(v)); }
// workgroups of a grid-stride digest over at most `items` items
inline u32 dg_grid(u64 items) {
    const u64 g = (items + DG_TPB - 1) / DG_TPB;
    return g < 1 ? 1u : (g > DG_MAX_GRID ? DG_MAX_GRID : (u32)g);
}
// workgroups of a grid-stride copy of `units` lane-sized units (the growth kernels): up to eight
// per CU, the rest by stride
inline u32 copy_grid(u64 units) {
    const u64 g = (units + DG_TPB - 1) / DG_TPB;
    return g < 1 ? 1u : (g > 2048 ? 2048u : (u32)g);
}
// Every lane's partial triple, reduced per wave, then per workgroup, then added into out3 (zeroed
// earlier in stream order) with one set of atomics per workgroup that found anything.
__device__ __forceinline__ void dg_commit(u64 c, u64 sm, u64 x, u64* out3) {
    __shared__ u64 s_dg[3][DG_TPB / 64];
    for (int off = 32; off > 0; off >>= 1) {
        c += __shfl_xor(c, off, 64);
        sm += __shfl_xor(sm, off, 64);
        x ^= __shfl_xor(x, off, 64);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_dg[0][w] = c;
        s_dg[1][w] = sm;
        s_dg[2][w] = x;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        c = sm = x = 0;
        for (int v = 0; v < DG_TPB / 64; v++) {
            c += s_dg[0][v];
            sm += s_dg[1][v];
            x ^= s_dg[2][v];
        }
        if (c) {
            atomicAdd(&out3[0], c);
            atomicAdd(&out3[1], sm);
            atomicXor(&out3[2], x);
        }
    }
}

// The snapshot image (nrg_snapshot_async / nrg_restore, include/nrgpu.h): a 64-byte header of eight
// u64 words {magic, kind | version << 32, items, bytes, log_idx, digest[3]} and the kind's payload,
// the whole rounded up to a multiple of 64 bytes with the padding zeroed.
constexpr u64 SNAP_MAGIC = 0x3150414E5347524Eull;  // the ASCII bytes "NRGSNAP1", little endian
constexpr u32 SNAP_VERSION = 1;
constexpr u64 SNAP_HDR = 64;
__host__ __device__ __forceinline__ u64 snap_bytes(u64 payload) { return (SNAP_HDR + payload + 63) & ~63ull; }
// One thread of a snapshot kernel, for a payload of `payload` bytes (a multiple of 4): header words
// 0..4 and the zeroed padding when the image fits into cap bytes (the digest fills words 5..7
// afterwards); else magic = 0 where the header itself fits, and ERR_CAPACITY. Nothing is stored
// at or past buf + cap either way.
__device__ __forceinline__ void snap_head(u64* buf, u64 cap, u32 kind, u64 items, u64 payload, u64 log_idx,
                                          DevCtl* ctl) {
    const u64 bytes = snap_bytes(payload);
    if (bytes > cap) {
        if (cap >= SNAP_HDR) buf[0] = 0;
        atomicOr(&ctl->err, ERR_CAPACITY);
        return;
    }
    buf[0] = SNAP_MAGIC;
    buf[1] = (u64)kind | ((u64)SNAP_VERSION << 32);
    buf[2] = items;
    buf[3] = bytes;
    buf[4] = log_idx;
    u32* pad = (u32*)((char*)buf + SNAP_HDR + payload);
    for (u64 i = 0; i < (bytes - SNAP_HDR - payload) / 4; i++) pad[i] = 0;
}

// Wave-wide (64-lane) inclusive scan helpers.
__device__ __forceinline__ u32 lane_id() { return threadIdx.x & 63; }

}  // namespace nrg
