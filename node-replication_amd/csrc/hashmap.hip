// hashmap.hip — NrHashMap replica replay on gfx950.
//
// Replaces the hot loop of Log::exec -> NrHashMap::dispatch_mut (nr/src/log.rs:494-518,
// benches/hashmap.rs:114-119, nr/examples/hashmap.rs:46-50) and the read path
// Replica::read_only -> dispatch (nr/src/replica.rs:483-497, benches/hashmap.rs:107-111).
//
// Table: 2^k open-addressing slots of 32 B {key, value, stamp[2]} (common.hpp), probed from
// mix64(key) >> (64 - k) round the home slot's group of four (one 128-B line), then group by group
// (common.hpp probe_slot); the one key equal to the empty marker lives in DevCtl::sp. Every
// replay round covers the log records [lo, lo+n) and takes a fresh epoch e. Two schedules:
//
// Stamp rounds (no previous-value responses, key stream not skewed): ONE launch per round,
//   {index(e) | apply(e-1) | reads(e-1)} on disjoint block ranges of hm_round_kernel:
//   index(e)   per Put: find the key's slot or claim an empty one (64-bit CAS; a fresh slot is
//              marked in the other parity, stamp (e, 0), so the reads of round e-1 running in
//              the same launch see it as absent); elect the round's last writer of every key
//              with atomicMax(st[e&1], e << 32 | i+1), pre-combined per block in LDS.
//   apply(e-1) per Put: the elected writer (st == (e-1, i+1)) stores its value.
//   reads(e-1) a key is present iff its stamp of parity e-1 is nonzero with epoch <= e-1; if the
//              epoch is e-1 the value is the elected record's (apply may be storing it).
//   index(e) touches only st[e&1], claims of empty slots and values apply never reads; apply and
//   reads look only at st[(e-1)&1]. The latency-bound index pass overlaps the reads.
// Partition rounds (previous-value responses, skewed key streams -- see skew_sample -- and rounds
//   of >= PART_MIN Puts): TWO launches per round and no device atomic per Put.
//   hm_round_kernel {partition(e) | reads(e-1)}: partition(e) only reads the records; each tile
//   writes its Puts grouped by the bucket of their key's HOME slot, in log order inside a
//   bucket, and a [tile][bucket] count word (the table is not touched, so the previous round's
//   reads run beside it against a quiescent table, without stamps);
//   hm_papply_kernel(e): one workgroup per bucket takes the bucket's entries (every tile's run,
//   tile order = log order) in chunks, finds each key's last writer in an LDS hash, and that
//   thread finds or claims the key's slot and stores its value: one table line read and written
//   per distinct key. All Puts of a key share its home bucket, so one workgroup decides each key.
//   512-thread workgroups over <= 512 buckets for rounds of >= 64k Puts (256 over <= 1024
//   below), buckets dealt to XCDs in contiguous ranges, the next chunk's entries loaded while a
//   chunk resolves. It runs at the memory-side request floor (profiles/r04_papply_phases.txt).
//   With previous values every Put keeps its entry and one wave walks each chunk in log order:
//   a Put's previous value is its predecessor's, else the key's value before the chunk, else None.
// Removal (nrg_hashmap_enable_removal; std::collections::HashMap::remove on the HashMap<u64, u64> of
//   benches/hashmap.rs:77-79; DESIGN.md "NrHashMap", Removal): on an enabled context a record whose
//   value is the tombstone is Remove(key), and every write round is a previous-value partition round
//   with the apply kernel's removal arm. A removed key keeps its slot, DEAD: val = tombstone for the
//   table scans, both stamps 0 for the Gets (which then always consult the stamp); a Put revives it, a
//   rehash drops it. A context that never enables launches what it always launched.
#include <cstring>

#include "internal.hpp"
#include "../../include/nrgpu_testing.h"

namespace nrg {

typedef u64 u64x2 __attribute__((ext_vector_type(2)));

// Streaming (nt) stores for the streamed outputs (log copy, read responses) of partition-round and
// reads-only launches: plain stores leave them dirty in the XCD's L2 for the kernel-end write-back
// after the last workgroup; streamed, they drain during the kernel. N = 8 per-GPU round 78.7 vs
// 80.5 us, configs[2] 256.9 vs 263.4; stamp rounds keep plain stores (B1 34.5-34.7 plain vs
// 34.7-35.0 streamed; profiles/r04_nt_stores.txt).
// Round 6: the compiler merges st_out's two branches into one plain store and drops the hint, so
// only the 16-B log copy (st_rec) is streamed; the responses are plain stores. Streamed for real
// (the plain branch as a relaxed wavefront-scope atomic store, which is not merged) they measured
// the same on one box: B1 34.15-34.19 us per round by the window (stamp-round reads streamed) vs
// 34.16-34.17, N = 8 per-GPU round 77.2-77.3 both, configs[2] 250.2 vs 250.7
// (profiles/r06/nt_single_stores.txt).
template <typename T>
__device__ __forceinline__ void st_out(T* p, T v, bool plain) {
    if (plain) *p = v;
    else __builtin_nontemporal_store(v, p);
}
__device__ __forceinline__ void st_rec(nrg_put* p, const nrg_put& r, bool plain) {
    if (plain) *p = r;
    else __builtin_nontemporal_store(u64x2{r.key, r.val}, (u64x2*)p);
}

// Round 6 (profiles/r06/b1_apply_nt.txt): the stamp-round apply's random value stores are streamed:
// they drain during the launch instead of in its end-of-kernel L2 write-back. Same box, three
// pairs: 34.16-34.20 -> 33.93-34.02 us per B1 step (window 34.03-34.13 -> 33.80-33.97); the
// driver's 20 steps 27,507-27,866 -> 27,823-27,875 Mops/s. The index role's put_slot / win / over
// words stay plain stores: streamed they were slower (34.49-34.53 vs 34.25).
// The partition apply's value stores are streamed in rounds of at most PA_NT_MAX Puts: same box,
// two pairs, N = 8 per-GPU round (800k Puts + 900k Gets) 77.24-77.35 -> 75.35-75.57 us, 50 % writes
// 53.7-53.8 -> 53.1-53.2; configs[2]'s 4M Puts slower streamed (251.1-251.3 -> 257.3-258.3), so
// they stay plain above it (profiles/r06/papply_nt.txt).
constexpr u64 PA_NT_MAX = 2000000;
template <bool NT, typename T>
__device__ __forceinline__ void st_pol(T* p, T v) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

constexpr int TPB = 256;
constexpr u32 SIDE_ID = 0x7FFFFFFFu;    // slot id standing for the side slot (slot ids are < 2^30)
constexpr u32 FULL_SLOT = 0xFFFFFFFFu;  // no slot could be claimed (table full)

// record i of a round: from a caller's buffer when given, else from the log ring
struct RecSrc {
    const nrg_put* src;
    const nrg_put* ring;
    u64 mask, lo;
    __device__ __forceinline__ nrg_put at(u64 i) const { return src ? src[i] : ring[(lo + i) & mask]; }
};

struct IndexJob {
    RecSrc rec;
    nrg_put* ring_out;  // log copy to write (nullptr: records already in the ring)
    u64 n;
    u32 nblocks;
    u32 nb_log;    // slot buckets = 1 << nb_log
    u32 bk_shift;  // bucket of a slot id = id >> bk_shift
    u64x2* ent;    // [nblocks][tile] {id << 32 | i+1, value}
    u32* eidx;     // partition rounds: [nblocks][tile] round offset i of each entry (previous values)
    u32* cnt;      // [bucket][nblocks] start << 16 | count
    u64* dup_acc;  // [HM_DUP_SLOTS] Puts overwritten inside their block (key skew statistic)
    bool plain;    // plain stores for the log copy (st_out)
};
struct ReadJob {
    const u64* keys;
    u64 R;
    u64* vals;
    uint8_t* found;
    u32 nblocks;
    u32 epoch;    // the reads see the state after round `epoch`
    bool use_rec; // that round's apply may run in the same launch: take its winners' records
    bool quiet;   // nothing in this launch writes the table (no stamp index, no apply): a key is
                  // present iff its probe chain holds it, and the stamps are not read
    RecSrc rec;
    // key-skew sample riding in this launch (skew_sample): the launch's last block moves the
    // duplicate counters to mapped host memory as {seq, dups}; seq 0 = none
    u64* s_acc;
    volatile u64* s_host;
    u64 s_seq;
    bool plain;  // plain stores for the responses (st_out)
};


// Block-wide exclusive prefix sum of one u32 per thread (NT threads); *total gets the sum.
template <int NT = TPB>
__device__ __forceinline__ u32 block_scan_excl(u32 v, u32* total) {
    __shared__ u32 s_w[NT / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    u32 inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u32 y = __shfl_up(inc, off, 64);
        if (lane >= off) inc += y;
    }
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    u32 pre = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; i++) {
        pre += i < w ? s_w[i] : 0u;
        tot += s_w[i];
    }
    __syncthreads();
    if (total) *total = tot;
    return pre + inc - v;
}

// ---- role: partition(e) (partition rounds) -------------------------------------------------------
// The tile's Puts go to the bucket of their key's HOME slot (home >> bk_shift; the side key to
// bucket 0), grouped by bucket in log order inside a bucket: {key, value} entries (+ the round
// offset i when previous values are wanted) and a count word cnt[bucket][tile] = start << 16 | count.
// Tile = TPB * K1 Puts; wave w owns [w*64*K1, (w+1)*64*K1) of it, so (q, lane) order inside a wave
// is log order and waves follow each other. DEDUP drops a Put that a later Put of the same key in
// the tile overwrites (rounds without previous values). The table is not touched: the previous
// round's reads run beside this pass in the same launch, and hm_papply_kernel does the rest.
template <int K1>
struct PartLds {
    static constexpr int TILE = TPB * K1;
    static constexpr int HSZ = TILE / 2;  // lossy dedup entries (u64 key + u32 position)
    static constexpr int PROBES = 16;
    static unsigned bytes(bool dedup, u32 nb) {
        const unsigned rank = nb * 4 + 4 * nb * 2;
        return dedup && HSZ * 12 > (int)rank ? (unsigned)(HSZ * 12) : rank;
    }
};

template <int K1, bool DEDUP>
__device__ __forceinline__ void part_role(const IndexJob& j, u32 blk, u32 shift, char* lds) {
    constexpr int WT = 64 * K1;
    constexpr int TILE = PartLds<K1>::TILE;
    constexpr int HSZ = PartLds<K1>::HSZ;
    constexpr u32 NOH = 0xFFFFFFFFu;  // the key found no dedup entry: always emitted
    __shared__ u32 s_side;  // dedup of the side-slot key: largest tile position + 1
    __shared__ u32 s_dup;   // Puts whose key another Put of the tile already entered
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const u64 base = (u64)blk * TILE;
    const u32 nb = 1u << j.nb_log;
    u64* s_hk = (u64*)lds;               // [HSZ] dedup keys
    u32* s_hp = (u32*)(lds + HSZ * 8);   // [HSZ] largest tile position + 1 per key
    if (DEDUP) {
        for (int q = threadIdx.x; q < HSZ; q += TPB) {
            s_hk[q] = EMPTY_KEY;
            s_hp[q] = 0;
        }
        if (threadIdx.x == 0) s_side = s_dup = 0;
    }
    nrg_put rec[K1];
    u32 bkt[K1];
    bool valid[K1];
#pragma unroll
    for (int q = 0; q < K1; q++) {
        const u64 i = base + (u64)(w * WT + q * 64 + lane);
        valid[q] = i < j.n;
        rec[q] = valid[q] ? j.rec.at(i) : nrg_put{0, 0};
    }
#pragma unroll
    for (int q = 0; q < K1; q++) {
        const u64 i = base + (u64)(w * WT + q * 64 + lane);
        if (valid[q] && j.ring_out) st_rec(&j.ring_out[(j.rec.lo + i) & j.rec.mask], rec[q], j.plain);
        bkt[q] = rec[q].key == EMPTY_KEY ? 0u : (u32)(table_home(rec[q].key, shift) >> j.bk_shift);
    }
    bool emit[K1];
    if (DEDUP) {
        __syncthreads();  // hash initialised
        u32 hq[K1];
        u32 dup = 0;
#pragma unroll
        for (int q = 0; q < K1; q++) {
            if (!valid[q]) continue;
            const u32 pos1 = (u32)(w * WT + q * 64 + lane) + 1;
            if (rec[q].key == EMPTY_KEY) {
                atomicMax(&s_side, pos1);
                continue;
            }
            // Lossy: a key that finds no entry within PROBES steps is not deduplicated. That is
            // consistent for all Puts of a key (entries are never freed, so every Put of a key that
            // got one walks into it); hot keys, the ones that matter, get one early.
            u32 h = (u32)(((mix64(rec[q].key) >> 32) * (u64)HSZ) >> 32);
            hq[q] = NOH;
            for (int pr = 0; pr < PartLds<K1>::PROBES; pr++) {
                const u64 old = atomicCAS((unsigned long long*)&s_hk[h], (unsigned long long)EMPTY_KEY,
                                          (unsigned long long)rec[q].key);
                if (old == EMPTY_KEY || old == rec[q].key) {
                    dup += old == rec[q].key ? 1u : 0u;
                    hq[q] = h;
                    break;
                }
                h = h + 1 == (u32)HSZ ? 0u : h + 1;
            }
            if (hq[q] != NOH) atomicMax(&s_hp[h], pos1);
        }
        if (dup) atomicAdd(&s_dup, dup);
        __syncthreads();
        if (threadIdx.x == 0 && s_dup && j.dup_acc) atomicAdd(&j.dup_acc[blk % HM_DUP_SLOTS], (u64)s_dup);
#pragma unroll
        for (int q = 0; q < K1; q++) {
            const u32 pos1 = (u32)(w * WT + q * 64 + lane) + 1;
            emit[q] = valid[q] && (rec[q].key == EMPTY_KEY ? s_side == pos1 : hq[q] == NOH || s_hp[hq[q]] == pos1);
        }
        __syncthreads();  // the hash region is reused below
    } else {
#pragma unroll
        for (int q = 0; q < K1; q++) emit[q] = valid[q];
    }
    // ---- stable grouping by bucket: wave-private counts, then a prefix over waves ----
    u32* s_start = (u32*)lds;                       // [nb] bucket start in the tile
    uint16_t* s_wc = (uint16_t*)(lds + nb * 4);     // [4][nb] per-wave counts -> wave offsets
    for (u32 b = threadIdx.x; b < 4 * nb; b += TPB) s_wc[b] = 0;
    __syncthreads();
    u32 rnk[K1];
#pragma unroll
    for (int q = 0; q < K1; q++) {
        // one returning LDS add per Put on the wave's packed u16 count (lanes of one instruction
        // get their old values in lane order: synthetic.hip's rankings, nrg_test_lds_add_order)
        if (emit[q]) {
            const u32 ix = w * nb + bkt[q], sh = (ix & 1u) * 16u;
            rnk[q] = (atomicAdd((u32*)s_wc + (ix >> 1), 1u << sh) >> sh) & 0xFFFFu;
        }
    }
    __syncthreads();
    constexpr int PER = HM_BK_MAX / TPB;  // buckets per thread (contiguous ownership)
    u32 tot[PER], loc = 0;
#pragma unroll
    for (int r = 0; r < PER; r++) {
        const u32 b = threadIdx.x * PER + r;
        tot[r] = 0;
        if (b < nb) {
            u32 run = 0;
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const u32 c = s_wc[v * nb + b];
                s_wc[v * nb + b] = (uint16_t)run;
                run += c;
            }
            tot[r] = run;
            loc += run;
        }
    }
    u32 off = block_scan_excl(loc, nullptr);
#pragma unroll
    for (int r = 0; r < PER; r++) {
        const u32 b = threadIdx.x * PER + r;
        if (b < nb) {
            j.cnt[(u64)blk * nb + b] = (off << 16) | tot[r];
            s_start[b] = off;
        }
        off += tot[r];
    }
    __syncthreads();
    u64x2* ent = j.ent + (u64)blk * TILE;
#pragma unroll
    for (int q = 0; q < K1; q++) {
        if (!emit[q]) continue;
        const u32 p = s_start[bkt[q]] + s_wc[w * nb + bkt[q]] + rnk[q];
        u64x2 e;
        e.x = rec[q].key;
        e.y = rec[q].val;
        ent[p] = e;  // (streamed: 75.4-75.8 -> 93.5-93.7 us per N = 8 round, profiles/r06/papply_nt.txt)
        if (j.eidx) j.eidx[(u64)blk * TILE + p] = (u32)(base + (u64)(w * WT + q * 64 + lane));
    }
}

// claim (or find) k's slot from its home slot; *fresh = this call inserted it; -1: table full
__device__ __forceinline__ long long claim_slot(Slot* table, u64 k, u64 home, u64 tmask, bool* fresh) {
    *fresh = false;
    for (u64 pr = 0; pr <= tmask; pr++) {
        const u64 s = probe_slot(home, pr, tmask);
        const u64 key = ld_relaxed(&table[s].key);
        if (key == k) return (long long)s;
        if (key == EMPTY_KEY) {
            const u64 old = atomicCAS((unsigned long long*)&table[s].key, (unsigned long long)EMPTY_KEY,
                                      (unsigned long long)k);
            if (old == EMPTY_KEY) {
                *fresh = true;
                return (long long)s;
            }
            if (old == k) return (long long)s;
        }
    }
    return -1;
}

// ---- stamp rounds: index(e) with claims and stamps, apply(e-1) ------------------------------------
struct StampJob {
    u64* dup_acc;  // [HM_DUP_SLOTS] Puts combined with another Put of their block (key skew)
    RecSrc rec;
    nrg_put* ring_out;
    u64 n;
    u32 nblocks;
    u32 epoch;
    u32* put_slot;  // [n] slot of each Put (SIDE_SLOT, FULL_SLOT)
    u32* win;       // [n] = epoch: the Put took its slot's stamp (it was the largest so far)
    u32* over;      // [n] = epoch: a later Put of the key took the stamp from it
    u64* created_acc;
    bool plain;  // plain stores for the log copy (st_out)
};
struct ApplyJob {
    RecSrc rec;
    u64 n;
    const u32* put_slot;
    const u32* win;
    const u32* over;
    u32 epoch;
    u32 nblocks;
};
constexpr u32 SIDE_SLOT = 0xFFFFFFFEu;  // put_slot of the key EMPTY_KEY

template <int K1>
struct StampLds {
    static constexpr int TILE = TPB * K1;
    static constexpr int HT = 2 * TILE;  // LDS combine table (slot -> largest i+1)
    static constexpr unsigned BYTES = HT * 8;
};

// find k from its home slot s (first key loaded: key0), or claim an empty slot; a slot this
// call claims is marked in the other parity (stamp (e, 0)) so the concurrent reads of round
// e-1 see it as absent; -1: table full
__device__ __forceinline__ long long find_or_claim_marked(Slot* table, u64 k, u64 s, u64 tmask, u64 key0, u32 e,
                                                          u32* created) {
    u64 key = key0;
    for (u64 pr = 0; pr <= tmask; pr++) {
        if (key == k) return (long long)s;
        if (key == EMPTY_KEY) {
            const u64 old = atomicCAS((unsigned long long*)&table[s].key, (unsigned long long)EMPTY_KEY,
                                      (unsigned long long)k);
            if (old == EMPTY_KEY) {
                table[s].st[(e - 1) & 1] = stamp_make(e, 0);
                *created += 1;
                return (long long)s;
            }
            if (old == k) return (long long)s;
        }
        s = probe_next(s, pr, tmask);
        key = ld_relaxed(&table[s].key);
    }
    return -1;
}

template <int K1>
__device__ __forceinline__ void stamp_index_role(const StampJob& j, u32 blk, Slot* table, u32 shift, u64 tmask,
                                                 DevCtl* ctl, char* lds) {
    constexpr int TILE = StampLds<K1>::TILE;
    constexpr int HT = StampLds<K1>::HT;
    __shared__ u32 s_side, s_created, s_dup;
    u32* s_slot = (u32*)lds;        // [HT] slot ids, ~0u free
    u32* s_max = (u32*)lds + HT;    // [HT] largest i+1 per slot in this block
    for (int q = threadIdx.x; q < HT; q += TPB) {
        s_slot[q] = 0xFFFFFFFFu;
        s_max[q] = 0;
    }
    if (threadIdx.x == 0) s_side = s_created = s_dup = 0;
    const u32 e = j.epoch, par = e & 1;
    const u64 base = (u64)blk * TILE;
    nrg_put rec[K1];
    u64 home[K1], key0[K1];
    // every record load, then every first probe, in flight before waiting on any of them
#pragma unroll
    for (int q = 0; q < K1; q++) {
        const u64 i = base + (u64)q * TPB + threadIdx.x;
        rec[q] = i < j.n ? j.rec.at(i) : nrg_put{EMPTY_KEY, 0};
    }
#pragma unroll
    for (int q = 0; q < K1; q++) {
        const u64 i = base + (u64)q * TPB + threadIdx.x;
        if (i < j.n && j.ring_out) st_rec(&j.ring_out[(j.rec.lo + i) & j.rec.mask], rec[q], j.plain);
        home[q] = table_home(rec[q].key, shift);
        key0[q] = i < j.n && rec[q].key != EMPTY_KEY ? table[home[q]].key : EMPTY_KEY;
    }
    __syncthreads();  // LDS table initialised
    u32 created = 0, dup = 0;
#pragma unroll
    for (int q = 0; q < K1; q++) {
        const u64 i = base + (u64)q * TPB + threadIdx.x;
        if (i >= j.n) continue;
        const u64 k = rec[q].key;
        if (k == EMPTY_KEY) {  // the side-slot key
            if (ld_relaxed32(&ctl->sp_claim) == 0 && atomicCAS(&ctl->sp_claim, 0u, 1u) == 0u) {
                ctl->sp.st[(e - 1) & 1] = stamp_make(e, 0);
                created++;
            }
            atomicMax(&s_side, (u32)(i + 1));
            j.put_slot[i] = SIDE_SLOT;
            continue;
        }
        const long long s = find_or_claim_marked(table, k, home[q], tmask, key0[q], e, &created);
        if (s < 0) {
            atomicOr(&ctl->err, ERR_TABLE_FULL);
            j.put_slot[i] = FULL_SLOT;
            continue;
        }
        j.put_slot[i] = (u32)s;
        u32 h = (u32)(mix64((u64)s) & (HT - 1));
        for (;;) {
            const u32 old = atomicCAS(&s_slot[h], 0xFFFFFFFFu, (u32)s);
            if (old == 0xFFFFFFFFu || old == (u32)s) {
                dup += old == (u32)s ? 1u : 0u;
                break;
            }
            h = (h + 1) & (HT - 1);
        }
        atomicMax(&s_max[h], (u32)(i + 1));
    }
    if (created) atomicAdd(&s_created, created);
    if (dup) atomicAdd(&s_dup, dup);
    __syncthreads();
    // one stamp atomic per distinct slot of the block (a hot key costs one per block). Its old
    // value settles who stores: a Put that raised the stamp is the winner so far (win = e); if the
    // stamp was already this round's, the Put it took it from is overtaken (over = e). So apply
    // finds the last writer from two coalesced words per Put, not from a random read of the
    // slot's stamp (n8: 31 us of apply for 800k Puts).
    for (int q = threadIdx.x; q < HT; q += TPB) {
        const u32 sl = s_slot[q];
        if (sl != 0xFFFFFFFFu) {
            const u64 mine = stamp_make(e, s_max[q]);
            const u64 old = atomicMax((unsigned long long*)&table[sl].st[par], (unsigned long long)mine);
            if (old < mine) {
                j.win[s_max[q] - 1] = e;
                if (stamp_epoch(old) == e && (u32)old) j.over[(u32)old - 1] = e;
            }
        }
    }
    if (threadIdx.x == 0) {
        if (s_side) atomicMax((unsigned long long*)&ctl->sp.st[par], (unsigned long long)stamp_make(e, s_side));
        if (s_created) atomicAdd(&j.created_acc[blk % HM_CREATED_SLOTS], (u64)s_created);
        if (s_dup && j.dup_acc) atomicAdd(&j.dup_acc[blk % HM_DUP_SLOTS], (u64)s_dup);
    }
}

// apply(e): per Put, the elected writer stores its value
__device__ __forceinline__ void apply_role(const ApplyJob& j, u32 blk, Slot* table, DevCtl* ctl) {
    const u64 i = (u64)blk * TPB + threadIdx.x;
    if (i >= j.n) return;
    const u32 par = j.epoch & 1;
    const u32 s = j.put_slot[i];
    const u64 want = stamp_make(j.epoch, i + 1);
    if (s == SIDE_SLOT) {
        if (ctl->sp.st[par] == want) ctl->sp.val = j.rec.at(i).val;
    } else if (s != FULL_SLOT) {
        // (a 16-B {key, val} store costs the same: a partial-line write is priced per line,
        // profiles/r03_apply_store_width.txt)
        if (j.win[i] == j.epoch && j.over[i] != j.epoch) __builtin_nontemporal_store(j.rec.at(i).val, &table[s].val);
    }
}

// ---- role: reads -------------------------------------------------------------------------------
// Present iff the stamp of the round's parity is nonzero with epoch <= ep (0: claim in flight;
// a later epoch: created by the concurrent round); epoch == ep: written by round ep, whose
// elected record holds the value while its apply may run in this launch.
__device__ __forceinline__ bool resolve(u64 val, u64 st, const ReadJob& j, u64* v) {
    const u32 se = stamp_epoch(st);
    if (st == 0 || se > j.epoch) return false;
    *v = (se == j.epoch && j.use_rec) ? j.rec.at((u32)st - 1).val : val;
    return true;
}

// A block's reads: TPB * RPT consecutive Gets. (RPT: Gets per thread with every key load and every
// home-line load of the thread in flight together, measured on one box, profiles/r03_read_rpt.txt, B1
// per round: RPT 1 34.4 us, 2 36.2, 4 39.8; the N=8 per-GPU round 99.3 / 100.8 / 105.4 us.)
constexpr int RPT = 1;
static_assert(RPT == 1, "read_role gives a wave 64 consecutive Gets");

// quad_perm DPP moves (lane ^ 1 and lane ^ 2 inside each four lanes) and the OR over a quad of lanes
__device__ __forceinline__ u32 quad_x1(u32 x) { return (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xF, 0xF, true); }
__device__ __forceinline__ u32 quad_x2(u32 x) { return (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xF, 0xF, true); }
__device__ __forceinline__ u64 quad_or(u64 x) {
    u32 lo = (u32)x, hi = (u32)(x >> 32);
    lo |= quad_x1(lo);
    hi |= quad_x1(hi);
    lo |= quad_x2(lo);
    hi |= quad_x2(hi);
    return ((u64)hi << 32) | lo;
}

// A Get reads its key's whole home group (four slots, one 128-B line) in one trip: the probe sequence
// (common.hpp probe_slot) keeps a key in its home group whenever the group had room, so a group with
// a match or an empty slot answers the Get, and only a full group without the key (4e-4 of the
// groups at B1's load) sends it on to the next group. A wave owns 64 consecutive Gets and takes them
// in READ_PASSES passes of 16: in pass p the quad of lanes 4g .. 4g+3 owns Get 16 p + g, and lane
// sub = lane & 3 loads {key, val} and the stamp of slot sub of the group, two loads of one line
// issued back to back, every pass's loads in flight before the first wait (one wave instruction
// touches 16 lines, 4 lanes each). At most one lane of a quad matches (a key sits in one slot), so
// the quad's answer is the OR of its lanes' (0 where nothing matched); the answers then go back to
// one Get per lane, so a wave stores whole 512-B / 64-B runs. Against the per-lane chain walk:
// 22.8-22.9 us against 23.8-23.9 per 900k Gets (microbench/read_chain.hip groupA against dyn2;
// 64 Gets per block and one pass measured slower, groupB; profiles/read_group.txt).
//
// STAMP: the role inside a stamp round's kernel, which launch() uses only with index blocks: the
// table is being written (never quiet) and the responses are plain stores. With both flags known
// when the kernel is compiled the chain walk measured 2 us faster per 900k Gets than with the flags
// read from the job (microbench/read_chain.hip dyn2 against dyn3, profiles/read_chain.txt).
constexpr int READ_PASSES = 4;
static_assert(READ_PASSES * 16 == 64, "a wave's passes of 16 quads cover its 64 Gets");
template <bool STAMP>
__device__ __forceinline__ void read_role(const ReadJob& j, u32 blk, const Slot* table, u32 shift, u64 tmask,
                                          const DevCtl* ctl) {
    const u32 par = j.epoch & 1;
    const auto quiet = [&] { return STAMP ? false : j.quiet; };
    const auto plain = [&] { return STAMP ? true : j.plain; };
    const u32 lane = lane_id(), sub = lane & 3, quad = lane >> 2, qsh = lane & ~3u;
    const u64 wbase = (u64)blk * TPB + (threadIdx.x & ~63u);  // the wave's first Get
    if (wbase >= j.R) return;
    u64 k[READ_PASSES], s[READ_PASSES], st[READ_PASSES];
    u64x2 w[READ_PASSES];
#pragma unroll
    for (int p = 0; p < READ_PASSES; p++) {
        const u64 q = wbase + p * 16 + quad;
        k[p] = q < j.R ? j.keys[q] : EMPTY_KEY;  // (a Get past the end is not stored)
    }
#pragma unroll
    for (int p = 0; p < READ_PASSES; p++) {
        s[p] = ((table_home(k[p], shift) & ~3ull) | sub) & tmask;
        w[p].x = EMPTY_KEY;
        w[p].y = 0;
        st[p] = 0;
        if (k[p] != EMPTY_KEY) {
            // (round 6: with the streaming hint on these two loads, 34.04-34.13 -> 44.25-44.36 us per
            // B1 round; profiles/r06/b1_apply_nt.txt)
            w[p] = *(const u64x2*)&table[s[p]];
            if (!quiet()) st[p] = table[s[p]].st[par];
        }
    }
    u64 rv[READ_PASSES], fb[READ_PASSES];
#pragma unroll
    for (int p = 0; p < READ_PASSES; p++) {
        u64 kk = w[p].x, vv = w[p].y, stt = st[p], sl = s[p], v = 0;
        // (without these the compiler sinks the stamp load below the loop, a second dependent trip)
        asm volatile("" : "+v"(kk), "+v"(vv), "+v"(stt));
        bool f = false, act = k[p] != EMPTY_KEY;
        // at most one group per step and every group once: an absent key in a full table terminates
        for (u64 g = 0;; g++) {
            const bool hit = act && kk == k[p];
            if (hit) {
                if (quiet()) {
                    f = true;
                    v = vv;
                } else {
                    f = resolve(vv, stt, j, &v);
                }
            }
            // a match or an empty slot ends the quad's search (a lane that does not probe reads as empty)
            const u64 done = __ballot(hit || !act || kk == EMPTY_KEY);
            act = ((done >> qsh) & 15) == 0 && g < (tmask >> 2);
            if (!__ballot(act)) break;
            if (act) {
                sl = (sl + 4) & tmask;
                const u64x2 x = *(const u64x2*)&table[sl];
                if (!quiet()) stt = table[sl].st[par];
                kk = x.x;
                vv = x.y;
            }
        }
        if (k[p] == EMPTY_KEY && sub == 0 && ctl->sp_claim) {  // the side key, answered by the quad's first lane
            if (quiet()) {
                f = true;
                v = ctl->sp.val;
            } else {
                f = resolve(ctl->sp.val, ctl->sp.st[par], j, &v);
            }
        }
        if (!f) v = 0;
        rv[p] = quad_or(v);
        fb[p] = __ballot(f);
    }
    // back to one Get per lane: lane l keeps pass (l & 3)'s answer of its quad, and Get 16 p + g of
    // the wave is then in lane 4 g + p; its found bit is any of the quad's four bits of pass p
    u64 c = rv[0], b = fb[0];
#pragma unroll
    for (int p = 1; p < READ_PASSES; p++) {
        if (sub == (u32)p) c = rv[p];
        if ((lane >> 4) == (u32)p) b = fb[p];
    }
    const u64 v = __shfl(c, (int)(4 * (lane & 15) + (lane >> 4)), 64);
    const u64 q = wbase + lane;
    if (q < j.R) {
        st_out(&j.vals[q], v, plain());
        st_out(&j.found[q], (uint8_t)(((b >> (4 * (lane & 15))) & 15) != 0), plain());
    }
}

// index-role kinds of a round launch
constexpr int IX_STAMP = 2;       // stamp round
constexpr int IX_PART = 3;        // partition round, dedup (hm_papply_kernel<false> follows)
constexpr int IX_PART_ALL = 4;    // partition round, every Put kept (previous values)
constexpr int IX_PART_NODUP = 5;  // partition round, every Put kept, no previous values (uniform keys)

// One launch = {index(e)} + {apply(e-1)} + {reads(e-1)} over disjoint block ranges (any may be
// empty). Index blocks come first so the latency-bound pass starts first.
// <= 80 SGPRs: 256-thread blocks are admitted 8 per CU only up to 80 SGPRs (82-96: 7 per CU,
// MI355X_MICROARCH.md "Residency"), and the read role needs every resident wave.
template <int K1, int IX>
__global__ __launch_bounds__(TPB) __attribute__((amdgpu_num_sgpr(80))) void hm_round_kernel(IndexJob ij, StampJob sj,
                                                                                             ApplyJob aj, ReadJob rj,
                                                       Slot* table, u32 shift, u64 tmask, DevCtl* ctl) {
    extern __shared__ __attribute__((aligned(16))) char s_lds[];
    u32 b = blockIdx.x;
    if (rj.s_seq && b == gridDim.x - 1) {  // the tail block
        // the skew sample (counters read and cleared atomically)
        if (rj.s_seq && threadIdx.x < HM_DUP_SLOTS) {
            u64 v = atomicExch((unsigned long long*)&rj.s_acc[threadIdx.x], 0ull);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            if (threadIdx.x == 0) {
                rj.s_host[1] = v;
                __threadfence_system();
                rj.s_host[0] = rj.s_seq;
            }
        }
        return;
    }
    const u32 nix = IX == IX_STAMP ? sj.nblocks : ij.nblocks;
    if (b < nix) {
        if constexpr (IX == IX_STAMP) stamp_index_role<K1>(sj, b, table, shift, tmask, ctl, s_lds);
        else part_role<K1, IX == IX_PART>(ij, b, shift, s_lds);
        return;
    }
    b -= nix;
    if (b < aj.nblocks) {
        apply_role(aj, b, table, ctl);
        return;
    }
    b -= aj.nblocks;
    read_role<IX == IX_STAMP>(rj, b, table, shift, tmask, ctl);
}

// ---- hm_papply_kernel: partition rounds' table pass, one workgroup per bucket ---------------------
// The bucket's entries (every tile's run, tile order = log order) are taken in chunks of PA_C:
// an LDS hash finds each key's last entry in the chunk, whose thread finds the key's slot from
// its home (or claims an empty one: a new key) and stores the value -- one table line read and
// written per distinct key, no device atomics per Put. All Puts of a key share a bucket (the
// bucket is the home slot's), so one workgroup decides each key; a later chunk of the bucket
// overwrites an earlier one's store in log order. Claims of other buckets' workgroups only fill
// empty slots and cannot cut a present key's probe chain.
// PREV (HashMap::insert's previous values, nr/examples/hashmap.rs:46-50): every Put has an entry;
// the first entry of a key in the chunk finds (or claims) the slot and its value before the
// chunk; wave 0 then walks the chunk in log order, 64 entries a step: a Put's previous value is
// its predecessor's value, else the key's value before the chunk, else None.
struct PApplyJob {
    const u64x2* ent;  // [tiles][tile] {key, value}
    const u32* eidx;   // [tiles][tile] round offset (PREV)
    const u32* cnt;    // [tiles][bucket] start << 16 | count
    u32 ntiles, tile, nb;
    Slot* table;
    u32 shift;
    u64 tmask;
    DevCtl* ctl;
    u64* created_acc;
    u64 lo, resp_lo, resp_hi;
    u64* prev;
    uint8_t* prevf;
    u32 stall;  // NRG_KNOB_STALL (tests)
    u64* dbg;   // (NRG_KNOB_EXP bit 2, diagnostic) per bucket, 8 words: [0] start [1] counts scanned
                // [2] first chunk hashed [3] its slots resolved [4] its stores done [5] end [6] chunks
    // removal (hm_papply_kernel<true, 256, false, true> alone reads these; they stay last, so the
    // fields above are where the other instantiations have always found them)
    u64 tomb;       // an entry whose value is this is Remove(key)
    u64* dead_acc;  // [HM_CREATED_SLOTS] slots that died minus slots revived (wrapping)
};

// T threads per workgroup (rounds without previous values: 256, 512 or 1024 over at most 1024,
// 512 or 256 buckets). Wider workgroups over wider buckets: a bucket's run in a tile holds more
// entries (a 128-B line at 1024 instead of ~32 B at 256) and there are fewer [tile][bucket] count
// words to gather, each a line.
template <bool PREV, int T>
struct PaGeo {
    static_assert(!PREV || T == 256, "previous values use 256-thread workgroups");
    static constexpr int TPB = T;
    static constexpr int C = PREV ? 512 : 4 * T;  // entries per chunk
    static constexpr int HT = 2 * C;              // LDS hash entries (load <= 1/2)
    static constexpr int PER = C / TPB;
    static constexpr u32 NB_LOG = T == 1024 ? 8 : T == 512 ? 9 : 10;  // at most this many buckets
};

__device__ __forceinline__ u32 pa_hash(u64 k, u32 ht) { return (u32)(mix64(k) >> 40) & (ht - 1); }

// Find or claim the slots of up to N keys of one thread together: every probe load, then every
// CAS on an empty slot, of all N keys is in flight before any is resolved (one or two memory
// round trips for most keys instead of one or two per key). on[r]: key r takes part (not the
// side key). Out: slot[r] (-1: table full), fresh[r] (this call claimed it: epoch-1 stamps
// written), val[r] = the slot's value before this call (found keys; WANT_VAL).
// FIND (removal): key r claims only if claim[r]; else its probe ends at the first empty slot, as a
// reader's does, with slot[r] = PA_ABSENT and the table untouched.
constexpr long long PA_ABSENT = -2;
template <int N, bool WANT_VAL, bool FIND = false>
__device__ __forceinline__ void pa_resolve(Slot* table, u32 shift, u64 tmask, const u64* k, const bool* on,
                                           long long* slot, bool* fresh, u64* val, const bool* claim = nullptr) {
    u64 s[N], kk[N], vv[N];
    u32 st[N];  // 0 done, 1 key loaded, 2 CAS needed, 3 moved on to the chain's next slot
#pragma unroll
    for (int r = 0; r < N; r++) {
        st[r] = on[r] ? 1u : 0u;
        s[r] = on[r] ? table_home(k[r], shift) : 0;
        slot[r] = -1;
        fresh[r] = false;
        kk[r] = EMPTY_KEY;
        vv[r] = 0;
        if (on[r]) {
            if (WANT_VAL) {
                const u64x2 x = *(const u64x2*)&table[s[r]];
                kk[r] = x.x;
                vv[r] = x.y;
            } else {
                kk[r] = ld_relaxed(&table[s[r]].key);
            }
        }
    }
    for (u64 pr = 0; pr <= tmask; pr++) {
        bool any = false;
#pragma unroll
        for (int r = 0; r < N; r++) {
            if (st[r] != 1) continue;
            if (kk[r] == k[r]) {
                slot[r] = (long long)s[r];
                if (WANT_VAL) val[r] = vv[r];
                st[r] = 0;
            } else if (kk[r] == EMPTY_KEY) {
                if (FIND && !claim[r]) {
                    slot[r] = PA_ABSENT;
                    st[r] = 0;
                } else {
                    st[r] = 2;
                }
            } else {
                s[r] = probe_next(s[r], pr, tmask);
                st[r] = 3;
            }
            any = any || st[r] != 0;
        }
        if (!any) return;
        u64 old[N];
#pragma unroll
        for (int r = 0; r < N; r++)
            if (st[r] == 2)
                old[r] = atomicCAS((unsigned long long*)&table[s[r]].key, (unsigned long long)EMPTY_KEY,
                                   (unsigned long long)k[r]);
#pragma unroll
        for (int r = 0; r < N; r++) {
            if (st[r] != 2) continue;
            if (old[r] == EMPTY_KEY) {  // claimed: a new key, present for every later read
                u64x2 z;
                z.x = z.y = STAMP_PRESENT;
                *(u64x2*)&table[s[r]].st[0] = z;
                slot[r] = (long long)s[r];
                fresh[r] = true;
                st[r] = 0;
            } else if (old[r] == k[r]) {
                slot[r] = (long long)s[r];
                if (WANT_VAL) val[r] = ld_relaxed(&table[s[r]].val);
                st[r] = 0;
            } else {
                s[r] = probe_next(s[r], pr, tmask);
                st[r] = 3;
            }
        }
#pragma unroll
        for (int r = 0; r < N; r++) {
            if (st[r] != 3) continue;
            if (WANT_VAL) {
                const u64x2 x = *(const u64x2*)&table[s[r]];
                kk[r] = x.x;
                vv[r] = x.y;
            } else {
                kk[r] = ld_relaxed(&table[s[r]].key);
            }
            st[r] = 1;
        }
    }
    // every slot probed and none matched: a table with no empty slot left. A key that would have
    // claimed is refused (slot -1); a find-only probe has its answer, absent, as a reader's has.
    if constexpr (FIND) {
#pragma unroll
        for (int r = 0; r < N; r++)
            if (st[r] != 0 && !claim[r]) slot[r] = PA_ABSENT;
    }
}

// NT: the table values are stored streamed (round 6; rounds of <= PA_NT_MAX Puts, see the launch)
// RM: removal (nrg_hashmap_enable_removal; every write round of an enabled context). An entry whose
// value is j.tomb is Remove(key) (HashMap::remove): it answers what a Put answers, None after a
// Remove, and leaves the key without a value. A removed key keeps its slot (common.hpp probe_slot:
// no slot is ever emptied), which becomes DEAD: val = tomb, both stamps 0. Per key and chunk:
//   first entry   find the slot; claim one only if the key has a Put in this chunk (s_hf bit 1), so a
//                 Remove of an absent key takes no slot. A dead slot is "no value before the chunk"
//                 and is remembered for revival (s_hf bit 2).
//   last entry    live: the value, and the two present stamps if the slot was dead; not live and a slot
//                 exists (it was live, or a Put of this chunk claimed it): the slot dies.
// created_acc counts claims (occupancy); dead_acc the deaths minus the revivals.
template <bool PREV, int T, bool NT = false, bool RM = false>
__global__ __launch_bounds__(T) __attribute__((amdgpu_waves_per_eu(PREV ? 3 : 4))) void hm_papply_kernel(PApplyJob j) {
    static_assert(!RM || (PREV && !NT), "removal rides the previous-value arm");
    using G = PaGeo<PREV, T>;
    constexpr int PA_TPB = G::TPB, C = G::C, HT = G::HT, PER = G::PER;
    constexpr u32 NOFIRST = 0xFFFFFFFFu;
    constexpr u32 NO_SLOT = 0xFFFFFFFDu;  // RM: the key holds no slot (absent, and only removed in this chunk)
    constexpr u32 HF_LIVE = 1u, HF_PUT = 2u, HF_DEAD = 4u;  // s_hf: bits 1 and 2 are RM's
    extern __shared__ u32 s_dyn[];  // s_pre[ntiles + 1] entry prefix, s_off[ntiles] (u16)
    __shared__ u64 s_hk[HT];
    __shared__ u32 s_hp[HT + 1];   // last chunk position + 1 of the key; [HT]: the side key
    __shared__ uint16_t s_tile[2][C];        // entry tile maps of this chunk and the next
    __shared__ u32 s_h1[PREV ? HT + 1 : 1];  // PREV: first chunk position + 1
    __shared__ u32 s_hs[PREV ? HT + 1 : 1];  // PREV: the key's slot (SIDE_ID, FULL_SLOT)
    __shared__ u64 s_lv[PREV ? HT + 1 : 1];  // PREV: the key's value so far in the walk
    __shared__ u32 s_hf[PREV ? HT + 1 : 1];  // PREV: s_lv holds a value
    __shared__ u64 s_mk[PREV ? HT + 1 : 1];  // PREV: lanes of the current walk step per key
    __shared__ u64 s_ev[PREV ? C : 1];       // PREV: the chunk's values, hash entries, round offsets
    __shared__ uint16_t s_eh[PREV ? C : 1];
    __shared__ u32 s_ei[PREV ? C : 1];
    __shared__ u32 s_created;
    __shared__ int s_died;  // RM: deaths minus revivals
    // Workgroups are dealt to the 8 XCDs round-robin; bucket b goes to workgroup 8 (b % per) + b / per
    // (per = nb / 8), so each XCD takes a contiguous range of buckets. Neighbouring buckets' entry
    // runs and count words share lines, and those lines are then fetched into one XCD's L2
    // instead of several.
    const u32 per = j.nb >> 3;
    const u32 nt = j.ntiles, b = j.nb >= 64 ? (blockIdx.x & 7u) * per + (blockIdx.x >> 3) : blockIdx.x;
#define PA_MARK(K, V) \
    if (j.dbg && threadIdx.x == 0) j.dbg[(u64)b * 8 + (K)] = (V)
    PA_MARK(0, wall_clock64());
    u32* s_pre = s_dyn;
    uint16_t* s_off = (uint16_t*)(s_dyn + nt + 1);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // this bucket's (offset, count) in every tile; thread owns tiles [tid*K, tid*K + K)
    const u32 K = (nt + PA_TPB - 1) / PA_TPB;
    u32 loc = 0;
    for (u32 q = 0; q < K; q++) {
        const u32 t = threadIdx.x * K + q;
        if (t < nt) {
            const u32 v = j.cnt[(u64)t * j.nb + b];
            s_off[t] = (uint16_t)(v >> 16);
            s_pre[t] = v & 0xFFFFu;
            loc += v & 0xFFFFu;
        }
    }
    for (int h = threadIdx.x; h <= HT; h += PA_TPB) {
        if (h < HT) s_hk[h] = EMPTY_KEY;
        s_hp[h] = 0;
        if (PREV) {
            s_h1[h] = NOFIRST;
            s_mk[h] = 0;
        }
        if (RM) s_hf[h] = 0;
    }
    u32 total;
    u32 run = block_scan_excl<PA_TPB>(loc, &total);  // (its barriers also order the initialisation above)
    for (u32 q = 0; q < K; q++) {
        const u32 t = threadIdx.x * K + q;
        if (t < nt) {
            const u32 c = s_pre[t];
            s_pre[t] = run;
            run += c;
        }
    }
    if (threadIdx.x == 0) {
        s_pre[nt] = total;
        s_created = 0;
        if (RM) s_died = 0;
    }
    __syncthreads();
    PA_MARK(1, wall_clock64());
    PA_MARK(6, (total + C - 1) / C);
    u32 created = 0;
    int died = 0;
    // entry tile map of the chunk at `base`
    auto map_chunk = [&](u32 base, uint16_t* map) {
        const u32 cn = total - base < (u32)C ? total - base : (u32)C;
        for (u32 q = 0; q < K; q++) {
            const u32 t = threadIdx.x * K + q;
            if (t >= nt) break;
            const u32 lo_ = s_pre[t] > base ? s_pre[t] : base;
            const u32 hi_ = s_pre[t + 1] < base + cn ? s_pre[t + 1] : base + cn;
            for (u32 i = lo_; i < hi_; i++) map[i - base] = (uint16_t)t;
        }
    };
    // this thread's entries of the chunk at `base` (issued; used a chunk later)
    u64x2 xn[PER];
    u32 in_[PER];
    auto load_chunk = [&](u32 base, const uint16_t* map) {
        const u32 cn = total - base < (u32)C ? total - base : (u32)C;
#pragma unroll
        for (int r = 0; r < PER; r++) {
            const u32 p = r * PA_TPB + threadIdx.x;
            xn[r].x = EMPTY_KEY;
            xn[r].y = 0;
            in_[r] = 0;
            if (p < cn) {
                const u32 t = map[p];
                const u64 e = (u64)t * j.tile + s_off[t] + (base + p - s_pre[t]);
                xn[r] = j.ent[e];
                if (PREV) in_[r] = j.eidx[e];
            }
        }
    };
    if (total) {
        map_chunk(0, s_tile[0]);
        __syncthreads();
        test_stall(j.stall & 1, w);  // (tests) slow waves read the map while the next is built
        load_chunk(0, s_tile[0]);
    }
    // Software pipelined: the next chunk's entries are in flight while this chunk resolves.
    for (u32 base = 0, pb = 0; base < total; base += C, pb ^= 1) {
        const u32 cn = total - base < (u32)C ? total - base : (u32)C;
        u64x2 x[PER];
        u32 ix[PER], hh[PER];
#pragma unroll
        for (int r = 0; r < PER; r++) {
            x[r] = xn[r];
            ix[r] = in_[r];
        }
        const u32 nbase = base + C;
        if (nbase < total) map_chunk(nbase, s_tile[pb ^ 1]);  // (published by the barrier below)
        // one hash entry per key: its last (and first) position in the chunk
#pragma unroll
        for (int r = 0; r < PER; r++) {
            const u32 p = r * PA_TPB + threadIdx.x;
            hh[r] = HT;
            if (p >= cn) continue;
            const u64 k = x[r].x;
            u32 h = HT;
            if (k != EMPTY_KEY) {
                h = pa_hash(k, HT);
                for (;;) {  // at most C keys in 2C entries: an entry is always found
                    const u64 old = atomicCAS((unsigned long long*)&s_hk[h], (unsigned long long)EMPTY_KEY,
                                              (unsigned long long)k);
                    if (old == EMPTY_KEY || old == k) break;
                    h = (h + 1) & (HT - 1);
                }
            }
            hh[r] = h;
            atomicMax(&s_hp[h], p + 1);
            if (PREV) {
                atomicMin(&s_h1[h], p + 1);
                s_ev[p] = x[r].y;
                s_eh[p] = (uint16_t)h;
                s_ei[p] = ix[r];
                if (RM && x[r].y != j.tomb) atomicOr(&s_hf[h], HF_PUT);  // (s_hf is 0 between chunks)
            }
        }
        __syncthreads();
        if (base == 0) PA_MARK(2, wall_clock64());
        if (nbase < total) {
            test_stall(j.stall & 1, w);  // (tests) slow waves read the next map after the others moved on
            load_chunk(nbase, s_tile[pb ^ 1]);
        }
        if (!PREV) {
            // the key's last entry finds or claims its slot and stores its value
            bool dec[PER], on[PER], fr[PER];
            u64 kx[PER], vx[PER];
            long long sl[PER];
#pragma unroll
            for (int r = 0; r < PER; r++) {
                const u32 p = r * PA_TPB + threadIdx.x;
                dec[r] = p < cn && s_hp[hh[r]] == p + 1;
                on[r] = dec[r] && x[r].x != EMPTY_KEY;
                kx[r] = x[r].x;
            }
            pa_resolve<PER, false>(j.table, j.shift, j.tmask, kx, on, sl, fr, vx);
            if (base == 0) PA_MARK(3, wall_clock64());
#pragma unroll
            for (int r = 0; r < PER; r++) {
                if (!dec[r]) continue;
                if (x[r].x == EMPTY_KEY) {
                    if (!j.ctl->sp_claim) {
                        j.ctl->sp_claim = 1;
                        j.ctl->sp.st[0] = j.ctl->sp.st[1] = STAMP_PRESENT;
                        created++;
                    }
                    j.ctl->sp.val = x[r].y;
                } else if (sl[r] < 0) {
                    atomicOr(&j.ctl->err, ERR_TABLE_FULL);
                } else {
                    st_pol<NT>(&j.table[sl[r]].val, x[r].y);
                    created += fr[r];
                }
            }
            __syncthreads();  // every decider has read s_hp
#pragma unroll
            for (int r = 0; r < PER; r++) {  // the deciders free their keys' entries for the next chunk
                if (!dec[r]) continue;
                if (hh[r] < (u32)HT) s_hk[hh[r]] = EMPTY_KEY;
                s_hp[hh[r]] = 0;
            }
        } else {
            // the key's first entry: its slot and its value before the chunk
            bool fst[PER], on[PER], fr[PER], cl[PER];
            u64 kx[PER], vx[PER];
            long long sl[PER];
#pragma unroll
            for (int r = 0; r < PER; r++) {
                const u32 p = r * PA_TPB + threadIdx.x;
                fst[r] = p < cn && s_h1[hh[r]] == p + 1;
                on[r] = fst[r] && x[r].x != EMPTY_KEY;
                kx[r] = x[r].x;
                vx[r] = 0;
                cl[r] = RM && fst[r] && (s_hf[hh[r]] & HF_PUT);
            }
            if constexpr (RM) pa_resolve<PER, true, true>(j.table, j.shift, j.tmask, kx, on, sl, fr, vx, cl);
            else pa_resolve<PER, true>(j.table, j.shift, j.tmask, kx, on, sl, fr, vx);
#pragma unroll
            for (int r = 0; r < PER; r++) {
                if (!fst[r]) continue;
                const u32 h = hh[r];
                if constexpr (RM) {
                    // (this thread alone writes the key's s_hf here: the Puts' atomicOr ran before the barrier)
                    u32 f = cl[r] ? HF_PUT : 0u;
                    if (x[r].x == EMPTY_KEY) {
                        if (j.ctl->sp_claim) {
                            const u64 v0 = j.ctl->sp.val;
                            s_hs[h] = SIDE_ID;
                            s_lv[h] = v0;
                            f |= v0 == j.tomb ? HF_DEAD : HF_LIVE;
                        } else if (cl[r]) {
                            j.ctl->sp_claim = 1;
                            j.ctl->sp.st[0] = j.ctl->sp.st[1] = STAMP_PRESENT;
                            created++;
                            s_hs[h] = SIDE_ID;
                        } else {
                            s_hs[h] = NO_SLOT;
                        }
                    } else if (sl[r] == PA_ABSENT) {
                        s_hs[h] = NO_SLOT;
                    } else if (sl[r] < 0) {
                        atomicOr(&j.ctl->err, ERR_TABLE_FULL);
                        s_hs[h] = FULL_SLOT;
                    } else {
                        s_hs[h] = (u32)sl[r];
                        created += fr[r];
                        s_lv[h] = vx[r];
                        if (!fr[r]) f |= vx[r] == j.tomb ? HF_DEAD : HF_LIVE;
                    }
                    s_hf[h] = f;
                    continue;
                }
                if (x[r].x == EMPTY_KEY) {
                    s_hs[h] = SIDE_ID;
                    if (j.ctl->sp_claim) {
                        s_lv[h] = j.ctl->sp.val;
                        s_hf[h] = 1;
                    } else {
                        j.ctl->sp_claim = 1;
                        j.ctl->sp.st[0] = j.ctl->sp.st[1] = STAMP_PRESENT;
                        created++;
                        s_hf[h] = 0;
                    }
                } else if (sl[r] < 0) {
                    atomicOr(&j.ctl->err, ERR_TABLE_FULL);
                    s_hs[h] = FULL_SLOT;
                    s_hf[h] = 0;
                } else {
                    s_hs[h] = (u32)sl[r];
                    created += fr[r];
                    s_hf[h] = fr[r] ? 0u : 1u;
                    s_lv[h] = vx[r];
                }
            }
            __syncthreads();
            // wave 0 walks the chunk in log order, 64 entries a step
            if (w == 0) {
                for (u32 s0 = 0; s0 < cn; s0 += 64) {
                    const u32 p = s0 + lane;
                    const bool v = p < cn;
                    const u32 h = v ? s_eh[p] : 0u;
                    const u64 val = v ? s_ev[p] : 0ull;
                    if (v) atomicOr((unsigned long long*)&s_mk[h], 1ull << lane);
                    const u64 m = v ? s_mk[h] : 0ull;
                    const u64 lower = m & ((1ull << lane) - 1);
                    const int pl = lower ? 63 - __clzll((long long)lower) : lane;
                    const u64 pv_lane = __shfl(val, pl, 64);
                    if (v) {
                        u64 pv;
                        uint8_t pf;
                        if (lower) {
                            pv = pv_lane;
                            pf = 1;
                            if (RM && pv_lane == j.tomb) {  // the predecessor is a Remove
                                pv = 0;
                                pf = 0;
                            }
                        } else {
                            pf = (RM ? s_hf[h] & HF_LIVE : s_hf[h]) ? 1 : 0;
                            pv = pf ? s_lv[h] : 0;
                        }
                        const u64 g = j.lo + s_ei[p];
                        if (g >= j.resp_lo && g < j.resp_hi) {
                            j.prev[g - j.resp_lo] = pv;
                            j.prevf[g - j.resp_lo] = pf;
                        }
                        if ((m >> lane) == 1ull) {  // the key's last entry in this step
                            if constexpr (RM) {
                                if (val == j.tomb) {  // a Remove leaves the running value empty
                                    s_hf[h] &= ~HF_LIVE;
                                } else {
                                    s_lv[h] = val;
                                    s_hf[h] |= HF_LIVE;
                                }
                            } else {
                                s_lv[h] = val;
                                s_hf[h] = 1;
                            }
                            s_mk[h] = 0;
                        }
                    }
                }
            }
            __syncthreads();
            // the key's last entry stores its final value
#pragma unroll
            for (int r = 0; r < PER; r++) {
                const u32 p = r * PA_TPB + threadIdx.x;
                if (p >= cn || s_hp[hh[r]] != p + 1) continue;
                const u32 h = hh[r];
                const u32 sl = s_hs[h];
                if constexpr (RM) {
                    const u32 f = s_hf[h];
                    Slot* t = sl == SIDE_ID ? &j.ctl->sp : sl < NO_SLOT ? &j.table[sl] : nullptr;
                    if (t && (f & HF_LIVE)) {
                        t->val = s_lv[h];
                        if (f & HF_DEAD) {  // revived
                            u64x2 z;
                            z.x = z.y = STAMP_PRESENT;
                            *(u64x2*)&t->st[0] = z;
                            died--;
                        }
                    } else if (t && !(f & HF_DEAD)) {  // it was live, or a Put of this chunk claimed it: it dies
                        u64x2 z;
                        z.x = z.y = 0;
                        t->val = j.tomb;
                        *(u64x2*)&t->st[0] = z;
                        died++;
                    }
                    s_hf[h] = 0;
                } else {
                    if (sl == SIDE_ID) j.ctl->sp.val = s_lv[h];
                    else if (sl != FULL_SLOT) j.table[sl].val = s_lv[h];  // (streamed, with the answers: slower, profiles/r06/papply_nt.txt)
                }
                if (h < HT) s_hk[h] = EMPTY_KEY;
                s_hp[h] = 0;
                s_h1[h] = NOFIRST;
            }
        }
        __syncthreads();  // hash entries free; the next iteration builds the map after next in s_tile[pb]
        if (base == 0) PA_MARK(4, wall_clock64());
    }
    if (created) atomicAdd(&s_created, created);
    if (RM && died) atomicAdd(&s_died, died);
    __syncthreads();
    if (threadIdx.x == 0 && s_created) atomicAdd(&j.created_acc[b % HM_CREATED_SLOTS], (u64)s_created);
    if (RM && threadIdx.x == 0 && s_died) atomicAdd(&j.dead_acc[b % HM_CREATED_SLOTS], (u64)(long long)s_died);
    PA_MARK(5, wall_clock64());
#undef PA_MARK
}

// ---- small rounds: one workgroup, one launch (the flat combiner's batches) ----------------------
// A round of at most SM_W Puts and SM_R Gets, whole in one 1024-thread workgroup: the Puts are
// hashed by key in LDS (how many, the last one); one thread per distinct key finds or claims
// its slot, answers the previous values of the key's Puts in log order (the slot's value before
// the round for the first; nr/examples/hashmap.rs:46-50) and stores the last value. No deferred
// half and no device atomics per Put: round 2's index + elector + reads launches for the
// combiner's batches (about 20 us of GPU time for a few hundred ops) became one.
// The Gets do not wait for the Puts: a Get of a key the round Puts is answered from the LDS hash
// (the key's last value), and for any other key the round changes nothing the Get reads -- a
// present key's probe chain holds no empty slot, so claims (which fill empty slots) cannot
// change where its chain ends, and only Put keys' values are stored. So every Get's table probe
// is issued with the Put records, and resolves while the Puts claim and store.
// Runs with no other round in flight (the caller flushes first). Keys present in the table are
// present (quiescent: no claim in flight); fresh claims get epoch-1 stamps, as the partition
// apply's.
constexpr int SM_TPB = 1024;
constexpr u32 SM_W = 2048, SM_R = 8192, SM_HT = 4096;  // SM_HT: LDS hash entries (+1: the side key)
struct SmallJob {
    RecSrc rec;
    nrg_put* ring_out;  // log copy to write (nullptr: the records are in the ring)
    u32 n;
    u64 lo, resp_lo, resp_hi;
    u64* prev;
    uint8_t* prevf;
    const u64* keys;  // Gets
    u32 R;
    u64* vals;
    uint8_t* found;
    u32* e_out;  // the replica's error latch after the round (the combiner's batch), or nullptr
    u64* created_acc;
};

__device__ __forceinline__ u32 sm_hash(u64 k) { return (u32)(mix64(k) >> 40) & (SM_HT - 1); }

struct SmallLds {
    u64 val[SM_W];
    uint16_t ent[SM_W];    // hash entry of each Put
    u64 hk[SM_HT];
    u32 cnt[SM_HT + 1];    // Puts of the key; [SM_HT]: the side key
    u32 last[SM_HT + 1];   // its last Put + 1
    u32 created;
};

// a word for the host, stored write-through (system scope: the line leaves the L2), so the host
// sees it now and not at the next L2 writeback (the resident server has no kernel end to flush it)
__device__ __forceinline__ void host_put(u64* p, u64 v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// RQ Gets per thread (RQ * SM_TPB <= SM_R per round); FLUSH: the responses and the error word are
// made visible to the host at once (the resident server's rounds)
template <int RQ, bool FLUSH>
__device__ __forceinline__ void small_body(const SmallJob& j, Slot* table, u32 shift, u64 tmask, DevCtl* ctl,
                                           SmallLds& L) {
    u64* s_val = L.val;
    uint16_t* s_ent = L.ent;
    u64* s_hk = L.hk;
    u32* s_cnt = L.cnt;
    u32* s_last = L.last;
    u32& s_created = L.created;
    const int tid = threadIdx.x;
    constexpr int WQ = (int)(SM_W / SM_TPB);
    // every Put record, every Get key and every Get's first probe in flight together
    nrg_put r[WQ];
#pragma unroll
    for (int q = 0; q < WQ; q++) {
        const u32 i = q * SM_TPB + tid;
        r[q] = i < j.n ? j.rec.at(i) : nrg_put{EMPTY_KEY, 0};
    }
    u64 k[RQ], s[RQ];
    u64x2 w[RQ];
#pragma unroll
    for (int q = 0; q < RQ; q++) {
        const u32 i = q * SM_TPB + tid;
        k[q] = i < j.R ? j.keys[i] : EMPTY_KEY;
    }
#pragma unroll
    for (int q = 0; q < RQ; q++) {
        const u32 i = q * SM_TPB + tid;
        s[q] = table_home(k[q], shift);
        w[q].x = EMPTY_KEY;
        w[q].y = 0;
        if (i < j.R && k[q] != EMPTY_KEY) w[q] = *(const u64x2*)&table[s[q]];
    }
    for (int h = tid; h <= (int)SM_HT; h += SM_TPB) {
        if (h < (int)SM_HT) s_hk[h] = EMPTY_KEY;
        s_cnt[h] = 0;
        s_last[h] = 0;
    }
    if (tid == 0) s_created = 0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < WQ; q++) {
        const u32 i = q * SM_TPB + tid;
        if (i >= j.n) continue;
        if (j.ring_out) j.ring_out[(j.rec.lo + i) & j.rec.mask] = r[q];
        s_val[i] = r[q].val;
        const u64 kk = r[q].key;
        u32 h = SM_HT;
        if (kk != EMPTY_KEY) {
            h = sm_hash(kk);
            for (;;) {  // at most SM_W keys in SM_HT entries: an entry is always found
                const u64 old = atomicCAS((unsigned long long*)&s_hk[h], (unsigned long long)EMPTY_KEY,
                                          (unsigned long long)kk);
                if (old == EMPTY_KEY || old == kk) break;
                h = (h + 1) & (SM_HT - 1);
            }
        }
        s_ent[i] = (uint16_t)h;
        atomicAdd(&s_cnt[h], 1u);
        atomicMax(&s_last[h], i + 1);
    }
    __syncthreads();
    // one thread per distinct key: its slot, its Puts' previous values, its last value
    u32 created = 0;
    for (int h = tid; h <= (int)SM_HT; h += SM_TPB) {
        const u32 c = s_cnt[h];
        if (!c) continue;
        u64 cur = 0;
        bool has = false;
        Slot* slot = nullptr;
        if (h == (int)SM_HT) {  // the key EMPTY_KEY lives in the side slot
            has = ctl->sp_claim != 0;
            if (has) {
                cur = ctl->sp.val;
            } else {
                ctl->sp_claim = 1;
                ctl->sp.st[0] = ctl->sp.st[1] = STAMP_PRESENT;
                created++;
            }
        } else {
            bool fresh = false;
            const u64 kk = s_hk[h];
            const long long sl = claim_slot(table, kk, table_home(kk, shift), tmask, &fresh);
            if (sl < 0) {
                atomicOr(&ctl->err, ERR_TABLE_FULL);
                // its Puts answer None, as the partition apply answers a Put that found no slot
                for (u32 i = 0, seen = 0; j.prev && seen < c; i++) {
                    if (s_ent[i] != (uint16_t)h) continue;
                    seen++;
                    const u64 g = j.lo + i;
                    if (g >= j.resp_lo && g < j.resp_hi) {
                        j.prev[g - j.resp_lo] = 0;
                        j.prevf[g - j.resp_lo] = 0;
                    }
                }
                s_cnt[h] = 0;  // the Gets of this key find it absent, as the other paths leave it
                continue;
            }
            slot = &table[sl];
            if (fresh) {
                slot->st[0] = slot->st[1] = STAMP_PRESENT;
                created++;
            } else {
                cur = slot->val;
                has = true;
            }
        }
        const u32 last = s_last[h] - 1;
        if (c == 1) {  // the common case: one Put of the key in the round
            const u64 g = j.lo + last;
            if (j.prev && g >= j.resp_lo && g < j.resp_hi) {
                j.prev[g - j.resp_lo] = has ? cur : 0;
                j.prevf[g - j.resp_lo] = has ? 1 : 0;
            }
            cur = s_val[last];
        } else {  // the key's Puts in log order (a scan of the round; rare for uniform keys)
            for (u32 i = 0, seen = 0; seen < c; i++) {
                if (s_ent[i] != (uint16_t)h) continue;
                seen++;
                const u64 g = j.lo + i;
                if (j.prev && g >= j.resp_lo && g < j.resp_hi) {
                    j.prev[g - j.resp_lo] = has ? cur : 0;
                    j.prevf[g - j.resp_lo] = has ? 1 : 0;
                }
                cur = s_val[i];
                has = true;
            }
        }
        if (slot) slot->val = cur;
        else ctl->sp.val = cur;
    }
    if (created) atomicAdd(&s_created, created);
    // Gets: keys of the round's Puts from the LDS hash (read only after the barrier: a full
    // table zeroes the key's count above), every other key from its probe chain
    const u64 sp_val = ctl->sp.val;
    const bool sp_has = ctl->sp_claim != 0;
    __syncthreads();
    if (tid == 0 && s_created) atomicAdd(&j.created_acc[0], (u64)s_created);
#pragma unroll
    for (int q = 0; q < RQ; q++) {
        const u32 i = q * SM_TPB + tid;
        if (i >= j.R) continue;
        u64 v = 0;
        bool f = false;
        u32 h = SM_HT;
        if (k[q] != EMPTY_KEY) {
            h = sm_hash(k[q]);
            while (s_hk[h] != k[q] && s_hk[h] != EMPTY_KEY) h = (h + 1) & (SM_HT - 1);
            if (s_hk[h] != k[q]) h = SM_HT + 1;  // not a key of the round's Puts
        }
        if (h <= SM_HT && s_cnt[h]) {
            f = true;
            v = s_val[s_last[h] - 1];
        } else if (k[q] == EMPTY_KEY) {
            f = sp_has;
            v = f ? sp_val : 0;
        } else {
            u64 kk = w[q].x, vv = w[q].y;
            for (u64 pr = 0; pr <= tmask; pr++) {
                if (kk == k[q]) {
                    f = true;
                    v = vv;
                    break;
                }
                if (kk == EMPTY_KEY) break;
                const u64 sl = probe_slot(s[q], pr + 1, tmask);
                const u64x2 x = *(const u64x2*)&table[sl];
                kk = x.x;
                vv = x.y;
            }
        }
        j.vals[i] = v;
        j.found[i] = f ? 1 : 0;
    }
    if (j.e_out) {  // the round's last write: the host (nrg_combiner) polls it as the round's completion
        // every wave's response stores issued before the barrier (the barrier alone does not wait
        // for them), then one lane's system release and the word (MI355X_MICROARCH.md, producer form)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            const u32 e = atomicExch(&ctl->err, 0u);
            if constexpr (FLUSH) {
                // the responses (plain stores, every wave waited for them above) written back
                // from the L2 by one system release, then the word itself write-through: the
                // resident server has no kernel end to write its L2 back (write-through stores
                // of every response, bytes included, measured slower: 18.8 vs 15.2 us a round)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
                __hip_atomic_store(j.e_out, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            } else {
                __threadfence_system();
                *(volatile u32*)j.e_out = e;
            }
        }
    }
}

__global__ __launch_bounds__(SM_TPB) void hm_small_round_kernel(SmallJob j, Slot* table, u32 shift, u64 tmask,
                                                                DevCtl* ctl) {
    __shared__ SmallLds L;
    small_body<(int)(SM_R / SM_TPB), false>(j, table, shift, tmask, ctl, L);
}

// ---- the combiner's round server: small rounds without a launch per round -----------------------
// One resident workgroup serves the flat combiner's hashmap batches (nrg_combiner) from mapped
// host memory. It reads every batch slot's fixed job fields (its buffers) once, then per round k
// polls slot k's doorbell, `(k + 1) << 32 | Puts << 16 | Gets`, runs the round as
// hm_small_round_kernel would (its log position tracked here: each round starts where the last
// ended) and ends it with the batch's error word, as there, and `served`. The host's launch and the
// dispatch from an idle queue leave the round's critical path. It exits when the host asks
// (`stop`, every rung round served) or after idle_ticks of the 100-MHz wall clock without a round,
// and then writes its session number to `exited`: every wave reaches that exit, so a host that
// stops posting (or dies) never leaves it running. A host that finds `exited` at its session with
// rounds still unserved relaunches from `served` (the old server never reads a doorbell again).
static_assert(sizeof(SmallJob) <= sizeof(SmallJobBlob), "a server slot holds one SmallJob");
static_assert(SERVE_R <= SM_R && SERVE_R % SM_TPB == 0, "server rounds are small rounds");
__device__ __forceinline__ u64 sgpr64(u64 v) {
    // (readfirstlane returns int: through u32, or a set bit 31 sign-extends over the high word)
    return ((u64)(u32)__builtin_amdgcn_readfirstlane((u32)(v >> 32)) << 32) |
           (u64)(u32)__builtin_amdgcn_readfirstlane((u32)v);
}
__global__ __launch_bounds__(SM_TPB) void hm_serve_kernel(ServeCtl* sc, const SmallJobBlob* hdr, u32 nslots, u64 first,
                                                          u64 first_lo, u64 session, u64 idle_ticks, Slot* table,
                                                          u32 shift, u64 tmask, DevCtl* ctl) {
    __shared__ SmallLds L;
    __shared__ SmallJob s_job[SERVE_SLOTS];  // the slots' fixed job fields, read once
    __shared__ int s_cmd;
    __shared__ u32 s_n, s_r;
    __shared__ u64 s_k, s_lo;  // (in LDS: nothing of the loop stays live in registers across a round)
    constexpr u32 JW = (u32)(sizeof(SmallJob) / 8);
    static_assert(sizeof(SmallJob) % 8 == 0, "job copied in words");
    for (u32 t = threadIdx.x; t < nslots * JW; t += SM_TPB)
        ((u64*)s_job)[t] = __hip_atomic_load((const u64*)hdr[t / JW].b + t % JW, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_SYSTEM);
    if (threadIdx.x == 0) {
        s_k = first;
        s_lo = first_lo;
    }
    __syncthreads();
    // wave 0 polls the round's doorbell, as a whole wave in uniform control flow (readfirstlane'd
    // values, scalar branches): a loop run by lane 0 alone under an exec mask never saw the host's
    // next post (microbench/serve_mech.hip)
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (;;) {
        if (wave == 0) {
            const u64 k = sgpr64(s_k);
            const u64* door = &sc->door[k % nslots];
            const u64 t0 = wall_clock64();
            u64 d = 0;
            int cmd = 0;
            for (u64 polls = 0;; polls++) {
                d = sgpr64(__hip_atomic_load(door, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM));
                if ((polls & 4095) == 0 && threadIdx.x == 0) {  // (diagnostic trace, Combiner.probe)
                    host_put(&sc->trace[1], k);
                    host_put(&sc->trace[2], d >> 32);
                    host_put(&sc->trace[3], polls);
                }
                if ((d >> 32) == k + 1) {
                    cmd = 1;
                    break;
                }
                if (__builtin_amdgcn_readfirstlane(__hip_atomic_load(&sc->stop, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM))) {
                    // the host rings every doorbell before it asks to stop: look once more
                    d = sgpr64(__hip_atomic_load(door, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM));
                    cmd = (d >> 32) == k + 1 ? 1 : 0;
                    break;
                }
                if (wall_clock64() - t0 > idle_ticks) break;
                __builtin_amdgcn_s_sleep(2);
            }
            if (threadIdx.x == 0) {
                s_cmd = cmd;
                s_n = (u32)(d >> 16) & 0xFFFFu;
                s_r = (u32)d & 0xFFFFu;
            }
        }
        __syncthreads();  // (also: every wave is done with the previous round's LDS)
        if (!s_cmd) break;
        // the round's job: the slot's fixed fields, the round's counts, its log position
        const SmallJob& h = s_job[s_k % nslots];
        const u64 lo = sgpr64(s_lo);
        const u32 n = (u32)__builtin_amdgcn_readfirstlane(s_n), R = (u32)__builtin_amdgcn_readfirstlane(s_r);
        SmallJob j;
        j.rec.src = (const nrg_put*)sgpr64((u64)h.rec.src);
        j.rec.ring = (const nrg_put*)sgpr64((u64)h.rec.ring);
        j.rec.mask = sgpr64(h.rec.mask);
        j.rec.lo = lo;
        j.ring_out = (nrg_put*)sgpr64((u64)h.ring_out);
        j.n = n;
        j.lo = lo;
        j.resp_lo = lo;
        j.resp_hi = lo + n;
        j.prev = n ? (u64*)sgpr64((u64)h.prev) : nullptr;
        j.prevf = n ? (uint8_t*)sgpr64((u64)h.prevf) : nullptr;
        j.keys = R ? (const u64*)sgpr64((u64)h.keys) : nullptr;
        j.R = R;
        j.vals = (u64*)sgpr64((u64)h.vals);
        j.found = (uint8_t*)sgpr64((u64)h.found);
        j.e_out = (u32*)sgpr64((u64)h.e_out);
        j.created_acc = (u64*)sgpr64((u64)h.created_acc);
        small_body<(int)(SERVE_R / SM_TPB), true>(j, table, shift, tmask, ctl, L);  // ends with the error word
        if (threadIdx.x == 0) {
            s_k = s_k + 1;
            s_lo = s_lo + n;
            host_put(&sc->served, s_k);
        }
    }
    if (threadIdx.x == 0) {
        __threadfence_system();
        host_put(&sc->exited, session);
    }
}

static RecSrc ring_src(nrg_ctx* c, const nrg_put* src, u64 lo);
static hipError_t hm_flush(nrg_ctx* c);
static hipError_t hm_count(nrg_ctx* c);  // DevCtl::nkeys_total = number of keys

// A round through hm_small_round_kernel (hm_replay_chunk decides; n <= SM_W, R <= SM_R).
static hipError_t small_round(nrg_ctx* c, const nrg_put* src, u64 lo, u64 n, bool write_ring, const u64* keys, u64 R,
                              u64* vals, uint8_t* found, u64 resp_lo, u64 resp_hi, u64* prev, uint8_t* prevf) {
    hipError_t e = hm_flush(c);
    if (e != hipSuccess) return e;
    SmallJob j;
    j.rec = ring_src(c, src, lo);
    j.ring_out = write_ring ? (nrg_put*)c->d_ring : nullptr;
    j.n = (u32)n;
    j.lo = lo;
    j.resp_lo = resp_lo;
    j.resp_hi = resp_hi;
    j.prev = prev;
    j.prevf = prev ? prevf : nullptr;
    j.keys = keys;
    j.R = keys ? (u32)R : 0u;
    j.vals = vals;
    j.found = found;
    j.e_out = c->hm.err_out;
    c->hm.err_out = nullptr;
    j.created_acc = c->hm.d_created;
    NRG_LAUNCH(c, "hm_small", hm_small_round_kernel, 1, SM_TPB, 0, c->stream, j, c->hm.d_table, c->hm.slot_shift,
               (u64)(c->hm.slots - 1), c->d_ctl);
    return hipGetLastError();
}

// The job of a small round of records [lo, lo + W) (hm_small_round_kernel's, as small_round would
// launch it with the log copy written) into `blob`, for hm_serve_kernel; hm_small_job
// does the replica's log bookkeeping around it.
bool hm_small_fill(nrg_ctx* c, const nrg_put* recs, u64 lo, u64 W, const u64* keys, u64 R, u64* vals, uint8_t* found,
                   u64* prev, uint8_t* prevf, u32* e_out, SmallJobBlob* blob) {
    if (W > SM_W || R > SERVE_R || c->hm.pend.valid) return false;
    if (!blob) return true;  // (the server's slots hold the fixed fields; only the checks)
    SmallJob j;
    j.rec = ring_src(c, recs, lo);
    j.ring_out = (nrg_put*)c->d_ring;
    j.n = (u32)W;
    j.lo = lo;
    j.resp_lo = lo;
    j.resp_hi = lo + W;
    j.prev = (prev && prevf && W) ? prev : nullptr;
    j.prevf = j.prev ? prevf : nullptr;
    j.keys = R ? keys : nullptr;
    j.R = R ? (u32)R : 0u;
    j.vals = vals;
    j.found = found;
    j.e_out = e_out;
    j.created_acc = c->hm.d_created;
    std::memcpy(blob->b, &j, sizeof j);
    return true;
}

hipError_t hm_serve_launch(nrg_ctx* c, ServeCtl* sc, const SmallJobBlob* hdr, u32 nslots, u64 first, u64 first_lo,
                           u64 session, u64 idle_ticks) {
    if (nslots > SERVE_SLOTS) return hipErrorInvalidValue;
    NRG_LAUNCH(c, "hm_serve", hm_serve_kernel, 1, SM_TPB, 0, c->stream, sc, hdr, nslots, first, first_lo, session,
               idle_ticks, c->hm.d_table, c->hm.slot_shift, (u64)(c->hm.slots - 1), c->d_ctl);
    return hipGetLastError();
}

__global__ __launch_bounds__(TPB) void hm_init_table_kernel(Slot* table, u64 slots) {
    for (u64 s = blockIdx.x * (u64)TPB + threadIdx.x; s < slots; s += (u64)gridDim.x * TPB) {
        u64x2 z;
        z.x = EMPTY_KEY;
        z.y = 0;
        *(u64x2*)&table[s] = z;
        z.x = z.y = 0;
        *(u64x2*)&table[s].st[0] = z;
    }
}

// ---- hm_rehash_kernel: table growth (hm_grow) ------------------------------------------------------
// Every key of the old table moves to the new, larger one: claimed from its new home, its value
// copied, both stamps "present since before the replay rounds" (the epochs restart, as after
// hm_renorm_kernel). Nothing else runs on the replica (hm_grow flushed the deferred half), so every
// non-empty old slot holds a present key and the old stamps are not needed: a lane loads the 16 B
// {key, value} of its slot, a wave 64 consecutive slots (the memory side moves their 16 lines whole
// either way).
// The home slot is the TOP bits of mix64(key) (table_home), so growing by 2^d sends old home h to
// (h << d) | the next d bits: the map is monotone, and a key found at old slot s lands near s << d
// (its old home h lies in s's group of four or, for the few keys that met a full group, in a group
// shortly before it: probe_slot goes round the home group and then forward group by group, so s
// may sit up to three slots before h but never a group before it). So each workgroup takes a
// CONTIGUOUS run of RH_RUN old slots (128 KiB), not a grid-stride interleave: its claims, stamps and
// values fall into one contiguous region of the new table (RH_RUN << d slots), the lines it
// dirties are dirtied while they sit in its XCD's L2, and the pass streams through both tables
// instead of writing a random line per key. Probe chains cross the regions' edges and wrap at the
// table's end; the 64-bit CAS of the claim makes that safe without any order between workgroups.
// A thread takes RH_Q slots at a time, RH_TPB apart: their loads are in flight together, then their
// claims. A claim is the CAS alone, from the home slot on, with no first probe of the slot as
// claim_slot / pa_resolve make it: the new table holds none of the keys being moved and, when the load limit
// manages it, at most one key per four slots, so the probe would nearly always read "empty" and only add a memory round
// trip and a request per key (configs[1], 2^26 -> 2^27 slots, 10M keys: 1222 us with pa_resolve,
// 898-950 us with the CAS alone).
constexpr int RH_TPB = 256, RH_Q = 8;
constexpr u64 RH_RUN = 4096;  // old slots per workgroup
static_assert(RH_RUN % ((u64)RH_TPB * RH_Q) == 0, "a run is whole batches");
// With removal enabled (rm) a dead slot (val == tomb) is not moved, and a dead side key gives its slot
// back: after a rehash every taken slot holds a live key. The new table may then be one of the SAME
// size (hm_grow's purge).
__global__ __launch_bounds__(RH_TPB) void hm_rehash_kernel(const Slot* __restrict__ old, u64 old_slots, Slot* table,
                                                           u32 shift, u64 tmask, DevCtl* ctl, bool rm, u64 tomb) {
    __shared__ u32 s_moved;
    if (threadIdx.x == 0) s_moved = 0;
    __syncthreads();
    const u64 run0 = (u64)blockIdx.x * RH_RUN;
    u32 moved = 0;
    for (u64 b0 = run0; b0 < run0 + RH_RUN && b0 < old_slots; b0 += (u64)RH_TPB * RH_Q) {
        u64 k[RH_Q], v[RH_Q];
        bool on[RH_Q];
#pragma unroll
        for (int q = 0; q < RH_Q; q++) {
            const u64 s = b0 + (u64)q * RH_TPB + threadIdx.x;
            u64x2 e;
            e.x = EMPTY_KEY;
            e.y = 0;
            if (s < old_slots) e = *(const u64x2*)&old[s];
            k[q] = e.x;
            v[q] = e.y;
            on[q] = e.x != EMPTY_KEY && !(rm && e.y == tomb);
        }
        u64 s[RH_Q];
        bool any = false;
#pragma unroll
        for (int q = 0; q < RH_Q; q++) {
            s[q] = table_home(k[q], shift);
            any = any || on[q];
        }
        for (u64 pr = 0; any && pr <= tmask; pr++) {
            u64 was[RH_Q];
#pragma unroll
            for (int q = 0; q < RH_Q; q++)
                if (on[q])
                    was[q] = atomicCAS((unsigned long long*)&table[s[q]].key, (unsigned long long)EMPTY_KEY,
                                       (unsigned long long)k[q]);
            any = false;
#pragma unroll
            for (int q = 0; q < RH_Q; q++) {
                if (!on[q]) continue;
                if (was[q] == EMPTY_KEY || was[q] == k[q]) {
                    u64x2 z;
                    z.x = z.y = STAMP_PRESENT;
                    *(u64x2*)&table[s[q]].st[0] = z;
                    table[s[q]].val = v[q];
                    moved++;
                    on[q] = false;
                } else {
                    s[q] = probe_next(s[q], pr, tmask);
                    any = true;
                }
            }
        }
        if (any) atomicOr(&ctl->err, ERR_TABLE_FULL);  // (cannot happen: the new table is the larger one)
    }
    if (moved) atomicAdd(&s_moved, moved);
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 m = s_moved;
        if (blockIdx.x == 0 && ctl->sp_claim) {  // the side slot lives in DevCtl and does not move
            if (rm && ctl->sp.val == tomb) {
                ctl->sp_claim = 0;
            } else {
                ctl->sp.st[0] = ctl->sp.st[1] = STAMP_PRESENT;
                m++;
            }
        }
        if (m) atomicAdd((unsigned long long*)&ctl->nkeys, (unsigned long long)m);  // (hm_grow zeroed it)
    }
}

// Epoch renormalisation (before the 32-bit epoch wraps): every present key becomes "present
// since before the replay rounds" (epoch 1); claims in flight do not exist at this point.
// With removal enabled (rm) a dead slot (val == tomb, stamps 0) stays dead.
__global__ __launch_bounds__(TPB) void hm_renorm_kernel(Slot* table, u64 slots, DevCtl* ctl, bool rm, u64 tomb) {
    for (u64 s = blockIdx.x * (u64)TPB + threadIdx.x; s < slots; s += (u64)gridDim.x * TPB) {
        const u64x2 e = *(const u64x2*)&table[s];
        if (e.x == EMPTY_KEY || (rm && e.y == tomb)) continue;
        u64x2 z;
        z.x = z.y = STAMP_PRESENT;
        *(u64x2*)&table[s].st[0] = z;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && ctl->sp_claim && !(rm && ctl->sp.val == tomb))
        ctl->sp.st[0] = ctl->sp.st[1] = STAMP_PRESENT;
}

// NrHashMap::default (benches/hashmap.rs:91-100): keys 0..n-1 -> k + off, inserted directly.
// With removal enabled (dead_acc given; no value is the tombstone, the host checked) a key whose slot is
// dead is revived: counted out of dead_acc, so both counts stay exact.
__global__ __launch_bounds__(TPB) void hm_prefill_range_kernel(Slot* table, u64 n, u64 off, u32 shift, u64 tmask,
                                                               DevCtl* ctl, u32 part, u32 parts, u64 tomb,
                                                               u64* dead_acc) {
    __shared__ u32 s_ins, s_rev;
    if (threadIdx.x == 0) s_ins = s_rev = 0;
    __syncthreads();
    u32 inserted = 0, revived = 0;
    for (u64 k = blockIdx.x * (u64)TPB + threadIdx.x; k < n; k += (u64)gridDim.x * TPB) {
        if (parts > 1 && key_owner(k, parts) != part) continue;  // a key partition's share only
        if (k == EMPTY_KEY) {  // only reachable for n = 2^64, kept for the full key domain
            inserted += ctl->sp_claim == 0;
            revived += dead_acc && ctl->sp_claim && ctl->sp.val == tomb;
            ctl->sp.val = k + off;
            ctl->sp.st[0] = ctl->sp.st[1] = STAMP_PRESENT;
            ctl->sp_claim = 1;
            continue;
        }
        bool fresh;
        const long long s = claim_slot(table, k, table_home(k, shift), tmask, &fresh);
        if (s < 0) {
            atomicOr(&ctl->err, ERR_TABLE_FULL);
            continue;
        }
        revived += dead_acc && !fresh && table[s].val == tomb;
        table[s].val = k + off;
        table[s].st[0] = table[s].st[1] = STAMP_PRESENT;
        inserted += fresh;
    }
    if (inserted) atomicAdd(&s_ins, inserted);
    if (revived) atomicAdd(&s_rev, revived);
    __syncthreads();
    if (threadIdx.x == 0 && s_ins) atomicAdd(&ctl->nkeys, (u64)s_ins);
    if (threadIdx.x == 0 && s_rev) atomicAdd(&dead_acc[blockIdx.x % HM_CREATED_SLOTS], 0ull - (u64)s_rev);
}

// number of keys = direct inserts (ctl->nkeys) + keys created by replay rounds
// With removal enabled (dead given) that sum is the occupancy, the slots taken (DevCtl::occ_total), and
// the number of keys is the occupancy minus the dead slots (deaths minus revivals, a wrapping sum).
__global__ __launch_bounds__(TPB) void hm_count_kernel(const u64* __restrict__ acc, u64 n, DevCtl* ctl,
                                                       const u64* __restrict__ dead) {
    __shared__ u64 s_w[TPB / 64], s_d[TPB / 64];
    u64 x = 0, d = 0;
    for (u64 q = threadIdx.x; q < n; q += TPB) {
        x += acc[q];
        if (dead) d += dead[q];
    }
    for (int off = 32; off > 0; off >>= 1) {
        x += __shfl_xor(x, off, 64);
        d += __shfl_xor(d, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_w[threadIdx.x >> 6] = x;
        s_d[threadIdx.x >> 6] = d;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 t = ctl->nkeys, dd = 0;
        for (int w = 0; w < TPB / 64; w++) {
            t += s_w[w];
            dd += s_d[w];
        }
        ctl->occ_total = t;
        ctl->nkeys_total = t - dd;
    }
}

// nrg_hashmap_enable_removal / nrg_restore into an enabled context: how many of the n {key, value}
// pairs, `stride` words apart, hold `tomb` as their value (table: empty slots are no pairs), added to
// DevCtl::counter.
__global__ __launch_bounds__(TPB) void hm_find_val_kernel(const u64* __restrict__ pairs, u64 n, u32 stride, bool table,
                                                          u64 tomb, DevCtl* ctl) {
    u32 hits = 0;
    for (u64 i = blockIdx.x * (u64)TPB + threadIdx.x; i < n; i += (u64)gridDim.x * TPB) {
        const u64x2 e = *(const u64x2*)&pairs[i * stride];
        hits += e.y == tomb && !(table && e.x == EMPTY_KEY);
    }
    if (table && blockIdx.x == 0 && threadIdx.x == 0 && ctl->sp_claim && ctl->sp.val == tomb) hits++;
    for (int off = 32; off > 0; off >>= 1) hits += __shfl_xor(hits, off, 64);
    if ((threadIdx.x & 63) == 0 && hits) atomicAdd(&ctl->counter, (u64)hits);
}

// (rm, here and in the digest and the snapshot: removal is enabled, and a slot whose value is tomb is
// dead, a removed key that keeps its slot; no live value equals tomb there)
__global__ __launch_bounds__(TPB) void hm_dump_kernel(const Slot* __restrict__ table, u64 slots, DevCtl* ctl,
                                                      u64* __restrict__ ok, u64* __restrict__ ov, bool rm, u64 tomb) {
    const u64 gid = blockIdx.x * (u64)TPB + threadIdx.x;
    if (gid == 0 && ctl->sp_claim && !(rm && ctl->sp.val == tomb)) {
        const u64 i = atomicAdd(&ctl->counter, 1ull);
        ok[i] = EMPTY_KEY;
        ov[i] = ctl->sp.val;
    }
    for (u64 s = gid; s < slots; s += (u64)gridDim.x * TPB) {
        const u64x2 e = *(const u64x2*)&table[s];
        if (e.x != EMPTY_KEY && !(rm && e.y == tomb)) {
            const u64 i = atomicAdd(&ctl->counter, 1ull);
            ok[i] = e.x;
            ov[i] = e.y;
        }
    }
}

__global__ __launch_bounds__(TPB) void hm_digest_kernel(const Slot* __restrict__ table, u64 slots,
                                                        const DevCtl* ctl, u64* out3, bool rm, u64 tomb) {
    __shared__ u64 s_c[TPB / 64], s_s[TPB / 64], s_x[TPB / 64];
    const u64 gid = blockIdx.x * (u64)TPB + threadIdx.x;
    u64 c = 0, sm = 0, x = 0;
    if (gid == 0 && ctl->sp_claim && !(rm && ctl->sp.val == tomb)) {
        const u64 h = mix64(EMPTY_KEY ^ mix64(ctl->sp.val));
        c++;
        sm += h;
        x ^= h;
    }
    for (u64 s = gid; s < slots; s += (u64)gridDim.x * TPB) {
        const u64x2 e = *(const u64x2*)&table[s];
        if (e.x != EMPTY_KEY && !(rm && e.y == tomb)) {
            const u64 h = mix64(e.x ^ mix64(e.y));
            c++;
            sm += h;
            x ^= h;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        c += __shfl_xor(c, off, 64);
        sm += __shfl_xor(sm, off, 64);
        x ^= __shfl_xor(x, off, 64);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_c[w] = c;
        s_s[w] = sm;
        s_x[w] = x;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        c = sm = x = 0;
        for (int v = 0; v < TPB / 64; v++) {
            c += s_c[v];
            sm += s_s[v];
            x ^= s_x[v];
        }
        atomicAdd(&out3[0], c);
        atomicAdd(&out3[1], sm);
        atomicXor(&out3[2], x);
    }
}

// ---- nrg_snapshot_async / nrg_restore ----------------------------------------------------------
// hm_snapshot_kernel: the present {key, value} pairs of the whole table, written densely, in any
// order. The table is read as hm_digest_kernel reads it (a lane loads the 16 B {key, value} of its
// slot). A workgroup takes tiles of SN_TILE consecutive slots (128 KiB of table): every lane holds
// SN_Q slots, a wave counts each of its SN_Q rows with a ballot, the SN_Q * 4 row counts are
// scanned by the first wave (one per lane), and ONE returning atomic per tile on DevCtl::counter
// reserves the tile's run of the output: 2^26 slots make 16384 atomics on that word, about 30 per
// us of the scan, a third of what one word takes (the dump's one atomic per key: 10M). A tile
// whose run would pass cap_items stores nothing, but still counts, so the head kernel sees the
// overrun. No workgroup waits for another.
constexpr int SN_Q = 16;
constexpr u64 SN_TILE = (u64)TPB * SN_Q;
static_assert(SN_Q * (TPB / 64) == 64, "the row counts of a tile are scanned by one wave, one per lane");
__global__ __launch_bounds__(TPB) void hm_snapshot_kernel(const Slot* __restrict__ table, u64 slots, DevCtl* ctl,
                                                          u64x2* __restrict__ out, u64 cap_items, bool rm,
                                                          u64 tomb) {
    __shared__ u32 s_cnt[64];
    __shared__ u64 s_base;
    const u32 lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const u64 tiles = (slots + SN_TILE - 1) / SN_TILE;
    for (u64 t = blockIdx.x; t < tiles; t += gridDim.x) {
        const u64 s0 = t * SN_TILE + threadIdx.x;
        u64x2 e[SN_Q];
        u32 rank[SN_Q];
#pragma unroll
        for (int q = 0; q < SN_Q; q++) {
            const u64 s = s0 + (u64)q * TPB;
            e[q].x = EMPTY_KEY;
            e[q].y = 0;
            if (s < slots) e[q] = *(const u64x2*)&table[s];
            if (rm && e[q].y == tomb) e[q].x = EMPTY_KEY;  // a dead slot: no pair
        }
#pragma unroll
        for (int q = 0; q < SN_Q; q++) {
            const u64 b = __ballot(e[q].x != EMPTY_KEY);
            rank[q] = (u32)__popcll(b & ((1ull << lane) - 1));
            if (lane == 0) s_cnt[q * (TPB / 64) + w] = (u32)__popcll(b);
        }
        __syncthreads();
        if (w == 0) {
            const u32 c = s_cnt[lane];
            u32 incl = c;
            for (int off = 1; off < 64; off <<= 1) {
                const u32 v = __shfl_up(incl, off, 64);
                if ((int)lane >= off) incl += v;
            }
            s_cnt[lane] = incl - c;  // where the row's pairs start inside the tile's run
            if (lane == 63) {
                u64 base = ~0ull;
                if (incl) {
                    base = atomicAdd((unsigned long long*)&ctl->counter, (unsigned long long)incl);
                    if (base + incl > cap_items) base = ~0ull;
                }
                s_base = base;
            }
        }
        __syncthreads();
        const u64 base = s_base;
        if (base != ~0ull) {
#pragma unroll
            for (int q = 0; q < SN_Q; q++)
                if (e[q].x != EMPTY_KEY) out[base + s_cnt[q * (TPB / 64) + w] + rank[q]] = e[q];
        }
        __syncthreads();  // (s_cnt and s_base are the next tile's too)
    }
}

// After the scan: the side key's pair behind the table's, then the header or the refusal.
__global__ void hm_snapshot_head_kernel(DevCtl* ctl, u64* buf, u64 cap, u64 log_idx, bool rm, u64 tomb) {
    if (threadIdx.x || blockIdx.x) return;
    u64 n = ctl->counter;
    const u64 cap_items = cap >= SNAP_HDR ? (cap - SNAP_HDR) / 16 : 0;
    if (ctl->sp_claim && !(rm && ctl->sp.val == tomb)) {
        if (n < cap_items) {
            buf[SNAP_HDR / 8 + 2 * n] = EMPTY_KEY;
            buf[SNAP_HDR / 8 + 2 * n + 1] = ctl->sp.val;
        }
        n++;
    }
    snap_head(buf, cap, NRG_DS_HASHMAP, n, n * 16, log_idx, ctl);
}

// The snapshot's pairs into a table hm_init_table_kernel has just initialised: claimed from the
// home slot as hm_prefill_range_kernel claims them, stamps "present since before the replay
// rounds", the key EMPTY_KEY into the side slot. Fresh claims are counted into DevCtl::nkeys, so a
// payload that repeats a key restores fewer keys than its header says and fails the digest check.
__global__ __launch_bounds__(TPB) void hm_restore_kernel(Slot* table, const u64x2* __restrict__ recs, u64 n, u32 shift,
                                                         u64 tmask, DevCtl* ctl) {
    __shared__ u32 s_ins;
    if (threadIdx.x == 0) s_ins = 0;
    __syncthreads();
    u32 inserted = 0;
    for (u64 i = blockIdx.x * (u64)TPB + threadIdx.x; i < n; i += (u64)gridDim.x * TPB) {
        const u64x2 r = recs[i];
        if (r.x == EMPTY_KEY) {
            inserted += atomicExch(&ctl->sp_claim, 1u) == 0;
            ctl->sp.val = r.y;
            ctl->sp.st[0] = ctl->sp.st[1] = STAMP_PRESENT;
            continue;
        }
        bool fresh;
        const long long s = claim_slot(table, r.x, table_home(r.x, shift), tmask, &fresh);
        if (s < 0) {
            atomicOr(&ctl->err, ERR_TABLE_FULL);
            continue;
        }
        table[s].val = r.y;
        table[s].st[0] = table[s].st[1] = STAMP_PRESENT;
        inserted += fresh;
    }
    if (inserted) atomicAdd(&s_ins, inserted);
    __syncthreads();
    if (threadIdx.x == 0 && s_ins) atomicAdd((unsigned long long*)&ctl->nkeys, (unsigned long long)s_ins);
}

struct SegArgs {
    u64 start[64];  // exclusive prefix of lens (in records)
    u64 total;
    u32 nseg;
    u32 words;  // record size in u64 words
};

__global__ __launch_bounds__(TPB) void copy_segments_kernel(const u64* __restrict__ base, u64 seg_stride_words,
                                                            SegArgs a, u64* ring, u64 ring_mask, u64 dst_lo) {
    for (u64 r = blockIdx.x * (u64)TPB + threadIdx.x; r < a.total; r += (u64)gridDim.x * TPB) {
        u32 s = 0;
        while (s + 1 < a.nseg && a.start[s + 1] <= r) s++;
        const u64 j = r - a.start[s];
        const u64* srcp = base + s * seg_stride_words + j * a.words;
        u64* dst = ring + ((dst_lo + r) & ring_mask) * a.words;
        for (u32 q = 0; q < a.words; q++) dst[q] = srcp[q];
    }
}

static inline unsigned grid_for(u64 n, u64 cap = 4096) {
    u64 g = (n + TPB - 1) / TPB;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

// ---- host side ----------------------------------------------------------------------------
static RecSrc ring_src(nrg_ctx* c, const nrg_put* src, u64 lo) {
    RecSrc r;
    r.src = src;
    r.ring = (const nrg_put*)c->d_ring;
    r.mask = c->log_size - 1;
    r.lo = lo;
    return r;
}

// Stamp rounds: Puts per index thread by round size (one Get per read thread). K1 1 / 2 / 4 in us
// per round (profiles/r03_stamp_k1.txt): 50k Puts + 950k Gets 31.4 / 32.0, B1 (100k + 900k)
// 33.7 / 34.2 / 38.7, 200k + 800k 39.0 / 39.5, 200k + 900k 41.5 / 41.9, 400k + 900k 63.2 / 59.0,
// 500k + 500k 62.5 / 58.3 / 63.8, 800k + 900k (the N = 8 per-GPU round) - / 106.6 / 98.9; at
// 4 there the read blocks behind the index blocks start earlier, but without that many Gets 4
// loses (1M Puts, 2M Puts). NRG_KNOB_K1 overrides.
static u32 stamp_k1_for(const nrg_ctx* c, u64 n, u64 R) {
    if (c->hm.k1_items) return c->hm.k1_items >= 4 ? 4u : c->hm.k1_items >= 2 ? 2u : 1u;
    if (n <= (1u << 18)) return 1u;
    return n >= 655360 && R >= n ? 4u : 2u;
}

// The jobs of one hm_round_kernel launch.
struct Launch {
    IndexJob ij{};
    StampJob sj{};
    ApplyJob aj{};
    ReadJob rj{};
    int ix = IX_PART_NODUP;
    u32 K1 = 1;
    u32 nb = 0;
};

// The deferred half of the last round rides in this launch: its apply (stamp rounds) and reads.
static void attach_deferred(nrg_ctx* c, Launch& L) {
    const HmDeferred& p = c->hm.pend;
    L.rj.epoch = c->hm.epoch;  // reads without a deferred round: every round applied
    if (p.valid) {
        const RecSrc rs = ring_src(c, p.src, p.lo);
        L.rj.keys = p.keys;
        L.rj.R = p.R;
        L.rj.vals = p.vals;
        L.rj.found = p.found;
        L.rj.epoch = p.epoch;
        L.rj.use_rec = p.apply;
        L.rj.rec = rs;
        if (p.apply) {
            L.aj.rec = rs;
            L.aj.n = p.n;
            L.aj.put_slot = c->hm.d_put_slot[p.epoch & 1];
            L.aj.win = L.aj.put_slot + c->hm.stamp_alloc;
            L.aj.over = L.aj.put_slot + 2 * c->hm.stamp_alloc;
            L.aj.epoch = p.epoch;
            L.aj.nblocks = (u32)((p.n + TPB - 1) / TPB);
        }
    }
    c->hm.pend = HmDeferred{};
}

template <int K1, int IX>
static void launch_round(nrg_ctx* c, const Launch& L, u32 blocks, unsigned lds) {
    NRG_LAUNCH(c, "hm_round", (hm_round_kernel<K1, IX>), blocks, TPB, lds, c->stream, L.ij, L.sj, L.aj, L.rj,
               c->hm.d_table, c->hm.slot_shift, (u64)(c->hm.slots - 1), c->d_ctl);
}

static hipError_t launch(nrg_ctx* c, Launch& L) {
    L.rj.nblocks = (u32)((L.rj.R + TPB * RPT - 1) / (TPB * RPT));
    const u32 nix = L.ix == IX_STAMP ? L.sj.nblocks : L.ij.nblocks;
    L.ij.plain = L.sj.plain = L.rj.plain = L.ix == IX_STAMP && nix;  // stamp rounds keep plain stores (st_out)
    // reads beside a bucket or partition pass (which only read the table, or not even that), or
    // alone, with no stamp round's apply riding along: the table is quiescent
    // (removal enabled: a removed key's slot still holds the key, with zeroed stamps, so every read
    // there consults the stamp -- read_role's resolve() answers absent for stamp 0)
    L.rj.quiet = (L.ix != IX_STAMP || nix == 0) && L.aj.nblocks == 0 && !c->hm.removal;
    u32 blocks = nix + L.aj.nblocks + L.rj.nblocks;
    if (blocks == 0) return hipSuccess;
    // a pending skew sample rides in the launch's last block. (The combiner's error copy,
    // c->hm.err_out, is taken only by hm_small_round_kernel, whose last write it is: a multi-block
    // launch's tail block may run before its other blocks' responses land, nrg_combiner retire().)
    if (c->hm.sample_seq) {
        L.rj.s_acc = c->hm.d_dup + ((c->hm.dup_seq - 1) & 1) * HM_DUP_SLOTS;  // the window just ended
        L.rj.s_host = c->hm.h_dup_dev;
        L.rj.s_seq = c->hm.sample_seq;
        c->hm.sample_seq = 0;
        blocks++;
    }
    unsigned lds = 0;
    if (nix && L.ix == IX_STAMP) {
        lds = L.K1 == 4 ? StampLds<4>::BYTES : L.K1 == 2 ? StampLds<2>::BYTES : StampLds<1>::BYTES;
    } else if (nix) {
        const bool dedup = L.ix == IX_PART;
        lds = L.K1 == 8   ? PartLds<8>::bytes(dedup, L.nb)
              : L.K1 == 4 ? PartLds<4>::bytes(dedup, L.nb)
              : L.K1 == 2 ? PartLds<2>::bytes(dedup, L.nb)
                          : PartLds<1>::bytes(dedup, L.nb);
    }
    if (!nix) launch_round<1, IX_PART_NODUP>(c, L, blocks, 0);
#define NRG_RK(KK, XX) else if (L.K1 == KK && L.ix == XX) launch_round<KK, XX>(c, L, blocks, lds)
    NRG_RK(1, IX_STAMP); NRG_RK(2, IX_STAMP); NRG_RK(4, IX_STAMP);
    NRG_RK(1, IX_PART); NRG_RK(1, IX_PART_ALL); NRG_RK(1, IX_PART_NODUP);
    NRG_RK(2, IX_PART); NRG_RK(2, IX_PART_ALL); NRG_RK(2, IX_PART_NODUP);
    NRG_RK(4, IX_PART); NRG_RK(4, IX_PART_ALL); NRG_RK(4, IX_PART_NODUP);
    NRG_RK(8, IX_PART); NRG_RK(8, IX_PART_ALL); NRG_RK(8, IX_PART_NODUP);
#undef NRG_RK
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// The deferred half of the last replayed round (its reads and, for a stamp round, its apply), if any.
static hipError_t hm_flush(nrg_ctx* c) {
    if (!c->hm.pend.valid) return hipSuccess;
    Launch L;
    attach_deferred(c, L);
    return launch(c, L);
}

// Reads against the current state (no writes): attached to the deferred round if it has none.
static hipError_t hm_reads(nrg_ctx* c, const u64* keys, u64 R, u64* vals, uint8_t* found) {
    if (R == 0) return hipSuccess;
    if (c->hm.pend.valid && c->hm.pend.R == 0) {
        c->hm.pend.keys = keys;
        c->hm.pend.R = R;
        c->hm.pend.vals = vals;
        c->hm.pend.found = found;
        return hm_flush(c);
    }
    hipError_t e = hm_flush(c);
    if (e != hipSuccess) return e;
    Launch L;
    attach_deferred(c, L);
    L.rj.keys = keys;
    L.rj.R = R;
    L.rj.vals = vals;
    L.rj.found = found;
    return launch(c, L);
}

// per-round scratch (entries, counts, overlays)
static hipError_t hm_alloc(nrg_ctx* c, u64 mb) {
    const u64 tiles = (mb + TPB - 1) / TPB;  // index tiles of >= TPB Puts
    const u64 ents = tiles * TPB;
    hipError_t e;
    if ((e = hipMalloc(&c->hm.d_bk_ent, ents * 16)) != hipSuccess) return e;
    if ((e = hipMalloc(&c->hm.d_bk_idx, ents * 4)) != hipSuccess) return e;
    if ((e = hipMalloc(&c->hm.d_bk_cnt, (u64)HM_BK_MAX * tiles * sizeof(u32))) != hipSuccess) return e;
    if (c->hm.stamp_max > mb) c->hm.stamp_max = mb;
    // per parity: put_slot, win and over (stamp_max each; epoch tags, zeroed here and whenever
    // the epochs restart, hm_renorm)
    for (int i = 0; i < 2 && c->hm.stamp_max; i++) {
        if ((e = hipMalloc(&c->hm.d_put_slot[i], 3 * c->hm.stamp_max * sizeof(u32))) != hipSuccess) return e;
        if ((e = hipMemsetAsync(c->hm.d_put_slot[i], 0, 3 * c->hm.stamp_max * sizeof(u32), c->stream)) != hipSuccess) return e;
    }
    // two sets of duplicate counters, by sample-window parity: the launch that takes a window's
    // sample reads and clears its set while its own index blocks add to the other
    if ((e = hipMalloc(&c->hm.d_dup, 2 * HM_DUP_SLOTS * sizeof(u64))) != hipSuccess) return e;
    if ((e = hipMemsetAsync(c->hm.d_dup, 0, 2 * HM_DUP_SLOTS * sizeof(u64), c->stream)) != hipSuccess) return e;
    void* h = nullptr;
    if ((e = hipHostMalloc(&h, 2 * sizeof(u64), hipHostMallocMapped)) != hipSuccess) return e;
    c->hm.h_dup = (volatile u64*)h;
    c->hm.h_dup[0] = c->hm.h_dup[1] = 0;
    void* dp = nullptr;
    if ((e = hipHostGetDevicePointer(&dp, h, 0)) != hipSuccess) return e;
    c->hm.h_dup_dev = (u64*)dp;
    return hipSuccess;
}

static void hm_close(nrg_ctx* c) {
    void* ptrs[] = {c->hm.d_table, c->hm.d_created, c->hm.d_bk_ent, c->hm.d_bk_idx, c->hm.d_bk_cnt, c->hm.d_put_slot[0],
                    c->hm.d_put_slot[1], c->hm.d_dup, c->hm.d_dead};
    for (void* p : ptrs) (void)hipFree(p);
    if (c->hm.h_dup) (void)hipHostFree((void*)c->hm.h_dup);
    pt_close(c);  // the scratch of this replica's key partitioning, if it ever partitioned
}

// Every dup_every rounds: read the previous sample (if it has landed) and decide whether the
// stream is skewed, then sample the rounds since. Skewed: more than 1/64 of the Puts were
// combined inside their index block or tile (Zipf 0.99 is far above, uniform keys far below).
// Stamp rounds then cost one same-address atomic per block for each hot key, and partition
// rounds (no atomics per Put) are faster at every size (Zipf 0.99 at 10 % / 50 % writes: 31.9 /
// 55.3 us, profiles/r04_part_sweep.txt); uniform streams below PART_MIN take stamp rounds.
static hipError_t skew_sample(nrg_ctx* c) {
    if (c->hm.dup_seq && c->hm.h_dup[0] == c->hm.dup_seq && c->hm.dup_puts_sampled)
        c->hm.skewed = c->hm.h_dup[1] * 64 > c->hm.dup_puts_sampled;
    c->hm.sample_seq = ++c->hm.dup_seq;  // taken by the next hm_round launch (its last block)
    c->hm.dup_puts_sampled = c->hm.dup_puts;
    c->hm.dup_puts = 0;
    c->hm.dup_rounds = 0;
    return hipSuccess;
}

static int hm_open(nrg_ctx* c) {
    const nrg_config& cf = c->cfg;
    // slot ids are < 2^30 (entry ids carry two flag values above them); replay chunks are
    // bounded by the partition rounds' 16-bit tile offsets (HM_MAX_BATCH)
    if (cf.log2_slots < 4 || cf.log2_slots > 30 || cf.max_batch > HM_MAX_BATCH) return NRG_E_INVAL;
    c->hm.grow_max_log2 = cf.hashmap_max_log2_slots;  // (checked by nrg_open; 0: a fixed table)
    c->hm.slots = 1ull << cf.log2_slots;
    c->hm.slot_shift = 64 - cf.log2_slots;
    HIPCHK(hipMalloc(&c->hm.d_table, c->hm.slots * sizeof(Slot)));
    hm_init_table_kernel<<<grid_for(c->hm.slots, 16384), TPB, 0, c->stream>>>(c->hm.d_table, c->hm.slots);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMalloc(&c->hm.d_created, HM_CREATED_SLOTS * sizeof(u64)));
    HIPCHK(hipMemsetAsync(c->hm.d_created, 0, HM_CREATED_SLOTS * sizeof(u64), c->stream));
    // rounds without previous values replay in one launch (stamp rounds) unless the key
    // stream is skewed (skew_sample) or the round is large (PART_MIN); skewed, large and
    // previous-value rounds take partition rounds
    c->hm.stamp_max = HM_MAX_BATCH;       // (NRG_KNOB_STAMP_MAX lowers it for tests)
    HIPCHK(hm_alloc(c, cf.max_batch));  // clamps stamp_max to max_batch (the put_slot arrays' size)
    c->hm.stamp_alloc = c->hm.stamp_max;
    c->pipeline = cf.pipeline != 0;
    return NRG_OK;
}

// ---- table growth ---------------------------------------------------------------------------------
// HashMap<u64, u64> grows as it fills (nr/examples/hashmap.rs starts from an empty map;
// benches/hashmap.rs:91-100 only pre-sizes it). Here: a synchronous rehash into a larger table,
// rare, decided on the host from an upper bound of the key count (hm_room).
static u32 hm_slots_for(u64 keys) {
    u32 l = 4;  // the smallest table nrg_open accepts
    while (l < 63 && (1ull << l) / HM_GROW_SLOTS_PER_KEY < keys) l++;
    return l;
}

// Steps, in stream order: the deferred half of the last round runs against the old table (after
// it no claim is in flight: what hm_renorm_kernel relies on too); the new table is initialised;
// the rehash; the epochs restart as in next_epoch's renormalisation (every stamp is "present",
// the put_slot / win / over tags hold slot ids and epochs of the old table); the key count is
// folded into DevCtl::nkeys (exact) and the created-key counters cleared. Then the stream is
// synchronised, the old table freed and the new one installed. If the allocation fails nothing
// has been launched but the flush: the old table stays installed and the replica is as it was.
// With removal enabled the rehash drops the dead slots, and new_log2 may be the current size: a purge.
static hipError_t hm_grow(nrg_ctx* c, u32 new_log2) {
    const bool rm = c->hm.removal;
    if (new_log2 > 30 || (1ull << new_log2) < c->hm.slots || (!rm && (1ull << new_log2) == c->hm.slots))
        return hipErrorInvalidValue;
    hipError_t e = hm_flush(c);
    if (e != hipSuccess) return e;
    const u64 nslots = 1ull << new_log2;
    Slot* nt = nullptr;
    if ((e = hipMalloc(&nt, nslots * sizeof(Slot))) != hipSuccess) {
        (void)hipGetLastError();  // (the failure is reported by the return value alone)
        return hipErrorOutOfMemory;
    }
    // (plain stores: streamed, the init measured 2.6x slower)
    NRG_LAUNCH(c, "hm_grow_init", hm_init_table_kernel, grid_for(nslots, 16384), TPB, 0, c->stream, nt, nslots);
    if ((e = hipGetLastError()) == hipSuccess) e = hipMemsetAsync(&c->d_ctl->nkeys, 0, sizeof(u64), c->stream);
    if (e == hipSuccess) {
        const unsigned grid = (unsigned)((c->hm.slots + RH_RUN - 1) / RH_RUN);
        NRG_LAUNCH(c, "hm_rehash", hm_rehash_kernel, grid, RH_TPB, 0, c->stream, c->hm.d_table, c->hm.slots, nt,
                   64 - new_log2, nslots - 1, c->d_ctl, rm, c->hm.tombstone);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemsetAsync(c->hm.d_created, 0, HM_CREATED_SLOTS * sizeof(u64), c->stream);
    if (e == hipSuccess && rm) e = hipMemsetAsync(c->hm.d_dead, 0, HM_CREATED_SLOTS * sizeof(u64), c->stream);
    for (int i = 0; i < 2 && c->hm.d_put_slot[i] && e == hipSuccess; i++)
        e = hipMemsetAsync(c->hm.d_put_slot[i], 0, 3 * c->hm.stamp_alloc * sizeof(u32), c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        // a launch or the stream failed: the old table is still the replica's
        (void)hipFree(nt);
        return e;
    }
    (void)hipFree(c->hm.d_table);
    c->hm.d_table = nt;
    c->hm.slots = nslots;
    c->hm.slot_shift = 64 - new_log2;
    c->hm.epoch = 1;
    return hipSuccess;
}

// The growth policy. With growth enabled a table of S slots is kept to S / HM_GROW_SLOTS_PER_KEY
// keys. The n Puts about to be replayed (or keys about to be prefilled) are added to the upper
// bound keys_ub; only when the bound passes the limit is the exact count taken (hm_count sums 8192
// counters and does not scan the table; an 8-B copy and a stream synchronise), and only if
// exact + n still passes the limit does the table grow, straight to the smallest size that holds
// exact + n keys or to the configured maximum. At the maximum the table is a fixed one: nothing
// is counted, and a table that really fills latches ERR_TABLE_FULL as a fixed table does. The
// decision (exact + n against the size) depends on the log prefix and the configuration alone, so
// the replicas of a group, which replay the same log in the same chunks, grow at the same round.
hipError_t hm_room(nrg_ctx* c, u64 n, bool* due) {
    if (due) *due = false;
    const u32 log2_slots = 64 - c->hm.slot_shift;
    if (!n || c->hm.grow_max_log2 <= log2_slots) return hipSuccess;
    if (n > (1ull << 31)) n = 1ull << 31;  // (more than any table holds; keeps the sums below from wrapping)
    const u64 limit = c->hm.slots / HM_GROW_SLOTS_PER_KEY;
    if (c->hm.keys_ub + n <= limit) {
        c->hm.keys_ub += n;
        return hipSuccess;
    }
    if (due) {
        *due = true;
        return hipSuccess;
    }
    hipError_t e = hm_count(c);  // (flushes the deferred half first)
    if (e != hipSuccess) return e;
    u64 exact = 0;
    if ((e = hipMemcpyAsync(&exact, &c->d_ctl->nkeys_total, sizeof(u64), hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return e;
    if (c->hm.removal) {
        // Removal enabled: keys_ub bounds the OCCUPANCY (live and dead slots: what the load limit and
        // a full table see), and a record still claims at most one slot. Over the limit, the target is
        // the size that holds the live keys and the n records, never a smaller table: a larger one is
        // a grow, the same one with dead slots a purge (a rehash into a table of the same size);
        // either leaves no dead slot behind. The decision depends on the log prefix and the
        // configuration alone, as above.
        u64 occ = 0;
        if ((e = hipMemcpyAsync(&occ, &c->d_ctl->occ_total, sizeof(u64), hipMemcpyDeviceToHost, c->stream)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return e;
        if (occ + n > limit) {
            u32 want = hm_slots_for(exact + n);
            if (want > c->hm.grow_max_log2) want = c->hm.grow_max_log2;
            if (want < log2_slots) want = log2_slots;
            if (want > log2_slots || occ > exact) {
                if ((e = hm_grow(c, want)) != hipSuccess) return e;
                occ = exact;
            }
        }
        c->hm.keys_ub = occ + n;
        return hipSuccess;
    }
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return e;
    if (exact + n > limit) {
        u32 want = hm_slots_for(exact + n);
        if (want > c->hm.grow_max_log2) want = c->hm.grow_max_log2;
        if ((e = hm_grow(c, want)) != hipSuccess) return e;
    }
    c->hm.keys_ub = exact + n;
    return hipSuccess;
}

// The next round's epoch; before the 32-bit epoch wraps, every stamp is renormalised to epoch 1.
static hipError_t next_epoch(nrg_ctx* c, u32* e) {
    if (c->hm.epoch >= c->hm.epoch_limit) {
        hipError_t r = hm_flush(c);
        if (r != hipSuccess) return r;
        hm_renorm_kernel<<<grid_for(c->hm.slots, 16384), TPB, 0, c->stream>>>(c->hm.d_table, c->hm.slots, c->d_ctl,
                                                                              c->hm.removal, c->hm.tombstone);
        if ((r = hipGetLastError()) != hipSuccess) return r;
        for (int i = 0; i < 2 && c->hm.d_put_slot[i]; i++)  // win / over epoch tags of the old epochs
            if ((r = hipMemsetAsync(c->hm.d_put_slot[i], 0, 3 * c->hm.stamp_alloc * sizeof(u32), c->stream)) != hipSuccess)
                return r;
        c->hm.epoch = 1;
    }
    *e = ++c->hm.epoch;
    return hipSuccess;
}

// Replay the records [lo, lo+n) (from `src_recs` if given, else from the ring; writing the
// ring copy if write_ring) and answer R reads against the state after them.
hipError_t hm_replay_chunk(nrg_ctx* c, const void* src_recs, u64 lo, u64 n, bool write_ring, const u64* d_get_keys,
                           u64 R, u64* d_get_vals, uint8_t* d_get_found, u64 resp_lo, u64 resp_hi, u64* d_prev,
                           uint8_t* d_prev_found) {
    // (an empty round still completes the last round's deferred half: "the next call" does)
    if (n == 0) return R ? hm_reads(c, d_get_keys, R, d_get_vals, d_get_found) : hm_flush(c);
    if (n > HM_MAX_BATCH) return hipErrorInvalidValue;
    const nrg_put* src = (const nrg_put*)src_recs;
    // Removal enabled: ONE schedule. Every write round is a previous-value partition round (IX_PART_ALL,
    // then the apply kernel's removal arm), with or without responses (then the window is empty):
    // no small round, no stamp round, no dedup, whatever the knobs say.
    const bool rm = c->hm.removal;
    const bool have_resp = d_prev && resp_lo < lo + n && resp_hi > lo;
    const bool want_prev = have_resp || rm;
    if (!have_resp) resp_lo = resp_hi = 0;
    hipError_t eg = hm_room(c, n);  // every round kind below: the table grows first if it has to
    if (eg != hipSuccess) return eg;
    if (!rm && c->hm.small_max && n <= c->hm.small_max && n <= SM_W && R <= SM_R) {  // one launch, nothing deferred
        hipError_t e = small_round(c, src, lo, n, write_ring, d_get_keys, R, d_get_vals, d_get_found, resp_lo, resp_hi,
                                   want_prev ? d_prev : nullptr, d_prev_found);
        c->rounds++;
        return e;
    }
    // records the deferred half reads: the caller's buffer only when no ring copy is written
    const nrg_put* keep = (src && !write_ring) ? src : nullptr;
    hipError_t e;
    u32 epoch;
    if ((e = next_epoch(c, &epoch)) != hipSuccess) return e;
    Launch L;
    bool measured = false;  // the round's index role counts the Puts its per-tile dedup drops (key skew)
    // Round kinds (NRG_KNOB_PART 1, the default): stamp rounds (one launch, one stamp atomic per
    // distinct key per block) for unskewed rounds without previous values of fewer than
    // PART_MIN Puts; partition rounds (two launches, no device atomic per Put) for the rest.
    // Measured per round (profiles/r04_part_sweep.txt): B1 100k Puts + 900k Gets 34.8 stamp vs
    // 38.1 partition us, 200k + 900k 41.9 / 44.2, 400k + 900k 59.7 / 57.7, 800k + 900k 99.0 / 84.8,
    // 4M + 500k 413 / 271; previous values and skewed streams: partition rounds everywhere.
    constexpr u64 PART_MIN = 3ull << 17;
    const bool stamp0 = !want_prev && c->hm.stamp_max && n <= c->hm.stamp_max && !c->hm.skewed;
    const bool part = !stamp0 || c->hm.part_mode >= 2 || (c->hm.part_mode == 1 && n >= PART_MIN);
    const bool stamp = stamp0 && !part;
    if (part) {
        // ---- partition round: {partition(e) | apply(e-1) | reads(e-1)}, then hm_papply_kernel(e) ----
        // Tiles of 256..2048 Puts, buckets of >= 64 Puts up to 1024 (one apply workgroup each): the
        // [tile][bucket] count words stay <= n / 2
        const u32 K1 = n <= (1u << 14) ? 1u : n <= (1u << 16) ? 2u : n <= (1u << 18) ? 4u : 8u;
        const u32 tile = TPB * K1;
        const u32 log2_slots = 64 - c->hm.slot_shift;
        u32 nb_log = 0;
        while ((64ull << nb_log) < n && (1u << nb_log) < HM_BK_MAX) nb_log++;
        // apply workgroup width (NRG_KNOB_PA_TPB; 0: 512 threads over <= 512 buckets for rounds of
        // >= PA_WIDE_MIN Puts without previous values, else 256 over <= 1024). Round 6, 512 vs 1024
        // (profiles/r06/papply_width.txt): N = 8 per-GPU round 77.2 vs 78.9 us, N = 4 53.9-54.2 vs 54.9,
        // configs[2] 251.1-251.6 vs 255.0, 100 % writes 71.4 vs 72.9, 50 % 54.0 vs 55.1, Zipf 10 % 30.4
        // vs 30.8, Zipf 50 % 47.5 vs 47.9 (scrambled: equal)
        constexpr u64 PA_WIDE_MIN = 1ull << 16;
        const u32 pa_t = want_prev ? 256u : c->hm.pa_tpb ? c->hm.pa_tpb : n >= PA_WIDE_MIN ? 512u : 256u;
        const u32 pa_nb_log = pa_t == 1024 ? PaGeo<false, 1024>::NB_LOG : pa_t == 512 ? PaGeo<false, 512>::NB_LOG
                                                                                      : PaGeo<false, 256>::NB_LOG;
        if (nb_log > pa_nb_log) nb_log = pa_nb_log;
        if (nb_log > log2_slots) nb_log = log2_slots;
        // previous values keep every Put; otherwise a Put overwritten later in its tile is dropped
        // when the key stream is skewed (uniform streams have next to no such Puts: no LDS hash)
        // (the last round of every skew-sample window deduplicates too: it measures the skew)
        L.ix = want_prev ? IX_PART_ALL : (c->hm.skewed || c->hm.dup_rounds + 1 >= c->hm.dup_every) ? IX_PART : IX_PART_NODUP;
        measured = L.ix == IX_PART;
        L.K1 = K1;
        L.nb = 1u << nb_log;
        IndexJob& ij = L.ij;
        ij.rec = ring_src(c, src, lo);
        ij.ring_out = write_ring ? (nrg_put*)c->d_ring : nullptr;
        ij.n = n;
        ij.nblocks = (u32)((n + tile - 1) / tile);
        ij.nb_log = nb_log;
        ij.bk_shift = log2_slots - nb_log;
        ij.ent = (u64x2*)c->hm.d_bk_ent;
        ij.eidx = want_prev ? c->hm.d_bk_idx : nullptr;
        ij.cnt = c->hm.d_bk_cnt;
        ij.dup_acc = c->hm.d_dup + (c->hm.dup_seq & 1) * HM_DUP_SLOTS;
        attach_deferred(c, L);  // the previous round's apply and reads ride along (partition only reads)
        if ((e = launch(c, L)) != hipSuccess) return e;
        PApplyJob aj{};
        aj.ent = ij.ent;
        aj.eidx = ij.eidx;
        aj.cnt = ij.cnt;
        aj.ntiles = ij.nblocks;
        aj.tile = tile;
        aj.nb = 1u << nb_log;
        aj.table = c->hm.d_table;
        aj.shift = c->hm.slot_shift;
        aj.tmask = c->hm.slots - 1;
        aj.ctl = c->d_ctl;
        aj.created_acc = c->hm.d_created;
        aj.lo = lo;
        aj.resp_lo = resp_lo;
        aj.resp_hi = resp_hi;
        aj.prev = d_prev;
        aj.prevf = d_prev_found;
        aj.stall = c->stall;
        aj.dbg = (c->exp & 2) ? c->d_dbg : nullptr;
        aj.tomb = c->hm.tombstone;
        aj.dead_acc = c->hm.d_dead;
        const unsigned dyn = ((ij.nblocks + 1) * 4 + ij.nblocks * 2 + 3) & ~3u;
        if (rm) NRG_LAUNCH(c, "hm_papply", (hm_papply_kernel<true, 256, false, true>), 1u << nb_log, 256, dyn, c->stream, aj);
        else if (want_prev) NRG_LAUNCH(c, "hm_papply", (hm_papply_kernel<true, 256>), 1u << nb_log, 256, dyn, c->stream, aj);
        else if (pa_t == 1024) NRG_LAUNCH(c, "hm_papply", (hm_papply_kernel<false, 1024>), 1u << nb_log, 1024, dyn, c->stream, aj);
        else if (pa_t == 512 && n <= PA_NT_MAX)
            NRG_LAUNCH(c, "hm_papply", (hm_papply_kernel<false, 512, true>), 1u << nb_log, 512, dyn, c->stream, aj);
        else if (pa_t == 512) NRG_LAUNCH(c, "hm_papply", (hm_papply_kernel<false, 512>), 1u << nb_log, 512, dyn, c->stream, aj);
        else NRG_LAUNCH(c, "hm_papply", (hm_papply_kernel<false, 256>), 1u << nb_log, 256, dyn, c->stream, aj);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    } else if (stamp) {
        // ---- stamp round: one launch {index(e) | apply(e-1) | reads(e-1)} ----
        const u32 K1 = stamp_k1_for(c, n, R);
        const u32 tile = TPB * K1;
        L.ix = IX_STAMP;
        L.K1 = K1;
        measured = true;
        L.sj.rec = ring_src(c, src, lo);
        L.sj.ring_out = write_ring ? (nrg_put*)c->d_ring : nullptr;
        L.sj.n = n;
        L.sj.nblocks = (u32)((n + tile - 1) / tile);
        L.sj.epoch = epoch;
        L.sj.put_slot = c->hm.d_put_slot[epoch & 1];
        L.sj.win = L.sj.put_slot + c->hm.stamp_alloc;
        L.sj.over = L.sj.put_slot + 2 * c->hm.stamp_alloc;
        L.sj.created_acc = c->hm.d_created;
        L.sj.dup_acc = c->hm.d_dup + (c->hm.dup_seq & 1) * HM_DUP_SLOTS;
        attach_deferred(c, L);
        if ((e = launch(c, L)) != hipSuccess) return e;
    }
    c->rounds++;
    if (measured) c->hm.dup_puts += n;  // the skew ratio is over the rounds that measured it
    if (++c->hm.dup_rounds >= c->hm.dup_every && (e = skew_sample(c)) != hipSuccess) return e;
    HmDeferred& p = c->hm.pend;
    p.valid = true;
    p.epoch = epoch;
    p.apply = stamp;
    p.src = keep;
    p.lo = lo;
    p.n = n;
    p.keys = d_get_keys;
    p.R = R;
    p.vals = d_get_vals;
    p.found = d_get_found;
    if (!c->pipeline || (stamp && keep)) return hm_flush(c);
    return hipSuccess;
}

static hipError_t hm_get_only(nrg_ctx* c, const u64* d_keys, u64 n, u64* d_vals, uint8_t* d_found) {
    return hm_reads(c, d_keys, n, d_vals, d_found);
}

// a chunk without reads; responses are the Puts' previous values
static hipError_t hm_replay(nrg_ctx* c, const void* src, u64 lo, u64 n, u64 resp_lo, u64 resp_hi, void* d_resp,
                            uint8_t* d_some) {
    return hm_replay_chunk(c, src, lo, n, src != nullptr, nullptr, 0, nullptr, nullptr, resp_lo, resp_hi,
                           (u64*)d_resp, d_some);
}

// A deferred stamp round's apply and reads take values from the ring: the log is held back to its
// first record.
static u64 hm_floor(const nrg_ctx* c) {
    const HmDeferred& p = c->hm.pend;
    if (p.valid && p.apply && !p.src && p.lo < c->ltail) return p.lo;
    return c->ltail;
}

static int hm_set_knob(nrg_ctx* c, int knob, uint64_t v) {
    switch (knob) {
        case NRG_KNOB_STAMP_MAX:
            c->hm.stamp_max = std::min<uint64_t>(v, c->hm.stamp_alloc);
            return NRG_OK;
        case NRG_KNOB_SKEW_EVERY:
            if (v < 1 || v > (1u << 30)) return NRG_E_INVAL;
            c->hm.dup_every = (uint32_t)v;
            return NRG_OK;
        case NRG_KNOB_EPOCH_LIMIT:
            if (v < 2 || v > 0xFFFFFFF0ull) return NRG_E_INVAL;
            c->hm.epoch_limit = (uint32_t)v;
            return NRG_OK;
        case NRG_KNOB_K1:
            if (v > 4) return NRG_E_INVAL;
            c->hm.k1_items = (uint32_t)v;
            return NRG_OK;
        case NRG_KNOB_PART:
            if (v > 2) return NRG_E_INVAL;  // 0: partition rounds only where stamp rounds cannot
            c->hm.part_mode = (uint32_t)v;
            return NRG_OK;
        case NRG_KNOB_PA_TPB:
            if (v != 0 && v != 256 && v != 512 && v != 1024) return NRG_E_INVAL;
            c->hm.pa_tpb = (uint32_t)v;
            return NRG_OK;
        case NRG_KNOB_SMALL_MAX:
            if (v > 2048) return NRG_E_INVAL;
            c->hm.small_max = v;
            return NRG_OK;
        default: return NRG_E_INVAL;
    }
}

// NRG_KNOB_EXP bit 2: 8 words per partition-round apply bucket
static u64 hm_dbg_words(const nrg_ctx*) { return (u64)HM_BK_MAX * 8; }

static hipError_t hm_digest(nrg_ctx* c, u64* d_out3);
static int hm_items(nrg_ctx* c, u64* n);
static hipError_t hm_snapshot(nrg_ctx* c, void* d_buf, u64 cap, u64 log_idx);
static int hm_restore(nrg_ctx* c, const void* d_payload, u64 items, bool check_only);

// *hits = how many of n {key, value} pairs, `stride` words apart, hold the tombstone as their value
// (table: the slots of the table and the side slot; empty slots are no pairs). Synchronous.
static int hm_find_val(nrg_ctx* c, const u64* pairs, u64 n, u32 stride, bool table, u64* hits) {
    HIPCHK(hipMemsetAsync(&c->d_ctl->counter, 0, sizeof(u64), c->stream));
    NRG_LAUNCH(c, "hm_find_val", hm_find_val_kernel, grid_for(n, 8192), TPB, 0, c->stream, pairs, n, stride, table,
               c->hm.tombstone, c->d_ctl);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hits, &c->d_ctl->counter, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return NRG_OK;
}

bool hm_removal(const nrg_ctx* c) { return c->cfg.ds_kind == NRG_DS_HASHMAP && c->hm.removal; }

const DsOps* hm_ops() {
    static const DsOps ops = {sizeof(nrg_put), sizeof(u64), hm_open, hm_close, hm_flush, hm_replay,
                              hm_floor, hm_set_knob, hm_dbg_words, nullptr, hm_digest,
                              hm_items, hm_snapshot, hm_restore};
    return &ops;
}

hipError_t hm_prefill_range(nrg_ctx* c, u64 n, u64 off, u32 part, u32 parts) {
    hipError_t e = hm_flush(c);
    if (e != hipSuccess) return e;
    // room for the keys first (growth enabled): all n, or a key partition's exact share of them
    u64 mine = n;
    if (parts > 1 && c->hm.grow_max_log2 > 64 - c->hm.slot_shift) {
        mine = 0;
        for (u64 k = 0; k < n; k++) mine += key_owner(k, parts) == part;
    }
    if ((e = hm_room(c, mine)) != hipSuccess) return e;
    hm_prefill_range_kernel<<<grid_for(n, 8192), TPB, 0, c->stream>>>(c->hm.d_table, n, off, c->hm.slot_shift,
                                                                      c->hm.slots - 1, c->d_ctl, part, parts,
                                                                      c->hm.tombstone, c->hm.removal ? c->hm.d_dead : nullptr);
    return hipGetLastError();
}

static hipError_t hm_count(nrg_ctx* c) {
    hipError_t e = hm_flush(c);
    if (e != hipSuccess) return e;
    hm_count_kernel<<<1, TPB, 0, c->stream>>>(c->hm.d_created, HM_CREATED_SLOTS, c->d_ctl,
                                              c->hm.removal ? c->hm.d_dead : nullptr);
    return hipGetLastError();
}

static hipError_t hm_dump(nrg_ctx* c, u64* d_keys, u64* d_vals) {
    hipError_t e = hm_flush(c);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(&c->d_ctl->counter, 0, sizeof(u64), c->stream);
    if (e != hipSuccess) return e;
    NRG_LAUNCH(c, "hm_dump", hm_dump_kernel, grid_for(c->hm.slots, 8192), TPB, 0, c->stream, (const Slot*)c->hm.d_table,
               (u64)c->hm.slots, c->d_ctl, d_keys, d_vals, c->hm.removal, c->hm.tombstone);
    return hipGetLastError();
}

static hipError_t hm_digest(nrg_ctx* c, u64* d_out3) {
    hipError_t e = hm_flush(c);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(d_out3, 0, 3 * sizeof(u64), c->stream);
    if (e != hipSuccess) return e;
    NRG_LAUNCH(c, "hm_digest", hm_digest_kernel, grid_for(c->hm.slots, 8192), TPB, 0, c->stream,
               (const Slot*)c->hm.d_table, (u64)c->hm.slots, (const DevCtl*)c->d_ctl, d_out3, c->hm.removal,
               c->hm.tombstone);
    return hipGetLastError();
}

// the exact key count, as nrg_hashmap_size takes it
static int hm_items(nrg_ctx* c, u64* n) {
    HIPCHK(hm_count(c));
    HIPCHK(hipMemcpyAsync(n, &c->d_ctl->nkeys_total, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return NRG_OK;
}

// The scan (one atomic per tile on DevCtl::counter), then the side key and the header. The grid
// covers the tiles up to 8192 workgroups: 2^26 slots are 16384 tiles, two per workgroup.
static hipError_t hm_snapshot(nrg_ctx* c, void* d_buf, u64 cap, u64 log_idx) {
    hipError_t e = hm_flush(c);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(&c->d_ctl->counter, 0, sizeof(u64), c->stream)) != hipSuccess) return e;
    const u64 cap_items = cap >= SNAP_HDR ? (cap - SNAP_HDR) / 16 : 0;
    const u64 tiles = (c->hm.slots + SN_TILE - 1) / SN_TILE;
    NRG_LAUNCH(c, "hm_snapshot", hm_snapshot_kernel, (unsigned)(tiles < 8192 ? tiles : 8192), TPB, 0, c->stream,
               (const Slot*)c->hm.d_table, (u64)c->hm.slots, c->d_ctl, (u64x2*)((char*)d_buf + SNAP_HDR), cap_items,
               c->hm.removal, c->hm.tombstone);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hm_snapshot_head_kernel<<<1, 64, 0, c->stream>>>(c->d_ctl, (u64*)d_buf, cap, log_idx, c->hm.removal,
                                                     c->hm.tombstone);
    return hipGetLastError();
}

// A restored map is one that holds the pairs since before any replay round: the table sized as
// hm_room would have sized it for `items` keys (growth on) and initialised as hm_grow initialises a
// new one, every key claimed and stamped "present", the count exact in DevCtl::nkeys, the created-key
// counters, the epochs and their tags, the key bound and the skew sampler as after nrg_open.
static int hm_restore(nrg_ctx* c, const void* d_payload, u64 items, bool check_only) {
    const u32 cur = 64 - c->hm.slot_shift;
    const bool grows = c->hm.grow_max_log2 > cur;
    if (check_only) {
        const u64 limit = grows ? (1ull << c->hm.grow_max_log2) / HM_GROW_SLOTS_PER_KEY : c->hm.slots;
        if (items > limit) return NRG_E_TABLE_FULL;
        // removal enabled: an image that holds the tombstone as a value is not a state of this context
        if (c->hm.removal && d_payload && items) {
            u64 hits = 0;
            int r = hm_find_val(c, (const u64*)d_payload, items, 2, false, &hits);
            if (r) return r;
            if (hits) return NRG_E_INVAL;
        }
        return NRG_OK;
    }
    if (!d_payload) items = 0;
    if (grows) {
        u32 want = hm_slots_for(items);
        if (want > c->hm.grow_max_log2) want = c->hm.grow_max_log2;
        if ((1ull << want) > c->hm.slots) {
            Slot* nt = nullptr;
            if (hipMalloc(&nt, (1ull << want) * sizeof(Slot)) != hipSuccess) {
                (void)hipGetLastError();
                return NRG_E_NOMEM;  // the old table stays installed, its contents as they were
            }
            (void)hipFree(c->hm.d_table);
            c->hm.d_table = nt;
            c->hm.slots = 1ull << want;
            c->hm.slot_shift = 64 - want;
        }
    }
    c->hm.pend.valid = false;
    NRG_LAUNCH(c, "hm_restore_init", hm_init_table_kernel, grid_for(c->hm.slots, 16384), TPB, 0, c->stream,
               c->hm.d_table, c->hm.slots);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(c->d_ctl, 0, sizeof(DevCtl), c->stream));
    HIPCHK(hipMemsetAsync(c->hm.d_created, 0, HM_CREATED_SLOTS * sizeof(u64), c->stream));
    if (c->hm.d_dead) HIPCHK(hipMemsetAsync(c->hm.d_dead, 0, HM_CREATED_SLOTS * sizeof(u64), c->stream));
    for (int i = 0; i < 2 && c->hm.d_put_slot[i]; i++)
        HIPCHK(hipMemsetAsync(c->hm.d_put_slot[i], 0, 3 * c->hm.stamp_alloc * sizeof(u32), c->stream));
    HIPCHK(hipMemsetAsync(c->hm.d_dup, 0, 2 * HM_DUP_SLOTS * sizeof(u64), c->stream));
    c->hm.h_dup[0] = c->hm.h_dup[1] = 0;
    c->hm.dup_seq = c->hm.dup_puts = c->hm.dup_puts_sampled = c->hm.sample_seq = 0;
    c->hm.dup_rounds = 0;
    c->hm.skewed = false;
    c->hm.epoch = 1;
    c->hm.keys_ub = items;
    if (items) {
        NRG_LAUNCH(c, "hm_restore", hm_restore_kernel, grid_for(items, 8192), TPB, 0, c->stream, c->hm.d_table,
                   (const u64x2*)d_payload, items, c->hm.slot_shift, (u64)(c->hm.slots - 1), c->d_ctl);
        HIPCHK(hipGetLastError());
    }
    return NRG_OK;
}

hipError_t copy_segments(nrg_ctx* c, const void* d_base, u32 nseg, u64 seg_stride, const u64* lens, u64 dst_lo) {
    SegArgs a;
    if (nseg > 64) return hipErrorInvalidValue;
    a.nseg = nseg;
    a.words = c->rec_bytes / 8;
    u64 acc = 0;
    for (u32 s = 0; s < nseg; s++) {
        a.start[s] = acc;
        acc += lens[s];
    }
    a.total = acc;
    if (acc == 0) return hipSuccess;
    copy_segments_kernel<<<grid_for(acc, 8192), TPB, 0, c->stream>>>(
        (const u64*)d_base, seg_stride * a.words, a, (u64*)c->d_ring, c->log_size - 1, dst_lo);
    return hipGetLastError();
}

// A round as nrg_hashmap_round_async would run it as a small round, its log bookkeeping done and
// nothing launched (the combiner's round server runs it).
int hm_small_job(nrg_ctx* c, const nrg_put* recs, u64 W, u32 origin, const u64* keys, u64 R, u64* vals,
                 uint8_t* found, u64* prev, uint8_t* prevf, u32* e_out, SmallJobBlob* blob, u64* lo_out) {
    if (!c || c->cfg.ds_kind != NRG_DS_HASHMAP || W > c->cfg.max_batch || c->ltail != c->tail) return NRG_E_INVAL;
    if (c->hm.removal) return NRG_E_INVAL;  // (no small round there, and no combiner to ask for one)
    if ((W && !recs) || (R && (!keys || !vals || !found))) return NRG_E_INVAL;
    int r = reserve(c, W);  // (caught up and nothing deferred: only moves head, launches nothing)
    if (r) return r == NRG_E_RING_FULL ? NRG_E_INVAL : r;  // more than the log ever holds: not a small round
    const uint64_t lo = c->tail;
    if (!hm_small_fill(c, recs, lo, W, keys, R, vals, found, prev, prevf, e_out, blob)) return NRG_E_INVAL;
    // the round's Puts against the table's load limit (hm_room): a round before which the keys have
    // to be counted or the table has to grow is not served but launched -- the combiner stops the
    // server before any launch, and the launched round counts and grows in hm_replay_chunk
    bool due = false;
    if (hm_room(c, W, &due) != hipSuccess || due) return NRG_E_INVAL;
    if (lo_out) *lo_out = lo;
    c->rounds++;
    if (W) note_origin(c, lo, W, origin);
    commit_round(c, lo, W);
    return NRG_OK;
}

}  // namespace nrg

// ---- the NrHashMap entry points (include/nrgpu.h, nrgpu_testing.h) ----------------------------
using namespace nrg;

extern "C" {

int nrg_hashmap_get_async(nrg_ctx* c, const uint64_t* d_keys, uint64_t n, uint64_t* d_vals, uint8_t* d_found) {
    int r = need(c, NRG_DS_HASHMAP);
    if (r) return r;
    if (c->ltail != c->tail) return NRG_E_NOT_SYNCED;
    if (n && (!d_keys || !d_vals || !d_found)) return NRG_E_INVAL;
    return hip_fail(hm_get_only(c, d_keys, n, d_vals, d_found));
}

int nrg_hashmap_get(nrg_ctx* c, const uint64_t* keys, uint64_t n, uint64_t* vals, uint8_t* found) {
    int r = need(c, NRG_DS_HASHMAP);
    if (r) return r;
    if (c->ltail != c->tail) return NRG_E_NOT_SYNCED;
    if (n == 0) return NRG_OK;
    Staging* s = c->stg;
    if ((r = staging(s[0], n * 8)) || (r = staging(s[1], n * 8)) || (r = staging(s[2], n))) return r;
    HIPCHK(hipMemcpyAsync(s[0].p, keys, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hm_get_only(c, (u64*)s[0].p, n, (u64*)s[1].p, (uint8_t*)s[2].p));
    HIPCHK(hipMemcpyAsync(vals, s[1].p, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(found, s[2].p, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_all(c));
    return check_err(c);
}

int nrg_hashmap_round_async(nrg_ctx* c, const nrg_put* d_puts, uint64_t W, uint32_t origin,
                            const uint64_t* d_get_keys, uint64_t R, uint64_t* d_get_vals, uint8_t* d_get_found,
                            uint64_t* d_prev, uint8_t* d_prev_found) {
    int r = need(c, NRG_DS_HASHMAP);
    if (r) return r;
    if (W > c->cfg.max_batch) return NRG_E_CAPACITY;
    if ((W && !d_puts) || (R && (!d_get_keys || !d_get_vals || !d_get_found))) return NRG_E_INVAL;
    // catch up on anything appended by others first (Replica::combine execs the whole log)
    if ((r = exec_range(c, 0, 0, nullptr, nullptr))) return r;
    if ((r = reserve(c, W))) return r;
    const uint64_t lo = c->tail;
    if (!d_prev || !d_prev_found) d_prev = nullptr, d_prev_found = nullptr;
    HIPCHK(hm_replay_chunk(c, d_puts, lo, W, true, d_get_keys, R, d_get_vals, d_get_found, lo, lo + W, d_prev,
                           d_prev_found));
    if (W) note_origin(c, lo, W, origin);
    commit_round(c, lo, W);
    return NRG_OK;
}

int nrg_hashmap_round_segments_async(nrg_ctx* c, const nrg_put* d_base, uint32_t nseg, uint64_t seg_stride,
                                     const uint64_t* lens, const uint32_t* origins, uint32_t resp_seg,
                                     const uint64_t* d_get_keys, uint64_t R, uint64_t* d_get_vals,
                                     uint8_t* d_get_found, uint64_t* d_prev, uint8_t* d_prev_found) {
    int r = need(c, NRG_DS_HASHMAP);
    if (r) return r;
    if (!lens || nseg == 0 || nseg > 64 || !d_base) return NRG_E_INVAL;
    if (R && (!d_get_keys || !d_get_vals || !d_get_found)) return NRG_E_INVAL;
    if (!d_prev || !d_prev_found) d_prev = nullptr, d_prev_found = nullptr;
    uint64_t total = 0, own_off = 0;
    bool dense = true;
    for (uint32_t s = 0; s < nseg; s++) {
        if (lens[s] > seg_stride) return NRG_E_INVAL;
        if (s == resp_seg) own_off = total;
        if (s + 1 < nseg && lens[s] != seg_stride) dense = false;
        total += lens[s];
    }
    if ((r = exec_range(c, 0, 0, nullptr, nullptr))) return r;
    if ((r = reserve(c, total))) return r;
    const uint64_t lo = c->tail;
    const uint64_t rlo = resp_seg < nseg ? lo + own_off : 0;
    const uint64_t rhi = resp_seg < nseg ? rlo + lens[resp_seg] : 0;
    if (dense && total <= c->cfg.max_batch) {
        // the gathered segments are already the contiguous round W_0 || W_1 || ...: replay them
        // in place while K1 writes the log copy (no separate append pass)
        HIPCHK(hm_replay_chunk(c, d_base, lo, total, true, d_get_keys, R, d_get_vals, d_get_found, rlo, rhi, d_prev,
                               d_prev_found));
        for (uint32_t s = 0, off = 0; s < nseg; off += (uint32_t)lens[s], s++)
            if (lens[s]) note_origin(c, lo + off, lens[s], origins ? origins[s] : s + 1);
        commit_round(c, lo, total);
        return NRG_OK;
    }
    HIPCHK(copy_segments(c, d_base, nseg, seg_stride, lens, lo));
    for (uint32_t s = 0; s < nseg; s++) {
        if (lens[s]) note_origin(c, c->tail, lens[s], origins ? origins[s] : s + 1);
        c->tail += lens[s];
    }
    // replay them and answer the reads against the final state, fused into the last chunk
    if (c->ltail == c->tail) return hip_fail(hm_get_only(c, d_get_keys, R, d_get_vals, d_get_found));
    const uint64_t last = c->ltail + (c->tail - c->ltail - 1) / c->cfg.max_batch * c->cfg.max_batch;
    if ((r = exec_range(c, rlo, rhi, d_prev, d_prev_found, last))) return r;
    HIPCHK(hm_replay_chunk(c, nullptr, last, c->tail - last, false, d_get_keys, R, d_get_vals, d_get_found, rlo, rhi,
                           d_prev, d_prev_found));
    commit_round(c, last, c->tail - last);
    return NRG_OK;
}

int nrg_hashmap_prefill(nrg_ctx* c, const uint64_t* keys, const uint64_t* vals, uint64_t n) {
    int r = need(c, NRG_DS_HASHMAP);
    if (r) return r;
    if (c->hm.removal)  // a prefilled value is a value: never the tombstone
        for (uint64_t i = 0; i < n; i++)
            if (vals[i] == c->hm.tombstone) return NRG_E_INVAL;
    Staging* s = c->stg;
    uint64_t done = 0;
    const uint64_t chunk = c->cfg.max_batch;
    if ((r = staging(s[0], (n < chunk ? n : chunk) * sizeof(nrg_put)))) return r;
    while (done < n) {
        const uint64_t m = n - done < chunk ? n - done : chunk;
        nrg_put* h = (nrg_put*)std::malloc(m * sizeof(nrg_put));
        if (!h) return NRG_E_NOMEM;
        for (uint64_t i = 0; i < m; i++) h[i] = nrg_put{keys[done + i], vals[done + i]};
        hipError_t e = hipMemcpyAsync(s[0].p, h, m * sizeof(nrg_put), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        std::free(h);
        if (e != hipSuccess) return hip_fail(e);
        // direct insert (no log traffic): replay the records through the round pipeline
        // with a private log position, so duplicate keys keep last-writer-wins order.
        HIPCHK(hm_replay_chunk(c, s[0].p, 0, m, false, nullptr, 0, nullptr, nullptr, 0, 0, nullptr, nullptr));
        done += m;
    }
    HIPCHK(sync_all(c));
    return check_err(c);
}

int nrg_hashmap_prefill_range(nrg_ctx* c, uint64_t n, uint64_t off) {
    int r = need(c, NRG_DS_HASHMAP);
    if (r) return r;
    if (c->hm.removal && c->hm.tombstone - off < n) return NRG_E_INVAL;  // some k + off is the tombstone
    HIPCHK(hm_prefill_range(c, n, off));
    HIPCHK(sync_all(c));
    return check_err(c);
}

// HashMap::reserve / with_capacity (benches/hashmap.rs:91-100 pre-sizes the map; nr/examples/hashmap.rs
// lets it grow): a table that holds n_keys keys in all at the load limit. Never shrinks.
int nrg_hashmap_reserve(nrg_ctx* c, uint64_t n_keys) {
    int r = need(c, NRG_DS_HASHMAP);
    if (r) return r;
    if (n_keys > (1ull << 30) / HM_GROW_SLOTS_PER_KEY) return NRG_E_INVAL;  // beyond nrg_open's largest table
    const uint32_t want = hm_slots_for(n_keys);
    if ((1ull << want) <= c->hm.slots) return NRG_OK;
    HIPCHK(hm_grow(c, want));
    return NRG_OK;
}

// ---- removal (HashMap::remove; include/nrgpu.h, DESIGN.md "NrHashMap", Removal) --------------------
int nrg_hashmap_enable_removal(nrg_ctx* c, uint64_t tombstone) {
    int r = need(c, NRG_DS_HASHMAP);
    if (r) return r;
    if (c->hm.removal) return tombstone == c->hm.tombstone ? NRG_OK : NRG_E_INVAL;
    if (c->comb.open) return NRG_E_INVAL;
    if (c->ltail != c->tail) return NRG_E_NOT_SYNCED;
    HIPCHK(sync_all(c));  // (flushes the deferred half)
    // one scan before anything changes: no present value may be the tombstone
    c->hm.tombstone = tombstone;
    u64 hits = 0;
    r = hm_find_val(c, (const u64*)c->hm.d_table, c->hm.slots, (u32)(sizeof(Slot) / 8), true, &hits);
    if (r == NRG_OK && hits) r = NRG_E_INVAL;
    if (r == NRG_OK && !c->hm.d_dead) {
        hipError_t e = hipMalloc(&c->hm.d_dead, HM_CREATED_SLOTS * sizeof(u64));
        if (e == hipSuccess) e = hipMemsetAsync(c->hm.d_dead, 0, HM_CREATED_SLOTS * sizeof(u64), c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) (void)hipGetLastError();
        r = hip_fail(e);
    }
    if (r != NRG_OK) {
        c->hm.tombstone = 0;
        return r;
    }
    c->hm.removal = true;
    return NRG_OK;
}

int nrg_hashmap_removal(nrg_ctx* c, uint64_t* tombstone, int* enabled) {  // no device is touched
    if (!c || c->cfg.ds_kind != NRG_DS_HASHMAP) return NRG_E_INVAL;
    if (tombstone) *tombstone = c->hm.removal ? c->hm.tombstone : 0;
    if (enabled) *enabled = c->hm.removal ? 1 : 0;
    return NRG_OK;
}

int nrg_hashmap_occupancy(nrg_ctx* c, uint64_t* slots_taken) {
    int r = need(c, NRG_DS_HASHMAP);
    if (r) return r;
    if (!slots_taken) return NRG_E_INVAL;
    HIPCHK(hm_count(c));
    HIPCHK(hipMemcpyAsync(slots_taken, &c->d_ctl->occ_total, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_all(c));
    return check_err(c);
}

int nrg_hashmap_purge(nrg_ctx* c) {
    int r = need(c, NRG_DS_HASHMAP);
    if (r) return r;
    if (!c->hm.removal) return NRG_OK;
    u64 cnt[2] = {0, 0};  // live, taken
    HIPCHK(hm_count(c));
    HIPCHK(hipMemcpyAsync(&cnt[0], &c->d_ctl->nkeys_total, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&cnt[1], &c->d_ctl->occ_total, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (cnt[1] == cnt[0]) return NRG_OK;  // nothing dead
    HIPCHK(hm_grow(c, 64 - c->hm.slot_shift));
    if (c->hm.keys_ub > cnt[0]) c->hm.keys_ub = cnt[0];
    return NRG_OK;
}

int nrg_hashmap_capacity(nrg_ctx* c, uint32_t* log2_slots) {
    if (!c || !log2_slots || c->cfg.ds_kind != NRG_DS_HASHMAP) return NRG_E_INVAL;
    *log2_slots = 64 - c->hm.slot_shift;
    return NRG_OK;
}

int nrg_hashmap_size(nrg_ctx* c, uint64_t* n) {
    int r = need(c, NRG_DS_HASHMAP);
    if (r) return r;
    HIPCHK(hm_count(c));
    HIPCHK(hipMemcpyAsync(n, &c->d_ctl->nkeys_total, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_all(c));
    return check_err(c);
}

int nrg_hashmap_dump(nrg_ctx* c, uint64_t* keys, uint64_t* vals, uint64_t cap, uint64_t* n) {
    int r = nrg_hashmap_size(c, n);
    if (r) return r;
    if (*n > cap) return NRG_E_CAPACITY;
    if (*n == 0) return NRG_OK;
    Staging* s = c->stg;
    if ((r = staging(s[0], *n * 8)) || (r = staging(s[1], *n * 8))) return r;
    HIPCHK(hm_dump(c, (u64*)s[0].p, (u64*)s[1].p));
    HIPCHK(hipMemcpyAsync(keys, s[0].p, *n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(vals, s[1].p, *n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_all(c));
    return check_err(c);
}

int nrg_hashmap_digest(nrg_ctx* c, uint64_t out[3]) {
    int r = need(c, NRG_DS_HASHMAP);
    if (r) return r;
    return nrg_digest(c, out);
}

int nrg_test_hm_skewed(nrg_ctx* c, int* out) {
    if (!c || !out || c->cfg.ds_kind != NRG_DS_HASHMAP) return NRG_E_INVAL;
    *out = c->hm.skewed ? 1 : 0;
    return NRG_OK;
}

}  // extern "C"
