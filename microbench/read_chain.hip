// read_chain.hip — what separates the hashmap read role from the random-line floor.
//
// line_floor.hip serves 900k Get-shaped lookups in 21.3-22.0 us, but over a table where every Get
// ends at its first slot. This file fills the table in the product's hashed layout (keys [0, 2^23)
// -> k + 1 at mix64(key) >> 38, linear probing, as hm_prefill_range_kernel does: load 0.125) and
// times read kernels over it in line_floor's harness (16 rotating key batches, 16 warm-up + 64
// timed launches, keys uniform over 10M):
//   first    one probe only, as line_floor's gets<1, true>: the floor on the real table
//   chain    the read role's per-lane probe loop ({key, val} + stamp per probe, resolve, vals and
//            found stores): a wave stays until its slowest lane's chain ends
//   refillN  a wave owns 64 * N consecutive Gets, keys staged in LDS; a lane whose Get resolved
//            stores its answer and takes the window's next Get (ballot + prefix popcount), so every
//            trip to memory carries a full wave of probes. Slower than chain at N = 2, 4, 8.
//   dyn1..6, round, round_q   the product's read role rebuilt around chain one difference at a
//            time (see read_role below): what the bisect of chain against the product used.
//   groupA, groupB, groupA_q, groupB_q, groupA_s   over a second table filled in the line-grouped
//            probe sequence (common.hpp probe_slot): a quad of lanes loads a Get's whole four-slot
//            group per trip (group_role below). A: a block owns 256 Gets, four passes of 16 per
//            wave, answers shuffled back to one Get per lane; B: one pass, 64 Gets per block;
//            _q: the quiet reads of a reads-only round (against round_q); _s: A with one coalesced
//            key load and the passes' keys by shuffle. The yardsticks above stay on linear probing.
// It also counts how many Gets need a second, third, ... probe (a second group, on the grouped
// table) and how many trips a 64-Get wave makes, and checks chain's answers against a CPU lookup
// and every variant's against chain's. Results: profiles/read_chain.txt, profiles/read_group.txt.
// Usage: read_chain [gets_per_launch]   (default 900000, B1's Gets)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#define CHK(x)                                                                       \
    do {                                                                             \
        hipError_t e_ = (x);                                                         \
        if (e_ != hipSuccess) {                                                      \
            fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

typedef unsigned long long u64;
typedef unsigned int u32;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

struct __attribute__((aligned(32))) Slot {
    u64 key, val, st[2];
};

__device__ __host__ inline u64 mix64(u64 z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

constexpr int TPB = 256;
constexpr int LOG2_SLOTS = 26;
constexpr int SHIFT = 64 - LOG2_SLOTS;
constexpr u64 TMASK = (1ull << LOG2_SLOTS) - 1;
constexpr u64 EMPTY_KEY = ~0ull;
constexpr u64 NKEYS = 1ull << 23;
constexpr u64 STAMP_PRESENT = 1ull << 32;

// the read role's job, as far as the stamp path reads it
struct Job {
    const u64* keys;
    u64 R;
    u64* vals;
    unsigned char* found;
    u32 epoch;
    bool use_rec;
    const u64x2* rec;
};

__device__ __forceinline__ bool resolve(u64 val, u64 st, const Job& j, u64* v) {
    const u32 se = (u32)(st >> 32);
    if (st == 0 || se > j.epoch) return false;
    *v = (se == j.epoch && j.use_rec) ? j.rec[(u32)st - 1].y : val;
    return true;
}

__global__ __launch_bounds__(TPB) void first_kernel(const Slot* __restrict__ t, Job j) {
    const u64 q = (u64)blockIdx.x * TPB + threadIdx.x;
    if (q >= j.R) return;
    const u64 k = j.keys[q];
    const u64 s = mix64(k) >> SHIFT;
    const u64x2 w = *(const u64x2*)&t[s];
    const u64 st = t[s].st[j.epoch & 1];
    const bool f = w.x == k && st != 0;
    j.vals[q] = f ? w.y : 0;
    j.found[q] = f;
}

__global__ __launch_bounds__(TPB) void chain_kernel(const Slot* __restrict__ t, Job j) {
    const u32 par = j.epoch & 1;
    const u64 q = (u64)blockIdx.x * TPB + threadIdx.x;
    if (q >= j.R) return;
    const u64 k = j.keys[q];
    u64 sl = mix64(k) >> SHIFT;
    u64x2 w = *(const u64x2*)&t[sl];
    u64 stt = t[sl].st[par];
    u64 kk = w.x, vv = w.y, v = 0;
    bool f = false;
    // (as the product: without these the compiler sinks the stamp load below the loop, a second
    // dependent trip for every Get: 34.0 us)
    asm volatile("" : "+v"(kk), "+v"(vv), "+v"(stt));
    for (u64 pr = 0; pr <= TMASK; pr++) {
        if (kk == k) {
            f = resolve(vv, stt, j, &v);
            break;
        }
        if (kk == EMPTY_KEY) break;
        sl = (sl + 1) & TMASK;
        const u64x2 x = *(const u64x2*)&t[sl];
        stt = t[sl].st[par];
        kk = x.x;
        vv = x.y;
        asm volatile("" : "+v"(kk), "+v"(vv), "+v"(stt));
    }
    if (!f) v = 0;
    j.vals[q] = v;
    j.found[q] = f ? 1 : 0;
}

// The record index + 1 of a Get whose value is its round's elected record's (0: the slot's value).
__device__ __forceinline__ bool resolve_at(u64 st, const Job& j, u32* ri) {
    const u32 se = (u32)(st >> 32);
    if (st == 0 || se > j.epoch) return false;
    *ri = (se == j.epoch && j.use_rec) ? (u32)st : 0;
    return true;
}

template <int RW>
__global__ __launch_bounds__(TPB) void refill_kernel(const Slot* __restrict__ t, Job j) {
    constexpr u32 WIN = 64 * RW;
    __shared__ u64 s_keys[TPB * RW];
    const u32 par = j.epoch & 1;
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64* wk = s_keys + wave * WIN;
    const u64 wbase = ((u64)blockIdx.x * (TPB / 64) + wave) * WIN;
    if (wbase >= j.R) return;
    const u32 cnt = j.R - wbase < WIN ? (u32)(j.R - wbase) : WIN;
    // the window's keys: every load in flight before the first wait, then staged in LDS
    u64 kr[RW];
#pragma unroll
    for (int r = 0; r < RW; r++) {
        const u32 i = r * 64 + lane;
        kr[r] = j.keys[wbase + (i < cnt ? i : cnt - 1)];
    }
#pragma unroll
    for (int r = 1; r < RW; r++) wk[r * 64 + lane] = kr[r];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    u32 next = 64, my = lane, pr = 0;
    bool act = my < cnt, rcv = false;
    u64 k = kr[0];
    u64 sl = mix64(k) >> SHIFT;
    u64x2 w = {EMPTY_KEY, 0};
    u64 stt = 0;
    if (act) {
        w = *(const u64x2*)&t[sl];
        stt = t[sl].st[par];
    }
    while (__ballot(act)) {
        u64 kk = w.x, v = w.y, sx = stt;
        asm volatile("" : "+v"(kk), "+v"(v), "+v"(sx));  // the trip's loads are waited for here
        bool done = false, f = false;
        u32 ri = 0;
        if (act) {
            if (rcv) {  // the elected record has arrived
                f = done = true;
                rcv = false;
            } else if (kk == k) {
                f = resolve_at(sx, j, &ri);
                rcv = f && ri;  // the value is the round's elected record's: one more trip
                done = !rcv;
            } else if (kk == EMPTY_KEY || pr == (u32)TMASK) {
                done = true;
            }
        }
        if (done) {
            j.vals[wbase + my] = f ? v : 0;
            j.found[wbase + my] = f ? 1 : 0;
        }
        // refill: a finished lane takes the window's next Get; a lane on a chain moves one slot
        const u64 m = __ballot(done);
        if (done) {
            const u32 c = next + __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0));
            act = c < cnt;
            if (act) {
                my = c;
                k = wk[c];
                sl = mix64(k) >> SHIFT;
                pr = 0;
            }
        } else if (act && !rcv) {
            sl = (sl + 1) & TMASK;
            pr++;
        }
        next += __popcll(m);
        if (act) {
            const u64x2* p = rcv ? &j.rec[ri - 1] : (const u64x2*)&t[sl];
            w = *p;
            if (!rcv) stt = t[sl].st[par];
        }
    }
}

// ---- the product's read role around the same loop, one difference at a time ---------------------
// dyn<1>: the table's shift and mask as kernel arguments, the 80-SGPR cap; dyn<2>: + the side-key
// branch (DevCtl); dyn<3>: + the quiet / plain flags read from the job (the product's read role
// before this file, RPT = 1); dyn<4>: only plain read from the job; dyn<5>: only quiet, and the
// first stamp load unconditional; dyn<6>: dyn<2> with the side key looked at after the probe loop;
// round: + hm_round_kernel's four by-value jobs and its role dispatch (index and apply as stubs).
struct RecSrc {
    const u64x2* src;
    const u64x2* ring;
    u64 mask, lo;
    __device__ __forceinline__ u64x2 at(u64 i) const { return src ? src[i] : ring[(lo + i) & mask]; }
};
struct IndexJob {
    RecSrc rec;
    u64x2* ring_out;
    u64 n;
    u32 nblocks, nb_log, bk_shift;
    u64x2* ent;
    u32* eidx;
    u32* cnt;
    u64* dup_acc;
    bool plain;
};
struct StampJob {
    u64* dup_acc;
    RecSrc rec;
    u64x2* ring_out;
    u64 n;
    u32 nblocks, epoch;
    u32 *put_slot, *win, *over;
    u64* created_acc;
    bool plain;
};
struct ApplyJob {
    RecSrc rec;
    u64 n;
    const u32 *put_slot, *win, *over;
    u32 epoch, nblocks;
};
struct ReadJob {
    const u64* keys;
    u64 R;
    u64* vals;
    unsigned char* found;
    u32 nblocks, epoch;
    bool use_rec, quiet;
    RecSrc rec;
    u64* s_acc;
    volatile u64* s_host;
    u64 s_seq;
    bool plain;
};
struct Ctl {
    u32 err, sp_claim;
    u64 pad[7];
    Slot sp;
};

template <typename T>
__device__ __forceinline__ void st_out(T* p, T v, bool plain) {
    if (plain) *p = v;
    else __builtin_nontemporal_store(v, p);
}
__device__ __forceinline__ bool resolve(u64 val, u64 st, const ReadJob& j, u64* v) {
    const u32 se = (u32)(st >> 32);
    if (st == 0 || se > j.epoch) return false;
    *v = (se == j.epoch && j.use_rec) ? j.rec.at((u32)st - 1).y : val;
    return true;
}

template <int LV>
__device__ __forceinline__ void read_role(const ReadJob& j, u32 blk, const Slot* table, u32 shift, u64 tmask,
                                          const Ctl* ctl) {
    const u32 par = j.epoch & 1;
    const bool quiet = (LV == 3 || LV == 5) ? j.quiet : false, plain = (LV == 3 || LV == 4) ? j.plain : true;
    const u64 q = (u64)blk * TPB + threadIdx.x;
    const bool on = q < j.R;
    const u64 k = on ? j.keys[q] : EMPTY_KEY;
    u64 s = mix64(k) >> shift;
    const bool probe = on && (LV < 2 || LV == 6 || k != EMPTY_KEY);
    u64x2 w = {EMPTY_KEY, 0};
    u64 st = 0;
    if (probe) {
        w = *(const u64x2*)&table[s];
        if (LV == 5 || !quiet) st = table[s].st[par];
    }
    if (!on) return;
    u64 v = 0;
    bool f = false;
    const auto side = [&] {
        f = false;
        if (ctl->sp_claim) {
            if (quiet) {
                f = true;
                v = ctl->sp.val;
            } else {
                f = resolve(ctl->sp.val, ctl->sp.st[par], j, &v);
            }
        }
    };
    if (LV >= 2 && LV != 6 && k == EMPTY_KEY) {
        side();
    } else if (quiet) {
        u64 kk = w.x, vv = w.y, sl = s;
        for (u64 pr = 0; pr <= tmask; pr++) {
            if (kk == k) {
                f = true;
                v = vv;
                break;
            }
            if (kk == EMPTY_KEY) break;
            sl = (sl + 1) & tmask;
            const u64x2 x = *(const u64x2*)&table[sl];
            kk = x.x;
            vv = x.y;
        }
    } else {
        u64 kk = w.x, vv = w.y, stt = st, sl = s;
        asm volatile("" : "+v"(kk), "+v"(vv), "+v"(stt));
        for (u64 pr = 0; pr <= tmask; pr++) {
            if (kk == k) {
                f = resolve(vv, stt, j, &v);
                break;
            }
            if (kk == EMPTY_KEY) break;
            sl = (sl + 1) & tmask;
            const u64x2 x = *(const u64x2*)&table[sl];
            stt = table[sl].st[par];
            kk = x.x;
            vv = x.y;
            asm volatile("" : "+v"(kk), "+v"(vv), "+v"(stt));
        }
    }
    if (LV == 6 && k == EMPTY_KEY) side();  // (the side key probed the table like any key first)
    if (!f) v = 0;
    st_out(&j.vals[q], v, plain);
    st_out(&j.found[q], (unsigned char)(f ? 1 : 0), plain);
}

template <int LV>
__global__ __launch_bounds__(TPB) __attribute__((amdgpu_num_sgpr(80))) void dyn_kernel(ReadJob rj, const Slot* table,
                                                                                        u32 shift, u64 tmask,
                                                                                        const Ctl* ctl) {
    read_role<LV>(rj, blockIdx.x, table, shift, tmask, ctl);
}

__global__ __launch_bounds__(TPB) __attribute__((amdgpu_num_sgpr(80))) void round_kernel(IndexJob ij, StampJob sj,
                                                                                          ApplyJob aj, ReadJob rj,
                                                                                          Slot* table, u32 shift,
                                                                                          u64 tmask, Ctl* ctl) {
    u32 b = blockIdx.x;
    if (rj.s_seq && b == gridDim.x - 1) {  // the tail block
        if (threadIdx.x < 64) {
            u64 v = atomicExch(&rj.s_acc[threadIdx.x], 0ull);
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            if (threadIdx.x == 0) {
                rj.s_host[1] = v;
                __threadfence_system();
                rj.s_host[0] = rj.s_seq;
            }
        }
        return;
    }
    const u32 nix = sj.nblocks + ij.nblocks;
    if (b < nix) {  // (stub of the index role: never launched here)
        const u64 i = (u64)b * TPB + threadIdx.x;
        if (i < sj.n) {
            const u64x2 r = sj.rec.at(i);
            if (sj.ring_out) sj.ring_out[(sj.rec.lo + i) & sj.rec.mask] = r;
            sj.put_slot[i] = (u32)(mix64(r.x) >> shift);
            sj.win[i] = sj.epoch;
            if (ij.ent) ij.ent[i] = ij.rec.at(i);
        }
        return;
    }
    b -= nix;
    if (b < aj.nblocks) {  // (the apply role)
        const u64 i = (u64)b * TPB + threadIdx.x;
        if (i >= aj.n) return;
        const u32 s = aj.put_slot[i];
        if (aj.win[i] == aj.epoch && aj.over[i] != aj.epoch) __builtin_nontemporal_store(aj.rec.at(i).y, &table[s].val);
        return;
    }
    b -= aj.nblocks;
    read_role<3>(rj, b, table, shift, tmask, ctl);
}

// ---- the line-grouped probe sequence: a quad of lanes reads a Get's whole 128-B group per trip ----
// (common.hpp probe_slot, restated) round the home's four-slot group from the home slot, then the
// next group from the same offset, ...: a present key lies in the first group of its sequence that
// had an empty slot when it was inserted, so a group with an empty slot and no match ends a search.
__host__ __device__ constexpr u64 probe_slot(u64 home, u64 p, u64 tmask) {
    return ((((home >> 2) + (p >> 2)) << 2) | ((home + p) & 3)) & tmask;
}

// quad_perm DPP moves (lane ^ 1, lane ^ 2 inside each four lanes) and the OR over a quad
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

// A wave owns 16 * PASSES consecutive Gets; in pass p the quad of lanes 4g .. 4g+3 owns Get 16 p + g
// and lane sub = lane & 3 loads slot sub of the Get's home group: {key, val} and the stamp, back to
// back, every pass's loads issued before the first wait. At most one lane of a quad matches (a key
// sits in one slot), so the quad's answer is the OR of its lanes' (0 where there is no match); a
// quad with no match and no empty slot goes on to the next group (rare: a full group).
// PASSES 4 = (A): a block owns 256 Gets as today, and the answers go back to one Get per lane (one
// 64-bit shuffle), so a wave stores whole 512-B / 64-B runs. PASSES 1 = (B): 64 Gets per block,
// lane 0 of each quad stores. STAMP as the product's read_role<STAMP>.
template <int PASSES, bool STAMP, bool KSHFL = false>
__device__ __forceinline__ void group_role(const ReadJob& j, u32 blk, const Slot* table, u32 shift, u64 tmask,
                                           const Ctl* ctl) {
    const u32 par = j.epoch & 1;
    const auto quiet = [&] { return STAMP ? false : j.quiet; };
    const auto plain = [&] { return STAMP ? true : j.plain; };
    const u32 lane = threadIdx.x & 63, sub = lane & 3, quad = lane >> 2, qsh = lane & ~3u;
    const u64 wbase = ((u64)blk * (TPB / 64) + (threadIdx.x >> 6)) * (16 * PASSES);
    if (wbase >= j.R) return;
    u64 k[PASSES], s[PASSES], st[PASSES];
    u64x2 w[PASSES];
    bool probe[PASSES];
    if (KSHFL) {  // one coalesced key load per wave, the passes' keys by shuffle
        const u64 kown = wbase + lane < j.R ? j.keys[wbase + lane] : EMPTY_KEY;
#pragma unroll
        for (int p = 0; p < PASSES; p++) k[p] = __shfl(kown, (int)(p * 16 + quad), 64);
    } else {
#pragma unroll
        for (int p = 0; p < PASSES; p++) {
            const u64 q = wbase + p * 16 + quad;
            k[p] = q < j.R ? j.keys[q] : EMPTY_KEY;  // (a Get past the end reads as the side key and is not stored)
        }
    }
#pragma unroll
    for (int p = 0; p < PASSES; p++) {
        s[p] = (((mix64(k[p]) >> shift) & ~3ull) | sub) & tmask;
        probe[p] = k[p] != EMPTY_KEY;
        w[p].x = EMPTY_KEY;
        w[p].y = 0;
        st[p] = 0;
        if (probe[p]) {
            w[p] = *(const u64x2*)&table[s[p]];
            if (!quiet()) st[p] = table[s[p]].st[par];
        }
    }
    u64 rv[PASSES], fb[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; p++) {
        u64 kk = w[p].x, vv = w[p].y, stt = st[p], sl = s[p], v = 0;
        asm volatile("" : "+v"(kk), "+v"(vv), "+v"(stt));
        bool f = false, act = probe[p];
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
            // the quad is done on a match or an empty slot (a lane that does not probe reads as empty)
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
        if (k[p] == EMPTY_KEY && sub == 0 && ctl->sp_claim) {  // the side key
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
    if (PASSES == 1) {
        const u64 q = wbase + quad;
        if (sub == 0 && q < j.R) {
            st_out(&j.vals[q], rv[0], plain());
            st_out(&j.found[q], (unsigned char)(((fb[0] >> qsh) & 15) != 0), plain());
        }
    } else {
        // lane l holds pass (l & 3)'s answer of its quad; Get L = 16 p + g sits in lane 4 g + p
        u64 c = rv[0], b = fb[0];
#pragma unroll
        for (int p = 1; p < PASSES; p++) {
            if (sub == (u32)p) c = rv[p];
            if ((lane >> 4) == (u32)p) b = fb[p];
        }
        const u64 v = __shfl(c, (int)(4 * (lane & 15) + (lane >> 4)), 64);
        const u64 q = wbase + lane;
        if (q < j.R) {
            st_out(&j.vals[q], v, plain());
            st_out(&j.found[q], (unsigned char)(((b >> (4 * (lane & 15))) & 15) != 0), plain());
        }
    }
}

template <int PASSES, bool STAMP, bool KSHFL = false>
__global__ __launch_bounds__(TPB) __attribute__((amdgpu_num_sgpr(80))) void group_kernel(ReadJob rj, const Slot* table,
                                                                                          u32 shift, u64 tmask,
                                                                                          const Ctl* ctl) {
    group_role<PASSES, STAMP, KSHFL>(rj, blockIdx.x, table, shift, tmask, ctl);
}

__global__ void init_table(Slot* t, u64 slots) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (u64)gridDim.x * blockDim.x) {
        Slot s;
        s.key = EMPTY_KEY;
        s.val = 0;
        s.st[0] = s.st[1] = 0;
        t[i] = s;
    }
}

// as hm_prefill_range_kernel: claim by CAS from the home slot; GROUPED: the line-grouped sequence
// (probe_slot), else linear probing (the yardsticks' table)
template <bool GROUPED>
__global__ void prefill(Slot* t, u64 n) {
    for (u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (u64)gridDim.x * blockDim.x) {
        const u64 home = mix64(k) >> SHIFT;
        u64 s = home;
        for (u64 pr = 0; pr <= TMASK; pr++) {
            const u64 old = atomicCAS(&t[s].key, EMPTY_KEY, k);
            if (old == EMPTY_KEY || old == k) {
                t[s].val = k + 1;
                t[s].st[0] = t[s].st[1] = STAMP_PRESENT;
                break;
            }
            s = GROUPED ? probe_slot(home, pr + 1, TMASK) : (s + 1) & TMASK;
        }
    }
}

// groups read by every Get of a batch over the grouped table (1 = answered from its home group), capped at 16
__global__ void count_groups(const Slot* __restrict__ t, const u64* __restrict__ keys, u64 n, unsigned char* groups) {
    const u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const u64 k = keys[q];
    u64 g = (mix64(k) >> SHIFT) & ~3ull;
    u32 p = 1;
    for (; p < 16; p++) {
        bool end = false;
        for (int x = 0; x < 4; x++) end = end || t[g + x].key == k || t[g + x].key == EMPTY_KEY;
        if (end) break;
        g = (g + 4) & TMASK;
    }
    groups[q] = (unsigned char)p;
}

// probes of every Get of a batch (1 = ends at its home slot), capped at 16
__global__ void count_probes(const Slot* __restrict__ t, const u64* __restrict__ keys, u64 n, unsigned char* probes) {
    const u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const u64 k = keys[q];
    u64 s = mix64(k) >> SHIFT;
    u32 p = 1;
    while (p < 16 && t[s].key != k && t[s].key != EMPTY_KEY) {
        s = (s + 1) & TMASK;
        p++;
    }
    probes[q] = (unsigned char)p;
}

enum Variant { V_FIRST, V_CHAIN, V_REFILL2, V_REFILL4, V_REFILL8, V_DYN1, V_DYN2, V_DYN3, V_DYN4, V_DYN5, V_DYN6, V_ROUND, V_ROUNDQ, V_GROUPA, V_GROUPB, V_GROUPAQ, V_GROUPBQ, V_GROUPAS };
static Ctl* g_ctl;

static void launch(Variant v, const Slot* t, Job j, hipStream_t st) {
    const u64 n = j.R;
    switch (v) {
    case V_FIRST: first_kernel<<<(unsigned)((n + TPB - 1) / TPB), TPB, 0, st>>>(t, j); break;
    case V_CHAIN: chain_kernel<<<(unsigned)((n + TPB - 1) / TPB), TPB, 0, st>>>(t, j); break;
    case V_REFILL2: refill_kernel<2><<<(unsigned)((n + TPB * 2 - 1) / (TPB * 2)), TPB, 0, st>>>(t, j); break;
    case V_REFILL4: refill_kernel<4><<<(unsigned)((n + TPB * 4 - 1) / (TPB * 4)), TPB, 0, st>>>(t, j); break;
    case V_REFILL8: refill_kernel<8><<<(unsigned)((n + TPB * 8 - 1) / (TPB * 8)), TPB, 0, st>>>(t, j); break;
    default: {
        const unsigned grid = (unsigned)((n + TPB - 1) / TPB), grid_b = (unsigned)((n + 63) / 64);
        IndexJob ij{};
        StampJob sj{};
        ApplyJob aj{};
        ReadJob rj{};
        rj.keys = j.keys;
        rj.R = n;
        rj.vals = j.vals;
        rj.found = j.found;
        rj.nblocks = grid;
        rj.epoch = j.epoch;
        rj.use_rec = j.use_rec;
        rj.rec.ring = j.rec;
        rj.rec.mask = 255;
        // reads-only rounds: no stamps read, streamed responses asked for
        rj.quiet = v == V_ROUNDQ || v == V_GROUPAQ || v == V_GROUPBQ;
        rj.plain = !rj.quiet;
        if (v == V_DYN1) dyn_kernel<1><<<grid, TPB, 0, st>>>(rj, t, SHIFT, TMASK, g_ctl);
        else if (v == V_DYN2) dyn_kernel<2><<<grid, TPB, 0, st>>>(rj, t, SHIFT, TMASK, g_ctl);
        else if (v == V_DYN3) dyn_kernel<3><<<grid, TPB, 0, st>>>(rj, t, SHIFT, TMASK, g_ctl);
        else if (v == V_DYN4) dyn_kernel<4><<<grid, TPB, 0, st>>>(rj, t, SHIFT, TMASK, g_ctl);
        else if (v == V_DYN5) dyn_kernel<5><<<grid, TPB, 0, st>>>(rj, t, SHIFT, TMASK, g_ctl);
        else if (v == V_DYN6) dyn_kernel<6><<<grid, TPB, 0, st>>>(rj, t, SHIFT, TMASK, g_ctl);
        else if (v == V_GROUPA) group_kernel<4, true><<<grid, TPB, 0, st>>>(rj, t, SHIFT, TMASK, g_ctl);
        else if (v == V_GROUPAS) group_kernel<4, true, true><<<grid, TPB, 0, st>>>(rj, t, SHIFT, TMASK, g_ctl);
        else if (v == V_GROUPB) group_kernel<1, true><<<grid_b, TPB, 0, st>>>(rj, t, SHIFT, TMASK, g_ctl);
        else if (v == V_GROUPAQ) group_kernel<4, false><<<grid, TPB, 0, st>>>(rj, t, SHIFT, TMASK, g_ctl);
        else if (v == V_GROUPBQ) group_kernel<1, false><<<grid_b, TPB, 0, st>>>(rj, t, SHIFT, TMASK, g_ctl);
        else round_kernel<<<grid, TPB, 0, st>>>(ij, sj, aj, rj, (Slot*)t, SHIFT, TMASK, g_ctl);
    }
    }
}

static double run(Variant v, const char* name, const Slot* t, u64* const* keys, Job j, hipStream_t st) {
    for (int i = 0; i < 16; i++) {
        j.keys = keys[i & 15];
        launch(v, t, j, st);
    }
    hipEvent_t a, b;
    CHK(hipEventCreate(&a));
    CHK(hipEventCreate(&b));
    const int L = 64;
    CHK(hipEventRecord(a, st));
    for (int i = 0; i < L; i++) {
        j.keys = keys[i & 15];
        launch(v, t, j, st);
    }
    CHK(hipEventRecord(b, st));
    CHK(hipEventSynchronize(b));
    CHK(hipGetLastError());
    float ms = 0;
    CHK(hipEventElapsedTime(&ms, a, b));
    const double us = ms * 1e3 / L;
    printf("%-8s %8.2f us per launch  %7.2f G gets/s\n", name, us, j.R / us / 1e3);
    CHK(hipEventDestroy(a));
    CHK(hipEventDestroy(b));
    return us;
}

int main(int argc, char** argv) {
    const u64 n = argc > 1 ? strtoull(argv[1], 0, 10) : 900000ull;
    const u64 slots = 1ull << LOG2_SLOTS;
    Slot *t, *tg;  // the linear-probing table of the yardsticks and the line-grouped one
    CHK(hipMalloc((void**)&t, slots * sizeof(Slot)));
    CHK(hipMalloc((void**)&tg, slots * sizeof(Slot)));
    init_table<<<4096, 256>>>(t, slots);
    init_table<<<4096, 256>>>(tg, slots);
    prefill<false><<<4096, 256>>>(t, NKEYS);
    prefill<true><<<4096, 256>>>(tg, NKEYS);
    CHK(hipDeviceSynchronize());
    u64* keys[16];
    u64* h = (u64*)malloc(n * 8);
    for (int b = 0; b < 16; b++) {
        for (u64 i = 0; i < n; i++) h[i] = mix64(0x9e3779b97f4a7c15ull * (b * n + i + 1)) % 10000000ull;
        CHK(hipMalloc((void**)&keys[b], n * 8));
        CHK(hipMemcpy(keys[b], h, n * 8, hipMemcpyHostToDevice));
    }
    u64 *vals, *vals2;
    unsigned char *found, *found2, *probes;
    u64x2* rec;
    CHK(hipMalloc((void**)&vals, n * 8));
    CHK(hipMalloc((void**)&vals2, n * 8));
    CHK(hipMalloc((void**)&found, n));
    CHK(hipMalloc((void**)&found2, n));
    CHK(hipMalloc((void**)&probes, n));
    CHK(hipMalloc((void**)&rec, 4096));
    CHK(hipMalloc((void**)&g_ctl, sizeof(Ctl)));
    CHK(hipMemset(g_ctl, 0, sizeof(Ctl)));
    hipStream_t st;
    CHK(hipStreamCreate(&st));
    printf("read_chain: %llu Gets per launch, 2^%d x 32-B slots holding keys [0, 2^23) hashed, linear probing\n",
           (unsigned long long)n, LOG2_SLOTS);

    // the probe-length distribution of batch 0 and the trips of a 64-Get wave
    count_probes<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(t, keys[0], n, probes);
    unsigned char* hp = (unsigned char*)malloc(n);
    CHK(hipMemcpyAsync(hp, probes, n, hipMemcpyDeviceToHost, st));
    CHK(hipStreamSynchronize(st));
    {
        u64 hist[17] = {0}, total = 0, wave_trips = 0, waves = 0, wt[17] = {0};
        for (u64 i = 0; i < n; i += 64) {
            u32 mx = 0;
            for (u64 q = i; q < i + 64 && q < n; q++) {
                hist[hp[q]]++;
                total += hp[q];
                if (hp[q] > mx) mx = hp[q];
            }
            wave_trips += mx;
            wt[mx]++;
            waves++;
        }
        printf("probes per Get %.4f; Gets needing >= 2 probes %.2f %%, >= 3 %.2f %%, >= 4 %.2f %%\n", (double)total / n,
               100.0 * (n - hist[1]) / n, 100.0 * (n - hist[1] - hist[2]) / n,
               100.0 * (n - hist[1] - hist[2] - hist[3]) / n);
        printf("trips per 64-Get wave %.3f; waves with 1 trip %.2f %%, >= 3 %.2f %%, >= 4 %.2f %%\n",
               (double)wave_trips / waves, 100.0 * wt[1] / waves, 100.0 * (waves - wt[1] - wt[2]) / waves,
               100.0 * (waves - wt[1] - wt[2] - wt[3]) / waves);
    }
    count_groups<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(tg, keys[0], n, probes);
    CHK(hipMemcpyAsync(hp, probes, n, hipMemcpyDeviceToHost, st));
    CHK(hipStreamSynchronize(st));
    {
        u64 more = 0, waves = 0, wmore = 0;
        for (u64 i = 0; i < n; i += 64) {
            bool any = false;
            for (u64 q = i; q < i + 64 && q < n; q++) {
                more += hp[q] > 1;
                any = any || hp[q] > 1;
            }
            wmore += any;
            waves++;
        }
        printf("line-grouped table: Gets needing >= 2 groups %.4f %%; 64-Get runs with such a Get %.2f %%\n",
               100.0 * more / n, 100.0 * wmore / waves);
    }
    free(hp);

    Job j;
    j.R = n;
    j.vals = vals;
    j.found = found;
    j.epoch = 2;
    j.use_rec = true;  // never taken (every stamp is of epoch 1), compiled in as in the product
    j.rec = rec;

    // refill's answers against chain's, batch 0
    {
        Job a = j, b = j;
        a.keys = b.keys = keys[0];
        b.vals = vals2;
        b.found = found2;
        u64* hv = (u64*)malloc(n * 8);
        u64* hv2 = (u64*)malloc(n * 8);
        unsigned char* hf = (unsigned char*)malloc(n);
        unsigned char* hf2 = (unsigned char*)malloc(n);
        launch(V_CHAIN, t, a, st);
        CHK(hipMemcpyAsync(hv, vals, n * 8, hipMemcpyDeviceToHost, st));
        CHK(hipMemcpyAsync(hf, found, n, hipMemcpyDeviceToHost, st));
        CHK(hipStreamSynchronize(st));
        // chain's own answers against the CPU's: key k < NKEYS holds k + 1
        for (u64 i = 0; i < n; i++) {
            const u64 k = mix64(0x9e3779b97f4a7c15ull * (i + 1)) % 10000000ull;  // batch 0's Get i
            if (hf[i] != (k < NKEYS) || hv[i] != (k < NKEYS ? k + 1 : 0)) {
                printf("chain answers DIFFER FROM the CPU lookup at Get %llu\n", (unsigned long long)i);
                return 1;
            }
        }
        printf("chain answers equal the CPU lookup\n");
        const Variant rv[16] = {V_REFILL2, V_REFILL4, V_REFILL8, V_DYN1, V_DYN2, V_DYN3, V_DYN4, V_DYN5, V_DYN6, V_ROUND, V_ROUNDQ,
                                V_GROUPA, V_GROUPB, V_GROUPAQ, V_GROUPBQ, V_GROUPAS};
        const char* rn[16] = {"refill2", "refill4", "refill8", "dyn1", "dyn2", "dyn3", "dyn4", "dyn5", "dyn6", "round", "round_q",
                              "groupA", "groupB", "groupA_q", "groupB_q", "groupA_s"};
        for (int x = 0; x < 16; x++) {
            CHK(hipMemsetAsync(vals2, 0xAB, n * 8, st));
            CHK(hipMemsetAsync(found2, 0xAB, n, st));
            launch(rv[x], rv[x] >= V_GROUPA ? tg : t, b, st);
            CHK(hipMemcpyAsync(hv2, vals2, n * 8, hipMemcpyDeviceToHost, st));
            CHK(hipMemcpyAsync(hf2, found2, n, hipMemcpyDeviceToHost, st));
            CHK(hipStreamSynchronize(st));
            const bool same = !memcmp(hv, hv2, n * 8) && !memcmp(hf, hf2, n);
            printf("%s answers %s chain's\n", rn[x], same ? "equal" : "DIFFER FROM");
            if (!same) return 1;
        }
        u64 nf = 0;
        for (u64 i = 0; i < n; i++) nf += hf[i];
        printf("found %.2f %% of the Gets\n", 100.0 * nf / n);
        free(hv);
        free(hv2);
        free(hf);
        free(hf2);
    }
    free(h);

    for (int rep = 0; rep < 3; rep++) {
        run(V_FIRST, "first", t, keys, j, st);
        run(V_CHAIN, "chain", t, keys, j, st);
        run(V_REFILL2, "refill2", t, keys, j, st);
        run(V_REFILL4, "refill4", t, keys, j, st);
        run(V_REFILL8, "refill8", t, keys, j, st);
        run(V_DYN1, "dyn1", t, keys, j, st);
        run(V_DYN2, "dyn2", t, keys, j, st);
        run(V_DYN3, "dyn3", t, keys, j, st);
        run(V_DYN4, "dyn4", t, keys, j, st);
        run(V_DYN5, "dyn5", t, keys, j, st);
        run(V_DYN6, "dyn6", t, keys, j, st);
        run(V_ROUND, "round", t, keys, j, st);
        run(V_ROUNDQ, "round_q", t, keys, j, st);
        run(V_GROUPA, "groupA", tg, keys, j, st);
        run(V_GROUPB, "groupB", tg, keys, j, st);
        run(V_GROUPAQ, "groupA_q", tg, keys, j, st);
        run(V_GROUPBQ, "groupB_q", tg, keys, j, st);
        run(V_GROUPAS, "groupA_s", tg, keys, j, st);
    }
    CHK(hipStreamSynchronize(st));
    for (int b = 0; b < 16; b++) CHK(hipFree(keys[b]));
    CHK(hipFree(vals));
    CHK(hipFree(vals2));
    CHK(hipFree(found));
    CHK(hipFree(found2));
    CHK(hipFree(probes));
    CHK(hipFree(rec));
    CHK(hipFree(g_ctl));
    CHK(hipFree(t));
    CHK(hipFree(tg));
    return 0;
}
