// vspace.hip — replicated x86-64 four-level page table (VSpace) replay on gfx950
// (benches/vspace.rs:177-381 VSpace::map_generic, :436-467 resolve_addr, :499-526 VSpaceDispatcher:
// OpcodeWr::Map / OpcodeWr::MapDevice, OpcodeRd::Identify).
//
// The replica's tables live in a pool of 4 KiB tables (512 u64 entries each), zeroed at open and
// never freed. Table 0 is the PML4. An inner entry holds table_index * 4096 | P|RW|US (new_pdpt /
// new_pd / new_pt, :406-419); a leaf is paddr | P | rights (4 KiB) or paddr | P | PS | rights
// (2 MiB), rights as to_pt_rights / to_pd_rights (:92-122). 1 GiB pages never arise (len < 2^30).
//
// One op is walked frame by frame exactly as map_generic recurses (vs_walk): a frame starts at the
// op's vbase, after a run of 2 MiB pages and whenever the 4 KiB loop leaves a PT; an error answers
// the vbase of the frame it happened in, and everything written before it stays.
//
// Order. Two ops depend on each other when their [vbase, vbase + len) ranges, rounded out to
// 2 MiB granules, intersect (a zero-length op occupies its start granule). Ops in distinct granules
// share only inner tables, and no decision depends on who created those. The ops of a chunk with no
// earlier dependent op in the chunk (the chunk's first wave) are mutually independent and replay in
// parallel; every other op replays after them, in log order, in one workgroup. An op of the first
// wave precedes every op of the chunk it depends on, so the result is the sequential one.
//
// Six launches per chunk of up to 4096 ops (one more vs_seq_kernel for every further 4096), in
// stream order, none of which waits on another workgroup:
//   vs_prep_kernel   domain check, granule range per op, the log copy of a fused round
//   vs_dep_kernel    first wave or not, per op: a workgroup per pair of op tiles (x, y <= x)
//   vs_plan_kernel   one wave per first-wave op: the walk without stores: how many PTs the op
//                    creates before it ends or fails, and which page directories its frames reach
//   vs_alloc_kernel  one workgroup: the missing PDPTs and PDs the first wave reaches, deduplicated
//                    in two LDS bitmaps (512 PML4 slots, 2^18 PDPT slots) and numbered by bit rank;
//                    an exclusive scan of the ops' PT counts gives each op its PT range. Tables are
//                    counted, scanned and assigned, never raced for, so the table count is the
//                    sequential model's. First the total, plus the most the other ops can create
//                    (a PT per granule and four inner tables each), is compared with the pool: if
//                    the chunk might not fit, the first wave is handed to vs_seq_kernel, the whole
//                    chunk replays in log order, exactly the ops that do not fit are left out and
//                    ERR_CAPACITY is latched. The pool never runs out in a chunk replayed in parallel.
//   vs_apply_kernel  one workgroup per first-wave op: the same walk with stores (PTE runs are
//                    contiguous 8-B stores by consecutive lanes) and the response
//   vs_seq_kernel    one workgroup: every other op of a 4096-op slice in log order: walk without
//                    stores, capacity check, inner tables, walk with stores
#include <cstring>
#include <new>

#include "internal.hpp"

namespace nrg {

constexpr int VS_TPB = 256;          // lanes of a per-op workgroup that stores (and of prep / dep tiles)
constexpr int VS_PLAN_TPB = 64;      // one wave walks an op that stores nothing
constexpr u64 VS_SEQ_SLICE = 4096;   // ops of the chunk one in-order launch covers
constexpr int VS_ALLOC_TPB = 1024;   // lanes of the allocation workgroup
constexpr int VS_SEQ_TPB = 1024;     // lanes of the in-order workgroup: a 65,535-page op is 64 stores per lane
constexpr u32 VS_MAXG = 513;         // 2 MiB granules an op can touch (len < 2^30, any alignment)
constexpr u64 VS_P = 1, VS_RW = 2, VS_US = 4, VS_PS = 0x80, VS_XD = 1ull << 63;
constexpr u64 VS_ADDR = 0x000ffffffffff000ull;  // x86 ADDRESS_MASK: bits 12..51
constexpr u64 VS_INNER = VS_P | VS_RW | VS_US;
constexpr u64 VS_2M = 1ull << 21;
constexpr u32 VS_NONE = 0xFFFFFFFFu;
constexpr u32 VS_PDS = 1u << 18;     // page directories of the address space: (PML4 slot, PDPT slot)
constexpr uint8_t VS_F_INVALID = 0, VS_F_FIRST = 1, VS_F_LATER = 2;

struct VsJob {
    const nrg_vspace_op* src;  // the batch of a fused round (its log copy is written by prep), or
    nrg_vspace_op* ring;       // nullptr: the records are read from the log ring
    u64 ring_mask;
    u64 lo, n;                 // the chunk: log indices [lo, lo + n)
    u64 rlo, rhi;              // response window (log indices); resp == nullptr: none wanted
    nrg_vspace_resp* resp;
    uint8_t* some;
    u64* pool;
    u64 cap;                   // tables the pool holds
    VsState* st;
    DevCtl* ctl;
    u32* glo;                  // [n] first and last granule of each op (VS_NONE, 0: out of domain)
    u32* ghi;
    u32* npt;                  // [n] PTs a first-wave op creates
    u32* key;                  // [n] its first page directory (18 bits); bit 31: it reaches the next one
    u32* ptbase;               // [n] its first PT
    uint8_t* flag;             // [n] VS_F_*
};

__device__ __forceinline__ nrg_vspace_op vs_load(const VsJob& j, u64 i) {
    return j.src ? j.src[i] : j.ring[(j.lo + i) & j.ring_mask];
}

// leaf flags without PS: MapDevice maps ReadWriteUser (:519-523)
__device__ __forceinline__ u64 vs_leaf_flags(const nrg_vspace_op& o) {
    const u32 r = o.op == NRG_VSPACE_MAP_DEVICE ? 3u : o.rights;
    u64 f = VS_P;
    if (r == 3 || r == 4 || r == 7 || r == 8) f |= VS_RW;
    if (!(r & 1)) f |= VS_US;
    if (r <= 4) f |= VS_XD;
    return f;
}

__device__ __forceinline__ bool vs_in_domain(const nrg_vspace_op& o) {
    const u64 lim = 1ull << 48;
    if ((o.vbase | o.pbase | o.len) & 4095) return false;
    if (o.vbase >= lim || o.pbase >= lim || o.len >= (1ull << 30) || o.vbase + o.len > lim) return false;
    if (o.op == NRG_VSPACE_MAP) return o.rights >= 1 && o.rights <= 8;
    return o.op == NRG_VSPACE_MAP_DEVICE;
}

__device__ __forceinline__ void vs_answer(const VsJob& j, u64 i, bool ok, u64 a, u64 b) {
    const u64 g = j.lo + i;
    if (j.resp && g >= j.rlo && g < j.rhi) {
        j.resp[g - j.rlo] = nrg_vspace_resp{a, b};
        j.some[g - j.rlo] = ok ? 1 : 0;
    }
}

// the minimum of v over the workgroup, in every lane (s_red: one int per wave)
__device__ __forceinline__ int vs_block_min(int v, int* s_red) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const int o = __shfl_xor(v, s, 64);
        v = o < v ? o : v;
    }
    __syncthreads();  // the previous reduction's readers are done with s_red
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = s_red[0];
    for (u32 k = 1; k < (blockDim.x >> 6); k++) r = s_red[k] < r ? s_red[k] : r;
    return r;
}

// table of page directory k = PML4 slot << 9 | PDPT slot, or VS_NONE (the same in every lane)
__device__ __forceinline__ u32 vs_pd_table(const u64* pool, u32 k) {
    if (k >= VS_PDS) return VS_NONE;
    u64 e = ld_relaxed(pool + (k >> 9));
    if (!(e & VS_P)) return VS_NONE;
    e = ld_relaxed(pool + ((e & VS_ADDR) >> 12) * 512 + (k & 511));
    if (!(e & VS_P)) return VS_NONE;
    return (u32)((e & VS_ADDR) >> 12);
}

// inner tables missing on the way to page directory k: 2 (PDPT and PD), 1 (PD) or 0
__device__ __forceinline__ u32 vs_inner_need(const u64* pool, u32 k) {
    const u64 e = ld_relaxed(pool + (k >> 9));
    if (!(e & VS_P)) return 2;
    return (ld_relaxed(pool + ((e & VS_ADDR) >> 12) * 512 + (k & 511)) & VS_P) ? 0 : 1;
}

// the PD entries of the op's granules into LDS (0 where the page directory does not exist)
__device__ __forceinline__ void vs_load_pd(const u64* pool, const nrg_vspace_op& o, u32 tabA, u32 tabB, u64* s_pd) {
    const u32 g0 = (u32)(o.vbase >> 21);
    const u32 G = (o.len ? (u32)((o.vbase + o.len - 1) >> 21) : g0) - g0 + 1;
    __syncthreads();  // the previous op's walk is done with s_pd
    for (u32 g = threadIdx.x; g < G; g += blockDim.x) {
        const u32 gr = g0 + g;
        const u32 tab = (gr >> 9) == (g0 >> 9) ? tabA : tabB;
        s_pd[g] = tab == VS_NONE ? 0 : ld_relaxed(pool + (u64)tab * 512 + (gr & 511));
    }
    __syncthreads();
}

struct VsOut {
    u64 at;       // vbase of the last frame entered (the error's `at`)
    u32 npt;      // PTs created
    bool err;
    bool reach2;  // a frame started in the op's second page directory
};

// map_generic, frame by frame; the whole workgroup runs it with the same control flow. WRITE =
// false stores nothing. tabA / tabB: the tables of the op's first and second page directory (they
// exist when WRITE); ptbase: the op's first new PT. The allocation passes size the pool before
// anything is stored; `cap` only keeps a store inside the pool should they ever disagree.
template <bool WRITE>
__device__ VsOut vs_walk(u64* pool, u64 cap, const nrg_vspace_op& o, const u64* s_pd, int* s_red, u32 tabA,
                         u32 tabB, u32 ptbase) {
    const u32 g0 = (u32)(o.vbase >> 21);
    const u64 fl = vs_leaf_flags(o);
    const u64 delta = o.pbase - o.vbase;              // paddr of vaddr v: v + delta
    const bool cong = (delta & (VS_2M - 1)) == 0;     // pbase is 2 MiB-aligned wherever vbase is
    u64 v = o.vbase, rem = o.len;
    VsOut out{v, 0, false, false};
    for (;;) {
        const u32 gr = (u32)(v >> 21), g = gr - g0, idx = gr & 511;
        const bool second = (gr >> 9) != (g0 >> 9);
        if (second) out.reach2 = true;
        const u32 tab = second ? tabB : tabA;
        u64* pd = pool + (u64)tab * 512;
        out.at = v;
        if (WRITE && tab >= cap) {
            out.err = true;
            return out;
        }
        const u64 e = s_pd[g];
        const u32 pi = (u32)(v >> 12) & 511;
        u32 cnt = 512 - pi;  // 4 KiB pages of this frame
        if ((rem >> 12) < cnt) cnt = (u32)(rem >> 12);
        if (!(e & VS_P)) {
            if (!(v & (VS_2M - 1)) && cong && rem >= VS_2M) {
                // a run of 2 MiB pages: while 2 MiB remain and the PD has slots (:295-315)
                u32 k = 512 - idx;
                if ((rem >> 21) < k) k = (u32)(rem >> 21);
                int f = (int)k;
                for (u32 t = threadIdx.x; t < k; t += blockDim.x)
                    if (s_pd[g + t] & VS_P) {
                        f = (int)t;
                        break;
                    }
                f = vs_block_min(f, s_red);
                if (WRITE)
                    for (u32 t = threadIdx.x; t < (u32)f; t += blockDim.x)
                        pd[idx + t] = (v + delta + (u64)t * VS_2M) | fl | VS_PS;
                if ((u32)f < k) {
                    out.err = true;
                    return out;
                }
                v += (u64)k << 21;
                rem -= (u64)k << 21;
            } else {
                const u32 pt = ptbase + out.npt;  // new_pt (:341)
                if (WRITE && pt >= cap) {
                    out.err = true;
                    return out;
                }
                out.npt++;
                if (WRITE) {
                    if (threadIdx.x == 0) pd[idx] = ((u64)pt << 12) | VS_INNER;
                    u64* p = pool + (u64)pt * 512 + pi;
                    for (u32 t = threadIdx.x; t < cnt; t += blockDim.x) p[t] = (v + delta + ((u64)t << 12)) | fl;
                }
                v += (u64)cnt << 12;
                rem -= (u64)cnt << 12;
            }
        } else if (e & VS_PS) {  // a 2 MiB page covers the frame's start (:348-351)
            out.err = true;
            return out;
        } else {
            u64* p = pool + ((e & VS_ADDR) >> 12) * 512 + pi;
            int f = (int)cnt;  // the first present PTE of the frame
            for (u32 t = threadIdx.x; t < cnt; t += blockDim.x)
                if (ld_relaxed(p + t) & VS_P) {
                    f = (int)t;
                    break;
                }
            f = vs_block_min(f, s_red);  // (its barriers: every lane has read before any lane stores)
            if (WRITE)
                for (u32 t = threadIdx.x; t < (u32)f; t += blockDim.x) p[t] = (v + delta + ((u64)t << 12)) | fl;
            if ((u32)f < cnt) {
                out.err = true;
                return out;
            }
            v += (u64)cnt << 12;
            rem -= (u64)cnt << 12;
        }
        if (rem == 0) return out;
    }
}

__device__ __forceinline__ void vs_respond(const VsJob& j, u64 i, const nrg_vspace_op& o, const VsOut& w) {
    if (threadIdx.x != 0) return;
    if (w.err)
        vs_answer(j, i, false, w.at, 0);
    else if (o.op == NRG_VSPACE_MAP)
        vs_answer(j, i, true, o.pbase, o.len);  // Ok((pbase, len)) (:515-518)
    else
        vs_answer(j, i, true, 0, 0);            // Ok((0, 0)) (:519-523)
}

__global__ __launch_bounds__(VS_TPB) void vs_prep_kernel(VsJob j) {
    const u64 i = (u64)blockIdx.x * VS_TPB + threadIdx.x;
    if (i >= j.n) return;
    const nrg_vspace_op o = vs_load(j, i);
    if (j.src) j.ring[(j.lo + i) & j.ring_mask] = o;  // Log::append of a fused round
    j.npt[i] = 0;
    if (!vs_in_domain(o)) {  // the reference asserts; here: nothing changes, Err(at = vbase), latched
        j.glo[i] = VS_NONE;
        j.ghi[i] = 0;
        j.flag[i] = VS_F_INVALID;
        atomicOr(&j.ctl->err, ERR_INVAL);
        vs_answer(j, i, false, o.vbase, 0);
        return;
    }
    j.flag[i] = VS_F_FIRST;  // until vs_dep_kernel finds an earlier op on one of its granules
    j.glo[i] = (u32)(o.vbase >> 21);
    j.ghi[i] = o.len ? (u32)((o.vbase + o.len - 1) >> 21) : (u32)(o.vbase >> 21);
}

// workgroup (x, y): the ops of tile x against the ops of tile y <= x
__global__ __launch_bounds__(VS_TPB) void vs_dep_kernel(VsJob j) {
    __shared__ u32 s_lo[VS_TPB], s_hi[VS_TPB];
    if (blockIdx.y > blockIdx.x) return;
    const u32 t = threadIdx.x;
    const u64 i = (u64)blockIdx.x * VS_TPB + t, jb = (u64)blockIdx.y * VS_TPB;
    s_lo[t] = jb + t < j.n ? j.glo[jb + t] : VS_NONE;
    s_hi[t] = jb + t < j.n ? j.ghi[jb + t] : 0;
    __syncthreads();
    if (i >= j.n) return;
    const u32 lo = j.glo[i], hi = j.ghi[i];
    bool dep = false;
    for (u32 q = 0; q < VS_TPB; q++)
        if (jb + q < i && s_lo[q] <= hi && lo <= s_hi[q]) dep = true;
    if (dep) j.flag[i] = VS_F_LATER;  // (every workgroup that finds one stores the same value)
}

__global__ __launch_bounds__(VS_PLAN_TPB) void vs_plan_kernel(VsJob j) {
    __shared__ u64 s_pd[VS_MAXG + 7];
    __shared__ int s_red[VS_PLAN_TPB / 64];
    const u64 i = blockIdx.x;
    if (j.flag[i] != VS_F_FIRST) return;
    const nrg_vspace_op o = vs_load(j, i);
    const u32 k = (u32)(o.vbase >> 30);
    const u32 tabA = vs_pd_table(j.pool, k), tabB = vs_pd_table(j.pool, k + 1);
    vs_load_pd(j.pool, o, tabA, tabB, s_pd);
    const VsOut w = vs_walk<false>(j.pool, j.cap, o, s_pd, s_red, tabA, tabB, 0);
    if (threadIdx.x == 0) {
        j.npt[i] = w.npt;
        j.key[i] = k | (w.reach2 ? 1u << 31 : 0);
    }
}

// an exclusive scan of v over the workgroup's lanes; *total: the sum
__device__ __forceinline__ u32 vs_block_scan(u32 v, u32* s_scan, u32* total) {
    const u32 t = threadIdx.x;
    __syncthreads();
    s_scan[t] = v;
    __syncthreads();
    for (u32 s = 1; s < blockDim.x; s <<= 1) {
        const u32 o = t >= s ? s_scan[t - s] : 0;
        __syncthreads();
        s_scan[t] += o;
        __syncthreads();
    }
    *total = s_scan[blockDim.x - 1];
    return s_scan[t] - v;
}

__global__ __launch_bounds__(VS_ALLOC_TPB) void vs_alloc_kernel(VsJob j) {
    __shared__ u64 s_pml4[512];          // the PML4, with this chunk's new PDPTs
    __shared__ u64 s_need4[8];           // PML4 slots that get a PDPT
    __shared__ u64 s_needpd[VS_PDS / 64];  // page directories that get created
    __shared__ u32 s_scan[VS_ALLOC_TPB];
    const u32 t = threadIdx.x;
    if (t < 512) s_pml4[t] = j.pool[t];
    if (t < 8) s_need4[t] = 0;
    for (u32 w = t; w < VS_PDS / 64; w += VS_ALLOC_TPB) s_needpd[w] = 0;
    __syncthreads();
    for (u64 i = t; i < j.n; i += VS_ALLOC_TPB) {
        if (j.flag[i] != VS_F_FIRST) continue;
        const u32 key = j.key[i], k0 = key & (VS_PDS - 1);
        for (u32 q = 0; q <= (key >> 31); q++) {
            const u32 k = k0 + q;
            const u64 e = s_pml4[k >> 9];
            if (!(e & VS_P)) {
                atomicOr((unsigned long long*)&s_need4[k >> 15], 1ull << ((k >> 9) & 63));
                atomicOr((unsigned long long*)&s_needpd[k >> 6], 1ull << (k & 63));
            } else if (!(j.pool[((e & VS_ADDR) >> 12) * 512 + (k & 511)] & VS_P)) {
                atomicOr((unsigned long long*)&s_needpd[k >> 6], 1ull << (k & 63));
            }
        }
    }
    __syncthreads();
    // count: new PDPTs, new PDs (four bitmap words per lane), the ops' PTs (consecutive ops per lane)
    u32 n4 = 0;
    for (int w = 0; w < 8; w++) n4 += (u32)__popcll(s_need4[w]);
    u32 mypd = 0;
    for (u32 w = 4 * t; w < 4 * t + 4; w++) mypd += (u32)__popcll(s_needpd[w]);
    u32 npd = 0;
    const u32 pd_ex = vs_block_scan(mypd, s_scan, &npd);
    const u32 per = (u32)((j.n + VS_ALLOC_TPB - 1) / VS_ALLOC_TPB);
    const u64 i0 = (u64)t * per < j.n ? (u64)t * per : j.n;
    const u64 i1 = i0 + per < j.n ? i0 + per : j.n;
    u32 mypt = 0, mylater = 0;
    for (u64 i = i0; i < i1; i++) {
        mypt += j.npt[i];
        // an op can create no more than a PT per granule and four inner tables
        if (j.flag[i] == VS_F_LATER) mylater += j.ghi[i] - j.glo[i] + 1 + 4;
    }
    u32 npt = 0, nlater = 0;
    const u32 pt_ex = vs_block_scan(mypt, s_scan, &npt);
    (void)vs_block_scan(mylater, s_scan, &nlater);
    const u64 nt = j.st->ntables;
    const u64 inner_end = nt + n4 + npd;
    if (inner_end + npt + nlater > j.cap) {
        // The pool might not hold the chunk's tables: the first wave's, plus the most the other
        // ops can create. Applying the first wave ahead of the others could then give an op tables
        // that log order gives to an earlier one. Nothing is assigned here: the first wave's ops
        // join the others and the whole chunk replays one by one in log order (vs_seq_kernel),
        // where each op that does not fit is left out on its own and ERR_CAPACITY is latched. So
        // the pool only ever runs out in a chunk that replays sequentially, and the state after it
        // is the sequential one however the log was cut into chunks.
        for (u64 i = i0; i < i1; i++)
            if (j.flag[i] == VS_F_FIRST) j.flag[i] = VS_F_LATER;
        return;
    }
    if (t < 512 && (s_need4[t >> 6] >> (t & 63) & 1)) {
        u32 rank = (u32)__popcll(s_need4[t >> 6] & ((1ull << (t & 63)) - 1));
        for (u32 w = 0; w < (t >> 6); w++) rank += (u32)__popcll(s_need4[w]);
        s_pml4[t] = ((nt + rank) << 12) | VS_INNER;  // new_pdpt (:416-419)
        j.pool[t] = s_pml4[t];
    }
    __syncthreads();
    u32 rank = pd_ex;
    for (u32 w = 4 * t; w < 4 * t + 4; w++) {
        u64 m = s_needpd[w];
        while (m) {
            const u32 k = w * 64 + (u32)__builtin_ctzll(m);
            m &= m - 1;
            const u64 pdpt = (s_pml4[k >> 9] & VS_ADDR) >> 12;
            j.pool[pdpt * 512 + (k & 511)] = ((nt + n4 + rank) << 12) | VS_INNER;  // new_pd (:411-414)
            rank++;
        }
    }
    u32 run = pt_ex;
    for (u64 i = i0; i < i1; i++) {
        j.ptbase[i] = (u32)inner_end + run;
        run += j.npt[i];
    }
    if (t == 0) j.st->ntables = inner_end + npt;
}

__global__ __launch_bounds__(VS_TPB) void vs_apply_kernel(VsJob j) {
    __shared__ u64 s_pd[VS_MAXG + 7];
    __shared__ int s_red[VS_TPB / 64];
    const u64 i = blockIdx.x;
    if (j.flag[i] != VS_F_FIRST) return;
    const nrg_vspace_op o = vs_load(j, i);
    const u32 k = (u32)(o.vbase >> 30);
    const u32 tabA = vs_pd_table(j.pool, k), tabB = vs_pd_table(j.pool, k + 1);
    vs_load_pd(j.pool, o, tabA, tabB, s_pd);
    const VsOut w = vs_walk<true>(j.pool, j.cap, o, s_pd, s_red, tabA, tabB, j.ptbase[i]);
    vs_respond(j, i, o, w);
}

// lane 0: create what is missing on the way to page directory k, numbering from *next
__device__ __forceinline__ void vs_ensure_pd(u64* pool, u32 k, u64* next) {
    u64 e = ld_relaxed(pool + (k >> 9));
    if (!(e & VS_P)) {
        e = ((*next)++ << 12) | VS_INNER;
        pool[k >> 9] = e;
    }
    u64* slot = pool + ((e & VS_ADDR) >> 12) * 512 + (k & 511);
    if (!(ld_relaxed(slot) & VS_P)) *slot = ((*next)++ << 12) | VS_INNER;
}

// the ops [s0, s1) of the chunk that replay in log order
__global__ __launch_bounds__(VS_SEQ_TPB) void vs_seq_kernel(VsJob j, u64 s0, u64 s1) {
    __shared__ u64 s_pd[VS_MAXG + 7];
    __shared__ int s_red[VS_SEQ_TPB / 64];
    __shared__ u64 s_later[VS_SEQ_TPB / 64];  // the ops of this stretch that replay here, a bit each
    const u32 t = threadIdx.x;
    u64 nt = j.st->ntables;  // the same in every lane throughout
    bool full = false;
    for (u64 base = s0; base < s1; base += VS_SEQ_TPB) {
        const u64 mine = __ballot(base + t < s1 && j.flag[base + t] == VS_F_LATER);
        __syncthreads();
        if ((t & 63) == 0) s_later[t >> 6] = mine;
        __syncthreads();
        for (u32 wv = 0; wv < VS_SEQ_TPB / 64; wv++)
          for (u64 m = s_later[wv]; m; m &= m - 1) {
            const u64 i = base + wv * 64 + (u32)__builtin_ctzll(m);
            const nrg_vspace_op o = vs_load(j, i);
            const u32 k = (u32)(o.vbase >> 30);
            u32 tabA = vs_pd_table(j.pool, k), tabB = vs_pd_table(j.pool, k + 1);
            vs_load_pd(j.pool, o, tabA, tabB, s_pd);
            VsOut w = vs_walk<false>(j.pool, j.cap, o, s_pd, s_red, tabA, tabB, 0);
            u32 inner = vs_inner_need(j.pool, k);
            if (w.reach2) {
                if (((k + 1) >> 9) == (k >> 9))  // the same PDPT, which exists by then
                    inner += inner == 2 ? 1 : (vs_inner_need(j.pool, k + 1) ? 1 : 0);
                else
                    inner += vs_inner_need(j.pool, k + 1);
            }
            __syncthreads();  // every lane has read the inner entries before lane 0 creates any
            if (nt + inner + w.npt > j.cap) {  // the pool cannot hold the op's tables: nothing of it is applied
                full = true;
                if (t == 0) vs_answer(j, i, false, o.vbase, 0);
                continue;
            }
            if (inner) {
                if (t == 0) {
                    u64 next = nt;
                    vs_ensure_pd(j.pool, k, &next);
                    if (w.reach2) vs_ensure_pd(j.pool, k + 1, &next);
                }
                __threadfence();
                __syncthreads();
                tabA = vs_pd_table(j.pool, k);
                tabB = vs_pd_table(j.pool, k + 1);
            }
            w = vs_walk<true>(j.pool, j.cap, o, s_pd, s_red, tabA, tabB, (u32)(nt + inner));
            nt += inner + w.npt;
            vs_respond(j, i, o, w);
            __threadfence();  // the next op reads what this one stored
            __syncthreads();
        }
    }
    if (t == 0) {
        j.st->ntables = nt;
        if (full) atomicOr(&j.ctl->err, ERR_CAPACITY);
    }
}

// resolve_addr (:436-467) per address: the leaf's address plus the page offset, found = 0 and 0
// where nothing is mapped; VA bits 48..63 are ignored, as the index functions ignore them
__global__ __launch_bounds__(256) void vs_resolve_kernel(const u64* pool, const u64* va, u64 n, u64* pa,
                                                         uint8_t* found) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 a = va[i];
    u64 out = 0;
    uint8_t ok = 0;
    u64 e = pool[(a >> 39) & 511];
    if (e & VS_P) {
        e = pool[((e & VS_ADDR) >> 12) * 512 + ((a >> 30) & 511)];
        if (e & VS_P) {
            e = pool[((e & VS_ADDR) >> 12) * 512 + ((a >> 21) & 511)];
            if (e & VS_P) {
                if (e & VS_PS) {
                    out = (e & VS_ADDR) + (a & (VS_2M - 1));
                    ok = 1;
                } else {
                    e = pool[((e & VS_ADDR) >> 12) * 512 + ((a >> 12) & 511)];
                    if (e & VS_P) {
                        out = (e & VS_ADDR) + (a & 4095);
                        ok = 1;
                    }
                }
            }
        }
    }
    pa[i] = out;
    found[i] = ok;
}

// scratch of one chunk: five u32 and one u8 per op
static u64 vs_aux_bytes(u64 mb) { return mb * (5 * sizeof(u32) + 1); }

static hipError_t vs_replay_chunk(nrg_ctx* c, const void* src, u64 lo, u64 n, u64 resp_lo, u64 resp_hi, void* d_resp,
                                  uint8_t* d_some) {
    if (n == 0) return hipSuccess;
    const u64 mb = c->cfg.max_batch;
    VsJob j{};
    j.src = (const nrg_vspace_op*)src;
    j.ring = (nrg_vspace_op*)c->d_ring;
    j.ring_mask = c->log_size - 1;
    j.lo = lo;
    j.n = n;
    const bool want = d_resp != nullptr && d_some != nullptr && resp_lo < resp_hi && resp_lo < lo + n && resp_hi > lo;
    j.rlo = want ? resp_lo : 0;
    j.rhi = want ? resp_hi : 0;
    j.resp = want ? (nrg_vspace_resp*)d_resp : nullptr;
    j.some = want ? d_some : nullptr;
    j.pool = c->vs.d_pool;
    j.cap = c->vs.cap;
    j.st = c->vs.d_state;
    j.ctl = c->d_ctl;
    j.glo = (u32*)c->vs.d_aux;
    j.ghi = j.glo + mb;
    j.npt = j.ghi + mb;
    j.key = j.npt + mb;
    j.ptbase = j.key + mb;
    j.flag = (uint8_t*)(j.ptbase + mb);
    const unsigned tiles = (unsigned)((n + VS_TPB - 1) / VS_TPB);
    NRG_LAUNCH(c, "vs_prep", vs_prep_kernel, tiles, VS_TPB, 0, c->stream, j);
    NRG_LAUNCH(c, "vs_dep", vs_dep_kernel, dim3(tiles, tiles), VS_TPB, 0, c->stream, j);
    NRG_LAUNCH(c, "vs_plan", vs_plan_kernel, (unsigned)n, VS_PLAN_TPB, 0, c->stream, j);
    NRG_LAUNCH(c, "vs_alloc", vs_alloc_kernel, 1, VS_ALLOC_TPB, 0, c->stream, j);
    NRG_LAUNCH(c, "vs_apply", vs_apply_kernel, (unsigned)n, VS_TPB, 0, c->stream, j);
    // a launch per VS_SEQ_SLICE ops of the chunk bounds how long one kernel can run when many ops
    // depend on each other; the table count carries over in VsState
    for (u64 s0 = 0; s0 < n; s0 += VS_SEQ_SLICE)
        NRG_LAUNCH(c, "vs_seq", vs_seq_kernel, 1, VS_SEQ_TPB, 0, c->stream, j, s0,
                   s0 + VS_SEQ_SLICE < n ? s0 + VS_SEQ_SLICE : n);
    return hipGetLastError();
}

static hipError_t vs_resolve(nrg_ctx* c, const u64* d_va, u64 n, u64* d_pa, uint8_t* d_found) {
    if (n == 0) return hipSuccess;
    NRG_LAUNCH(c, "vs_resolve", vs_resolve_kernel, (unsigned)((n + 255) / 256), 256, 0, c->stream,
               (const u64*)c->vs.d_pool, d_va, n, d_pa, d_found);
    return hipGetLastError();
}

static int vs_open(nrg_ctx* c) {
    const nrg_config& cf = c->cfg;
    // log2_slots: the pool holds 2^log2_slots tables; max_batch <= 2^16: one workgroup scans a chunk
    if (cf.log2_slots < 2 || cf.log2_slots > 22 || cf.max_batch > (1ull << 16)) return NRG_E_INVAL;
    c->vs.cap = 1ull << cf.log2_slots;
    HIPCHK(hipMalloc(&c->vs.d_pool, c->vs.cap * 4096));
    HIPCHK(hipMemsetAsync(c->vs.d_pool, 0, c->vs.cap * 4096, c->stream));
    HIPCHK(hipMalloc(&c->vs.d_state, sizeof(VsState)));
    const VsState s0{1};  // table 0, the PML4 (VSpace::default, :165-174)
    HIPCHK(hipMemcpyAsync(c->vs.d_state, &s0, sizeof(s0), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));  // (s0 is on this frame)
    HIPCHK(hipMalloc(&c->vs.d_aux, vs_aux_bytes(cf.max_batch)));
    c->pipeline = false;  // config.pipeline is accepted: nothing is deferred
    return NRG_OK;
}

static void vs_close(nrg_ctx* c) {
    (void)hipFree(c->vs.d_pool);
    (void)hipFree(c->vs.d_state);
    (void)hipFree(c->vs.d_aux);
    (void)hipFree(c->vs.d_tag);
}

// ---- nrg_digest: {count, sum, xor} of dg_item(leaf's first vaddr, leaf entry) over the leaves ----
// A pool table knows neither its level nor the addresses it maps, so the digest goes top-down, a
// launch per level, none of which waits on another workgroup. tag[t] = base vaddr of table t |
// (level + 1), level 3 = PML4 .. 0 = PT; the low 12 bits of a base are free and 0 = never reached.
// Tables are never freed or moved and never change level, so a tag an earlier digest wrote is
// still right and a pass that writes it again stores the same value.
//   level 3   one workgroup: the PML4 tags its PDPTs and zeroes the output
//   level 2   the tables tagged as PDPTs tag their PDs
//   level 1   the tables tagged as PDs hash their 2 MiB leaves and tag their PTs
//   level 0   the tables tagged as PTs hash their leaves
// Levels 2..0 grid-stride over the tables [1, ntables) with ntables read on the device, a wave per
// table: four 16-B loads per lane, each instruction 1 KiB contiguous. A table is read by the pass of
// its level alone, so a digest reads every allocated table once: ntables * 4 KiB, plus 8 B of tag
// per table in each of the three passes. A child index >= ntables is skipped, as vs_collect skips it.
constexpr u32 VS_DG_MAX_GRID = 2048;

template <int LEVEL>
__device__ __forceinline__ void vs_digest_entry(u64 e, u64 base, u32 idx, u64 ntab, u64* tag, u64& c, u64& sm,
                                                u64& x) {
    if (!(e & VS_P)) return;
    const u64 va = base | ((u64)idx << (12 + 9 * LEVEL));
    if (LEVEL == 0 || (LEVEL == 1 && (e & VS_PS))) {
        const u64 h = dg_item(va, e);
        c++;
        sm += h;
        x ^= h;
    } else {
        const u64 child = (e & VS_ADDR) >> 12;
        if (child != 0 && child < ntab) tag[child] = va | (u64)LEVEL;  // the child's level + 1
    }
}

template <int LEVEL>
__device__ __forceinline__ void vs_digest_table(const u64* __restrict__ tab, u64 base, u64 ntab, u64* tag, u64& c,
                                                u64& sm, u64& x) {
    const u32 lane = threadIdx.x & 63;
#pragma unroll
    for (u32 q = 0; q < 4; q++) {
        const u32 idx = q * 128 + lane * 2;
        const ulonglong2 e = *(const ulonglong2*)(tab + idx);
        vs_digest_entry<LEVEL>(e.x, base, idx, ntab, tag, c, sm, x);
        vs_digest_entry<LEVEL>(e.y, base, idx + 1, ntab, tag, c, sm, x);
    }
}

__global__ __launch_bounds__(DG_TPB) void vs_digest_root_kernel(const u64* __restrict__ pool, const VsState* st,
                                                                u64 cap, u64* tag, u64* out3) {
    const u64 ntab = st->ntables < cap ? st->ntables : cap;
    if (threadIdx.x < 3) out3[threadIdx.x] = 0;
    u64 c = 0, sm = 0, x = 0;  // (a PML4 slot is never a leaf)
    if (threadIdx.x < 64) vs_digest_table<3>(pool, 0, ntab, tag, c, sm, x);
}

template <int LEVEL>
__global__ __launch_bounds__(DG_TPB) void vs_digest_level_kernel(const u64* __restrict__ pool, const VsState* st,
                                                                 u64 cap, u64* tag, u64* out3) {
    const u64 ntab = st->ntables < cap ? st->ntables : cap;
    const u64 waves = (u64)gridDim.x * (DG_TPB / 64);
    u64 c = 0, sm = 0, x = 0;
    for (u64 t = 1 + blockIdx.x * (u64)(DG_TPB / 64) + (threadIdx.x >> 6); t < ntab; t += waves) {
        const u64 tg = tag[t];  // the same in every lane of the wave
        if ((tg & 4095) != (u64)LEVEL + 1) continue;
        vs_digest_table<LEVEL>(pool + t * 512, tg & ~4095ull, ntab, tag, c, sm, x);
    }
    if (LEVEL <= 1) dg_commit(c, sm, x, out3);
}

static hipError_t vs_digest(nrg_ctx* c, u64* d_out3) {
    hipError_t e;
    if (!c->vs.d_tag) {
        if ((e = hipMalloc(&c->vs.d_tag, c->vs.cap * sizeof(u64))) != hipSuccess) return e;
        if ((e = hipMemsetAsync(c->vs.d_tag, 0, c->vs.cap * sizeof(u64), c->stream)) != hipSuccess) return e;
    }
    const u64* pool = c->vs.d_pool;
    const VsState* st = c->vs.d_state;
    u64* tag = c->vs.d_tag;
    const u64 cap = c->vs.cap;
    const u64 g = (cap + DG_TPB / 64 - 1) / (DG_TPB / 64);
    const unsigned grid = g > VS_DG_MAX_GRID ? VS_DG_MAX_GRID : (unsigned)g;
    NRG_LAUNCH(c, "vs_digest", vs_digest_root_kernel, 1, DG_TPB, 0, c->stream, pool, st, cap, tag, d_out3);
    NRG_LAUNCH(c, "vs_digest", vs_digest_level_kernel<2>, grid, DG_TPB, 0, c->stream, pool, st, cap, tag, d_out3);
    NRG_LAUNCH(c, "vs_digest", vs_digest_level_kernel<1>, grid, DG_TPB, 0, c->stream, pool, st, cap, tag, d_out3);
    NRG_LAUNCH(c, "vs_digest", vs_digest_level_kernel<0>, grid, DG_TPB, 0, c->stream, pool, st, cap, tag, d_out3);
    return hipGetLastError();
}

static void vs_defaults(nrg_config* cfg) {
    cfg->log2_slots = 18;       // the pool: 2^18 tables of 4 KiB, 1 GiB
    cfg->max_batch = 1u << 16;  // the largest chunk a page table replays
}

// ---- nrg_snapshot_async / nrg_restore: the pool image [0, ntables) ---------------------------------
typedef u64 vs_u64x2 __attribute__((ext_vector_type(2)));  // 16 B moved by one lane

// The one reader of VsState (the snapshot's item count, nrg_vspace_tables and nrg_vspace_dump).
// Drains the stream.
static int vs_read_state(nrg_ctx* c, VsState* s) {
    HIPCHK(hipMemcpyAsync(s, c->vs.d_state, sizeof(*s), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return NRG_OK;
}

static int vs_items(nrg_ctx* c, u64* n) {
    VsState s{};
    int r = vs_read_state(c, &s);
    if (r) return r;
    *n = s.ntables < c->vs.cap ? s.ntables : c->vs.cap;
    return NRG_OK;
}

// ntables * 4 KiB as they are, inner entries included (table_index * 4096 | flags: the indices stay
// valid in any pool of at least ntables tables); ntables is read here. A lane moves 16 B, a wave
// 1 KiB contiguous. The image must fit whole or nothing of the payload is stored.
__global__ __launch_bounds__(DG_TPB) void vs_snapshot_kernel(const u64* __restrict__ pool, const VsState* st,
                                                             u64 tables, u64* buf, u64 cap, u64 log_idx, DevCtl* ctl) {
    const u64 ntab = st->ntables < tables ? st->ntables : tables;
    if (blockIdx.x == 0 && threadIdx.x == 0) snap_head(buf, cap, NRG_DS_VSPACE, ntab, ntab * 4096, log_idx, ctl);
    if (snap_bytes(ntab * 4096) > cap) return;
    const vs_u64x2* src = (const vs_u64x2*)pool;
    vs_u64x2* out = (vs_u64x2*)(buf + SNAP_HDR / 8);
    for (u64 i = blockIdx.x * (u64)DG_TPB + threadIdx.x; i < ntab * 256; i += (u64)gridDim.x * DG_TPB) out[i] = src[i];
}

static hipError_t vs_snapshot(nrg_ctx* c, void* d_buf, u64 cap, u64 log_idx) {
    const u64 g = c->vs.cap;  // a workgroup per table where the pool is small
    NRG_LAUNCH(c, "vs_snapshot", vs_snapshot_kernel, (unsigned)(g > VS_DG_MAX_GRID ? VS_DG_MAX_GRID : g), DG_TPB, 0,
               c->stream, (const u64*)c->vs.d_pool, (const VsState*)c->vs.d_state, (u64)c->vs.cap, (u64*)d_buf, cap,
               log_idx, c->d_ctl);
    return hipGetLastError();
}

// The tables [0, items) from the payload, the rest of the pool zeroed, and the table count ntab.
__global__ __launch_bounds__(DG_TPB) void vs_restore_kernel(u64* pool, const u64* __restrict__ payload, u64 items,
                                                            u64 tables, u64 ntab, VsState* st) {
    const vs_u64x2* src = (const vs_u64x2*)payload;
    vs_u64x2* dst = (vs_u64x2*)pool;
    for (u64 i = blockIdx.x * (u64)DG_TPB + threadIdx.x; i < tables * 256; i += (u64)gridDim.x * DG_TPB) {
        vs_u64x2 v = {0, 0};
        if (i < items * 256) v = src[i];
        dst[i] = v;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) st->ntables = ntab;
}

// The tags of an earlier digest describe tables that no longer exist (a table that was a PT may now
// be a PD, or unreachable): they are cleared, so the next digest tags from the PML4 down again.
// Without a payload: the PML4 alone, zeroed (VSpace::default).
static int vs_restore(nrg_ctx* c, const void* d_payload, u64 items, bool check_only) {
    if (check_only) return items == 0 ? NRG_E_INVAL : (items > c->vs.cap ? NRG_E_CAPACITY : NRG_OK);
    const u64 g = c->vs.cap;
    NRG_LAUNCH(c, "vs_restore", vs_restore_kernel, (unsigned)(g > VS_DG_MAX_GRID ? VS_DG_MAX_GRID : g), DG_TPB, 0,
               c->stream, c->vs.d_pool, (const u64*)d_payload, (u64)(d_payload ? items : 0), (u64)c->vs.cap,
               (u64)(d_payload ? items : 1), c->vs.d_state);
    HIPCHK(hipGetLastError());
    if (c->vs.d_tag) HIPCHK(hipMemsetAsync(c->vs.d_tag, 0, c->vs.cap * sizeof(u64), c->stream));
    return NRG_OK;
}

// ---- growth of the pool (VSpace takes its tables from the heap: benches/vspace.rs:388-419) --------
// The tables [0, ntables) into a larger pool and the rest of it zeroed, in one launch (the rest of
// the code relies on a zeroed pool); ntables is read here. Inner entries are table indices, so they
// stay valid. A lane moves 16 B, a wave 1 KiB contiguous.
__global__ __launch_bounds__(DG_TPB) void vs_grow_kernel(const u64* __restrict__ from, u64 from_tables, u64* to,
                                                         u64 to_tables, const VsState* st) {
    const u64 ntab = st->ntables < from_tables ? st->ntables : from_tables;
    const vs_u64x2* src = (const vs_u64x2*)from;
    vs_u64x2* dst = (vs_u64x2*)to;
    // (four zero stores in flight per lane and turn instead of one: 0.920 against 0.935 ms for the
    // 2^18 -> 2^20 pool of microbench/capacity_grow.py, so the loop stays vs_restore_kernel's)
    for (u64 i = blockIdx.x * (u64)DG_TPB + threadIdx.x; i < to_tables * 256; i += (u64)gridDim.x * DG_TPB) {
        vs_u64x2 v = {0, 0};
        if (i < ntab * 256) v = src[i];
        dst[i] = v;
    }
}

// The copy, then the stream is synchronised (there is no stream-ordered free), the old pool freed
// and the new one installed with the capacity every launch reads (vs.cap). The digest's tags are
// sized by the pool: they are dropped, and the next digest allocates them for the new pool and tags
// from the PML4 down again. If the allocation fails nothing has been launched: the replica is as it
// was.
static hipError_t vs_grow(nrg_ctx* c, u64 new_cap) {
    if (new_cap <= c->vs.cap || new_cap > (1ull << 22)) return hipErrorInvalidValue;
    u64* np = nullptr;
    if (hipMalloc(&np, new_cap * 4096) != hipSuccess) {
        (void)hipGetLastError();  // (the failure is reported by the return value alone)
        return hipErrorOutOfMemory;
    }
    NRG_LAUNCH(c, "vs_grow", vs_grow_kernel, (unsigned)(new_cap > VS_DG_MAX_GRID ? VS_DG_MAX_GRID : new_cap), DG_TPB, 0,
               c->stream, (const u64*)c->vs.d_pool, (u64)c->vs.cap, np, new_cap, (const VsState*)c->vs.d_state);
    hipError_t e = hipGetLastError();
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        (void)hipFree(np);
        return e;
    }
    (void)hipFree(c->vs.d_pool);
    (void)hipFree(c->vs.d_tag);
    c->vs.d_pool = np;
    c->vs.d_tag = nullptr;
    c->vs.cap = new_cap;
    return hipSuccess;
}

static u64 vs_capacity(const nrg_ctx* c) { return c->vs.cap; }

const DsOps* vs_ops() {  // (reserve only: the tables a chunk needs are known on the device alone)
    static const DsOps ops = {sizeof(nrg_vspace_op), sizeof(nrg_vspace_resp), vs_open, vs_close, nullptr,
                              vs_replay_chunk, floor_ltail, nullptr, nullptr, vs_defaults, vs_digest,
                              vs_items, vs_snapshot, vs_restore, 1ull << 22, vs_capacity, vs_grow, false};
    return &ops;
}

}  // namespace nrg

// ---- the page table's entry points (include/nrgpu.h) ------------------------------------------
using namespace nrg;

extern "C" {

int nrg_vspace_round_async(nrg_ctx* c, const nrg_vspace_op* d_ops, uint64_t n, uint32_t origin,
                           nrg_vspace_resp* d_resp, uint8_t* d_some) {
    return round_common(c, NRG_DS_VSPACE, d_ops, n, origin, d_resp, d_some);
}

int nrg_vspace_resolve_async(nrg_ctx* c, const uint64_t* d_vaddrs, uint64_t n, uint64_t* d_paddrs, uint8_t* d_found) {
    int r = need(c, NRG_DS_VSPACE);
    if (r) return r;
    if (c->ltail != c->tail) return NRG_E_NOT_SYNCED;
    if (n > c->cfg.max_reads) return NRG_E_CAPACITY;
    if (n && (!d_vaddrs || !d_paddrs || !d_found)) return NRG_E_INVAL;
    return hip_fail(vs_resolve(c, d_vaddrs, n, d_paddrs, d_found));
}

int nrg_vspace_resolve(nrg_ctx* c, const uint64_t* vaddrs, uint64_t n, uint64_t* paddrs, uint8_t* found) {
    int r = need(c, NRG_DS_VSPACE);
    if (r) return r;
    if (c->ltail != c->tail) return NRG_E_NOT_SYNCED;
    if (n > c->cfg.max_reads) return NRG_E_CAPACITY;
    if (n == 0) return NRG_OK;
    if (!vaddrs || !paddrs || !found) return NRG_E_INVAL;
    Staging* s = c->stg;
    if ((r = staging(s[0], n * 8)) || (r = staging(s[1], n * 8)) || (r = staging(s[2], n))) return r;
    HIPCHK(hipMemcpyAsync(s[0].p, vaddrs, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(vs_resolve(c, (u64*)s[0].p, n, (u64*)s[1].p, (uint8_t*)s[2].p));
    HIPCHK(hipMemcpyAsync(paddrs, s[1].p, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(found, s[2].p, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_all(c));
    return check_err(c);
}

// tables allocated from the pool
static int vs_get_tables(nrg_ctx* c, uint64_t* n) {
    VsState s{};
    int r = vs_read_state(c, &s);
    if (r) return r;
    *n = s.ntables;
    if (s.ntables > c->vs.cap) return NRG_E_HIP;  // (the allocation passes never hand out more than the pool holds)
    return check_err(c);
}

int nrg_vspace_tables(nrg_ctx* c, uint64_t* n) {
    int r = need(c, NRG_DS_VSPACE);
    if (r) return r;
    if (!n) return NRG_E_INVAL;
    return vs_get_tables(c, n);
}

int nrg_vspace_reserve(nrg_ctx* c, uint64_t n_tables) { return reserve_common(c, NRG_DS_VSPACE, n_tables); }

int nrg_vspace_capacity(nrg_ctx* c, uint64_t* n) { return capacity_common(c, NRG_DS_VSPACE, n); }

int nrg_test_vspace_table(nrg_ctx* c, uint64_t table, uint64_t out[512]) {
    int r = need(c, NRG_DS_VSPACE);
    if (r) return r;
    if (!out || table >= c->vs.cap) return NRG_E_INVAL;
    HIPCHK(hipMemcpyAsync(out, c->vs.d_pool + table * 512, 4096, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_all(c));
    return NRG_OK;
}

// The leaves below table `tab` of level `level` (3 = PML4 .. 0 = PT) in ascending vaddr: slots are
// walked in index order, so nothing depends on the order in which the tables were allocated.
static void vs_collect(const uint64_t* pool, uint64_t ntab, uint64_t tab, int level, uint64_t va,
                       std::vector<nrg_vspace_leaf>& out) {
    const uint64_t ADDR = 0x000ffffffffff000ull;
    for (uint64_t i = 0; i < 512; i++) {
        const uint64_t e = pool[tab * 512 + i];
        if (!(e & 1)) continue;
        const uint64_t v = va | (i << (12 + 9 * level));
        if (level == 0 || (level == 1 && (e & 0x80))) {
            out.push_back(nrg_vspace_leaf{v, e});
        } else {
            const uint64_t next = (e & ADDR) >> 12;
            if (next < ntab) vs_collect(pool, ntab, next, level - 1, v, out);
        }
    }
}

int nrg_vspace_dump(nrg_ctx* c, nrg_vspace_leaf* leaves, uint64_t cap, uint64_t* n) {
    int r = need(c, NRG_DS_VSPACE);
    if (r) return r;
    if (!n) return NRG_E_INVAL;
    uint64_t ntab = 0;
    if ((r = vs_get_tables(c, &ntab))) return r;
    // Replica::verify's view, not a hot path: the allocated tables are copied out and walked here
    std::vector<uint64_t> pool;
    std::vector<nrg_vspace_leaf> out;
    try {
        pool.resize(ntab * 512);
        HIPCHK(hipMemcpyAsync(pool.data(), c->vs.d_pool, ntab * 4096, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(sync_all(c));
        vs_collect(pool.data(), ntab, 0, 3, 0, out);
    } catch (const std::bad_alloc&) {
        return NRG_E_NOMEM;
    }
    *n = out.size();
    if (*n > cap) return NRG_E_CAPACITY;
    if (*n) {
        if (!leaves) return NRG_E_INVAL;
        std::memcpy(leaves, out.data(), *n * sizeof(nrg_vspace_leaf));
    }
    return NRG_OK;
}

}  // extern "C"
