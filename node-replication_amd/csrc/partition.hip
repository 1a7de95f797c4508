// partition.hip — cnr-style key partitioning of hashmap rounds across replicas.
//
// cnr (cnr/src/lib.rs:134-167) maps every operation to one of several logs with
// LogMapper::hash(); conflicting operations (the same key) share a log, so each log replays
// independently (cnr/src/replica.rs:430-445 hash -> log, :673-736 combine(hashidx)). Across GPUs
// the log of partition p lives on GPU p, which holds only the keys it owns: a round's Puts and
// Gets are routed to their owners, each owner replays the Puts it received in rank order (the
// global log order restricted to its keys, so every key sees its writes in the same order as an
// NR replay of W_0 || W_1 || ...), answers the Gets it received, and the answers travel back.
//
// Owner of a key: the low 32 bits of mix64(key) scaled to [0, parts). The table's home slot uses
// the top bits of the same mix (common.hpp table_home), so a partition's keys still spread over
// its whole table.
//
// Kernels (records of `words` u64 with the key in word 0: Puts 2, Get keys 1):
//   pt_count_kernel    per 2048-record tile: records per owner
//   pt_scan_kernel     per owner: exclusive scan of the tile counts, and the owner's total
//   pt_scatter_kernel  per tile: stable rank of each record among its owner's records of the
//                      tile (per wave, one ballot per distinct owner in a 64-record round; the
//                      per-owner counts of a wave live in lane `owner`), then out[dest] = record
//                      and pos[i] = dest, dest = owner start + tile offset + wave offset + rank
//   pt_gather_kernel   answers back to the caller's order: dst[i] = src[pos[i]]
// The file store's records are partitioned by FILE, not by key (benches/nrfs.rs: one log per file):
// fp_count_kernel / fp_scatter_kernel / fp_route_kernel further down, with pt_scan_kernel between them;
// the requests of a group-wide pread go the same way (rd_scatter_kernel).
#include "internal.hpp"

namespace nrg {

constexpr int PT_TPB = 256;
constexpr int PT_WAVES = PT_TPB / 64;
constexpr int PT_ROUNDS = 8;                             // 64-record rounds per wave
constexpr u32 PT_TILE = PT_TPB * PT_ROUNDS;              // 2048 records per tile

__global__ __launch_bounds__(PT_TPB) void pt_count_kernel(const u64* __restrict__ in, u64 n, u32 words, u32 parts,
                                                          u32* __restrict__ tcnt) {
    __shared__ u32 s_c[PT_MAX_PARTS];
    if (threadIdx.x < PT_MAX_PARTS) s_c[threadIdx.x] = 0;
    __syncthreads();
    const u64 t0 = (u64)blockIdx.x * PT_TILE;
    for (u32 k = threadIdx.x; k < PT_TILE; k += PT_TPB) {
        const u64 i = t0 + k;
        if (i < n) atomicAdd(&s_c[key_owner(in[i * words], parts)], 1u);
    }
    __syncthreads();
    if (threadIdx.x < parts) tcnt[(u64)blockIdx.x * parts + threadIdx.x] = s_c[threadIdx.x];
}

// one block per owner p: toff[t][p] = sum of tcnt[t'][p], t' < t; total[p]
__global__ __launch_bounds__(PT_TPB) void pt_scan_kernel(const u32* __restrict__ tcnt, u32 ntiles, u32 parts,
                                                         u32* __restrict__ toff, u64* __restrict__ total) {
    __shared__ u32 s_w[PT_WAVES];
    const u32 p = blockIdx.x;
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    const u32 K = (ntiles + PT_TPB - 1) / PT_TPB;  // tiles [t*K, t*K + K) per thread
    u32 loc = 0;
    for (u32 q = 0; q < K; q++) {
        const u32 tile = t * K + q;
        if (tile < ntiles) loc += tcnt[(u64)tile * parts + p];
    }
    u32 inc = loc;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u32 y = __shfl_up(inc, off, 64);
        if (lane >= off) inc += y;
    }
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    u32 run = inc - loc;
    for (int i = 0; i < w; i++) run += s_w[i];
    for (u32 q = 0; q < K; q++) {
        const u32 tile = t * K + q;
        if (tile < ntiles) {
            const u32 c = tcnt[(u64)tile * parts + p];
            toff[(u64)tile * parts + p] = run;
            run += c;
        }
    }
    if (t == PT_TPB - 1) {
        u32 all = 0;
        for (int i = 0; i < PT_WAVES; i++) all += s_w[i];
        total[p] = all;
    }
}

__global__ __launch_bounds__(PT_TPB) void pt_scatter_kernel(const u64* __restrict__ in, u64 n, u32 words, u32 parts,
                                                            const u32* __restrict__ toff, const u64* __restrict__ total,
                                                            u64* __restrict__ out, u32* __restrict__ pos) {
    __shared__ u32 s_base[PT_MAX_PARTS];          // owner start: exclusive prefix of the totals
    __shared__ u32 s_wc[PT_WAVES][PT_MAX_PARTS];  // per wave counts, then wave offsets
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    if (t == 0) {
        u32 acc = 0;
        for (u32 p = 0; p < parts; p++) {
            s_base[p] = acc;
            acc += (u32)total[p];
        }
    }
    const u64 t0 = (u64)blockIdx.x * PT_TILE + (u64)w * (PT_ROUNDS * 64);
    u32 own[PT_ROUNDS], rank[PT_ROUNDS];
    u32 cnt = 0;  // lane p: this wave's records of owner p so far
#pragma unroll
    for (int r = 0; r < PT_ROUNDS; r++) {
        const u64 i = t0 + (u64)r * 64 + lane;
        const bool valid = i < n;
        const u32 o = valid ? key_owner(in[i * words], parts) : 0u;
        own[r] = o;
        rank[r] = 0;
        u64 act = __ballot(valid);
        while (act) {  // one ballot per distinct owner among the 64 records (wave-uniform loop)
            const int leader = __ffsll((long long)act) - 1;
            const u32 ol = (u32)__shfl((int)o, leader, 64);
            const u64 m = __ballot(valid && o == ol);
            const u32 c0 = (u32)__shfl((int)cnt, (int)ol, 64);
            if (valid && o == ol) rank[r] = c0 + (u32)__popcll(m & ((1ull << lane) - 1));
            if ((u32)lane == ol) cnt += (u32)__popcll(m);
            act &= ~m;
        }
    }
    if ((u32)lane < parts) s_wc[w][lane] = cnt;
    __syncthreads();
    if (t < (int)parts) {
        u32 acc = 0;
        for (int i = 0; i < PT_WAVES; i++) {
            const u32 c = s_wc[i][t];
            s_wc[i][t] = acc;
            acc += c;
        }
    }
    __syncthreads();
    const u32* to = toff + (u64)blockIdx.x * parts;
#pragma unroll
    for (int r = 0; r < PT_ROUNDS; r++) {
        const u64 i = t0 + (u64)r * 64 + lane;
        if (i >= n) continue;
        const u32 o = own[r];
        const u32 dest = s_base[o] + to[o] + s_wc[w][o] + rank[r];
        for (u32 k = 0; k < words; k++) out[(u64)dest * words + k] = in[i * words + k];
        pos[i] = dest;
    }
}

__global__ __launch_bounds__(PT_TPB) void pt_gather_kernel(const u64* __restrict__ src, const uint8_t* __restrict__ src8,
                                                           const u32* __restrict__ pos, u64 n, u64* __restrict__ dst,
                                                           uint8_t* __restrict__ dst8) {
    for (u64 i = blockIdx.x * (u64)PT_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * PT_TPB) {
        const u32 p = pos[i];
        if (dst) dst[i] = src[p];
        if (dst8) dst8[i] = src8[p];
    }
}

// ---- the replica group's fused partition (nrg_group_partitioned_round) -----------------------
// One launch partitions a round's Puts and Get keys together, in one pass: owner o's records go to
// a region of fixed capacity (out + o * cap, cap = the job's own record count, so any owner can
// take all of them), so no global scan of the owner totals is needed. Tiles are blockIdx-ordered
// (Puts first, then Gets); each publishes its per-owner counts as a look-back descriptor and takes
// its offsets from its predecessors' (decoupled look-back, relaxed agent-scope atomics; the
// descriptor word IS the flag, epoch-tagged so no reset pass runs between rounds). The last tile
// of a job writes the owner totals into the round's count-exchange words, and block 0 the
// member's host words (XW_*), so the exchange needs no host copy.
typedef u64 pt_u64x2 __attribute__((ext_vector_type(2)));
constexpr u64 PD_CNT = (1ull << 40) - 1, PD_AGG = 1ull << 40, PD_INC = 2ull << 40, PD_ST = 3ull << 40;
constexpr int PD_EP = 42, PD_WIN = 16;
// fused tiles: 16 waves x 8 rounds of 64 = 8192 records, so a 1M-op round has ~123 tiles and the
// look-back reaches an inclusive descriptor in a few windowed steps (2048-record tiles: 22 us per
// B1 round, the look-back chain of ~490 tiles)
constexpr int PF_TPB = 1024, PF_WAVES = PF_TPB / 64;
constexpr u32 PF_TILE = PF_TPB * PT_ROUNDS;

struct PtFJob {
    const u64* in;
    u64 n;
    u64 cap;      // owner o's records at out[(o * cap + j) * words]
    u64* out;
    u32* pos;     // pos[i] = o * cap + j: where record i went
    u64* desc;    // [tiles][parts] look-back descriptors
    u64* counts;  // [parts] the job's records per owner
    u32 tiles;
};
struct PtFWords {
    u64 w[PT_XW_MAX];
    u64* dst;
    u32 n;
};

template <int WORDS>
__device__ __forceinline__ void ptf_tile(const PtFJob& J, u32 tile, u32 parts, u64 ep, u32* s_wc_flat, u64* s_base) {
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    u32(*s_wc)[PT_MAX_PARTS] = (u32(*)[PT_MAX_PARTS])s_wc_flat;
    const u64 t0 = (u64)tile * PF_TILE + (u64)w * (PT_ROUNDS * 64);
    u64 rec[PT_ROUNDS][WORDS];
#pragma unroll
    for (int r = 0; r < PT_ROUNDS; r++) {
        const u64 i = t0 + (u64)r * 64 + lane;
        if (i < J.n) {
            if constexpr (WORDS == 2) {
                const pt_u64x2 v = ((const pt_u64x2*)J.in)[i];
                rec[r][0] = v.x;
                rec[r][1] = v.y;
            } else {
                rec[r][0] = J.in[i];
            }
        } else {
#pragma unroll
            for (int k = 0; k < WORDS; k++) rec[r][k] = 0;
        }
    }
    u32 own[PT_ROUNDS], rank[PT_ROUNDS];
    u32 cnt = 0;  // lane p: this wave's records of owner p so far
#pragma unroll
    for (int r = 0; r < PT_ROUNDS; r++) {
        const u64 i = t0 + (u64)r * 64 + lane;
        const bool valid = i < J.n;
        const u32 o = valid ? key_owner(rec[r][0], parts) : 0u;
        own[r] = o;
        rank[r] = 0;
        u64 act = __ballot(valid);
        while (act) {  // one ballot per distinct owner among the 64 records (wave-uniform loop)
            const int leader = __ffsll((long long)act) - 1;
            const u32 ol = (u32)__shfl((int)o, leader, 64);
            const u64 m = __ballot(valid && o == ol);
            const u32 c0 = (u32)__shfl((int)cnt, (int)ol, 64);
            if (valid && o == ol) rank[r] = c0 + (u32)__popcll(m & ((1ull << lane) - 1));
            if ((u32)lane == ol) cnt += (u32)__popcll(m);
            act &= ~m;
        }
    }
    if ((u32)lane < parts) s_wc[w][lane] = cnt;
    __syncthreads();
    if (t < (int)parts) {  // wave 0, lane = owner: tile count, wave offsets, look-back
        u32 tc = 0;
        for (int i = 0; i < PF_WAVES; i++) {
            const u32 c = s_wc[i][t];
            s_wc[i][t] = tc;
            tc += c;
        }
        u64* my = J.desc + (u64)tile * parts + t;
        __hip_atomic_store(my, ep | (tile == 0 ? PD_INC : PD_AGG) | tc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        u64 excl = 0;
        if (tile > 0) {
            // windowed: PD_WIN predecessor descriptors in flight per step, consumed newest-first
            // until an inclusive one (radix_sort.hip's look-back; stale epochs read as unpublished)
            int tt = (int)tile - 1;
            for (;;) {
                u64 v[PD_WIN];
#pragma unroll
                for (int q = 0; q < PD_WIN; q++)
                    v[q] = tt - q >= 0 ? __hip_atomic_load(J.desc + (u64)(tt - q) * parts + t, __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_AGENT)
                                       : (ep | PD_INC);
                int used = 0;
                bool done = false;
#pragma unroll
                for (int q = 0; q < PD_WIN; q++) {
                    if (done || used < q) continue;
                    const u64 st = (v[q] >> PD_EP) == (ep >> PD_EP) ? (v[q] & PD_ST) : 0ull;
                    if (st == 0) continue;  // not published yet: retry from here
                    excl += v[q] & PD_CNT;
                    used = q + 1;
                    if (st == PD_INC) done = true;
                }
                if (done) break;
                tt -= used;
                if (used < PD_WIN) __builtin_amdgcn_s_sleep(1);
            }
            __hip_atomic_store(my, ep | PD_INC | (excl + tc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        s_base[t] = (u64)t * J.cap + excl;
        if (tile + 1 == J.tiles) J.counts[t] = excl + tc;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < PT_ROUNDS; r++) {
        const u64 i = t0 + (u64)r * 64 + lane;
        if (i >= J.n) continue;
        const u32 o = own[r];
        const u64 dest = s_base[o] + s_wc[w][o] + rank[r];
        if constexpr (WORDS == 2) {
            pt_u64x2 v;
            v.x = rec[r][0];
            v.y = rec[r][1];
            ((pt_u64x2*)J.out)[dest] = v;
        } else {
            J.out[dest] = rec[r][0];
        }
        J.pos[i] = (u32)dest;
    }
}

__global__ __launch_bounds__(PF_TPB) void pt_fused_kernel(PtFJob P, PtFJob K, u32 parts, u64 ep, PtFWords xw) {
    __shared__ u32 s_wc[PF_WAVES * PT_MAX_PARTS];
    __shared__ u64 s_base[PT_MAX_PARTS];
    const u32 b = blockIdx.x;
    if (b == 0) {
        if (threadIdx.x == 0) {  // (constant indices: a lane-indexed argument array goes to scratch)
#pragma unroll
            for (u32 k = 0; k < PT_XW_MAX; k++)
                if (k < xw.n) xw.dst[k] = xw.w[k];
        }
        if (threadIdx.x < parts) {  // a job without tiles has no owner records
            if (P.tiles == 0) P.counts[threadIdx.x] = 0;
            if (K.tiles == 0) K.counts[threadIdx.x] = 0;
        }
    }
    if (b < P.tiles) ptf_tile<2>(P, b, parts, ep, s_wc, s_base);
    else if (b - P.tiles < K.tiles) ptf_tile<1>(K, b - P.tiles, parts, ep, s_wc, s_base);
}

struct PtRoute {
    const u64* src;
    const uint8_t* src8;
    const u32* pos;
    u64 n;
    u64* dst;
    uint8_t* dst8;
};
// answers back to the caller's order, both routes of a round in one launch: dst[i] = src[pos[i]]
__global__ __launch_bounds__(PT_TPB) void pt_route2_kernel(PtRoute a, PtRoute b) {
    const u64 N = a.n + b.n;
    for (u64 i = blockIdx.x * (u64)PT_TPB + threadIdx.x; i < N; i += (u64)gridDim.x * PT_TPB) {
        const bool first = i < a.n;
        const PtRoute& r = first ? a : b;
        const u64 j = first ? i : i - a.n;
        const u32 p = r.pos[j];
        if (r.dst) r.dst[j] = r.src[p];
        if (r.dst8) r.dst8[j] = r.src8[p];
    }
}

// One owner: the stable partition is the identity (out = in, pos[i] = i, counts = n), a copy at
// streaming rate instead of a look-back over 8192-record tiles (a one-rank group: 28 -> ~5 us).
__global__ __launch_bounds__(PT_TPB) void pt_copy1_kernel(const u64* __restrict__ puts, u64 W, u64* __restrict__ pout,
                                                          u32* __restrict__ ppos, const u64* __restrict__ keys, u64 R,
                                                          u64* __restrict__ kout, u32* __restrict__ gpos, u64* counts,
                                                          PtFWords xw) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        counts[0] = W;
        counts[1] = R;
#pragma unroll
        for (u32 k = 0; k < PT_XW_MAX; k++)
            if (k < xw.n) xw.dst[k] = xw.w[k];
    }
    const u64 stride = (u64)gridDim.x * PT_TPB;
    for (u64 i = blockIdx.x * (u64)PT_TPB + threadIdx.x; i < W + R; i += stride) {
        if (i < W) {
            ((pt_u64x2*)pout)[i] = ((const pt_u64x2*)puts)[i];
            ppos[i] = (u32)i;
        } else {
            const u64 j = i - W;
            kout[j] = keys[j];
            gpos[j] = (u32)j;
        }
    }
}

hipError_t pt_fused(hipStream_t s, const u64* puts, u64 W, u64 cap_p, u64* pout, u32* ppos, const u64* keys, u64 R,
                    u64 cap_k, u64* kout, u32* gpos, u64* desc, u32 parts, u32 epoch, u64* counts, const u64* xw,
                    u32 nxw) {
    if (parts == 0 || parts > PT_MAX_PARTS || nxw > PT_XW_MAX) return hipErrorInvalidValue;
    if (W && (W > cap_p || (u64)parts * cap_p > 0xFFFFFFFFull)) return hipErrorInvalidValue;
    if (R && (R > cap_k || (u64)parts * cap_k > 0xFFFFFFFFull)) return hipErrorInvalidValue;
    PtFJob P{(const u64*)puts, W, cap_p, pout, ppos, desc, counts, (u32)((W + PF_TILE - 1) / PF_TILE)};
    PtFJob K{keys, R, cap_k, kout, gpos, desc + (u64)P.tiles * parts, counts + parts,
             (u32)((R + PF_TILE - 1) / PF_TILE)};
    PtFWords x{};
    for (u32 k = 0; k < nxw; k++) x.w[k] = xw[k];
    x.dst = counts + 2 * parts;
    x.n = nxw;
    if (parts == 1) {
        const u64 nb = (W + R + PT_TPB - 1) / PT_TPB;
        pt_copy1_kernel<<<(unsigned)(nb < 2048 ? (nb ? nb : 1) : 2048), PT_TPB, 0, s>>>(puts, W, pout, ppos, keys, R, kout,
                                                                                     gpos, counts, x);
        return hipGetLastError();
    }
    const u32 blocks = P.tiles + K.tiles;
    pt_fused_kernel<<<blocks ? blocks : 1u, PF_TPB, 0, s>>>(P, K, parts, (u64)(epoch & ((1u << 22) - 1)) << PD_EP, x);
    return hipGetLastError();
}

hipError_t pt_route2(hipStream_t s, const u64* src_a, const uint8_t* src8_a, const u32* pos_a, u64 n_a, u64* dst_a,
                     uint8_t* dst8_a, const u64* src_b, const uint8_t* src8_b, const u32* pos_b, u64 n_b, u64* dst_b,
                     uint8_t* dst8_b) {
    const u64 n = n_a + n_b;
    if (n == 0) return hipSuccess;
    const u64 blocks = (n + PT_TPB - 1) / PT_TPB;
    pt_route2_kernel<<<(unsigned)(blocks < 4096 ? blocks : 4096), PT_TPB, 0, s>>>(
        PtRoute{src_a, src8_a, pos_a, n_a, dst_a, dst8_a}, PtRoute{src_b, src8_b, pos_b, n_b, dst_b, dst8_b});
    return hipGetLastError();
}

u64 pt_desc_words(u64 W, u64 R, u32 parts) {
    return ((W + PF_TILE - 1) / PF_TILE + (R + PF_TILE - 1) / PF_TILE) * parts;
}

// Scratch for the tile counts and offsets, grown on demand (the replica's stream is drained
// before a reallocation).
static hipError_t pt_scratch(nrg_ctx* c, u64 words) {
    if (c->pt.words >= words) return hipSuccess;
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return e;
    if (c->pt.d_buf) (void)hipFree(c->pt.d_buf);
    c->pt.d_buf = nullptr;
    c->pt.words = 0;
    if ((e = hipMalloc(&c->pt.d_buf, words * sizeof(u32))) != hipSuccess) return e;
    c->pt.words = words;
    return hipSuccess;
}

void pt_close(nrg_ctx* c) {
    if (c->pt.d_buf) (void)hipFree(c->pt.d_buf);
    c->pt.d_buf = nullptr;
    c->pt.words = 0;
}

// stable partition of records (key in word 0) by key owner
static hipError_t pt_partition(nrg_ctx* c, const u64* in, u64 n, u32 words, u32 parts, u64* out, u32* pos, u64* total) {
    if (parts == 0 || parts > PT_MAX_PARTS) return hipErrorInvalidValue;
    if (n == 0) return hipMemsetAsync(total, 0, parts * sizeof(u64), c->stream);
    const u64 ntiles = (n + PT_TILE - 1) / PT_TILE;
    if (ntiles > 0xFFFFFFFFull || n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipError_t e = pt_scratch(c, 2 * ntiles * parts);
    if (e != hipSuccess) return e;
    u32* tcnt = (u32*)c->pt.d_buf;
    u32* toff = tcnt + ntiles * parts;
    pt_count_kernel<<<(unsigned)ntiles, PT_TPB, 0, c->stream>>>(in, n, words, parts, tcnt);
    pt_scan_kernel<<<parts, PT_TPB, 0, c->stream>>>(tcnt, (u32)ntiles, parts, toff, total);
    pt_scatter_kernel<<<(unsigned)ntiles, PT_TPB, 0, c->stream>>>(in, n, words, parts, toff, total, out, pos);
    return hipGetLastError();
}

static hipError_t pt_gather(nrg_ctx* c, const u64* src, const uint8_t* src8, const u32* pos, u64 n, u64* dst, uint8_t* dst8) {
    if (n == 0) return hipSuccess;
    const u64 blocks = (n + PT_TPB - 1) / PT_TPB;
    pt_gather_kernel<<<(unsigned)(blocks < 4096 ? blocks : 4096), PT_TPB, 0, c->stream>>>(src, src8, pos, n, dst, dst8);
    return hipGetLastError();
}

// ---- file partitioning of file-store records (nrg_memfs_partition_async, nrg_group_file_round) ----
// benches/nrfs.rs:25-39 maps an op to the log of its file (LogMapper::hash = fd - 1), cnr/src/replica.rs
// :430-445 takes it modulo the logs: file_owner (common.hpp). The same three launches as the key
// partition above (tile counts, per-owner scan of them, scatter; no workgroup waits on another and
// nothing global is atomic), for nrg_memfs_op records of 19 u64 words with the ino in word 0.
// A record is too wide for a lane to carry, so the two halves of the scatter are split:
//   the rank   one lane per record, one record per thread of a 256-record tile (the ballot loop of
//              pt_scatter_kernel, one round); the record's destination goes to LDS (1 KiB per tile);
//   the move   the tile's 256 * 19 words by the whole workgroup, thread t taking words t, t + 256, ...:
//              the loads are contiguous over the whole tile, 8 bytes per lane (the widest aligned
//              access of a 152-byte record, as mf_frag notes), all 19 in flight before the first
//              store; the stores are contiguous inside a record and across the records of an owner's
//              run, whose destinations are consecutive; the lanes of one record read one LDS word.
// The route-back moves 17-word responses the same way with the sides exchanged: contiguous stores,
// loads contiguous inside a record.
constexpr u32 FP_TILE = PT_TPB;  // records per tile, one per thread (include/nrgpu.h says so to the tests)
constexpr u32 FP_REC_WORDS = sizeof(nrg_memfs_op) / 8, FP_RESP_WORDS = sizeof(nrg_memfs_resp) / 8;
constexpr u32 RD_REQ_WORDS = sizeof(nrg_memfs_rd) / 8;  // a pread request {ino, offset, len}: rd_partition below
static_assert(sizeof(nrg_memfs_op) == 152 && sizeof(nrg_memfs_resp) == 136 && MF_FIRST_INO == NRG_MEMFS_FIRST_INO &&
                  PT_MAX_PARTS == NRG_MAX_PARTS && FP_TILE == NRG_MEMFS_PARTITION_TILE,
              "file partition: record layout");

// (WORDS: u64 words per record, the ino in word 0: an nrg_memfs_op's 19, or a pread request's 3)
template <u32 WORDS>
__global__ __launch_bounds__(PT_TPB) void fp_count_kernel(const u64* __restrict__ in, u64 n, u32 parts,
                                                          u32* __restrict__ tcnt) {
    __shared__ u32 s_c[PT_MAX_PARTS];
    if (threadIdx.x < PT_MAX_PARTS) s_c[threadIdx.x] = 0;
    __syncthreads();
    const u64 i = (u64)blockIdx.x * FP_TILE + threadIdx.x;
    if (i < n) atomicAdd(&s_c[file_owner(in[i * WORDS], parts)], 1u);
    __syncthreads();
    if (threadIdx.x < parts) tcnt[(u64)blockIdx.x * parts + threadIdx.x] = s_c[threadIdx.x];
}

// The rank: where the tile's record of this thread goes in the compact output (valid: it has one, of
// owner o). s_base (owner start: exclusive prefix of the totals) and s_wc (per wave counts, then wave
// offsets) are the calling kernel's LDS; every thread of the workgroup calls this.
__device__ __forceinline__ u32 fp_dest(bool valid, u32 o, u32 parts, const u32* __restrict__ toff,
                                       const u64* __restrict__ total, u32* s_base, u32 (*s_wc)[PT_MAX_PARTS]) {
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    if (t == 0) {
        u32 acc = 0;
        for (u32 p = 0; p < parts; p++) {
            s_base[p] = acc;
            acc += (u32)total[p];
        }
    }
    u32 rank = 0, cnt = 0;  // cnt, lane p: this wave's records of owner p
    u64 act = __ballot(valid);
    while (act) {  // one ballot per distinct owner among the wave's 64 records (wave-uniform loop)
        const int leader = __ffsll((long long)act) - 1;
        const u32 ol = (u32)__shfl((int)o, leader, 64);
        const u64 m = __ballot(valid && o == ol);
        if (valid && o == ol) rank = (u32)__popcll(m & ((1ull << lane) - 1));
        if ((u32)lane == ol) cnt = (u32)__popcll(m);
        act &= ~m;
    }
    if ((u32)lane < parts) s_wc[w][lane] = cnt;
    __syncthreads();
    if (t < (int)parts) {
        u32 acc = 0;
        for (int q = 0; q < PT_WAVES; q++) {
            const u32 c = s_wc[q][t];
            s_wc[q][t] = acc;
            acc += c;
        }
    }
    __syncthreads();
    return valid ? s_base[o] + toff[(u64)blockIdx.x * parts + o] + s_wc[w][o] + rank : 0xFFFFFFFFu;
}

__global__ __launch_bounds__(PT_TPB) void fp_scatter_kernel(const u64* __restrict__ in, u64 n, u32 parts,
                                                            const u32* __restrict__ toff, const u64* __restrict__ total,
                                                            u64* __restrict__ out, u32* __restrict__ pos) {
    __shared__ u32 s_base[PT_MAX_PARTS];
    __shared__ u32 s_wc[PT_WAVES][PT_MAX_PARTS];
    __shared__ u32 s_dest[FP_TILE];  // where the tile's record j goes
    const int t = threadIdx.x;
    const u64 t0 = (u64)blockIdx.x * FP_TILE;
    const u64 i = t0 + t;
    const bool valid = i < n;
    const u32 o = valid ? file_owner(in[i * FP_REC_WORDS], parts) : 0u;
    const u32 dest = fp_dest(valid, o, parts, toff, total, s_base, s_wc);
    if (valid) pos[i] = dest;
    s_dest[t] = dest;
    __syncthreads();
    // the move: word wd of the tile belongs to its record wd / 19
    const u64 left = n - t0;
    const u32 nw = (u32)(left < FP_TILE ? left : FP_TILE) * FP_REC_WORDS;
    const u64* src = in + t0 * FP_REC_WORDS;
    u64 v[FP_REC_WORDS];
#pragma unroll
    for (u32 k = 0; k < FP_REC_WORDS; k++) {
        const u32 wd = k * PT_TPB + t;
        v[k] = wd < nw ? src[wd] : 0ull;
    }
#pragma unroll
    for (u32 k = 0; k < FP_REC_WORDS; k++) {
        const u32 wd = k * PT_TPB + t;
        const u32 j = wd / FP_REC_WORDS;
        const u32 d = s_dest[j];
        // (d < n always: the counts come from the same records; the bound keeps a caller that
        // rewrites them under the kernels from storing outside out)
        if (wd < nw && d < n) out[(u64)d * FP_REC_WORDS + (wd - j * FP_REC_WORDS)] = v[k];
    }
}

// A pread request is three words, so a lane carries its own: the rank above, then three 8-byte stores
// (every destination index is bounded by n, as above).
__global__ __launch_bounds__(PT_TPB) void rd_scatter_kernel(const u64* __restrict__ in, u64 n, u32 parts,
                                                            const u32* __restrict__ toff, const u64* __restrict__ total,
                                                            u64* __restrict__ out, u32* __restrict__ pos) {
    __shared__ u32 s_base[PT_MAX_PARTS];
    __shared__ u32 s_wc[PT_WAVES][PT_MAX_PARTS];
    const u64 i = (u64)blockIdx.x * FP_TILE + threadIdx.x;
    const bool valid = i < n;
    u64 ino = 0, off = 0, len = 0;
    if (valid) ino = in[i * RD_REQ_WORDS], off = in[i * RD_REQ_WORDS + 1], len = in[i * RD_REQ_WORDS + 2];
    const u32 dest = fp_dest(valid, valid ? file_owner(ino, parts) : 0u, parts, toff, total, s_base, s_wc);
    if (!valid) return;
    pos[i] = dest;
    if (dest < n) {
        u64* d = out + (u64)dest * RD_REQ_WORDS;
        d[0] = ino, d[1] = off, d[2] = len;
    }
}

// responses back into issue order: dst[i] = src[pos[i]] (17 words), dst8[i] = src8[pos[i]]
__global__ __launch_bounds__(PT_TPB) void fp_route_kernel(const u64* __restrict__ src, const uint8_t* __restrict__ src8,
                                                          const u32* __restrict__ pos, u64 n, u64* __restrict__ dst,
                                                          uint8_t* __restrict__ dst8) {
    __shared__ u32 s_pos[FP_TILE];
    const int t = threadIdx.x;
    const u64 t0 = (u64)blockIdx.x * FP_TILE;
    const u64 i = t0 + t;
    u32 p = 0xFFFFFFFFu;
    if (i < n) {
        p = pos[i];
        if (dst8 && p < n) dst8[i] = src8[p];  // (p < n: see fp_scatter_kernel)
    }
    s_pos[t] = p;
    __syncthreads();
    if (!dst) return;
    const u64 left = n - t0;
    const u32 nw = (u32)(left < FP_TILE ? left : FP_TILE) * FP_RESP_WORDS;
    u64* d = dst + t0 * FP_RESP_WORDS;
    u64 v[FP_RESP_WORDS];
    u32 ok = 0;
#pragma unroll
    for (u32 k = 0; k < FP_RESP_WORDS; k++) {
        const u32 wd = k * PT_TPB + t;
        const u32 j = wd / FP_RESP_WORDS;
        const u32 pj = s_pos[j];
        const bool live = wd < nw && pj < n;
        v[k] = live ? src[(u64)pj * FP_RESP_WORDS + (wd - j * FP_RESP_WORDS)] : 0ull;
        ok |= live ? 1u << k : 0u;
    }
#pragma unroll
    for (u32 k = 0; k < FP_RESP_WORDS; k++)
        if (ok >> k & 1) d[k * PT_TPB + t] = v[k];
}

hipError_t fp_partition(nrg_ctx* c, const nrg_memfs_op* in, u64 n, u32 parts, nrg_memfs_op* out, u32* pos, u64* total) {
    if (parts == 0 || parts > PT_MAX_PARTS || n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (n == 0) return hipMemsetAsync(total, 0, parts * sizeof(u64), c->stream);
    const u64 ntiles = (n + FP_TILE - 1) / FP_TILE;
    hipError_t e = pt_scratch(c, 2 * ntiles * parts);
    if (e != hipSuccess) return e;
    u32* tcnt = (u32*)c->pt.d_buf;
    u32* toff = tcnt + ntiles * parts;
    NRG_LAUNCH(c, "fp_count", fp_count_kernel<FP_REC_WORDS>, (unsigned)ntiles, PT_TPB, 0, c->stream, (const u64*)in, n, parts, tcnt);
    NRG_LAUNCH(c, "fp_scan", pt_scan_kernel, parts, PT_TPB, 0, c->stream, (const u32*)tcnt, (u32)ntiles, parts, toff,
               total);
    NRG_LAUNCH(c, "fp_scatter", fp_scatter_kernel, (unsigned)ntiles, PT_TPB, 0, c->stream, (const u64*)in, n, parts,
               (const u32*)toff, (const u64*)total, (u64*)out, pos);
    return hipGetLastError();
}

hipError_t rd_partition(nrg_ctx* c, const nrg_memfs_rd* in, u64 n, u32 parts, nrg_memfs_rd* out, u32* pos, u64* total) {
    if (parts == 0 || parts > PT_MAX_PARTS || n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (n == 0) return hipMemsetAsync(total, 0, parts * sizeof(u64), c->stream);
    const u64 ntiles = (n + FP_TILE - 1) / FP_TILE;
    hipError_t e = pt_scratch(c, 2 * ntiles * parts);
    if (e != hipSuccess) return e;
    u32* tcnt = (u32*)c->pt.d_buf;
    u32* toff = tcnt + ntiles * parts;
    NRG_LAUNCH(c, "rd_count", fp_count_kernel<RD_REQ_WORDS>, (unsigned)ntiles, PT_TPB, 0, c->stream, (const u64*)in, n,
               parts, tcnt);
    NRG_LAUNCH(c, "rd_scan", pt_scan_kernel, parts, PT_TPB, 0, c->stream, (const u32*)tcnt, (u32)ntiles, parts, toff,
               total);
    NRG_LAUNCH(c, "rd_scatter", rd_scatter_kernel, (unsigned)ntiles, PT_TPB, 0, c->stream, (const u64*)in, n, parts,
               (const u32*)toff, (const u64*)total, (u64*)out, pos);
    return hipGetLastError();
}

hipError_t fp_route(nrg_ctx* c, const nrg_memfs_resp* src, const uint8_t* src8, const u32* pos, u64 n,
                    nrg_memfs_resp* dst, uint8_t* dst8) {
    if (n == 0 || (!dst && !dst8)) return hipSuccess;
    if (n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    NRG_LAUNCH(c, "fp_route", fp_route_kernel, (unsigned)((n + FP_TILE - 1) / FP_TILE), PT_TPB, 0, c->stream,
               (const u64*)src, src8, pos, n, (u64*)dst, dst8);
    return hipGetLastError();
}

}  // namespace nrg

// ---- the key-partitioning entry points (include/nrgpu.h) -------------------------
using namespace nrg;

extern "C" {

uint32_t nrg_key_owner(uint64_t key, uint32_t parts) { return parts ? nrg::key_owner(key, parts) : 0u; }

int nrg_hashmap_partition_async(nrg_ctx* c, const nrg_put* d_puts, uint64_t W, const uint64_t* d_keys, uint64_t R,
                                uint32_t parts, nrg_put* d_puts_out, uint32_t* d_put_pos, uint64_t* d_keys_out,
                                uint32_t* d_get_pos, uint64_t* d_counts) {
    int r = need(c, NRG_DS_HASHMAP);
    if (r) return r;
    if (parts == 0 || parts > NRG_MAX_PARTS || !d_counts) return NRG_E_INVAL;
    if ((W && (!d_puts || !d_puts_out || !d_put_pos)) || (R && (!d_keys || !d_keys_out || !d_get_pos)))
        return NRG_E_INVAL;
    if (W >= (1ull << 32) || R >= (1ull << 32)) return NRG_E_CAPACITY;
    HIPCHK(pt_partition(c, (const u64*)d_puts, W, 2, parts, (u64*)d_puts_out, d_put_pos, d_counts));
    HIPCHK(pt_partition(c, d_keys, R, 1, parts, d_keys_out, d_get_pos, d_counts + parts));
    return NRG_OK;
}

int nrg_route_back_async(nrg_ctx* c, const uint64_t* d_src, const uint8_t* d_src8, const uint32_t* d_pos, uint64_t n,
                         uint64_t* d_dst, uint8_t* d_dst8) {
    if (!c) return NRG_E_INVAL;
    int r = ctx_use_device(c);
    if (r) return r;
    if (n && (!d_pos || (d_dst && !d_src) || (d_dst8 && !d_src8))) return NRG_E_INVAL;
    HIPCHK(pt_gather(c, d_src, d_src8, d_pos, n, d_dst, d_dst8));
    return NRG_OK;
}

// ---- the file-partitioning entry points (include/nrgpu.h; benches/nrfs.rs:25-39) -----------------
uint32_t nrg_memfs_owner(uint64_t ino, uint32_t parts) { return parts ? nrg::file_owner(ino, parts) : 0u; }

int nrg_memfs_partition_async(nrg_ctx* c, const nrg_memfs_op* d_ops, uint64_t n, uint32_t parts, nrg_memfs_op* d_out,
                              uint32_t* d_pos, uint64_t* d_counts) {
    int r = need(c, NRG_DS_MEMFS);
    if (r) return r;
    if (parts == 0 || parts > NRG_MAX_PARTS || !d_counts) return NRG_E_INVAL;
    if (n && (!d_ops || !d_out || !d_pos)) return NRG_E_INVAL;
    if (((uintptr_t)d_ops | (uintptr_t)d_out) & 7) return NRG_E_INVAL;  // (records move as u64 words)
    if (n >= (1ull << 32)) return NRG_E_CAPACITY;
    HIPCHK(fp_partition(c, d_ops, n, parts, d_out, d_pos, d_counts));
    return NRG_OK;
}

int nrg_memfs_rd_partition_async(nrg_ctx* c, const nrg_memfs_rd* d_reqs, uint64_t n, uint32_t parts, nrg_memfs_rd* d_out,
                                 uint32_t* d_pos, uint64_t* d_counts) {
    int r = need(c, NRG_DS_MEMFS);
    if (r) return r;
    if (parts == 0 || parts > NRG_MAX_PARTS || !d_counts) return NRG_E_INVAL;
    if (n && (!d_reqs || !d_out || !d_pos)) return NRG_E_INVAL;
    if (((uintptr_t)d_reqs | (uintptr_t)d_out) & 7) return NRG_E_INVAL;  // (requests move as u64 words)
    if (n >= (1ull << 32)) return NRG_E_CAPACITY;
    HIPCHK(rd_partition(c, d_reqs, n, parts, d_out, d_pos, d_counts));
    return NRG_OK;
}

int nrg_memfs_route_back_async(nrg_ctx* c, const nrg_memfs_resp* d_src, const uint8_t* d_src_some, const uint32_t* d_pos,
                               uint64_t n, nrg_memfs_resp* d_dst, uint8_t* d_dst_some) {
    int r = need(c, NRG_DS_MEMFS);
    if (r) return r;
    if (n && (!d_pos || (d_dst && !d_src) || (d_dst_some && !d_src_some))) return NRG_E_INVAL;
    if (((uintptr_t)d_src | (uintptr_t)d_dst) & 7) return NRG_E_INVAL;
    if (n >= (1ull << 32)) return NRG_E_CAPACITY;
    HIPCHK(fp_route(c, d_src, d_src_some, d_pos, n, d_dst, d_dst_some));
    return NRG_OK;
}

int nrg_hashmap_prefill_partition(nrg_ctx* c, uint64_t n, uint64_t off, uint32_t part, uint32_t parts) {
    int r = need(c, NRG_DS_HASHMAP);
    if (r) return r;
    if (parts == 0 || parts > NRG_MAX_PARTS || part >= parts) return NRG_E_INVAL;
    if (c->hm.removal && c->hm.tombstone - off < n) return NRG_E_INVAL;  // some k + off is the tombstone
    HIPCHK(hm_prefill_range(c, n, off, part, parts));
    HIPCHK(sync_all(c));
    return check_err(c);
}

}  // extern "C"
