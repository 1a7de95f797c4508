// queue.hip — FIFO queue replica replay on gfx950 (benches/lockfree.rs:43-52 QueueWr::Push(u64) /
// QueueWr::Pop, QueueRd::Len; benches/lockfree_comparisons.rs:75-101 SegQueueWrapper).
//
// Push appends at the back and answers Some(v); Pop removes the front and answers Some(front), or
// None on an empty queue, which stays empty. As for the stack, a run of ops maps the length x
// before it to max(x + e, e - m), where e is the end of its unclamped ±1 walk and m <= 0 the
// walk's minimum; runs compose associatively, so the start length of every tile and lane is an
// exclusive scan. Lengths are conserved: length = L0 + Pushes - successful Pops, so the number of
// successful Pops before an op follows from its start length and the Pushes before it.
//
// The queue is a ring of u64 addressed by a monotonic head H (elements ever popped) and the length
// L0 at chunk start. The chunk's Push of rank p lives at position H + L0 + p; its successful Pop
// of rank r takes position H + r, which is an element from before the chunk (r < L0) or a Push
// that precedes the Pop in log order. The ring holds a power of two >= capacity + max_batch
// slots: the positions a chunk touches, [H, H + L0 + Pushes), are then distinct slots, so no Push
// lands on a slot a Pop of the same chunk still has to read, whatever order the tiles run in.
//
// Four launches per chunk, in stream order, none of which waits on another workgroup:
//   qu_agg_kernel     one (e, m, Pushes) aggregate per tile of 2048 ops (and the log copy of a
//                     fused round); a wave takes its ops as eight rows of 64 consecutive ops
//   qu_scan_kernel    one workgroup: every tile's start length and Pushes before it; publishes
//                     the head and length after the chunk
//   qu_tile_kernel    every lane takes one op per row with the length before it (the scanned tile
//                     start, the waves and rows before, the row's prefix): Push values into the
//                     ring, Push / failed-Pop responses, Pops of elements from before the chunk
//                     answered directly, the length checked against the capacity; a Pop of one of
//                     the chunk's own Pushes leaves its slot in its response word
//   qu_gather_kernel  those Pops read their slot (skipped when the chunk has none)
#include <algorithm>

#include "internal.hpp"

namespace nrg {

constexpr int QU_OPS = 8;                    // ops per lane: a wave takes 8 rows of 64 consecutive ops
constexpr int QU_WAVES = 4;                  // a tile is one workgroup of 4 waves
constexpr int QU_LANES = 64 * QU_WAVES;      // 256 lanes
constexpr int QU_TILE = QU_LANES * QU_OPS;   // 2048 ops
constexpr int QU_SCAN = 256;                 // lanes of the scan workgroup
constexpr uint8_t QU_PENDING = 2;            // some[] of a Pop whose value the gather still fetches

// x -> max(x + b, a): the length after a run of ops (b = e, a = e - m), as stack.hip's Fn
struct QFn {
    long long b;
    long long a;
};
constexpr QFn QFN_ID = {0, -(1ll << 50)};
__device__ __forceinline__ QFn qfn_then(QFn f, QFn g) {  // apply f, then g
    QFn r;
    r.b = f.b + g.b;
    const long long t = f.a + g.b;
    r.a = g.a > t ? g.a : t;
    return r;
}
__device__ __forceinline__ long long qfn_apply(QFn f, long long x) {
    const long long t = x + f.b;
    return f.a > t ? f.a : t;
}

struct QuAgg {  // one tile's run aggregate
    long long b, a;
    u64 pushes;
};
struct QuStart {  // what the scan gives a tile
    long long x;  // length at its first op
    u64 pushes;   // Pushes of the chunk before it
};

struct QuJob {
    const nrg_queue_op* src;  // the batch of a fused round (its log copy is written here), or
    nrg_queue_op* ring;       // nullptr: the records are read from the log ring
    u64 ring_mask;
    u64 lo, n;                // the chunk: log indices [lo, lo + n)
    u64 rlo, rhi;             // response window (log indices); resp == nullptr: none wanted
    u64* resp;
    uint8_t* some;
    u64* q;                   // the queue's ring
    u64 qmask;
    u64 cap;
    QuState* st;
    QuAgg* agg;               // [tiles]
    QuStart* start;           // [tiles]
    DevCtl* ctl;
    u32 tiles;
    u32 stall;
};

__device__ __forceinline__ nrg_queue_op qu_load(const QuJob& j, u64 i) {
    return j.src ? j.src[i] : j.ring[(j.lo + i) & j.ring_mask];
}
__device__ __forceinline__ bool qu_is_push(const nrg_queue_op& o) { return o.op == NRG_QUEUE_PUSH; }

// One workgroup: lane t composes tiles [t * per, (t + 1) * per), the 256 lane results are scanned
// in LDS, and every lane walks its tiles again from its start.
__global__ __launch_bounds__(QU_SCAN) void qu_scan_kernel(QuJob j) {
    __shared__ long long s_b[QU_SCAN], s_a[QU_SCAN];
    __shared__ u64 s_p[QU_SCAN];
    const u32 t = threadIdx.x;
    const int wave = t >> 6;
    const u64 H0 = j.st->head;
    const long long L0 = (long long)j.st->len;
    const u32 per = (j.tiles + QU_SCAN - 1) / QU_SCAN;
    const u32 t0 = t * per < j.tiles ? t * per : j.tiles;
    const u32 t1 = t0 + per < j.tiles ? t0 + per : j.tiles;
    QFn f = QFN_ID;
    u64 p = 0;
    for (u32 k = t0; k < t1; k++) {
        const QuAgg a = j.agg[k];
        f = qfn_then(f, QFn{a.b, a.a});
        p += a.pushes;
    }
    s_b[t] = f.b;
    s_a[t] = f.a;
    s_p[t] = p;
    __syncthreads();
    for (u32 s = 1; s < QU_SCAN; s <<= 1) {
        test_stall(j.stall, wave);
        QFn o = QFN_ID;
        u64 op = 0;
        if (t >= s) {
            o = QFn{s_b[t - s], s_a[t - s]};
            op = s_p[t - s];
        }
        __syncthreads();  // every lane has read its partner before any lane overwrites its own
        test_stall(j.stall, wave);
        if (t >= s) {
            f = qfn_then(o, f);
            p += op;
            s_b[t] = f.b;
            s_a[t] = f.a;
            s_p[t] = p;
        }
        __syncthreads();
    }
    QFn ex = QFN_ID;
    u64 pb = 0;
    if (t > 0) {
        ex = QFn{s_b[t - 1], s_a[t - 1]};
        pb = s_p[t - 1];
    }
    long long x = qfn_apply(ex, L0);
    for (u32 k = t0; k < t1; k++) {
        const QuAgg a = j.agg[k];
        j.start[k] = QuStart{x, pb};
        x = qfn_apply(QFn{a.b, a.a}, x);
        pb += a.pushes;
    }
    if (t == QU_SCAN - 1) {
        // the chunk as a whole: its start for the tile pass and the gather, and the queue after it
        const long long Lf = qfn_apply(f, L0);
        const u64 pops = (u64)(L0 + (long long)p - Lf);  // successful Pops
        j.st->ck_head = H0;
        j.st->ck_len = (u64)L0;
        j.st->ck_pops = pops;
        j.st->head = H0 + pops;
        // an overflowing chunk latches ERR_CAPACITY (tile pass); the length never exceeds the capacity
        j.st->len = (u64)Lf > j.cap ? j.cap : (u64)Lf;
    }
}

// Pops that took one of the chunk's own Pushes: resp[] holds the slot, some[] QU_PENDING.
__global__ __launch_bounds__(256) void qu_gather_kernel(QuJob j, u64 w0, u64 w1) {
    if (j.st->ck_pops <= j.st->ck_len) return;  // every Pop took an element from before the chunk
    const u64 i0 = w0 + (u64)blockIdx.x * 1024 + threadIdx.x;  // a wave's lanes take consecutive ops
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const u64 g = i0 + (u64)k * 256;
        if (g >= w1) break;
        if (j.some[g - j.rlo] == QU_PENDING) {
            j.resp[g - j.rlo] = j.q[j.resp[g - j.rlo] & j.qmask];
            j.some[g - j.rlo] = 1;
        }
    }
}

// A wave's 64 lanes hold 64 consecutive ops (one row, one coalesced load), eight rows per wave.
// What lane l needs about its row: the map of the row's ops before its own, the Pushes among
// them, and (the same in every lane) the whole row's map and Pushes. `valid` is false past the
// chunk's end: such a lane counts for nothing.
struct QRow {
    int b_ex, a_ex;  // x -> max(x + b_ex, a_ex) over the row's ops before this lane's
    int cpush;       // Pushes of the row before this lane's op
    int rb, ra, rp;  // the row as a whole
};
__device__ __forceinline__ QRow qu_row(bool valid, bool push) {
    const int lane = threadIdx.x & 63;
    const u64 vm = __ballot(valid), pm = __ballot(valid && push);
    const u64 below = (1ull << lane) - 1;
    const int nv = __popcll(vm & below), np = __popcll(pm & below);
    const int w_ex = 2 * np - nv;  // the unclamped walk before this op, and after it
    const int w_in = w_ex + (valid ? (push ? 1 : -1) : 0);
    int mn = w_in;  // inclusive prefix minimum of the walk
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int o = __shfl_up(mn, s, 64);
        if (lane >= s) mn = o < mn ? o : mn;
    }
    int m_ex = __shfl_up(mn, 1, 64);
    if (lane == 0 || m_ex > 0) m_ex = 0;
    int m_all = __shfl(mn, 63, 64);
    if (m_all > 0) m_all = 0;
    QRow r;
    r.b_ex = w_ex;
    r.a_ex = w_ex - m_ex;
    r.cpush = np;
    r.rp = __popcll(pm);
    r.rb = 2 * r.rp - __popcll(vm);
    r.ra = r.rb - m_all;
    return r;
}

__global__ __launch_bounds__(QU_LANES) void qu_agg_kernel(QuJob j) {
    __shared__ long long s_b[QU_WAVES], s_a[QU_WAVES];
    __shared__ u64 s_p[QU_WAVES];
    const u32 t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const u64 base = (u64)blockIdx.x * QU_TILE + (u64)wave * (64 * QU_OPS) + lane;
    QFn f = QFN_ID;
    u64 p = 0;
#pragma unroll
    for (int k = 0; k < QU_OPS; k++) {
        const u64 i = base + (u64)k * 64;
        const bool valid = i < j.n;
        bool push = false;
        if (valid) {
            const nrg_queue_op o = qu_load(j, i);
            if (j.src) j.ring[(j.lo + i) & j.ring_mask] = o;  // Log::append of a fused round
            push = qu_is_push(o);
        }
        const QRow r = qu_row(valid, push);
        f = qfn_then(f, QFn{r.rb, r.ra});
        p += (u64)r.rp;
    }
    if (lane == 0) {
        s_b[wave] = f.b;
        s_a[wave] = f.a;
        s_p[wave] = p;
    }
    __syncthreads();
    if (t == 0) {
        QFn r = {s_b[0], s_a[0]};
        u64 rp = s_p[0];
        for (int w = 1; w < QU_WAVES; w++) {
            r = qfn_then(r, QFn{s_b[w], s_a[w]});
            rp += s_p[w];
        }
        j.agg[blockIdx.x] = QuAgg{r.b, r.a, rp};
    }
}

__global__ __launch_bounds__(QU_LANES) void qu_tile_kernel(QuJob j) {
    __shared__ long long s_b[QU_WAVES], s_a[QU_WAVES];
    __shared__ u64 s_p[QU_WAVES];
    const u32 t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const u64 base = (u64)blockIdx.x * QU_TILE + (u64)wave * (64 * QU_OPS) + lane;
    u64 val[QU_OPS];
    int b_ex[QU_OPS], a_ex[QU_OPS], cpush[QU_OPS], rb[QU_OPS], ra[QU_OPS], rp[QU_OPS];
    u32 pushbits = 0;
    QFn f = QFN_ID;
    u64 p = 0;
#pragma unroll
    for (int k = 0; k < QU_OPS; k++) {
        const u64 i = base + (u64)k * 64;
        const bool valid = i < j.n;
        bool push = false;
        val[k] = 0;
        if (valid) {
            const nrg_queue_op o = qu_load(j, i);
            val[k] = o.val;
            push = qu_is_push(o);
        }
        if (push) pushbits |= 1u << k;
        const QRow r = qu_row(valid, push);
        b_ex[k] = r.b_ex, a_ex[k] = r.a_ex, cpush[k] = r.cpush;
        rb[k] = r.rb, ra[k] = r.ra, rp[k] = r.rp;
        f = qfn_then(f, QFn{r.rb, r.ra});
        p += (u64)r.rp;
    }
    if (lane == 0) {
        s_b[wave] = f.b;
        s_a[wave] = f.a;
        s_p[wave] = p;
    }
    __syncthreads();
    const QuStart s0 = j.start[blockIdx.x];
    long long x = s0.x;  // the length and the chunk's Pushes before the row (the same in every lane)
    u64 pb = s0.pushes;
    for (int w = 0; w < wave; w++) {
        x = qfn_apply(QFn{s_b[w], s_a[w]}, x);
        pb += s_p[w];
    }
    const u64 H = j.st->ck_head, L0 = j.st->ck_len;
    bool over = false;
#pragma unroll
    for (int k = 0; k < QU_OPS; k++) {
        const u64 i = base + (u64)k * 64;
        if (i < j.n) {
            const u64 g = j.lo + i;
            const bool win = j.resp && g >= j.rlo && g < j.rhi;
            const long long xb = qfn_apply(QFn{b_ex[k], a_ex[k]}, x);  // the length before this op
            const u64 pbl = pb + (u64)cpush[k];
            u64 out = 0;
            uint8_t sm = 0;
            if (pushbits & (1u << k)) {
                j.q[(H + L0 + pbl) & j.qmask] = val[k];
                over |= (u64)(xb + 1) > j.cap;
                out = val[k];
                sm = 1;
            } else if (xb > 0) {
                const u64 r = L0 + pbl - (u64)xb;  // successful Pops before this one
                const u64 slot = (H + r) & j.qmask;
                if (r < L0) {  // an element from before the chunk: no Push of the chunk lands on its slot
                    if (win) out = j.q[slot];
                    sm = 1;
                } else {       // one of the chunk's own Pushes: the gather reads it after every tile ran
                    out = slot;
                    sm = QU_PENDING;
                }
            }
            if (win) {
                j.resp[g - j.rlo] = out;
                j.some[g - j.rlo] = sm;
            }
        }
        x = qfn_apply(QFn{rb[k], ra[k]}, x);
        pb += (u64)rp[k];
    }
    if (__ballot(over) != 0 && lane == 0) atomicOr(&j.ctl->err, ERR_CAPACITY);
}

__global__ void qu_range_kernel(u64* q, u64 n, QuState* st) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) q[i] = i;
    if (i == 0) {
        st->head = 0;
        st->len = n;
    }
}

// n Len reads against the current length (QueueRd::Len, benches/lockfree_comparisons.rs:99)
__global__ void qu_len_kernel(const QuState* st, u32 n, u64* out, uint8_t* some) {
    const u64 len = st->len;
    for (u32 i = threadIdx.x; i < n; i += blockDim.x) {
        out[i] = len;
        some[i] = 1;
    }
}

static u64 qu_max_tiles(u64 max_batch) { return (max_batch + QU_TILE - 1) / QU_TILE; }

static u64 qu_aux_bytes(u64 max_batch) { return qu_max_tiles(max_batch) * (sizeof(QuAgg) + sizeof(QuStart)); }

// ---- growth (SegQueue never refuses a push: benches/lockfree_comparisons.rs:75-101) ---------------
// A re-layout, not a copy: the live elements are the ring positions [head, head + len) under the
// old mask (the range may wrap the old ring's end) and go to the same positions under the new mask,
// so head stays monotonic and QuState is unchanged. head and the length are read here, the length
// clamped as nrg_queue_len clamps it; consecutive lanes take consecutive elements.
__global__ __launch_bounds__(DG_TPB) void qu_grow_kernel(const u64* __restrict__ from, u64 from_mask,
                                                         u64* __restrict__ to, u64 to_mask, const QuState* st,
                                                         u64 from_cap) {
    const u64 head = st->head;
    const u64 n = st->len > from_cap ? from_cap : st->len;
    for (u64 i = blockIdx.x * (u64)DG_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * DG_TPB)
        to[(head + i) & to_mask] = from[(head + i) & from_mask];
}

// The ring is reallocated to the power of two at or above new_cap + max_batch (qu_open's invariant);
// where that is the ring it has, only the capacity changes. The re-layout, then the stream is
// synchronised (there is no stream-ordered free), the old ring freed and the new one installed with
// the capacity every launch and clamp reads (cfg.queue_capacity, qu.size). If the allocation fails
// nothing has been launched: the replica is as it was.
static hipError_t qu_grow(nrg_ctx* c, u64 new_cap) {
    const u64 cap = c->cfg.queue_capacity;
    if (new_cap <= cap || new_cap > (1ull << 32)) return hipErrorInvalidValue;
    const u64 nsize = pow2_at_least(new_cap + c->cfg.max_batch);
    if (nsize != c->qu.size) {
        u64* nq = nullptr;
        if (hipMalloc(&nq, nsize * sizeof(u64)) != hipSuccess) {
            (void)hipGetLastError();  // (the failure is reported by the return value alone)
            return hipErrorOutOfMemory;
        }
        NRG_LAUNCH(c, "qu_grow", qu_grow_kernel, copy_grid(cap), DG_TPB, 0, c->stream, (const u64*)c->qu.d_queue,
                   c->qu.size - 1, nq, nsize - 1, (const QuState*)c->qu.d_state, cap);
        hipError_t e = hipGetLastError();
        const hipError_t es = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = es;
        if (e != hipSuccess) {
            (void)hipFree(nq);
            return e;
        }
        (void)hipFree(c->qu.d_queue);
        c->qu.d_queue = nq;
        c->qu.size = nsize;
    }
    c->cfg.queue_capacity = new_cap;
    return hipSuccess;
}

// One chunk of at most max_batch records: log indices [lo, lo + n), read from the ring or, for a
// fused round, from `src` (the log copy is then written by the aggregate pass).
static hipError_t qu_replay_chunk(nrg_ctx* c, const void* src, u64 lo, u64 n, u64 resp_lo, u64 resp_hi, void* d_resp,
                                  uint8_t* d_some) {
    if (n == 0) return hipSuccess;
    // the ring grows first if it has to (one comparison if not)
    if (!growth_fits(c->growth, c->cfg.queue_capacity, n)) {
        const hipError_t eg = room(c, n, "qu_room");
        if (eg != hipSuccess) return eg;
    }
    QuJob j{};
    j.src = (const nrg_queue_op*)src;
    j.ring = (nrg_queue_op*)c->d_ring;
    j.ring_mask = c->log_size - 1;
    j.lo = lo;
    j.n = n;
    // (an empty window inside the chunk, a group member without writes, wants nothing either)
    const bool want = d_resp != nullptr && d_some != nullptr && resp_lo < resp_hi && resp_lo < lo + n && resp_hi > lo;
    j.rlo = want ? resp_lo : 0;
    j.rhi = want ? resp_hi : 0;
    j.resp = want ? (u64*)d_resp : nullptr;
    j.some = want ? d_some : nullptr;
    j.q = c->qu.d_queue;
    j.qmask = c->qu.size - 1;
    j.cap = c->cfg.queue_capacity;
    j.st = c->qu.d_state;
    j.tiles = (u32)((n + QU_TILE - 1) / QU_TILE);
    j.agg = (QuAgg*)c->qu.d_aux;
    j.start = (QuStart*)(j.agg + qu_max_tiles(c->cfg.max_batch));
    j.ctl = c->d_ctl;
    j.stall = c->stall;
    timer_begin(c, "qu_replay");
    qu_agg_kernel<<<j.tiles, QU_LANES, 0, c->stream>>>(j);
    qu_scan_kernel<<<1, QU_SCAN, 0, c->stream>>>(j);
    qu_tile_kernel<<<j.tiles, QU_LANES, 0, c->stream>>>(j);
    if (want) {
        const u64 w0 = resp_lo > lo ? resp_lo : lo, w1 = resp_hi < lo + n ? resp_hi : lo + n;
        qu_gather_kernel<<<(unsigned)((w1 - w0 + 1023) / 1024), 256, 0, c->stream>>>(j, w0, w1);
    }
    timer_end(c, "qu_replay");
    return hipGetLastError();
}

static hipError_t qu_init_range(nrg_ctx* c, u64 n) {
    qu_range_kernel<<<(unsigned)((n + 255) / 256 + (n == 0)), 256, 0, c->stream>>>(c->qu.d_queue, n, c->qu.d_state);
    return hipGetLastError();
}

hipError_t qu_len_answers(nrg_ctx* c, u32 n, u64* d_out, uint8_t* d_some) {
    qu_len_kernel<<<1, 256, 0, c->stream>>>(c->qu.d_state, n, d_out, d_some);
    return hipGetLastError();
}

static int qu_open(nrg_ctx* c) {
    const nrg_config& cf = c->cfg;
    const u64 mb = cf.max_batch;
    // max_batch <= 2^24: one workgroup scans the tile aggregates; the capacity bounds the ring of
    // u64 values
    if (!cf.queue_capacity || cf.queue_capacity > (1ull << 32) || mb > (1ull << 24)) return NRG_E_INVAL;
    // capacity + max_batch slots: the positions one chunk touches never alias
    c->qu.size = pow2_at_least(cf.queue_capacity + mb);
    HIPCHK(hipMalloc(&c->qu.d_queue, c->qu.size * sizeof(u64)));
    HIPCHK(hipMalloc(&c->qu.d_state, sizeof(QuState)));
    HIPCHK(hipMemsetAsync(c->qu.d_state, 0, sizeof(QuState), c->stream));
    HIPCHK(hipMalloc(&c->qu.d_aux, qu_aux_bytes(mb)));
    c->pipeline = false;  // config.pipeline is accepted: nothing is deferred
    return NRG_OK;
}

static void qu_close(nrg_ctx* c) {
    (void)hipFree(c->qu.d_queue);
    (void)hipFree(c->qu.d_state);
    (void)hipFree(c->qu.d_aux);
}

// nrg_digest: item i from the front is (i, q[(head + i) & mask]): the logical position, whatever
// ring slot holds it; head and the length are read here, the length clamped as nrg_queue_len clamps it
__global__ __launch_bounds__(DG_TPB) void qu_digest_kernel(const u64* __restrict__ q, u64 qmask, const QuState* st,
                                                           u64 cap, u64* out3) {
    const u64 head = st->head;
    const u64 n = st->len > cap ? cap : st->len;
    u64 c = 0, sm = 0, x = 0;
    for (u64 i = blockIdx.x * (u64)DG_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * DG_TPB) {
        const u64 h = dg_item(i, q[(head + i) & qmask]);
        c++;
        sm += h;
        x ^= h;
    }
    dg_commit(c, sm, x, out3);
}

static hipError_t qu_digest(nrg_ctx* c, u64* d_out3) {
    hipError_t e = hipMemsetAsync(d_out3, 0, 3 * sizeof(u64), c->stream);
    if (e != hipSuccess) return e;
    NRG_LAUNCH(c, "qu_digest", qu_digest_kernel, dg_grid(c->cfg.queue_capacity), DG_TPB, 0, c->stream,
               (const u64*)c->qu.d_queue, (u64)(c->qu.size - 1), (const QuState*)c->qu.d_state,
               (u64)c->cfg.queue_capacity, d_out3);
    return hipGetLastError();
}

// ---- nrg_snapshot_async / nrg_restore: the elements, front first ---------------------------------
// The one reader of QuState (the snapshot's item count, the growth policy's exact length,
// nrg_queue_len and nrg_queue_dump): the length never more than the capacity. Drains the stream.
static int qu_read_state(nrg_ctx* c, QuState* s) {
    HIPCHK(hipMemcpyAsync(s, c->qu.d_state, sizeof(*s), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (s->len > c->cfg.queue_capacity) s->len = c->cfg.queue_capacity;
    return NRG_OK;
}

static int qu_items(nrg_ctx* c, u64* n) {
    QuState s{};
    int r = qu_read_state(c, &s);
    if (r) return r;
    *n = s.len;
    return NRG_OK;
}

// The logical order, whatever ring slots hold it: out[i] = q[(head + i) & mask], head and the
// length read here. The image must fit whole or nothing of the payload is stored.
__global__ __launch_bounds__(DG_TPB) void qu_snapshot_kernel(const u64* __restrict__ q, u64 qmask, const QuState* st,
                                                             u64 elems, u64* buf, u64 cap, u64 log_idx, DevCtl* ctl) {
    const u64 head = st->head;
    const u64 n = st->len > elems ? elems : st->len;
    if (blockIdx.x == 0 && threadIdx.x == 0) snap_head(buf, cap, NRG_DS_QUEUE, n, n * 8, log_idx, ctl);
    if (snap_bytes(n * 8) > cap) return;
    u64* out = buf + SNAP_HDR / 8;
    for (u64 i = blockIdx.x * (u64)DG_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * DG_TPB)
        out[i] = q[(head + i) & qmask];
}

static hipError_t qu_snapshot(nrg_ctx* c, void* d_buf, u64 cap, u64 log_idx) {
    NRG_LAUNCH(c, "qu_snapshot", qu_snapshot_kernel, dg_grid(c->cfg.queue_capacity), DG_TPB, 0, c->stream,
               (const u64*)c->qu.d_queue, (u64)(c->qu.size - 1), (const QuState*)c->qu.d_state,
               (u64)c->cfg.queue_capacity, (u64*)d_buf, cap, log_idx, c->d_ctl);
    return hipGetLastError();
}

// ring positions [0, n) and the state of a queue initialised with these values (nrg_queue_init):
// front at 0, the checkpoint fields clear
__global__ __launch_bounds__(DG_TPB) void qu_restore_kernel(u64* q, const u64* __restrict__ src, u64 n, QuState* st) {
    for (u64 i = blockIdx.x * (u64)DG_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * DG_TPB) q[i] = src[i];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->head = 0;
        st->len = n;
        st->ck_head = st->ck_len = st->ck_pops = 0;
    }
}

static int qu_restore(nrg_ctx* c, const void* d_payload, u64 items, bool check_only) {
    int r;
    if (restore_room(c, d_payload, &items, check_only, &r)) return r;
    NRG_LAUNCH(c, "qu_restore", qu_restore_kernel, dg_grid(items), DG_TPB, 0, c->stream, c->qu.d_queue,
               (const u64*)d_payload, items, c->qu.d_state);
    c->growth.len_ub = items;
    return hip_fail(hipGetLastError());
}

static u64 qu_capacity(const nrg_ctx* c) { return c->cfg.queue_capacity; }

const DsOps* qu_ops() {
    static const DsOps ops = {sizeof(nrg_queue_op), sizeof(u64), qu_open, qu_close, nullptr, qu_replay_chunk,
                              floor_ltail, nullptr, nullptr, nullptr, qu_digest,
                              qu_items, qu_snapshot, qu_restore, 1ull << 32, qu_capacity, qu_grow, true};
    return &ops;
}

}  // namespace nrg

// ---- the queue's entry points (include/nrgpu.h) -----------------------------------------------
using namespace nrg;

extern "C" {

int nrg_queue_round_async(nrg_ctx* c, const nrg_queue_op* d_ops, uint64_t n, uint32_t origin, uint64_t* d_resp,
                          uint8_t* d_some) {
    return round_common(c, NRG_DS_QUEUE, d_ops, n, origin, d_resp, d_some);
}

static int qu_set_state(nrg_ctx* c, uint64_t n) {
    QuState s{};
    s.len = n;
    HIPCHK(hipMemcpyAsync(c->qu.d_state, &s, sizeof(s), hipMemcpyHostToDevice, c->stream));
    HIPCHK(sync_all(c));
    return NRG_OK;
}

int nrg_queue_init(nrg_ctx* c, const uint64_t* vals, uint64_t n) {
    int r = need(c, NRG_DS_QUEUE);
    if (r) return r;
    if (n > c->cfg.queue_capacity) return NRG_E_CAPACITY;
    if (n && !vals) return NRG_E_INVAL;
    // head = 0: the n values sit at the start of the ring (capacity <= its size)
    if (n) HIPCHK(hipMemcpyAsync(c->qu.d_queue, vals, n * 8, hipMemcpyHostToDevice, c->stream));
    if ((r = qu_set_state(c, n))) return r;
    c->growth.len_ub = n;
    return NRG_OK;
}

int nrg_queue_init_range(nrg_ctx* c, uint64_t n) {
    int r = need(c, NRG_DS_QUEUE);
    if (r) return r;
    if (n > c->cfg.queue_capacity) return NRG_E_CAPACITY;
    HIPCHK(qu_init_range(c, n));
    HIPCHK(sync_all(c));
    c->growth.len_ub = n;
    return NRG_OK;
}

int nrg_queue_reserve(nrg_ctx* c, uint64_t n_elems) { return reserve_common(c, NRG_DS_QUEUE, n_elems); }

int nrg_queue_capacity(nrg_ctx* c, uint64_t* n) { return capacity_common(c, NRG_DS_QUEUE, n); }

// the front's monotonic position and the length, then the error latch
static int qu_get_state(nrg_ctx* c, uint64_t* head, uint64_t* len) {
    QuState s{};
    int r = qu_read_state(c, &s);
    if (r) return r;
    *head = s.head;
    *len = s.len;
    return check_err(c);
}

int nrg_queue_len(nrg_ctx* c, uint64_t* n) {
    int r = need(c, NRG_DS_QUEUE);
    if (r) return r;
    if (!n) return NRG_E_INVAL;
    uint64_t head = 0;
    return qu_get_state(c, &head, n);
}

int nrg_queue_dump(nrg_ctx* c, uint64_t* vals, uint64_t cap, uint64_t* n) {
    int r = need(c, NRG_DS_QUEUE);
    if (r) return r;
    if (!n) return NRG_E_INVAL;
    uint64_t head = 0;
    if ((r = qu_get_state(c, &head, n))) return r;
    if (*n > cap) return NRG_E_CAPACITY;
    if (*n) {
        if (!vals) return NRG_E_INVAL;
        const uint64_t phys = head & (c->qu.size - 1);
        const uint64_t first = *n < c->qu.size - phys ? *n : c->qu.size - phys;
        HIPCHK(hipMemcpyAsync(vals, c->qu.d_queue + phys, first * 8, hipMemcpyDeviceToHost, c->stream));
        if (first < *n)
            HIPCHK(hipMemcpyAsync(vals + first, c->qu.d_queue, (*n - first) * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(sync_all(c));
    }
    return NRG_OK;
}

}  // extern "C"
