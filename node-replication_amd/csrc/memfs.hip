// memfs.hip — replicated file store (memfs Write / Read / GetAttr) replay on gfx950
// (benches/memfs.rs:24-85 OperationWr, :88-98 Response, :112-121 the initial file, :194-292 Dispatch,
// :294-322 generate_fs_operations).
//
// What this structure has and the six others have not: READS GO THROUGH THE LOG. In memfs.rs
// ReadOperation = () and dispatch is unreachable!() (:194-201); OperationWr::Read is a write
// operation (:73-78, :267-282), so a Read's answer is the file's bytes as every earlier record of the
// log left them. And the payload is bytes (data: &[u8], [3; 128] in generate_fs_operations), not a u64.
//
// What the reference pins: the op set (Write / Read / GetAttr of :24-85), the initial file (ino 5,
// 4096 bytes of 1, :112-121), the responses Written(len) and Data(bytes) (:88-98), and that both ops
// are logged. The file system itself (btfs) is a crates.io dependency and is not part of the
// reference checkout, so everything else is DEFINED HERE as POSIX pwrite / pread on files of fixed
// size: a replica holds F files of B bytes, inodes NRG_MEMFS_FIRST_INO .. +F-1, every byte 0x01 at
// open; a Write past the end fails whole (EFBIG), a Read is clipped at the end. A record is checked
// in this order: len > 128 or an unknown op (EINVAL, latched), then the ino (ENOENT), then the
// Write's range (EFBIG).
// Out of scope: directories, names, inode creation and removal, rename.
// Sizes (SetAttr as ftruncate, Writes that grow a file) are off unless nrg_memfs_enable_sizes was called:
// the section "Sizes" below. Out of scope: the other SetAttrRequest fields.
// Capacity growth past B (nrg_set_max_capacity, nrg_memfs_reserve; sized contexts only): the section
// "Capacity growth" below. B is read from the context by every call; nothing holds a value from open.
// benches/nrfs.rs's whole-file 4096-byte ops: its read-only FileRead is nrg_memfs_pread* below, which
// goes through no log record; its FileWrite is nrg_memfs_pwrite* below, a write of any length as a
// contiguous run of these records, cut on the device straight into the log ring (mf_frag).
// memfs.rs's own Read with a size of any length is nrg_memfs_pread_logged* below: a contiguous run of
// Read records (mf_rfrag), replayed like any others, their responses gathered into the caller's bytes
// (mf_rgather, mf_rcount).
// Out of scope: the combiner, partitioned groups and growth inside a partitioned round.
// (That sentence speaks of the key-partitioned entry points, nrg_group_partitioned_round*, which still
// return NRG_E_INVAL for this kind: a file has no key to hash. A group of file stores is partitioned by
// file, as benches/nrfs.rs runs it, in group_files.cpp: nrg_group_file_round, with the record partition
// and the response route-back in partition.hip; a member with a growth bound is refused there, since an
// owner replays its own files' records alone, and such a group grows with nrg_memfs_reserve.)
//
// A file is cut into aligned 128-byte LINES; an op of at most 128 bytes touches at most two. Lines
// are independent of each other; within a line log order decides. A chunk of n records, in stream
// order, no workgroup waiting on another except inside the radix sort's look-back:
//   mf_expand  one lane per record: the log copy of a fused round, the validation, the whole
//              response inside the response window (n, some, 128 data bytes zeroed; 8-byte coalesced
//              stores), a descriptor per record {first byte, count, is-write}, and exactly two slots
//              2i and 2i + 1 keyed by the global line id (file * B/128 + line) of each line the op
//              touches; the sentinel F*B/128, which sorts last and is no line, for an unused slot, a
//              failed op, an op of no bytes and GetAttr. ERR_INVAL latched for len > 128 / unknown op.
//   sort       radix_sort.hip sort_pairs of the 2n (key, slot) pairs, stable: slot order is log order,
//              so every line's run is in log order. Timed as "mf_sort".
//   mf_lines   one wave per line of the store. The wave finds its run by a lower-bound search of the
//              sorted keys (uniform: scalar loads); an empty run exits without touching the line. Else
//              lane l holds bytes 2l and 2l + 1 of the line and the wave walks the run in batches of 64
//              slots: lane j fetches slot t0 + j and its record's descriptor, the batch loop broadcasts
//              each descriptor (v_readlane: the values are uniform, so are the branches on them) and
//              applies it: a Write's covered lanes take data[x - offset], a Read's covered lanes store
//              their byte to resp[i].data[x - offset] (records inside the response window only). The
//              only serial dependence is the line register: the data loads of MF_AHEAD ops are issued
//              before the first of them is applied, and the next batch's slots and descriptors are
//              fetched before this batch is walked. The line is stored back once. No LDS, no atomics,
//              no spinning.
// Known limit: memfs.rs's own shape, one 4 KiB file, is 32 lines and so 32 waves (DESIGN.md "File
// store replay"; the next step is a segmented reduce-then-scan over tiles of a line's run).
#include <cstring>

#include "../../include/nrgpu_testing.h"
#include "internal.hpp"
#include "memfs_plan.hpp"

namespace nrg {

constexpr int MF_TPB = 256;
constexpr u32 MF_LINE = 128;      // bytes of a line; also the most bytes a record carries
constexpr u32 MF_REC_WORDS = 19;  // nrg_memfs_op in u64 words
constexpr u32 MF_RESP_WORDS = 17; // nrg_memfs_resp in u64 words
constexpr u32 MF_AHEAD = 8;       // ops whose data loads are in flight together (divides 64)
constexpr u32 MF_LOG2_MIN = 7, MF_LOG2_MAX = 26, MF_LOG2_DEFAULT = 12;
constexpr u64 MF_MAX_FILES = 1ull << 16, MF_MAX_BYTES = 1ull << 29, MF_MAX_BATCH = 1ull << 20;
static_assert(sizeof(nrg_memfs_op) == MF_REC_WORDS * 8 && sizeof(nrg_memfs_resp) == MF_RESP_WORDS * 8, "ABI");
static_assert(64 % MF_AHEAD == 0, "a batch of 64 slots is walked in whole groups");

struct MfJob {
    const u64* src;  // the batch of a fused round in u64 words, or nullptr: read from the ring
    u64* ring;       // the log ring; written when src is given
    u64 ring_mask;
    u64 lo, n;       // the chunk: log indices [lo, lo + n)
    u64 rlo, rhi;    // response window
    u64* resp;       // responses in u64 words (nullptr: none wanted)
    uint8_t* some;
    DevCtl* ctl;
    uint8_t* files;  // F files of B bytes, inode order
    u32 log2_b, nfiles;
    u64 adm;         // sized kernels: what a Write's end and a SetAttr's size are admitted against: B, or
                     // the growth bound where one is set above it ("Capacity growth" below)
    u32 nlines;      // F * B / 128: the sentinel key
    u32* keys;       // [2n] slot keys
    u64* desc;       // [n] first byte in the store | count << 32 | is-write << 48; 0: touches nothing
};

__device__ __forceinline__ const u64* mf_rec(const MfJob& j, u64 i) {
    return j.src ? j.src + i * MF_REC_WORDS : j.ring + ((j.lo + i) & j.ring_mask) * MF_REC_WORDS;
}

__global__ __launch_bounds__(MF_TPB) void mf_expand_kernel(MfJob j) {
    __shared__ u64 s_n[MF_TPB];
    const u32 t = threadIdx.x;
    const u64 base = (u64)blockIdx.x * MF_TPB;
    const u32 cnt = j.n - base < MF_TPB ? (u32)(j.n - base) : MF_TPB;
    bool inval = false;
    if (t < cnt) {
        const u64 i = base + t;
        const u64* r = mf_rec(j, i);
        const u64 ino = r[0], off = r[1], w2 = r[2];
        const u32 op = (u32)w2, len = (u32)(w2 >> 32);
        const u64 B = 1ull << j.log2_b;
        u64 nresp;
        u32 cover = 0;
        uint8_t sm = 0;
        bool wr = false;
        if (op > NRG_MEMFS_GETATTR || len > MF_LINE) {
            nresp = NRG_MEMFS_EINVAL;
            inval = true;
        } else if (ino < NRG_MEMFS_FIRST_INO || ino - NRG_MEMFS_FIRST_INO >= j.nfiles) {
            nresp = NRG_MEMFS_ENOENT;
        } else if (op == NRG_MEMFS_GETATTR) {  // Attr(FileAttr): the size
            nresp = B, sm = 1;
        } else if (op == NRG_MEMFS_WRITE) {
            if (off <= B && len <= B - off) nresp = len, cover = len, sm = 1, wr = true;  // Written(len)
            else nresp = NRG_MEMFS_EFBIG;
        } else {  // Data(bytes), clipped at the end of the file
            nresp = off >= B ? 0 : (len < B - off ? len : B - off);
            cover = (u32)nresp, sm = 1;
        }
        u32 k0 = j.nlines, k1 = j.nlines;
        u64 d = 0;
        if (cover) {
            const u64 start = ((ino - NRG_MEMFS_FIRST_INO) << j.log2_b) + off;  // < 2^29
            k0 = (u32)(start >> 7);
            const u32 kl = (u32)((start + cover - 1) >> 7);
            if (kl != k0) k1 = kl;
            d = start | ((u64)cover << 32) | ((u64)(wr ? 1 : 0) << 48);
        }
        *(uint2*)(j.keys + 2 * i) = make_uint2(k0, k1);
        j.desc[i] = d;
        s_n[t] = nresp;
        const u64 g = j.lo + i;
        if (j.resp && g >= j.rlo && g < j.rhi) j.some[g - j.rlo] = sm;
    }
    if (__any(inval) && (t & 63) == 0) atomicOr(&j.ctl->err, ERR_INVAL);
    __syncthreads();
    if (j.src)  // Log::append of a fused round
        for (u32 w = t; w < cnt * MF_REC_WORDS; w += MF_TPB) {
            const u32 rec = w / MF_REC_WORDS, q = w - rec * MF_REC_WORDS;
            j.ring[((j.lo + base + rec) & j.ring_mask) * MF_REC_WORDS + q] = j.src[(base + rec) * MF_REC_WORDS + q];
        }
    if (j.resp)
        for (u32 w = t; w < cnt * MF_RESP_WORDS; w += MF_TPB) {
            const u32 rec = w / MF_RESP_WORDS, q = w - rec * MF_RESP_WORDS;
            const u64 g = j.lo + base + rec;
            if (g >= j.rlo && g < j.rhi) j.resp[(g - j.rlo) * MF_RESP_WORDS + q] = q ? 0 : s_n[rec];
        }
}

// One wave per line. sk / sv: the m = 2n sorted (key, slot) pairs.
__global__ __launch_bounds__(MF_TPB) void mf_lines_kernel(MfJob j, const u32* __restrict__ sk,
                                                          const u32* __restrict__ sv, u32 m) {
    const u32 lane = threadIdx.x & 63;
    const u32 X = __builtin_amdgcn_readfirstlane(blockIdx.x * (MF_TPB / 64) + (threadIdx.x >> 6));
    if (X >= j.nlines) return;
    u32 lo = 0, hi = m;
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (sk[mid] < X) lo = mid + 1; else hi = mid;
    }
    const u32 r0 = lo;
    if (r0 >= m || sk[r0] != X) return;  // no op of the chunk touches the line
    lo = r0 + 1, hi = m;
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (sk[mid] <= X) lo = mid + 1; else hi = mid;
    }
    const u32 r1 = lo;
    unsigned short* lp = (unsigned short*)(j.files + (u64)X * MF_LINE) + lane;
    const u32 w = *lp;
    u32 b0 = w & 0xFF, b1 = w >> 8;
    const u32 gx0 = X * MF_LINE + 2 * lane;  // this lane's first byte in the store
    uint8_t* const rbytes = (uint8_t*)j.resp;
    u32 myrec = 0;
    u64 mydesc = 0;
    if (r0 + lane < r1) {
        myrec = sv[r0 + lane] >> 1;
        mydesc = j.desc[myrec];
    }
    for (u32 t0 = r0; t0 < r1; t0 += 64) {
        const u32 cnt = r1 - t0 < 64 ? r1 - t0 : 64;
        u32 nrec = 0;  // the next batch, fetched before this one is walked
        u64 ndesc = 0;
        if (t0 + 64 + lane < r1) {
            nrec = sv[t0 + 64 + lane] >> 1;
            ndesc = j.desc[nrec];
        }
        const u32 dlo = (u32)mydesc, dhi = (u32)(mydesc >> 32);  // (lanes at or past cnt hold 0: no bytes)
        for (u32 k = 0; k < cnt; k += MF_AHEAD) {
            u32 rec[MF_AHEAD], rel[MF_AHEAD], cn[MF_AHEAD], d0[MF_AHEAD], d1[MF_AHEAD];
            bool wr[MF_AHEAD];
#pragma unroll
            for (u32 u = 0; u < MF_AHEAD; u++) {
                const u32 st = __builtin_amdgcn_readlane(dlo, k + u), h = __builtin_amdgcn_readlane(dhi, k + u);
                rec[u] = __builtin_amdgcn_readlane(myrec, k + u);
                cn[u] = h & 0xFFFF;
                wr[u] = (h >> 16) != 0;
                rel[u] = gx0 - st;  // byte 0's offset into the op (wraps where the op starts later)
                d0[u] = d1[u] = 0;
                if (wr[u]) {
                    const uint8_t* p = (const uint8_t*)(mf_rec(j, rec[u]) + 3);
                    if (rel[u] < cn[u]) d0[u] = p[rel[u]];
                    if (rel[u] + 1 < cn[u]) d1[u] = p[rel[u] + 1];
                }
            }
#pragma unroll
            for (u32 u = 0; u < MF_AHEAD; u++) {
                const bool c0 = rel[u] < cn[u], c1 = rel[u] + 1 < cn[u];
                if (wr[u]) {
                    b0 = c0 ? d0[u] : b0;
                    b1 = c1 ? d1[u] : b1;
                } else if (cn[u]) {
                    const u64 g = j.lo + rec[u];
                    if (rbytes && g >= j.rlo && g < j.rhi) {
                        uint8_t* o = rbytes + (g - j.rlo) * sizeof(nrg_memfs_resp) + 8;
                        if (c0) o[rel[u]] = (uint8_t)b0;
                        if (c1) o[rel[u] + 1] = (uint8_t)b1;
                    }
                }
            }
        }
        myrec = nrec, mydesc = ndesc;
    }
    *lp = (unsigned short)(b0 | (b1 << 8));
}

// every byte of every file 0x01 (benches/memfs.rs:118), 8 bytes per lane
__global__ __launch_bounds__(DG_TPB) void mf_fill_kernel(u64* words, u64 n) {
    for (u64 i = blockIdx.x * (u64)DG_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * DG_TPB)
        words[i] = 0x0101010101010101ull;
}

// ---- Sizes (nrg_memfs_enable_sizes): SetAttr { ino, new_attrs } of benches/memfs.rs:26-85, :210-213 as
// ---- ftruncate, and Writes that grow a file ------------------------------------------------------------
// A file has a size 0 .. B beside its capacity B, and EVERY STORED BYTE AT OR PAST THE SIZE IS ZERO. So
// growth and holes cost nothing, a Read is the unsized Read clipped at the size, and only a shrink has to
// erase. A Read's clip, a GetAttr's answer and whether a SetAttr shrinks depend on the size at the
// record's own log position, so a chunk of a sized context runs, in stream order:
//   mfs_keys    one lane per record: its file as a sort key and its function on the size, one word:
//               a valid Write of len > 0 is x -> max(x, offset + len), a valid SetAttr x -> s, every
//               other record the identity (a record that names no file: file 0).
//   file sort   sort_pairs on ceil(log2 F) bits, stable: a file's records in log order. None if F == 1.
//   mfs_reduce / _aggscan / _scan   the segmented exclusive scan of the composed functions over the
//               grouped records in tiles of MFS_TILE, the shape of mf_pread_reduce / _aggscan / _scan;
//               one segment may be the whole chunk. The scan element (mfs_then) carries the size
//               function {constant or max, v}, the shrinks already decided k, their smallest target m
//               and at most one undecided SetAttr t, which shrinks exactly when t < the size at the
//               segment's start; composition is associative, not commutative. _scan evaluates each
//               record's prefix at the file's stored size: sc[i] = {size before, shrinks before},
//               stores a shrink's target at ev[fstart + shrinks before] (fstart: the segment's first
//               grouped position), and the segment's last record writes fm[file] = {fstart, shrinks,
//               smallest target, new size}, stamped with the chunk's epoch. Nothing writes size[] here:
//               every lane of the scan may still read it.
//   mfs_expand  mf_expand with the size before the record for B in Read and GetAttr, and SetAttr.
//   line sort   as above.
//   mfs_lines   mf_lines plus the shrinks. A run's op carries the shrinks of its file before it; when
//               that count passes the count already applied (c0), the wave first zeroes its bytes at or
//               past the smallest target of ev[fstart + c0, fstart + count): right there, since no op
//               touched the line in between and what grew the file afterwards touched other lines or
//               comes later in the run. The check sits in the apply order, not with the MF_AHEAD loads.
//               After the run come the remaining shrinks; a line with no run is cut at fm's smallest
//               target. The range minimum is a forward walk of the file's list, 64 targets per step and
//               one wave reduction: a chunk of E shrinks of one file costs a touched line E / 64 loads
//               and at most min(E, run) reductions. The wave of a file's first line stores the new size.
// What the sized kernels share.
struct MfSz {
    u64* size;        // [F] every file's size; bytes at or past it are zero
    u32* fkey;        // [n] a record's file (0 for a record that names none)
    u32* el;          // [n] a record's function on the size: MFS_CST | s, or the a of max(., a)
    uint2* sc;        // [n] {the size before the record, the shrinks of its file before it in the chunk}
    u32* ev;          // shrink targets, a file's at [fstart, fstart + nev) in log order
    uint4* fm;        // [F] {fstart, nev, the smallest target, the new size} of a file the chunk names
    u32* fep;         // [F] the epoch of the chunk that wrote fm last
    uint4* agg;       // [tiles] scan-tile aggregates
    u32 epoch;
};

// the smallest of ev[c0, c1), the same in every lane (c0 < c1, uniform)
__device__ __forceinline__ u32 mfs_range_min(const u32* __restrict__ ev, u32 c0, u32 c1, u32 lane) {
    u32 mn = 0xFFFFFFFFu;
    for (u32 q = c0 + lane; q < c1; q += 64) mn = min(mn, ev[q]);
#pragma unroll
    for (u32 d = 32; d; d >>= 1) mn = min(mn, (u32)__shfl_xor((int)mn, (int)d, 64));
    return mn;
}

constexpr u32 MFS_ITEMS = 4;
constexpr u32 MFS_TILE = MF_TPB * MFS_ITEMS;
constexpr u32 MFS_NONE = 0xFFFFFFFFu;
constexpr u32 MFS_VMASK = (1u << 30) - 1, MFS_CST = 1u << 30, MFS_HEAD = 1u << 31;
static_assert((1ull << MF_LOG2_MAX) < MFS_VMASK, "a size fits under the flags");

// The scan element: x = v | MFS_CST (the size becomes v; else max(size, v)) | MFS_HEAD (a segment
// starts inside), y = k, z = t (MFS_NONE: none; t set implies MFS_CST), w = m (MFS_NONE: none).
__device__ __forceinline__ uint4 mfs_id() { return make_uint4(0, 0, MFS_NONE, MFS_NONE); }

// F, then G
__device__ __forceinline__ uint4 mfs_then(uint4 F, uint4 G) {
    if (G.x & MFS_HEAD) return G;
    const u32 fv = F.x & MFS_VMASK, gv = G.x & MFS_VMASK;
    u32 k = F.y + G.y, t = F.z, m = F.w < G.w ? F.w : G.w;
    if (G.z != MFS_NONE) {  // G's undecided SetAttr meets F's size: v, or max(x, v) >= v
        if (G.z < fv) k++, m = m < G.z ? m : G.z;
        else if (!(F.x & MFS_CST)) t = G.z;  // still x's to decide (F has no SetAttr: F.z is none)
    }
    const u32 v = (G.x & MFS_CST) ? gv : (fv > gv ? fv : gv);
    return make_uint4((F.x & MFS_HEAD) | ((F.x | G.x) & MFS_CST) | v, k, t, m);
}

__device__ __forceinline__ uint4 mfs_shfl_up(uint4 v, u32 d) {
    return make_uint4(__shfl_up(v.x, d, 64), __shfl_up(v.y, d, 64), __shfl_up(v.z, d, 64), __shfl_up(v.w, d, 64));
}

// exclusive scan of v over the workgroup's threads under mfs_then, and the workgroup's total. s_w:
// MF_TPB / 64 elements; a caller that calls again puts a barrier between the calls.
__device__ __forceinline__ uint4 mfs_block_excl(uint4 v, uint4* s_w, uint4* total) {
    const u32 lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint4 inc = v;
#pragma unroll
    for (u32 d = 1; d < 64; d <<= 1) {
        const uint4 o = mfs_shfl_up(inc, d);
        if (lane >= d) inc = mfs_then(o, inc);
    }
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    uint4 base = mfs_id(), tot = mfs_id();
#pragma unroll
    for (u32 k = 0; k < MF_TPB / 64; k++) {
        const uint4 x = s_w[k];
        if (k < w) base = mfs_then(base, x);
        tot = mfs_then(tot, x);
    }
    *total = tot;
    uint4 prev = mfs_shfl_up(inc, 1);
    if (lane == 0) prev = mfs_id();
    return mfs_then(base, prev);
}

__global__ __launch_bounds__(MF_TPB) void mfs_keys_kernel(MfJob j, MfSz z) {
    const u64 i = (u64)blockIdx.x * MF_TPB + threadIdx.x;
    if (i >= j.n) return;
    const u64* r = mf_rec(j, i);
    const u64 ino = r[0], off = r[1], w2 = r[2];
    const u32 op = (u32)w2, len = (u32)(w2 >> 32);
    const u64 B = j.adm;  // (B itself without a growth bound; a Write of len > 0 that passes ends within B)
    u32 f = 0, e = 0;
    if (op <= NRG_MEMFS_SETATTR && len <= MF_LINE && ino >= NRG_MEMFS_FIRST_INO && ino - NRG_MEMFS_FIRST_INO < j.nfiles) {
        f = (u32)(ino - NRG_MEMFS_FIRST_INO);
        if (op == NRG_MEMFS_WRITE && len && off <= B && len <= B - off) e = (u32)(off + len);
        if (op == NRG_MEMFS_SETATTR && off <= B) e = MFS_CST | (u32)off;
    }
    z.fkey[i] = f;
    z.el[i] = e;
}

// Grouped position p of the chunk: its record, its file and its scan element. gk / gv: the sorted file
// keys and record indices, or nullptr where F == 1 (the log order is the grouped order).
struct MfsIn {
    const u32* gk;
    const u32* gv;
    u64 n;
};
__device__ __forceinline__ uint4 mfs_load(const MfsIn& in, const MfSz& z, u64 p, u32* file, u32* rec) {
    const u32 f = in.gk ? in.gk[p] : 0;
    *file = f;
    *rec = in.gv ? in.gv[p] : (u32)p;
    const bool head = p == 0 || (in.gk && in.gk[p - 1] != f);
    const u32 e = z.el[*rec];
    return make_uint4(e | (head ? MFS_HEAD : 0), 0, (e & MFS_CST) ? (e & MFS_VMASK) : MFS_NONE, MFS_NONE);
}

// agg[tile] = the composition of the tile's elements
__global__ __launch_bounds__(MF_TPB) void mfs_reduce_kernel(MfsIn in, MfSz z) {
    __shared__ uint4 s_w[MF_TPB / 64];
    const u64 first = (u64)blockIdx.x * MFS_TILE + threadIdx.x * MFS_ITEMS;
    uint4 acc = mfs_id();
#pragma unroll
    for (u32 k = 0; k < MFS_ITEMS; k++) {
        u32 f, rec;
        if (first + k < in.n) acc = mfs_then(acc, mfs_load(in, z, first + k, &f, &rec));
    }
    uint4 tot;
    (void)mfs_block_excl(acc, s_w, &tot);
    if (threadIdx.x == 0) z.agg[blockIdx.x] = tot;
}

// agg[tile] = the composition of the tiles before it; one workgroup
__global__ __launch_bounds__(MF_TPB) void mfs_aggscan_kernel(uint4* agg, u32 tiles) {
    __shared__ uint4 s_w[MF_TPB / 64];
    uint4 carry = mfs_id();
    for (u32 b = 0; b < tiles; b += MF_TPB) {
        const u32 i = b + threadIdx.x;
        uint4 tot;
        const uint4 ex = mfs_block_excl(i < tiles ? agg[i] : mfs_id(), s_w, &tot);
        if (i < tiles) agg[i] = mfs_then(carry, ex);
        carry = mfs_then(carry, tot);
        __syncthreads();
    }
}

// the first grouped position of file f (it has one)
__device__ __forceinline__ u32 mfs_first(const MfsIn& in, u32 f) {
    if (!in.gk) return 0;
    u64 lo = 0, hi = in.n;
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (in.gk[mid] < f) lo = mid + 1; else hi = mid;
    }
    return (u32)lo;
}

// sc, ev and fm; carried: agg holds the scanned aggregates (more than one tile)
__global__ __launch_bounds__(MF_TPB) void mfs_scan_kernel(MfsIn in, MfSz z, u32 carried) {
    __shared__ uint4 s_w[MF_TPB / 64];
    const u64 first = (u64)blockIdx.x * MFS_TILE + threadIdx.x * MFS_ITEMS;
    uint4 e[MFS_ITEMS], acc = mfs_id();
    u32 file[MFS_ITEMS], rec[MFS_ITEMS];
#pragma unroll
    for (u32 k = 0; k < MFS_ITEMS; k++) {
        e[k] = mfs_id(), file[k] = rec[k] = 0;
        if (first + k < in.n) e[k] = mfs_load(in, z, first + k, &file[k], &rec[k]);
        acc = mfs_then(acc, e[k]);
    }
    uint4 tot;
    const uint4 ex = mfs_block_excl(acc, s_w, &tot);
    uint4 run = mfs_then(carried ? z.agg[blockIdx.x] : mfs_id(), ex);
#pragma unroll
    for (u32 k = 0; k < MFS_ITEMS; k++) {
        const u64 p = first + k;
        if (p < in.n) {
            const uint4 E = (e[k].x & MFS_HEAD) ? mfs_id() : run;  // the file's records of the chunk before this one
            const u32 x0 = (u32)z.size[file[k]];
            const bool pend = E.z != MFS_NONE && E.z < x0;
            const u32 pv = E.x & MFS_VMASK;
            const u32 sb = (E.x & MFS_CST) ? pv : (x0 > pv ? x0 : pv);
            const u32 cb = E.y + (pend ? 1 : 0);
            z.sc[rec[k]] = make_uint2(sb, cb);
            const u32 s = e[k].x & MFS_VMASK;
            const bool shrink = (e[k].x & MFS_CST) && s < sb;
            const bool last = p + 1 == in.n || (in.gk && in.gk[p + 1] != file[k]);
            if (shrink || last) {
                const u32 fs = mfs_first(in, file[k]);
                if (shrink) z.ev[fs + cb] = s;  // (fs + cb <= p: in bounds)
                if (last) {
                    u32 mn = E.w;
                    if (pend) mn = mn < E.z ? mn : E.z;
                    if (shrink) mn = mn < s ? mn : s;
                    const u32 ns = (e[k].x & MFS_CST) ? s : (sb > s ? sb : s);
                    z.fm[file[k]] = make_uint4(fs, cb + (shrink ? 1 : 0), mn, ns);
                    z.fep[file[k]] = z.epoch;
                }
            }
        }
        run = mfs_then(run, e[k]);
    }
}

// mf_expand of a sized context: sc[i].x is record i's file's size before the record
__global__ __launch_bounds__(MF_TPB) void mfs_expand_kernel(MfJob j, const uint2* __restrict__ sc) {
    __shared__ u64 s_n[MF_TPB];
    const u32 t = threadIdx.x;
    const u64 base = (u64)blockIdx.x * MF_TPB;
    const u32 cnt = j.n - base < MF_TPB ? (u32)(j.n - base) : MF_TPB;
    bool inval = false;
    if (t < cnt) {
        const u64 i = base + t;
        const u64* r = mf_rec(j, i);
        const u64 ino = r[0], off = r[1], w2 = r[2];
        const u32 op = (u32)w2, len = (u32)(w2 >> 32);
        const u64 B = j.adm;  // (as in mfs_keys; a Write of no bytes may lie past B: it touches nothing)
        const u64 size = sc[i].x;
        u64 nresp;
        u32 cover = 0;
        uint8_t sm = 0;
        bool wr = false;
        if (op > NRG_MEMFS_SETATTR || len > MF_LINE) {
            nresp = NRG_MEMFS_EINVAL;
            inval = true;
        } else if (ino < NRG_MEMFS_FIRST_INO || ino - NRG_MEMFS_FIRST_INO >= j.nfiles) {
            nresp = NRG_MEMFS_ENOENT;
        } else if (op == NRG_MEMFS_GETATTR) {  // Attr(FileAttr): the size
            nresp = size, sm = 1;
        } else if (op == NRG_MEMFS_WRITE) {
            if (off <= B && len <= B - off) nresp = len, cover = len, sm = 1, wr = true;  // Written(len)
            else nresp = NRG_MEMFS_EFBIG;
        } else if (op == NRG_MEMFS_SETATTR) {  // Attr: the new size; what a shrink erases is mf_lines' work
            if (off <= B) nresp = off, sm = 1;
            else nresp = NRG_MEMFS_EFBIG;
        } else {  // Data(bytes), clipped at the end of the file
            nresp = off >= size ? 0 : (len < size - off ? len : size - off);
            cover = (u32)nresp, sm = 1;
        }
        u32 k0 = j.nlines, k1 = j.nlines;
        u64 d = 0;
        if (cover) {
            const u64 start = ((ino - NRG_MEMFS_FIRST_INO) << j.log2_b) + off;  // < 2^29
            k0 = (u32)(start >> 7);
            const u32 kl = (u32)((start + cover - 1) >> 7);
            if (kl != k0) k1 = kl;
            d = start | ((u64)cover << 32) | ((u64)(wr ? 1 : 0) << 48);
        }
        *(uint2*)(j.keys + 2 * i) = make_uint2(k0, k1);
        j.desc[i] = d;
        s_n[t] = nresp;
        const u64 g = j.lo + i;
        if (j.resp && g >= j.rlo && g < j.rhi) j.some[g - j.rlo] = sm;
    }
    if (__any(inval) && (t & 63) == 0) atomicOr(&j.ctl->err, ERR_INVAL);
    __syncthreads();
    if (j.src)  // Log::append of a fused round
        for (u32 w = t; w < cnt * MF_REC_WORDS; w += MF_TPB) {
            const u32 rec = w / MF_REC_WORDS, q = w - rec * MF_REC_WORDS;
            j.ring[((j.lo + base + rec) & j.ring_mask) * MF_REC_WORDS + q] = j.src[(base + rec) * MF_REC_WORDS + q];
        }
    if (j.resp)
        for (u32 w = t; w < cnt * MF_RESP_WORDS; w += MF_TPB) {
            const u32 rec = w / MF_RESP_WORDS, q = w - rec * MF_RESP_WORDS;
            const u64 g = j.lo + base + rec;
            if (g >= j.rlo && g < j.rhi) j.resp[(g - j.rlo) * MF_RESP_WORDS + q] = q ? 0 : s_n[rec];
        }
}

// mf_lines of a sized context: the same walk, which also applies the chunk's shrinks in log order.
__global__ __launch_bounds__(MF_TPB) void mfs_lines_kernel(MfJob j, const u32* __restrict__ sk,
                                                           const u32* __restrict__ sv, u32 m, MfSz z) {
    const u32 lane = threadIdx.x & 63;
    const u32 X = __builtin_amdgcn_readfirstlane(blockIdx.x * (MF_TPB / 64) + (threadIdx.x >> 6));
    if (X >= j.nlines) return;
    u32 fstart = 0, nev = 0, fmin = 0xFFFFFFFFu, c0 = 0;  // the file's shrinks; c0: those already applied
    const u32 fx0 = ((X << 7) & ((1u << j.log2_b) - 1)) + 2 * lane;  // this lane's first byte in its file
    const u32 f = X >> (j.log2_b - 7);
    if (z.fep[f] == z.epoch) {  // the chunk names the file
        const uint4 q = z.fm[f];
        fstart = q.x, nev = q.y, fmin = q.z;
        if ((X & ((1u << (j.log2_b - 7)) - 1)) == 0 && lane == 0) z.size[f] = q.w;  // the file's first line commits
    }
    u32 lo = 0, hi = m;
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (sk[mid] < X) lo = mid + 1; else hi = mid;
    }
    const u32 r0 = lo;
    if (r0 >= m || sk[r0] != X) {  // no op of the chunk touches the line
        if (nev && fmin < (fx0 - 2 * lane) + MF_LINE) {  // a shrink of the chunk cuts it
            unsigned short* lp = (unsigned short*)(j.files + (u64)X * MF_LINE) + lane;
            const u32 w = *lp;
            *lp = (unsigned short)((fx0 >= fmin ? 0 : w & 0xFF) | (fx0 + 1 >= fmin ? 0 : w & 0xFF00));
        }
        return;
    }
    lo = r0 + 1, hi = m;
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (sk[mid] <= X) lo = mid + 1; else hi = mid;
    }
    const u32 r1 = lo;
    unsigned short* lp = (unsigned short*)(j.files + (u64)X * MF_LINE) + lane;
    const u32 w = *lp;
    u32 b0 = w & 0xFF, b1 = w >> 8;
    const u32 gx0 = X * MF_LINE + 2 * lane;  // this lane's first byte in the store
    uint8_t* const rbytes = (uint8_t*)j.resp;
    u32 myrec = 0, mycb = 0;  // mycb: the shrinks of the file before the slot's record
    u64 mydesc = 0;
    if (r0 + lane < r1) {
        myrec = sv[r0 + lane] >> 1;
        mydesc = j.desc[myrec];
        mycb = z.sc[myrec].y;
    }
    for (u32 t0 = r0; t0 < r1; t0 += 64) {
        const u32 cnt = r1 - t0 < 64 ? r1 - t0 : 64;
        u32 nrec = 0, ncb = 0;  // the next batch, fetched before this one is walked
        u64 ndesc = 0;
        if (t0 + 64 + lane < r1) {
            nrec = sv[t0 + 64 + lane] >> 1;
            ndesc = j.desc[nrec];
            ncb = z.sc[nrec].y;
        }
        const u32 dlo = (u32)mydesc, dhi = (u32)(mydesc >> 32);  // (lanes at or past cnt hold 0: no bytes)
        for (u32 k = 0; k < cnt; k += MF_AHEAD) {
            u32 rec[MF_AHEAD], rel[MF_AHEAD], cn[MF_AHEAD], d0[MF_AHEAD], d1[MF_AHEAD];
            bool wr[MF_AHEAD];
#pragma unroll
            for (u32 u = 0; u < MF_AHEAD; u++) {
                const u32 st = __builtin_amdgcn_readlane(dlo, k + u), h = __builtin_amdgcn_readlane(dhi, k + u);
                rec[u] = __builtin_amdgcn_readlane(myrec, k + u);
                cn[u] = h & 0xFFFF;
                wr[u] = (h >> 16) != 0;
                rel[u] = gx0 - st;  // byte 0's offset into the op (wraps where the op starts later)
                d0[u] = d1[u] = 0;
                if (wr[u]) {
                    const uint8_t* p = (const uint8_t*)(mf_rec(j, rec[u]) + 3);
                    if (rel[u] < cn[u]) d0[u] = p[rel[u]];
                    if (rel[u] + 1 < cn[u]) d1[u] = p[rel[u] + 1];
                }
            }
#pragma unroll
            for (u32 u = 0; u < MF_AHEAD; u++) {
                const u32 cu = __builtin_amdgcn_readlane(mycb, k + u);
                if (cu > c0) {  // the shrinks between the run's previous op and this one (slots past cnt: 0)
                    const u32 tm = mfs_range_min(z.ev + fstart, c0, cu, lane);
                    b0 = fx0 >= tm ? 0 : b0;
                    b1 = fx0 + 1 >= tm ? 0 : b1;
                    c0 = cu;
                }
                const bool in0 = rel[u] < cn[u], in1 = rel[u] + 1 < cn[u];
                if (wr[u]) {
                    b0 = in0 ? d0[u] : b0;
                    b1 = in1 ? d1[u] : b1;
                } else if (cn[u]) {
                    const u64 g = j.lo + rec[u];
                    if (rbytes && g >= j.rlo && g < j.rhi) {
                        uint8_t* o = rbytes + (g - j.rlo) * sizeof(nrg_memfs_resp) + 8;
                        if (in0) o[rel[u]] = (uint8_t)b0;
                        if (in1) o[rel[u] + 1] = (uint8_t)b1;
                    }
                }
            }
        }
        myrec = nrec, mydesc = ndesc, mycb = ncb;
    }
    if (nev > c0) {  // the shrinks after the run's last op
        const u32 tm = mfs_range_min(z.ev + fstart, c0, nev, lane);
        b0 = fx0 >= tm ? 0 : b0;
        b1 = fx0 + 1 >= tm ? 0 : b1;
    }
    *lp = (unsigned short)(b0 | (b1 << 8));
}

// every size B: the state nrg_memfs_enable_sizes describes is the one it found
__global__ __launch_bounds__(DG_TPB) void mfs_fill_kernel(u64* size, u64 n, u64 B) {
    for (u64 i = blockIdx.x * (u64)DG_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * DG_TPB) size[i] = B;
}

// nrg_restore of a sized image: ERR_INVAL for a size above B or a non-zero byte at or past a file's size
__global__ __launch_bounds__(DG_TPB) void mfs_check_kernel(const u64* words, u64 n, u32 log2_wpf, const u64* size,
                                                           DevCtl* ctl) {
    bool bad = false;
    for (u64 i = blockIdx.x * (u64)DG_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * DG_TPB) {
        const u64 sz = size[i >> log2_wpf], off = (i & ((1ull << log2_wpf) - 1)) * 8, w = words[i];
        if (sz > (8ull << log2_wpf)) bad = true;
        else if (off >= sz) bad |= w != 0;
        else if (off + 8 > sz) bad |= (w >> (8 * (sz - off))) != 0;
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&ctl->err, ERR_INVAL);
}

// ---- Capacity growth (nrg_set_max_capacity, nrg_memfs_reserve): the file system behind benches/memfs.rs
// ---- keeps a file's bytes in a growing vector, so a write past the end extends the file ---------------
// Sized contexts only: every stored byte at or past a size is zero, so the bytes a larger capacity adds
// are zero and nothing else has to be said about them. With a bound of max bytes per file, B after a log
// prefix is max(B at open or the last reserve, the power of two at or above the largest end admitted so
// far) (memfs_plan.hpp mf_rec_need, mf_grow_log2): a maximum, so it does not depend on how the log was
// cut into chunks, and neither does the digest. B changes BEFORE a chunk is replayed, to what the whole
// chunk needs; after that "within B" and "within max" are the same test for every record of the chunk
// that carries bytes, so the line keys and descriptors stay inside the store. The sized kernels test
// against MfJob::adm = max(B, max), which also gives a Write of no bytes or a refused record the same
// answer however the log was cut. While a bound is set and B < max a chunk first runs
//   mf_need   one lane per record: mf_rec_need, a wave reduction, the workgroup's maximum and, where it
//             is above B, one atomicMax into the context's need word (a running maximum: never reset, so
//             no memset rides on the round). The host reads the word back (8 bytes and a stream
//             synchronise, timed as "mf_room") and, where B does not hold it,
//   mf_grow   moves the F files from stride B to stride B' into a new allocation and zeroes each file's
//             tail [B, B') in the same pass: 16-byte loads and stores, grid-stride over the NEW store,
//             no atomics. Then the stream is synchronised (there is no stream-ordered free), the old
//             store freed and log2_b, nlines (the sentinel key) and key_bits follow. Scratch sized by
//             max_batch or by F does not change.
// At B >= max the store is a fixed one and nothing of this is launched or read. A path whose records
// the host planned itself (nrg_memfs_pwrite*) takes the need from its plan, grows once and replays
// with MfHost::planned set: no need kernel, no readback.
__global__ __launch_bounds__(MF_TPB) void mf_need_kernel(MfJob j, u64 max_bytes, u64* need) {
    __shared__ u64 s_w[MF_TPB / 64];
    const u64 i = (u64)blockIdx.x * MF_TPB + threadIdx.x;
    u64 v = 0;
    if (i < j.n) {
        const u64* r = mf_rec(j, i);
        const u64 w2 = r[2];
        v = mfp::mf_rec_need(r[0], r[1], (u32)w2, (u32)(w2 >> 32), j.nfiles, max_bytes);
    }
#pragma unroll
    for (u32 d = 32; d; d >>= 1) {
        const u64 o = __shfl_xor(v, (int)d, 64);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 m = 0;
#pragma unroll
        for (u32 k = 0; k < MF_TPB / 64; k++) m = s_w[k] > m ? s_w[k] : m;
        if (m > (1ull << j.log2_b)) atomicMax((unsigned long long*)need, (unsigned long long)m);
    }
}

// to: F files of 16 << to_l4 bytes; from: the same files of 16 << from_l4 (from_l4 < to_l4). n: the
// 16-byte units of `to`.
__global__ __launch_bounds__(DG_TPB) void mf_grow_kernel(const uint4* __restrict__ from, uint4* __restrict__ to, u64 n,
                                                         u32 from_l4, u32 to_l4) {
    for (u64 i = blockIdx.x * (u64)DG_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * DG_TPB) {
        const u64 f = i >> to_l4, w = i & ((1ull << to_l4) - 1);
        to[i] = w < (1ull << from_l4) ? from[(f << from_l4) + w] : make_uint4(0, 0, 0, 0);
    }
}

// ---- read-only reads (nrg_memfs_pread*): Replica::execute -> read_only of nr/src/replica.rs:483-497
// ---- for benches/nrfs.rs:88-101 OpRd::FileRead, here pread of any length ---------------------------
// n requests {ino, offset, len} against the store as it stands; the answers packed in request order.
// A request may be of 0 bytes or of a whole 64-MiB file, so no lane, wave or workgroup is given a
// request: the clipped lengths are scanned into d_offs, then the OUTPUT is cut into tiles.
//   mf_pread_reduce / _aggscan / _scan   the exclusive u64 scan of the clipped lengths in tiles of
//              MF_PR_SCAN requests, three launches in stream order, no workgroup waiting on another;
//              n <= MF_PR_SCAN is the one launch of _scan. _scan also writes some and offs[n].
//   mf_pread_copy   one workgroup per MF_PREAD_TILE bytes of output (grid-stride over the tiles that
//              exist: the grid is sized from the host's bound, the total is read from offs[n]). The
//              workgroup finds the first and last request of its tile by upper-bound searches of
//              d_offs (an upper bound: a run of empty requests at a position is skipped whole). The
//              tile is cut into the destination's aligned 16-byte chunks, lane after lane; a lane
//              finds its chunk's request by the same search inside the tile's range. A chunk that lies
//              inside one request is two aligned 16-byte loads around the source, a byte shift and
//              one 16-byte store; any other chunk (a request boundary inside it, the head or tail of
//              the output) is gathered byte by byte, stepping to the next request, or searching for it
//              where the next is empty, and stored whole when all 16 bytes are output bytes.
//              Plain loads and stores; no LDS, no atomics, no spinning.
// The kernels are templates over where a request's count and bytes come from. PACKED = false is the
// store, above. PACKED = true is the re-pack of a group-wide pread (nrg_memfs_pread_repack_async,
// group_file_reads.cpp): the owners' answers lie packed in PARTITION order in a buffer, position p
// holding src_cnt[p] bytes, and request i sits at p = pos[i]. The scan then sums src_cnt (once in
// partition order for the positions' offsets src_offs, once through pos for offs) and the copy is the
// same variable-length move with the source address src + src_offs[pos[r]] instead of the file's: one
// kernel, balanced over the tiles of the OUTPUT either way. The wide path reads the aligned 16-byte
// blocks around a source byte, so a packed source is 16-byte aligned and readable up to the next
// multiple of 16 past its end, as a file is by its size.
constexpr u32 MF_PR_ITEMS = 4;                      // requests per lane of the scan
constexpr u32 MF_PR_SCAN = MF_TPB * MF_PR_ITEMS;    // requests per scan tile
constexpr u32 MF_PREAD_TILE = 16384;                // output bytes per copy workgroup (measured)
constexpr u32 MF_PR_MAX_GRID = 1u << 20;            // copy workgroups at most; the tiles are strided over
static_assert(MF_PREAD_TILE == NRG_MF_PREAD_TILE, "the tests place requests around this tile");
static_assert(MF_PREAD_TILE % (16 * MF_TPB) == 0, "every lane takes the same number of 16-byte chunks");
static_assert(sizeof(nrg_memfs_rd) == 24, "ABI");

struct MfRdJob {
    const u64* rq;   // the requests in u64 words: ino, offset, len
    u64 n;
    u64* offs;       // [n + 1]
    uint8_t* some;   // [n]
    uint8_t* data;   // the packed output
    u64 cap;
    const uint8_t* files;
    u32 log2_b, nfiles;
    const u64* size;  // a sized context's sizes: the clip (nullptr: B)
    u64* cnt;         // [n] every request's clipped length as well (nullptr: not wanted)
    // A packed source instead of the store (PACKED kernels, the re-pack of a group-wide pread): request
    // i's answer is the src_cnt[p] bytes at src + src_offs[p] and the byte src_some[p], p = pos[i]
    // (pos == nullptr: p = i; src_some == nullptr: 1; some == nullptr: not written).
    const uint8_t* src;
    const u64 *src_offs, *src_cnt;
    const uint8_t* src_some;
    const u32* pos;
};

// request i's clipped length; ok: its ino names a file. PACKED: what its owner counted and answered
// (a position outside [0, n) is no request's: nothing).
template <bool PACKED>
__device__ __forceinline__ u64 mf_rd_count(const MfRdJob& j, u64 i, bool* ok) {
    if constexpr (PACKED) {
        const u64 p = j.pos ? j.pos[i] : i;
        *ok = p < j.n && (!j.src_some || j.src_some[p]);
        return p < j.n ? j.src_cnt[p] : 0;
    }
    const u64 ino = j.rq[3 * i], off = j.rq[3 * i + 1], len = j.rq[3 * i + 2];
    *ok = ino >= NRG_MEMFS_FIRST_INO && ino - NRG_MEMFS_FIRST_INO < j.nfiles;
    if (!*ok) return 0;
    const u64 B = j.size ? j.size[ino - NRG_MEMFS_FIRST_INO] : 1ull << j.log2_b;
    return off >= B ? 0 : (len < B - off ? len : B - off);
}

// exclusive scan of v over the workgroup's threads, and the workgroup's total. s_w: MF_TPB / 64 words;
// a caller that calls again puts a barrier between the calls.
__device__ __forceinline__ u64 mf_block_excl(u64 v, u64* s_w, u64* total) {
    const u32 lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    u64 inc = v;
#pragma unroll
    for (u32 d = 1; d < 64; d <<= 1) {
        const u64 o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    u64 base = 0, tot = 0;
#pragma unroll
    for (u32 k = 0; k < MF_TPB / 64; k++) {
        const u64 x = s_w[k];
        if (k < w) base += x;
        tot += x;
    }
    *total = tot;
    return base + inc - v;
}

// agg[tile] = the sum of the tile's clipped lengths
template <bool PACKED>
__global__ __launch_bounds__(MF_TPB) void mf_pread_reduce_kernel(MfRdJob j, u64* agg) {
    __shared__ u64 s_w[MF_TPB / 64];
    const u64 first = (u64)blockIdx.x * MF_PR_SCAN + threadIdx.x * MF_PR_ITEMS;
    u64 sum = 0;
#pragma unroll
    for (u32 k = 0; k < MF_PR_ITEMS; k++) {
        bool ok;
        if (first + k < j.n) sum += mf_rd_count<PACKED>(j, first + k, &ok);
    }
    u64 tot;
    (void)mf_block_excl(sum, s_w, &tot);
    if (threadIdx.x == 0) agg[blockIdx.x] = tot;
}

// agg[tile] = the sum of the tiles before it; one workgroup
__global__ __launch_bounds__(MF_TPB) void mf_pread_aggscan_kernel(u64* agg, u32 tiles) {
    __shared__ u64 s_w[MF_TPB / 64];
    u64 carry = 0;
    for (u32 b = 0; b < tiles; b += MF_TPB) {
        const u32 i = b + threadIdx.x;
        u64 tot;
        const u64 ex = mf_block_excl(i < tiles ? agg[i] : 0, s_w, &tot);
        if (i < tiles) agg[i] = carry + ex;
        carry += tot;
        __syncthreads();
    }
}

// some[i], offs[i] and offs[n]; agg: the scanned aggregates, or nullptr for a single tile
template <bool PACKED>
__global__ __launch_bounds__(MF_TPB) void mf_pread_scan_kernel(MfRdJob j, const u64* agg) {
    __shared__ u64 s_w[MF_TPB / 64];
    const u64 first = (u64)blockIdx.x * MF_PR_SCAN + threadIdx.x * MF_PR_ITEMS;
    u64 c[MF_PR_ITEMS], sum = 0;
#pragma unroll
    for (u32 k = 0; k < MF_PR_ITEMS; k++) {
        c[k] = 0;
        if (first + k < j.n) {
            bool ok;
            c[k] = mf_rd_count<PACKED>(j, first + k, &ok);
            if (!PACKED || j.some) j.some[first + k] = ok ? 1 : 0;
            if (!PACKED && j.cnt) j.cnt[first + k] = c[k];
        }
        sum += c[k];
    }
    u64 tot;
    u64 run = mf_block_excl(sum, s_w, &tot) + (agg ? agg[blockIdx.x] : 0);
#pragma unroll
    for (u32 k = 0; k < MF_PR_ITEMS; k++)
        if (first + k < j.n) {
            j.offs[first + k] = run;
            run += c[k];
            if (first + k == j.n - 1) j.offs[j.n] = run;
        }
}

// the first index i of [lo, hi] with offs[i] > p; offs[hi] > p holds
__device__ __forceinline__ u64 mf_upper(const u64* offs, u64 lo, u64 hi, u64 p) {
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (offs[mid] <= p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// where the first byte of request r's answer lies (r has bytes): in the store, or PACKED in src
template <bool PACKED>
__device__ __forceinline__ const uint8_t* mf_rd_src(const MfRdJob& j, u64 r) {
    if constexpr (PACKED) return j.src + j.src_offs[j.pos[r]];
    return j.files + ((j.rq[3 * r] - NRG_MEMFS_FIRST_INO) << j.log2_b) + j.rq[3 * r + 1];
}

// Positions below are packed positions plus mis = data & 15, so that a multiple of 16 is an aligned
// address of the output: the output bytes are [mis, aend). The kernel is the same for both sources: a
// PACKED one is 16-byte aligned and readable up to the next multiple of 16 past its end, as a file is.
template <bool PACKED>
__global__ __launch_bounds__(MF_TPB) void mf_pread_copy_kernel(MfRdJob j) {
    const u64* __restrict__ offs = j.offs;
    const u64 total = offs[j.n];
    const u64 end = total < j.cap ? total : j.cap;
    if (end == 0) return;
    const u64 mis = (uintptr_t)j.data & 15;
    uint8_t* const out = j.data - mis;
    const u64 aend = end + mis;
    const u64 ntiles = (aend + MF_PREAD_TILE - 1) / MF_PREAD_TILE;
    for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const u64 a0 = tile * MF_PREAD_TILE;
        const u64 a1 = a0 + MF_PREAD_TILE < aend ? a0 + MF_PREAD_TILE : aend;
        const u64 v0 = a0 > mis ? a0 : mis;  // the tile's output bytes are [v0, a1), not empty
        // requests r_first .. r_last - 1 hold them (the same in every lane)
        const u64 r_first = mf_upper(offs, 1, j.n, v0 - mis) - 1;
        const u64 r_last = mf_upper(offs, r_first + 1, j.n, a1 - 1 - mis);
        for (u64 a = a0 + 16 * threadIdx.x; a < a1; a += 16 * MF_TPB) {
            const u64 lo = a > v0 ? a : v0, hi = a + 16 < a1 ? a + 16 : a1;  // the chunk's output bytes
            u64 r = mf_upper(offs, r_first + 1, r_last, lo - mis) - 1;
            u64 rl = offs[r] + mis, rh = offs[r + 1] + mis;  // request r's bytes: rl <= lo < rh
            const uint8_t* src = mf_rd_src<PACKED>(j, r);
            const bool whole = hi - lo == 16;
            if (whole && a + 16 <= rh) {  // inside one request
                const uint8_t* s = src + (a - rl);
                const u32 sh = (u32)((uintptr_t)s & 15);
                const ulonglong2 x = *(const ulonglong2*)(s - sh);
                u64 w0 = x.x, w1 = x.y;
                if (sh) {  // (the chunk's last byte lies in the second 16 bytes: inside the file or the source)
                    const ulonglong2 y = *(const ulonglong2*)(s - sh + 16);
                    u64 w2 = y.x;
                    if (sh >= 8) w0 = w1, w1 = y.x, w2 = y.y;
                    const u32 b = (sh & 7) * 8;
                    if (b) {
                        w0 = (w0 >> b) | (w1 << (64 - b));
                        w1 = (w1 >> b) | (w2 << (64 - b));
                    }
                }
                *(ulonglong2*)(out + a) = make_ulonglong2(w0, w1);
                continue;
            }
            u64 w0 = 0, w1 = 0;
            for (u64 q = lo; q < hi; q++) {
                if (q >= rh) {  // the next request that has bytes
                    r++;
                    rl = rh, rh = offs[r + 1] + mis;
                    if (rh <= q) {  // an empty one: search past the run
                        r = mf_upper(offs, r + 1, r_last, q - mis) - 1;
                        rl = offs[r] + mis, rh = offs[r + 1] + mis;
                    }
                    src = mf_rd_src<PACKED>(j, r);
                }
                const u64 byte = src[q - rl];
                const u32 k = (u32)(q - a);
                if (k < 8) w0 |= byte << (8 * k); else w1 |= byte << (8 * (k - 8));
            }
            if (whole) {
                *(ulonglong2*)(out + a) = make_ulonglong2(w0, w1);
            } else {
                for (u64 q = lo; q < hi; q++) {
                    const u32 k = (u32)(q - a);
                    out[q] = (uint8_t)(k < 8 ? w0 >> (8 * k) : w1 >> (8 * (k - 8)));
                }
            }
        }
    }
}

// out[s] = the bytes this owner answers asker s with, from the scanned offsets at the asker boundaries:
// it holds the requests of rank 0, then rank 1, ..., and allcnt (every rank's exchange words, cw per
// rank, its requests per owner first) says how many of each. One thread per asker.
__global__ void mf_pread_totals_kernel(const u64* __restrict__ offs, u64 recvd, const u64* __restrict__ allcnt, u32 G,
                                       u32 cw, u32 rank, u64* __restrict__ out) {
    const u32 s = threadIdx.x;
    if (s >= G) return;
    u64 lo = 0;
    for (u32 q = 0; q < s; q++) lo += allcnt[(u64)q * cw + rank];
    u64 hi = lo + allcnt[(u64)s * cw + rank];
    lo = lo < recvd ? lo : recvd;  // (the plan gives hi <= recvd: the bound keeps the loads inside offs)
    hi = hi < recvd ? hi : recvd;
    out[s] = offs[hi] - offs[lo];
}

// ---- the launchers of the kernels above: nrg_memfs_pread_async, nrg_memfs_pread_repack_async and the
// ---- replica group's group-wide pread (group_file_reads.cpp), which brings its own scratch -----------
static MfRdJob mf_rd_job(const nrg_ctx* c, u64 n, u64* offs, uint8_t* some) {
    MfRdJob j{};
    j.n = n;
    j.offs = offs;
    j.some = some;
    j.files = c->mf.d_files;
    j.log2_b = c->mf.log2_b;
    j.nfiles = (u32)c->mf.files;
    j.size = c->mf.d_size;
    return j;
}

template <bool PACKED>
static hipError_t mf_scan_launch(nrg_ctx* c, const MfRdJob& j, u64* agg) {
    if (j.n == 0) return j.offs ? hipMemsetAsync(j.offs, 0, sizeof(u64), c->stream) : hipSuccess;
    const unsigned tiles = (unsigned)((j.n + MF_PR_SCAN - 1) / MF_PR_SCAN);
    if (tiles > 1) {
        NRG_LAUNCH(c, PACKED ? "mf_repack_reduce" : "mf_pread_reduce", mf_pread_reduce_kernel<PACKED>, tiles, MF_TPB, 0,
                   c->stream, j, agg);
        NRG_LAUNCH(c, PACKED ? "mf_repack_aggscan" : "mf_pread_aggscan", mf_pread_aggscan_kernel, 1, MF_TPB, 0, c->stream,
                   agg, (u32)tiles);
    }
    NRG_LAUNCH(c, PACKED ? "mf_repack_scan" : "mf_pread_scan", mf_pread_scan_kernel<PACKED>, tiles, MF_TPB, 0, c->stream, j,
               tiles > 1 ? (const u64*)agg : (const u64*)nullptr);
    return hipGetLastError();
}

// one workgroup per tile of the `bound` bytes the host knows the output cannot exceed (the tiles that
// exist are strided over, surplus workgroups exit)
template <bool PACKED>
static hipError_t mf_copy_launch(nrg_ctx* c, const MfRdJob& j, u64 bound) {
    if (j.n == 0 || bound == 0) return hipSuccess;
    const u64 ct = (bound + 15 + MF_PREAD_TILE - 1) / MF_PREAD_TILE;
    NRG_LAUNCH(c, PACKED ? "mf_repack_copy" : "mf_pread_copy", mf_pread_copy_kernel<PACKED>,
               (unsigned)(ct < MF_PR_MAX_GRID ? ct : MF_PR_MAX_GRID), MF_TPB, 0, c->stream, j);
    return hipGetLastError();
}

u64 mf_pread_agg_words(u64 n) { return (n + MF_PR_SCAN - 1) / MF_PR_SCAN; }

// the most bytes n requests can answer, or cap if that is less
u64 mf_pread_bound(const nrg_ctx* c, u64 n, u64 cap) {
    const u32 lb = c->mf.log2_b;
    return n > (~0ull >> lb) || (n << lb) > cap ? cap : n << lb;
}

hipError_t mf_pread_scan_launch(nrg_ctx* c, const nrg_memfs_rd* d_reqs, u64 n, u64* d_offs, uint8_t* d_some, u64* d_cnt,
                                u64* d_agg) {
    MfRdJob j = mf_rd_job(c, n, d_offs, d_some);
    j.rq = (const u64*)d_reqs;
    j.cnt = d_cnt;
    return mf_scan_launch<false>(c, j, d_agg);
}

hipError_t mf_pread_copy_launch(nrg_ctx* c, const nrg_memfs_rd* d_reqs, u64 n, const u64* d_offs, uint8_t* d_data, u64 cap,
                                u64 bound) {
    MfRdJob j = mf_rd_job(c, n, const_cast<u64*>(d_offs), nullptr);
    j.rq = (const u64*)d_reqs;
    j.data = d_data;
    j.cap = cap;
    return mf_copy_launch<false>(c, j, bound);
}

hipError_t mf_pread_totals_launch(nrg_ctx* c, const u64* d_offs, u64 recvd, const u64* d_allcnt, u32 G, u32 cw, u32 rank,
                                  u64* d_out) {
    if (G == 0 || G > 64) return hipErrorInvalidValue;
    NRG_LAUNCH(c, "mf_pread_totals", mf_pread_totals_kernel, 1, 64, 0, c->stream, d_offs, recvd, d_allcnt, G, cw, rank,
               d_out);
    return hipGetLastError();
}

hipError_t mf_repack_scan_launch(nrg_ctx* c, const u64* d_src_cnt, const uint8_t* d_src_some, const u32* d_pos, u64 n,
                                 u64* d_offs, uint8_t* d_some, u64* d_src_offs, u64* d_agg) {
    // where each position's bytes begin in the source: the scan of the counts in partition order
    MfRdJob a = mf_rd_job(c, n, d_src_offs, nullptr);
    a.src_cnt = d_src_cnt;
    hipError_t e = mf_scan_launch<true>(c, a, d_agg);
    if (e != hipSuccess) return e;
    // ... and in the output: the scan of the same counts in request order, with the some bytes
    MfRdJob b = mf_rd_job(c, n, d_offs, d_some);
    b.src_cnt = d_src_cnt;
    b.src_some = d_src_some;
    b.pos = d_pos;
    return mf_scan_launch<true>(c, b, d_agg);
}

hipError_t mf_repack_copy_launch(nrg_ctx* c, const uint8_t* d_src, const u64* d_src_offs, const u32* d_pos, u64 n,
                                 const u64* d_offs, uint8_t* d_data, u64 cap, u64 bound) {
    MfRdJob j = mf_rd_job(c, n, const_cast<u64*>(d_offs), nullptr);
    j.src = d_src;
    j.src_offs = d_src_offs;
    j.pos = d_pos;
    j.data = d_data;
    j.cap = cap;
    return mf_copy_launch<true>(c, j, bound);
}

// ---- writes of any length (nrg_memfs_pwrite*): Replica::combine for benches/nrfs.rs:103-115
// ---- OpWr::FileWrite, here pwrite of any length ------------------------------------------------------
// A long write is a contiguous run of ordinary Write records, cut at the file's 128-byte lines
// (memfs_plan.hpp: the host plans first[0..n], the running sum of the requests' record counts, before
// anything is queued). A request may be of 0 bytes or of a whole 64-MiB file, so no lane, wave or
// workgroup is given a request: the OUTPUT is cut, the twin of mf_pread_copy.
//   mf_frag   fragment records [t0, t1) of the call, each to record (pos0 + t - t0) & mask of dst: the
//             log ring at the tail, or the caller's linear buffer. A workgroup takes MF_FR_TILE
//             fragments and finds the first and last request of its tile by upper-bound searches of
//             first[] (the same in every lane; every request has at least one record, so a fragment has
//             exactly one request). MF_FR_LANES = 16 lanes take one fragment: the same search inside the
//             tile's range (uniform within the 16), the request's four words, the cut (memfs_plan.hpp
//             cut_of / frag_of, the host's own arithmetic); lane l then stores data word l, the first
//             three lanes a header word each, the first lane of a request's first fragment its written
//             and some. A record is 8-byte aligned (152 = 19 * 8) and its data starts at byte 24, so the
//             widest aligned store is 8 bytes: 16 lanes store a record's 128 data bytes as one contiguous
//             run. The source data + data_off + ... has any alignment: a lane reads the one or two
//             aligned 8-byte words that hold its bytes and shifts, never a word that is not wholly
//             inside [data, data + data_bytes): the head and the last bytes of data, where such a word
//             would reach outside, are gathered byte by byte. Bytes past the record's len are zero.
//             Plain loads and stores; no LDS, no atomics, no spinning.
constexpr u32 MF_FR_LANES = 16;                      // lanes of one fragment: one per 8-byte data word
constexpr u32 MF_FR_PER_WG = MF_TPB / MF_FR_LANES;   // fragments a workgroup writes at a time
constexpr u32 MF_FR_TILE = 4 * MF_FR_PER_WG;         // fragments per workgroup
static_assert(MF_FR_LANES * 8 == MF_LINE && MF_REC_WORDS == 3 + MF_FR_LANES, "one lane per data word of a record");
static_assert(sizeof(nrg_memfs_wr) == 32, "ABI");
static_assert(mfp::LINE == MF_LINE && mfp::LOG2_MIN == MF_LOG2_MIN && mfp::LOG2_MAX == MF_LOG2_MAX &&
                  mfp::MAX_FILES == MF_MAX_FILES && mfp::MAX_BYTES == MF_MAX_BYTES,
              "the plan's geometry is nrg_open's");

struct MfWrJob {
    const u64* rq;     // the requests in u64 words: ino, offset, len, data_off
    const u64* first;  // [n + 1] the running sum of the requests' record counts
    u64 n;
    u64 t0, t1;        // the fragments of this launch
    u64* dst;          // records in u64 words
    u64 pos0, mask;    // fragment t is record (pos0 + t - t0) & mask of dst
    const uint8_t* data;
    u64 data_bytes;
    u32 log2_b, nfiles;
    u64* written;      // [n] (nullptr with some: not wanted)
    uint8_t* some;
};

__global__ __launch_bounds__(MF_TPB) void mf_frag_kernel(MfWrJob j) {
    const u64* __restrict__ first = j.first;
    const u32 sub = threadIdx.x & (MF_FR_LANES - 1), grp = threadIdx.x / MF_FR_LANES;
    const u64 a0 = j.t0 + (u64)blockIdx.x * MF_FR_TILE;
    if (a0 >= j.t1) return;
    const u64 a1 = a0 + MF_FR_TILE < j.t1 ? a0 + MF_FR_TILE : j.t1;
    // requests r_first .. r_last - 1 hold the tile's fragments (the same in every lane)
    const u64 r_first = mf_upper(first, 1, j.n, a0) - 1;
    const u64 r_last = mf_upper(first, r_first + 1, j.n, a1 - 1);
    const uint8_t* const dend = j.data + j.data_bytes;
    for (u64 t = a0 + grp; t < a1; t += MF_FR_PER_WG) {
        const u64 r = mf_upper(first, r_first + 1, r_last, t) - 1;  // first[r] <= t < first[r + 1]
        const u64 ino = j.rq[4 * r], off = j.rq[4 * r + 1], len = j.rq[4 * r + 2];
        const mfp::Cut c = mfp::cut_of(j.log2_b, j.nfiles, ino, off, len);
        const u64 k = t - first[r];
        u64 roff, src;
        u32 rlen;
        mfp::frag_of(j.log2_b, c.kind, off, len, k, &roff, &rlen, &src);
        u64* rec = j.dst + ((j.pos0 + (t - j.t0)) & j.mask) * MF_REC_WORDS;
        u64 w = 0;
        const u32 b0 = 8 * sub;  // this lane's first byte of the record's data
        if (c.kind == mfp::CUT_BYTES && b0 < rlen) {
            const u32 cnt = rlen - b0 < 8 ? rlen - b0 : 8;
            const uint8_t* s = j.data + j.rq[4 * r + 3] + src + b0;  // [s, s + cnt) lies inside data (the plan)
            const u32 sh = (u32)((uintptr_t)s & 7);
            const uint8_t* a = s - sh;  // the aligned words of the first and the last byte
            const uint8_t* al = s + cnt - 1 - ((uintptr_t)(s + cnt - 1) & 7);
            if (a >= j.data && al + 8 <= dend) {
                w = *(const u64*)a;
                if (sh) {
                    w >>= 8 * sh;
                    if (al != a) w |= *(const u64*)al << (64 - 8 * sh);
                }
            } else {  // the head or the last bytes of data
                for (u32 q = 0; q < cnt; q++) w |= (u64)s[q] << (8 * q);
            }
            if (cnt < 8) w &= (1ull << (8 * cnt)) - 1;
        }
        rec[3 + sub] = w;
        if (sub < 3) rec[sub] = sub == 0 ? ino : (sub == 1 ? roff : (u64)NRG_MEMFS_WRITE | ((u64)rlen << 32));
        if (sub == 0 && k == 0 && j.written) {
            j.written[r] = c.written;
            j.some[r] = c.some;
        }
    }
}

// ---- logged reads of any length (nrg_memfs_pread_logged*): memfs.rs:73-78, :267-282 OperationWr::Read
// ---- with a size of any length, the read the structure is named for ---------------------------------
// A long read is a contiguous run of ordinary Read records, one per 128-byte line of what the request
// plans to read (memfs_plan.hpp rcut_of: planned = min(len, A - offset), A the admission bound); request i
// owns the slot [offs[i], offs[i + 1]) of the caller's buffer, offs the running sum of planned. first[]
// and offs[] are host arithmetic, uploaded with the requests. The run is replayed by mf_expand / mf_lines
// (or their sized twins) like any other records; one pass's 136-byte responses go to library scratch and
// from there into the slots.
//   mf_rfrag    mf_frag's twin without a data source: fragments [t0, t1) of the uploaded call to records
//               (pos0 + t - t0) & mask of dst, the same tile and 16-lane shape, the request found by the
//               same upper-bound search of first[]. Three header words and sixteen zero data words, as
//               8-byte stores: the ring holds what MemFs.encode makes of an MfRead.
//   mf_rgather  cut by OUTPUT, as mf_pread_copy is: the slot bytes [p0, p1) that fragments [t0, t1) own
//               are cut into MF_RG_TILE-byte tiles of the destination's aligned 8-byte words, one word
//               per lane and step. A workgroup finds the first and last request of its tile by upper-bound
//               searches of offs[] (a run of empty slots is skipped whole), a lane its word's request by
//               the same search inside that range. Byte q of request i's slot is byte idx of fragment
//               k = ((offset + q) >> 7) - (offset >> 7) (memfs_plan.hpp rfrag_at) and is copied iff idx is
//               below that response's n. A word whose 8 bytes lie in one fragment below its n is the one
//               or two aligned 8-byte loads around the source, a shift and one 8-byte store; any other
//               word (a fragment or request boundary, the clip, the ragged ends of the pass) goes byte by
//               byte, and only the bytes that pass the test are stored. Nothing outside
//               [offs[i], offs[i] + count_i) is written.
//   mf_rcount   one lane per request that has fragments in [t0, t1): its fragments' n are full, then at
//               most one partial, then zero, so the sum is a binary search for the first fragment that is
//               not full. The pass that holds a request's first fragment stores count and some; a later
//               pass adds, in stream order.
// Plain loads and stores; no LDS, no atomics, no spinning.
constexpr u32 MF_RG_TILE = 8 * MF_TPB * 4;  // slot bytes per gather workgroup: four words per lane
constexpr u32 MF_RG_MAX_GRID = 1u << 20;    // gather workgroups at most; the tiles are strided over

struct MfRlJob {
    const u64* rq;     // the requests in u64 words: ino, offset, len
    const u64* first;  // [n + 1] the running sum of the requests' record counts
    const u64* offs;   // [n + 1] the running sum of planned
    u64 n;
    u64 t0, t1;        // the fragments of this launch
    u64* dst;          // mf_rfrag: records in u64 words
    u64 pos0, mask;    //           fragment t is record (pos0 + t - t0) & mask of dst
    u32 log2_adm, nfiles;
    const u64* resp;   // mf_rgather / mf_rcount: fragment t's response is resp + (t - t0) * MF_RESP_WORDS
    const uint8_t* rsome;
    uint8_t* data;     // the slots
    u64 p0, p1;        // the slot bytes fragments [t0, t1) own
    u64* cnt;          // [n]
    uint8_t* some;     // [n]
    u64 r0, nr;        // mf_rcount: requests [r0, r0 + nr) have fragments in [t0, t1)
};

__global__ __launch_bounds__(MF_TPB) void mf_rfrag_kernel(MfRlJob j) {
    const u64* __restrict__ first = j.first;
    const u32 sub = threadIdx.x & (MF_FR_LANES - 1), grp = threadIdx.x / MF_FR_LANES;
    const u64 a0 = j.t0 + (u64)blockIdx.x * MF_FR_TILE;
    if (a0 >= j.t1) return;
    const u64 a1 = a0 + MF_FR_TILE < j.t1 ? a0 + MF_FR_TILE : j.t1;
    const u64 r_first = mf_upper(first, 1, j.n, a0) - 1;
    const u64 r_last = mf_upper(first, r_first + 1, j.n, a1 - 1);
    for (u64 t = a0 + grp; t < a1; t += MF_FR_PER_WG) {
        const u64 r = mf_upper(first, r_first + 1, r_last, t) - 1;  // first[r] <= t < first[r + 1]
        const u64 ino = j.rq[3 * r], off = j.rq[3 * r + 1], len = j.rq[3 * r + 2];
        const mfp::RCut c = mfp::rcut_of(j.log2_adm, j.nfiles, ino, off, len);
        u64 roff;
        u32 rlen;
        mfp::rfrag_of(c, off, t - first[r], &roff, &rlen);
        u64* rec = j.dst + ((j.pos0 + (t - j.t0)) & j.mask) * MF_REC_WORDS;
        rec[3 + sub] = 0;
        if (sub < 3) rec[sub] = sub == 0 ? ino : (sub == 1 ? roff : (u64)NRG_MEMFS_READ | ((u64)rlen << 32));
    }
}

// Positions below are slot positions plus mis = data & 7, so that a multiple of 8 is an aligned address
// of the output.
__global__ __launch_bounds__(MF_TPB) void mf_rgather_kernel(MfRlJob j) {
    const u64* __restrict__ offs = j.offs;
    const u64 mis = (uintptr_t)j.data & 7;
    uint8_t* const out = j.data - mis;
    const u64 v0 = j.p0 + mis, v1 = j.p1 + mis;  // this launch's bytes, not empty
    const u64 w0 = v0 & ~7ull;
    const u64 ntiles = (v1 - w0 + MF_RG_TILE - 1) / MF_RG_TILE;
    const uint8_t* const rbytes = (const uint8_t*)j.resp;
    for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const u64 a0 = w0 + tile * MF_RG_TILE;
        const u64 a1 = a0 + MF_RG_TILE < v1 ? a0 + MF_RG_TILE : v1;
        const u64 b0 = a0 > v0 ? a0 : v0;  // the tile's bytes are [b0, a1), not empty
        // requests r_first .. r_last - 1 hold them (the same in every lane)
        const u64 r_first = mf_upper(offs, 1, j.n, b0 - mis) - 1;
        const u64 r_last = mf_upper(offs, r_first + 1, j.n, a1 - 1 - mis);
        for (u64 a = a0 + 8 * threadIdx.x; a < a1; a += 8 * MF_TPB) {
            const u64 lo = a > b0 ? a : b0, hi = a + 8 < a1 ? a + 8 : a1;  // the word's bytes of this launch
            u64 r = mf_upper(offs, r_first + 1, r_last, lo - mis) - 1;
            u64 rl = offs[r] + mis, rh = offs[r + 1] + mis;  // request r's slot: rl <= lo < rh
            u64 off = j.rq[3 * r + 1];
            u32 idx;
            u64 k = mfp::rfrag_at(off, lo - rl, &idx);
            const uint8_t* rp = rbytes + (j.first[r] + k - j.t0) * sizeof(nrg_memfs_resp);
            u64 nn = *(const u64*)rp;
            if (hi - lo == 8 && a + 8 <= rh && idx + 8 <= MF_LINE && (u64)idx + 8 <= nn) {  // inside one fragment's bytes
                const uint8_t* s = rp + 8 + idx;
                const u32 sh = idx & 7;  // (a response and its data are 8-byte aligned)
                u64 w = *(const u64*)(s - sh);
                if (sh) w = (w >> (8 * sh)) | (*(const u64*)(s - sh + 8) << (64 - 8 * sh));  // (within data: idx + 8 <= 128)
                *(u64*)(out + a) = w;
                continue;
            }
            for (u64 q = lo; q < hi; q++) {
                bool moved = false;
                if (q >= rh) {  // the next request that has a slot
                    r++;
                    rl = rh, rh = offs[r + 1] + mis;
                    if (rh <= q) {  // an empty one: search past the run
                        r = mf_upper(offs, r + 1, r_last, q - mis) - 1;
                        rl = offs[r] + mis, rh = offs[r + 1] + mis;
                    }
                    off = j.rq[3 * r + 1];
                    moved = true;
                }
                u32 ix;
                const u64 kq = mfp::rfrag_at(off, q - rl, &ix);
                if (moved || kq != k) {
                    k = kq;
                    rp = rbytes + (j.first[r] + k - j.t0) * sizeof(nrg_memfs_resp);
                    nn = *(const u64*)rp;
                }
                if (ix < nn) out[q] = rp[8 + ix];
            }
        }
    }
}

__global__ __launch_bounds__(MF_TPB) void mf_rcount_kernel(MfRlJob j) {
    const u64 x = (u64)blockIdx.x * MF_TPB + threadIdx.x;
    if (x >= j.nr) return;
    const u64 r = j.r0 + x;
    const u64 f0 = j.first[r], f1 = j.first[r + 1];
    const u64 klo = (f0 > j.t0 ? f0 : j.t0) - f0, khi = (f1 < j.t1 ? f1 : j.t1) - f0;  // its fragments here, not empty
    const u64 off = j.rq[3 * r + 1];
    const mfp::RCut c = mfp::rcut_of(j.log2_adm, j.nfiles, j.rq[3 * r], off, j.rq[3 * r + 2]);
    u64 sum = 0;
    if (c.bytes) {
        // the first fragment of [klo, khi) whose n is below its planned length (khi: none)
        u64 lo = klo, hi = khi;
        while (lo < hi) {
            const u64 mid = lo + ((hi - lo) >> 1);
            const u64 full = mfp::rfrag_pos(off, c.planned, c.frags, mid + 1) - mfp::rfrag_pos(off, c.planned, c.frags, mid);
            if (j.resp[(f0 + mid - j.t0) * MF_RESP_WORDS] >= full) lo = mid + 1; else hi = mid;
        }
        sum = mfp::rfrag_pos(off, c.planned, c.frags, lo) - mfp::rfrag_pos(off, c.planned, c.frags, klo);
        if (lo < khi) sum += j.resp[(f0 + lo - j.t0) * MF_RESP_WORDS];
    }
    if (klo == 0) {
        j.cnt[r] = sum;
        j.some[r] = j.rsome[f0 - j.t0];
    } else {
        j.cnt[r] += sum;
    }
}

// ---- host side -------------------------------------------------------------------------------------
// everything that follows from a file's capacity 2^log2_b
static void mf_set_geometry(MfHost& s, u32 log2_b) {
    s.log2_b = log2_b;
    s.nlines = (u32)((s.files << s.log2_b) / MF_LINE);
    s.key_bits = 1;  // ceil(log2(nlines + 1)): the sentinel is a key too
    while ((1ull << s.key_bits) <= s.nlines) s.key_bits++;
}

// may a store of this context's F files hold file_bytes (a power of two) each? nrg_open's limits
static bool mf_cap_ok(const nrg_ctx* c, u64 file_bytes) {
    return file_bytes >= (1ull << MF_LOG2_MIN) && file_bytes <= (1ull << MF_LOG2_MAX) && !(file_bytes & (file_bytes - 1)) &&
           c->mf.files * file_bytes <= MF_MAX_BYTES;
}

static u32 mf_log2(u64 pow2) {
    u32 l = 0;
    while ((1ull << l) < pow2) l++;
    return l;
}

static u64 mf_capacity(const nrg_ctx* c) { return 1ull << c->mf.log2_b; }

// DsOps::grow: the store at new_cap bytes per file (a power of two above B within nrg_open's limits),
// "Capacity growth" above. With keep == false the old bytes are not moved (nrg_restore: the image
// replaces them). If the allocation fails nothing has been launched: the replica is as it was.
static hipError_t mf_regrow(nrg_ctx* c, u64 new_cap, bool keep) {
    MfHost& s = c->mf;
    if (new_cap <= mf_capacity(c) || !mf_cap_ok(c, new_cap)) return hipErrorInvalidValue;
    const u32 nl2 = mf_log2(new_cap);
    uint8_t* nf = nullptr;
    if (hipMalloc(&nf, s.files << nl2) != hipSuccess) {
        (void)hipGetLastError();  // (the failure is reported by the return value alone)
        return hipErrorOutOfMemory;
    }
    hipError_t e = hipSuccess;
    if (keep) {
        const u64 units = (s.files << nl2) / 16;
        NRG_LAUNCH(c, "mf_grow", mf_grow_kernel, copy_grid(units), DG_TPB, 0, c->stream, (const uint4*)s.d_files, (uint4*)nf,
                   units, s.log2_b - 4, nl2 - 4);
        e = hipGetLastError();
    }
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        (void)hipFree(nf);
        return e;
    }
    (void)hipFree(s.d_files);
    s.d_files = nf;
    mf_set_geometry(s, nl2);
    return hipSuccess;
}

static hipError_t mf_grow(nrg_ctx* c, u64 new_cap) { return mf_regrow(c, new_cap, true); }

// Before a chunk of a context with a bound above B: the chunk's need (mf_need), read back, and the grow
// where B does not hold it. j: the chunk's records and the geometry as it stands.
static hipError_t mf_room(nrg_ctx* c, const MfJob& j) {
    MfHost& s = c->mf;
    NRG_LAUNCH(c, "mf_need", mf_need_kernel, (unsigned)((j.n + MF_TPB - 1) / MF_TPB), MF_TPB, 0, c->stream, j,
               1ull << s.max_log2, s.d_need);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    u64 need = 0;
    timer_begin(c, "mf_room");
    e = hipMemcpyAsync(&need, s.d_need, sizeof(u64), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    timer_end(c, "mf_room");
    if (e != hipSuccess) return e;
    const u32 to = mfp::mf_grow_log2(s.log2_b, need, s.max_log2);
    return to > s.log2_b ? mf_grow(c, 1ull << to) : hipSuccess;
}

static hipError_t mf_replay_chunk(nrg_ctx* c, const void* src, u64 lo, u64 n, u64 resp_lo, u64 resp_hi, void* d_resp,
                                  uint8_t* d_some) {
    if (n == 0) return hipSuccess;
    MfHost& s = c->mf;
    MfJob j{};
    j.src = (const u64*)src;
    j.ring = (u64*)c->d_ring;
    j.ring_mask = c->log_size - 1;
    j.lo = lo;
    j.n = n;
    if (s.max_log2 > s.log2_b && !s.planned) {  // the store grows first if the chunk needs it
        j.log2_b = s.log2_b;
        j.nfiles = (u32)s.files;
        const hipError_t eg = mf_room(c, j);
        if (eg != hipSuccess) return eg;
    }
    const bool want = d_resp != nullptr && d_some != nullptr && resp_lo < resp_hi && resp_lo < lo + n && resp_hi > lo;
    j.rlo = want ? resp_lo : 0;
    j.rhi = want ? resp_hi : 0;
    j.resp = want ? (u64*)d_resp : nullptr;
    j.some = want ? d_some : nullptr;
    j.ctl = c->d_ctl;
    j.files = s.d_files;
    j.log2_b = s.log2_b;
    j.nfiles = (u32)s.files;
    j.adm = 1ull << (s.max_log2 > s.log2_b ? s.max_log2 : s.log2_b);
    j.nlines = s.nlines;
    j.keys = s.d_keys;
    j.desc = s.d_desc;
    const unsigned eg = (unsigned)((n + MF_TPB - 1) / MF_TPB);
    MfSz z{};
    if (s.d_size) {  // the sizes at every log position of the chunk ("Sizes" above)
        if (++s.epoch == 0) {
            hipError_t e0 = hipMemsetAsync(s.d_fep, 0, s.files * sizeof(u32), c->stream);
            if (e0 != hipSuccess) return e0;
            s.epoch = 1;
        }
        z = MfSz{s.d_size, s.d_fkey, s.d_el, (uint2*)s.d_sc, s.d_ev, (uint4*)s.d_fm, s.d_fep, (uint4*)s.d_sagg, s.epoch};
        NRG_LAUNCH(c, "mfs_keys", mfs_keys_kernel, eg, MF_TPB, 0, c->stream, j, z);
        MfsIn in{nullptr, nullptr, n};
        if (s.files > 1) {
            u32 *gk = nullptr, *gv = nullptr;
            timer_begin(c, "mfs_sort");
            const hipError_t e1 = sort_pairs(c->sort, s.d_fkey, nullptr, n, (int)s.file_bits, c->stream, &gk, &gv);
            timer_end(c, "mfs_sort");
            if (e1 != hipSuccess) return e1;
            in.gk = gk, in.gv = gv;
        }
        const unsigned tiles = (unsigned)((n + MFS_TILE - 1) / MFS_TILE);
        if (tiles > 1) {
            NRG_LAUNCH(c, "mfs_reduce", mfs_reduce_kernel, tiles, MF_TPB, 0, c->stream, in, z);
            NRG_LAUNCH(c, "mfs_aggscan", mfs_aggscan_kernel, 1, MF_TPB, 0, c->stream, z.agg, (u32)tiles);
        }
        NRG_LAUNCH(c, "mfs_scan", mfs_scan_kernel, tiles, MF_TPB, 0, c->stream, in, z, tiles > 1 ? 1u : 0u);
        NRG_LAUNCH(c, "mfs_expand", mfs_expand_kernel, eg, MF_TPB, 0, c->stream, j, (const uint2*)z.sc);
    } else {
        NRG_LAUNCH(c, "mf_expand", mf_expand_kernel, eg, MF_TPB, 0, c->stream, j);
    }
    u32 *sk = nullptr, *sv = nullptr;
    timer_begin(c, "mf_sort");
    const hipError_t e = sort_pairs(c->sort, s.d_keys, nullptr, 2 * n, (int)s.key_bits, c->stream, &sk, &sv);
    timer_end(c, "mf_sort");
    if (e != hipSuccess) return e;
    const u32 per = MF_TPB / 64;
    if (s.d_size)
        NRG_LAUNCH(c, "mfs_lines", mfs_lines_kernel, (s.nlines + per - 1) / per, MF_TPB, 0, c->stream, j, (const u32*)sk,
                   (const u32*)sv, (u32)(2 * n), z);
    else
        NRG_LAUNCH(c, "mf_lines", mf_lines_kernel, (s.nlines + per - 1) / per, MF_TPB, 0, c->stream, j, (const u32*)sk,
                   (const u32*)sv, (u32)(2 * n));
    return hipGetLastError();
}

static hipError_t mf_fill(nrg_ctx* c) {
    const u64 words = c->mf.files * (1ull << c->mf.log2_b) / 8;
    mf_fill_kernel<<<copy_grid(words), DG_TPB, 0, c->stream>>>((u64*)c->mf.d_files, words);
    if (c->mf.d_size)
        mfs_fill_kernel<<<copy_grid(c->mf.files), DG_TPB, 0, c->stream>>>(c->mf.d_size, c->mf.files, 1ull << c->mf.log2_b);
    return hipGetLastError();
}

// nrg_memfs_enable_sizes: the size table (every size B) and the scratch of a sized chunk. The stream
// has been drained. On a failed allocation the context stays unsized (mf_close frees what was made).
static int mf_enable(nrg_ctx* c) {
    MfHost& s = c->mf;
    if (s.d_size) return NRG_OK;
    const u64 mb = c->cfg.max_batch;
    u64* size = nullptr;
    HIPCHK(hipMalloc(&s.d_fkey, mb * sizeof(u32)));
    HIPCHK(hipMalloc(&s.d_el, mb * sizeof(u32)));
    HIPCHK(hipMalloc(&s.d_sc, mb * sizeof(uint2)));
    HIPCHK(hipMalloc(&s.d_ev, mb * sizeof(u32)));
    HIPCHK(hipMalloc(&s.d_fm, s.files * sizeof(uint4)));
    HIPCHK(hipMalloc(&s.d_fep, s.files * sizeof(u32)));
    HIPCHK(hipMalloc(&s.d_sagg, (mb / MFS_TILE + 1) * sizeof(uint4)));
    HIPCHK(hipMalloc(&size, s.files * sizeof(u64)));
    HIPCHK(hipMemsetAsync(s.d_fep, 0, s.files * sizeof(u32), c->stream));
    mfs_fill_kernel<<<copy_grid(s.files), DG_TPB, 0, c->stream>>>(size, s.files, 1ull << s.log2_b);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    s.epoch = 0;
    s.d_size = size;
    return NRG_OK;
}

static int mf_open(nrg_ctx* c) {
    const nrg_config& cf = c->cfg;
    MfHost& s = c->mf;
    // log2_slots: log2 of a file's bytes; queue_capacity: the number of files (include/nrgpu.h)
    if (cf.log2_slots < MF_LOG2_MIN || cf.log2_slots > MF_LOG2_MAX || cf.queue_capacity < 1 ||
        cf.queue_capacity > MF_MAX_FILES || (cf.queue_capacity << cf.log2_slots) > MF_MAX_BYTES ||
        cf.max_batch > MF_MAX_BATCH)
        return NRG_E_INVAL;
    s.files = cf.queue_capacity;
    mf_set_geometry(s, cf.log2_slots);
    s.file_bits = 1;  // ceil(log2 F): what a sized chunk's file sort sorts by
    while ((1ull << s.file_bits) < s.files) s.file_bits++;
    HIPCHK(hipMalloc(&s.d_files, s.files << s.log2_b));
    HIPCHK(hipMalloc(&s.d_keys, 2 * cf.max_batch * sizeof(u32)));
    HIPCHK(hipMalloc(&s.d_desc, cf.max_batch * sizeof(u64)));
    HIPCHK(hipMalloc(&s.d_pagg, (cf.max_reads / MF_PR_SCAN + 1) * sizeof(u64)));
    if (sort_alloc(c->sort, 2 * cf.max_batch) != NRG_OK) return NRG_E_NOMEM;
    HIPCHK(mf_fill(c));
    c->pipeline = false;  // config.pipeline is accepted: nothing is deferred
    return NRG_OK;
}

static void mf_close(nrg_ctx* c) {
    MfHost& s = c->mf;
    void* ptrs[] = {s.d_files, s.d_keys, s.d_desc, s.d_pagg, s.d_size, s.d_fkey, s.d_el,
                    s.d_sc,    s.d_ev,   s.d_fm,   s.d_fep,  s.d_sagg, s.d_need};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (s.d_rpk) (void)hipFree(s.d_rpk);  // nrg_memfs_pread_repack_async's scratch
    if (s.d_rresp) (void)hipFree(s.d_rresp);  // nrg_memfs_pread_logged*'s responses of one pass
    if (s.d_wup) (void)hipFree(s.d_wup);  // nrg_memfs_pwrite*'s and nrg_memfs_pread_logged*'s upload
    if (s.h_wup) (void)hipHostFree(s.h_wup);
    if (s.ev_wup) (void)hipEventDestroy(s.ev_wup);
    pt_close(c);  // the scratch of this replica's file partitioning, if it ever partitioned
}

static void mf_defaults(nrg_config* cfg) {
    cfg->log2_slots = MF_LOG2_DEFAULT;  // one 4096-byte file (benches/memfs.rs:112-121)
    cfg->queue_capacity = 1;
}

// nrg_digest: items are the aligned 8-byte words of every file, (file << 32 | word index, the word)
__global__ __launch_bounds__(DG_TPB) void mf_digest_kernel(const u64* words, u64 n, u32 log2_wpf, u64* out3) {
    u64 c = 0, sm = 0, x = 0;
    for (u64 i = blockIdx.x * (u64)DG_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * DG_TPB) {
        const u64 h = dg_item(((i >> log2_wpf) << 32) | (i & ((1ull << log2_wpf) - 1)), words[i]);
        c++;
        sm += h;
        x ^= h;
    }
    dg_commit(c, sm, x, out3);
}

// a sized context's further items: one per file, (file << 32 | 0xFFFFFFFF, its size); no word index
// reaches that key
__global__ __launch_bounds__(DG_TPB) void mfs_digest_kernel(const u64* size, u64 n, u64* out3) {
    u64 c = 0, sm = 0, x = 0;
    for (u64 i = blockIdx.x * (u64)DG_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * DG_TPB) {
        const u64 h = dg_item((i << 32) | 0xFFFFFFFFull, size[i]);
        c++;
        sm += h;
        x ^= h;
    }
    dg_commit(c, sm, x, out3);
}

static u64 mf_words(const nrg_ctx* c) { return (c->mf.files << c->mf.log2_b) / 8; }

static hipError_t mf_digest(nrg_ctx* c, u64* d_out3) {
    hipError_t e = hipMemsetAsync(d_out3, 0, 3 * sizeof(u64), c->stream);
    if (e != hipSuccess) return e;
    NRG_LAUNCH(c, "mf_digest", mf_digest_kernel, dg_grid(mf_words(c)), DG_TPB, 0, c->stream, (const u64*)c->mf.d_files,
               mf_words(c), c->mf.log2_b - 3, d_out3);
    // (nrg_restore's comparison of an unsized image's digest, which has no size items: once)
    if (c->mf.d_size && !c->mf.unsized_image)
        NRG_LAUNCH(c, "mfs_digest", mfs_digest_kernel, dg_grid(c->mf.files), DG_TPB, 0, c->stream,
                   (const u64*)c->mf.d_size, c->mf.files, d_out3);
    c->mf.unsized_image = false;
    return hipGetLastError();
}

static int mf_items(nrg_ctx* c, u64* n) {
    *n = mf_words(c) + (c->mf.d_size ? c->mf.files : 0);
    return NRG_OK;
}

// The snapshot payload: the files' bytes in inode order (items: their 8-byte words), and in a sized
// context the nf = F sizes after them, one item each.
__global__ __launch_bounds__(DG_TPB) void mf_snapshot_kernel(const u64* words, u64 n, const u64* size, u64 nf, u64* buf,
                                                             u64 cap, u64 log_idx, DevCtl* ctl) {
    const u64 items = n + nf;
    if (blockIdx.x == 0 && threadIdx.x == 0) snap_head(buf, cap, NRG_DS_MEMFS, items, items * 8, log_idx, ctl);
    if (snap_bytes(items * 8) > cap) return;
    u64* out = buf + SNAP_HDR / 8;
    for (u64 i = blockIdx.x * (u64)DG_TPB + threadIdx.x; i < items; i += (u64)gridDim.x * DG_TPB)
        out[i] = i < n ? words[i] : size[i - n];
}

static hipError_t mf_snapshot(nrg_ctx* c, void* d_buf, u64 cap, u64 log_idx) {
    NRG_LAUNCH(c, "mf_snapshot", mf_snapshot_kernel, copy_grid(mf_words(c)), DG_TPB, 0, c->stream,
               (const u64*)c->mf.d_files, mf_words(c), (const u64*)c->mf.d_size, c->mf.d_size ? c->mf.files : 0,
               (u64*)d_buf, cap, log_idx, c->d_ctl);
    return hipGetLastError();
}

// An image goes only into a context of the same geometry. The header carries the item count alone:
// another total is refused by check_only with nothing touched; the same total cut into other files
// has another digest (the items' keys carry the file), which nrg_restore's comparison refuses.
// An image of F * B / 8 + F items is a sized one: the F sizes follow the bytes, the context becomes
// sized, and a size above B or a non-zero byte at or past a size latches ERR_INVAL on the device, which
// nrg_restore reads before it compares the digests. An unsized image leaves a sized context sized, every
// size B.
// With a bound (nrg_set_max_capacity) a sized image of the same F and a power-of-two B_img in (B, max] is
// taken too: the store is reallocated to B_img first, no old byte copied. A smaller B_img stays refused:
// the store never shrinks.
// log2 of the capacity of an image of `items` items that may go into this context; 0: none may
static u32 mf_image_log2(const nrg_ctx* c, u64 items) {
    const MfHost& s = c->mf;
    if (items == mf_words(c) || items == mf_words(c) + s.files) return s.log2_b;
    for (u32 l = s.log2_b + 1; l <= s.max_log2; l++)
        if (items == (s.files << l) / 8 + s.files) return l;
    return 0;
}

static int mf_restore(nrg_ctx* c, const void* d_payload, u64 items, bool check_only) {
    const u32 il = d_payload || check_only ? mf_image_log2(c, items) : c->mf.log2_b;
    if (check_only) return il ? NRG_OK : NRG_E_INVAL;
    if (!d_payload) return hip_fail(mf_fill(c));
    if (!il) return NRG_E_INVAL;
    if (il > c->mf.log2_b) HIPCHK(mf_regrow(c, 1ull << il, false));
    const u64 words = mf_words(c);
    int r;
    if (items != words && (r = mf_enable(c))) return r;
    HIPCHK(hipMemcpyAsync(c->mf.d_files, d_payload, words * 8, hipMemcpyDeviceToDevice, c->stream));
    if (items == words) {
        c->mf.unsized_image = c->mf.d_size != nullptr;
        if (c->mf.d_size)
            mfs_fill_kernel<<<copy_grid(c->mf.files), DG_TPB, 0, c->stream>>>(c->mf.d_size, c->mf.files, 1ull << c->mf.log2_b);
        return hip_fail(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(c->mf.d_size, (const u64*)d_payload + words, c->mf.files * 8, hipMemcpyDeviceToDevice, c->stream));
    NRG_LAUNCH(c, "mfs_check", mfs_check_kernel, copy_grid(words), DG_TPB, 0, c->stream, (const u64*)c->mf.d_files, words,
               c->mf.log2_b - 3, (const u64*)c->mf.d_size, c->d_ctl);
    return hip_fail(hipGetLastError());
}

// nrg_set_max_capacity: the bound in bytes per file, 0 for none. No item count is read: the need of a
// chunk is not a count (the len_ub fast path of capacity.hpp does not apply), so Growth carries the
// bound alone. The stream has been drained.
static int mf_set_bound(nrg_ctx* c, u64 max_bytes) {
    MfHost& s = c->mf;
    if (!s.d_size) return NRG_E_INVAL;  // the new bytes are defined by the sizes' invariant
    if (max_bytes && (!mf_cap_ok(c, max_bytes) || !growth_bound_ok(max_bytes, mf_capacity(c), mf_ops()->cap_limit)))
        return NRG_E_INVAL;
    if (c->ltail != c->tail) return NRG_E_NOT_SYNCED;  // a record is admitted by the bound at its own log index
    if (max_bytes && !s.d_need) {
        HIPCHK(hipMalloc(&s.d_need, sizeof(u64)));
        HIPCHK(hipMemsetAsync(s.d_need, 0, sizeof(u64), c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    s.max_log2 = max_bytes ? mf_log2(max_bytes) : 0;
    c->growth = Growth{max_bytes, 0};
    return NRG_OK;
}

const DsOps* mf_ops() {
    static const DsOps ops = {sizeof(nrg_memfs_op), sizeof(nrg_memfs_resp), mf_open, mf_close, nullptr,
                              mf_replay_chunk, floor_ltail, nullptr, nullptr, mf_defaults, mf_digest,
                              mf_items, mf_snapshot, mf_restore, 1ull << MF_LOG2_MAX, mf_capacity, mf_grow,
                              true, mf_set_bound};
    return &ops;
}

}  // namespace nrg

// ---- the file store's entry points (include/nrgpu.h) ------------------------------------------------
using namespace nrg;

// the file of `ino` in a memfs context's store; nullptr for an ino outside the range
static uint8_t* mf_file(nrg_ctx* c, uint64_t ino) {
    if (ino < NRG_MEMFS_FIRST_INO || ino - NRG_MEMFS_FIRST_INO >= c->mf.files) return nullptr;
    return c->mf.d_files + ((ino - NRG_MEMFS_FIRST_INO) << c->mf.log2_b);
}

// a sized context's size of file f, read from the device (what has been replayed so far)
static int mf_size_get(nrg_ctx* c, uint64_t f, uint64_t* out) {
    HIPCHK(hipMemcpyAsync(out, c->mf.d_size + f, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_all(c));
    return NRG_OK;
}

static int mf_size_put(nrg_ctx* c, uint64_t f, uint64_t v) {
    HIPCHK(hipMemcpyAsync(c->mf.d_size + f, &v, sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(sync_all(c));
    return NRG_OK;
}

// log2 of what a Write's end and a SetAttr's size are admitted against: B, or the bound where it is above
static uint32_t mf_admit_log2(const nrg_ctx* c) {
    return c->mf.max_log2 > c->mf.log2_b ? c->mf.max_log2 : c->mf.log2_b;
}

// ---- nrg_memfs_pwrite*: what the three entries share ----
// the checks, in order: the kind, the batch bound, the pointers
static int mf_pwrite_check(nrg_ctx* c, const nrg_memfs_wr* reqs, uint64_t n, const uint8_t* d_data, uint64_t data_bytes) {
    int r = need(c, NRG_DS_MEMFS);
    if (r) return r;
    if (n > c->cfg.max_batch) return NRG_E_CAPACITY;
    if ((n && !reqs) || (data_bytes && !d_data)) return NRG_E_INVAL;
    return NRG_OK;
}

// The upload buffers of a planned call (a logged write's or a logged read's): made by the first such
// call, after that the wait for the previous call's upload to have left the pinned copy.
static int mf_wup_ready(nrg_ctx* c) {
    MfHost& s = c->mf;
    const uint64_t words = 5 * c->cfg.max_batch + 2;
    if (!s.d_wup) {
        HIPCHK(hipMalloc(&s.d_wup, words * 8));
        HIPCHK(hipHostMalloc(&s.h_wup, words * 8));
        HIPCHK(hipEventCreateWithFlags(&s.ev_wup, hipEventDisableTiming));
    } else {
        HIPCHK(hipEventSynchronize(s.ev_wup));
    }
    return NRG_OK;
}

// The upload of a planned call: the requests and first[] through the pinned copy into d_wup, on the
// context's stream. The buffers are made by the first call (a context that never writes this way
// allocates nothing) and freed by mf_close. first: n + 1 words.
static int mf_pwrite_upload(nrg_ctx* c, const nrg_memfs_wr* reqs, const uint64_t* first, uint64_t n) {
    MfHost& s = c->mf;
    const uint64_t mb = c->cfg.max_batch;
    int r = mf_wup_ready(c);
    if (r) return r;
    memcpy(s.h_wup, reqs, n * sizeof(nrg_memfs_wr));
    memcpy(s.h_wup + 4 * mb, first, (n + 1) * 8);
    HIPCHK(hipMemcpyAsync(s.d_wup, s.h_wup, n * sizeof(nrg_memfs_wr), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s.d_wup + 4 * mb, s.h_wup + 4 * mb, (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(s.ev_wup, c->stream));
    return NRG_OK;
}

// fragments [t0, t1) of the uploaded call to records (pos0 + t - t0) & mask of dst
static hipError_t mf_frag_launch(nrg_ctx* c, uint64_t n, uint64_t t0, uint64_t t1, void* dst, uint64_t pos0, uint64_t mask,
                                 const uint8_t* d_data, uint64_t data_bytes, uint64_t* d_written, uint8_t* d_some,
                                 uint32_t adm_log2) {
    MfHost& s = c->mf;
    MfWrJob j{};
    j.rq = s.d_wup;
    j.first = s.d_wup + 4 * c->cfg.max_batch;
    j.n = n;
    j.t0 = t0, j.t1 = t1;
    j.dst = (u64*)dst;
    j.pos0 = pos0, j.mask = mask;
    j.data = d_data;
    j.data_bytes = data_bytes;
    j.log2_b = adm_log2;  // the plan's: what the requests were admitted against
    j.nfiles = (u32)s.files;
    j.written = d_written;
    j.some = d_some;
    NRG_LAUNCH(c, "mf_frag", mf_frag_kernel, (unsigned)((t1 - t0 + MF_FR_TILE - 1) / MF_FR_TILE), MF_TPB, 0, c->stream, j);
    return hipGetLastError();
}

// ---- nrg_memfs_pread_logged*: what the entries share ----
// the checks, in order: the kind, the batch bound, the pointers
static int mf_rl_check(nrg_ctx* c, const nrg_memfs_rd* reqs, uint64_t n) {
    int r = need(c, NRG_DS_MEMFS);
    if (r) return r;
    if (n > c->cfg.max_batch) return NRG_E_CAPACITY;
    if (n && !reqs) return NRG_E_INVAL;
    return NRG_OK;
}

// The upload of a planned call: the requests, first[] and offs[] (n + 1 words each) through the pinned
// copy into d_wup, on the context's stream.
static int mf_rl_upload(nrg_ctx* c, const nrg_memfs_rd* reqs, const uint64_t* first, const uint64_t* offs, uint64_t n) {
    MfHost& s = c->mf;
    const uint64_t mb = c->cfg.max_batch;
    int r = mf_wup_ready(c);
    if (r) return r;
    memcpy(s.h_wup, reqs, n * sizeof(nrg_memfs_rd));
    memcpy(s.h_wup + 3 * mb, first, (n + 1) * 8);
    memcpy(s.h_wup + 3 * mb + n + 1, offs, (n + 1) * 8);  // (right after first[]: one copy takes both)
    HIPCHK(hipMemcpyAsync(s.d_wup, s.h_wup, n * sizeof(nrg_memfs_rd), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s.d_wup + 3 * mb, s.h_wup + 3 * mb, 2 * (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(s.ev_wup, c->stream));
    return NRG_OK;
}

static MfRlJob mf_rl_job(nrg_ctx* c, uint64_t n, uint64_t t0, uint64_t t1, uint32_t adm_log2) {
    MfHost& s = c->mf;
    const uint64_t mb = c->cfg.max_batch;
    MfRlJob j{};
    j.rq = s.d_wup;
    j.first = s.d_wup + 3 * mb;
    j.offs = s.d_wup + 3 * mb + n + 1;
    j.n = n;
    j.t0 = t0, j.t1 = t1;
    j.log2_adm = adm_log2;  // the plan's
    j.nfiles = (u32)s.files;
    return j;
}

// fragments [t0, t1) of the uploaded call to records (pos0 + t - t0) & mask of dst
static hipError_t mf_rfrag_launch(nrg_ctx* c, uint64_t n, uint64_t t0, uint64_t t1, void* dst, uint64_t pos0, uint64_t mask,
                                  uint32_t adm_log2) {
    MfRlJob j = mf_rl_job(c, n, t0, t1, adm_log2);
    j.dst = (u64*)dst;
    j.pos0 = pos0, j.mask = mask;
    NRG_LAUNCH(c, "mf_rfrag", mf_rfrag_kernel, (unsigned)((t1 - t0 + MF_FR_TILE - 1) / MF_FR_TILE), MF_TPB, 0, c->stream, j);
    return hipGetLastError();
}

// the request of fragment t (< first[n]): first[r] <= t < first[r + 1]
static uint64_t mf_rl_req(const uint64_t* first, uint64_t n, uint64_t t) {
    uint64_t lo = 1, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (first[mid] <= t) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// where fragment t's bytes start in the slot space; t == first[n]: offs[n]
static uint64_t mf_rl_pos(const nrg_ctx* c, uint32_t adm, const nrg_memfs_rd* reqs, const uint64_t* first, const uint64_t* offs,
                          uint64_t n, uint64_t t) {
    if (t >= first[n]) return offs[n];
    const uint64_t r = mf_rl_req(first, n, t);
    const mfp::RCut cut = mfp::rcut_of(adm, c->mf.files, reqs[r].ino, reqs[r].offset, reqs[r].len);
    return offs[r] + (cut.bytes ? mfp::rfrag_pos(reqs[r].offset, cut.planned, cut.frags, t - first[r]) : 0);
}

// The way back: the responses of fragments [t0, t1) (d_resp, d_rsome: that many) into the slots, and the
// counts and some bytes of the requests that have fragments there (d_counts == nullptr: not wanted).
static hipError_t mf_rgather_launch(nrg_ctx* c, uint32_t adm, const nrg_memfs_rd* reqs, const uint64_t* first,
                                    const uint64_t* offs, uint64_t n, uint64_t t0, uint64_t t1, const void* d_resp,
                                    const uint8_t* d_rsome, uint8_t* d_data, uint64_t* d_counts, uint8_t* d_some) {
    MfRlJob j = mf_rl_job(c, n, t0, t1, adm);
    j.resp = (const u64*)d_resp;
    j.rsome = d_rsome;
    j.data = d_data;
    j.cnt = d_counts;
    j.some = d_some;
    j.p0 = mf_rl_pos(c, adm, reqs, first, offs, n, t0);
    j.p1 = mf_rl_pos(c, adm, reqs, first, offs, n, t1);
    if (j.p1 > j.p0) {
        const uint64_t tiles = (j.p1 - j.p0 + 7 + MF_RG_TILE - 1) / MF_RG_TILE;
        NRG_LAUNCH(c, "mf_rgather", mf_rgather_kernel, (unsigned)(tiles < MF_RG_MAX_GRID ? tiles : MF_RG_MAX_GRID), MF_TPB, 0,
                   c->stream, j);
    }
    if (d_counts) {
        j.r0 = mf_rl_req(first, n, t0);
        j.nr = mf_rl_req(first, n, t1 - 1) - j.r0 + 1;
        NRG_LAUNCH(c, "mf_rcount", mf_rcount_kernel, (unsigned)((j.nr + MF_TPB - 1) / MF_TPB), MF_TPB, 0, c->stream, j);
    }
    return hipGetLastError();
}

// the plan of a call on this context: first, offs (n + 1 each) against the admission bound
static int mf_rl_plan(nrg_ctx* c, const nrg_memfs_rd* reqs, uint64_t n, std::vector<uint64_t>& first,
                      std::vector<uint64_t>& offs) {
    first.resize(n + 1);
    offs.resize(n + 1);
    return mfp::read_plan(mf_admit_log2(c), c->mf.files, reqs, n, first.data(), offs.data(), nullptr);
}

extern "C" {

int nrg_memfs_enable_sizes(nrg_ctx* c) {
    int r = need(c, NRG_DS_MEMFS);
    if (r) return r;
    if (c->ltail != c->tail) return NRG_E_NOT_SYNCED;
    HIPCHK(sync_all(c));
    return mf_enable(c);
}

int nrg_memfs_size(nrg_ctx* c, uint64_t ino, uint64_t* size) {
    int r = need(c, NRG_DS_MEMFS);
    if (r) return r;
    if (!c->mf.d_size || !size || !mf_file(c, ino)) return NRG_E_INVAL;
    return mf_size_get(c, ino - NRG_MEMFS_FIRST_INO, size);
}

int nrg_memfs_truncate(nrg_ctx* c, uint64_t ino, uint64_t size) {
    int r = need(c, NRG_DS_MEMFS);
    if (r) return r;
    if (!c->mf.d_size || !mf_file(c, ino) || size > (1ull << mf_admit_log2(c))) return NRG_E_INVAL;
    if (c->ltail != c->tail) return NRG_E_NOT_SYNCED;
    if (size > mf_capacity(c)) HIPCHK(mf_grow(c, 1ull << mfp::mf_grow_log2(c->mf.log2_b, size, c->mf.max_log2)));
    uint8_t* f = mf_file(c, ino);
    uint64_t cur = 0;
    if ((r = mf_size_get(c, ino - NRG_MEMFS_FIRST_INO, &cur))) return r;
    if (size < cur) HIPCHK(hipMemsetAsync(f + size, 0, cur - size, c->stream));  // bytes [size, cur) are gone
    return mf_size_put(c, ino - NRG_MEMFS_FIRST_INO, size);
}

int nrg_memfs_round_async(nrg_ctx* c, const nrg_memfs_op* d_ops, uint64_t n, uint32_t origin, nrg_memfs_resp* d_resp,
                          uint8_t* d_some) {
    if (((uintptr_t)d_ops | (uintptr_t)d_resp) & 7) return NRG_E_INVAL;  // (records and responses move as u64 words)
    return round_common(c, NRG_DS_MEMFS, d_ops, n, origin, d_resp, d_some);
}

int nrg_memfs_init(nrg_ctx* c, uint64_t ino, const uint8_t* bytes, uint64_t len) {
    int r = need(c, NRG_DS_MEMFS);
    if (r) return r;
    uint8_t* f = mf_file(c, ino);
    if (!f || len > (1ull << c->mf.log2_b) || (len && !bytes)) return NRG_E_INVAL;
    if (len) HIPCHK(hipMemcpyAsync(f, bytes, len, hipMemcpyHostToDevice, c->stream));
    HIPCHK(sync_all(c));
    if (c->mf.d_size) {  // size = max(size, len)
        uint64_t cur = 0;
        if ((r = mf_size_get(c, ino - NRG_MEMFS_FIRST_INO, &cur))) return r;
        if (len > cur) return mf_size_put(c, ino - NRG_MEMFS_FIRST_INO, len);
    }
    return NRG_OK;
}

int nrg_memfs_read(nrg_ctx* c, uint64_t ino, uint64_t offset, uint64_t len, uint8_t* buf, uint64_t* n) {
    int r = need(c, NRG_DS_MEMFS);
    if (r) return r;
    if (!n) return NRG_E_INVAL;
    if (c->ltail != c->tail) return NRG_E_NOT_SYNCED;
    const uint8_t* f = mf_file(c, ino);
    if (!f) return NRG_E_INVAL;
    uint64_t B = 1ull << c->mf.log2_b;
    if (c->mf.d_size && (r = mf_size_get(c, ino - NRG_MEMFS_FIRST_INO, &B))) return r;  // clipped at the size
    *n = offset >= B ? 0 : (len < B - offset ? len : B - offset);
    if (*n && !buf) return NRG_E_INVAL;
    if (*n) HIPCHK(hipMemcpyAsync(buf, f + offset, *n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_all(c));
    return check_err(c);
}

int nrg_memfs_dump(nrg_ctx* c, uint64_t ino, uint8_t* buf, uint64_t cap, uint64_t* n) {
    int r = need(c, NRG_DS_MEMFS);
    if (r) return r;
    if (!n) return NRG_E_INVAL;
    const uint8_t* f = mf_file(c, ino);
    if (!f) return NRG_E_INVAL;
    *n = 1ull << c->mf.log2_b;
    if (c->mf.d_size && (r = mf_size_get(c, ino - NRG_MEMFS_FIRST_INO, n))) return r;  // the file ends at its size
    if (*n > cap) return NRG_E_CAPACITY;
    if (!buf) return *n ? NRG_E_INVAL : NRG_OK;
    if (*n) HIPCHK(hipMemcpyAsync(buf, f, *n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_all(c));
    return NRG_OK;
}

int nrg_memfs_reserve(nrg_ctx* c, uint64_t file_bytes) {
    int r = need(c, NRG_DS_MEMFS);
    if (r) return r;
    if (!c->mf.d_size || file_bytes > (1ull << MF_LOG2_MAX)) return NRG_E_INVAL;
    const uint64_t want = pow2_at_least(file_bytes);
    if (want <= mf_capacity(c)) return NRG_OK;  // never shrinks
    if (!mf_cap_ok(c, want)) return NRG_E_INVAL;
    return reserve_common(c, NRG_DS_MEMFS, want);
}

int nrg_memfs_max_capacity(nrg_ctx* c, uint64_t* max_bytes) {
    if (!c || !max_bytes || c->cfg.ds_kind != NRG_DS_MEMFS) return NRG_E_INVAL;
    *max_bytes = c->growth.max_items;
    return NRG_OK;
}

int nrg_memfs_geometry(nrg_ctx* c, uint64_t* files, uint64_t* file_bytes) {
    if (!c || c->cfg.ds_kind != NRG_DS_MEMFS) return NRG_E_INVAL;
    if (files) *files = c->mf.files;
    if (file_bytes) *file_bytes = 1ull << c->mf.log2_b;
    return NRG_OK;
}

// the checks both preads share, in nrg_skiplist_get's order
static int mf_pread_check(nrg_ctx* c, const void* reqs, uint64_t n, const void* data, uint64_t cap, const void* offs,
                          const void* some) {
    int r = need(c, NRG_DS_MEMFS);
    if (r) return r;
    if (c->ltail != c->tail) return NRG_E_NOT_SYNCED;
    if (n > c->cfg.max_reads) return NRG_E_CAPACITY;
    if (((uintptr_t)reqs | (uintptr_t)offs) & 7) return NRG_E_INVAL;
    if (n && (!reqs || !offs || !some || (cap && !data))) return NRG_E_INVAL;
    return NRG_OK;
}

int nrg_memfs_pread_async(nrg_ctx* c, const nrg_memfs_rd* d_reqs, uint64_t n, uint8_t* d_data, uint64_t cap,
                          uint64_t* d_offs, uint8_t* d_some) {
    int r = mf_pread_check(c, d_reqs, n, d_data, cap, d_offs, d_some);
    if (r) return r;
    // the total is on the device: the copy's grid comes from the host's bound, surplus workgroups exit
    HIPCHK(mf_pread_scan_launch(c, d_reqs, n, d_offs, d_some, nullptr, c->mf.d_pagg));
    return hip_fail(mf_pread_copy_launch(c, d_reqs, n, d_offs, d_data, cap, mf_pread_bound(c, n, cap)));
}

// The packed answers' scratch of nrg_memfs_pread_repack_async on a plain replica, grown on demand (the
// replica's stream is drained before a reallocation): the positions' offsets and the scan aggregates.
static hipError_t mf_repack_scratch(nrg_ctx* c, uint64_t words) {
    MfHost& s = c->mf;
    if (s.rpk_words >= words) return hipSuccess;
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return e;
    if (s.d_rpk) (void)hipFree(s.d_rpk);
    s.d_rpk = nullptr;
    s.rpk_words = 0;
    if ((e = hipMalloc((void**)&s.d_rpk, words * 8)) != hipSuccess) return e;
    s.rpk_words = words;
    return hipSuccess;
}

int nrg_memfs_pread_repack_async(nrg_ctx* c, const uint8_t* d_src, const uint64_t* d_src_cnt, const uint8_t* d_src_some,
                                 const uint32_t* d_pos, uint64_t n, uint8_t* d_data, uint64_t cap, uint64_t* d_offs,
                                 uint8_t* d_some) {
    int r = need(c, NRG_DS_MEMFS);
    if (r) return r;
    if (((uintptr_t)d_src & 15) || (((uintptr_t)d_src_cnt | (uintptr_t)d_offs) & 7)) return NRG_E_INVAL;
    if (n && (!d_src_cnt || !d_src_some || !d_pos || !d_offs || !d_some || (cap && !d_data))) return NRG_E_INVAL;
    if (n >= (1ull << 32)) return NRG_E_CAPACITY;  // positions are u32
    HIPCHK(mf_repack_scratch(c, n + 1 + mf_pread_agg_words(n)));
    uint64_t* so = c->mf.d_rpk;
    HIPCHK(mf_repack_scan_launch(c, d_src_cnt, d_src_some, d_pos, n, d_offs, d_some, so, so + n + 1));
    return hip_fail(mf_repack_copy_launch(c, d_src, so, d_pos, n, d_offs, d_data, cap, mf_pread_bound(c, n, cap)));
}

int nrg_memfs_pread(nrg_ctx* c, const nrg_memfs_rd* reqs, uint64_t n, uint8_t* data, uint64_t cap, uint64_t* offs,
                    uint8_t* some) {
    int r = mf_pread_check(c, reqs, n, data, cap, offs, some);
    if (r) return r;
    if (n == 0) {
        if (offs) offs[0] = 0;
        return NRG_OK;
    }
    const uint64_t room = mf_pread_bound(c, n, cap);  // what the device buffer has to hold
    Staging* g = c->stg;
    if ((r = staging(g[0], n * sizeof(nrg_memfs_rd))) || (r = staging(g[1], (n + 1) * 8)) || (r = staging(g[2], n)) ||
        (r = staging(g[3], room)))
        return r;
    HIPCHK(hipMemcpyAsync(g[0].p, reqs, n * sizeof(nrg_memfs_rd), hipMemcpyHostToDevice, c->stream));
    if ((r = nrg_memfs_pread_async(c, (const nrg_memfs_rd*)g[0].p, n, (uint8_t*)g[3].p, room, (uint64_t*)g[1].p,
                                   (uint8_t*)g[2].p)))
        return r;
    HIPCHK(hipMemcpyAsync(offs, g[1].p, (n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(some, g[2].p, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_all(c));
    const uint64_t got = offs[n] < cap ? offs[n] : cap;
    if (got) {
        HIPCHK(hipMemcpyAsync(data, g[3].p, got, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(sync_all(c));
    }
    if ((r = check_err(c))) return r;
    return offs[n] > cap ? NRG_E_CAPACITY : NRG_OK;
}

int nrg_memfs_pwrite_plan(uint32_t log2_b, uint64_t files, const nrg_memfs_wr* reqs, uint64_t n, uint64_t data_bytes,
                          uint64_t* first, uint64_t* written, uint8_t* some) {
    return mfp::plan(log2_b, files, reqs, n, data_bytes, first, written, some);
}

int nrg_memfs_pwrite_async(nrg_ctx* c, const nrg_memfs_wr* reqs, uint64_t n, const uint8_t* d_data, uint64_t data_bytes,
                           uint32_t origin, uint64_t* d_written, uint8_t* d_some, uint64_t* n_records) {
    int r = mf_pwrite_check(c, reqs, n, d_data, data_bytes);
    if (r) return r;
    if ((d_written == nullptr) != (d_some == nullptr)) return NRG_E_INVAL;
    if (n_records) *n_records = 0;
    if (n == 0) return NRG_OK;
    // EFBIG is decided against the bound where one is set (the catch-up below may grow B, never past it)
    const uint32_t adm = mf_admit_log2(c);
    std::vector<uint64_t> first(n + 1);
    if ((r = mfp::plan(adm, c->mf.files, reqs, n, data_bytes, first.data(), nullptr, nullptr))) return r;
    const uint64_t T = first[n];
    // catch up on anything appended by others first (Replica::combine execs the whole log)
    if ((r = exec_range(c, 0, 0, nullptr, nullptr))) return r;
    // the need of all the requests is in the plan: grow once, and the passes make no readback
    const uint32_t to = mfp::mf_grow_log2(c->mf.log2_b, mfp::plan_need(adm, c->mf.files, reqs, n), adm);
    if (to > c->mf.log2_b) HIPCHK(mf_grow(c, 1ull << to));
    if ((r = mf_pwrite_upload(c, reqs, first.data(), n))) return r;
    struct Planned {  // for the passes' replays
        bool& f;
        explicit Planned(bool& x) : f(x) { f = true; }
        ~Planned() { f = false; }
    } planned(c->mf.planned);
    for (uint64_t done = 0; done < T;) {  // passes: what one append may carry, straight into the ring
        const uint64_t m = T - done < append_max(c) ? T - done : append_max(c);
        if ((r = reserve(c, m))) return r;
        const uint64_t lo = c->tail;
        HIPCHK(mf_frag_launch(c, n, done, done + m, c->d_ring, lo, c->log_size - 1, d_data, data_bytes, d_written, d_some,
                              adm));
        note_origin(c, lo, m, origin);
        c->tail = lo + m;
        if ((r = exec_range(c, 0, 0, nullptr, nullptr))) return r;
        done += m;
    }
    if (n_records) *n_records = T;
    return NRG_OK;
}

int nrg_memfs_pwrite(nrg_ctx* c, const nrg_memfs_wr* reqs, uint64_t n, const uint8_t* data, uint64_t data_bytes,
                     uint32_t origin, uint64_t* written, uint8_t* some, uint64_t* n_records) {
    int r = mf_pwrite_check(c, reqs, n, data, data_bytes);
    if (r) return r;
    if ((written == nullptr) != (some == nullptr)) return NRG_E_INVAL;
    if (n == 0) {
        if (n_records) *n_records = 0;
        return NRG_OK;
    }
    Staging* g = c->stg;
    if ((r = staging(g[0], data_bytes)) || (r = staging(g[1], n * 8)) || (r = staging(g[2], n))) return r;
    if (data_bytes) HIPCHK(hipMemcpyAsync(g[0].p, data, data_bytes, hipMemcpyHostToDevice, c->stream));
    if ((r = nrg_memfs_pwrite_async(c, reqs, n, data_bytes ? (const uint8_t*)g[0].p : nullptr, data_bytes, origin,
                                    written ? (uint64_t*)g[1].p : nullptr, written ? (uint8_t*)g[2].p : nullptr,
                                    n_records)))
        return r;
    if (written) {
        HIPCHK(hipMemcpyAsync(written, g[1].p, n * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(some, g[2].p, n, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(sync_all(c));
    return check_err(c);
}

int nrg_memfs_pwrite_records_async(nrg_ctx* c, const nrg_memfs_wr* reqs, uint64_t n, const uint8_t* d_data,
                                   uint64_t data_bytes, nrg_memfs_op* d_recs, uint64_t cap, uint64_t* n_records) {
    int r = mf_pwrite_check(c, reqs, n, d_data, data_bytes);
    if (r) return r;
    if ((uintptr_t)d_recs & 7) return NRG_E_INVAL;  // (records move as u64 words)
    if (n_records) *n_records = 0;
    if (n == 0) return NRG_OK;
    std::vector<uint64_t> first(n + 1);
    // admitted against the bound where one is set, against B otherwise; nothing grows here: the replay of
    // these records does
    const uint32_t adm = mf_admit_log2(c);
    if ((r = mfp::plan(adm, c->mf.files, reqs, n, data_bytes, first.data(), nullptr, nullptr))) return r;
    const uint64_t T = first[n];
    if (n_records) *n_records = T;
    if (T > cap) return NRG_E_CAPACITY;
    if (!d_recs) return NRG_E_INVAL;
    if ((r = mf_pwrite_upload(c, reqs, first.data(), n))) return r;
    return hip_fail(mf_frag_launch(c, n, 0, T, d_recs, 0, ~0ull, d_data, data_bytes, nullptr, nullptr, adm));
}

int nrg_memfs_pread_logged_plan(uint32_t log2_adm, uint64_t files, const nrg_memfs_rd* reqs, uint64_t n, uint64_t* first,
                                uint64_t* offs, uint8_t* some) {
    return mfp::read_plan(log2_adm, files, reqs, n, first, offs, some);
}

int nrg_memfs_pread_logged_async(nrg_ctx* c, const nrg_memfs_rd* reqs, uint64_t n, uint32_t origin, uint8_t* d_data,
                                 uint64_t cap, uint64_t* d_counts, uint8_t* d_some, uint64_t* offs, uint64_t* n_records) {
    int r = mf_rl_check(c, reqs, n);
    if (r) return r;
    if ((d_counts == nullptr) != (d_some == nullptr) || ((uintptr_t)d_counts & 7) || (cap && !d_data)) return NRG_E_INVAL;
    if (n_records) *n_records = 0;
    if (n == 0) {
        if (offs) offs[0] = 0;
        return NRG_OK;
    }
    const uint32_t adm = mf_admit_log2(c);
    std::vector<uint64_t> first, po;
    if ((r = mf_rl_plan(c, reqs, n, first, po))) return r;
    if (offs) memcpy(offs, po.data(), (n + 1) * 8);
    const uint64_t T = first[n];
    if (po[n] > cap) return NRG_E_CAPACITY;  // host-known: nothing is logged
    // catch up on anything appended by others first (Replica::combine execs the whole log)
    if ((r = exec_range(c, 0, 0, nullptr, nullptr))) return r;
    MfHost& s = c->mf;
    const uint64_t mb = c->cfg.max_batch;
    if (!s.d_rresp) HIPCHK(hipMalloc(&s.d_rresp, mb * sizeof(nrg_memfs_resp) + mb));
    uint8_t* const rsome = (uint8_t*)(s.d_rresp + mb * MF_RESP_WORDS);
    if ((r = mf_rl_upload(c, reqs, first.data(), po.data(), n))) return r;
    struct Planned {  // a pass of Reads needs no growth: no need check, no readback
        bool& f;
        explicit Planned(bool& x) : f(x) { f = true; }
        ~Planned() { f = false; }
    } planned(s.planned);
    // passes: what one append may carry and the scratch holds, so a pass is one replay chunk
    const uint64_t pass = append_max(c) < mb ? append_max(c) : mb;
    for (uint64_t done = 0; done < T;) {
        const uint64_t m = T - done < pass ? T - done : pass;
        if ((r = reserve(c, m))) return r;
        const uint64_t lo = c->tail;
        HIPCHK(mf_rfrag_launch(c, n, done, done + m, c->d_ring, lo, c->log_size - 1, adm));
        note_origin(c, lo, m, origin);
        c->tail = lo + m;
        if ((r = exec_range(c, lo, lo + m, s.d_rresp, rsome))) return r;
        HIPCHK(mf_rgather_launch(c, adm, reqs, first.data(), po.data(), n, done, done + m, s.d_rresp, rsome, d_data, d_counts,
                                 d_some));
        done += m;
    }
    if (n_records) *n_records = T;
    return NRG_OK;
}

int nrg_memfs_pread_logged(nrg_ctx* c, const nrg_memfs_rd* reqs, uint64_t n, uint32_t origin, uint8_t* data, uint64_t cap,
                           uint64_t* counts, uint8_t* some, uint64_t* offs, uint64_t* n_records) {
    int r = mf_rl_check(c, reqs, n);
    if (r) return r;
    if ((counts == nullptr) != (some == nullptr) || (cap && !data)) return NRG_E_INVAL;
    if (n == 0) {
        if (n_records) *n_records = 0;
        if (offs) offs[0] = 0;
        return NRG_OK;
    }
    std::vector<uint64_t> first, po;
    if ((r = mf_rl_plan(c, reqs, n, first, po))) return r;
    const uint64_t total = po[n] <= cap ? po[n] : 0;  // (above cap the call below refuses before it logs)
    Staging* g = c->stg;
    if ((r = staging(g[0], total ? total : 1)) || (r = staging(g[1], n * 8)) || (r = staging(g[2], n))) return r;
    if ((r = nrg_memfs_pread_logged_async(c, reqs, n, origin, (uint8_t*)g[0].p, cap, (uint64_t*)g[1].p, (uint8_t*)g[2].p, offs,
                                          n_records)))
        return r;
    // only a request's count bytes may land in the caller's data: through host copies of the slots
    std::vector<uint64_t> cn(n);
    std::vector<uint8_t> bytes(total);
    HIPCHK(hipMemcpyAsync(cn.data(), g[1].p, n * 8, hipMemcpyDeviceToHost, c->stream));
    if (some) HIPCHK(hipMemcpyAsync(some, g[2].p, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_all(c));
    uint64_t lo = ~0ull, hi = 0;  // the slot bytes that hold answers
    for (uint64_t i = 0; i < n; i++)
        if (cn[i]) lo = po[i] < lo ? po[i] : lo, hi = po[i] + cn[i] > hi ? po[i] + cn[i] : hi;
    if (hi > lo) {
        HIPCHK(hipMemcpyAsync(bytes.data() + lo, (uint8_t*)g[0].p + lo, hi - lo, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(sync_all(c));
    }
    for (uint64_t i = 0; i < n; i++) {
        if (cn[i]) memcpy(data + po[i], bytes.data() + po[i], cn[i]);
        if (counts) counts[i] = cn[i];
    }
    return check_err(c);
}

int nrg_memfs_pread_logged_records_async(nrg_ctx* c, const nrg_memfs_rd* reqs, uint64_t n, nrg_memfs_op* d_recs, uint64_t cap,
                                         uint64_t* n_records) {
    int r = mf_rl_check(c, reqs, n);
    if (r) return r;
    if ((uintptr_t)d_recs & 7) return NRG_E_INVAL;  // (records move as u64 words)
    if (n_records) *n_records = 0;
    if (n == 0) return NRG_OK;
    std::vector<uint64_t> first, po;
    if ((r = mf_rl_plan(c, reqs, n, first, po))) return r;
    const uint64_t T = first[n];
    if (n_records) *n_records = T;
    if (T > cap) return NRG_E_CAPACITY;
    if (!d_recs) return NRG_E_INVAL;
    if ((r = mf_rl_upload(c, reqs, first.data(), po.data(), n))) return r;
    return hip_fail(mf_rfrag_launch(c, n, 0, T, d_recs, 0, ~0ull, mf_admit_log2(c)));
}

int nrg_memfs_pread_logged_gather_async(nrg_ctx* c, const nrg_memfs_rd* reqs, uint64_t n, const nrg_memfs_resp* d_resp,
                                        const uint8_t* d_resp_some, uint64_t T, uint8_t* d_data, uint64_t cap,
                                        uint64_t* d_counts, uint8_t* d_some) {
    int r = mf_rl_check(c, reqs, n);
    if (r) return r;
    if ((d_counts == nullptr) != (d_some == nullptr) || (((uintptr_t)d_counts | (uintptr_t)d_resp) & 7) || (cap && !d_data))
        return NRG_E_INVAL;
    if (n == 0) return T ? NRG_E_INVAL : NRG_OK;
    std::vector<uint64_t> first, po;
    if ((r = mf_rl_plan(c, reqs, n, first, po))) return r;
    if (T != first[n] || !d_resp || !d_resp_some) return NRG_E_INVAL;
    if (po[n] > cap) return NRG_E_CAPACITY;
    if ((r = mf_rl_upload(c, reqs, first.data(), po.data(), n))) return r;
    return hip_fail(mf_rgather_launch(c, mf_admit_log2(c), reqs, first.data(), po.data(), n, 0, T, d_resp, d_resp_some, d_data,
                                      d_counts, d_some));
}

}  // extern "C"
