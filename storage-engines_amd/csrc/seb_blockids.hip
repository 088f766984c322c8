// seb_blockids.hip — the block-id step on the device: a located cell (slot, block offset)
// becomes an id of the block pool.  The rules and the host half are in seb_blockids.h / seb_blockids.cpp.
//
//   k_bid_resident  a grid-stride stream, a lane per cell: rules 1-3; a miss cell gets SEB_NO_BLOCK_ID.  The three
//                   counts are summed per wave and added once per wave.
//   k_bid_insert    a lane per cell: a miss cell's packed pair goes into the open-addressing table (linear probing,
//                   a counted loop of at most table-size steps) and the cell's index into the slot's minimum.  Every
//                   access to the table in this launch is an agent-scope atomic: the per-XCD L2s are not coherent
//                   with each other, and only what an atomic returned decides anything.  A lane that runs out of
//                   steps sets the overflow word, which the other lanes poll every 32 steps.
//   k_bid_flags     a workgroup per tile of kBidTile cells: the number of first appearances (the cell whose index
//                   is its slot's minimum).  The table is read with plain loads from here on: the passes hand
//                   over at kernel boundaries.
//   k_bid_scan      exclusive scan of the tile sums (seb_scan.h); the total and the header's constant words
//   k_bid_rank      a workgroup per tile, four consecutive cells per lane: each first cell's rank by a scan in the
//                   workgroup, written beside its slot
//   k_bid_emit      a lane per cell: rules 1-3 as k_bid_resident; a miss cell finds its slot again and writes
//                   id_base + rank; a first cell also writes its entry of the read list
//
// Workspace: a 128-byte header [magic][cells][table][max_uniq][resident][misses][bad][uniq][overflow][tiles], the
// table's pairs (u64 each, all ones = empty), its minima (u32), its ranks (u32), the tile sums (u64).  The emit
// stores nothing unless the header is the plan's that returned its `sizes`; a rank that is not below sizes.uniq
// stores nothing to the read list, and every probe is masked into the table.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "seb_blockids.h"
#include "seb_kernels.h"
#include "seb_scan.h"

namespace seb {

namespace {

typedef unsigned long long u64a;  // what the 64-bit atomics take

constexpr uint32_t BT = kBidTile;
constexpr uint64_t kBidMagic = 0x5344494B434F4C42ull;  // "BLOCKIDS"
constexpr u64a kEmpty = ~0ull;
enum : uint32_t { hMagic, hCells, hTable, hMaxUniq, hResident, hMisses, hBad, hUniq, hOverflow, hTiles };  // u64 words
constexpr uint64_t kHeadBytes = 128;

struct BidIn {  // the cells and the residency table
    const uint16_t *cand;
    const uint64_t *blocks;
    uint64_t cells;
    const uint32_t *res_first, *res_count;
    uint32_t res_slots;
};

struct BidWs {
    uint64_t *hdr;
    u64a *pairs;
    uint32_t *minidx, *rank;
    uint64_t *sums;
    uint64_t table, tiles;  // table: a power of two
};

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ uint64_t pair_hash(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    return x ^ x >> 31;
}

__device__ __forceinline__ BidKind classify(const BidIn &in, uint64_t c, uint32_t *id, uint64_t *pair) {
    return bid_classify(in.cand[c], in.blocks[c], in.res_first, in.res_count, in.res_slots, id, pair);
}

// per-lane counts -> one add per wave and counter; every lane of the wave calls it
__device__ __forceinline__ void add_counts(u64a *dst, u64a resident, u64a misses, u64a bad) {
    resident = wave_sum(resident), misses = wave_sum(misses), bad = wave_sum(bad);
    if ((threadIdx.x & 63) == 0) {
        if (resident) atomicAdd(dst + 0, resident);
        if (misses) atomicAdd(dst + 1, misses);
        if (bad) atomicAdd(dst + 2, bad);
    }
}

__global__ __launch_bounds__(256) void k_bid_resident(BidIn in, uint32_t *__restrict__ bid, u64a *counts) {
    u64a resident = 0, misses = 0, bad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x; c < in.cells; c += stride) {
        uint32_t id = kBidNoId;
        uint64_t pair;
        const BidKind k = classify(in, c, &id, &pair);
        resident += k == kBidResident, misses += k == kBidMiss, bad += k == kBidBad;
        bid[c] = id;
    }
    if (counts) add_counts(counts, resident, misses, bad);
}

#define BID_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ void table_insert(const BidWs &w, uint64_t pair, uint32_t c) {
    const uint64_t mask = w.table - 1;
    u64a *ovf = (u64a *)(w.hdr + hOverflow);
    uint64_t i = pair_hash(pair) & mask;
    for (uint64_t step = 0; step < w.table; ++step, i = (i + 1) & mask) {
        if ((step & 31) == 31 && __hip_atomic_load(ovf, BID_RLX_AGENT)) return;  // the plan fails anyway
        // a slot goes from empty to one pair once and then keeps it: a pair seen here stays; "empty" is only a
        // reason to try the exchange, whose returned value decides
        u64a cur = __hip_atomic_load(w.pairs + i, BID_RLX_AGENT);
        if (cur == kEmpty) {
            u64a seen = kEmpty;
            if (__hip_atomic_compare_exchange_strong(w.pairs + i, &seen, (u64a)pair, __ATOMIC_RELAXED, BID_RLX_AGENT))
                cur = pair;
            else
                cur = seen;
        }
        if (cur != pair) continue;
        // the minimum only falls: a value already at or below c makes the atomic needless
        if (__hip_atomic_load(w.minidx + i, BID_RLX_AGENT) > c) __hip_atomic_fetch_min(w.minidx + i, c, BID_RLX_AGENT);
        return;
    }
    __hip_atomic_store(ovf, (u64a)1, BID_RLX_AGENT);
}

__global__ __launch_bounds__(256) void k_bid_insert(BidIn in, BidWs w) {
    u64a resident = 0, misses = 0, bad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x; c < in.cells; c += stride) {
        uint32_t id;
        uint64_t pair;
        const BidKind k = classify(in, c, &id, &pair);
        resident += k == kBidResident, misses += k == kBidMiss, bad += k == kBidBad;
        if (k == kBidMiss) table_insert(w, pair, (uint32_t)c);
    }
    add_counts((u64a *)(w.hdr + hResident), resident, misses, bad);
}

// The pair's slot, read only; w.table for a pair the table does not hold.
__device__ __forceinline__ uint64_t table_find(const BidWs &w, uint64_t pair) {
    const uint64_t mask = w.table - 1;
    uint64_t i = pair_hash(pair) & mask;
    for (uint64_t step = 0; step < w.table; ++step, i = (i + 1) & mask) {
        const u64a cur = w.pairs[i];
        if (cur == pair) return i;
        if (cur == kEmpty) break;
    }
    return w.table;
}

// cell c is the first appearance of its pair; *slot = the pair's slot
__device__ __forceinline__ bool first_cell(const BidIn &in, const BidWs &w, uint64_t c, uint64_t *slot) {
    uint32_t id;
    uint64_t pair;
    if (c >= in.cells || classify(in, c, &id, &pair) != kBidMiss) return false;
    *slot = table_find(w, pair);
    return *slot < w.table && w.minidx[*slot] == (uint32_t)c;
}

__global__ __launch_bounds__(256) void k_bid_flags(BidIn in, BidWs w) {
    __shared__ unsigned long long acc;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) acc = 0;
    __syncthreads();
    unsigned long long cnt = 0;
    if (w.hdr[hOverflow] == 0) {
        const uint64_t ts = (uint64_t)blockIdx.x * BT;
        for (uint32_t q = 0; q < BT / 256; ++q) {
            uint64_t slot;
            cnt += first_cell(in, w, ts + q * 256 + tid, &slot);
        }
    }
    cnt = wave_sum(cnt);
    if ((tid & 63) == 0 && cnt) atomicAdd(&acc, cnt);
    __syncthreads();
    if (tid == 0) w.sums[blockIdx.x] = acc;
}

__global__ __launch_bounds__(kScanWidth) void k_bid_scan(BidIn in, BidWs w, uint64_t max_uniq) {
    scan_tile_sums(w.sums, w.tiles, w.hdr + hUniq);
    if (threadIdx.x == 0)
        w.hdr[hMagic] = kBidMagic, w.hdr[hCells] = in.cells, w.hdr[hTable] = w.table, w.hdr[hMaxUniq] = max_uniq,
        w.hdr[hTiles] = w.tiles;
}

__global__ __launch_bounds__(256) void k_bid_rank(BidIn in, BidWs w) {
    __shared__ uint32_t wcnt[4];
    if (w.hdr[hOverflow] != 0) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t first = (uint64_t)blockIdx.x * BT + 4 * tid;
    bool f[4];
    uint64_t slot[4];
    uint32_t c = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        f[q] = first_cell(in, w, first + q, &slot[q]);
        c += f[q];
    }
    uint32_t ic = c;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(ic, d, 64);
        if (lane >= d) ic += t;
    }
    if (lane == 63) wcnt[wv] = ic;
    __syncthreads();
    uint64_t r = w.sums[blockIdx.x] + (ic - c);
#pragma unroll
    for (uint32_t v = 0; v < 4; ++v)
        if (v < wv) r += wcnt[v];
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q)
        if (f[q]) w.rank[slot[q]] = (uint32_t)(r++);  // slot < table: first_cell found it
}

struct BidSizes {  // seb_blockids_sizes
    uint64_t cells, resident, misses, uniq, bad, reserved;
};

__global__ __launch_bounds__(256) void k_bid_emit(BidIn in, BidWs w, BidSizes sz, uint64_t max_uniq, uint32_t id_base,
                                                  uint32_t *__restrict__ bid, uint16_t *__restrict__ uniq_slot,
                                                  uint64_t *__restrict__ uniq_block) {
    const uint64_t *h = w.hdr;
    if (h[hMagic] != kBidMagic || h[hCells] != sz.cells || in.cells != sz.cells || h[hTable] != w.table ||
        h[hMaxUniq] != max_uniq || h[hTiles] != w.tiles || h[hOverflow] != 0 || h[hResident] != sz.resident ||
        h[hMisses] != sz.misses || h[hBad] != sz.bad || h[hUniq] != sz.uniq)
        return;  // not the plan that returned these sizes
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x; c < in.cells; c += stride) {
        uint32_t id = kBidNoId;
        uint64_t pair;
        if (classify(in, c, &id, &pair) == kBidMiss) {
            const uint64_t slot = table_find(w, pair);
            if (slot < w.table) {
                const uint64_t r = w.rank[slot];
                if (r < sz.uniq) {  // also keeps id_base + r below 2^32 - 1: the host checked id_base + uniq
                    id = id_base + (uint32_t)r;
                    if (w.minidx[slot] == (uint32_t)c) {
                        uniq_slot[r] = (uint16_t)(pair >> 48);
                        uniq_block[r] = pair & ((1ull << 48) - 1);
                    }
                }
            }
        }
        bid[c] = id;
    }
}

inline uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

// the smallest power of two >= 2 * max_uniq, at least 4
inline uint64_t table_slots(uint64_t max_uniq) {
    uint64_t t = 4;
    while (t < 2 * max_uniq) t <<= 1;
    return t;
}

inline BidWs ws_layout(void *ws, uint64_t cells, uint64_t max_uniq) {
    BidWs w;
    w.table = table_slots(max_uniq);
    w.tiles = (cells + BT - 1) / BT;
    uint8_t *p = (uint8_t *)ws;
    w.hdr = (uint64_t *)p;
    w.pairs = (u64a *)(p + kHeadBytes);
    w.minidx = (uint32_t *)(p + kHeadBytes + 8 * w.table);
    w.rank = w.minidx + w.table;
    w.sums = (uint64_t *)(p + kHeadBytes + 16 * w.table);
    return w;
}

hipError_t drained(hipStream_t s, hipError_t e) {
    (void)hipStreamSynchronize(s);
    return e;
}

}  // namespace

uint64_t blockids_max_uniq(uint64_t cells, uint64_t max_uniq) { return max_uniq < cells ? max_uniq : cells; }

uint64_t blockids_ws_bytes(uint64_t cells, uint64_t max_uniq) {
    return kHeadBytes + 16 * table_slots(blockids_max_uniq(cells, max_uniq)) + up16(8 * ((cells + BT - 1) / BT));
}

hipError_t launch_blockids_resident(const uint16_t *cand, const uint64_t *blocks, uint64_t cells, const uint32_t *res_first,
                                    const uint32_t *res_count, uint32_t res_slots, uint32_t *bid, uint64_t *counts,
                                    hipStream_t s) {
    hipError_t e;
    if (counts && (e = hipMemsetAsync(counts, 0, 24, s)) != hipSuccess) return e;
    const BidIn in{cand, blocks, cells, res_first, res_count, res_slots};
    hipLaunchKernelGGL(k_bid_resident, dim3(stream_grid(cells)), dim3(256), 0, s, in, bid, (u64a *)counts);
    return hipGetLastError();
}

hipError_t launch_blockids_plan(const uint16_t *cand, const uint64_t *blocks, uint64_t cells, const uint32_t *res_first,
                                const uint32_t *res_count, uint32_t res_slots, uint64_t max_uniq, void *ws,
                                void *sizes_host, bool *overflow, hipStream_t s) {
    max_uniq = blockids_max_uniq(cells, max_uniq);
    const BidIn in{cand, blocks, cells, res_first, res_count, res_slots};
    const BidWs w = ws_layout(ws, cells, max_uniq);
    hipError_t e;
    if ((e = hipMemsetAsync(w.hdr, 0, kHeadBytes, s)) != hipSuccess) return drained(s, e);
    if ((e = hipMemsetAsync(w.pairs, 0xFF, 16 * w.table, s)) != hipSuccess) return drained(s, e);  // pairs, minima, ranks
    hipLaunchKernelGGL(k_bid_insert, dim3(stream_grid(cells)), dim3(256), 0, s, in, w);
    hipLaunchKernelGGL(k_bid_flags, dim3((unsigned)w.tiles), dim3(256), 0, s, in, w);
    hipLaunchKernelGGL(k_bid_scan, dim3(1), dim3(kScanWidth), 0, s, in, w, max_uniq);
    hipLaunchKernelGGL(k_bid_rank, dim3((unsigned)w.tiles), dim3(256), 0, s, in, w);
    if ((e = hipGetLastError()) != hipSuccess) return drained(s, e);
    uint64_t h[kHeadBytes / 8];
    if ((e = hipMemcpyAsync(h, w.hdr, sizeof h, hipMemcpyDeviceToHost, s)) != hipSuccess) return drained(s, e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    *overflow = h[hOverflow] != 0;
    // a table that filled held more than max_uniq distinct pairs; which number is not known
    const uint64_t out[6] = {cells, h[hResident], h[hMisses], *overflow ? max_uniq + 1 : h[hUniq], h[hBad], 0};
    memcpy(sizes_host, out, sizeof out);
    return hipSuccess;
}

hipError_t launch_blockids_emit(const uint16_t *cand, const uint64_t *blocks, uint64_t cells, const uint32_t *res_first,
                                const uint32_t *res_count, uint32_t res_slots, uint64_t max_uniq, uint32_t id_base,
                                const void *sizes, const void *ws, uint32_t *bid, uint16_t *uniq_slot, uint64_t *uniq_block,
                                hipStream_t s) {
    max_uniq = blockids_max_uniq(cells, max_uniq);
    BidSizes sz;
    memcpy(&sz, sizes, sizeof sz);
    const BidIn in{cand, blocks, cells, res_first, res_count, res_slots};
    const BidWs w = ws_layout(const_cast<void *>(ws), cells, max_uniq);
    hipLaunchKernelGGL(k_bid_emit, dim3(stream_grid(cells)), dim3(256), 0, s, in, w, sz, max_uniq, id_base, bid, uniq_slot,
                       uniq_block);
    return hipGetLastError();
}

}  // namespace seb
