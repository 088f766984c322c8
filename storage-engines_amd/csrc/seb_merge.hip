// seb_merge.hip — batched compaction merge on the device: k sorted runs of a block pool into one sorted,
// de-duplicated run in the SSTable builder's input layout.
//
// What mergeFiles computes before its builder (lsm/compaction.go:226-333): loadBlock's walk over every block
// (:69-124), a k-way merge by key, one entry per distinct key, tombstones dropped at the last level.  Of
// several entries with one key the entry of the lowest-numbered run survives (seb_bloom.h states why this
// departs from the reference's heap-dependent choice).
//
//   k_merge_count   a lane per block: loadBlock's walk in global memory, the block's entry count
//   k_merge_groups, k_merge_scan, k_merge_spread   exclusive scan of the counts in three steps (sums of 256
//                   blocks, their scan by one workgroup, the scan inside each group): each block's first
//                   record, and the total
//   k_merge_runs    each run's first record
//   k_merge_decode  a lane per block again: one 32-byte record per entry (the key's first 16 bytes as two
//                   big-endian words, the entry's place in the pool, its lengths, the deleted bit)
//   k_merge_check   adjacent records of a run must increase strictly: the least (run, entry) that does not
//   k_merge_cuts, k_merge_pass   one level of a stable pairwise merge tree over records: runs [2jw, 2jw + w) and
//                   [2jw + w, 2jw + 2w) into one.  A workgroup makes kMergeTile consecutive outputs of a pair:
//                   two merge-path diagonal searches in global memory (k_merge_cuts: a lane per search, all of
//                   a pass's tiles at once) bound its inputs, they go to LDS, and
//                   every record finds its output rank by a bisection of the other side (a record of the left
//                   side counts the right side's records below it, one of the right side the left side's
//                   records at or below it: ties take the left, lower-numbered side first)
//   k_merge_mark    after the last level equal keys are adjacent, the lowest run first: the survivor is the
//                   first of its group, unless it is a tombstone to drop; per tile of kMergeTile records the
//                   survivors' count, key bytes and value bytes
//   k_merge_scan    exclusive scan of the tiles' three sums (one workgroup each); the totals are the sizes
//   k_merge_emit    per tile: the survivors' offsets by a scan in the workgroup, key_off / val_off / deleted,
//                   then the tile's two output ranges (its keys, its values), each contiguous, filled 16
//                   aligned bytes at a time: a chunk inside one entry is two aligned 16-byte loads and a
//                   shift, a chunk across entries and the ranges' ends go byte by byte
// Records compare by their prefix words; only a tie on all 16 bytes reads key bytes from the pool.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <utility>
#include <vector>

#include "seb_kernels.h"

namespace seb {

constexpr uint32_t MT = kMergeTile;
constexpr uint32_t kMergeMaxPerBlock = 454;  // entries a block can hold: 4 + 9 * 454 = 4090

struct __attribute__((aligned(16))) MergeRec {
    uint64_t k0, k1;  // the key's first 16 bytes, zero padded, big-endian
    uint32_t blk;     // the entry's 9-byte header is at pool[blk * 4096 + off]
    uint16_t off, klen, vlen;
    uint8_t del, keep;  // deleted == 1; keep: set by k_merge_mark
    uint32_t pad;
};
static_assert(sizeof(MergeRec) == 32, "MergeRec layout");

// the workspace header (u64 words)
enum : uint32_t { kHdrErr = 0, kHdrTotal = 1, kHdrRec = 2, kHdrSums = 3, kHdrOut = 4, kHdrKey = 5, kHdrVal = 6,
                  kHdrShadowed = 7, kHdrDropped = 8, kHdrTiles = 9 };

typedef const __attribute__((address_space(1))) uint8_t *gbytes;

__device__ __forceinline__ uint32_t gle32(gbytes p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

__device__ __forceinline__ uint64_t be64g(gbytes p, uint32_t len) {  // first min(len, 8) bytes, big-endian
    uint64_t v = 0;
    for (uint32_t i = 0; i < 8; ++i) v = (v << 8) | (i < len ? p[i] : 0u);
    return v;
}

// loadBlock's walk over blk[0, L), L <= kBlockBytes; every read is below L.  With out != nullptr entry i < cap
// becomes out[i]; the count is returned either way.
__device__ __forceinline__ uint32_t walk_block(const uint8_t *blk, uint32_t L, uint32_t b, MergeRec *out, uint32_t cap) {
    if (L < 4) return 0;
    gbytes g = (gbytes)blk;
    const uint32_t num = gle32(g);
    uint32_t off = 4, c = 0;
    for (uint32_t i = 0; i < num; ++i) {
        if (off + 9 > L) break;
        const uint32_t ks = gle32(g + off), vs = gle32(g + off + 4);
        if ((uint64_t)off + 9 + ks + vs > L) break;
        if (out) {
            if (c >= cap) break;
            MergeRec r;
            const uint32_t at = off + 9;
            if (at + 16 <= L) {  // two 8-byte loads, the bytes past the key masked off
                uint64_t a, d;
                __builtin_memcpy(&a, g + at, 8);
                __builtin_memcpy(&d, g + at + 8, 8);
                const uint64_t va = __builtin_bswap64(a), vd = __builtin_bswap64(d);
                r.k0 = ks >= 8 ? va : ks == 0 ? 0ull : va & (~0ull << (8 * (8 - ks)));
                r.k1 = ks >= 16 ? vd : ks <= 8 ? 0ull : vd & (~0ull << (8 * (16 - ks)));
            } else {  // the block's last bytes: ks <= L - at < 16
                r.k0 = be64g(g + at, ks);
                r.k1 = ks > 8 ? be64g(g + at + 8, ks - 8) : 0ull;
            }
            r.blk = b;
            r.off = (uint16_t)off;
            r.klen = (uint16_t)ks;
            r.vlen = (uint16_t)vs;
            r.del = g[off + 8] == 1 ? 1 : 0;
            r.keep = 0;
            r.pad = 0;
            out[c] = r;
        }
        ++c;
        off += 9 + ks + vs;
    }
    return c;
}

__global__ __launch_bounds__(256) void k_merge_count(const uint8_t *__restrict__ pool, const uint16_t *__restrict__ blen,
                                                     uint32_t nblocks, uint16_t *__restrict__ cnt) {
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= nblocks) return;
    uint32_t L = blen[b];
    if (L > kBlockBytes) L = kBlockBytes;
    cnt[b] = (uint16_t)walk_block(pool + b * kBlockBytes, L, (uint32_t)b, nullptr, 0);
}

// The blocks' first records in three steps, a group being 256 consecutive blocks: k_merge_groups sums each
// group's counts, k_merge_scan (below) scans the group sums in place and leaves the total in the header, and
// k_merge_spread scans inside each group: first[b] = the records before block b, first[nblocks] = all.
__device__ __forceinline__ uint32_t scan256(uint32_t v, uint32_t *X) {  // inclusive, over the workgroup's 256 lanes
    const uint32_t tid = threadIdx.x;
    X[tid] = v;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const uint32_t a = tid >= d ? X[tid - d] : 0;
        __syncthreads();
        X[tid] += a;
        __syncthreads();
    }
    return X[tid];
}

__global__ __launch_bounds__(256) void k_merge_groups(const uint16_t *__restrict__ cnt, uint32_t nblocks,
                                                      uint64_t *__restrict__ gsum) {
    __shared__ uint32_t X[256];
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t c = b < nblocks ? (cnt[b] < kMergeMaxPerBlock ? cnt[b] : kMergeMaxPerBlock) : 0;
    const uint32_t inc = scan256(c, X);
    if (threadIdx.x == 255) gsum[blockIdx.x] = inc;
}

__global__ __launch_bounds__(256) void k_merge_spread(const uint16_t *__restrict__ cnt, uint32_t nblocks,
                                                      const uint64_t *__restrict__ gbase, uint32_t *__restrict__ first) {
    __shared__ uint32_t X[256];
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t c = b < nblocks ? (cnt[b] < kMergeMaxPerBlock ? cnt[b] : kMergeMaxPerBlock) : 0;
    const uint64_t inc = gbase[blockIdx.x] + scan256(c, X);
    if (b < nblocks) first[b] = (uint32_t)(inc - c);
    if (b + 1 == nblocks) first[nblocks] = (uint32_t)inc;
}

// rf[r] = run r's first record, r = 0 .. nruns (run_begin[r] <= nblocks is checked on the host)
__global__ __launch_bounds__(256) void k_merge_runs(const uint64_t *__restrict__ run_begin, uint32_t nruns,
                                                    const uint32_t *__restrict__ first, uint64_t *__restrict__ rf) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r <= nruns) rf[r] = first[run_begin[r]];
}

// Block b's records at rec[first[b], first[b+1]): the walk again, never past the count the scan used; a block
// that now yields fewer entries (a pool changed since the count) leaves empty-key records that read nothing.
__global__ __launch_bounds__(256) void k_merge_decode(const uint8_t *__restrict__ pool, const uint16_t *__restrict__ blen,
                                                      uint32_t nblocks, const uint32_t *__restrict__ first,
                                                      uint64_t n, MergeRec *__restrict__ rec) {
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= nblocks) return;
    const uint64_t f0 = first[b], f1 = first[b + 1];
    if (f0 >= f1 || f1 > n || f1 - f0 > kMergeMaxPerBlock) return;
    const uint32_t cap = (uint32_t)(f1 - f0);
    uint32_t L = blen[b];
    if (L > kBlockBytes) L = kBlockBytes;
    const uint32_t c = walk_block(pool + b * kBlockBytes, L, (uint32_t)b, rec + f0, cap);
    MergeRec z{};
    for (uint32_t i = c; i < cap; ++i) rec[f0 + i] = z;
}

// Go string order of two records' keys: the prefix words, then on a tie of all 16 bytes the key bytes past
// them in the pool (both keys longer than 16), then the lengths.
__device__ __forceinline__ int rec_cmp(uint64_t ak0, uint64_t ak1, uint32_t ablk, uint32_t aoff, uint32_t aklen,
                                       uint64_t bk0, uint64_t bk1, uint32_t bblk, uint32_t boff, uint32_t bklen,
                                       const uint8_t *__restrict__ pool) {
    if (ak0 != bk0) return ak0 < bk0 ? -1 : 1;
    if (ak1 != bk1) return ak1 < bk1 ? -1 : 1;
    const uint32_t m = aklen < bklen ? aklen : bklen;
    if (m > 16) {
        gbytes pa = (gbytes)pool + (uint64_t)ablk * kBlockBytes + aoff + 9;
        gbytes pb = (gbytes)pool + (uint64_t)bblk * kBlockBytes + boff + 9;
        for (uint32_t i = 16; i < m; ++i)
            if (pa[i] != pb[i]) return pa[i] < pb[i] ? -1 : 1;
    }
    return (int)aklen - (int)bklen;
}

__device__ __forceinline__ int rec_cmp(const MergeRec &a, const MergeRec &b, const uint8_t *__restrict__ pool) {
    return rec_cmp(a.k0, a.k1, a.blk, a.off, a.klen, b.k0, b.k1, b.blk, b.off, b.klen, pool);
}

__global__ __launch_bounds__(256) void k_merge_check(const MergeRec *__restrict__ rec, uint64_t n,
                                                     const uint64_t *__restrict__ rf, uint32_t nruns,
                                                     const uint8_t *__restrict__ pool, uint64_t *__restrict__ hdr) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x + 1;
    if (e >= n) return;
    if (rec_cmp(rec[e - 1], rec[e], pool) < 0) return;
    uint32_t lo = 0, hi = nruns - 1;  // the last run that starts at or before e: the one that holds it
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1) >> 1);
        if (rf[mid] <= e) lo = mid; else hi = mid - 1;
    }
    if (rf[lo] == e) return;  // a run's first record has no predecessor
    atomicMin((unsigned long long *)&hdr[kHdrErr], (unsigned long long)lo << 32 | (e - rf[lo]));
}

// ------------------------------------------------------------------ the merge tree ----------

__device__ __forceinline__ MergeRec rec_load(const MergeRec *__restrict__ p) {
    union { uint4 q[2]; MergeRec r; } u;
    u.q[0] = ((const uint4 *)p)[0];
    u.q[1] = ((const uint4 *)p)[1];
    return u.r;
}

// the number of A's records among the first d outputs of merge(A[0, na), B[0, nb)), ties taking A first
__device__ __forceinline__ uint64_t merge_path(const MergeRec *__restrict__ A, uint64_t na, const MergeRec *__restrict__ B,
                                               uint64_t nb, uint64_t d, const uint8_t *__restrict__ pool) {
    uint64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        const MergeRec a = rec_load(A + mid), b = rec_load(B + (d - 1 - mid));
        if (rec_cmp(a, b, pool) <= 0) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// A tile of a pass: its pair's two sides in src and the diagonals it lies between.
struct MergeTile {
    uint64_t a0, a1, na, nb, d0, d1;  // A = src[a0, a0 + na), B = src[a1, a1 + nb), outputs [d0, d1) of the pair
};
__device__ __forceinline__ MergeTile merge_tile(const uint64_t *__restrict__ rf, uint32_t nruns, uint32_t w, uint2 t) {
    MergeTile m;
    const uint64_t r0 = 2ull * t.x * w, r1 = r0 + w, r2 = r1 + w;
    m.a0 = rf[r0 < nruns ? r0 : nruns], m.a1 = rf[r1 < nruns ? r1 : nruns];
    m.na = m.a1 - m.a0, m.nb = rf[r2 < nruns ? r2 : nruns] - m.a1;
    m.d0 = (uint64_t)t.y * MT;
    m.d1 = m.d0 + MT < m.na + m.nb ? m.d0 + MT : m.na + m.nb;
    return m;
}

// cuts[2t], cuts[2t + 1] = the left side's records before tile t's first and last diagonal: every tile's two
// searches (≈23 dependent pairs of loads each) run side by side here, not at the head of each merge workgroup
// (1.98 -> 1.75 ms per plan of the 10M-entry shape; tools/diag/merge_inline_search.patch).
__global__ __launch_bounds__(256) void k_merge_cuts(const MergeRec *__restrict__ src, const uint64_t *__restrict__ rf,
                                                    uint32_t nruns, uint32_t w, const uint2 *__restrict__ tab,
                                                    uint32_t ntiles, const uint8_t *__restrict__ pool,
                                                    uint32_t *__restrict__ cuts) {
    const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= 2ull * ntiles) return;
    const MergeTile m = merge_tile(rf, nruns, w, tab[x >> 1]);
    uint64_t d = x & 1 ? m.d1 : m.d0;
    if (d > m.na + m.nb) d = m.na + m.nb;
    cuts[x] = (uint32_t)merge_path(src + m.a0, m.na, src + m.a1, m.nb, d, pool);
}

__global__ __launch_bounds__(256) void k_merge_pass(const MergeRec *__restrict__ src, MergeRec *__restrict__ dst,
                                                    const uint64_t *__restrict__ rf, uint32_t nruns, uint32_t w,
                                                    const uint2 *__restrict__ tab, const uint32_t *__restrict__ cuts,
                                                    const uint8_t *__restrict__ pool) {
    __shared__ uint64_t sk0[MT], sk1[MT];
    __shared__ uint4 sm[MT];  // blk, off | klen << 16, vlen | del << 16 | keep << 24, pad
    const uint32_t tid = threadIdx.x;
    const MergeTile mt = merge_tile(rf, nruns, w, tab[blockIdx.x]);
    const uint64_t a0 = mt.a0, d0 = mt.d0, d1 = mt.d1;
    if (d0 >= mt.na + mt.nb) return;  // not a tile of this pass (the same for the whole workgroup)
    const MergeRec *A = src + a0, *B = src + mt.a1;
    const uint64_t i0 = cuts[2 * blockIdx.x], i1 = cuts[2 * blockIdx.x + 1];
    if (i0 > d0 || i1 > d1 || i1 < i0 || i1 > mt.na || d1 - i1 > mt.nb || d1 - i1 < d0 - i0) return;  // not this tile's cuts
    const uint64_t j0 = d0 - i0;
    const uint32_t ta = (uint32_t)(i1 - i0), tb = (uint32_t)((d1 - i1) - j0);  // ta + tb = d1 - d0 <= MT
    if (ta > MT || tb > MT - ta) return;
    for (uint32_t x = tid; x < ta + tb; x += 256) {
        const MergeRec *p = x < ta ? A + i0 + x : B + j0 + (x - ta);
        const uint4 q0 = ((const uint4 *)p)[0], q1 = ((const uint4 *)p)[1];
        sk0[x] = (uint64_t)q0.x | (uint64_t)q0.y << 32;
        sk1[x] = (uint64_t)q0.z | (uint64_t)q0.w << 32;
        sm[x] = q1;
    }
    __syncthreads();
    for (uint32_t x = tid; x < ta + tb; x += 256) {
        const uint64_t k0 = sk0[x], k1 = sk1[x];
        const uint4 m = sm[x];
        const bool left = x < ta;
        // left: the right side's records below this one; right: the left side's records at or below it
        uint32_t lo = left ? ta : 0, hi = left ? ta + tb : ta;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            const uint4 o = sm[mid];
            const int c = rec_cmp(sk0[mid], sk1[mid], o.x, o.y & 0xFFFFu, o.y >> 16, k0, k1, m.x, m.y & 0xFFFFu, m.y >> 16, pool);
            if (left ? c < 0 : c <= 0) lo = mid + 1; else hi = mid;
        }
        const uint32_t rank = left ? x + (lo - ta) : (x - ta) + lo;
        uint4 *o = (uint4 *)(dst + a0 + d0 + rank);
        o[0] = make_uint4((uint32_t)k0, (uint32_t)(k0 >> 32), (uint32_t)k1, (uint32_t)(k1 >> 32));
        o[1] = m;
    }
}

// ------------------------------------------------------------------ survivors ---------------

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(256) void k_merge_mark(MergeRec *__restrict__ rec, uint64_t n, uint32_t flags,
                                                    const uint8_t *__restrict__ pool, uint64_t *__restrict__ sums,
                                                    uint64_t tiles, uint64_t *__restrict__ hdr) {
    __shared__ unsigned long long acc[5];
    const uint32_t tid = threadIdx.x;
    if (tid < 5) acc[tid] = 0;
    __syncthreads();
    const uint64_t ts = (uint64_t)blockIdx.x * MT;
    unsigned long long cnt = 0, kb = 0, vb = 0, sh = 0, dr = 0;
    for (uint32_t q = 0; q < MT / 256; ++q) {
        const uint64_t e = ts + q * 256 + tid;
        if (e >= n) break;
        const MergeRec r = rec_load(rec + e);
        bool keep = true;
        if (e > 0 && rec_cmp(rec_load(rec + e - 1), r, pool) == 0) keep = false, ++sh;
        if (keep && r.del && (flags & 1u)) keep = false, ++dr;
        rec[e].keep = keep ? 1 : 0;
        if (keep) ++cnt, kb += r.klen, vb += r.vlen;
    }
    cnt = wave_sum(cnt), kb = wave_sum(kb), vb = wave_sum(vb), sh = wave_sum(sh), dr = wave_sum(dr);
    if ((tid & 63) == 0) {
        atomicAdd(&acc[0], cnt), atomicAdd(&acc[1], kb), atomicAdd(&acc[2], vb), atomicAdd(&acc[3], sh), atomicAdd(&acc[4], dr);
    }
    __syncthreads();
    if (tid == 0) {
        sums[blockIdx.x] = acc[0];
        sums[tiles + blockIdx.x] = acc[1];
        sums[2 * tiles + blockIdx.x] = acc[2];
        if (acc[3]) atomicAdd((unsigned long long *)&hdr[kHdrShadowed], acc[3]);
        if (acc[4]) atomicAdd((unsigned long long *)&hdr[kHdrDropped], acc[4]);
    }
}

// x = the exclusive scan of x in place, *total = the sum; one workgroup
__global__ __launch_bounds__(1024) void k_merge_scan(uint64_t *x, uint64_t count, uint64_t *total) {
    __shared__ uint64_t X[1024];
    __shared__ uint64_t carry_s;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (uint64_t base = 0; base < count; base += 1024) {
        const uint64_t v = base + tid < count ? x[base + tid] : 0;
        X[tid] = v;
        __syncthreads();
        for (uint32_t d = 1; d < 1024; d <<= 1) {
            const uint64_t a = tid >= d ? X[tid - d] : 0;
            __syncthreads();
            X[tid] += a;
            __syncthreads();
        }
        const uint64_t carry = carry_s;
        if (base + tid < count) x[base + tid] = carry + X[tid] - v;
        __syncthreads();
        if (tid == 1023) carry_s = carry + X[tid];
        __syncthreads();
    }
    if (tid == 0) *total = carry_s;
}

// ------------------------------------------------------------------ the emit ----------------

// One of a tile's two output ranges: dst[0, total) (dst = the output array + the tile's base, any alignment)
// is the concatenation of the tile's survivors' keys (or values); q[i] = survivor i's offset in it
// (q[cnt] = total), its bytes are at pool + sp[i].  room = the bytes the caller's array still holds from dst.
__device__ __forceinline__ void emit_stream(uint8_t *__restrict__ dst, uint32_t total, uint64_t room, const uint32_t *q,
                                            const uint64_t *sp, uint32_t cnt, const uint8_t *__restrict__ pool) {
    if (total == 0 || cnt == 0) return;
    if (room < total) total = (uint32_t)room;
    const uint64_t a = (uint64_t)dst, a0 = a & ~15ull;
    const uint32_t lead = (uint32_t)(a - a0), chunks = (lead + total + 15) >> 4;
    for (uint32_t c = threadIdx.x; c < chunks; c += blockDim.x) {
        const int64_t j0 = (int64_t)((uint64_t)c << 4) - (int64_t)lead;  // the chunk's first byte as a range position
        const uint32_t lo = j0 < 0 ? 0u : (uint32_t)j0, hi = (uint64_t)(j0 + 16) < total ? (uint32_t)(j0 + 16) : total;
        uint32_t i = 0, ih = cnt - 1;  // the last survivor with q[i] <= lo: the one that holds byte lo
        while (i < ih) {
            const uint32_t mid = (i + ih + 1) >> 1;
            if (q[mid] <= lo) i = mid; else ih = mid - 1;
        }
        uint32_t end = q[i + 1];
        const bool full = j0 >= 0 && (uint64_t)j0 + 16 <= total;
        if (full && lo + 16 <= end) {  // inside one entry: 16 source bytes at any alignment
            const uint64_t s = (uint64_t)pool + sp[i] + (lo - q[i]), s0 = s & ~15ull;
            uint32_t sh = (uint32_t)(s - s0);
            const uint4 u = *(const uint4 *)s0;
            uint64_t w0 = (uint64_t)u.x | (uint64_t)u.y << 32, w1 = (uint64_t)u.z | (uint64_t)u.w << 32;
            if (sh) {  // the second aligned word lies inside the pool: its last byte is below s + 16
                const uint4 v = *(const uint4 *)(s0 + 16);
                uint64_t w2 = (uint64_t)v.x | (uint64_t)v.y << 32, w3 = (uint64_t)v.z | (uint64_t)v.w << 32;
                if (sh >= 8) w0 = w1, w1 = w2, w2 = w3, sh -= 8;
                if (sh) {
                    const uint32_t bits = 8 * sh;
                    w0 = w0 >> bits | w1 << (64 - bits);
                    w1 = w1 >> bits | w2 << (64 - bits);
                }
            }
            *(uint4 *)(a0 + ((uint64_t)c << 4)) = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
        } else {
            gbytes src = (gbytes)pool + sp[i];
            uint32_t beg = q[i];
            for (uint32_t j = lo; j < hi; ++j) {
                while (j >= end) {  // j < total = q[cnt]: ends with i < cnt
                    ++i;
                    beg = end;
                    end = q[i + 1];
                    src = (gbytes)pool + sp[i];
                }
                dst[j] = src[j - beg];
            }
        }
    }
}

struct MergeSizesArg {  // seb_merge_sizes
    uint64_t entries_in, entries_out, key_bytes, val_bytes, shadowed, dropped;
};

__global__ __launch_bounds__(256) void k_merge_emit(const uint8_t *__restrict__ pool, const uint8_t *__restrict__ ws,
                                                    MergeSizesArg sz, uint8_t *__restrict__ keys,
                                                    uint64_t *__restrict__ key_off, uint8_t *__restrict__ vals,
                                                    uint64_t *__restrict__ val_off, uint8_t *__restrict__ deleted) {
    __shared__ uint32_t lk[MT + 1], lv[MT + 1];
    __shared__ uint64_t spk[MT], spv[MT];
    __shared__ uint32_t sc[256], sk[256], sv[256];
    const uint32_t tid = threadIdx.x;
    const uint64_t *hdr = (const uint64_t *)ws;
    const uint64_t n = sz.entries_in, tiles = (n + MT - 1) / MT;
    if (hdr[kHdrTotal] != n || hdr[kHdrTiles] != tiles) return;  // not this plan's sizes
    const MergeRec *rec = (const MergeRec *)(ws + hdr[kHdrRec]);
    const uint64_t *sums = (const uint64_t *)(ws + hdr[kHdrSums]);
    const uint64_t ts = (uint64_t)blockIdx.x * MT;
    const uint64_t obase = sums[blockIdx.x], kbase = sums[tiles + blockIdx.x], vbase = sums[2 * tiles + blockIdx.x];
    // a thread takes 4 consecutive records
    MergeRec r[4];
    uint32_t c = 0, ks = 0, vs = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        const uint64_t e = ts + 4 * tid + q;
        r[q].keep = 0;
        if (e < n) r[q] = rec_load(rec + e);
        if (r[q].keep) ++c, ks += r[q].klen, vs += r[q].vlen;
    }
    sc[tid] = c, sk[tid] = ks, sv[tid] = vs;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const uint32_t x = tid >= d ? sc[tid - d] : 0, y = tid >= d ? sk[tid - d] : 0, z = tid >= d ? sv[tid - d] : 0;
        __syncthreads();
        sc[tid] += x, sk[tid] += y, sv[tid] += z;
        __syncthreads();
    }
    const uint32_t cnt = sc[255], ktot = sk[255], vtot = sv[255];
    uint32_t ci = sc[tid] - c, ko = sk[tid] - ks, vo = sv[tid] - vs;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        if (!r[q].keep) continue;
        lk[ci] = ko, lv[ci] = vo;
        spk[ci] = (uint64_t)r[q].blk * kBlockBytes + r[q].off + 9;
        spv[ci] = spk[ci] + r[q].klen;
        const uint64_t o = obase + ci;
        if (o < sz.entries_out) {
            key_off[o] = kbase + ko;
            val_off[o] = vbase + vo;
            deleted[o] = r[q].del;
        }
        ++ci, ko += r[q].klen, vo += r[q].vlen;
    }
    if (tid == 0) {
        lk[cnt] = ktot, lv[cnt] = vtot;
        if (blockIdx.x == 0) key_off[sz.entries_out] = sz.key_bytes, val_off[sz.entries_out] = sz.val_bytes;
    }
    __syncthreads();
    if (kbase < sz.key_bytes) emit_stream(keys + kbase, ktot, sz.key_bytes - kbase, lk, spk, cnt, pool);
    if (vbase < sz.val_bytes) emit_stream(vals + vbase, vtot, sz.val_bytes - vbase, lv, spv, cnt, pool);
}

// ------------------------------------------------------------------ workspace + launches ----

static inline uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

// An error return after an asynchronous copy from or to host memory that dies with the caller's frame: wait
// for what was enqueued before giving the error back.
static hipError_t drained(hipStream_t s, hipError_t e) {
    (void)hipStreamSynchronize(s);
    return e;
}

static uint32_t merge_passes(uint32_t nruns) {
    uint32_t p = 0;
    while ((1ull << p) < nruns) ++p;
    return p;
}

MergeWs merge_ws_layout(uint64_t n, uint32_t nblocks, uint32_t nruns) {
    MergeWs w{};
    uint64_t at = 128;  // the header
    auto take = [&](uint64_t bytes) {
        const uint64_t o = at;
        at += up16(bytes);
        return o;
    };
    w.tiles = (n + MT - 1) / MT;
    w.passes = merge_passes(nruns);
    w.run_begin = take(8 * ((uint64_t)nruns + 1));
    w.run_first = take(8 * ((uint64_t)nruns + 1));
    w.block_first = take(4 * ((uint64_t)nblocks + 1));
    w.groups = take(8 * ((uint64_t)nblocks / 256 + 1));
    w.head_bytes = at;  // what the plan needs before it knows n
    w.sums = take(8 * 3 * w.tiles);
    w.rec_a = take(32 * n);
    w.rec_b = take(w.passes ? 32 * n : 0);
    w.tab_cap = (uint64_t)w.passes * (w.tiles + 1) + 2ull * nruns;
    w.tab = take(8 * w.tab_cap);
    w.cuts = take(w.passes ? 8 * (w.tiles + nruns + 1) : 0);  // two per tile of the largest pass
    w.bytes = at;
    return w;
}

hipError_t launch_merge_count(const uint8_t *pool, const uint16_t *blen, uint32_t nblocks, uint16_t *block_entries,
                              hipStream_t s) {
    hipLaunchKernelGGL(k_merge_count, dim3((nblocks + 255) / 256), dim3(256), 0, s, pool, blen, nblocks, block_entries);
    return hipGetLastError();
}

hipError_t launch_merge_head(const uint64_t *run_begin_host, uint32_t nruns, const uint16_t *block_entries,
                             uint32_t nblocks, void *ws, uint64_t *n_host, uint64_t *run_first_host, hipStream_t s) {
    const MergeWs w = merge_ws_layout(0, nblocks, nruns);
    uint8_t *p = (uint8_t *)ws;
    uint64_t *hdr = (uint64_t *)p, *rb = (uint64_t *)(p + w.run_begin), *rf = (uint64_t *)(p + w.run_first);
    uint32_t *first = (uint32_t *)(p + w.block_first);
    hipError_t e;
    if ((e = hipMemsetAsync(hdr, 0, 128, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(hdr + kHdrErr, 0xFF, 8, s)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(rb, run_begin_host, 8ull * (nruns + 1), hipMemcpyHostToDevice, s)) != hipSuccess) return drained(s, e);
    const unsigned groups = (nblocks + 255) / 256;
    uint64_t *gsum = (uint64_t *)(p + w.groups);
    hipLaunchKernelGGL(k_merge_groups, dim3(groups), dim3(256), 0, s, block_entries, nblocks, gsum);
    hipLaunchKernelGGL(k_merge_scan, dim3(1), dim3(1024), 0, s, gsum, (uint64_t)groups, hdr + kHdrTotal);
    hipLaunchKernelGGL(k_merge_spread, dim3(groups), dim3(256), 0, s, block_entries, nblocks, (const uint64_t *)gsum, first);
    hipLaunchKernelGGL(k_merge_runs, dim3(nruns / 256 + 1), dim3(256), 0, s, rb, nruns, first, rf);
    if ((e = hipGetLastError()) != hipSuccess) return drained(s, e);
    if ((e = hipMemcpyAsync(n_host, hdr + kHdrTotal, 8, hipMemcpyDeviceToHost, s)) != hipSuccess) return drained(s, e);
    if ((e = hipMemcpyAsync(run_first_host, rf, 8ull * (nruns + 1), hipMemcpyDeviceToHost, s)) != hipSuccess) return drained(s, e);
    return hipStreamSynchronize(s);
}

hipError_t launch_merge_decode(const uint8_t *pool, const uint16_t *blen, uint32_t nblocks, uint32_t nruns, uint64_t n,
                               void *ws, uint64_t *err_host, hipStream_t s) {
    const MergeWs w = merge_ws_layout(n, nblocks, nruns);
    uint8_t *p = (uint8_t *)ws;
    uint64_t *hdr = (uint64_t *)p;
    MergeRec *rec = (MergeRec *)(p + w.rec_a);
    hipLaunchKernelGGL(k_merge_decode, dim3((nblocks + 255) / 256), dim3(256), 0, s, pool, blen, nblocks,
                       (const uint32_t *)(p + w.block_first), n, rec);
    if (n > 1)
        hipLaunchKernelGGL(k_merge_check, dim3((unsigned)((n - 1 + 255) / 256)), dim3(256), 0, s, rec, n,
                           (const uint64_t *)(p + w.run_first), nruns, pool, hdr);
    hipError_t e;
    if ((e = hipGetLastError()) != hipSuccess) return drained(s, e);
    if ((e = hipMemcpyAsync(err_host, hdr + kHdrErr, 8, hipMemcpyDeviceToHost, s)) != hipSuccess) return drained(s, e);
    return hipStreamSynchronize(s);
}

hipError_t launch_merge_tree(const uint8_t *pool, uint32_t nblocks, uint32_t nruns, uint64_t n,
                             const uint64_t *run_first_host, uint32_t flags, void *ws, void *sizes_host, hipStream_t s) {
    const MergeWs w = merge_ws_layout(n, nblocks, nruns);
    uint8_t *p = (uint8_t *)ws;
    uint64_t *hdr = (uint64_t *)p, *sums = (uint64_t *)(p + w.sums);
    const uint64_t *rf = (const uint64_t *)(p + w.run_first);
    // each pass's tiles: (pair, tile of the pair), pairs without records left out
    std::vector<uint2> tab;
    std::vector<uint64_t> pass_at(w.passes + 1, 0);
    auto rfh = [&](uint64_t r) { return run_first_host[r < nruns ? r : nruns]; };
    for (uint32_t ps = 0; ps < w.passes; ++ps) {
        const uint64_t wd = 1ull << ps;
        for (uint64_t j = 0; 2 * j * wd < nruns; ++j) {
            const uint64_t len = rfh(2 * j * wd + 2 * wd) - rfh(2 * j * wd);
            for (uint64_t k = 0; k * MT < len; ++k) tab.push_back(make_uint2((uint32_t)j, (uint32_t)k));
        }
        pass_at[ps + 1] = tab.size();
    }
    hipError_t e;
    if (tab.size() > w.tab_cap) return hipErrorInvalidValue;
    if (!tab.empty() &&
        (e = hipMemcpyAsync(p + w.tab, tab.data(), 8 * tab.size(), hipMemcpyHostToDevice, s)) != hipSuccess)
        return drained(s, e);
    uint64_t src_at = w.rec_a, dst_at = w.rec_b;
    for (uint32_t ps = 0; ps < w.passes; ++ps) {
        const uint64_t cnt = pass_at[ps + 1] - pass_at[ps];
        if (cnt > w.tiles + nruns + 1) return drained(s, hipErrorInvalidValue);
        if (cnt) {
            const uint2 *tiles = (const uint2 *)(p + w.tab) + pass_at[ps];
            uint32_t *cuts = (uint32_t *)(p + w.cuts);
            hipLaunchKernelGGL(k_merge_cuts, dim3((unsigned)((2 * cnt + 255) / 256)), dim3(256), 0, s,
                               (const MergeRec *)(p + src_at), rf, nruns, 1u << ps, tiles, (uint32_t)cnt, pool, cuts);
            hipLaunchKernelGGL(k_merge_pass, dim3((unsigned)cnt), dim3(256), 0, s, (const MergeRec *)(p + src_at),
                               (MergeRec *)(p + dst_at), rf, nruns, 1u << ps, tiles, cuts, pool);
        }
        std::swap(src_at, dst_at);
    }
    const uint64_t where[3] = {src_at, w.sums, w.tiles};
    if ((e = hipMemcpyAsync(hdr + kHdrRec, where, 16, hipMemcpyHostToDevice, s)) != hipSuccess) return drained(s, e);
    if ((e = hipMemcpyAsync(hdr + kHdrTiles, where + 2, 8, hipMemcpyHostToDevice, s)) != hipSuccess) return drained(s, e);
    hipLaunchKernelGGL(k_merge_mark, dim3((unsigned)w.tiles), dim3(256), 0, s, (MergeRec *)(p + src_at), n, flags, pool,
                       sums, w.tiles, hdr);
    hipLaunchKernelGGL(k_merge_scan, dim3(1), dim3(1024), 0, s, sums, w.tiles, hdr + kHdrOut);
    hipLaunchKernelGGL(k_merge_scan, dim3(1), dim3(1024), 0, s, sums + w.tiles, w.tiles, hdr + kHdrKey);
    hipLaunchKernelGGL(k_merge_scan, dim3(1), dim3(1024), 0, s, sums + 2 * w.tiles, w.tiles, hdr + kHdrVal);
    if ((e = hipGetLastError()) != hipSuccess) return drained(s, e);
    uint64_t h[16];
    if ((e = hipMemcpyAsync(h, hdr, sizeof h, hipMemcpyDeviceToHost, s)) != hipSuccess) return drained(s, e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;  // tab and where are read before this returns
    const uint64_t out[6] = {n, h[kHdrOut], h[kHdrKey], h[kHdrVal], h[kHdrShadowed], h[kHdrDropped]};
    memcpy(sizes_host, out, sizeof out);
    return hipSuccess;
}

uint64_t merge_emit_min_bytes(uint64_t n) { return 128 + 8 * 3 * ((n + MT - 1) / MT) + 32 * n; }

// Whether the workspace header is the plan's that returned `sizes`, and its arrays lie inside ws_bytes: reads the
// header back, so it waits for what the stream holds.
hipError_t merge_ws_check(const void *sizes, const void *ws, uint64_t ws_bytes, bool *ok, hipStream_t s) {
    MergeSizesArg sz;
    memcpy(&sz, sizes, sizeof sz);
    uint64_t h[16];
    hipError_t e;
    if ((e = hipMemcpyAsync(h, ws, sizeof h, hipMemcpyDeviceToHost, s)) != hipSuccess) return drained(s, e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    const uint64_t n = sz.entries_in, tiles = (n + MT - 1) / MT;
    *ok = h[kHdrErr] == ~0ull && h[kHdrTotal] == n && h[kHdrTiles] == tiles && h[kHdrOut] == sz.entries_out &&
          h[kHdrKey] == sz.key_bytes && h[kHdrVal] == sz.val_bytes && h[kHdrShadowed] == sz.shadowed &&
          h[kHdrDropped] == sz.dropped && (h[kHdrRec] & 15) == 0 && (h[kHdrSums] & 15) == 0 && h[kHdrRec] >= 128 &&
          h[kHdrSums] >= 128 && h[kHdrRec] <= ws_bytes && 32 * n <= ws_bytes - h[kHdrRec] && h[kHdrSums] <= ws_bytes &&
          24 * tiles <= ws_bytes - h[kHdrSums];
    return hipSuccess;
}

hipError_t launch_merge_emit(const uint8_t *pool, const void *sizes, const void *ws, uint8_t *keys, uint64_t *key_off,
                             uint8_t *vals, uint64_t *val_off, uint8_t *deleted, hipStream_t s) {
    MergeSizesArg sz;
    memcpy(&sz, sizes, sizeof sz);
    const uint64_t tiles = (sz.entries_in + MT - 1) / MT;
    hipLaunchKernelGGL(k_merge_emit, dim3((unsigned)tiles), dim3(256), 0, s, pool, (const uint8_t *)ws, sz, keys, key_off,
                       vals, val_off, deleted);
    return hipGetLastError();
}

}  // namespace seb
