// seb_sst.hip — batched SSTable builder on the device: the block cut, the data-block images, the
// index blocks and the metadata of many files in one call.
//
// What SSTableBuilder computes between its Write calls (lsm/sstable_builder.go:42-135,185-290):
//   Add:   entry = [keySize u32][valueSize u32][deleted u8][key][value], e = 9 + keySize + valueSize
//          if len(cur) + e > 4096 && len(cur) > 4 { flush }; cur = append(cur, entry...)
//   flush: cur[0:4] = numEntries; write cur, zero padded to 4096; index += (first key, offset)
// With P(i) = 9 i + keyOffset(i) + valueOffset(i), the 64-bit prefix sum of e up to a constant (the
// inputs' offset arrays already are prefix sums, so P costs two loads), the block that starts at entry
// s ends before next(s) = the smallest t > s with P(t+1) - P(s) > 4092, clamped to the file's end.  A
// block holds at most 454 entries (4 + 9 * 455 > 4096), so next(s) <= s + 454.
//
// The cut is the set reachable from each file's first entry under next(), a sequential recurrence.
// next() is monotone, so chains merge, and the plan finds the set tile by tile (kSstTile entries):
//   k_sst_next   per tile: next() of every entry by bisection over P in LDS, then every entry's exit
//                from the tile (the first chain element at or past the tile's end) by pointer doubling
//   k_sst_walk   a lane per file hops from tile to tile through the exits (n / kSstTile steps per file,
//                files in parallel) and leaves each tile its entry point.  Because next() is clamped to
//                the file's end, a chain runs through every later file's first entry: one chain covers
//                the batch, and each tile has exactly one entry point, whoever writes it
//   k_sst_tile   per tile: one lane follows next() from the entry point inside the tile (LDS), which
//                lists the tile's block starts; their index-entry sizes are scanned
//   k_sst_scan   exclusive scan of the tiles' block counts and index bytes (one workgroup)
//   k_sst_gather block b's first entry, compacted over the batch; k_sst_files / k_sst_sizes: per file,
//                its first block, its index bytes, its sizes
// The encode then has a wave per block: the entry table in LDS, the 9-byte headers, and the two
// contiguous input ranges (the block's keys, the block's values) read as aligned 16-byte chunks, each
// chunk's bytes placed in the 4 KiB LDS image at 13 + 9 i + (the other stream's offset) + its own
// stream position; the image goes out in 16-byte stores, zero padding included.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "seb_kernels.h"

namespace seb {

constexpr uint32_t T = kSstTile;
constexpr uint32_t kMaxPerBlock = 454;          // entries a block can hold: 4 + 9 * 454 = 4090
constexpr uint32_t kWin = T + kMaxPerBlock + 2;  // P values a tile's bisections read
constexpr uint64_t kBody = kBlockBytes - 4;      // 4092: entry bytes a block holds besides its header

__device__ __forceinline__ uint64_t koff(const KeyBatch &kb, uint64_t i) {
    return kb.offsets ? kb.offsets[i] : i * (uint64_t)kb.stride;
}

// the file of entry i: the last f with fbeg[f] <= i (so fbeg[f+1] > i: never an empty file), f in [lo, hi]
__device__ __forceinline__ uint32_t file_of(const uint64_t *__restrict__ fbeg, uint32_t lo, uint32_t hi, uint64_t i) {
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (fbeg[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ------------------------------------------------------------------ the plan ----------------

__global__ __launch_bounds__(1024) void k_sst_next(KeyBatch kb, const uint64_t *__restrict__ voff, uint64_t n,
                                                   const uint64_t *__restrict__ fbeg, uint32_t nf,
                                                   uint16_t *__restrict__ nxt, uint16_t *__restrict__ ex,
                                                   unsigned long long *__restrict__ ovs_cnt,
                                                   unsigned long long *__restrict__ ovs_exc) {
    __shared__ uint64_t P[kWin];
    __shared__ uint16_t J[T];
    __shared__ uint32_t frange[2];
    const uint32_t tid = threadIdx.x;
    const uint64_t ts = (uint64_t)blockIdx.x * T;
    for (uint32_t j = tid; j < kWin; j += 1024) {
        const uint64_t g = ts + j;
        if (g <= n) P[j] = 9 * g + koff(kb, g) + voff[g];
    }
    if (tid == 0) {
        const uint64_t last = (ts + T < n ? ts + T : n) - 1;
        frange[0] = file_of(fbeg, 0, nf - 1, ts);
        frange[1] = file_of(fbeg, frange[0], nf - 1, last);
    }
    __syncthreads();
    const uint64_t i = ts + tid;
    uint32_t nx = T;  // past the batch: leaves the tile at once
    if (i < n) {
        const uint32_t f = file_of(fbeg, frange[0], frange[1], i);
        const uint64_t fe = fbeg[f + 1];
        uint64_t lo = i + 1, hi = i + kMaxPerBlock + 1 < fe ? i + kMaxPerBlock + 1 : fe;
        const uint64_t base = P[tid] + kBody;
        while (lo < hi) {  // the smallest t with t >= fe or P(t+1) - P(i) > 4092; it holds at hi
            const uint64_t mid = (lo + hi) >> 1;
            if (P[mid + 1 - ts] > base) hi = mid; else lo = mid + 1;
        }
        nx = (uint32_t)(lo - ts);
        const uint64_t e = P[tid + 1] - P[tid];
        if (e > kBody) {  // an oversized entry: a block of its own, e + 4 bytes long
            atomicAdd(&ovs_cnt[f], 1ull);
            atomicAdd(&ovs_exc[f], (unsigned long long)(e + 4 - kBlockBytes));
        }
    }
    nxt[ts + tid] = (uint16_t)nx;
    J[tid] = (uint16_t)nx;
    __syncthreads();
    // J = next^(2^r), stopped at the first element outside the tile: 10 rounds cover a chain of T
    for (uint32_t r = 0; r < 10; ++r) {
        const uint32_t v = J[tid];
        const uint32_t w = v < T ? J[v] : v;
        __syncthreads();
        J[tid] = (uint16_t)w;
        __syncthreads();
    }
    ex[ts + tid] = J[tid];
}

// entry[u] = the first element of the batch's chain at or past u * T.  Its predecessor lies in tile
// u - 1, in some file f, and f's lane reaches it: every write of entry[u] stores the same value.
__global__ __launch_bounds__(64) void k_sst_walk(const uint64_t *__restrict__ fbeg, uint32_t nf, uint64_t n,
                                                 const uint16_t *__restrict__ ex, uint32_t *__restrict__ entry) {
    const uint32_t f = blockIdx.x * 64 + threadIdx.x;
    if (f >= nf) return;
    uint64_t e = fbeg[f];
    const uint64_t fe = fbeg[f + 1];
    if (e < fe && e % T == 0) entry[e / T] = (uint32_t)e;
    while (e < fe) {
        const uint64_t e2 = e / T * T + ex[e];  // > e: an exit is at or past the tile's end
        if (e2 <= fe && e2 < n) entry[e2 / T] = (uint32_t)e2;
        e = e2;
    }
}

__global__ __launch_bounds__(1024) void k_sst_tile(KeyBatch kb, uint64_t n, const uint16_t *__restrict__ nxt,
                                                   const uint32_t *__restrict__ entry, uint16_t *__restrict__ starts,
                                                   uint64_t *__restrict__ tix, uint64_t *__restrict__ tile_cnt,
                                                   uint64_t *__restrict__ tile_ix) {
    __shared__ uint16_t N[T], S[T];
    __shared__ uint64_t X[T];
    __shared__ uint32_t cnt_s;
    const uint32_t tid = threadIdx.x;
    const uint64_t ts = (uint64_t)blockIdx.x * T;
    N[tid] = nxt[ts + tid];
    __syncthreads();
    if (tid == 0) {
        uint32_t pos = (uint32_t)(entry[blockIdx.x] - ts), c = 0;  // unsigned: a bad entry point ends the loop
        while (pos < T && ts + pos < n && c < T) {
            S[c++] = (uint16_t)pos;
            const uint32_t nx = N[pos];
            pos = nx > pos ? nx : T;
        }
        cnt_s = c;
    }
    __syncthreads();
    const uint32_t cnt = cnt_s;
    uint64_t v = 0;
    if (tid < cnt) {
        const uint64_t s = ts + S[tid];
        v = 12 + (koff(kb, s + 1) - koff(kb, s));  // the block's index entry
    }
    X[tid] = v;
    __syncthreads();
    for (uint32_t d = 1; d < T; d <<= 1) {
        const uint64_t a = tid >= d ? X[tid - d] : 0;
        __syncthreads();
        X[tid] += a;
        __syncthreads();
    }
    if (tid < cnt) {
        starts[ts + tid] = S[tid];
        tix[ts + tid] = X[tid] - v;
    }
    if (tid == T - 1) {
        tile_cnt[blockIdx.x] = cnt;
        tile_ix[blockIdx.x] = X[tid];
    }
}

// out = the exclusive scan of in (may be the same array), *total = the sum; one workgroup
__global__ __launch_bounds__(1024) void k_sst_scan(const uint64_t *in, uint64_t *out, uint64_t count, uint64_t *total) {
    __shared__ uint64_t X[1024];
    __shared__ uint64_t carry_s;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (uint64_t base = 0; base < count; base += 1024) {
        const uint64_t v = base + tid < count ? in[base + tid] : 0;
        X[tid] = v;
        __syncthreads();
        for (uint32_t d = 1; d < 1024; d <<= 1) {
            const uint64_t a = tid >= d ? X[tid - d] : 0;
            __syncthreads();
            X[tid] += a;
            __syncthreads();
        }
        const uint64_t carry = carry_s;
        if (base + tid < count) out[base + tid] = carry + X[tid] - v;
        __syncthreads();
        if (tid == 1023) carry_s = carry + X[tid];
        __syncthreads();
    }
    if (tid == 0) *total = carry_s;
}

__global__ __launch_bounds__(1024) void k_sst_gather(uint64_t n, const uint16_t *__restrict__ starts,
                                                     const uint64_t *__restrict__ tile_cnt,
                                                     const uint64_t *__restrict__ tile_base,
                                                     const uint64_t *__restrict__ hdr, uint32_t *__restrict__ blk_first) {
    const uint64_t ts = (uint64_t)blockIdx.x * T;
    if (threadIdx.x < tile_cnt[blockIdx.x]) blk_first[tile_base[blockIdx.x] + threadIdx.x] = (uint32_t)(ts + starts[ts + threadIdx.x]);
    if (blockIdx.x == 0 && threadIdx.x == 0) blk_first[hdr[0]] = (uint32_t)n;  // block B "starts" at n
}

// fbk[f], fix[f] = the block id and the index bytes before it of the block that starts at fbeg[f]
// (f = 0 .. nf; an empty file's are its successor's; fbeg == n: the totals)
__global__ __launch_bounds__(256) void k_sst_files(const uint64_t *__restrict__ fbeg, uint32_t nf, uint64_t n,
                                                   const uint16_t *__restrict__ starts, const uint64_t *__restrict__ tix,
                                                   const uint64_t *__restrict__ tile_cnt,
                                                   const uint64_t *__restrict__ tile_base,
                                                   const uint64_t *__restrict__ tile_ixbase,
                                                   const uint64_t *__restrict__ hdr, uint64_t *__restrict__ fbk,
                                                   uint64_t *__restrict__ fix) {
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f > nf) return;
    const uint64_t e = fbeg[f];
    if (e >= n) {
        fbk[f] = hdr[0];
        fix[f] = hdr[1];
        return;
    }
    const uint64_t u = e / T, ts = u * T;
    const uint32_t rel = (uint32_t)(e - ts);
    uint32_t lo = 0, hi = (uint32_t)tile_cnt[u];  // the first j with starts[j] >= rel: it is rel, a block start
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (starts[ts + mid] < rel) lo = mid + 1; else hi = mid;
    }
    fbk[f] = tile_base[u] + lo;
    fix[f] = tile_ixbase[u] + (lo < tile_cnt[u] ? tix[ts + lo] : 0);
}

struct DevSizes {  // seb_sst_sizes
    uint64_t num_blocks, data_bytes, index_bytes, meta_bytes, oversize_entries;
};

__global__ __launch_bounds__(256) void k_sst_sizes(KeyBatch kb, const uint64_t *__restrict__ fbeg, uint32_t nf,
                                                   const uint64_t *__restrict__ fbk, const uint64_t *__restrict__ fix,
                                                   const unsigned long long *__restrict__ ovs_cnt,
                                                   const unsigned long long *__restrict__ ovs_exc,
                                                   DevSizes *__restrict__ sizes, uint64_t *__restrict__ meta_len) {
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    const uint64_t b = fbeg[f], e = fbeg[f + 1];
    DevSizes s;
    s.num_blocks = fbk[f + 1] - fbk[f];
    s.data_bytes = s.num_blocks * kBlockBytes + ovs_exc[f];
    s.index_bytes = 4 + (fix[f + 1] - fix[f]);
    s.meta_bytes = 8 + (b < e ? (koff(kb, b + 1) - koff(kb, b)) + (koff(kb, e) - koff(kb, e - 1)) : 0);
    s.oversize_entries = ovs_cnt[f];
    sizes[f] = s;
    meta_len[f] = s.meta_bytes;
}

// ------------------------------------------------------------------ the encode --------------

__device__ __forceinline__ void lds_put32(uint8_t *img, uint32_t at, uint32_t v) {
    img[at] = (uint8_t)v, img[at + 1] = (uint8_t)(v >> 8), img[at + 2] = (uint8_t)(v >> 16), img[at + 3] = (uint8_t)(v >> 24);
}

// One of a block's two input streams into the image: src[0, total) is the concatenation of the
// block's keys (KEYS) or values; q[i] = entry i's offset in it (q[cnt] = total), o = the other
// stream's table.  Byte j of entry i lands at 13 + 9 i + j + (KEYS ? o[i] : o[i + 1]).  Reads are
// 16-byte loads at 16-byte aligned addresses that lie wholly inside the stream, bytes at its two ends.
template <bool KEYS>
__device__ __forceinline__ void copy_stream(const uint8_t *__restrict__ src, uint32_t total, const uint16_t *q,
                                            const uint16_t *o, uint32_t cnt, uint8_t *img) {
    if (total == 0) return;
    const uint64_t a = (uint64_t)src, a0 = a & ~15ull;
    const uint32_t lead = (uint32_t)(a - a0), chunks = (lead + total + 15) >> 4;
    for (uint32_t c = threadIdx.x; c < chunks; c += blockDim.x) {
        const int32_t j0 = (int32_t)(c << 4) - (int32_t)lead;  // the chunk's first byte as a stream position
        const uint32_t lo = j0 < 0 ? 0u : (uint32_t)j0, hi = (uint32_t)(j0 + 16) < total ? (uint32_t)(j0 + 16) : total;
        uint32_t i = 0, ih = cnt - 1;  // the last entry with q[i] <= lo: the one that holds byte lo
        while (i < ih) {
            const uint32_t mid = (i + ih + 1) >> 1;
            if (q[mid] <= lo) i = mid; else ih = mid - 1;
        }
        uint32_t end = q[i + 1];
        uint32_t add = 13 + 9 * i + (KEYS ? o[i] : o[i + 1]);
        if (j0 >= 0 && (uint32_t)j0 + 16 <= total) {
            const uint4 w = *(const uint4 *)(a0 + ((uint64_t)c << 4));
            const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (uint32_t k = 0; k < 16; ++k) {
                const uint32_t j = lo + k;
                while (j >= end) {  // j < total = q[cnt]: ends with i < cnt
                    ++i;
                    end = q[i + 1];
                    add = 13 + 9 * i + (KEYS ? o[i] : o[i + 1]);
                }
                const uint32_t dst = add + j;
                if (dst < kBlockBytes) img[dst] = (uint8_t)(ww[k >> 2] >> (8 * (k & 3)));
            }
        } else {
            for (uint32_t j = lo; j < hi; ++j) {
                while (j >= end) {
                    ++i;
                    end = q[i + 1];
                    add = 13 + 9 * i + (KEYS ? o[i] : o[i + 1]);
                }
                const uint32_t dst = add + j;
                if (dst < kBlockBytes) img[dst] = src[j];
            }
        }
    }
}

// One wave per block: a block's chain (its two boundaries, its offsets, its bytes, the store) is four
// dependent round trips to memory, and what hides them is blocks in flight per CU, 27 of them by LDS at
// 64 threads against 8 at 256 (measured: 0.77 ms against 1.22 ms for the compaction shape, DESIGN.md 5.11;
// tools/diag/sst_data_threads256.patch).
constexpr uint32_t kDataThreads = 64;
__global__ __launch_bounds__(kDataThreads) void k_sst_data(KeyBatch kb, const uint8_t *__restrict__ vals,
                                                  const uint64_t *__restrict__ voff, const uint8_t *__restrict__ del,
                                                  const uint32_t *__restrict__ blk_first, const uint64_t *__restrict__ hdr,
                                                  uint64_t nblocks, uint8_t *__restrict__ data,
                                                  uint16_t *__restrict__ blen) {
    __shared__ __attribute__((aligned(16))) uint8_t img[kBlockBytes];
    __shared__ uint16_t kq[kMaxPerBlock + 2], vq[kMaxPerBlock + 2];
    const uint32_t tid = threadIdx.x;
    const uint64_t B = nblocks < hdr[0] ? nblocks : hdr[0];
    for (uint64_t b = blockIdx.x; b < B; b += gridDim.x) {
        const uint64_t s = blk_first[b], t = blk_first[b + 1];
        if (s >= t || t > kb.n) continue;  // not a plan's (the same for the whole workgroup)
        uint32_t cnt = (uint32_t)(t - s);
        if (cnt > kMaxPerBlock) cnt = kMaxPerBlock;  // never for a plan without oversized entries
        const uint64_t k0 = koff(kb, s), v0 = voff[s];
        for (uint32_t i = tid; i <= cnt; i += kDataThreads) {
            const uint64_t kr = koff(kb, s + i) - k0, vr = voff[s + i] - v0;
            kq[i] = (uint16_t)(kr < kBlockBytes ? kr : kBlockBytes);
            vq[i] = (uint16_t)(vr < kBlockBytes ? vr : kBlockBytes);
        }
        __syncthreads();
        uint32_t len = 4 + 9 * cnt + kq[cnt] + vq[cnt];
        if (len > kBlockBytes) len = kBlockBytes;
        if (tid == 0) lds_put32(img, 0, cnt);
        for (uint32_t i = tid; i < cnt; i += kDataThreads) {
            const uint32_t at = 4 + 9 * i + kq[i] + vq[i];
            if (at + 9 <= kBlockBytes) {
                lds_put32(img, at, (uint32_t)kq[i + 1] - kq[i]);
                lds_put32(img, at + 4, (uint32_t)vq[i + 1] - vq[i]);
                img[at + 8] = del && del[s + i] ? 1 : 0;
            }
        }
        copy_stream<true>(kb.data + k0, kq[cnt], kq, vq, cnt, img);
        copy_stream<false>(vals + v0, vq[cnt], vq, kq, cnt, img);
        for (uint32_t j = len + tid; j < kBlockBytes; j += kDataThreads) img[j] = 0;
        __syncthreads();
        for (uint32_t q = tid; q < kBlockBytes / 16; q += kDataThreads) ((uint4 *)(data + b * kBlockBytes))[q] = ((const uint4 *)img)[q];
        if (tid == 0 && blen) blen[b] = (uint16_t)len;
        __syncthreads();  // the image and the tables are reused
    }
}

__device__ __forceinline__ void g_put32(uint8_t *p, uint32_t v) {
    p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24);
}

// index entries: block b of file f, [keySize u32][blockOffset u64][key] at 4 (f + 1) + (the index
// bytes of the blocks before it in the batch)
__global__ __launch_bounds__(1024) void k_sst_index(KeyBatch kb, const uint64_t *__restrict__ fbeg, uint32_t nf,
                                                    const uint16_t *__restrict__ starts, const uint64_t *__restrict__ tix,
                                                    const uint64_t *__restrict__ tile_cnt,
                                                    const uint64_t *__restrict__ tile_base,
                                                    const uint64_t *__restrict__ tile_ixbase,
                                                    const uint64_t *__restrict__ fbk, uint8_t *__restrict__ index,
                                                    uint64_t index_total) {
    const uint64_t ts = (uint64_t)blockIdx.x * T;
    if (threadIdx.x >= tile_cnt[blockIdx.x]) return;
    const uint64_t first = ts + starts[ts + threadIdx.x];
    const uint64_t b = tile_base[blockIdx.x] + threadIdx.x;
    const uint32_t f = file_of(fbeg, 0, nf - 1, first);
    const uint64_t k0 = koff(kb, first), klen = koff(kb, first + 1) - k0;
    const uint64_t at = 4ull * (f + 1) + tile_ixbase[blockIdx.x] + tix[ts + threadIdx.x];
    if (at + 12 + klen > index_total || at + 12 + klen < at) return;  // a plan and sizes that disagree
    uint8_t *p = index + at;
    const uint64_t off = (b - fbk[f]) * kBlockBytes;
    g_put32(p, (uint32_t)klen);
    g_put32(p + 4, (uint32_t)off);
    g_put32(p + 8, (uint32_t)(off >> 32));
    for (uint64_t j = 0; j < klen; ++j) p[12 + j] = kb.data[k0 + j];
}

// per file: the index block's numEntries, and the metadata [minKeySize u32][maxKeySize u32][minKey][maxKey]
__global__ __launch_bounds__(64) void k_sst_filemeta(KeyBatch kb, const uint64_t *__restrict__ fbeg, uint32_t nf,
                                                     const uint64_t *__restrict__ fbk, const uint64_t *__restrict__ fix,
                                                     const uint64_t *__restrict__ meta_base, uint8_t *__restrict__ index,
                                                     uint64_t index_total, uint8_t *__restrict__ meta,
                                                     uint64_t meta_total) {
    const uint32_t f = blockIdx.x * 64 + threadIdx.x;
    if (f >= nf) return;
    const uint64_t iat = 4ull * f + fix[f];
    if (iat + 4 <= index_total) g_put32(index + iat, (uint32_t)(fbk[f + 1] - fbk[f]));
    const uint64_t b = fbeg[f], e = fbeg[f + 1];
    uint64_t kmin0 = 0, kmin = 0, kmax0 = 0, kmax = 0;
    if (b < e) {
        kmin0 = koff(kb, b), kmin = koff(kb, b + 1) - kmin0;
        kmax0 = koff(kb, e - 1), kmax = koff(kb, e) - kmax0;
    }
    const uint64_t mat = meta_base[f];
    if (mat + 8 + kmin + kmax > meta_total || mat + 8 + kmin + kmax < mat) return;
    uint8_t *p = meta + mat;
    g_put32(p, (uint32_t)kmin);
    g_put32(p + 4, (uint32_t)kmax);
    for (uint64_t j = 0; j < kmin; ++j) p[8 + j] = kb.data[kmin0 + j];
    for (uint64_t j = 0; j < kmax; ++j) p[8 + kmin + j] = kb.data[kmax0 + j];
}

// ------------------------------------------------------------------ workspace + launches ----

static inline uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

SstWs sst_ws_layout(uint64_t n, uint32_t nf) {
    SstWs w{};
    const uint64_t tiles = (n + T - 1) / T, pad = tiles * T, F = nf;
    uint64_t at = 64;  // the header: total blocks, total index-entry bytes, total metadata bytes
    auto take = [&](uint64_t bytes) {
        const uint64_t o = at;
        at += up16(bytes);
        return o;
    };
    w.tiles = tiles;
    w.fbeg = take(8 * (F + 1));
    w.ovs_cnt = take(8 * F);
    w.ovs_exc = take(8 * F);
    w.fbk = take(8 * (F + 1));
    w.fix = take(8 * (F + 1));
    w.sizes = take(40 * F);
    w.meta_len = take(8 * F);
    w.entry = take(4 * tiles);
    w.tile_cnt = take(8 * tiles);
    w.tile_base = take(8 * tiles);
    w.tile_ix = take(8 * tiles);
    w.tile_ixbase = take(8 * tiles);
    w.nxt = take(2 * pad);
    w.ex = take(2 * pad);
    w.tix = take(8 * pad);
    w.blk_first = take(4 * (n + 1));
    w.bytes = at;
    return w;
}

hipError_t launch_sst_plan(const KeyBatch &kb, const uint64_t *voff, const uint64_t *file_begin_host, uint32_t nf,
                           void *ws, void *sizes_host, hipStream_t s) {
    const uint64_t n = kb.n;
    const SstWs w = sst_ws_layout(n, nf);
    uint8_t *p = (uint8_t *)ws;
    uint64_t *hdr = (uint64_t *)p, *fbeg = (uint64_t *)(p + w.fbeg);
    hipError_t e;
    if ((e = hipMemcpyAsync(fbeg, file_begin_host, 8ull * (nf + 1), hipMemcpyHostToDevice, s)) != hipSuccess) return e;
    // the header and the per-file oversize counters start at zero (contiguous up to fbk)
    if ((e = hipMemsetAsync(hdr, 0, 64, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(p + w.ovs_cnt, 0, w.fbk - w.ovs_cnt, s)) != hipSuccess) return e;
    const unsigned tiles = (unsigned)w.tiles;
    uint16_t *nxt = (uint16_t *)(p + w.nxt), *ex = (uint16_t *)(p + w.ex);
    uint64_t *tile_cnt = (uint64_t *)(p + w.tile_cnt), *tile_base = (uint64_t *)(p + w.tile_base),
             *tile_ix = (uint64_t *)(p + w.tile_ix), *tile_ixbase = (uint64_t *)(p + w.tile_ixbase),
             *tix = (uint64_t *)(p + w.tix), *fbk = (uint64_t *)(p + w.fbk), *fix = (uint64_t *)(p + w.fix),
             *meta_len = (uint64_t *)(p + w.meta_len);
    uint32_t *entry = (uint32_t *)(p + w.entry), *blk_first = (uint32_t *)(p + w.blk_first);
    unsigned long long *ovs_cnt = (unsigned long long *)(p + w.ovs_cnt), *ovs_exc = (unsigned long long *)(p + w.ovs_exc);
    hipLaunchKernelGGL(k_sst_next, dim3(tiles), dim3(1024), 0, s, kb, voff, n, fbeg, nf, nxt, ex, ovs_cnt, ovs_exc);
    hipLaunchKernelGGL(k_sst_walk, dim3((nf + 63) / 64), dim3(64), 0, s, fbeg, nf, n, ex, entry);
    hipLaunchKernelGGL(k_sst_tile, dim3(tiles), dim3(1024), 0, s, kb, n, nxt, entry, ex, tix, tile_cnt, tile_ix);
    hipLaunchKernelGGL(k_sst_scan, dim3(1), dim3(1024), 0, s, tile_cnt, tile_base, (uint64_t)tiles, hdr);
    hipLaunchKernelGGL(k_sst_scan, dim3(1), dim3(1024), 0, s, tile_ix, tile_ixbase, (uint64_t)tiles, hdr + 1);
    hipLaunchKernelGGL(k_sst_gather, dim3(tiles), dim3(1024), 0, s, n, ex, tile_cnt, tile_base, hdr, blk_first);
    hipLaunchKernelGGL(k_sst_files, dim3(nf / 256 + 1), dim3(256), 0, s, fbeg, nf, n, ex, tix, tile_cnt, tile_base,
                       tile_ixbase, hdr, fbk, fix);
    hipLaunchKernelGGL(k_sst_sizes, dim3((nf + 255) / 256), dim3(256), 0, s, kb, fbeg, nf, fbk, fix, ovs_cnt, ovs_exc,
                       (DevSizes *)(p + w.sizes), meta_len);
    // the metadata's place per file: the scan runs in place
    hipLaunchKernelGGL(k_sst_scan, dim3(1), dim3(1024), 0, s, meta_len, meta_len, (uint64_t)nf, hdr + 2);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(sizes_host, p + w.sizes, 40ull * nf, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    return hipStreamSynchronize(s);
}

hipError_t launch_sst_encode(const KeyBatch &kb, const uint8_t *vals, const uint64_t *voff, const uint8_t *deleted,
                             uint32_t nf, const void *ws, uint64_t nblocks, uint64_t index_total, uint64_t meta_total,
                             uint8_t *data, uint16_t *blen, uint8_t *index, uint8_t *meta, hipStream_t s) {
    const SstWs w = sst_ws_layout(kb.n, nf);
    const uint8_t *p = (const uint8_t *)ws;
    const uint64_t *hdr = (const uint64_t *)p, *fbeg = (const uint64_t *)(p + w.fbeg);
    const uint64_t *fbk = (const uint64_t *)(p + w.fbk), *fix = (const uint64_t *)(p + w.fix);
    if (nblocks) {
        uint64_t g = nblocks;
        if (g > options().grid_cap) g = options().grid_cap;
        hipLaunchKernelGGL(k_sst_data, dim3((unsigned)g), dim3(kDataThreads), 0, s, kb, vals, voff, deleted,
                           (const uint32_t *)(p + w.blk_first), hdr, nblocks, data, blen);
        hipLaunchKernelGGL(k_sst_index, dim3((unsigned)w.tiles), dim3(1024), 0, s, kb, fbeg, nf,
                           (const uint16_t *)(p + w.ex), (const uint64_t *)(p + w.tix),
                           (const uint64_t *)(p + w.tile_cnt), (const uint64_t *)(p + w.tile_base),
                           (const uint64_t *)(p + w.tile_ixbase), fbk, index, index_total);
    }
    hipLaunchKernelGGL(k_sst_filemeta, dim3((nf + 63) / 64), dim3(64), 0, s, kb, fbeg, nf, fbk, fix,
                       (const uint64_t *)(p + w.meta_len), index, index_total, meta, meta_total);
    return hipGetLastError();
}

}  // namespace seb
