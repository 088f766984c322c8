// seb_replay.hip — WAL replay on the device: a log image into the memtable's sorted run, in the SSTable
// builder's input layout.
//
// What recoverFromWAL computes through MemTable.Put / Delete and what GetAllEntries then returns
// (lsm/lsm.go:273-298, lsm/memtable.go:34-93,129-137): a sort of the records by (key, record index) in which the
// last record of each key survives.  The index makes the order total, so no sort here needs to be stable and
// every output byte is determined.
//
//   k_replay_sort   a workgroup per tile of kMergeTile records: a lane per record checks its offsets and its
//                   framing (one atomicMin keeps the least bad record), builds a 32-byte sort record in LDS (the
//                   key's first 16 bytes as two big-endian words, the record index, the lengths, the deleted
//                   bit) and folds the sequence into the maximum; then a bitonic sort of a u16 permutation over
//                   the records, which stay put in LDS, and the tile goes out in order
//   k_replay_cuts, k_replay_pass   one level of a pairwise merge tree over the sorted tiles: runs of w records
//                   (the last one short) [2jw, 2jw + w) and [2jw + w, 2jw + 2w) into one.  The (pair, tile)
//                   couples are arithmetic: 2w is a multiple of the tile, so output tile t belongs to pair
//                   t * tile / 2w.  A workgroup makes one output tile: two merge-path diagonal searches
//                   (k_replay_cuts: a lane per search, all of a pass's tiles at once) bound its inputs, they go
//                   to LDS, and every record finds its rank by a bisection of the other side
//   k_replay_mark   after the last level equal keys are adjacent in index order: the survivor is the last of
//                   its group; per tile the survivors' count, key bytes and value bytes (0 for a tombstone)
//   k_replay_scan   exclusive scan of the tiles' three sums (one workgroup each); the totals are the sizes
//   k_replay_emit   per tile: the survivors' offsets by a scan in the workgroup, key_off / val_off / deleted /
//                   seq, then the tile's two output ranges (its keys, its values), each contiguous, filled 16
//                   aligned bytes at a time: a chunk inside one entry whose two aligned source words lie inside
//                   the image is two 16-byte loads and a shift, every other chunk goes byte by byte
// Records compare by their prefix words; only a tie on all 16 bytes reads key bytes from the image, at
// rec_off[index] + 21.  No load leaves [rec_off[0], rec_off[n]), and none touches a record that is not framed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <utility>

#include "seb_kernels.h"

namespace seb {

namespace {

constexpr uint32_t RT = kMergeTile;
constexpr uint32_t kWalHdr = 21;  // [crc u32][seq u64][keySize u32][valueSize u32][deleted u8]
constexpr uint64_t kReplayMagic = 0x59414C5045524C57ull;  // "WLREPLAY"

enum : uint32_t { kRecDeleted = 1, kRecKeep = 2, kRecBad = 4 };

struct __attribute__((aligned(16))) SortRec {
    uint64_t k0, k1;     // the key's first 16 bytes, zero padded, big-endian
    uint32_t idx;        // the record: its bytes are at data + rec_off[idx]
    uint32_t klen, vlen;
    uint32_t flags;      // kRecDeleted (byte == 1), kRecKeep (set by k_replay_mark), kRecBad (reads nothing)
};
static_assert(sizeof(SortRec) == 32, "SortRec layout");

// the workspace header (u64 words)
enum : uint32_t { rHdrErr = 0, rHdrTotal = 1, rHdrRec = 2, rHdrSums = 3, rHdrOut = 4, rHdrKey = 5, rHdrVal = 6,
                  rHdrTomb = 7, rHdrMaxSeq = 8, rHdrTiles = 9, rHdrMagic = 10 };

typedef const __attribute__((address_space(1))) uint8_t *gbytes;

__device__ __forceinline__ uint32_t gle32(gbytes p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ __forceinline__ uint64_t gle64(gbytes p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
__device__ __forceinline__ uint64_t be64g(gbytes p, uint32_t len) {  // first min(len, 8) bytes, big-endian
    uint64_t v = 0;
    for (uint32_t i = 0; i < 8; ++i) v = (v << 8) | (i < len ? p[i] : 0u);
    return v;
}

// Record i of the image as a sort record; lo = rec_off[0], hi = rec_off[n].  A record whose offsets decrease
// or leave [lo, hi], or that is not framed, reads nothing past its two offsets (and its header's sizes, once 21
// bytes are known to be there) and becomes an empty-key kRecBad record; *bad = i << 1 | (1: framing, 0: offsets).
__device__ __forceinline__ SortRec decode_record(const uint8_t *__restrict__ data, const uint64_t *__restrict__ rec_off,
                                                 uint64_t i, uint64_t lo, uint64_t hi, uint64_t *seq, uint64_t *bad) {
    SortRec r;
    r.k0 = r.k1 = 0;
    r.idx = (uint32_t)i;
    r.klen = r.vlen = 0;
    r.flags = kRecBad;
    *seq = 0;
    *bad = ~0ull;
    const uint64_t a = rec_off[i], b = rec_off[i + 1];
    if (a < lo || b < a || b > hi) {
        *bad = i << 1;
        return r;
    }
    const uint64_t len = b - a;
    gbytes g = (gbytes)data + a;
    uint32_t ks = 0, vs = 0;
    bool framed = len >= kWalHdr;
    if (framed) {
        ks = gle32(g + 12), vs = gle32(g + 16);
        framed = (uint64_t)kWalHdr + ks + vs == len;
    }
    if (!framed) {
        *bad = i << 1 | 1;
        return r;
    }
    *seq = gle64(g + 4);
    const uint64_t at = a + kWalHdr;
    gbytes kp = g + kWalHdr;
    if (at + 16 <= hi) {  // two 8-byte loads inside the image, the bytes past the key masked off
        const uint64_t va = __builtin_bswap64(gle64(kp)), vd = __builtin_bswap64(gle64(kp + 8));
        r.k0 = ks >= 8 ? va : ks == 0 ? 0ull : va & (~0ull << (8 * (8 - ks)));
        r.k1 = ks >= 16 ? vd : ks <= 8 ? 0ull : vd & (~0ull << (8 * (16 - ks)));
    } else {  // the image's last bytes: ks <= hi - at < 16
        r.k0 = be64g(kp, ks);
        r.k1 = ks > 8 ? be64g(kp + 8, ks - 8) : 0ull;
    }
    r.klen = ks;
    r.vlen = vs;
    r.flags = g[20] == 1 ? kRecDeleted : 0;
    return r;
}

// Go string order of two records' keys: the prefix words, then on a tie of all 16 bytes the key bytes past them
// in the image (both keys longer than 16, so both records are framed), then the lengths.
__device__ __forceinline__ int key_cmp(uint64_t ak0, uint64_t ak1, uint32_t aidx, uint32_t aklen, uint64_t bk0,
                                       uint64_t bk1, uint32_t bidx, uint32_t bklen, const uint8_t *__restrict__ data,
                                       const uint64_t *__restrict__ rec_off) {
    if (ak0 != bk0) return ak0 < bk0 ? -1 : 1;
    if (ak1 != bk1) return ak1 < bk1 ? -1 : 1;
    const uint32_t m = aklen < bklen ? aklen : bklen;
    if (m > 16) {
        gbytes pa = (gbytes)data + rec_off[aidx] + kWalHdr;
        gbytes pb = (gbytes)data + rec_off[bidx] + kWalHdr;
        uint32_t i = 16;
        for (; i + 8 <= m; i += 8) {  // 8 key bytes of each at a time: inside both keys
            const uint64_t x = gle64(pa + i), y = gle64(pb + i);
            if (x != y) return __builtin_bswap64(x) < __builtin_bswap64(y) ? -1 : 1;
        }
        for (; i < m; ++i)
            if (pa[i] != pb[i]) return pa[i] < pb[i] ? -1 : 1;
    }
    return aklen < bklen ? -1 : aklen > bklen ? 1 : 0;
}

// (key, record index): a total order, no two records compare equal
__device__ __forceinline__ int rec_cmp(uint64_t ak0, uint64_t ak1, uint32_t aidx, uint32_t aklen, uint64_t bk0,
                                       uint64_t bk1, uint32_t bidx, uint32_t bklen, const uint8_t *__restrict__ data,
                                       const uint64_t *__restrict__ rec_off) {
    const int c = key_cmp(ak0, ak1, aidx, aklen, bk0, bk1, bidx, bklen, data, rec_off);
    return c ? c : aidx < bidx ? -1 : aidx > bidx ? 1 : 0;
}

__device__ __forceinline__ SortRec rec_load(const SortRec *__restrict__ p) {
    union { uint4 q[2]; SortRec r; } u;
    u.q[0] = ((const uint4 *)p)[0];
    u.q[1] = ((const uint4 *)p)[1];
    return u.r;
}

__device__ __forceinline__ int rec_cmp(const SortRec &a, const SortRec &b, const uint8_t *__restrict__ data,
                                       const uint64_t *__restrict__ rec_off) {
    return rec_cmp(a.k0, a.k1, a.idx, a.klen, b.k0, b.k1, b.idx, b.klen, data, rec_off);
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// ------------------------------------------------------------------ decode + tile sort ------

__global__ __launch_bounds__(256) void k_replay_sort(const uint8_t *__restrict__ data, const uint64_t *__restrict__ rec_off,
                                                     uint64_t n, SortRec *__restrict__ rec, uint64_t *__restrict__ hdr) {
    __shared__ uint64_t sk0[RT], sk1[RT];
    __shared__ uint4 sm[RT];  // idx, klen, vlen, flags
    __shared__ uint16_t perm[RT];
    const uint32_t tid = threadIdx.x;
    const uint64_t ts = (uint64_t)blockIdx.x * RT;
    if (ts >= n) return;
    const uint32_t cnt = n - ts < RT ? (uint32_t)(n - ts) : RT;
    const uint64_t lo = rec_off[0], hi = rec_off[n];
    unsigned long long mseq = 0, bad = ~0ull;
    for (uint32_t x = tid; x < RT; x += 256) {
        perm[x] = (uint16_t)x;
        if (x >= cnt) continue;
        uint64_t seq, b;
        const SortRec r = decode_record(data, rec_off, ts + x, lo, hi, &seq, &b);
        sk0[x] = r.k0, sk1[x] = r.k1;
        sm[x] = make_uint4(r.idx, r.klen, r.vlen, r.flags);
        mseq = seq > mseq ? seq : mseq;
        bad = b < bad ? b : bad;
    }
    mseq = wave_max(mseq), bad = wave_min(bad);
    if ((tid & 63) == 0) {
        if (mseq) atomicMax((unsigned long long *)&hdr[rHdrMaxSeq], mseq);
        if (bad != ~0ull) atomicMin((unsigned long long *)&hdr[rHdrErr], bad);
    }
    __syncthreads();
    // bitonic sort of the permutation; the slots past cnt hold no record and sort last, by their number
    for (uint32_t k = 2; k <= RT; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < RT / 2; t += 256) {
                const uint32_t i = 2 * t - (t & (j - 1)), l = i + j;
                const uint32_t a = perm[i], b = perm[l];
                bool gt;
                if (a >= cnt || b >= cnt) {
                    gt = a > b;
                } else {
                    const uint4 ma = sm[a], mb = sm[b];
                    gt = rec_cmp(sk0[a], sk1[a], ma.x, ma.y, sk0[b], sk1[b], mb.x, mb.y, data, rec_off) > 0;
                }
                if (gt == ((i & k) == 0)) perm[i] = (uint16_t)b, perm[l] = (uint16_t)a;
            }
            __syncthreads();
        }
    }
    for (uint32_t x = tid; x < cnt; x += 256) {
        const uint32_t p = perm[x];  // < cnt: the cnt records sort before every empty slot
        const uint64_t k0 = sk0[p], k1 = sk1[p];
        uint4 *o = (uint4 *)(rec + ts + x);
        o[0] = make_uint4((uint32_t)k0, (uint32_t)(k0 >> 32), (uint32_t)k1, (uint32_t)(k1 >> 32));
        o[1] = sm[p];
    }
}

// ------------------------------------------------------------------ the merge tree ----------

// the number of A's records among the first d outputs of merge(A[0, na), B[0, nb))
__device__ __forceinline__ uint64_t merge_path(const SortRec *__restrict__ A, uint64_t na, const SortRec *__restrict__ B,
                                               uint64_t nb, uint64_t d, const uint8_t *__restrict__ data,
                                               const uint64_t *__restrict__ rec_off) {
    uint64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        const SortRec a = rec_load(A + mid), b = rec_load(B + (d - 1 - mid));
        if (rec_cmp(a, b, data, rec_off) < 0) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Output tile t of a pass over runs of w records (w a multiple of RT): its pair's two sides and the diagonals it
// lies between.  A = src[a0, a0 + na), B = src[a0 + na, a0 + na + nb), outputs [d0, d1) of the pair; t * RT < n.
struct ReplayTile {
    uint64_t a0, na, nb, d0, d1;
};
__device__ __forceinline__ ReplayTile replay_tile(uint64_t n, uint64_t w, uint64_t t) {
    ReplayTile m;
    const uint64_t g = t * RT;
    m.a0 = g / (2 * w) * (2 * w);
    m.na = n - m.a0 < w ? n - m.a0 : w;
    const uint64_t rest = n - m.a0 - m.na;
    m.nb = rest < w ? rest : w;
    m.d0 = g - m.a0;
    m.d1 = m.d0 + RT < m.na + m.nb ? m.d0 + RT : m.na + m.nb;
    return m;
}

// cuts[2t], cuts[2t + 1] = the left side's records before tile t's first and last diagonal
__global__ __launch_bounds__(256) void k_replay_cuts(const SortRec *__restrict__ src, uint64_t n, uint64_t w, uint64_t tiles,
                                                     const uint8_t *__restrict__ data, const uint64_t *__restrict__ rec_off,
                                                     uint32_t *__restrict__ cuts) {
    const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= 2 * tiles) return;
    const ReplayTile m = replay_tile(n, w, x >> 1);
    const uint64_t d = x & 1 ? m.d1 : m.d0;
    cuts[x] = (uint32_t)merge_path(src + m.a0, m.na, src + m.a0 + m.na, m.nb, d, data, rec_off);
}

__global__ __launch_bounds__(256) void k_replay_pass(const SortRec *__restrict__ src, SortRec *__restrict__ dst, uint64_t n,
                                                     uint64_t w, const uint32_t *__restrict__ cuts,
                                                     const uint8_t *__restrict__ data, const uint64_t *__restrict__ rec_off) {
    __shared__ uint64_t sk0[RT], sk1[RT];
    __shared__ uint4 sm[RT];  // idx, klen, vlen, flags
    const uint32_t tid = threadIdx.x;
    if ((uint64_t)blockIdx.x * RT >= n) return;
    const ReplayTile mt = replay_tile(n, w, blockIdx.x);
    const uint64_t a0 = mt.a0, d0 = mt.d0, d1 = mt.d1;
    const SortRec *A = src + a0, *B = src + a0 + mt.na;
    const uint64_t i0 = cuts[2 * blockIdx.x], i1 = cuts[2 * blockIdx.x + 1];
    if (i0 > d0 || i1 > d1 || i1 < i0 || i1 > mt.na || d1 - i1 > mt.nb || d1 - i1 < d0 - i0) return;  // not this tile's cuts
    const uint64_t j0 = d0 - i0;
    const uint32_t ta = (uint32_t)(i1 - i0), tb = (uint32_t)((d1 - i1) - j0);  // ta + tb = d1 - d0 <= RT
    if (ta > RT || tb > RT - ta) return;
    for (uint32_t x = tid; x < ta + tb; x += 256) {
        const SortRec *p = x < ta ? A + i0 + x : B + j0 + (x - ta);
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
        uint32_t lo = left ? ta : 0, hi = left ? ta + tb : ta;  // the other side's records below this one
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            const uint4 o = sm[mid];
            if (rec_cmp(sk0[mid], sk1[mid], o.x, o.y, k0, k1, m.x, m.y, data, rec_off) < 0) lo = mid + 1; else hi = mid;
        }
        const uint32_t rank = left ? x + (lo - ta) : (x - ta) + lo;
        uint4 *o = (uint4 *)(dst + a0 + d0 + rank);
        o[0] = make_uint4((uint32_t)k0, (uint32_t)(k0 >> 32), (uint32_t)k1, (uint32_t)(k1 >> 32));
        o[1] = m;
    }
}

// ------------------------------------------------------------------ survivors ---------------

// Also leaves where the plan's arrays are in the header (workgroup 0), which the emit reads.
__global__ __launch_bounds__(256) void k_replay_mark(SortRec *__restrict__ rec, uint64_t n, const uint8_t *__restrict__ data,
                                                     const uint64_t *__restrict__ rec_off, uint64_t *__restrict__ sums,
                                                     uint64_t tiles, uint64_t *__restrict__ hdr, uint64_t rec_at,
                                                     uint64_t sums_at) {
    __shared__ unsigned long long acc[4];
    const uint32_t tid = threadIdx.x;
    if (tid < 4) acc[tid] = 0;
    __syncthreads();
    const uint64_t ts = (uint64_t)blockIdx.x * RT;
    unsigned long long cnt = 0, kb = 0, vb = 0, tomb = 0;
    for (uint32_t q = 0; q < RT / 256; ++q) {
        const uint64_t e = ts + q * 256 + tid;
        if (e >= n) break;
        const SortRec r = rec_load(rec + e);
        bool keep = true;  // the last record of its key
        if (e + 1 < n) {
            const SortRec nx = rec_load(rec + e + 1);
            keep = key_cmp(r.k0, r.k1, r.idx, r.klen, nx.k0, nx.k1, nx.idx, nx.klen, data, rec_off) != 0;
        }
        rec[e].flags = (r.flags & ~kRecKeep) | (keep ? kRecKeep : 0u);
        if (keep) {
            const bool del = r.flags & kRecDeleted;
            ++cnt, kb += r.klen, vb += del ? 0u : r.vlen, tomb += del ? 1 : 0;
        }
    }
    cnt = wave_sum(cnt), kb = wave_sum(kb), vb = wave_sum(vb), tomb = wave_sum(tomb);
    if ((tid & 63) == 0) atomicAdd(&acc[0], cnt), atomicAdd(&acc[1], kb), atomicAdd(&acc[2], vb), atomicAdd(&acc[3], tomb);
    __syncthreads();
    if (tid == 0) {
        sums[blockIdx.x] = acc[0];
        sums[tiles + blockIdx.x] = acc[1];
        sums[2 * tiles + blockIdx.x] = acc[2];
        if (acc[3]) atomicAdd((unsigned long long *)&hdr[rHdrTomb], acc[3]);
        if (blockIdx.x == 0) hdr[rHdrTotal] = n, hdr[rHdrRec] = rec_at, hdr[rHdrSums] = sums_at, hdr[rHdrTiles] = tiles, hdr[rHdrMagic] = kReplayMagic;
    }
}

// x = the exclusive scan of x in place, *total = the sum; one workgroup
__global__ __launch_bounds__(1024) void k_replay_scan(uint64_t *x, uint64_t count, uint64_t *total) {
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
// (q[cnt] = total), its bytes are at data + sp[i].  room = the bytes the caller's array still holds from dst.
// [img_lo, img_hi) = the image's addresses: an aligned 16-byte source load is made only inside them.
__device__ __forceinline__ void emit_stream(uint8_t *__restrict__ dst, uint64_t total, uint64_t room, const uint64_t *q,
                                            const uint64_t *sp, uint32_t cnt, const uint8_t *__restrict__ data,
                                            uint64_t img_lo, uint64_t img_hi) {
    if (total == 0 || cnt == 0) return;
    if (room < total) total = room;
    const uint64_t a = (uint64_t)dst, a0 = a & ~15ull;
    const uint64_t lead = a - a0, chunks = (lead + total + 15) >> 4;
    for (uint64_t c = threadIdx.x; c < chunks; c += blockDim.x) {
        const bool head = (c << 4) < lead;  // the chunk starts before dst
        const uint64_t lo = head ? 0 : (c << 4) - lead;  // the chunk's bytes as range positions [lo, hi)
        const uint64_t end16 = (c << 4) + 16 - lead, hi = end16 < total ? end16 : total;
        uint32_t i = 0, ih = cnt - 1;  // the last survivor with q[i] <= lo: the one that holds byte lo
        while (i < ih) {
            const uint32_t mid = (i + ih + 1) >> 1;
            if (q[mid] <= lo) i = mid; else ih = mid - 1;
        }
        uint64_t end = q[i + 1];
        const bool full = !head && end16 <= total;
        const uint64_t s = (uint64_t)data + sp[i] + (lo - q[i]), s0 = s & ~15ull;
        uint32_t sh = (uint32_t)(s - s0);
        if (full && lo + 16 <= end && s0 >= img_lo && s0 + (sh ? 32 : 16) <= img_hi) {
            const uint4 u = *(const uint4 *)s0;
            uint64_t w0 = (uint64_t)u.x | (uint64_t)u.y << 32, w1 = (uint64_t)u.z | (uint64_t)u.w << 32;
            if (sh) {
                const uint4 v = *(const uint4 *)(s0 + 16);
                uint64_t w2 = (uint64_t)v.x | (uint64_t)v.y << 32, w3 = (uint64_t)v.z | (uint64_t)v.w << 32;
                if (sh >= 8) w0 = w1, w1 = w2, w2 = w3, sh -= 8;
                if (sh) {
                    const uint32_t bits = 8 * sh;
                    w0 = w0 >> bits | w1 << (64 - bits);
                    w1 = w1 >> bits | w2 << (64 - bits);
                }
            }
            *(uint4 *)(a0 + (c << 4)) = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
        } else {
            gbytes src = (gbytes)data + sp[i];
            uint64_t beg = q[i];
            for (uint64_t j = lo; j < hi; ++j) {
                while (j >= end) {  // j < total <= q[cnt]: ends with i < cnt
                    ++i;
                    beg = end;
                    end = q[i + 1];
                    src = (gbytes)data + sp[i];
                }
                dst[j] = src[j - beg];
            }
        }
    }
}

struct ReplaySizesArg {  // seb_replay_sizes
    uint64_t records_in, entries_out, key_bytes, val_bytes, overwritten, tombstones, max_sequence, memtable_size;
};

__global__ __launch_bounds__(256) void k_replay_emit(const uint8_t *__restrict__ data, const uint64_t *__restrict__ rec_off,
                                                     const uint8_t *__restrict__ ws, ReplaySizesArg sz,
                                                     uint8_t *__restrict__ keys, uint64_t *__restrict__ key_off,
                                                     uint8_t *__restrict__ vals, uint64_t *__restrict__ val_off,
                                                     uint8_t *__restrict__ deleted, uint64_t *__restrict__ seq) {
    __shared__ uint64_t lk[RT + 1], lv[RT + 1];
    __shared__ uint64_t spk[RT], spv[RT];
    __shared__ uint32_t sc[256];
    __shared__ uint64_t sk[256], sv[256];
    const uint32_t tid = threadIdx.x;
    const uint64_t *hdr = (const uint64_t *)ws;
    const uint64_t n = sz.records_in, tiles = (n + RT - 1) / RT;
    if (hdr[rHdrMagic] != kReplayMagic || hdr[rHdrTotal] != n || hdr[rHdrTiles] != tiles) return;  // not this plan's sizes
    const SortRec *rec = (const SortRec *)(ws + hdr[rHdrRec]);
    const uint64_t *sums = (const uint64_t *)(ws + hdr[rHdrSums]);
    const uint64_t ts = (uint64_t)blockIdx.x * RT;
    const uint64_t obase = sums[blockIdx.x], kbase = sums[tiles + blockIdx.x], vbase = sums[2 * tiles + blockIdx.x];
    // a thread takes 4 consecutive records
    SortRec r[4];
    uint32_t c = 0;
    uint64_t ks = 0, vs = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        const uint64_t e = ts + 4 * tid + q;
        r[q].flags = 0;
        if (e < n) r[q] = rec_load(rec + e);
        if (r[q].flags & kRecBad) r[q].flags = 0;  // never in a plan that succeeded
        if (r[q].flags & kRecDeleted) r[q].vlen = 0;  // Delete stores no value, whatever the record carried
        if (r[q].flags & kRecKeep) ++c, ks += r[q].klen, vs += r[q].vlen;
    }
    sc[tid] = c, sk[tid] = ks, sv[tid] = vs;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const uint32_t x = tid >= d ? sc[tid - d] : 0;
        const uint64_t y = tid >= d ? sk[tid - d] : 0, z = tid >= d ? sv[tid - d] : 0;
        __syncthreads();
        sc[tid] += x, sk[tid] += y, sv[tid] += z;
        __syncthreads();
    }
    const uint32_t cnt = sc[255];
    const uint64_t ktot = sk[255], vtot = sv[255];
    uint32_t ci = sc[tid] - c;
    uint64_t ko = sk[tid] - ks, vo = sv[tid] - vs;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        if (!(r[q].flags & kRecKeep)) continue;
        const uint64_t at = rec_off[r[q].idx];
        lk[ci] = ko, lv[ci] = vo;
        spk[ci] = at + kWalHdr;
        spv[ci] = at + kWalHdr + r[q].klen;
        const uint64_t o = obase + ci;
        if (o < sz.entries_out) {
            key_off[o] = kbase + ko;
            val_off[o] = vbase + vo;
            deleted[o] = r[q].flags & kRecDeleted ? 1 : 0;
            if (seq) seq[o] = gle64((gbytes)data + at + 4);
        }
        ++ci, ko += r[q].klen, vo += r[q].vlen;
    }
    if (tid == 0) {
        lk[cnt] = ktot, lv[cnt] = vtot;
        if (blockIdx.x == 0) key_off[sz.entries_out] = sz.key_bytes, val_off[sz.entries_out] = sz.val_bytes;
    }
    __syncthreads();
    const uint64_t img_lo = (uint64_t)data + rec_off[0], img_hi = (uint64_t)data + rec_off[n];
    if (kbase < sz.key_bytes) emit_stream(keys + kbase, ktot, sz.key_bytes - kbase, lk, spk, cnt, data, img_lo, img_hi);
    if (vbase < sz.val_bytes) emit_stream(vals + vbase, vtot, sz.val_bytes - vbase, lv, spv, cnt, data, img_lo, img_hi);
}

inline uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

// An error return after an asynchronous copy to host memory that dies with the caller's frame: wait for what
// was enqueued before giving the error back.
hipError_t drained(hipStream_t s, hipError_t e) {
    (void)hipStreamSynchronize(s);
    return e;
}

}  // namespace

// ------------------------------------------------------------------ workspace + launches ----

ReplayWs replay_ws_layout(uint64_t n) {
    ReplayWs w{};
    uint64_t at = 128;  // the header
    auto take = [&](uint64_t bytes) {
        const uint64_t o = at;
        at += up16(bytes);
        return o;
    };
    w.tiles = (n + RT - 1) / RT;
    w.passes = 0;
    while ((1ull << w.passes) < w.tiles) ++w.passes;
    w.sums = take(8 * 3 * w.tiles);
    w.rec_a = take(32 * n);
    w.rec_b = take(w.passes ? 32 * n : 0);
    w.cuts = take(w.passes ? 8 * w.tiles : 0);  // two per tile
    w.bytes = at;
    return w;
}

uint64_t replay_emit_min_bytes(uint64_t n) { return 128 + 8 * 3 * ((n + RT - 1) / RT) + 32 * n; }

hipError_t launch_replay_plan(const uint8_t *data, const uint64_t *rec_off, uint64_t n, void *ws, void *sizes_host,
                              uint64_t *err_host, hipStream_t s) {
    const ReplayWs w = replay_ws_layout(n);
    uint8_t *p = (uint8_t *)ws;
    uint64_t *hdr = (uint64_t *)p, *sums = (uint64_t *)(p + w.sums);
    const unsigned tiles = (unsigned)w.tiles;
    hipError_t e;
    if ((e = hipMemsetAsync(hdr, 0, 128, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(hdr + rHdrErr, 0xFF, 8, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_replay_sort, dim3(tiles), dim3(256), 0, s, data, rec_off, n, (SortRec *)(p + w.rec_a), hdr);
    uint64_t src_at = w.rec_a, dst_at = w.rec_b;
    for (uint32_t ps = 0; ps < w.passes; ++ps) {
        const uint64_t width = (uint64_t)RT << ps;
        uint32_t *cuts = (uint32_t *)(p + w.cuts);
        hipLaunchKernelGGL(k_replay_cuts, dim3((unsigned)((2 * w.tiles + 255) / 256)), dim3(256), 0, s,
                           (const SortRec *)(p + src_at), n, width, w.tiles, data, rec_off, cuts);
        hipLaunchKernelGGL(k_replay_pass, dim3(tiles), dim3(256), 0, s, (const SortRec *)(p + src_at),
                           (SortRec *)(p + dst_at), n, width, (const uint32_t *)cuts, data, rec_off);
        std::swap(src_at, dst_at);
    }
    hipLaunchKernelGGL(k_replay_mark, dim3(tiles), dim3(256), 0, s, (SortRec *)(p + src_at), n, data, rec_off, sums, w.tiles,
                       hdr, src_at, w.sums);
    hipLaunchKernelGGL(k_replay_scan, dim3(1), dim3(1024), 0, s, sums, w.tiles, hdr + rHdrOut);
    hipLaunchKernelGGL(k_replay_scan, dim3(1), dim3(1024), 0, s, sums + w.tiles, w.tiles, hdr + rHdrKey);
    hipLaunchKernelGGL(k_replay_scan, dim3(1), dim3(1024), 0, s, sums + 2 * w.tiles, w.tiles, hdr + rHdrVal);
    if ((e = hipGetLastError()) != hipSuccess) return drained(s, e);
    uint64_t h[16];
    if ((e = hipMemcpyAsync(h, hdr, sizeof h, hipMemcpyDeviceToHost, s)) != hipSuccess) return drained(s, e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    *err_host = h[rHdrErr];
    const uint64_t out[8] = {n, h[rHdrOut], h[rHdrKey], h[rHdrVal], n - h[rHdrOut], h[rHdrTomb], h[rHdrMaxSeq],
                             h[rHdrKey] + 16 * h[rHdrOut] + h[rHdrVal]};
    memcpy(sizes_host, out, sizeof out);
    return hipSuccess;
}

hipError_t replay_ws_check(const void *sizes, const void *ws, uint64_t ws_bytes, bool *ok, hipStream_t s) {
    ReplaySizesArg sz;
    memcpy(&sz, sizes, sizeof sz);
    uint64_t h[16];
    hipError_t e;
    if ((e = hipMemcpyAsync(h, ws, sizeof h, hipMemcpyDeviceToHost, s)) != hipSuccess) return drained(s, e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    const uint64_t n = sz.records_in, tiles = (n + RT - 1) / RT;
    *ok = h[rHdrMagic] == kReplayMagic && h[rHdrErr] == ~0ull && h[rHdrTotal] == n && h[rHdrTiles] == tiles &&
          h[rHdrOut] == sz.entries_out && h[rHdrKey] == sz.key_bytes && h[rHdrVal] == sz.val_bytes &&
          h[rHdrTomb] == sz.tombstones && h[rHdrMaxSeq] == sz.max_sequence && (h[rHdrRec] & 15) == 0 &&
          (h[rHdrSums] & 15) == 0 && h[rHdrRec] >= 128 && h[rHdrSums] >= 128 && h[rHdrRec] <= ws_bytes &&
          32 * n <= ws_bytes - h[rHdrRec] && h[rHdrSums] <= ws_bytes && 24 * tiles <= ws_bytes - h[rHdrSums];
    return hipSuccess;
}

hipError_t launch_replay_emit(const uint8_t *data, const uint64_t *rec_off, const void *sizes, const void *ws, uint8_t *keys,
                              uint64_t *key_off, uint8_t *vals, uint64_t *val_off, uint8_t *deleted, uint64_t *seq,
                              hipStream_t s) {
    ReplaySizesArg sz;
    memcpy(&sz, sizes, sizeof sz);
    const uint64_t tiles = (sz.records_in + RT - 1) / RT;
    hipLaunchKernelGGL(k_replay_emit, dim3((unsigned)tiles), dim3(256), 0, s, data, rec_off, (const uint8_t *)ws, sz, keys,
                       key_off, vals, val_off, deleted, seq);
    return hipGetLastError();
}

}  // namespace seb
