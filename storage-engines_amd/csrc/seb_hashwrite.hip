// seb_hashwrite.hip — the hash index's write side on the device: a Put / Delete batch framed as
// segment.append's records with the rotation's cuts, compactSegments for the records of a prefix of the segments, and
// getLogicalSize over the key table.  The semantics and the host half are in seb_hashwrite.cpp.
//
//   k_sf_len      a workgroup per tile of kWriteTile ops, four consecutive ops per lane (k_frame_len's shape): an
//                 op's offsets are checked before anything else (one atomicMin keeps the least bad op and its
//                 reason), its record length is 20 + keyLen + (deleted ? 0 : valueLen), a scan in the workgroup
//                 leaves rec_off relative to the tile
//   k_sf_scan     the exclusive scan of the tiles' sums (scan_tile_sums, seb_scan.h), one workgroup per array
//   k_sf_add      rec_off[i] += its tile's base; rec_off[n] = the image's size
//   k_sf_cuts     one lane: the rotation's cuts as a chain of bisections over rec_off, one per new segment (a counted
//                 loop of at most n links; a batch makes size / limit of them)
//   k_sf_emit     a lane per 16 aligned bytes of the image (k_frame_emit's shape with the 20-byte header); the CRC
//                 field is left 0 for the seal, k_seg_crc's seal mode (seb_hashindex.hip)
//   k_sc_mark     after the scratch table is built by k_hidx_insert from these records alone: a workgroup per tile of
//                 kWriteTile records, four per lane.  A live record is checked against the pool (the least bad one
//                 fails the plan), looks its key up with plain loads (no insert runs in this launch), and survives
//                 iff the table names it and its value is not empty; a scan in the workgroup leaves its output
//                 offset and its survivor rank relative to the tile
//   k_sc_place    a lane per record: a survivor's output offset goes to out_rec_off[rank], its source offset to the
//                 workspace
//   k_sc_copy     a lane per 16 aligned bytes of the new image, whatever record they belong to (k_values' balance:
//                 one long value is spread over as many lanes as it has chunks): a bisection of out_rec_off finds the
//                 record, the source record is checked against the pool again, bytes 4..12 are the new timestamp
//   k_off_shift   seb_hidx_compact: the offsets of the segments that stay, moved behind the new image
//   k_hidx_logical a lane per slot: keySize + valueSize of the record the slot names, one atomic per wave
//
// Every offset that comes out of memory is checked before it is used: a record is re-checked against pool_bytes before
// a byte of it is read, and nothing is written outside the image and the offsets the plan sized.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "seb_hidx_dev.h"
#include "seb_kernels.h"
#include "seb_scan.h"

namespace seb {

namespace {

typedef const __attribute__((address_space(1))) uint8_t *gbytes;

constexpr uint32_t WT = kWriteTile;
constexpr uint32_t SW = kScanWidth;
constexpr uint64_t kCompactMagic = 0x5443504D43474553ull;  // "SEGCMPCT"
constexpr uint64_t kCutsEager = 1024;  // cuts copied back before their count is known

// the frame's scratch (u64 words): the least bad op << 2 | reason, the image's size, the cuts' count, then the tiles' sums
enum : uint32_t { sErr = 0, sBytes = 1, sCuts = 2, sSums = 4 };
// the compaction workspace's header (u64 words)
enum : uint32_t { cErr = 0, cLive = 1, cWin = 2, cTomb = 3, cBytes = 4, cSurv = 5, cN = 6, cMagic = 7 };

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}

// The 16 bytes at address s, when the aligned 16-byte words that cover them lie inside [lo, hi): two loads
// and a shift.  false: nothing was read.
__device__ __forceinline__ bool load16(uint64_t s, uint64_t lo, uint64_t hi, uint64_t &w0, uint64_t &w1) {
    const uint64_t s0 = s & ~15ull;
    uint32_t sh = (uint32_t)(s - s0);
    if (s0 < lo || s0 + (sh ? 32 : 16) > hi) return false;
    const uint4 u = *(const uint4 *)s0;
    w0 = (uint64_t)u.x | (uint64_t)u.y << 32, w1 = (uint64_t)u.z | (uint64_t)u.w << 32;
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
    return true;
}
__device__ __forceinline__ void store16(uint64_t at, uint64_t w0, uint64_t w1) {
    *(uint4 *)at = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
}

__global__ __launch_bounds__(SW) void k_sf_scan(uint64_t *x, uint64_t count, uint64_t *total) {
    scan_tile_sums(x + (uint64_t)blockIdx.x * count, count, total + blockIdx.x);
}

// ------------------------------------------------------------------ frame -------------------

// a pair of offsets as a length; one that decreases or spans 2^32 bytes or more reads as 0
__device__ __forceinline__ bool span32(uint64_t a, uint64_t b, uint32_t *len) {
    const bool ok = a <= b && b - a < (1ull << 32);
    *len = ok ? (uint32_t)(b - a) : 0u;
    return ok;
}

// reasons, in the order the host half tests them: 0 key offsets, 1 value offsets, 2 empty key, 3 keySize + valueSize
__global__ __launch_bounds__(256) void k_sf_len(KeyBatch kb, const uint64_t *__restrict__ val_off,
                                                const uint8_t *__restrict__ deleted, uint64_t *__restrict__ rec_off,
                                                uint64_t *__restrict__ scratch) {
    __shared__ uint64_t S[256];
    const uint32_t tid = threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * WT + 4 * tid;
    uint64_t len[4], sum = 0;
    unsigned long long bad = ~0ull;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        const uint64_t i = first + q;
        len[q] = 0;
        if (i >= kb.n) continue;
        uint32_t kl = kb.stride, vl;
        const bool kok = kb.offsets ? span32(kb.offsets[i], kb.offsets[i + 1], &kl) : true;
        const bool vok = span32(val_off[i], val_off[i + 1], &vl);
        const bool del = deleted && ((gbytes)deleted)[i] != 0;
        if (del) vl = 0;
        const uint32_t why = !kok ? 0u : !vok ? 1u : kl == 0 ? 2u : (uint64_t)kl + vl >= (1ull << 32) ? 3u : 4u;
        if (why != 4u) {
            const unsigned long long b = i << 2 | why;
            bad = b < bad ? b : bad;
            continue;
        }
        len[q] = (uint64_t)kSegHeader + kl + vl;
        sum += len[q];
    }
    bad = wave_min(bad);
    if ((tid & 63) == 0 && bad != ~0ull) atomicMin((unsigned long long *)scratch + sErr, bad);
    S[tid] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const uint64_t a = tid >= d ? S[tid - d] : 0;
        __syncthreads();
        S[tid] += a;
        __syncthreads();
    }
    uint64_t at = S[tid] - sum;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        if (first + q < kb.n) rec_off[first + q] = at;
        at += len[q];
    }
    if (tid == 255) scratch[sSums + blockIdx.x] = S[255];
}

__global__ __launch_bounds__(256) void k_sf_add(uint64_t *__restrict__ rec_off, uint64_t n,
                                                const uint64_t *__restrict__ scratch) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n)
        rec_off[i] += scratch[sSums + i / WT];
    else if (i == n)
        rec_off[n] = scratch[sBytes];
}

// size = active; for op j: if size >= limit: a cut at j, size = 0; size += len_j.  With rec_off the cut behind one
// at op c (c's segment starts at rec_off[c]) is the least j > c with rec_off[j] - rec_off[c] >= limit.
__global__ void k_sf_cuts(const uint64_t *__restrict__ rec_off, uint64_t n, uint64_t active, uint64_t limit,
                          uint64_t *__restrict__ cuts, uint64_t cap, uint64_t *__restrict__ scratch) {
    if (threadIdx.x || blockIdx.x) return;
    uint64_t count = 0;
    if (scratch[sErr] == ~0ull) {  // else the offsets mean nothing
        const uint64_t total = scratch[sBytes];
        uint64_t base = 0, held = active, from = 0;
        for (uint64_t link = 0; link < n; ++link) {
            const uint64_t need = limit > held ? limit - held : 0;
            if (need > total - base) break;
            const uint64_t target = base + need;
            uint64_t lo = from, hi = n;  // the least j in [from, n] with rec_off[j] >= target (rec_off[n] = total does)
            while (lo < hi) {
                const uint64_t mid = lo + ((hi - lo) >> 1);
                if (rec_off[mid] >= target) hi = mid; else lo = mid + 1;
            }
            if (lo >= n) break;  // no op is left to open the new segment
            if (count < cap) cuts[count] = lo;
            ++count;
            base = rec_off[lo], held = 0, from = lo + 1;
        }
    }
    scratch[sCuts] = count;
}

struct SegOp {  // what an op contributes to its record
    uint64_t key, val;  // addresses of its key and value bytes
    uint32_t klen, vlen;  // vlen 0 for a Delete
};
__device__ __forceinline__ SegOp seg_op(const KeyBatch &kb, const uint8_t *vals, const uint64_t *val_off,
                                        const uint8_t *deleted, uint64_t i) {
    SegOp o;
    uint64_t ko = i * (uint64_t)kb.stride;
    o.klen = kb.stride;
    if (kb.offsets) {
        ko = kb.offsets[i];
        span32(ko, kb.offsets[i + 1], &o.klen);
    }
    const uint64_t vo = val_off[i];
    span32(vo, val_off[i + 1], &o.vlen);
    if (deleted && ((gbytes)deleted)[i] != 0) o.vlen = 0;
    o.key = (uint64_t)kb.data + ko;
    o.val = (uint64_t)vals + vo;
    return o;
}
// byte p of the op's record, the CRC field as 0
__device__ __forceinline__ uint32_t seg_byte(const SegOp &o, uint64_t ts, uint64_t p) {
    if (p < 4) return 0;
    if (p < 12) return (uint32_t)(ts >> (8 * (p - 4))) & 0xFFu;
    if (p < 16) return (o.klen >> (8 * (p - 12))) & 0xFFu;
    if (p < 20) return (o.vlen >> (8 * (p - 16))) & 0xFFu;
    p -= kSegHeader;
    if (p < o.klen) return ((gbytes)o.key)[p];
    p -= o.klen;
    if (p < o.vlen) return ((gbytes)o.val)[p];
    return 0;  // behind the record: a rec_off that is not this batch's
}

__global__ __launch_bounds__(256) void k_sf_emit(KeyBatch kb, const uint8_t *__restrict__ vals,
                                                 const uint64_t *__restrict__ val_off, const uint8_t *__restrict__ deleted,
                                                 uint64_t ts, const uint64_t *__restrict__ rec_off,
                                                 uint8_t *__restrict__ image, uint64_t image_bytes) {
    const uint64_t n = kb.n;
    const uint64_t a = (uint64_t)image, a0 = a & ~15ull, lead = a - a0;
    const uint64_t chunks = (lead + image_bytes + 15) >> 4;
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= chunks) return;
    // the arrays' ends, inside which an aligned 16-byte load may be made
    const uint64_t klo = (uint64_t)kb.data + (kb.offsets ? kb.offsets[0] : 0);
    const uint64_t khi = (uint64_t)kb.data + (kb.offsets ? kb.offsets[n] : n * (uint64_t)kb.stride);
    const uint64_t vlo = (uint64_t)vals + val_off[0], vhi = (uint64_t)vals + val_off[n];
    const bool head = (c << 4) < lead;
    const uint64_t lo = head ? 0 : (c << 4) - lead;
    const uint64_t end16 = (c << 4) + 16 - lead, hi = end16 < image_bytes ? end16 : image_bytes;
    uint64_t i = 0, ih = n - 1;  // the last record with rec_off[i] <= lo
    while (i < ih) {
        const uint64_t mid = i + ((ih - i + 1) >> 1);
        if (rec_off[mid] <= lo) i = mid; else ih = mid - 1;
    }
    SegOp o = seg_op(kb, vals, val_off, deleted, i);
    uint64_t beg = rec_off[i], end = rec_off[i + 1];
    const uint64_t p0 = lo - beg;  // wraps where rec_off[0] > lo: no fast path, and seg_byte gives 0
    if (!head && end16 <= image_bytes && lo >= beg && lo + 16 <= end) {
        uint64_t w0, w1;
        bool done = false;
        if (p0 >= kSegHeader && p0 + 16 <= (uint64_t)kSegHeader + o.klen)
            done = load16(o.key + (p0 - kSegHeader), klo, khi, w0, w1);
        else if (p0 >= (uint64_t)kSegHeader + o.klen && p0 + 16 <= (uint64_t)kSegHeader + o.klen + o.vlen)
            done = load16(o.val + (p0 - kSegHeader - o.klen), vlo, vhi, w0, w1);
        if (done) {
            store16(a0 + (c << 4), w0, w1);
            return;
        }
    }
    for (uint64_t j = lo; j < hi; ++j) {
        while (j >= end && i + 1 < n) {
            ++i;
            o = seg_op(kb, vals, val_off, deleted, i);
            beg = end;
            end = rec_off[i + 1];
        }
        image[j] = (uint8_t)seg_byte(o, ts, j - beg);
    }
}

// ------------------------------------------------------------------ compaction --------------

// the offset the table holds for the key of the record at `off` (ks its key's length), ~0 where it holds none
__device__ __forceinline__ uint64_t table_names(const uint64_t *__restrict__ slots, uint64_t table, const uint8_t *pool,
                                                uint64_t pool_bytes, uint64_t off, uint32_t ks, uint64_t hmask) {
    const uint8_t *key = pool + off + kSegHeader;
    const uint64_t h = hash_key(key, ks, hmask), tag = h >> 48, mask = table - 1;
    uint64_t k0, k1;
    prefix_words(key, ks, k0, k1);
    uint64_t j = h & mask;
    for (uint64_t step = 0; step < table; ++step, j = (j + 1) & mask) {
        const uint64_t cur = slots[j];
        if (cur == 0) break;
        if (cur >> 48 != tag) continue;
        const uint64_t o = (cur & kLow48) - 1;
        uint32_t oks, ovs;
        if (o == off || same_key(pool, pool_bytes, o, key, ks, k0, k1, &oks, &ovs)) return o;
    }
    return ~0ull;
}

__global__ __launch_bounds__(256) void k_sc_mark(const uint8_t *__restrict__ pool, uint64_t pool_bytes,
                                                 const uint64_t *__restrict__ rec_off, const uint8_t *__restrict__ live,
                                                 uint64_t n, const uint64_t *__restrict__ slots, uint64_t table,
                                                 uint64_t hmask, u64a *__restrict__ hdr, uint64_t *__restrict__ sums,
                                                 uint64_t tiles, uint64_t *__restrict__ pos, uint32_t *__restrict__ mark) {
    __shared__ uint64_t S[256];
    __shared__ uint32_t C[256];
    const uint32_t tid = threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * WT + 4 * tid;
    uint64_t len[4], sum = 0;
    uint32_t cnt = 0;
    u64a bad = ~0ull, nlive = 0, nwin = 0, ntomb = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        const uint64_t r = first + q;
        len[q] = 0;
        if (r >= n || (live && ((gbytes)live)[r] == 0)) continue;
        ++nlive;
        const uint64_t off = rec_off[r];
        uint32_t ks, vs;
        if (!rec_extent(pool, pool_bytes, off, &ks, &vs)) {
            bad = r < bad ? r : bad;
            continue;
        }
        if (table_names(slots, table, pool, pool_bytes, off, ks, hmask) != off) continue;
        ++nwin;
        if (vs == 0) {
            ++ntomb;
            continue;
        }
        len[q] = (uint64_t)kSegHeader + ks + vs;
        sum += len[q], ++cnt;
    }
    bad = wave_min(bad), nlive = wave_sum(nlive), nwin = wave_sum(nwin), ntomb = wave_sum(ntomb);
    if ((tid & 63) == 0) {
        if (bad != ~0ull) __hip_atomic_fetch_min(hdr + cErr, bad, HIDX_RLX_AGENT);
        if (nlive) __hip_atomic_fetch_add(hdr + cLive, nlive, HIDX_RLX_AGENT);
        if (nwin) __hip_atomic_fetch_add(hdr + cWin, nwin, HIDX_RLX_AGENT);
        if (ntomb) __hip_atomic_fetch_add(hdr + cTomb, ntomb, HIDX_RLX_AGENT);
    }
    S[tid] = sum, C[tid] = cnt;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const uint64_t a = tid >= d ? S[tid - d] : 0;
        const uint32_t b = tid >= d ? C[tid - d] : 0;
        __syncthreads();
        S[tid] += a, C[tid] += b;
        __syncthreads();
    }
    uint64_t at = S[tid] - sum;
    uint32_t rank = C[tid] - cnt;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        if (first + q < n) {
            pos[first + q] = at;
            mark[first + q] = len[q] ? 0x80000000u | rank : 0u;
        }
        if (len[q]) at += len[q], ++rank;
    }
    if (tid == 255) sums[blockIdx.x] = S[255], sums[tiles + blockIdx.x] = C[255];
}

struct CompactArg {  // what the emit's kernels check the workspace's header against
    uint64_t n, survivors, image_bytes;
};
__device__ __forceinline__ bool plan_holds(const uint64_t *hdr, const CompactArg &a) {
    return hdr[cMagic] == kCompactMagic && hdr[cErr] == ~0ull && hdr[cN] == a.n && hdr[cSurv] == a.survivors &&
           hdr[cBytes] == a.image_bytes;
}

__global__ __launch_bounds__(256) void k_sc_place(const uint64_t *__restrict__ hdr, CompactArg a,
                                                  const uint64_t *__restrict__ rec_off, const uint64_t *__restrict__ sums,
                                                  uint64_t tiles, const uint64_t *__restrict__ pos,
                                                  const uint32_t *__restrict__ mark, uint64_t *__restrict__ src,
                                                  uint64_t *__restrict__ out_rec_off) {
    if (!plan_holds(hdr, a)) return;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < a.n; r += stride) {
        if (r == 0) out_rec_off[a.survivors] = a.image_bytes;
        const uint32_t m = mark[r];
        if (!(m & 0x80000000u)) continue;
        const uint64_t t = r / WT, k = sums[tiles + t] + (m & 0x7FFFFFFFu);
        if (k >= a.survivors) continue;  // never in a plan that holds
        out_rec_off[k] = sums[t] + pos[r];
        src[k] = rec_off[r];
    }
}

__global__ __launch_bounds__(256) void k_sc_copy(const uint64_t *__restrict__ hdr, CompactArg a,
                                                 const uint8_t *__restrict__ pool, uint64_t pool_bytes,
                                                 const uint64_t *__restrict__ src, const uint64_t *__restrict__ out_rec_off,
                                                 uint64_t ts, uint8_t *__restrict__ image) {
    if (!plan_holds(hdr, a)) return;
    const uint64_t image_bytes = a.image_bytes, S = a.survivors;
    const uint64_t ia = (uint64_t)image, a0 = ia & ~15ull, lead = ia - a0;
    const uint64_t chunks = (lead + image_bytes + 15) >> 4;
    const uint64_t plo = (uint64_t)pool, phi = plo + pool_bytes;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x; c < chunks; c += stride) {
        const bool head = (c << 4) < lead;
        const uint64_t lo = head ? 0 : (c << 4) - lead;
        const uint64_t end16 = (c << 4) + 16 - lead, hi = end16 < image_bytes ? end16 : image_bytes;
        uint64_t k = 0, kh = S - 1;  // the last survivor with out_rec_off[k] <= lo
        while (k < kh) {
            const uint64_t mid = k + ((kh - k + 1) >> 1);
            if (out_rec_off[mid] <= lo) k = mid; else kh = mid - 1;
        }
        uint64_t beg = out_rec_off[k], end = out_rec_off[k + 1], so = src[k];
        uint32_t ks, vs;
        // the source record as the pool holds it now: inside the pool, and of the length the plan gave it
        bool fits = rec_extent(pool, pool_bytes, so, &ks, &vs) && beg <= end && (uint64_t)kSegHeader + ks + vs == end - beg;
        const uint64_t p0 = lo - beg;
        if (!head && end16 <= image_bytes && fits && lo >= beg && lo + 16 <= end && p0 >= 12) {
            uint64_t w0, w1;
            if (load16(plo + so + p0, plo, phi, w0, w1)) {
                store16(a0 + (c << 4), w0, w1);
                continue;
            }
        }
        for (uint64_t j = lo; j < hi; ++j) {
            while (j >= end && k + 1 < S) {
                ++k;
                beg = end, end = out_rec_off[k + 1], so = src[k];
                fits = rec_extent(pool, pool_bytes, so, &ks, &vs) && beg <= end && (uint64_t)kSegHeader + ks + vs == end - beg;
            }
            const uint64_t p = j - beg;
            uint32_t b = 0;
            if (p >= 4 && p < 12)
                b = (uint32_t)(ts >> (8 * (p - 4))) & 0xFFu;
            else if (p >= 12 && fits && j < end)
                b = ((gbytes)pool)[so + p];
            image[j] = (uint8_t)b;
        }
    }
}

// ------------------------------------------------------------------ logical size ------------

__global__ __launch_bounds__(256) void k_hidx_logical(const uint64_t *__restrict__ slots, uint64_t table,
                                                      const uint8_t *__restrict__ pool, uint64_t pool_bytes, u64a *sum) {
    u64a acc = 0;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < table; j += stride) {
        const uint64_t cur = slots[j];
        if (cur == 0) continue;
        uint32_t ks, vs;
        if (rec_extent(pool, pool_bytes, (cur & kLow48) - 1, &ks, &vs)) acc += (u64a)ks + vs;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0 && acc) __hip_atomic_fetch_add(sum, acc, HIDX_RLX_AGENT);
}

// dst[i] = src[i] - sub + add; an offset below `sub` becomes all ones, which no pool holds
__global__ __launch_bounds__(256) void k_off_shift(const uint64_t *__restrict__ src, uint64_t n, uint64_t sub, uint64_t add,
                                                   uint64_t *__restrict__ dst, uint64_t end) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i <= n; i += stride)
        dst[i] = i == n ? end : src[i] >= sub ? src[i] - sub + add : ~0ull;
}

inline uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

hipError_t drained(hipStream_t s, hipError_t e) {
    (void)hipStreamSynchronize(s);
    return e;
}

}  // namespace

// ------------------------------------------------------------------ launches ----------------

uint64_t segframe_cut_slots(uint64_t n, uint64_t cut_cap) { return cut_cap < n ? cut_cap : n; }

uint64_t segframe_scratch_bytes(uint64_t n, uint64_t cut_cap) {
    return up16(8 * (sSums + (n + WT - 1) / WT)) + up16(8 * segframe_cut_slots(n, cut_cap));
}

hipError_t launch_segframe_plan(const KeyBatch &kb, const uint64_t *val_off, const uint8_t *deleted, uint64_t active_size,
                                uint64_t limit, uint64_t *rec_off, uint64_t *cut_host, uint64_t cut_cap, void *scratch,
                                uint64_t out_host[3], hipStream_t s) {
    uint64_t *sc = (uint64_t *)scratch;
    const uint64_t n = kb.n, tiles = (n + WT - 1) / WT, slots = segframe_cut_slots(n, cut_cap);
    uint64_t *cuts = (uint64_t *)((uint8_t *)scratch + up16(8 * (sSums + tiles)));
    hipError_t e;
    if ((e = hipMemsetAsync(sc, 0xFF, 8, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_sf_len, dim3((unsigned)tiles), dim3(256), 0, s, kb, val_off, deleted, rec_off, sc);
    hipLaunchKernelGGL(k_sf_scan, dim3(1), dim3(SW), 0, s, sc + sSums, tiles, sc + sBytes);
    hipLaunchKernelGGL(k_sf_add, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, s, rec_off, n, (const uint64_t *)sc);
    hipLaunchKernelGGL(k_sf_cuts, dim3(1), dim3(64), 0, s, (const uint64_t *)rec_off, n, active_size, limit, cuts, slots, sc);
    if ((e = hipGetLastError()) != hipSuccess) return drained(s, e);
    // the header and the first kCutsEager cuts come back in the one synchronisation; a batch that makes more of them
    // (a limit of a few records) pays a second copy
    const uint64_t eager = !cut_host ? 0 : slots < kCutsEager ? slots : kCutsEager;
    uint64_t h[3];
    if ((e = hipMemcpyAsync(h, sc, sizeof h, hipMemcpyDeviceToHost, s)) != hipSuccess) return drained(s, e);
    if (eager && (e = hipMemcpyAsync(cut_host, cuts, 8 * eager, hipMemcpyDeviceToHost, s)) != hipSuccess) return drained(s, e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    memcpy(out_host, h, sizeof h);
    const uint64_t have = h[sErr] != ~0ull || !cut_host ? 0 : h[sCuts] < slots ? h[sCuts] : slots;
    if (have > eager) {
        if ((e = hipMemcpyAsync(cut_host + eager, cuts + eager, 8 * (have - eager), hipMemcpyDeviceToHost, s)) != hipSuccess)
            return drained(s, e);
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_segframe_emit(const KeyBatch &kb, const uint8_t *vals, const uint64_t *val_off, const uint8_t *deleted,
                                uint64_t timestamp, const uint64_t *rec_off, uint8_t *image, uint64_t image_bytes,
                                hipStream_t s) {
    const uint64_t chunks = (((uint64_t)image & 15) + image_bytes + 15) >> 4, g = (chunks + 255) / 256;
    if (g >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sf_emit, dim3((unsigned)g), dim3(256), 0, s, kb, vals, val_off, deleted, timestamp, rec_off, image,
                       image_bytes);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_seg_seal(image, image_bytes, rec_off, kb.n, s);
}

SegCompactWs segcompact_ws_layout(uint64_t n) {
    SegCompactWs w{};
    w.tiles = (n + WT - 1) / WT;
    w.table = 64;  // behind the header
    w.sums = w.table + up16(hidx_table_bytes(n));
    w.pos = w.sums + up16(8 * 2 * w.tiles);
    w.src = w.pos + up16(8 * n);
    w.mark = w.src + up16(8 * n);
    w.bytes = w.mark + up16(4 * n);
    return w;
}

hipError_t launch_segcompact_plan(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, const uint8_t *live,
                                  uint64_t n, uint64_t hash_mask, void *ws, uint64_t out_host[8], hipStream_t s) {
    const SegCompactWs w = segcompact_ws_layout(n);
    uint8_t *p = (uint8_t *)ws;
    uint64_t *hdr = (uint64_t *)p, *sums = (uint64_t *)(p + w.sums);
    hipError_t e;
    if ((e = hipMemsetAsync(p, 0, w.sums, s)) != hipSuccess) return e;  // the header and the table
    if ((e = hipMemsetAsync(hdr + cErr, 0xFF, 8, s)) != hipSuccess) return e;
    if ((e = launch_hidx_insert(p + w.table, n, pool, pool_bytes, rec_off, live, n, hash_mask, s)) != hipSuccess) return drained(s, e);
    hipLaunchKernelGGL(k_sc_mark, dim3((unsigned)w.tiles), dim3(256), 0, s, pool, pool_bytes, rec_off, live, n,
                       (const uint64_t *)(p + w.table + kHidxHeadBytes), hidx_slots(n), hash_mask, (u64a *)hdr, sums, w.tiles,
                       (uint64_t *)(p + w.pos), (uint32_t *)(p + w.mark));
    hipLaunchKernelGGL(k_sf_scan, dim3(2), dim3(SW), 0, s, sums, w.tiles, hdr + cBytes);
    if ((e = hipGetLastError()) != hipSuccess) return drained(s, e);
    const uint64_t stamp[2] = {n, kCompactMagic};
    if ((e = hipMemcpyAsync(hdr + cN, stamp, sizeof stamp, hipMemcpyHostToDevice, s)) != hipSuccess) return drained(s, e);
    uint64_t h[8 + 3];  // the header and the table's [overflow][occupied slots][bad records]
    if ((e = hipMemcpyAsync(h, hdr, sizeof h, hipMemcpyDeviceToHost, s)) != hipSuccess) return drained(s, e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    // err, live_in, distinct, survivors, tombstoned, image_bytes, table overflow, winners
    const uint64_t out[8] = {h[cErr], h[cLive], h[8 + hCount], h[cSurv], h[cTomb], h[cBytes], h[8 + hOverflow], h[cWin]};
    memcpy(out_host, out, sizeof out);
    return hipSuccess;
}

hipError_t launch_segcompact_emit(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, uint64_t n,
                                  uint64_t timestamp, uint64_t survivors, uint64_t image_bytes, void *ws, uint8_t *image,
                                  uint64_t *out_rec_off, hipStream_t s) {
    if (survivors == 0) return hipMemsetAsync(out_rec_off, 0, 8, s);
    const SegCompactWs w = segcompact_ws_layout(n);
    uint8_t *p = (uint8_t *)ws;
    const uint64_t *hdr = (const uint64_t *)p;
    const CompactArg a{n, survivors, image_bytes};
    const uint64_t chunks = (((uint64_t)image & 15) + image_bytes + 15) >> 4;
    hipLaunchKernelGGL(k_sc_place, dim3(stream_grid(n)), dim3(256), 0, s, hdr, a, rec_off, (const uint64_t *)(p + w.sums), w.tiles,
                       (const uint64_t *)(p + w.pos), (const uint32_t *)(p + w.mark), (uint64_t *)(p + w.src), out_rec_off);
    hipLaunchKernelGGL(k_sc_copy, dim3(stream_grid(chunks) * 4u), dim3(256), 0, s, hdr, a, pool, pool_bytes,
                       (const uint64_t *)(p + w.src), (const uint64_t *)out_rec_off, timestamp, image);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_seg_seal(image, image_bytes, out_rec_off, survivors, s);
}

hipError_t launch_offsets_shift(const uint64_t *src, uint64_t n, uint64_t sub, uint64_t add, uint64_t *dst, uint64_t end,
                                hipStream_t s) {
    hipLaunchKernelGGL(k_off_shift, dim3(stream_grid(n + 1)), dim3(256), 0, s, src, n, sub, add, dst, end);
    return hipGetLastError();
}

hipError_t launch_hidx_logical(const void *table, uint64_t capacity, const uint8_t *pool, uint64_t pool_bytes,
                               uint64_t *sum_dev, uint64_t *sum_host, hipStream_t s) {
    hipError_t e;
    if ((e = hipMemsetAsync(sum_dev, 0, 8, s)) != hipSuccess) return e;
    const uint64_t slots = hidx_slots(capacity);
    hipLaunchKernelGGL(k_hidx_logical, dim3(stream_grid(slots)), dim3(256), 0, s,
                       (const uint64_t *)table + kHidxHeadBytes / 8, slots, pool, pool_bytes, (u64a *)sum_dev);
    if ((e = hipGetLastError()) != hipSuccess) return drained(s, e);
    if ((e = hipMemcpyAsync(sum_host, sum_dev, 8, hipMemcpyDeviceToHost, s)) != hipSuccess) return drained(s, e);
    return hipStreamSynchronize(s);
}

}  // namespace seb
