// seb_memwrite.hip — the memtable's write side on the device: a Put / Delete batch framed as
// WAL.Append's records, MemTable.size's change for a new run, and up to kMemRuns sorted runs folded into the
// one run GetAllEntries() returns.  The host half and the semantics are in seb_memwrite.cpp.
//
//   k_frame_len    a workgroup per tile of kWriteTile ops, four consecutive ops per lane: an op's offsets are
//                  checked (one atomicMin keeps the least bad op), its record length is 21 + keyLen + (deleted ?
//                  0 : valueLen), and a scan in the workgroup leaves rec_off relative to the tile
//   k_write_scan   exclusive scan of per-tile sums, one workgroup of kScanWidth lanes per array with a carry
//                  from one stretch of kScanWidth tiles to the next (scan_tile_sums, seb_scan.h, shared with the Get
//                  path's plan)
//   k_frame_add    rec_off[i] += its tile's base; rec_off[n] = the image's size
//   k_frame_emit   a lane per 16 aligned bytes of the image: a bisection of rec_off finds the record of its
//                  first byte; a chunk that lies inside one key or one value and whose aligned source words lie
//                  inside the ops' arrays is two 16-byte loads and a shift, every other chunk is made byte by
//                  byte (the header's fields, key bytes, value bytes).  The CRC field is left 0 for the seal
//   k_size_delta   a lane per entry of the new run: k_runs_search's bisection over the existing runs' prefix
//                  arrays, first holder wins; one wave-level sum and one 64-bit atomic per wave
//   k_fold_rank    a lane per (run, entry): its lower bound in every other run by the same bisection, and
//                  whether an earlier run holds its key.  Own index + the lower bounds + one per earlier holder
//                  is the entry's position in the union ordered by (key, run); (run, entry, live, deleted, key
//                  length, value length) goes to that slot
//   k_fold_sums    per tile of kWriteTile slots: the live entries' count, key bytes and value bytes
//   k_fold_emit    a workgroup per tile: the live entries' offsets by a scan in the workgroup, key_off / val_off /
//                  deleted / seq, then the tile's two output ranges, each contiguous, 16 aligned bytes at a time
//
// Every index and offset that comes out of memory is clamped before it is used: a rec_off, an index or a
// workspace that does not belong to its input gives wrong bytes, never an access outside the arrays the
// caller described.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "seb_kernels.h"
#include "seb_keycmp.h"
#include "seb_scan.h"

namespace seb {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) uint8_t *gbytes;

constexpr uint32_t WT = kWriteTile;
constexpr uint32_t SW = kScanWidth;
constexpr uint32_t kWalHdr = 21;  // [crc u32][seq u64][keySize u32][valueSize u32][deleted u8]
constexpr uint64_t kFoldMagic = 0x444C4F464E555253ull;  // "SRUNFOLD"

enum : uint32_t { kSlotLive = 1u << 8, kSlotDeleted = 1u << 9 };
// the fold workspace's header (u64 words)
enum : uint32_t { fErr = 0, fTotal = 1, fTiles = 2, fOut = 3, fKey = 4, fVal = 5, fTomb = 6, fMaxSeq = 7, fMagic = 8 };

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
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

// x[a * count ..] = its exclusive scan in place, total[a] = its sum; workgroup a takes array a
__global__ __launch_bounds__(SW) void k_write_scan(uint64_t *x, uint64_t count, uint64_t *total) {
    scan_tile_sums(x + (uint64_t)blockIdx.x * count, count, total + blockIdx.x);  // seb_scan.h
}

// ------------------------------------------------------------------ frame -------------------

// an op's lengths from its offsets alone; a pair that decreases or spans 2^32 bytes or more reads as 0
__device__ __forceinline__ bool span32(uint64_t a, uint64_t b, uint32_t *len) {
    const bool ok = a <= b && b - a < (1ull << 32);
    *len = ok ? (uint32_t)(b - a) : 0u;
    return ok;
}

// scratch: [0] the least bad op << 1 | (0 key, 1 value), all ones for none; [1] the image's size; [2..] tile sums
__global__ __launch_bounds__(256) void k_frame_len(KeyBatch kb, const uint64_t *__restrict__ val_off,
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
        if (!kok || !vok) {
            const unsigned long long b = i << 1 | (kok ? 1 : 0);
            bad = b < bad ? b : bad;
            continue;
        }
        const bool del = deleted && ((gbytes)deleted)[i] != 0;
        len[q] = (uint64_t)kWalHdr + kl + (del ? 0u : vl);
        sum += len[q];
    }
    bad = wave_min(bad);
    if ((tid & 63) == 0 && bad != ~0ull) atomicMin((unsigned long long *)scratch, bad);
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
    if (tid == 255) scratch[2 + blockIdx.x] = S[255];
}

__global__ __launch_bounds__(256) void k_frame_add(uint64_t *__restrict__ rec_off, uint64_t n,
                                                   const uint64_t *__restrict__ scratch) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n)
        rec_off[i] += scratch[2 + i / WT];
    else if (i == n)
        rec_off[n] = scratch[1];
}

struct FrameOp {  // what an op contributes to its record
    uint64_t key, val;  // addresses of its key and value bytes
    uint64_t seq;
    uint32_t klen, vlen;  // vlen 0 for a Delete
    uint32_t del;
};
__device__ __forceinline__ FrameOp frame_op(const KeyBatch &kb, const uint8_t *vals, const uint64_t *val_off,
                                            const uint8_t *deleted, uint64_t first_seq, uint64_t i) {
    FrameOp o;
    uint64_t ko = i * (uint64_t)kb.stride;
    o.klen = kb.stride;
    if (kb.offsets) {
        ko = kb.offsets[i];
        span32(ko, kb.offsets[i + 1], &o.klen);
    }
    const uint64_t vo = val_off[i];
    span32(vo, val_off[i + 1], &o.vlen);
    o.del = deleted && ((gbytes)deleted)[i] != 0 ? 1u : 0u;
    if (o.del) o.vlen = 0;
    o.key = (uint64_t)kb.data + ko;
    o.val = (uint64_t)vals + vo;
    o.seq = first_seq + i;
    return o;
}
// byte p of the op's record, the CRC field as 0
__device__ __forceinline__ uint32_t frame_byte(const FrameOp &o, uint64_t p) {
    if (p < 4) return 0;
    if (p < 12) return (uint32_t)(o.seq >> (8 * (p - 4))) & 0xFFu;
    if (p < 16) return (o.klen >> (8 * (p - 12))) & 0xFFu;
    if (p < 20) return (o.vlen >> (8 * (p - 16))) & 0xFFu;
    if (p == 20) return o.del;
    p -= kWalHdr;
    if (p < o.klen) return ((gbytes)o.key)[p];
    p -= o.klen;
    if (p < o.vlen) return ((gbytes)o.val)[p];
    return 0;  // behind the record: a rec_off that is not this batch's
}

__global__ __launch_bounds__(256) void k_frame_emit(KeyBatch kb, const uint8_t *__restrict__ vals,
                                                    const uint64_t *__restrict__ val_off,
                                                    const uint8_t *__restrict__ deleted, uint64_t first_seq,
                                                    const uint64_t *__restrict__ rec_off, uint8_t *__restrict__ image,
                                                    uint64_t image_bytes) {
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
        const uint64_t mid = (i + ih + 1) >> 1;
        if (rec_off[mid] <= lo) i = mid; else ih = mid - 1;
    }
    FrameOp o = frame_op(kb, vals, val_off, deleted, first_seq, i);
    uint64_t beg = rec_off[i], end = rec_off[i + 1];
    const uint64_t p0 = lo - beg;  // wraps where rec_off[0] > lo: no fast path, and frame_byte gives 0
    if (!head && end16 <= image_bytes && lo >= beg && lo + 16 <= end) {
        uint64_t w0, w1;
        bool done = false;
        if (p0 >= kWalHdr && p0 + 16 <= (uint64_t)kWalHdr + o.klen)
            done = load16(o.key + (p0 - kWalHdr), klo, khi, w0, w1);
        else if (p0 >= (uint64_t)kWalHdr + o.klen && p0 + 16 <= (uint64_t)kWalHdr + o.klen + o.vlen)
            done = load16(o.val + (p0 - kWalHdr - o.klen), vlo, vhi, w0, w1);
        if (done) {
            store16(a0 + (c << 4), w0, w1);
            return;
        }
    }
    for (uint64_t j = lo; j < hi; ++j) {
        while (j >= end && i + 1 < n) {
            ++i;
            o = frame_op(kb, vals, val_off, deleted, first_seq, i);
            beg = end;
            end = rec_off[i + 1];
        }
        image[j] = (uint8_t)frame_byte(o, j - beg);
    }
}

// ------------------------------------------------------------------ the bisection -----------

// key (k0, k1 = its prefix words) against entry e of run t, whose prefix is p (seb_memget.hip's cmp_entry)
__device__ __forceinline__ int cmp_entry(const MemRun &t, uint32_t e, const u32x4 p, const uint8_t *key, uint32_t klen,
                                         uint64_t k0, uint64_t k1) {
    const uint64_t be[2] = {(uint64_t)p.x | ((uint64_t)p.y << 32), (uint64_t)p.z | ((uint64_t)p.w << 32)};
    if (k0 != be[0]) return k0 < be[0] ? -1 : 1;
    if (k1 != be[1]) return k1 < be[1] ? -1 : 1;
    uint64_t o0 = gload(t.koff, e), o1 = gload(t.koff, (uint64_t)e + 1);
    o0 = o0 < t.key_bytes ? o0 : t.key_bytes;
    o1 = o1 < o0 ? o0 : o1 < t.key_bytes ? o1 : t.key_bytes;
    return cmp_key(key, klen, k0, k1, be, t.bytes + o0, (uint32_t)(o1 - o0));
}
// sort.Search: the least entry of t that is >= key (t.n for none); *eq = that entry is the key
__device__ __forceinline__ uint32_t lower_bound(const MemRun &t, const uint8_t *key, uint32_t klen, uint64_t k0,
                                                uint64_t k1, bool *eq) {
    uint32_t a = 0, b = t.n;
    bool e = false;
    while (a < b) {
        const uint32_t mid = a + ((b - a) >> 1);
        const int cmp = cmp_entry(t, mid, gload((const u32x4 *)t.pre, mid), key, klen, k0, k1);
        if (cmp > 0) {
            a = mid + 1;
        } else {
            b = mid;
            e = cmp == 0;
        }
    }
    *eq = e && a < t.n;
    return a;
}
// entry e's key with its offsets clamped to the run's key bytes
__device__ __forceinline__ const uint8_t *entry_key(const MemRun &t, uint32_t e, uint32_t *klen) {
    uint64_t o0 = gload(t.koff, e), o1 = gload(t.koff, (uint64_t)e + 1);
    o0 = o0 < t.key_bytes ? o0 : t.key_bytes;
    o1 = o1 < o0 ? o0 : o1 < t.key_bytes ? o1 : t.key_bytes;
    const uint64_t d = o1 - o0;
    *klen = d < 0xFFFFFFFFull ? (uint32_t)d : 0xFFFFFFFFu;
    return t.bytes + o0;
}
// entry e's value length as MemTable.size counts it: 0 for a tombstone; offsets that decrease read as 0
__device__ __forceinline__ uint32_t live_vlen(const MemRun &t, uint32_t e, bool *del) {
    *del = t.deleted && gload(t.deleted, e) != 0;
    const uint64_t v0 = gload(t.voff, e), v1 = gload(t.voff, (uint64_t)e + 1);
    const uint64_t d = v1 > v0 ? v1 - v0 : 0;
    return *del ? 0u : d < 0xFFFFFFFFull ? (uint32_t)d : 0xFFFFFFFFu;
}

// ------------------------------------------------------------------ size delta --------------

__global__ __launch_bounds__(256) void k_size_delta(MemRun fresh, MemRunTab tab, unsigned long long *delta) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    long long d = 0;
    if (e < fresh.n) {
        uint32_t klen;
        const uint8_t *key = entry_key(fresh, (uint32_t)e, &klen);
        const uint64_t k0 = be64(key, klen), k1 = klen > 8 ? be64(key + 8, klen - 8) : 0ull;
        bool del;
        const uint32_t vlen = live_vlen(fresh, (uint32_t)e, &del);
        bool held = false;
        for (uint32_t r = 0; r < tab.nruns && !held; ++r) {
            const MemRun &t = tab.r[r];
            const uint32_t a = lower_bound(t, key, klen, k0, k1, &held);
            if (held) {
                bool odel;
                d = (long long)vlen - (long long)live_vlen(t, a, &odel);
            }
        }
        if (!held) d = (long long)klen + 16 + vlen;
    }
    const unsigned long long s = wave_sum((unsigned long long)d);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(delta, s);
}

// ------------------------------------------------------------------ fold --------------------

__global__ __launch_bounds__(256) void k_fold_rank(FoldTab T, uint64_t N, uint4 *__restrict__ slot,
                                                   uint64_t *__restrict__ hdr) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long mseq = 0;
    if (g < N) {
        uint32_t r = 0;
        while (r + 1 < T.tab.nruns && g >= T.begin[r + 1]) ++r;
        const MemRun &t = T.tab.r[r];
        const uint32_t e = (uint32_t)(g - T.begin[r]);
        if (e == 0 && gload(t.voff, (uint64_t)t.n) > T.val_bytes[r]) atomicMin((unsigned long long *)&hdr[fErr], (unsigned long long)r);
        uint32_t klen;
        const uint8_t *key = entry_key(t, e, &klen);
        const u32x4 p = gload((const u32x4 *)t.pre, e);
        const uint64_t k0 = (uint64_t)p.x | ((uint64_t)p.y << 32), k1 = (uint64_t)p.z | ((uint64_t)p.w << 32);
        uint64_t pos = e;
        bool shadowed = false;
        for (uint32_t r2 = 0; r2 < T.tab.nruns; ++r2) {
            if (r2 == r || T.tab.r[r2].n == 0) continue;
            bool eq;
            pos += lower_bound(T.tab.r[r2], key, klen, k0, k1, &eq);
            if (eq && r2 < r) ++pos, shadowed = true;
        }
        bool del;
        uint32_t vlen = live_vlen(t, e, &del);
        {  // the value's bytes must lie inside the run's value bytes
            const uint64_t vb = T.val_bytes[r], v0 = gload(t.voff, e);
            const uint64_t room = v0 < vb ? vb - v0 : 0;
            if (vlen > room) vlen = (uint32_t)room;
        }
        if (t.seq) mseq = gload(t.seq, e);
        if (pos < N) slot[pos] = make_uint4(e, r | (shadowed ? 0u : kSlotLive) | (del ? kSlotDeleted : 0u), klen, vlen);
    }
    mseq = wave_max(mseq);
    if ((threadIdx.x & 63) == 0 && mseq) atomicMax((unsigned long long *)&hdr[fMaxSeq], mseq);
}

__global__ __launch_bounds__(256) void k_fold_sums(const uint4 *__restrict__ slot, uint64_t N, uint64_t *__restrict__ sums,
                                                   uint64_t tiles, uint64_t *__restrict__ hdr) {
    __shared__ unsigned long long acc[4];
    const uint32_t tid = threadIdx.x;
    if (tid < 4) acc[tid] = 0;
    __syncthreads();
    const uint64_t ts = (uint64_t)blockIdx.x * WT;
    unsigned long long cnt = 0, kb = 0, vb = 0, tomb = 0;
    for (uint32_t q = 0; q < WT / 256; ++q) {
        const uint64_t x = ts + q * 256 + tid;
        if (x >= N) break;
        const uint4 s = slot[x];
        if (s.y & kSlotLive) ++cnt, kb += s.z, vb += s.w, tomb += s.y & kSlotDeleted ? 1 : 0;
    }
    cnt = wave_sum(cnt), kb = wave_sum(kb), vb = wave_sum(vb), tomb = wave_sum(tomb);
    if ((tid & 63) == 0) atomicAdd(&acc[0], cnt), atomicAdd(&acc[1], kb), atomicAdd(&acc[2], vb), atomicAdd(&acc[3], tomb);
    __syncthreads();
    if (tid == 0) {
        sums[blockIdx.x] = acc[0];
        sums[tiles + blockIdx.x] = acc[1];
        sums[2 * tiles + blockIdx.x] = acc[2];
        if (acc[3]) atomicAdd((unsigned long long *)&hdr[fTomb], acc[3]);
        if (blockIdx.x == 0) hdr[fTotal] = N, hdr[fTiles] = tiles, hdr[fMagic] = kFoldMagic;
    }
}

// One of a tile's two output ranges: dst[0, total) is the concatenation of the tile's live entries' keys (or
// values); q[i] = entry i's offset in it (q[cnt] = total), its bytes are at address sp[i] in run sr[i]'s array
// [lo[sr[i]], hi[sr[i]]), inside which alone an aligned 16-byte load is made.  room = the bytes the caller's
// array still holds from dst.  (k_replay_emit's emit_stream with a source array per entry.)
__device__ __forceinline__ void copy_stream(uint8_t *__restrict__ dst, uint64_t total, uint64_t room, const uint64_t *q,
                                            const uint64_t *sp, const uint8_t *sr, uint32_t cnt, const uint64_t *lo8,
                                            const uint64_t *hi8) {
    if (total == 0 || cnt == 0) return;
    if (room < total) total = room;
    const uint64_t a = (uint64_t)dst, a0 = a & ~15ull;
    const uint64_t lead = a - a0, chunks = (lead + total + 15) >> 4;
    for (uint64_t c = threadIdx.x; c < chunks; c += blockDim.x) {
        const bool head = (c << 4) < lead;
        const uint64_t lo = head ? 0 : (c << 4) - lead;
        const uint64_t end16 = (c << 4) + 16 - lead, hi = end16 < total ? end16 : total;
        uint32_t i = 0, ih = cnt - 1;  // the last entry with q[i] <= lo: the one that holds byte lo
        while (i < ih) {
            const uint32_t mid = (i + ih + 1) >> 1;
            if (q[mid] <= lo) i = mid; else ih = mid - 1;
        }
        uint64_t end = q[i + 1];
        uint64_t w0, w1;
        if (!head && end16 <= total && lo + 16 <= end && load16(sp[i] + (lo - q[i]), lo8[sr[i]], hi8[sr[i]], w0, w1)) {
            store16(a0 + (c << 4), w0, w1);
            continue;
        }
        gbytes src = (gbytes)sp[i];
        uint64_t beg = q[i];
        for (uint64_t j = lo; j < hi; ++j) {
            while (j >= end) {  // j < total <= q[cnt]: ends with i < cnt
                ++i;
                beg = end;
                end = q[i + 1];
                src = (gbytes)sp[i];
            }
            dst[j] = src[j - beg];
        }
    }
}

struct FoldSizesArg {  // seb_fold_sizes
    uint64_t entries_in, entries_out, key_bytes, val_bytes, shadowed, tombstones, max_sequence, memtable_size;
};

__global__ __launch_bounds__(256) void k_fold_emit(FoldTab T, const uint8_t *__restrict__ ws, uint64_t sums_at,
                                                   uint64_t slot_at, FoldSizesArg sz, uint8_t *__restrict__ keys,
                                                   uint64_t *__restrict__ key_off, uint8_t *__restrict__ vals,
                                                   uint64_t *__restrict__ val_off, uint8_t *__restrict__ deleted,
                                                   uint64_t *__restrict__ seq) {
    __shared__ uint64_t lk[WT + 1], lv[WT + 1];
    __shared__ uint64_t spk[WT], spv[WT];
    __shared__ uint8_t sr[WT];
    __shared__ uint32_t sc[256];
    __shared__ uint64_t sk[256], sv[256];
    __shared__ uint64_t klo[kMemRuns], khi[kMemRuns], vlo[kMemRuns], vhi[kMemRuns];
    const uint32_t tid = threadIdx.x;
    const uint64_t *hdr = (const uint64_t *)ws;
    const uint64_t N = sz.entries_in, tiles = (N + WT - 1) / WT;
    if (hdr[fMagic] != kFoldMagic || hdr[fTotal] != N || hdr[fTiles] != tiles) return;  // not this plan's sizes
    if (tid < kMemRuns) {
        const bool on = tid < T.tab.nruns && T.tab.r[tid].n;
        klo[tid] = on ? (uint64_t)T.tab.r[tid].bytes : 0;
        khi[tid] = on ? klo[tid] + T.tab.r[tid].key_bytes : 0;
        vlo[tid] = on ? (uint64_t)T.vals[tid] : 0;
        vhi[tid] = on ? vlo[tid] + T.val_bytes[tid] : 0;
    }
    const uint64_t *sums = (const uint64_t *)(ws + sums_at);
    const uint4 *slot = (const uint4 *)(ws + slot_at);
    const uint64_t ts = (uint64_t)blockIdx.x * WT;
    const uint64_t obase = sums[blockIdx.x], kbase = sums[tiles + blockIdx.x], vbase = sums[2 * tiles + blockIdx.x];
    // a thread takes 4 consecutive slots
    uint4 s[4];
    uint64_t kat[4], vat[4];  // the addresses of a live entry's key and value bytes
    uint32_t c = 0;
    uint64_t ks = 0, vs = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        const uint64_t x = ts + 4 * tid + q;
        s[q] = make_uint4(0, 0, 0, 0);
        kat[q] = vat[q] = 0;
        if (x < N) s[q] = slot[x];
        const uint32_t r = s[q].y & 0xFFu;
        if (r >= T.tab.nruns || s[q].x >= T.tab.r[r].n) s[q].y = 0;  // never in a plan that succeeded
        if (s[q].y & kSlotLive) {
            // the entry's bytes as the run's offsets give them now, clamped to the run's key bytes and value
            // bytes: an entry the plan counted longer than that (a run that changed since) is dropped
            const MemRun &t = T.tab.r[r];
            uint32_t klen;
            kat[q] = (uint64_t)entry_key(t, s[q].x, &klen);
            const uint64_t vb = T.val_bytes[r];
            uint64_t v0 = gload(t.voff, s[q].x);
            v0 = v0 < vb ? v0 : vb;
            vat[q] = (uint64_t)T.vals[r] + v0;
            if (s[q].z > klen || (uint64_t)s[q].w > vb - v0) s[q].y = 0;
        }
        if (s[q].y & kSlotLive) ++c, ks += s[q].z, vs += s[q].w;
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
        if (!(s[q].y & kSlotLive)) continue;
        const uint32_t r = s[q].y & 0xFFu, e = s[q].x;
        const MemRun &t = T.tab.r[r];
        lk[ci] = ko, lv[ci] = vo;
        spk[ci] = kat[q];
        spv[ci] = vat[q];
        sr[ci] = (uint8_t)r;
        const uint64_t o = obase + ci;
        if (o < sz.entries_out) {
            key_off[o] = kbase + ko;
            val_off[o] = vbase + vo;
            deleted[o] = s[q].y & kSlotDeleted ? 1 : 0;
            if (seq) seq[o] = t.seq ? gload(t.seq, e) : 0;
        }
        ++ci, ko += s[q].z, vo += s[q].w;
    }
    if (tid == 0) {
        lk[cnt] = ktot, lv[cnt] = vtot;
        if (blockIdx.x == 0) key_off[sz.entries_out] = sz.key_bytes, val_off[sz.entries_out] = sz.val_bytes;
    }
    __syncthreads();
    if (kbase < sz.key_bytes) copy_stream(keys + kbase, ktot, sz.key_bytes - kbase, lk, spk, sr, cnt, klo, khi);
    if (vbase < sz.val_bytes) copy_stream(vals + vbase, vtot, sz.val_bytes - vbase, lv, spv, sr, cnt, vlo, vhi);
}

inline uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

hipError_t drained(hipStream_t s, hipError_t e) {
    (void)hipStreamSynchronize(s);
    return e;
}

}  // namespace

// ------------------------------------------------------------------ launches ----------------

uint64_t frame_scratch_bytes(uint64_t n) { return up16(8 * (2 + (n + WT - 1) / WT)); }

hipError_t launch_frame_plan(const KeyBatch &kb, const uint64_t *val_off, const uint8_t *deleted, uint64_t *rec_off,
                             void *scratch, uint64_t *image_bytes_host, uint64_t *err_host, hipStream_t s) {
    uint64_t *sc = (uint64_t *)scratch;
    const uint64_t n = kb.n, tiles = (n + WT - 1) / WT;
    hipError_t e;
    if ((e = hipMemsetAsync(sc, 0xFF, 8, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_frame_len, dim3((unsigned)tiles), dim3(256), 0, s, kb, val_off, deleted, rec_off, sc);
    hipLaunchKernelGGL(k_write_scan, dim3(1), dim3(SW), 0, s, sc + 2, tiles, sc + 1);
    hipLaunchKernelGGL(k_frame_add, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, s, rec_off, n, (const uint64_t *)sc);
    if ((e = hipGetLastError()) != hipSuccess) return drained(s, e);
    uint64_t h[2];
    if ((e = hipMemcpyAsync(h, sc, sizeof h, hipMemcpyDeviceToHost, s)) != hipSuccess) return drained(s, e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    *err_host = h[0];
    *image_bytes_host = h[1];
    return hipSuccess;
}

hipError_t launch_frame_emit(const KeyBatch &kb, const uint8_t *vals, const uint64_t *val_off, const uint8_t *deleted,
                             uint64_t first_seq, const uint64_t *rec_off, uint8_t *image, uint64_t image_bytes,
                             hipStream_t s) {
    const uint64_t chunks = (((uint64_t)image & 15) + image_bytes + 15) >> 4, g = (chunks + 255) / 256;
    if (g >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_frame_emit, dim3((unsigned)g), dim3(256), 0, s, kb, vals, val_off, deleted, first_seq, rec_off,
                       image, image_bytes);
    return hipGetLastError();
}

hipError_t launch_size_delta(const MemRun &fresh, const MemRunTab &tab, int64_t *delta, hipStream_t s) {
    hipError_t e;
    if ((e = hipMemsetAsync(delta, 0, 8, s)) != hipSuccess) return e;
    if (fresh.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_size_delta, dim3((fresh.n + 255) / 256), dim3(256), 0, s, fresh, tab, (unsigned long long *)delta);
    return hipGetLastError();
}

FoldWs fold_ws_layout(uint64_t entries) {
    FoldWs w{};
    w.tiles = (entries + WT - 1) / WT;
    w.sums = 128;  // behind the header
    w.slots = w.sums + up16(8 * 3 * w.tiles);
    w.bytes = w.slots + 16 * entries;
    return w;
}

hipError_t launch_fold_plan(const FoldTab &tab, uint64_t entries, void *ws, void *sizes_host, uint64_t *err_host,
                            hipStream_t s) {
    const FoldWs w = fold_ws_layout(entries);
    uint8_t *p = (uint8_t *)ws;
    uint64_t *hdr = (uint64_t *)p, *sums = (uint64_t *)(p + w.sums);
    uint4 *slot = (uint4 *)(p + w.slots);
    hipError_t e;
    // the slots start as "not live": positions a stale index leaves out read as nothing
    if ((e = hipMemsetAsync(p, 0, w.bytes, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(hdr + fErr, 0xFF, 8, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_fold_rank, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, tab, entries, slot, hdr);
    hipLaunchKernelGGL(k_fold_sums, dim3((unsigned)w.tiles), dim3(256), 0, s, (const uint4 *)slot, entries, sums, w.tiles, hdr);
    hipLaunchKernelGGL(k_write_scan, dim3(3), dim3(SW), 0, s, sums, w.tiles, hdr + fOut);
    if ((e = hipGetLastError()) != hipSuccess) return drained(s, e);
    uint64_t h[16];
    if ((e = hipMemcpyAsync(h, hdr, sizeof h, hipMemcpyDeviceToHost, s)) != hipSuccess) return drained(s, e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    *err_host = h[fErr];
    const uint64_t out[8] = {entries, h[fOut], h[fKey], h[fVal], entries - h[fOut], h[fTomb], h[fMaxSeq],
                             h[fKey] + 16 * h[fOut] + h[fVal]};
    memcpy(sizes_host, out, sizeof out);
    return hipSuccess;
}

hipError_t fold_ws_check(const void *sizes, const void *ws, bool *ok, hipStream_t s) {
    FoldSizesArg sz;
    memcpy(&sz, sizes, sizeof sz);
    uint64_t h[16];
    hipError_t e;
    if ((e = hipMemcpyAsync(h, ws, sizeof h, hipMemcpyDeviceToHost, s)) != hipSuccess) return drained(s, e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    const uint64_t n = sz.entries_in;
    *ok = h[fMagic] == kFoldMagic && h[fErr] == ~0ull && h[fTotal] == n && h[fTiles] == (n + WT - 1) / WT &&
          h[fOut] == sz.entries_out && h[fKey] == sz.key_bytes && h[fVal] == sz.val_bytes && h[fTomb] == sz.tombstones &&
          h[fMaxSeq] == sz.max_sequence;
    return hipSuccess;
}

hipError_t launch_fold_emit(const FoldTab &tab, const void *sizes, const void *ws, uint8_t *keys, uint64_t *key_off,
                            uint8_t *vals, uint64_t *val_off, uint8_t *deleted, uint64_t *seq, hipStream_t s) {
    FoldSizesArg sz;
    memcpy(&sz, sizes, sizeof sz);
    const FoldWs w = fold_ws_layout(sz.entries_in);
    hipLaunchKernelGGL(k_fold_emit, dim3((unsigned)w.tiles), dim3(256), 0, s, tab, (const uint8_t *)ws, w.sums, w.slots, sz,
                       keys, key_off, vals, val_off, deleted, seq);
    return hipGetLastError();
}

}  // namespace seb
