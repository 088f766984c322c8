// seb_hashindex.hip — the hash index's read side on the device: recover() for a set of segment
// images held back to back in one byte pool, and Get for a key batch.  The semantics and the host half are in
// seb_hashindex.cpp; a record is named by its pool offset and the later record of a key is the one at the greater
// offset.
//
//   k_seg_crc      k_wal_crc's verify mode for the 20-byte header (the same staging and the same LDS walk, seb_crc.h),
//                  with each record's length taken from its own header and checked against pool_bytes: a workgroup
//                  owns 256 consecutive records, stages their span in LDS where it fits, and each lane checksums its
//                  record.  A bad record's index goes into its segment's minimum (an agent-scope atomicMin).  Its
//                  seal mode (the write side) stores each record's checksum into its CRC field
//                  instead of comparing it, as SEB_WAL_SEAL does for k_wal_crc; the field is not part of the checksum.
//   k_seg_live     a lane per record: live[r] = r lies before its segment's first bad record
//   k_seg_valid    a lane per segment: the minimum clamped to the segment's record count = valid[s]
//   k_hidx_insert  a lane per live record into the open-addressing table (linear probing, a counted loop of at most
//                  table-size steps).  Every access to the table in this launch is an agent-scope atomic: the per-XCD
//                  L2s are not coherent with each other, and only what an atomic returned decides anything.  The
//                  pool does not change during the launch and is read with plain loads.  A lane that runs out of
//                  steps sets the overflow word, which the other lanes poll every 32 steps; no lane waits for another.
//   k_hidx_get     a lane per key probes with plain loads (no insert may run concurrently); with verify, the lane
//                  then checksums its hit's record before the tombstone rule.
//
// The table: a 64-byte header [overflow][occupied slots][bad records] and the smallest power of two >= 2 * capacity
// slots of one u64 each: 0 = empty, else a hash tag in the high 16 bits and record offset + 1 in the low 48.  A slot
// goes from empty to one key once and keeps that key; records of the same key carry the same tag, so an atomicMax on
// the slot keeps the one at the greatest offset.  Whatever the table or the pool hold, every slot index is masked and
// every record is re-checked against pool_bytes before a byte of it is read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "seb_crc.h"
#include "seb_hidx_dev.h"
#include "seb_kernels.h"

namespace seb {

namespace {

constexpr uint64_t kHeadBytes = kHidxHeadBytes;
constexpr uint32_t kSegRecs = 256;
constexpr uint32_t kSegLds = 36 * 1024;  // k_wal_crc's window

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// the last s < nseg with first[s] <= r (nseg >= 1)
__device__ __forceinline__ uint64_t seg_of(const uint64_t *__restrict__ first, uint64_t nseg, uint64_t r) {
    uint64_t lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo + 1) >> 1);
        if (first[mid] <= r) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// kSeal: the checksum of every record that lies inside the pool goes into its CRC field (bytes the walk above never
// uses: a neighbouring workgroup's window may hold them, its checksums start 4 bytes further on); ok and first_bad
// are not touched.
template <uint32_t kLds, bool kSeal>
__global__ __launch_bounds__(kSegRecs) void k_seg_crc(const uint8_t *pool, uint64_t pool_bytes,
                                                      const uint64_t *__restrict__ off, uint64_t n,
                                                      const uint64_t *__restrict__ seg_first, uint64_t nseg,
                                                      uint8_t *__restrict__ ok, u64a *__restrict__ first_bad) {
    __shared__ uint32_t tab[4][256];
    __shared__ uint4 stage[kLds / 16 + 1];
    crc_stage_tables(tab);
    const uint64_t r0 = (uint64_t)blockIdx.x * kSegRecs;
    const uint64_t r1 = r0 + kSegRecs < n ? r0 + kSegRecs : n;
    // the workgroup's span: from its first record to the end of its last, where that one lies inside the pool
    const uint64_t s0 = off[r0], sl = off[r1 - 1];
    uint32_t ks = 0, vs = 0;
    uint64_t el = 0;
    bool staged = false;
    uintptr_t base = 0;
    if (s0 <= sl && rec_extent(pool, pool_bytes, sl, &ks, &vs)) {
        el = sl + kSegHeader + ks + vs;
        base = ((uintptr_t)(pool + s0)) & ~(uintptr_t)15;
        const uintptr_t end = (uintptr_t)(pool + el);
        staged = end - base <= kLds;
        if (staged) {
            const uint32_t chunks = (uint32_t)((end - base + 15) >> 4);
            const uint4 *src = (const uint4 *)base;
            for (uint32_t c = threadIdx.x; c < chunks; c += blockDim.x) stage[c] = src[c];
        }
    }
    __syncthreads();
    const uint64_t i = r0 + threadIdx.x;
    if (i >= r1) return;
    const uint64_t s = off[i];
    bool good = false, whole = false;
    uint32_t crc = 0;
    if (staged && s >= s0 && s <= el && el - s >= kSegHeader) {  // the header is in the window
        const uint8_t *lb = (const uint8_t *)stage;
        const uint32_t b = (uint32_t)((uintptr_t)(pool + s) - base);
        ks = ld_u32_le(lb + b + 12), vs = ld_u32_le(lb + b + 16);
        const uint64_t payload = (uint64_t)ks + vs;
        if (payload < (1ull << 32) && payload <= pool_bytes - s - kSegHeader) {
            const uint64_t e = s + kSegHeader + payload;
            crc = e <= el ? crc_lds((const uint32_t *)stage, b + 4, (uint32_t)(kSegHeader - 4 + payload), tab)
                          : ~crc_range(~0u, pool, s + 4, e, tab);
            whole = true;
            if constexpr (!kSeal) good = crc == ld_u32_le(lb + b);
        }
    } else if (rec_extent(pool, pool_bytes, s, &ks, &vs)) {
        crc = ~crc_range(~0u, pool, s + 4, s + kSegHeader + ks + vs, tab);
        whole = true;
        if constexpr (!kSeal) good = crc == ld_u32_le(pool + s);
    }
    if constexpr (kSeal) {
        if (whole) {
            uint8_t *field = const_cast<uint8_t *>(pool) + s;
            field[0] = (uint8_t)crc, field[1] = (uint8_t)(crc >> 8), field[2] = (uint8_t)(crc >> 16), field[3] = (uint8_t)(crc >> 24);
        }
        return;
    }
    ok[i] = good ? 1 : 0;
    if (!good && first_bad && nseg) {
        const uint64_t sg = seg_of(seg_first, nseg, i);
        __hip_atomic_fetch_min(first_bad + sg, (u64a)(i - seg_first[sg]), HIDX_RLX_AGENT);
    }
}

__global__ __launch_bounds__(256) void k_seg_live(const uint64_t *__restrict__ seg_first, uint64_t nseg, uint64_t n,
                                                  const uint64_t *__restrict__ first_bad, uint8_t *__restrict__ live) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += stride) {
        const uint64_t sg = seg_of(seg_first, nseg, r);
        live[r] = r - seg_first[sg] < first_bad[sg] ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void k_seg_valid(const uint64_t *__restrict__ seg_first, uint64_t nseg,
                                                   uint64_t *__restrict__ valid) {
    const uint64_t sg = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (sg >= nseg) return;
    const uint64_t a = seg_first[sg], b = seg_first[sg + 1], cnt = b > a ? b - a : 0;
    if (valid[sg] > cnt) valid[sg] = cnt;
}

// 1: the record claimed an empty slot (a new key)
__device__ __forceinline__ uint32_t insert_one(u64a *hdr, u64a *slots, uint64_t table, const uint8_t *pool,
                                               uint64_t pool_bytes, uint64_t off, uint32_t ks, uint64_t hmask) {
    const uint8_t *key = pool + off + kSegHeader;
    const uint64_t h = hash_key(key, ks, hmask), tag = h >> 48, mask = table - 1;
    const u64a val = (u64a)(tag << 48 | (off + 1));
    uint64_t k0, k1;
    prefix_words(key, ks, k0, k1);
    uint64_t i = h & mask;
    for (uint64_t step = 0; step < table; ++step, i = (i + 1) & mask) {
        if ((step & 31) == 31 && __hip_atomic_load(hdr + hOverflow, HIDX_RLX_AGENT)) return 0;  // the call fails anyway
        // a slot goes from empty to one key once and then keeps it; "empty" is only a reason to try the exchange,
        // whose returned value decides
        u64a cur = __hip_atomic_load(slots + i, HIDX_RLX_AGENT);
        if (cur == 0) {
            u64a seen = 0;
            if (__hip_atomic_compare_exchange_strong(slots + i, &seen, val, __ATOMIC_RELAXED, HIDX_RLX_AGENT)) return 1;
            cur = seen;
        }
        if (cur >> 48 != tag) continue;
        const uint64_t o = (cur & kLow48) - 1;
        uint32_t oks, ovs;
        if (o != off && !same_key(pool, pool_bytes, o, key, ks, k0, k1, &oks, &ovs)) continue;
        // the slot's value only rises: one already at or above this record's makes the atomic needless
        if (cur < val) __hip_atomic_fetch_max(slots + i, val, HIDX_RLX_AGENT);
        return 0;
    }
    __hip_atomic_store(hdr + hOverflow, (u64a)1, HIDX_RLX_AGENT);
    return 0;
}

__global__ __launch_bounds__(256) void k_hidx_insert(u64a *hdr, u64a *slots, uint64_t table, const uint8_t *__restrict__ pool,
                                                     uint64_t pool_bytes, const uint64_t *__restrict__ rec_off,
                                                     const uint8_t *__restrict__ live, uint64_t n, uint64_t hmask) {
    u64a fresh = 0, bad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += stride) {
        if (live && !live[r]) continue;
        const uint64_t off = rec_off[r];
        uint32_t ks, vs;
        if (!rec_extent(pool, pool_bytes, off, &ks, &vs)) {
            ++bad;
            continue;
        }
        fresh += insert_one(hdr, slots, table, pool, pool_bytes, off, ks, hmask);
    }
    fresh = wave_sum(fresh), bad = wave_sum(bad);
    if ((threadIdx.x & 63) == 0) {
        if (fresh) __hip_atomic_fetch_add(hdr + hCount, fresh, HIDX_RLX_AGENT);
        if (bad) __hip_atomic_fetch_add(hdr + hBad, bad, HIDX_RLX_AGENT);
    }
}

struct HidxOut {
    uint8_t *status;
    uint64_t *rec, *vloc;
    uint32_t *vlen;
    uint8_t *source;
};

template <bool kVerify>
__global__ __launch_bounds__(256) void k_hidx_get(const uint64_t *__restrict__ slots, uint64_t table,
                                                  const uint8_t *__restrict__ pool, uint64_t pool_bytes, KeyBatch kb,
                                                  uint64_t hmask, HidxOut out) {
    __shared__ uint32_t tab[4][256];
    if constexpr (kVerify) {
        crc_stage_tables(tab);
        __syncthreads();
    }
    const uint64_t mask = table - 1, stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < kb.n; i += stride) {
        uint64_t kbeg = i * kb.stride, klen64 = kb.stride;
        if (kb.offsets) {
            kbeg = kb.offsets[i];
            const uint64_t kend = kb.offsets[i + 1];
            klen64 = kend > kbeg ? kend - kbeg : 0;
        }
        uint8_t st = kGetMiss;
        uint64_t at = kHidxNoRec, loc = 0;
        uint32_t vl = 0;
        if (klen64 < (1ull << 32)) {  // no record's key is longer
            const uint8_t *key = kb.data + kbeg;
            const uint32_t klen = (uint32_t)klen64;
            const uint64_t h = hash_key(key, klen, hmask), tag = h >> 48;
            uint64_t k0, k1;
            prefix_words(key, klen, k0, k1);
            uint64_t j = h & mask;
            for (uint64_t step = 0; step < table; ++step, j = (j + 1) & mask) {
                const uint64_t cur = slots[j];
                if (cur == 0) break;
                if (cur >> 48 != tag) continue;
                const uint64_t o = (cur & kLow48) - 1;
                uint32_t ks, vs;
                if (!same_key(pool, pool_bytes, o, key, klen, k0, k1, &ks, &vs)) continue;
                // segment.read: the CRC first, then the value; an empty value is ErrKeyNotFound
                bool good = true;
                if constexpr (kVerify)
                    good = ~crc_range(~0u, pool, o + 4, o + kSegHeader + ks + vs, tab) == ld_u32_le(pool + o);
                if (!good)
                    st = kGetError;
                else if (vs)
                    st = kGetFound, at = o, loc = o + kSegHeader + ks, vl = vs;
                break;
            }
        }
        out.status[i] = st;
        if (out.rec) out.rec[i] = at;
        if (out.vloc) out.vloc[i] = loc;
        if (out.vlen) out.vlen[i] = vl;
        if (out.source) out.source[i] = st == kGetFound ? 1 : 0;
    }
}

}  // namespace

uint64_t hidx_slots(uint64_t capacity) {
    uint64_t t = 1;
    while (t < 2 * capacity) t <<= 1;
    return t;
}

uint64_t hidx_table_bytes(uint64_t capacity) { return kHeadBytes + 8 * hidx_slots(capacity); }

hipError_t launch_hidx_clear(void *table, uint64_t capacity, hipStream_t s) {
    return hipMemsetAsync(table, 0, hidx_table_bytes(capacity), s);
}

hipError_t launch_seg_verify(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, uint64_t n,
                             const uint64_t *seg_first, uint64_t nseg, uint8_t *ok, uint64_t *valid, uint8_t *live,
                             hipStream_t s) {
    hipError_t e;
    if (nseg && (e = hipMemsetAsync(valid, 0xFF, 8 * nseg, s)) != hipSuccess) return e;
    if (n) {
        const uint64_t g = (n + kSegRecs - 1) / kSegRecs;
        if (g >= (1ull << 31)) return hipErrorInvalidValue;
        hipLaunchKernelGGL((k_seg_crc<kSegLds, false>), dim3((unsigned)g), dim3(kSegRecs), 0, s, pool, pool_bytes, rec_off, n,
                           seg_first, nseg, ok, (u64a *)valid);
        if (live && nseg) hipLaunchKernelGGL(k_seg_live, dim3(stream_grid(n)), dim3(256), 0, s, seg_first, nseg, n, valid, live);
    }
    if (nseg) hipLaunchKernelGGL(k_seg_valid, dim3((unsigned)((nseg + 255) / 256)), dim3(256), 0, s, seg_first, nseg, valid);
    return hipGetLastError();
}

hipError_t launch_seg_seal(uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, uint64_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint64_t g = (n + kSegRecs - 1) / kSegRecs;
    if (g >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_seg_crc<kSegLds, true>), dim3((unsigned)g), dim3(kSegRecs), 0, s, (const uint8_t *)pool, pool_bytes,
                       rec_off, n, (const uint64_t *)nullptr, (uint64_t)0, (uint8_t *)nullptr, (u64a *)nullptr);
    return hipGetLastError();
}

hipError_t launch_hidx_insert(void *table, uint64_t capacity, const uint8_t *pool, uint64_t pool_bytes,
                              const uint64_t *rec_off, const uint8_t *live, uint64_t n, uint64_t hash_mask, hipStream_t s) {
    if (n == 0) return hipSuccess;
    u64a *hdr = (u64a *)table;
    hipLaunchKernelGGL(k_hidx_insert, dim3(stream_grid(n)), dim3(256), 0, s, hdr, hdr + kHeadBytes / 8, hidx_slots(capacity), pool,
                       pool_bytes, rec_off, live, n, hash_mask);
    return hipGetLastError();
}

hipError_t launch_hidx_state(const void *table, uint64_t state_host[3], hipStream_t s) {
    hipError_t e = hipMemcpyAsync(state_host, table, 24, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(s);
        return e;
    }
    return hipStreamSynchronize(s);
}

hipError_t launch_hidx_get(const void *table, uint64_t capacity, const uint8_t *pool, uint64_t pool_bytes, const KeyBatch &kb,
                           bool verify, uint64_t hash_mask, uint8_t *status, uint64_t *rec, uint64_t *vloc, uint32_t *vlen,
                           uint8_t *source, hipStream_t s) {
    if (kb.n == 0) return hipSuccess;
    const uint64_t *slots = (const uint64_t *)table + kHeadBytes / 8;
    const HidxOut out{status, rec, vloc, vlen, source};
    if (verify)
        hipLaunchKernelGGL(k_hidx_get<true>, dim3(stream_grid(kb.n)), dim3(256), 0, s, slots, hidx_slots(capacity), pool, pool_bytes,
                           kb, hash_mask, out);
    else
        hipLaunchKernelGGL(k_hidx_get<false>, dim3(stream_grid(kb.n)), dim3(256), 0, s, slots, hidx_slots(capacity), pool, pool_bytes,
                           kb, hash_mask, out);
    return hipGetLastError();
}

}  // namespace seb
