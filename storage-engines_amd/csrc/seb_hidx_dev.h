// seb_hidx_dev.h — what the hash index's kernels share (seb_hashindex.hip: the read side; seb_hashwrite.hip: the
// write side): the table's layout, a record's extent check, the key hash and the key compare.
//
// The table: a 64-byte header [overflow][occupied slots][bad records] and the smallest power of two >= 2 * capacity
// slots of one u64 each: 0 = empty, else a hash tag in the high 16 bits and record offset + 1 in the low 48.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "seb_device.h"
#include "seb_hashindex.h"
#include "seb_keycmp.h"

namespace seb {

typedef unsigned long long u64a;  // what the 64-bit atomics take

constexpr uint64_t kHidxHeadBytes = 64;
enum : uint32_t { hOverflow = 0, hCount = 1, hBad = 2 };  // the header's u64 words
constexpr uint64_t kLow48 = (1ull << 48) - 1;

#define HIDX_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// The 8 bytes at p, little-endian, at any alignment: the two or three aligned dwords that cover them and a funnel
// shift, instead of 8 byte loads.  Each of those dwords holds at least one of the 8 bytes, so none crosses into a
// page the bytes do not touch (seb_device.h's fnv_range reads the same way).
__device__ __forceinline__ uint64_t ld_u64_le(const uint8_t *p) {
    const uint32_t sh = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t *w = (const uint32_t *)((uintptr_t)p & ~(uintptr_t)3);
    const uint32_t a0 = w[0], a1 = w[1];
    if (sh == 0) return (uint64_t)a0 | (uint64_t)a1 << 32;
    const uint32_t a2 = w[2];
    return (uint64_t)__builtin_amdgcn_alignbyte(a1, a0, sh) | (uint64_t)__builtin_amdgcn_alignbyte(a2, a1, sh) << 32;
}

// seb_keycmp.h's two big-endian prefix words of a key of klen bytes
__device__ __forceinline__ void prefix_words(const uint8_t *key, uint32_t klen, uint64_t &k0, uint64_t &k1) {
    if (klen >= 16) {
        k0 = __builtin_bswap64(ld_u64_le(key)), k1 = __builtin_bswap64(ld_u64_le(key + 8));
    } else {
        k0 = be64(key, klen), k1 = klen > 8 ? be64(key + 8, klen - 8) : 0ull;
    }
}

// The record at pool offset `off` lies whole inside the pool and keySize + valueSize < 2^32 (seg_record of the
// host half); no byte of the record is read before its header is known to fit.
__device__ __forceinline__ bool rec_extent(const uint8_t *pool, uint64_t pool_bytes, uint64_t off, uint32_t *ks, uint32_t *vs) {
    if (off > pool_bytes || pool_bytes - off < kSegHeader) return false;
    const uint64_t sizes = ld_u64_le(pool + off + 12);
    *ks = (uint32_t)sizes, *vs = (uint32_t)(sizes >> 32);
    const uint64_t payload = (uint64_t)*ks + *vs;
    return payload < (1ull << 32) && payload <= pool_bytes - off - kSegHeader;
}

// FNV-1a over the key bytes and a finishing mix (the tag is the hash's high 16 bits); hmask: the test-only option.
__device__ __forceinline__ uint64_t hash_key(const uint8_t *p, uint32_t len, uint64_t hmask) {
    uint64_t h = kFnvOffset;
    uint32_t i = 0;
    for (; i < len && (((uintptr_t)(p + i)) & 3u); ++i) h = (h ^ p[i]) * kFnvPrime;
    for (; i + 4 <= len; i += 4) {
        const uint32_t w = *(const uint32_t *)(p + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) h = (h ^ ((w >> (8 * j)) & 0xffu)) * kFnvPrime;
    }
    for (; i < len; ++i) h = (h ^ p[i]) * kFnvPrime;
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 32;
    return hmask ? h & hmask : h;
}

// key (klen bytes, k0 / k1 its first 16 as seb_keycmp.h holds them) equals the key of the record at `o`, which is
// checked against the pool first; *oks / *ovs are then that record's sizes
__device__ __forceinline__ bool same_key(const uint8_t *pool, uint64_t pool_bytes, uint64_t o, const uint8_t *key,
                                         uint32_t klen, uint64_t k0, uint64_t k1, uint32_t *oks, uint32_t *ovs) {
    if (!rec_extent(pool, pool_bytes, o, oks, ovs) || *oks != klen) return false;
    const uint8_t *stored = pool + o + kSegHeader;
    uint64_t be[2];
    prefix_words(stored, klen, be[0], be[1]);
    return cmp_key(key, klen, k0, k1, be, stored, klen) == 0;
}

}  // namespace seb
