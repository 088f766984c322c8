// seb_keycmp.h — Go string order on the device, shared by the registry's kernels (seb_multiget.hip:
// key ranges; seb_locate.hip: sparse-index keys; seb_search.hip: data-block entries).  A stored key is held as its zero-padded first 16
// bytes in two big-endian words plus its bytes; a batch key's prefix is built once per key.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "seb_kernels.h"

namespace seb {

__device__ __forceinline__ uint64_t be64(const uint8_t *p, uint32_t len) {  // first min(len,8) bytes, big-endian
    uint64_t v = 0;
    for (uint32_t i = 0; i < 8; ++i) v = (v << 8) | (i < len ? p[i] : 0u);
    return v;
}

// The key's first 16 bytes as two big-endian words: one 16-B load for aligned fixed-width 16-B
// keys (the batch layout of the benchmarks), else byte loads.
__device__ __forceinline__ void key_prefix(const KeyBatch &kb, const uint8_t *key, uint32_t klen, uint64_t &k0,
                                           uint64_t &k1) {
    if (!kb.offsets && kb.stride == 16 && ((uintptr_t)kb.data & 15) == 0) {
        const uint4 v = *(const uint4 *)key;
        k0 = __builtin_bswap64((uint64_t)v.x | ((uint64_t)v.y << 32));
        k1 = __builtin_bswap64((uint64_t)v.z | ((uint64_t)v.w << 32));
    } else {
        k0 = be64(key, klen);
        k1 = klen > 8 ? be64(key + 8, klen - 8) : 0ull;
    }
}

// A little-endian u64 of 8 loaded key bytes as the big-endian word of the key's first min(len, 8)
// bytes, zero padded (the bytes past len are dropped).
__device__ __forceinline__ uint64_t be64_of_le(uint64_t le, uint32_t len) {
    const uint64_t v = __builtin_bswap64(le);
    return len >= 8 ? v : len == 0 ? 0ull : v & (~0ull << (8 * (8 - len)));
}

// Go bytewise compare of key (k0,k1 = its first 16 bytes big-endian) vs a stored range key.
__device__ __forceinline__ int cmp_key(const uint8_t *key, uint32_t klen, uint64_t k0, uint64_t k1,
                                       const uint64_t be[2], const uint8_t *bytes, uint32_t blen) {
    if (k0 != be[0]) return k0 < be[0] ? -1 : 1;
    if (k1 != be[1]) return k1 < be[1] ? -1 : 1;
    // equal zero-padded 16-byte prefixes: the shorter key is a prefix of the other unless both
    // run past 16 bytes, where the tail bytes (in HBM) decide
    const uint32_t n = klen < blen ? klen : blen;
    for (uint32_t i = 16; i < n; ++i)
        if (key[i] != bytes[i]) return key[i] < bytes[i] ? -1 : 1;
    return (int)klen - (int)blen;
}

// p[i] through a pointer that came out of a table in memory (RegSlot, LocSlot): the compiler cannot
// tell such a pointer's address space and would issue flat loads; the cast makes them global loads.
template <typename T>
__device__ __forceinline__ T gload(const T *p, uint64_t i) {
    return ((const __attribute__((address_space(1))) T *)p)[i];
}

}  // namespace seb
