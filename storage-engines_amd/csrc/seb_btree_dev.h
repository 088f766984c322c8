// seb_btree_dev.h — what the B-tree's kernels share among themselves (seb_btree.hip, seb_btscan.hip): how a batch
// key is compared with a stored key on the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "seb_btree.h"
#include "seb_hidx_dev.h"  // ld_u64_le, prefix_words, u64a and the agent-scope atomics' spelling
#include "seb_kernels.h"

namespace seb {

struct DevCmp {  // the sign of bytes.Compare(key, stored): the prefix words first, the tails only on equal prefixes
    const uint8_t *key;
    uint32_t klen;
    uint64_t k0, k1;
    __device__ __forceinline__ int operator()(const uint8_t *stored, uint32_t slen) const {
        uint64_t be[2];
        prefix_words(stored, slen, be[0], be[1]);
        return cmp_key(key, klen, k0, k1, be, stored, slen);
    }
};

}  // namespace seb
