// seb_locate.hip — batched data-block locator over the registry's device-resident sparse indexes.
//
// After its bloom filter says "maybe", the reference's SSTable.Get bisects the file's sparse index
// (one entry per 4 KiB data block) for the key (lsm/sstable.go:210-222):
//   blockIdx := sort.Search(len(index), func(i) { return index[i].Key > key })
//   blockIdx == 0 -> not found; else read the block at index[blockIdx-1].BlockOffset
// k_locate does that for every cell of a MultiGet's candidate rows (n keys x cap u16 slots, as
// seb_registry_multiget_list* writes them): blocks[c] = the BlockOffset of the last index entry of
// slot cand[c] whose key is <= key c / cap, or kNoBlock when there is none, when the cell is
// padding (0xFFFF), or when it names a slot without an index (free, or past the table).
//
// One lane per cell, cells in linear order: the cand reads and the blocks writes are coalesced, and
// the padded cells, the majority (a present key has ~1 live cell plus ~1% false positives per other
// file tested), store kNoBlock and leave.  A live cell runs a plain upper-bound bisection over its
// file's prefix array: ceil(log2(entries + 1)) dependent 16-B gathers; key lengths and bytes are
// read only where the zero-padded 16-byte prefixes tie.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "seb_kernels.h"
#include "seb_keycmp.h"

namespace seb {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_locate(KeyBatch kb, const uint16_t *__restrict__ cand, uint32_t cap,
                                                uint64_t cells, const LocSlot *__restrict__ tab, uint32_t ntab,
                                                uint64_t *__restrict__ blocks) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += stride) {
        const uint32_t slot = cand[c];
        uint64_t out = kNoBlock;
        if (slot < ntab) {  // padding (0xFFFF) and ids past the table fail this: ntab <= kRegMaxFiles
            const LocSlot t = tab[slot];
            if (t.n) {  // a free slot's entry is all zero
                const uint64_t i = (c >> 32) ? c / cap : (uint64_t)((uint32_t)c / cap);
                const uint8_t *key;
                uint32_t klen;
                if (kb.offsets) {
                    key = kb.data + kb.offsets[i];
                    klen = (uint32_t)(kb.offsets[i + 1] - kb.offsets[i]);
                } else {
                    key = kb.data + i * (uint64_t)kb.stride;
                    klen = kb.stride;
                }
                uint64_t k0, k1;
                key_prefix(kb, key, klen, k0, k1);
                // a = the number of index keys <= key (sort.Search's blockIdx): entries below a
                // compare <= key, entries from b on compare > key
                uint32_t a = 0, b = t.n;
                while (a < b) {
                    const uint32_t mid = (a + b) >> 1;
                    const u32x4 p = gload((const u32x4 *)t.pre, mid);
                    const uint64_t be[2] = {(uint64_t)p.x | ((uint64_t)p.y << 32), (uint64_t)p.z | ((uint64_t)p.w << 32)};
                    int cmp;
                    if (k0 != be[0]) {
                        cmp = k0 < be[0] ? -1 : 1;
                    } else if (k1 != be[1]) {
                        cmp = k1 < be[1] ? -1 : 1;
                    } else {  // equal 16-byte prefixes: lengths, and past 16 bytes the tails, decide
                        const uint64_t o0 = gload(t.koff, mid), o1 = gload(t.koff, (uint64_t)mid + 1);
                        cmp = cmp_key(key, klen, k0, k1, be, t.bytes + o0, (uint32_t)(o1 - o0));
                    }
                    if (cmp >= 0)
                        a = mid + 1;
                    else
                        b = mid;
                }
                if (a) out = gload(t.boff, (uint64_t)a - 1);
            }
        }
        blocks[c] = out;
    }
}

hipError_t launch_locate(const KeyBatch &kb, const uint16_t *cand, uint32_t cap, const LocSlot *tab, uint32_t ntab,
                         uint64_t *blocks, hipStream_t s) {
    const uint64_t cells = kb.n * (uint64_t)cap;
    if (cells == 0) return hipSuccess;
    uint64_t g = (cells + 255) / 256;
    if (g > options().grid_cap) g = options().grid_cap;
    hipLaunchKernelGGL(k_locate, dim3((unsigned)g), dim3(256), 0, s, kb, cand, cap, cells, tab, ntab, blocks);
    return hipGetLastError();
}

}  // namespace seb
