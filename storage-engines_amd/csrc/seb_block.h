// seb_block.h — the host-only code of seb_block.cpp (no HIP dependency): the block walker, the
// read-list builder and the host half of the SSTable builder.
#pragma once
#include <cstdint>

namespace seb {

// 0, or -1 for a bad argument (len > 4096, a null pointer with a non-zero length, null cell).
int block_search(const uint8_t *block, uint64_t len, const uint8_t *key, uint64_t key_len, uint32_t *cell);
// 0; -1 bad argument; -2 uniq_cap too small (*num_uniq = the count needed); -3 out of memory;
// -4 more than 2^32 - 1 distinct blocks (ids are u32).
int blocks_dedup(const uint64_t *files, const uint64_t *blocks, uint64_t cells, uint32_t *bid, uint64_t *uniq_files,
                 uint64_t *uniq_blocks, uint64_t uniq_cap, uint64_t *num_uniq);

struct SstKeys {  // seb_keys, host pointers
    const uint8_t *data;
    const uint64_t *offsets;
    uint64_t n;
    uint32_t stride;
    uint64_t off(uint64_t i) const { return offsets ? offsets[i] : i * (uint64_t)stride; }
};
struct SstSizes {  // seb_sst_sizes
    uint64_t num_blocks, data_bytes, index_bytes, meta_bytes, oversize_entries;
};
struct SstOut {  // the three sections' buffers and capacities
    uint8_t *data, *index, *meta;
    uint64_t data_cap, index_cap, meta_cap;
};
// The builder's walk over one sorted run: out == nullptr sizes only.  0; -1 a null argument; -2 a key or a
// value of 2^32 bytes or more, or decreasing offsets; -3 a capacity below its section (*sz is still filled).
int sst_walk(const SstKeys &k, const uint8_t *vals, const uint64_t *voff, const uint8_t *deleted, const SstOut *out,
             SstSizes *sz);
// [indexOffset u64][bloomOffset u64][metadataOffset u64][0x5354424C u32]
void sst_footer(uint64_t index_offset, uint64_t bloom_offset, uint64_t metadata_offset, uint8_t *out28);

}  // namespace seb
