// seb_block.h — the host-only code of seb_block.cpp (no HIP dependency): the block walker, the
// read-list builder, the host half of the SSTable builder and the host half of the compaction merge.
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

// The host half of the compaction merge.
constexpr uint32_t kMaxBlockEntries = 454;  // 4 + 9 * 455 > 4096
// loadBlock's walk: the number of entries of block[0, len), len <= 4096; the first min(count, cap) headers'
// offsets go to entry_off.
uint32_t block_entries(const uint8_t *block, uint64_t len, uint16_t *entry_off, uint32_t cap);
struct MergeSizes {  // seb_merge_sizes
    uint64_t entries_in, entries_out, key_bytes, val_bytes, shadowed, dropped;
};
struct MergeOut {  // the run in the builder's layout: entries_out + 1 offsets each
    uint8_t *keys;
    uint64_t *key_off;
    uint8_t *vals;
    uint64_t *val_off;
    uint8_t *deleted;
};
// mergeFiles' loop over the runs of a block pool: out == nullptr sizes only; with out, nothing past `want`
// (a plan's sizes) is written.  0; -1 a null argument or a run_begin that decreases; -2 a run that is not
// strictly increasing (*err_run, *err_entry); -3 out of memory; -4 2^32 entries or more; -5 the walk does not
// fit `want`.
int merge_walk(const uint8_t *pool, const uint16_t *blen, const uint64_t *run_begin, uint32_t num_runs, uint32_t flags,
               const MergeOut *out, const MergeSizes *want, MergeSizes *sz, uint32_t *err_run, uint64_t *err_entry);

}  // namespace seb
