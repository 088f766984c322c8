// seb_block.cpp — the host side of the batched data-block search: searchBlock's walk
// (lsm/sstable.go:242-290) for one block image and one key, and the read-list builder.  No HIP
// dependency, so it compiles alone (tools/sanitize/block_check.cpp); the C ABI wrappers that set
// seb_last_error are in seb_host.cpp.
//
//   numEntries := u32(block[0:4]); off := 4                              sstable.go:243-248
//   for i := 0; i < numEntries; i++ {
//       if off+9 > len(block) { return error "block truncated" }         :251-253
//       keySize, valueSize, deleted := u32, u32, block[off+8] == 1; off += 9
//       if off+keySize+valueSize > len(block) { return error }           :261-263 (Go int: 64 bits)
//       if entryKey == key { deleted ? (nil, false) : (value, true) }    :268-281
//       if entryKey > key { return not found }                           :284-286
//       off += keySize + valueSize
//   }
//   return not found
#include <cstdint>
#include <cstring>
#include <new>
#include <unordered_map>

namespace seb {

constexpr uint64_t kBlockBytes = 4096;
enum : uint32_t { kCellNone = 0, kCellMiss = 1, kCellFound = 2, kCellTombstone = 3, kCellTrunc = 4 };
static inline uint32_t cell_pack(uint32_t status, uint32_t voff, uint32_t vlen) {
    return status << 28 | voff << 13 | vlen;
}

static inline uint32_t le32(const uint8_t *p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// 0, or -1 for a bad argument (len > 4096, a null pointer with a non-zero length, null cell).
int block_search(const uint8_t *block, uint64_t len, const uint8_t *key, uint64_t key_len, uint32_t *cell) {
    if (!cell || len > kBlockBytes || (len && !block) || (key_len && !key)) return -1;
    *cell = cell_pack(kCellMiss, 0, 0);
    if (len < 4) return 0;
    const uint32_t num = le32(block);
    uint64_t off = 4;
    for (uint32_t i = 0; i < num; ++i) {
        if (off + 9 > len) {
            *cell = cell_pack(kCellTrunc, 0, 0);
            return 0;
        }
        const uint64_t ks = le32(block + off), vs = le32(block + off + 4);
        const bool deleted = block[off + 8] == 1;
        off += 9;
        if (off + ks + vs > len) {  // 64-bit sums: 0xFFFFFFF0 + 0x20 does not wrap
            *cell = cell_pack(kCellTrunc, 0, 0);
            return 0;
        }
        const uint64_t common = ks < key_len ? ks : key_len;
        int c = common ? memcmp(block + off, key, common) : 0;
        if (c == 0) c = ks < key_len ? -1 : ks > key_len ? 1 : 0;  // a proper prefix sorts first
        if (c == 0) {
            *cell = deleted ? cell_pack(kCellTombstone, 0, 0) : cell_pack(kCellFound, (uint32_t)(off + ks), (uint32_t)vs);
            return 0;
        }
        if (c > 0) return 0;  // entryKey > key: not found
        off += ks + vs;
    }
    return 0;
}

struct PairHash {
    size_t operator()(const std::pair<uint64_t, uint64_t> &p) const {
        uint64_t h = p.first * 0x9E3779B97F4A7C15ull ^ (p.second + 0x7F4A7C15ull + (p.first << 6));
        h ^= h >> 29;
        return (size_t)(h * 0xBF58476D1CE4E5B9ull);
    }
};

// 0; -1 bad argument; -2 uniq_cap too small (*num_uniq = the count needed); -3 out of memory;
// -4 more than 2^32 - 1 distinct blocks (ids are u32).
int blocks_dedup(const uint64_t *files, const uint64_t *blocks, uint64_t cells, uint32_t *bid, uint64_t *uniq_files,
                 uint64_t *uniq_blocks, uint64_t uniq_cap, uint64_t *num_uniq) {
    if (!num_uniq || (cells && (!files || !blocks || !bid)) || (uniq_cap && (!uniq_files || !uniq_blocks))) return -1;
    *num_uniq = 0;
    try {
        std::unordered_map<std::pair<uint64_t, uint64_t>, uint32_t, PairHash> ids;
        uint64_t count = 0;
        for (uint64_t c = 0; c < cells; ++c) {
            if (blocks[c] == UINT64_MAX) {  // SEB_NO_BLOCK
                bid[c] = UINT32_MAX;
                continue;
            }
            auto it = ids.find({files[c], blocks[c]});
            if (it != ids.end()) {
                bid[c] = it->second;
                continue;
            }
            if (count >= UINT32_MAX) return -4;
            ids.emplace(std::make_pair(files[c], blocks[c]), (uint32_t)count);
            if (count < uniq_cap) {
                uniq_files[count] = files[c];
                uniq_blocks[count] = blocks[c];
            }
            bid[c] = (uint32_t)count++;
        }
        *num_uniq = count;
        return count > uniq_cap ? -2 : 0;
    } catch (const std::bad_alloc &) {
        return -3;
    }
}

}  // namespace seb
