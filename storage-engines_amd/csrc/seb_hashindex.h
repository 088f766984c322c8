// seb_hashindex.h — the host-only code of seb_hashindex.cpp (no HIP dependency): the host half of the hash
// index's read side: the segments' framing walk, recover()'s CRC pass and cuts, and Get.
#pragma once
#include <cstdint>

#include "seb_memtable.h"

namespace seb {

constexpr uint32_t kSegHeader = 20;               // [crc u32][timestamp u64][keySize u32][valueSize u32]
constexpr uint64_t kHidxPoolLimit = 1ull << 47;   // a record offset + 1 fits the slot's low 48 bits
constexpr uint64_t kHidxNoRec = ~0ull;

// One segment image's records by the sequential header walk; outputs are pool offsets (base + file offset).
// The walk ends at the image's end, at a tail that ends inside a header or a payload (*short_tail = 1; that
// tail is no record), or behind a header with keySize + valueSize >= 2^32, which is listed as the segment's
// last record and which seg_verify fails.  0; -1 a null argument; -2 more than cap records (*n = cap then).
int seg_scan(const uint8_t *data, uint64_t bytes, uint64_t base, uint64_t *rec_off, uint64_t cap, uint64_t *n,
             int *short_tail);

// record r is whole inside the pool and keySize + valueSize < 2^32; then *ks, *vs
bool seg_record(const uint8_t *pool, uint64_t pool_bytes, uint64_t off, uint32_t *ks, uint32_t *vs);

// ok[r] (nullable) = record r passes seg_record and its CRC; valid[s] = the records of segment s (records
// [seg_first[s], seg_first[s+1])) before its first bad one; size_after[s] = that record's offset - seg_base[s],
// or seg_bytes[s]; live[r] (nullable) = r < seg_first[s] + valid[s].  0; -1 a null argument; -2 pool_bytes >=
// 2^47; -3 seg_first does not start at 0, decreases or does not end at num_records.
int seg_verify(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, uint64_t num_records,
               const uint64_t *seg_first, const uint64_t *seg_base, const uint64_t *seg_bytes, uint64_t num_segments,
               uint8_t *ok, uint64_t *valid, uint64_t *size_after, uint8_t *live);

// Get for a key batch over the live records (live nullable: all are); the later record of a key wins.
// status / rec / vloc / vlen: keys.n elements each, rec, vloc and vlen nullable; *distinct (nullable) = the
// index's key count, tombstones included.  A live record that fails seg_record takes no part.  0; -1 a null
// argument; -2 pool_bytes >= 2^47; -3 out of memory.
int hidx_lookup(const uint8_t *pool, uint64_t pool_bytes, const uint64_t *rec_off, const uint8_t *live,
                uint64_t num_records, const KeysView &keys, int verify, uint8_t *status, uint64_t *rec, uint64_t *vloc,
                uint32_t *vlen, uint64_t *distinct);

}  // namespace seb
