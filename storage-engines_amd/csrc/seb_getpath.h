// seb_getpath.h — the host-only code of seb_getpath.cpp (no HIP dependency): the host half of the Get path's
// compaction of the keys the memtables leave undecided, and of the row-mapped join.
#pragma once
#include <cstdint>

#include "seb_memtable.h"

namespace seb {

struct CompactSizes {  // seb_compact_sizes
    uint64_t n, undecided, key_bytes, reserved;
};

// k_get_join's rule: a key is undecided unless its status is FOUND or TOMBSTONE, whatever else the byte holds
inline bool mem_undecided(uint8_t m) { return m != kMemFound && m != kMemTombstone; }

// The undecided keys of `keys` in batch order: sz always; out_keys / out_off / row all null: sizes only.  With
// outputs: key j at out_keys + j * stride, or out_off[0..m] for a batch with offsets (out_off is not written for
// a fixed-stride batch), row[j] = its batch index.  0; -1 a null required pointer; -2 keys.n >= 2^32; -3
// offsets decrease at key *bad; -4 a cap is below its size: sz is filled and nothing is written.
int get_compact(const KeysView &keys, const uint8_t *mem_status, CompactSizes *sz, uint8_t *out_keys, uint64_t key_cap,
                uint64_t *out_off, uint32_t *row, uint64_t row_cap, uint64_t *bad);

// LSM.Get's decision where the SSTable steps ran on the m compacted keys alone: sst_* are indexed by compacted
// key j and land on batch key row[j].  mem_vloc, mem_vlen, sst_col, sst_vloc, sst_vlen, source, col, vloc and
// vlen are nullable.  0; -1 a null required pointer; -2 n >= 2^32.
int get_join_rows(const uint8_t *mem_status, const uint64_t *mem_vloc, const uint32_t *mem_vlen, uint64_t n,
                  const uint32_t *row, uint64_t m, const uint8_t *sst_status, const uint16_t *sst_col,
                  const uint64_t *sst_vloc, const uint32_t *sst_vlen, uint8_t *status, uint8_t *source, uint16_t *col,
                  uint64_t *vloc, uint32_t *vlen);

}  // namespace seb
